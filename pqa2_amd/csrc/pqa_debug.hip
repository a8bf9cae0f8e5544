// The pqa_debug_* entries of the C ABI: single kernels and host tables exposed to the tests, on the default stream with
// scratch memory of their own (no context; pqa_debug_vif_strip_shape alone reads one's switches).  Declarations: include/pqa_vmaf.h.
#include "adm_need.h"
#include "pqa_ctx.h"

using namespace pqa;

namespace {

int need_device() {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(nullptr, PQA_EDEVICE, "no HIP device visible (this library has no CPU fallback)");
  return PQA_OK;
}

// the sample size of a plane at bit_depth into *es; its rows are whole samples and at least w of them apart
int plane_pitch_rule(const char* who, uint32_t bit_depth, uint32_t w, int64_t row_pitch_bytes, int* es) {
  *es = bit_depth > 8 ? 2 : 1;
  if (row_pitch_bytes < (int64_t)w * *es || row_pitch_bytes % *es)
    return fail(nullptr, PQA_EINVAL, "%s: bad row pitch %lld", who, (long long)row_pitch_bytes);
  return PQA_OK;
}

// The device allocations of one call, freed on every return path.  `err` is the first failure: once it is set, nothing
// more is allocated or copied, so a call makes its buffers in a row and looks at err once.
struct Scratch {
  void* held[12];
  int n = 0;
  hipError_t err = hipSuccess;
  ~Scratch() { for (int i = 0; i < n; ++i) hipFree(held[i]); }
  template <typename T>
  T* get(size_t count) {
    void* p = nullptr;
    if (err == hipSuccess) err = n < 12 ? hipMalloc(&p, count * sizeof(T)) : hipErrorOutOfMemory;
    if (p) held[n++] = p;
    return (T*)p;
  }
  // a packed copy of a host plane (null stays null)
  void* plane(const void* host, int64_t row_pitch_bytes, size_t row_bytes, uint32_t h) {
    if (!host) return nullptr;
    void* p = get<uint8_t>(row_bytes * h);
    if (err == hipSuccess) err = hipMemcpy2D(p, row_bytes, host, (size_t)row_pitch_bytes, row_bytes, h, hipMemcpyHostToDevice);
    return p;
  }
};

}  // namespace

extern "C" {

int pqa_debug_vif_march_table(uint16_t* out, int32_t capacity_halfwords) { return vif_march_table(out, capacity_halfwords); }
int pqa_debug_vif_march_shape(uint32_t width, uint32_t height, int32_t* out6) {
  if (!out6 || width == 0 || height == 0 || width > 65536 || height > 65536) return PQA_EINVAL;
  int shape[6];
  vif_march_shape((int)width, (int)height, shape);
  for (int i = 0; i < 6; ++i) out6[i] = shape[i];
  return PQA_OK;
}

int pqa_debug_vif_strip_shape(pqa_ctx* ctx, uint32_t scale, uint32_t n_frames, int32_t* out4) {
  if (!ctx) return PQA_EINVAL;
  if (!out4 || scale < 1 || scale > 3 || n_frames == 0 || n_frames > 65536)
    return fail(ctx, PQA_EINVAL, "pqa_debug_vif_strip_shape: bad argument");
  const Level& L = ctx->vif_lv[scale];
  int shape[4];
  // what run_vif passes to launch_vif_stat at this scale
  const int strip_seg = ctx->vif_fixed ? -1 : (ctx->vif_strip_mask >> scale & 1) ? ctx->vif_strip_seg : -1;
  vif_strip_shape((int)scale, L.w, L.h, (int)n_frames, strip_seg, shape);
  for (int i = 0; i < 4; ++i) out4[i] = shape[i];
  return PQA_OK;
}

int pqa_debug_adm_need(uint32_t width, uint32_t height, int32_t* out20) {
  if (!out20 || width == 0 || height == 0 || width > 65536 || height > 65536) return PQA_EINVAL;
  const AdmNeed n = adm_need((int)width, (int)height);
  for (int s = 0; s < 4; ++s) {
    out20[4 * s + 0] = n.rows[s].lo; out20[4 * s + 1] = n.rows[s].hi;
    out20[4 * s + 2] = n.cols[s].lo; out20[4 * s + 3] = n.cols[s].hi;
  }
  out20[16] = n.in_rows.lo; out20[17] = n.in_rows.hi; out20[18] = n.in_cols.lo; out20[19] = n.in_cols.hi;
  return PQA_OK;
}

int pqa_debug_partial_counts(uint32_t width, uint32_t height, uint32_t bit_depth, int32_t* out, int32_t cap) {
  static_assert(PQA_PARTIAL_COUNT_INTS == 14, "pqa_debug_partial_counts layout");
  if (!out || cap < PQA_PARTIAL_COUNT_INTS || width < 16 || height < 16 || width > 16384 || height > 16384 ||
      (bit_depth != 8 && bit_depth != 10 && bit_depth != 12))
    return fail(nullptr, PQA_EINVAL, "pqa_debug_partial_counts: bad argument");
  const int w = (int)width, h = (int)height;
  const Elem elem = bit_depth > 8 ? ELEM_U16 : ELEM_U8;
  // "written" is what the launcher itself reports for a launch of no frames (it fills *n_partials and launches nothing);
  // 0 where it does not take the planes
  hipError_t err = hipSuccess;
  int np = 0;
  out[0] = vif_march_partials_max(w, h);
  out[1] = vif_march_partials(w, h);   // launch_vif_s0_march's own n_part (it needs a device for its tap table)
  int aw = w, ah = h;                  // the levels of alloc_adm (ceil halving)
  for (int s = 0; s < 4; ++s) {
    if (s > 0) { aw = (aw + 1) / 2; ah = (ah + 1) / 2; }
    out[2 + 2 * s] = adm_march_partials((aw + 1) / 2, (ah + 1) / 2);
    const PlaneRun in{nullptr, aw, 0};
    np = 0;
    out[3 + 2 * s] = launch_adm_march(nullptr, s, s ? ELEM_F32 : elem, in, in, 0, aw, ah, 1.0f, 100.0f, MutPlaneRun{nullptr, 0, 0},
                                      MutPlaneRun{nullptr, 0, 0}, nullptr, &np, true, &err) ? np : 0;
  }
  static float band[4];                // launch_adm_pyramid wants an approximation band; a launch of no frames writes none
  const PlaneRun luma{nullptr, w, 0};
  const MutPlaneRun ll{band, (int64_t)((w / 4 + 15) / 16 * 16), 0};
  out[10] = adm_pyramid_takes(elem, w, h) ? adm_pyramid_partials(w, h) : 0;
  np = 0;
  out[11] = launch_adm_pyramid(nullptr, elem, luma, luma, 0, w, h, 1.0f, 100.0f, ll, ll, nullptr, nullptr, &np, true, &err) ? np : 0;
  out[12] = motion_march_partials(w, h);
  np = 0;
  out[13] = launch_motion_march(nullptr, elem, luma, nullptr, 0, 0, w, h, nullptr, &np, &err) ? np : 0;
  return PQA_OK;
}

int pqa_debug_ciede2000(const double* lab_pairs, int32_t n, double* de_out) {
  if (n < 0 || (n > 0 && (!lab_pairs || !de_out))) return fail(nullptr, PQA_EINVAL, "bad argument");
  const int rc = need_device();
  if (rc != PQA_OK) return rc;
  if (n == 0) return PQA_OK;
  std::vector<float> in((size_t)n * 6), out((size_t)n);
  for (size_t i = 0; i < in.size(); ++i) in[i] = (float)lab_pairs[i];
  Scratch s;
  float* d_in = s.get<float>(in.size());
  float* d_out = s.get<float>(out.size());
  hipError_t e = s.err;
  if (e == hipSuccess) e = hipMemcpy(d_in, in.data(), in.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = launch_ciede_debug(nullptr, d_in, n, d_out);
  if (e == hipSuccess) e = hipMemcpy(out.data(), d_out, out.size() * sizeof(float), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail(nullptr, PQA_EDEVICE, "pqa_debug_ciede2000: %s", hipGetErrorString(e));
  for (int32_t i = 0; i < n; ++i) de_out[i] = (double)out[i];
  return PQA_OK;
}

int pqa_debug_itp(const pqa_itp_spec* spec, const float* yuv_triples, int32_t n, float* itp_out) {
  if (!spec || n < 0 || (n > 0 && (!yuv_triples || !itp_out))) return fail(nullptr, PQA_EINVAL, "bad argument");
  if (const char* what = itp_spec_error(*spec)) return fail(nullptr, PQA_EINVAL, "pqa_debug_itp: %s", what);
  const int rc = need_device();
  if (rc != PQA_OK) return rc;
  if (n == 0) return PQA_OK;
  ItpCoef k;
  itp_prepare(*spec, &k);
  Scratch s;
  float* d_in = s.get<float>((size_t)n * 3);
  float* d_out = s.get<float>((size_t)n * 3);
  hipError_t e = s.err;
  if (e == hipSuccess) e = hipMemcpy(d_in, yuv_triples, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = launch_delta_itp_debug(nullptr, k, d_in, n, d_out);
  if (e == hipSuccess) e = hipMemcpy(itp_out, d_out, (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail(nullptr, PQA_EDEVICE, "pqa_debug_itp: %s", hipGetErrorString(e));
  return PQA_OK;
}

int pqa_debug_cambi_params(uint32_t w, uint32_t h, uint32_t bit_depth, int32_t* out, int32_t cap) {
  if (!out || cap < PQA_CAMBI_PARAM_INTS) return fail(nullptr, PQA_EINVAL, "pqa_debug_cambi_params: null or short output");
  if (w < 16 || h < 16 || w > 16384 || h > 16384 || (bit_depth != 8 && bit_depth != 10))
    return fail(nullptr, PQA_EINVAL, "pqa_debug_cambi_params: unsupported %ux%u at %u bit", w, h, bit_depth);
  static_assert(kCambiParamInts == PQA_CAMBI_PARAM_INTS, "pqa_debug_cambi_params layout");
  const CambiParams p = cambi_params((int)w, (int)h);
  int i = 0;
  out[i++] = p.ws; out[i++] = p.r; out[i++] = p.piw; out[i++] = p.mask_t;
  for (int d = 0; d < kCambiDiffs; ++d) out[i++] = p.tvi[d];
  for (int d = 0; d < kCambiDiffs; ++d) out[i++] = p.weights[d];
  for (int s = 0; s < kCambiScales; ++s) { out[i++] = p.sw[s]; out[i++] = p.sh[s]; }
  return PQA_OK;
}

int pqa_debug_cambi_cmap(const void* luma, int64_t row_pitch_bytes, uint32_t w, uint32_t h, uint32_t bit_depth, float* cmap,
                         int64_t cap, double* score) {
  if (!luma || !cmap || w < 16 || h < 16 || w > 16384 || h > 16384 || (bit_depth != 8 && bit_depth != 10))
    return fail(nullptr, PQA_EINVAL, "pqa_debug_cambi_cmap: bad argument");
  int es = 1;
  int rc = plane_pitch_rule("pqa_debug_cambi_cmap", bit_depth, w, row_pitch_bytes, &es);
  if (rc != PQA_OK) return rc;
  const CambiParams p = cambi_params((int)w, (int)h);
  const int64_t total = p.off[kCambiScales];
  if (cap < total) return fail(nullptr, PQA_EINVAL, "pqa_debug_cambi_cmap: cmap holds %lld floats, needs %lld", (long long)cap,
                               (long long)total);
  if ((rc = need_device()) != PQA_OK) return rc;
  Scratch s;
  s.err = cambi_prepare(p, (int)bit_depth);
  void* src = s.plane(luma, row_pitch_bytes, (size_t)w * es, h);
  double* ext = s.get<double>(PQA_EXT_DOUBLES);
  CambiWork wk{};
  wk.plane = s.get<uint16_t>((size_t)total);
  wk.mask = s.get<uint8_t>((size_t)total);
  wk.cmap = s.get<float>((size_t)total);
  wk.hist = s.get<uint32_t>((size_t)kCambiScales * 2048);
  wk.sel = s.get<int32_t>((size_t)kCambiScales * 4);
  wk.partials = s.get<double>((size_t)p.chunk[kCambiScales]);
  hipError_t e = s.err;
  if (e == hipSuccess) {
    const PlaneRun run{src, (int64_t)w, (int64_t)w * h};
    e = launch_cambi(nullptr, es == 1 ? ELEM_U8 : ELEM_U16, run, 1, (int)w, (int)h, (int)bit_depth, p, wk, ext, PQA_EXT_DOUBLES,
                     PQA_EXT_CAMBI, 0, 1, 1);
  }
  if (e == hipSuccess) e = hipMemcpy(cmap, wk.cmap, (size_t)total * sizeof(float), hipMemcpyDeviceToHost);
  double ext_row[PQA_EXT_DOUBLES];
  if (e == hipSuccess) e = hipMemcpy(ext_row, ext, sizeof ext_row, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail(nullptr, PQA_EDEVICE, "pqa_debug_cambi_cmap: %s", hipGetErrorString(e));
  if (score) *score = ext_row[PQA_EXT_CAMBI];
  return PQA_OK;
}

int pqa_debug_psnr_hvs_dct8x8(const int32_t* in, int32_t* out, int32_t n) {
  if (!in || !out || n < 0) return fail(nullptr, PQA_EINVAL, "pqa_debug_psnr_hvs_dct8x8: bad argument");
  psnr_hvs_fdct8x8_host(in, out, n);
  return PQA_OK;
}

int pqa_debug_psnr_hvs_tables(float* out, int32_t cap) {
  static_assert(kPhvTableFloats == PQA_PSNR_HVS_TABLE_FLOATS, "pqa_debug_psnr_hvs_tables layout");
  if (!out || cap < PQA_PSNR_HVS_TABLE_FLOATS)
    return fail(nullptr, PQA_EINVAL, "pqa_debug_psnr_hvs_tables: null or short output");
  psnr_hvs_tables(out);
  return PQA_OK;
}

int pqa_debug_psnr_hvs_plane(const void* ref, const void* dis, int64_t row_pitch_bytes, uint32_t w, uint32_t h,
                             uint32_t bit_depth, uint32_t plane_kind, float* block_err, double* mse) {
  if (!ref || !dis || !block_err || w < 8 || h < 8 || w > 16384 || h > 16384 || plane_kind > 2 ||
      (bit_depth != 8 && bit_depth != 10 && bit_depth != 12))
    return fail(nullptr, PQA_EINVAL, "pqa_debug_psnr_hvs_plane: bad argument");
  int es = 1;
  int rc = plane_pitch_rule("pqa_debug_psnr_hvs_plane", bit_depth, w, row_pitch_bytes, &es);
  if (rc == PQA_OK) rc = need_device();
  if (rc != PQA_OK) return rc;
  // the plane pair stands in for all three planes; plane_kind picks whose tables and block sums are read back
  const int pw[3] = {(int)w, (int)w, (int)w}, ph[3] = {(int)h, (int)h, (int)h};
  PsnrHvsGeometry geo{};
  psnr_hvs_geometry(pw, ph, &geo);
  const int nb = geo.nbx[0] * geo.nby[0];
  Scratch s;
  s.err = psnr_hvs_prepare();
  void* src = s.plane(ref, row_pitch_bytes, (size_t)w * es, h);
  void* dst = s.plane(dis, row_pitch_bytes, (size_t)w * es, h);
  double* part = s.get<double>((size_t)geo.tile0[3]);
  double* ext2 = s.get<double>(PQA_EXT2_DOUBLES);
  float* err = s.get<float>((size_t)nb);
  hipError_t e = s.err;
  if (e == hipSuccess) {
    PlaneRun r3[3], d3[3];
    for (int p = 0; p < 3; ++p) {
      r3[p] = PlaneRun{src, (int64_t)w, (int64_t)w * h};
      d3[p] = PlaneRun{dst, (int64_t)w, (int64_t)w * h};
    }
    e = launch_psnr_hvs(nullptr, es == 1 ? ELEM_U8 : ELEM_U16, r3, d3, 1, geo, part, err, (int)plane_kind);
  }
  if (e == hipSuccess) {
    PsnrHvsFinalizeArgs pa{};
    pa.n_frames = 1;
    pa.ext2 = ext2;
    pa.ext_stride = PQA_EXT2_DOUBLES;
    pa.slot_base = 0; pa.slot_step = 1; pa.capacity = 1;
    pa.partials = part;
    for (int p = 0; p < 4; ++p) pa.tile0[p] = geo.tile0[p];
    for (int p = 0; p < 3; ++p) pa.blocks[p] = nb;
    pa.peak = (double)((1 << bit_depth) - 1);
    e = launch_psnr_hvs_finalize(nullptr, pa);
  }
  if (e == hipSuccess) e = hipMemcpy(block_err, err, (size_t)nb * sizeof(float), hipMemcpyDeviceToHost);
  double row[PQA_EXT2_DOUBLES];
  if (e == hipSuccess) e = hipMemcpy(row, ext2, sizeof row, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail(nullptr, PQA_EDEVICE, "pqa_debug_psnr_hvs_plane: %s", hipGetErrorString(e));
  if (mse) *mse = row[PQA_EXT2_PSNR_HVS_MSE + plane_kind];
  return PQA_OK;
}

int pqa_debug_xpsnr_blocks(const void* ref, const void* ref_m1, const void* ref_m2, const void* dis, int64_t row_pitch_bytes,
                           uint32_t w, uint32_t h, uint32_t bit_depth, int32_t hfr, uint64_t* out, double* wsse) {
  if (!ref || !dis || !out || w < 16 || h < 16 || w > 16384 || h > 16384 ||
      (bit_depth != 8 && bit_depth != 10 && bit_depth != 12))
    return fail(nullptr, PQA_EINVAL, "pqa_debug_xpsnr_blocks: bad argument");
  int es = 1;
  int rc = plane_pitch_rule("pqa_debug_xpsnr_blocks", bit_depth, w, row_pitch_bytes, &es);
  if (rc != PQA_OK) return rc;
  XpsnrGeometry geo{};
  xpsnr_geometry((int)w, (int)h, (int)w, (int)h, 1, (int)bit_depth, &geo);
  if (geo.bv == 2 && ((w | h) & 1)) return fail(nullptr, PQA_EINVAL, "pqa_debug_xpsnr_blocks: odd size above 2048x1152");
  if ((rc = need_device()) != PQA_OK) return rc;
  Scratch s;
  const void* host[4] = {ref, ref_m1, ref_m2, dis};
  void* dev[4];
  for (int i = 0; i < 4; ++i) dev[i] = s.plane(host[i], row_pitch_bytes, (size_t)w * es, h);
  auto* blk = s.get<unsigned long long>((size_t)geo.n_blk * kXpBlockVals);
  double* wb = s.get<double>((size_t)geo.n_blk);
  double* ext3 = s.get<double>(PQA_EXT3_DOUBLES);
  hipError_t e = s.err;
  if (e == hipSuccess) {
    PlaneRun r3[3] = {{dev[0], (int64_t)w, (int64_t)w * h}}, d3[3] = {{dev[3], (int64_t)w, (int64_t)w * h}};
    e = launch_xpsnr_blocks(nullptr, es == 1 ? ELEM_U8 : ELEM_U16, r3, d3, 1, dev[1], dev[1] ? (int64_t)w : 0, dev[2],
                            dev[2] ? (int64_t)w : 0, hfr != 0, geo, blk);
  }
  if (e == hipSuccess) {
    XpFinalizeArgs xa{};
    xa.n_frames = 1;
    xa.blk = blk;
    xa.wbuf = wb;
    xa.ext3 = ext3;
    xa.ext_stride = PQA_EXT3_DOUBLES;
    xa.slot_base = 0;
    xa.capacity = 1;
    xa.g = geo;
    e = launch_xpsnr_finalize(nullptr, xa);
  }
  std::vector<unsigned long long> hb;
  double row[PQA_EXT3_DOUBLES];
  if (e == hipSuccess) {
    hb.resize((size_t)geo.n_blk * kXpBlockVals);
    e = hipMemcpy(hb.data(), blk, hb.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost);
  }
  if (e == hipSuccess) e = hipMemcpy(row, ext3, sizeof row, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail(nullptr, PQA_EDEVICE, "pqa_debug_xpsnr_blocks: %s", hipGetErrorString(e));
  for (int k = 0; k < geo.n_blk; ++k)
    for (int i = 0; i < 3; ++i) out[k * 3 + i] = hb[(size_t)k * kXpBlockVals + i];
  if (wsse) *wsse = row[PQA_EXT3_WSSE];
  return PQA_OK;
}

int pqa_debug_siti_plane(const void* cur, const void* prev, int64_t row_pitch_bytes, uint32_t w, uint32_t h,
                         uint32_t bit_depth, int32_t full_range, float* gmap, double* si_ti) {
  if (!cur || !si_ti || w < 3 || h < 3 || w > 16384 || h > 16384 || (bit_depth != 8 && bit_depth != 10))
    return fail(nullptr, PQA_EINVAL, "pqa_debug_siti_plane: bad argument");
  int es = 1;
  int rc = plane_pitch_rule("pqa_debug_siti_plane", bit_depth, w, row_pitch_bytes, &es);
  if (rc == PQA_OK) rc = need_device();
  if (rc != PQA_OK) return rc;
  const size_t map_floats = (size_t)(w - 2) * (h - 2);
  Scratch s;
  void* dev[2] = {s.plane(cur, row_pitch_bytes, (size_t)w * es, h), s.plane(prev, row_pitch_bytes, (size_t)w * es, h)};
  double* part = s.get<double>((size_t)siti_partials((int)w, (int)h) * 2 * 4);
  double* ext4 = s.get<double>(PQA_EXT4_DOUBLES);
  float* dmap = gmap ? s.get<float>(map_floats) : nullptr;
  hipError_t e = s.err;
  if (e == hipSuccess) {
    const PlaneRun clip[2] = {{dev[0], (int64_t)w, (int64_t)w * h}, {dev[0], (int64_t)w, (int64_t)w * h}};
    const void* p0[2] = {dev[1], nullptr};
    const int64_t pp[2] = {dev[1] ? (int64_t)w : 0, 0};
    const bool full[2] = {full_range != 0, false};
    e = launch_siti(nullptr, es == 1 ? ELEM_U8 : ELEM_U16, clip, p0, pp, full, 1, 1, (int)w, (int)h, part, ext4,
                    PQA_EXT4_DOUBLES, 0, 1, dmap);
  }
  double row[PQA_EXT4_DOUBLES];
  if (e == hipSuccess) e = hipMemcpy(row, ext4, sizeof row, hipMemcpyDeviceToHost);
  if (e == hipSuccess && gmap) e = hipMemcpy(gmap, dmap, map_floats * sizeof(float), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail(nullptr, PQA_EDEVICE, "pqa_debug_siti_plane: %s", hipGetErrorString(e));
  si_ti[0] = row[PQA_EXT4_SI];
  si_ti[1] = row[PQA_EXT4_TI];
  return PQA_OK;
}

int pqa_debug_resample_table(uint32_t filter, int32_t n_src, int32_t n_dst, int64_t x0_q16, int64_t ext_q16, int32_t* first,
                             int16_t* coeff, int32_t cap_taps, int32_t* taps) {
  if (!first || !coeff || !taps || filter > PQA_RESAMPLE_LANCZOS3 || n_src < 1 || n_src > 8192 || n_dst < 1 || n_dst > 8192 ||
      ext_q16 <= 0 || cap_taps < 1)
    return fail(nullptr, PQA_EINVAL, "pqa_debug_resample_table: bad argument");
  ResampleTable t;
  if (resample_table((int)filter, n_src, n_dst, x0_q16, ext_q16, &t) != 0)
    return fail(nullptr, PQA_EINVAL, "pqa_debug_resample_table: a destination sample needs more than %d taps", kRsMaxTaps);
  *taps = t.taps;
  if (cap_taps < t.taps) return fail(nullptr, PQA_EINVAL, "pqa_debug_resample_table: coeff holds %d taps a row, needs %d", cap_taps, t.taps);
  for (int i = 0; i < n_dst; ++i) {
    first[i] = t.first[i];
    for (int k = 0; k < cap_taps; ++k) coeff[(size_t)i * cap_taps + k] = k < t.taps ? t.coeff[(size_t)i * t.taps + k] : 0;
  }
  return PQA_OK;
}

int pqa_debug_colour(uint32_t bit_depth, uint32_t hshift, uint32_t vshift, uint32_t w, uint32_t h, const void* const ref[3],
                     const void* const dis[3], uint32_t lo, uint32_t hi, uint64_t* sums28, const int32_t* m, void* const applied[3]) {
  if (!ref || !dis || w < 1 || h < 1 || w > 16384 || h > 16384 || (bit_depth != 8 && bit_depth != 10 && bit_depth != 12) ||
      !colour_shift_ok((int)hshift, (int)vshift) || lo > hi || hi > (1u << bit_depth) - 1u || (m && (!applied || !colour_matrix_ok(m))))
    return fail(nullptr, PQA_EINVAL, "pqa_debug_colour: bad argument");
  for (int p = 0; p < 3; ++p)
    if (!ref[p] || !dis[p] || (m && !applied[p])) return fail(nullptr, PQA_EINVAL, "pqa_debug_colour: plane %d pointer is null", p);
  const int rc = need_device();
  if (rc != PQA_OK) return rc;
  const int es = bit_depth > 8 ? 2 : 1;
  const uint32_t pw[3] = {w, (w + (1u << hshift) - 1) >> hshift, (w + (1u << hshift) - 1) >> hshift};
  const uint32_t ph[3] = {h, (h + (1u << vshift) - 1) >> vshift, (h + (1u << vshift) - 1) >> vshift};
  Scratch s;
  PlaneRun r[3], d[3];
  MutPlaneRun o[3];
  for (int p = 0; p < 3; ++p) {
    const size_t row = (size_t)pw[p] * es;
    r[p] = PlaneRun{s.plane(ref[p], (int64_t)row, row, ph[p]), (int64_t)pw[p], 0};
    d[p] = PlaneRun{s.plane(dis[p], (int64_t)row, row, ph[p]), (int64_t)pw[p], 0};
    o[p] = MutPlaneRun{m ? s.get<uint8_t>(row * ph[p]) : nullptr, (int64_t)pw[p], 0};
  }
  unsigned long long* sums = s.get<unsigned long long>(kColourSums);
  hipError_t e = s.err;
  const Elem elem = es == 1 ? ELEM_U8 : ELEM_U16;
  if (e == hipSuccess && sums28)
    e = launch_colour_moments(nullptr, elem, (int)bit_depth, (int)hshift, (int)vshift, r, d, 1, (int)w, (int)h, lo, hi, sums);
  if (e == hipSuccess && sums28) e = hipMemcpy(sums28, sums, kColourSums * sizeof(uint64_t), hipMemcpyDeviceToHost);
  if (e == hipSuccess && m) e = launch_colour_apply(nullptr, elem, (int)bit_depth, (int)hshift, (int)vshift, m, d, o, 1, (int)w, (int)h);
  for (int p = 0; p < 3 && e == hipSuccess && m; ++p) e = hipMemcpy(applied[p], o[p].base, (size_t)pw[p] * es * ph[p], hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail(nullptr, PQA_EDEVICE, "pqa_debug_colour: %s", hipGetErrorString(e));
  return PQA_OK;
}

}  // extern "C"
