// libvmaf's psnr_hvs feature: per plane (Y, Cb, Cr) 8x8 blocks at a step of 7, on both frames the global / quadrant
// variance ratio g, Daala's integer lifting DCT (od_bin_fdct8x8), the contrast masks sqrt(g * sum_AC coef^2 M) / 32, then
// the CSF-weighted, mask-thresholded squared coefficient differences.  The definition, its constants and its unpinned
// items: tests/psnr_hvs_ref.py and DESIGN.md section 1.
//
// Two kernels:
//   phv_kernel<T>        eight lanes per block, 32 blocks side by side per workgroup, kPhvTileRows block rows per
//                        workgroup.  Lane j loads column j of the block (ref and dis) and runs od_bin_fdct8 on it in
//                        registers; the 8 x 8 intermediate is transposed through LDS (rows padded to 9 dwords: both the
//                        writes and the column reads are conflict-free) and lane i runs the second pass, ending with row i
//                        of the coefficients.  The block's sums (samples, quadrant halves, variances, masks, error) reduce
//                        over the eight lanes with three DPP adds (two quad_perm, one row_half_mirror), in a fixed order.
//                        The DCT is exact int32 with 24-bit multiplies (|u| < 2^17, |u * mul| < 2^29 at 12 bit); what
//                        follows it is f32 per block, each block's error sum is added in double, and every workgroup
//                        writes one double partial.  DC needs no branch: M[0][0] = 0 drops it from the mask sum and
//                        1 / M[0][0] is stored as 0, so its threshold is 0.
//   phv_finalize_kernel  per frame: fixed-order sums of each plane's partials, mse_p = sum / (64 blocks_p), the dB values
//                        and the 0.8 / 0.1 / 0.1 combination in double, into slots 0..6 of the frame's ext2 row.
// No atomics, no scratch: a frame's value does not depend on batch, launch, pitch or alignment.
#include <cmath>

#include "../../include/pqa_vmaf.h"
#include "kernels.h"
#include "pqa_device.h"

namespace pqa {

// ---- tables (tests/psnr_hvs_ref.py CONST) --------------------------------------------------------------------------------
static const double kCsf[3][8][8] = {
    {{1.6193873005, 2.2901594831, 2.08509755623, 1.48366094411, 1.00227514334, 0.678296995242, 0.466224900598, 0.3265091542},
     {2.2901594831, 1.94321815382, 2.04793073064, 1.68731108984, 1.2305666963, 0.868920337363, 0.61280991668, 0.436405793551},
     {2.08509755623, 2.04793073064, 1.34329019223, 1.09205635862, 0.875748795257, 0.670882927016, 0.501731932449, 0.372504254596},
     {1.48366094411, 1.68731108984, 1.09205635862, 0.772819797575, 0.605636379554, 0.48309405692, 0.380429446972, 0.295774038565},
     {1.00227514334, 1.2305666963, 0.875748795257, 0.605636379554, 0.448996256676, 0.352889268808, 0.283006984131, 0.226951348204},
     {0.678296995242, 0.868920337363, 0.670882927016, 0.48309405692, 0.352889268808, 0.27032073436, 0.215017739696, 0.17408067321},
     {0.466224900598, 0.61280991668, 0.501731932449, 0.380429446972, 0.283006984131, 0.215017739696, 0.168869545842, 0.136153931001},
     {0.3265091542, 0.436405793551, 0.372504254596, 0.295774038565, 0.226951348204, 0.17408067321, 0.136153931001, 0.109083846276}},
    {{1.91113096927, 2.46074210438, 1.18284184739, 1.14982565193, 1.05017074788, 0.898018824055, 0.74725392039, 0.615105596242},
     {2.46074210438, 1.58529308355, 1.21363250036, 1.38190029285, 1.33100189972, 1.17428548929, 0.996404342439, 0.830890433625},
     {1.18284184739, 1.21363250036, 0.978712413627, 1.02624506078, 1.03145147362, 0.960060382087, 0.849823426169, 0.731221236837},
     {1.14982565193, 1.38190029285, 1.02624506078, 0.861317501629, 0.801821139099, 0.751437590932, 0.685398513368, 0.608694761374},
     {1.05017074788, 1.33100189972, 1.03145147362, 0.801821139099, 0.676555426187, 0.605503172737, 0.55002013668, 0.495804539034},
     {0.898018824055, 1.17428548929, 0.960060382087, 0.751437590932, 0.605503172737, 0.514674450957, 0.454353482512, 0.407050308965},
     {0.74725392039, 0.996404342439, 0.849823426169, 0.685398513368, 0.55002013668, 0.454353482512, 0.389234902883, 0.342353999733},
     {0.615105596242, 0.830890433625, 0.731221236837, 0.608694761374, 0.495804539034, 0.407050308965, 0.342353999733, 0.295530605237}},
    {{2.03871978502, 2.62502345193, 1.26180942886, 1.11019789803, 1.01397751469, 0.867069376285, 0.721500455585, 0.593906509971},
     {2.62502345193, 1.69112867013, 1.17180569821, 1.3342742857, 1.28513006198, 1.13381474809, 0.962064122248, 0.802254508198},
     {1.26180942886, 1.17180569821, 0.944981930573, 0.990876405848, 0.995903384143, 0.926972725286, 0.820534991409, 0.706020324706},
     {1.11019789803, 1.3342742857, 0.990876405848, 0.831632933426, 0.77418706195, 0.725539939514, 0.661776842059, 0.587716619023},
     {1.01397751469, 1.28513006198, 0.995903384143, 0.77418706195, 0.653238524286, 0.584635025748, 0.531064164893, 0.478717061273},
     {0.867069376285, 1.13381474809, 0.926972725286, 0.725539939514, 0.584635025748, 0.496936637883, 0.438694579826, 0.393021669543},
     {0.721500455585, 0.962064122248, 0.820534991409, 0.661776842059, 0.531064164893, 0.438694579826, 0.375820256136, 0.330555063063},
     {0.593906509971, 0.802254508198, 0.706020324706, 0.587716619023, 0.478717061273, 0.393021669543, 0.330555063063, 0.285345396658}}};
constexpr double kMaskK = 0.3885746225901003;

void psnr_hvs_tables(float* out) {
  for (int k = 0; k < 3; ++k)
    for (int i = 0; i < 64; ++i) {
      const float c = (float)kCsf[k][i / 8][i % 8];
      out[k * 64 + i] = c;
      out[192 + k * 64 + i] = (float)(((double)c * kMaskK) * ((double)c * kMaskK));   // as libvmaf stores M
    }
}

// ---- Daala's od_bin_fdct8 (tests/psnr_hvs_ref.py fdct8): lifting steps (u * mul + r) >> s, exact in int32 ---------------
// |u| < 2^17 and |u * mul + r| < 2^29 for samples below 2^12, so the products fit 24-bit multiplies (v_mul_i32_i24).
// (with __mul24 the compiler left a third of them as v_mul_lo_u32; the rounding term rides in the same v_mad_i32_i24)
template <int MUL, int SHIFT>
__host__ __device__ __forceinline__ int phv_lift(int u) {
#if defined(__HIP_DEVICE_COMPILE__)
  int p;
  asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(p) : "v"(u), "s"(MUL), "v"(1 << (SHIFT - 1)));
  return p >> SHIFT;
#else
  return (u * MUL + (1 << (SHIFT - 1))) >> SHIFT;
#endif
}
// OD_DCT_RSHIFT(a, 1): halving rounded toward zero (the sign bit is added before the arithmetic shift)
__host__ __device__ __forceinline__ int phv_half(int a) { return (a + (int)((unsigned)a >> 31)) >> 1; }

__host__ __device__ __forceinline__ void psnr_hvs_fdct8(int (&x)[8]) {
  int t0 = x[0], t4 = x[1], t2 = x[2], t6 = x[3], t7 = x[4], t3 = x[5], t5 = x[6], t1 = x[7];
  t1 = t0 - t1;
  const int t1h = phv_half(t1);
  t0 -= t1h;
  t4 += t5;
  const int t4h = phv_half(t4);
  t5 -= t4h;
  t3 = t2 - t3;
  t2 -= phv_half(t3);
  t6 += t7;
  const int t6h = phv_half(t6);
  t7 = t6h - t7;
  t0 += t6h;
  t6 = t0 - t6;
  t2 = t4h - t2;
  t4 = t2 - t4;
  t0 -= phv_lift<13573, 15>(t4);
  t4 += phv_lift<11585, 14>(t0);
  t0 -= phv_lift<13573, 15>(t4);
  t6 -= phv_lift<21895, 15>(t2);
  t2 += phv_lift<15137, 14>(t6);
  t6 -= phv_lift<21895, 15>(t2);
  t3 += phv_lift<19195, 15>(t5);
  t5 += phv_lift<11585, 14>(t3);
  t3 -= phv_lift<7489, 13>(t5);
  t7 = phv_half(t5) - t7;
  t5 -= t7;
  t3 = t1h - t3;
  t1 -= t3;
  t7 += phv_lift<3227, 15>(t1);
  t1 -= phv_lift<6393, 15>(t7);
  t7 += phv_lift<3227, 15>(t1);
  t5 += phv_lift<2485, 13>(t3);
  t3 -= phv_lift<18205, 15>(t5);
  t5 += phv_lift<2485, 13>(t3);
  x[0] = t0; x[1] = t1; x[2] = t2; x[3] = t3; x[4] = t4; x[5] = t5; x[6] = t6; x[7] = t7;
}

void psnr_hvs_fdct8x8_host(const int32_t* in, int32_t* out, int n) {
  for (int b = 0; b < n; ++b) {
    const int32_t* x = in + (int64_t)b * 64;
    int z[8][8];
    for (int j = 0; j < 8; ++j) {            // column j of the block -> row j of z
      int c[8];
      for (int i = 0; i < 8; ++i) c[i] = x[i * 8 + j];
      psnr_hvs_fdct8(c);
      for (int i = 0; i < 8; ++i) z[j][i] = c[i];
    }
    for (int j = 0; j < 8; ++j) {            // column j of z -> coefficient row j
      int c[8];
      for (int i = 0; i < 8; ++i) c[i] = z[i][j];
      psnr_hvs_fdct8(c);
      for (int i = 0; i < 8; ++i) out[(int64_t)b * 64 + j * 8 + i] = c[i];
    }
  }
}

namespace {

constexpr int kBx = kBlock / 8;          // blocks side by side per workgroup (eight lanes each)
constexpr int kRows = kPhvTileRows;      // block rows per workgroup
constexpr int kPad = 9;                  // LDS row of the 8 x 8 transpose (dwords)

// per plane kind: csf[8][8], mask[8][8] (M[0][0] = 0), 1 / mask[8][8] (0 at DC)
struct PhvTables {
  float csf[3][64], mask[3][64], inv[3][64];
};
__constant__ PhvTables g_phv;

// ---- the frame kernel ----------------------------------------------------------------------------------------------------
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ int dpp_i(int v) {
  return __builtin_amdgcn_update_dpp(0, v, CTRL, ROW_MASK, 0xf, true);
}
// Sum over the eight lanes of a block, identical in all eight (quad swaps, then the mirrored half-row).
__device__ __forceinline__ int red8(int v) {
  v += dpp_i<0xb1>(v);
  v += dpp_i<0x4e>(v);
  return v + dpp_i<0x141>(v);
}
__device__ __forceinline__ float red8(float v) {
  v += __builtin_bit_cast(float, dpp_i<0xb1>(__builtin_bit_cast(int, v)));
  v += __builtin_bit_cast(float, dpp_i<0x4e>(__builtin_bit_cast(int, v)));
  return v + __builtin_bit_cast(float, dpp_i<0x141>(__builtin_bit_cast(int, v)));
}
// Over the four lanes of a half-block (columns 0-3 or 4-7).
__device__ __forceinline__ int red4(int v) {
  v += dpp_i<0xb1>(v);
  return v + dpp_i<0x4e>(v);
}

struct PhvArgs {
  const void* ref[3];
  const void* dis[3];
  int64_t fp_r[3], fp_d[3];            // frame pitches, elements
  int rp_r[3], rp_d[3];                // row pitches, elements
  int nbx[3], nby[3];                  // blocks across / down
  int tiles_x[3];
  int tile0[4];                        // plane p owns workgroups [tile0[p], tile0[p + 1])
  double* partials;                    // [n_frames][tile0[3]]
  float* block_err;                    // nullable (debug): [nby][nbx] block sums of plane dbg_plane of frame 0
  int dbg_plane;
};

// g = sum of the quadrant variances / the global variance (0 for a flat block); s[0..7] is this lane's column of the block
__device__ __forceinline__ float phv_g(const int (&s)[8]) {
  int cs = 0, top = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) cs += s[i];
#pragma unroll
  for (int i = 0; i < 4; ++i) top += s[i];
  const int gsum = red8(cs), tsum = red4(top), bsum = red4(cs - top);
  const float gm = (float)gsum * (1.0f / 64.0f), tm = (float)tsum * (1.0f / 16.0f), bm = (float)bsum * (1.0f / 16.0f);
  float gv = 0.0f, qv = 0.0f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float x = (float)s[i], d = x - gm, dq = x - (i < 4 ? tm : bm);
    gv = fmaf(d, d, gv);
    qv = fmaf(dq, dq, qv);
  }
  gv = red8(gv) * (64.0f / 63.0f);
  qv = red8(qv) * (16.0f / 15.0f);
  return gv > 0.0f ? qv / gv : 0.0f;
}

// the eight lanes of a block sit in one wave: ordering their LDS traffic needs a wave-scope fence, not a workgroup barrier
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// transpose of the eight lanes' rows r[0..7] through this block's LDS tile (lane j writes row j, reads column j)
__device__ __forceinline__ void phv_transpose(int (&r)[8], int* t, int j) {
#pragma unroll
  for (int k = 0; k < 8; ++k) t[j * kPad + k] = r[k];
  wave_sync();
#pragma unroll
  for (int k = 0; k < 8; ++k) r[k] = t[k * kPad + j];
  wave_sync();
}

template <typename T>
__global__ __launch_bounds__(kBlock) void phv_kernel(const PhvArgs a) {
  __shared__ int lds[kBx * 8 * kPad];
  __shared__ double red[4];
  const int fr = blockIdx.y;
  const int tile = blockIdx.x;
  const int p = tile >= a.tile0[2] ? 2 : tile >= a.tile0[1] ? 1 : 0;
  const int t = tile - a.tile0[p];
  const int g = threadIdx.x >> 3, j = threadIdx.x & 7;
  const int bx = (t % a.tiles_x[p]) * kBx + g;
  const int by0 = (t / a.tiles_x[p]) * kRows;
  const T* rp = (const T*)a.ref[p] + (int64_t)fr * a.fp_r[p];
  const T* dp = (const T*)a.dis[p] + (int64_t)fr * a.fp_d[p];
  const int rpr = a.rp_r[p], rpd = a.rp_d[p];
  int* tl = lds + g * 8 * kPad;
  // lane j ends with coefficient row j: its CSF, mask and threshold rows of this plane kind
  float csf[8], msk[8], inv[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    csf[k] = g_phv.csf[p][j * 8 + k];
    msk[k] = g_phv.mask[p][j * 8 + k];
    inv[k] = g_phv.inv[p][j * 8 + k];
  }
  const bool ok = bx < a.nbx[p];
  const int bxc = ok ? bx : a.nbx[p] - 1;
  const T* rcol = rp + bxc * 7 + j;
  const T* dcol = dp + bxc * 7 + j;
  double acc = 0.0;
  for (int r = 0; r < kRows; ++r) {
    const int by = by0 + r;
    if (by >= a.nby[p]) break;                      // uniform over the workgroup
    // the groups right of the plane's last block load that block again (no branches around the loads); their sums stay
    // inside their own eight lanes and are dropped
    int s[8], d[8];
    const T* rr = rcol + (int64_t)by * 7 * rpr;
    const T* dr = dcol + (int64_t)by * 7 * rpd;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      s[i] = (int)rr[(int64_t)i * rpr];   // 64-bit: seven rows of a pitch near 2^31 samples leave `int`
      d[i] = (int)dr[(int64_t)i * rpd];
    }
    const float gs = phv_g(s), gd = phv_g(d);
    // od_bin_fdct8x8: column j -> row j of the intermediate, transpose, column j of that -> coefficient row j
    psnr_hvs_fdct8(s);
    psnr_hvs_fdct8(d);
    phv_transpose(s, tl, j);
    psnr_hvs_fdct8(s);
    phv_transpose(d, tl, j);
    psnr_hvs_fdct8(d);
    float ms = 0.0f, md = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      ms = fmaf((float)__mul24(s[k], s[k]), msk[k], ms);
      md = fmaf((float)__mul24(d[k], d[k]), msk[k], md);
    }
    ms = red8(ms);
    md = red8(md);
    const float m = fmaxf(__builtin_sqrtf(ms * gs), __builtin_sqrtf(md * gd)) * (1.0f / 32.0f);
    float e = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float err = fmaxf((float)abs(s[k] - d[k]) - m * inv[k], 0.0f) * csf[k];
      e = fmaf(err, err, e);
    }
    e = red8(e);
    if (ok && j == 0) {
      acc += (double)e;
      if (a.block_err && p == a.dbg_plane && fr == 0) a.block_err[(int64_t)by * a.nbx[p] + bx] = e;
    }
  }
  double v[1] = {acc};
  block_sum<1>(v, red);
  if (threadIdx.x == 0) a.partials[(int64_t)fr * a.tile0[3] + tile] = v[0];
}

__global__ __launch_bounds__(kBlock) void phv_finalize_kernel(const PsnrHvsFinalizeArgs a) {
  __shared__ double red[4 * 3];
  const int fr = blockIdx.x;
  double acc[3] = {0.0, 0.0, 0.0};
  const double* q = a.partials + (int64_t)fr * a.tile0[3];
#pragma unroll
  for (int p = 0; p < 3; ++p)
    for (int i = a.tile0[p] + (int)threadIdx.x; i < a.tile0[p + 1]; i += kBlock) acc[p] += q[i];
  block_sum<3>(acc, red);
  if (threadIdx.x != 0) return;
  const int row = (int)(((int64_t)a.slot_base + (int64_t)fr * a.slot_step) % a.capacity);
  double* e = a.ext2 + (int64_t)row * a.ext_stride;
  const double peak2 = a.peak * a.peak;
  double mse[3];
  for (int p = 0; p < 3; ++p) {
    mse[p] = acc[p] / (64.0 * (double)a.blocks[p]);
    e[PQA_EXT2_PSNR_HVS_MSE + p] = mse[p];
    e[PQA_EXT2_PSNR_HVS_Y + p] = mse[p] > 0.0 ? 10.0 * log10(peak2 / mse[p]) : __builtin_inf();
  }
  const double comb = 0.8 * mse[0] + (0.1 * mse[1] + 0.1 * mse[2]);
  e[PQA_EXT2_PSNR_HVS] = comb > 0.0 ? 10.0 * log10(peak2 / comb) : __builtin_inf();
}

template <typename T>
hipError_t launch_phv_t(hipStream_t stream, const dim3 grid, const PhvArgs& a) {
  hipLaunchKernelGGL((phv_kernel<T>), grid, dim3(kBlock), 0, stream, a);
  return hipGetLastError();
}

}  // namespace

void psnr_hvs_geometry(const int pw[3], const int ph[3], PsnrHvsGeometry* g) {
  g->tile0[0] = 0;
  for (int p = 0; p < 3; ++p) {
    g->nbx[p] = pw[p] >= 8 ? (pw[p] - 1) / 7 : 0;
    g->nby[p] = ph[p] >= 8 ? (ph[p] - 1) / 7 : 0;
    g->tiles_x[p] = (g->nbx[p] + kBx - 1) / kBx;
    g->tile0[p + 1] = g->tile0[p] + g->tiles_x[p] * ((g->nby[p] + kRows - 1) / kRows);
  }
}

hipError_t psnr_hvs_prepare() {
  PhvTables t{};
  float f[384];
  psnr_hvs_tables(f);
  for (int k = 0; k < 3; ++k)
    for (int i = 0; i < 64; ++i) {
      t.csf[k][i] = f[k * 64 + i];
      t.mask[k][i] = i ? f[192 + k * 64 + i] : 0.0f;
      t.inv[k][i] = i ? 1.0f / f[192 + k * 64 + i] : 0.0f;
    }
  return hipMemcpyToSymbol(HIP_SYMBOL(g_phv), &t, sizeof t);
}

hipError_t launch_psnr_hvs(hipStream_t stream, Elem elem, const PlaneRun ref[3], const PlaneRun dis[3], int n_frames,
                           const PsnrHvsGeometry& geo, double* partials, float* block_err, int dbg_plane) {
  if (n_frames <= 0 || geo.tile0[3] <= 0) return hipSuccess;
  PhvArgs a{};
  for (int p = 0; p < 3; ++p) {
    if (ref[p].row_pitch >= (1ll << 31) || dis[p].row_pitch >= (1ll << 31)) return hipErrorInvalidValue;
    if (geo.nbx[p] <= 0 || geo.nby[p] <= 0) return hipErrorInvalidValue;
    a.ref[p] = ref[p].base; a.dis[p] = dis[p].base;
    a.rp_r[p] = (int)ref[p].row_pitch; a.fp_r[p] = ref[p].frame_pitch;
    a.rp_d[p] = (int)dis[p].row_pitch; a.fp_d[p] = dis[p].frame_pitch;
    a.nbx[p] = geo.nbx[p]; a.nby[p] = geo.nby[p]; a.tiles_x[p] = geo.tiles_x[p];
  }
  for (int p = 0; p < 4; ++p) a.tile0[p] = geo.tile0[p];
  a.partials = partials;
  a.block_err = block_err;
  a.dbg_plane = dbg_plane;
  const dim3 grid(geo.tile0[3], n_frames);
  switch (elem) {
    case ELEM_U8: return launch_phv_t<uint8_t>(stream, grid, a);
    case ELEM_U16: return launch_phv_t<uint16_t>(stream, grid, a);
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_psnr_hvs_finalize(hipStream_t stream, const PsnrHvsFinalizeArgs& args) {
  if (args.n_frames <= 0) return hipSuccess;
  hipLaunchKernelGGL(phv_finalize_kernel, dim3(args.n_frames), dim3(kBlock), 0, stream, args);
  return hipGetLastError();
}

}  // namespace pqa
