// The one-shot analyses of the C ABI that leave the scoring chain alone: anchored frame differences, luma statistics,
// temporal / spatial / level alignment, the resampler, the registration moments, the line profiles, the tile moments, the band moments, the temporal moments, the edge profiles, the colour moments and matrix apply.  Each has an entry for a clip in HBM and one for frames in host memory; the host
// entries share one staging path (stage_frames), every entry ends in one epilogue (side_finish).
// Declarations: include/pqa_vmaf.h; the context: pqa_ctx.h.
#include "pqa_ctx.h"

#include <climits>
#include <cstdio>

using namespace pqa;

namespace {

int chunk_len(int total, int done, int cap) { return total - done < cap ? total - done : cap; }

// ---- argument rules; no device call ----------------------------------------------------------------------------------
// `who` opens the message ("cross_sse: ", "plane 1 ", "").

// A clip in HBM: both pitches are whole samples, and rows lie at least min_row bytes apart.
int check_device_clip(pqa_ctx* c, const char* who, int64_t row_pitch, int64_t frame_pitch, int64_t min_row) {
  if (row_pitch % c->esize || frame_pitch % c->esize) return fail(c, PQA_EINVAL, "%spitch is not a multiple of the sample size", who);
  if (row_pitch < min_row) return fail(c, PQA_EINVAL, "%spitch smaller than a row", who);
  return PQA_OK;
}

// A list of n host frames, `step` pointers from one to the next (`kind`: "reference ", "captured ", ""): rows `stride` bytes
// apart hold a row, no pointer is null.  The entries disagree on a negative stride -- pqa_level_stats and pqa_frame_sad
// refuse it, the others let it pass the unsigned comparison -- and each keeps its answer: refuse_negative.
int check_host_frames(pqa_ctx* c, const char* who, const char* kind, const void* const* frames, int step, int n, int64_t stride,
                      size_t row_bytes, bool refuse_negative) {
  if (n > 0 && ((refuse_negative && stride < 0) || (size_t)stride < row_bytes))
    return fail(c, PQA_EINVAL, "%sstride smaller than a row", who);
  for (int f = 0; f < n; ++f)   // before anything is queued
    if (!frames[(size_t)f * step]) return fail(c, PQA_EINVAL, "%s%sframe %d pointer is null", who, kind, f);
  return PQA_OK;
}

// ---- host frames onto the stream ---------------------------------------------------------------------------------------
// the two pinned + two device halves of LB luma planes that the host entries pack their frames into
int luma_staging_ensure(pqa_ctx* c) {
  if (c->luma_ready) return PQA_OK;   // lazily: most contexts never detect bookends
  c->luma_pitch = round_up((int64_t)c->pw[0] * c->esize, 64);
  c->LB = c->B < 8 ? c->B : 8;
  const size_t half = (size_t)c->luma_pitch * c->ph[0] * c->LB;
  hipError_t e = hipSuccess;
  for (int i = 0; i < 2 && e == hipSuccess; ++i) {
    Half& H = c->luma_half[i];
    if (!H.pinned) e = hipHostMalloc((void**)&H.pinned, half, hipHostMallocDefault);
    if (e == hipSuccess && !H.dev) e = hipMalloc((void**)&H.dev, half);
    if (e == hipSuccess && !H.copied) e = hipEventCreateWithFlags(&H.copied, hipEventDisableTiming);
  }
  if (e != hipSuccess) {   // all six or none: a half-made set must not make every later call fail on a null handle
    for (Half& H : c->luma_half) {
      if (H.pinned) hipHostFree(H.pinned);
      if (H.dev) hipFree(H.dev);
      if (H.copied) hipEventDestroy(H.copied);
      H = Half{};
    }
    return fail(c, e == hipErrorOutOfMemory ? PQA_ENOMEM : PQA_EDEVICE, "luma staging allocation failed: %s", hipGetErrorString(e));
  }
  c->luma_ready = true;
  return PQA_OK;
}

// n planes of row_bytes x h from frames[0 .. n) (rows `stride` bytes apart) through pinned half hf onto the stream: waits
// until the upload that last used the half has left it, packs, queues the upload, records the half's event.  The planes
// land in device half hf, one after the other -- or, with ring_base, frame k in slot (first + k) % ring_slots of that ring,
// each uploaded as soon as it is packed (a ring may wrap inside a chunk).  A plane smaller than the luma plane travels
// with the luma pitches.
hipError_t stage_frames(pqa_ctx* c, int hf, const void* const* frames, int64_t stride, int n, size_t row_bytes, int h,
                        uint8_t* ring_base = nullptr, int ring_slots = 1, int64_t first = 0) {
  Half& H = c->luma_half[hf];
  const size_t frame_bytes = (size_t)c->luma_pitch * c->ph[0];
  hipError_t e = hipSuccess;
  if (H.copied_pending) {
    e = hipEventSynchronize(H.copied);
    H.copied_pending = false;
  }
  for (int f = 0; f < n && e == hipSuccess; ++f) {
    uint8_t* pin = H.pinned + (size_t)f * frame_bytes;
    copy_plane_rows(pin, c->luma_pitch, (const uint8_t*)frames[f], stride, row_bytes, h);
    if (ring_base)
      e = hipMemcpyAsync(ring_base + (size_t)((first + f) % ring_slots) * frame_bytes, pin, frame_bytes, hipMemcpyHostToDevice,
                         c->stream);
  }
  if (e == hipSuccess && !ring_base) e = hipMemcpyAsync(H.dev, H.pinned, (size_t)n * frame_bytes, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipEventRecord(H.copied, c->stream);
  H.copied_pending = e == hipSuccess;
  return e;
}

// The end of every entry, after its launches (e: the first error among them): the results go to the caller unless
// something failed or the call was cancelled, and the stream is ALWAYS synchronised -- nothing queued on it may still point
// at the pinned halves or at `out` when the call returns.
int side_finish(pqa_ctx* c, const char* what, hipError_t e, void* out, const void* dev_out, size_t bytes) {
  if (e == hipSuccess && !c->cancelled.load() && bytes) e = hipMemcpyAsync(out, dev_out, bytes, hipMemcpyDeviceToHost, c->stream);
  const hipError_t es = hipStreamSynchronize(c->stream);
  c->luma_half[0].copied_pending = c->luma_half[1].copied_pending = false;
  if (c->cancelled.load()) return fail(c, PQA_ECANCELLED, "cancelled");
  if (e != hipSuccess) return fail(c, PQA_EDEVICE, "%s failed: %s", what, hipGetErrorString(e));
  if (es != hipSuccess) return fail(c, PQA_EDEVICE, "hipStreamSynchronize failed: %s", hipGetErrorString(es));
  return PQA_OK;
}

// a grow-only device buffer of the side analyses
int side_reserve(pqa_ctx* c, SideBuf which, size_t bytes) {
  if (bytes == 0) bytes = 1;
  if (c->side_cap[which] >= bytes) return PQA_OK;
  if (c->side_buf[which]) {
    HIPCHK(c, hipFree(c->side_buf[which]));
    c->side_buf[which] = nullptr;
    c->side_cap[which] = 0;
  }
  HIPCHK(c, hipMalloc(&c->side_buf[which], bytes));
  c->side_cap[which] = bytes;
  return PQA_OK;
}

// the launch of pqa_frame_sad[_device]: n frames (at most B) of a device clip against the anchor planes, results to out
int frame_sad_launch(pqa_ctx* c, const void* const anchor[3], const int64_t anchor_pitch_bytes[3], const pqa_device_clip* f,
                     int n, uint64_t* out) {
  const int es = c->esize;
  PlaneRun cur[3] = {};
  int64_t app[3] = {0, 0, 0};
  for (int p = 0; p < c->n_planes; ++p) {
    cur[p] = PlaneRun{f->plane[p], f->row_pitch[p] / es, f->frame_pitch[p] / es};
    app[p] = anchor_pitch_bytes[p] / es;
  }
  if (!c->ig_out) {
    const int rc = dev_alloc(c, &c->ig_out, (size_t)c->B * 3);
    if (rc != PQA_OK) return rc;
  }
  const hipError_t e = launch_integrity(c->stream, c->elem, cur, anchor, app, c->pw, c->ph, c->n_planes, n, true, c->black_thr,
                                        c->ig_part, nullptr, 0, 0, 1, c->ig_out);
  return side_finish(c, "frame_sad", e, out, c->ig_out, (size_t)n * 3 * sizeof(uint64_t));
}

// ---- temporal alignment (cross_sse.hip): argument rules (no device call) and workspaces ------------------------------
int xs_check(pqa_ctx* c, const void* ref, const void* dis, int32_t n_ref, int32_t n_dis, int32_t k_lo, int32_t k_hi,
             const uint64_t* out) {
  if (!c) return PQA_EINVAL;
  if (!ref || !dis) return fail(c, PQA_EINVAL, "cross_sse: null clip pointer");
  if (n_ref < 0 || n_dis < 0) return fail(c, PQA_EINVAL, "cross_sse: negative frame count");
  if (k_lo > k_hi) return fail(c, PQA_EINVAL, "cross_sse: k_lo %d > k_hi %d", k_lo, k_hi);
  if (k_lo < -64 || k_hi > 64) return fail(c, PQA_EINVAL, "cross_sse: offsets %d ... %d outside -64 ... 64", k_lo, k_hi);
  if ((int64_t)k_hi - k_lo + 1 > 129) return fail(c, PQA_EINVAL, "cross_sse: span above 129");
  if (!out) return fail(c, PQA_EINVAL, "cross_sse: null output pointer");
  return PQA_OK;
}

constexpr int kXsTilesPerLaunch = 8;   // reference tiles (of 32 frames) per launch of the device-resident entry

int xs_prepare(pqa_ctx* c, bool mfma, int span, int n_tiles, int32_t n_ref, int32_t n_dis) {
  int rc = side_reserve(c, SIDE_XSSE_PART, xsse_part_bytes(mfma, c->pw[0], c->ph[0], span, n_tiles));
  if (rc == PQA_OK) rc = side_reserve(c, SIDE_XSSE_OUT, (size_t)n_ref * span * sizeof(uint64_t));
  if (rc == PQA_OK && mfma) rc = side_reserve(c, SIDE_XSSE_NORM_REF, (size_t)n_ref * kXsseNormBlocks * sizeof(uint64_t));
  if (rc == PQA_OK && mfma) rc = side_reserve(c, SIDE_XSSE_NORM_DIS, (size_t)n_dis * kXsseNormBlocks * sizeof(uint64_t));
  return rc;
}

// ---- spatial alignment (shift_sse.hip): argument rules and workspaces ------------------------------------------------
int sh_check(pqa_ctx* c, const void* ref, const void* dis, int32_t n_frames, int32_t radius, const uint64_t* out) {
  if (!c) return PQA_EINVAL;
  if (n_frames < 0) return fail(c, PQA_EINVAL, "shift_sse: negative frame count");
  if (radius < 0 || radius > kShiftMaxRadius) return fail(c, PQA_EINVAL, "shift_sse: radius %d outside 0 ... %d", radius, kShiftMaxRadius);
  if (c->pw[0] <= 2 * radius || c->ph[0] <= 2 * radius)
    return fail(c, PQA_EINVAL, "shift_sse: a %dx%d frame is not larger than twice the radius %d", c->pw[0], c->ph[0], radius);
  if (n_frames > 0 && (!ref || !dis)) return fail(c, PQA_EINVAL, "shift_sse: null clip pointer");
  if (n_frames > 0 && !out) return fail(c, PQA_EINVAL, "shift_sse: null output pointer");
  return PQA_OK;
}

int sh_prepare(pqa_ctx* c, int radius, int32_t n_frames) {
  const int chunk = n_frames < kShiftChunk ? n_frames : kShiftChunk;
  const size_t n = (size_t)(2 * radius + 1) * (2 * radius + 1);
  int rc = side_reserve(c, SIDE_SHIFT_PART, shift_part_bytes(c->elem, c->pw[0], c->ph[0], radius, chunk));
  if (rc == PQA_OK) rc = side_reserve(c, SIDE_SHIFT_ROWSQ, shift_rowsq_bytes(c->ph[0], radius, chunk));
  if (rc == PQA_OK) rc = side_reserve(c, SIDE_SHIFT_OUT, (size_t)n_frames * n * sizeof(uint64_t));
  return rc;
}

// ---- level alignment (level_stats.hip): argument rules ---------------------------------------------------------------
int lv_check(pqa_ctx* c, const void* ref, const void* dis, int32_t n_frames, int32_t plane, const uint64_t* out) {
  if (!c) return PQA_EINVAL;
  if (n_frames < 0) return fail(c, PQA_EINVAL, "level_stats: negative frame count");
  if (plane < 0 || plane >= c->n_planes) return fail(c, PQA_EINVAL, "level_stats: plane %d of a context with %d", plane, c->n_planes);
  if (n_frames > 0 && (!ref || !dis)) return fail(c, PQA_EINVAL, "level_stats: null clip pointer");
  if (n_frames > 0 && !out) return fail(c, PQA_EINVAL, "level_stats: null output pointer");
  return PQA_OK;
}


// ---- resampler (resample.hip): argument rules (no device call), tables, pinned chunks ---------------------------------
int rs_check(pqa_ctx* c, const pqa_resample_spec* sp) {
  if (!c) return PQA_EINVAL;
  if (!sp) return fail(c, PQA_EINVAL, "resample: null spec");
  if (sp->struct_size != sizeof(pqa_resample_spec)) return fail(c, PQA_EINVAL, "resample: bad struct_size %u", sp->struct_size);
  if (sp->filter > PQA_RESAMPLE_LANCZOS3) return fail(c, PQA_EINVAL, "resample: bad filter %u", sp->filter);
  for (uint32_t v : {sp->src_width, sp->src_height, sp->dst_width, sp->dst_height})
    if (v < 1 || v > 8192) return fail(c, PQA_EINVAL, "resample: plane size %u outside 1 ... 8192", v);
  if (sp->w_q16 <= 0 || sp->h_q16 <= 0) return fail(c, PQA_EINVAL, "resample: the source window is not positive");
  return PQA_OK;
}

// the cached device tables of a spec (built and uploaded when the context has not seen it): *slot
int rs_tables(pqa_ctx* c, const pqa_resample_spec* sp, int* slot) {
  for (int i = 0; i < kRsCached; ++i)
    if (c->rs_cache[i].valid && !memcmp(&c->rs_cache[i].spec, sp, sizeof *sp)) {
      *slot = i;
      return PQA_OK;
    }
  ResampleTable th, tv;
  if (resample_table((int)sp->filter, (int)sp->src_width, (int)sp->dst_width, sp->x0_q16, sp->w_q16, &th) != 0 ||
      resample_table((int)sp->filter, (int)sp->src_height, (int)sp->dst_height, sp->y0_q16, sp->h_q16, &tv) != 0)
    return fail(c, PQA_EINVAL, "resample: a destination sample needs more than %d taps", kRsMaxTaps);
  const int i = c->rs_next;
  RsCached& e = c->rs_cache[i];
  e.valid = false;
  resample_plan(th, tv, (int)sp->dst_width, (int)sp->dst_height, &e.plan);
  HIPCHK(c, hipSetDevice(c->device));
  const SideBuf buf = (SideBuf)(SIDE_RS_TABLE0 + i);
  const size_t bytes = e.plan.words.size() * sizeof(int32_t);
  const int rc = side_reserve(c, buf, bytes);
  if (rc != PQA_OK) return rc;
  HIPCHK(c, hipMemcpy(c->side_buf[buf], e.plan.words.data(), bytes, hipMemcpyHostToDevice));   // nothing of this call is queued yet
  std::vector<int32_t>().swap(e.plan.words);
  e.spec = *sp;
  e.valid = true;
  c->rs_next = (i + 1) % kRsCached;
  *slot = i;
  return PQA_OK;
}

int rs_pin_reserve(pqa_ctx* c, int which, size_t bytes) {
  if (c->rs_pin_cap[which] >= bytes) return PQA_OK;
  if (c->rs_pin[which]) {
    HIPCHK(c, hipHostFree(c->rs_pin[which]));
    c->rs_pin[which] = nullptr;
    c->rs_pin_cap[which] = 0;
  }
  HIPCHK(c, hipHostMalloc((void**)&c->rs_pin[which], bytes, hipHostMallocDefault));
  c->rs_pin_cap[which] = bytes;
  return PQA_OK;
}

// ---- registration moments (flow_moments.hip): argument rules (no device call) --------------------------------------------
int fl_check(pqa_ctx* c, const pqa_flow_spec* sp, const void* ref, const void* dis, int32_t n_frames, const int64_t* out) {
  if (!c) return PQA_EINVAL;
  if (!sp) return fail(c, PQA_EINVAL, "flow_moments: null spec");
  if (sp->struct_size != sizeof(pqa_flow_spec)) return fail(c, PQA_EINVAL, "flow_moments: bad struct_size %u", sp->struct_size);
  if (sp->tile > 64 || !flow_tile_ok((int)sp->tile)) return fail(c, PQA_EINVAL, "flow_moments: tile %u is not 8, 16, 32 or 64", sp->tile);
  for (uint32_t v : {sp->width, sp->height})
    if (v < 3 || v > 8192) return fail(c, PQA_EINVAL, "flow_moments: plane size %u outside 3 ... 8192", v);
  if (n_frames < 0) return fail(c, PQA_EINVAL, "flow_moments: negative frame count");
  if (n_frames > 0 && (!ref || !dis)) return fail(c, PQA_EINVAL, "flow_moments: null clip pointer");
  if (n_frames > 0 && !out) return fail(c, PQA_EINVAL, "flow_moments: null output pointer");
  return PQA_OK;
}

// ---- colour-matrix alignment (colour_moments.hip): argument rules (no device call), the layout of a staged frame --------------
int cl_check(pqa_ctx* c, const char* who, int32_t n_frames) {
  if (n_frames < 0) return fail(c, PQA_EINVAL, "%s: negative frame count", who);
  if (c->n_planes != 3) return fail(c, PQA_EINVAL, "%s needs the chroma planes: n_planes must be 3 (got %d)", who, c->n_planes);
  if (!colour_shift_ok((int)c->cfg.chroma_hshift, (int)c->cfg.chroma_vshift))
    return fail(c, PQA_EINVAL, "%s: chroma shifts %u, %u (0 or 1 each)", who, c->cfg.chroma_hshift, c->cfg.chroma_vshift);
  return PQA_OK;
}

int cl_check_clip(pqa_ctx* c, const char* who, const pqa_device_clip* d) {
  for (int p = 0; p < 3; ++p) {
    if (!d->plane[p]) return fail(c, PQA_EINVAL, "%splane %d pointer is null", who, p);
    const int rc = check_device_clip(c, who, d->row_pitch[p], d->frame_pitch[p], (int64_t)c->pw[p] * c->esize);
    if (rc != PQA_OK) return rc;
  }
  return PQA_OK;
}

int cl_check_host(pqa_ctx* c, const char* who, const char* kind, const void* const* frames, const int64_t strides[3], int n) {
  for (int p = 0; p < 3; ++p) {
    const int rc = check_host_frames(c, who, kind, frames + p, 3, n, strides[p], (size_t)c->pw[p] * c->esize, true);
    if (rc != PQA_OK) return rc;
  }
  return PQA_OK;
}

// A frame as the host entries stage it: plane p at off[p] with rows pitch[p] bytes apart, `bytes` in all; every offset and
// pitch is a multiple of 16 bytes, so the kernels take their wide loads.
struct ClLayout {
  size_t off[3], bytes;
  int64_t pitch[3];
};
ClLayout cl_layout(const pqa_ctx* c) {
  ClLayout L{};
  for (int p = 0; p < 3; ++p) {
    L.off[p] = L.bytes;
    L.pitch[p] = round_up((int64_t)c->pw[p] * c->esize, 16);
    L.bytes += (size_t)round_up(L.pitch[p] * c->ph[p], 256);
  }
  return L;
}
void cl_runs(const pqa_ctx* c, const ClLayout& L, const void* base, PlaneRun run[3]) {
  for (int p = 0; p < 3; ++p) run[p] = PlaneRun{(const uint8_t*)base + L.off[p], L.pitch[p] / c->esize, (int64_t)(L.bytes / c->esize)};
}
void cl_pack(const pqa_ctx* c, const ClLayout& L, uint8_t* pin, const void* const* frames, const int64_t strides[3], int n) {
  for (int f = 0; f < n; ++f)
    for (int p = 0; p < 3; ++p)
      copy_plane_rows(pin + (size_t)f * L.bytes + L.off[p], L.pitch[p], (const uint8_t*)frames[(size_t)f * 3 + p], strides[p],
                      (size_t)c->pw[p] * c->esize, c->ph[p]);
}

// ---- active-picture detection (line_profiles.hip): argument rules (no device call) -----------------------------------------
int pr_check(pqa_ctx* c, const pqa_profile_spec* sp, const void* planes, int32_t n_frames, const uint64_t* out) {
  if (!c) return PQA_EINVAL;
  if (!sp) return fail(c, PQA_EINVAL, "line_profiles: null spec");
  if (sp->struct_size != sizeof(pqa_profile_spec)) return fail(c, PQA_EINVAL, "line_profiles: bad struct_size %u", sp->struct_size);
  for (uint32_t v : {sp->width, sp->height})
    if (v < 1 || v > 8192) return fail(c, PQA_EINVAL, "line_profiles: plane size %u outside 1 ... 8192", v);
  if (n_frames < 0) return fail(c, PQA_EINVAL, "line_profiles: negative frame count");
  if (n_frames > 0 && !planes) return fail(c, PQA_EINVAL, "line_profiles: null clip pointer");
  if (n_frames > 0 && !out) return fail(c, PQA_EINVAL, "line_profiles: null output pointer");
  return PQA_OK;
}

// ---- distortion map (tile_moments.hip): argument rules (no device call) ----------------------------------------------------
int tl_check(pqa_ctx* c, const pqa_tile_spec* sp, const void* ref, const void* dis, int32_t n_frames, const uint64_t* out) {
  if (!c) return PQA_EINVAL;
  if (!sp) return fail(c, PQA_EINVAL, "tile_moments: null spec");
  if (sp->struct_size != sizeof(pqa_tile_spec)) return fail(c, PQA_EINVAL, "tile_moments: bad struct_size %u", sp->struct_size);
  if (sp->tile > 64 || !tile_size_ok((int)sp->tile)) return fail(c, PQA_EINVAL, "tile_moments: tile %u is not 8, 16, 32 or 64", sp->tile);
  for (uint32_t v : {sp->width, sp->height})
    if (v < 1 || v > 8192) return fail(c, PQA_EINVAL, "tile_moments: plane size %u outside 1 ... 8192", v);
  if (n_frames < 0) return fail(c, PQA_EINVAL, "tile_moments: negative frame count");
  if (n_frames > 0 && (!ref || !dis)) return fail(c, PQA_EINVAL, "tile_moments: null clip pointer");
  if (n_frames > 0 && !out) return fail(c, PQA_EINVAL, "tile_moments: null output pointer");
  return PQA_OK;
}

// ---- distortion spectrum (band_moments.hip): argument rules (no device call) ------------------------------------------------
int bd_check(pqa_ctx* c, const pqa_band_spec* sp, const void* ref, const void* dis, int32_t n_frames, const uint64_t* out) {
  if (!c) return PQA_EINVAL;
  if (!sp) return fail(c, PQA_EINVAL, "band_moments: null spec");
  if (sp->struct_size != sizeof(pqa_band_spec)) return fail(c, PQA_EINVAL, "band_moments: bad struct_size %u", sp->struct_size);
  if (sp->levels > 6 || !band_levels_ok((int)sp->levels)) return fail(c, PQA_EINVAL, "band_moments: %u levels outside 1 ... 6", sp->levels);
  for (uint32_t v : {sp->width, sp->height})
    if (v < 1 || v > 8192) return fail(c, PQA_EINVAL, "band_moments: plane size %u outside 1 ... 8192", v);
  if (n_frames < 0) return fail(c, PQA_EINVAL, "band_moments: negative frame count");
  if (n_frames > 0 && (!ref || !dis)) return fail(c, PQA_EINVAL, "band_moments: null clip pointer");
  if (n_frames > 0 && !out) return fail(c, PQA_EINVAL, "band_moments: null output pointer");
  return PQA_OK;
}

// ---- temporal distortion (temporal_moments.hip): argument rules (no device call) ---------------------------------------------
int tm_check(pqa_ctx* c, const pqa_temporal_spec* sp, const void* ref, const void* dis, int32_t n_frames, const uint64_t* out) {
  if (!c) return PQA_EINVAL;
  if (!sp) return fail(c, PQA_EINVAL, "temporal_moments: null spec");
  if (sp->struct_size != sizeof(pqa_temporal_spec)) return fail(c, PQA_EINVAL, "temporal_moments: bad struct_size %u", sp->struct_size);
  if (sp->tile > 64 || !tile_size_ok((int)sp->tile)) return fail(c, PQA_EINVAL, "temporal_moments: tile %u is not 8, 16, 32 or 64", sp->tile);
  for (uint32_t v : {sp->width, sp->height})
    if (v < 1 || v > 8192) return fail(c, PQA_EINVAL, "temporal_moments: plane size %u outside 1 ... 8192", v);
  if (n_frames < 0) return fail(c, PQA_EINVAL, "temporal_moments: negative frame count");
  if (n_frames > 0 && (!ref || !dis)) return fail(c, PQA_EINVAL, "temporal_moments: null clip pointer");
  if (n_frames > 1 && !out) return fail(c, PQA_EINVAL, "temporal_moments: null output pointer");
  return PQA_OK;
}

// ---- coding-grid detection (edge_profiles.hip): argument rules (no device call) ----------------------------------------------
int eg_check(pqa_ctx* c, const pqa_edge_spec* sp, const void* ref, const void* dis, int32_t n_frames, const uint64_t* out) {
  if (!c) return PQA_EINVAL;
  if (!sp) return fail(c, PQA_EINVAL, "edge_profiles: null spec");
  if (sp->struct_size != sizeof(pqa_edge_spec)) return fail(c, PQA_EINVAL, "edge_profiles: bad struct_size %u", sp->struct_size);
  for (uint32_t v : {sp->width, sp->height})
    if (v < 1 || v > 8192) return fail(c, PQA_EINVAL, "edge_profiles: plane size %u outside 1 ... 8192", v);
  if (n_frames < 0) return fail(c, PQA_EINVAL, "edge_profiles: negative frame count");
  if (n_frames > 0 && (!ref || !dis)) return fail(c, PQA_EINVAL, "edge_profiles: null clip pointer");
  if (n_frames > 0 && !out) return fail(c, PQA_EINVAL, "edge_profiles: null output pointer");
  return PQA_OK;
}

}  // namespace

extern "C" {

int pqa_frame_sad_device(pqa_ctx* c, const void* const anchor_planes[3], const int64_t anchor_row_pitch[3],
                         const pqa_device_clip* frames, int32_t n_frames, uint64_t* out) {
  if (!c) return PQA_EINVAL;
  if (!anchor_planes || !anchor_row_pitch || !frames || n_frames < 0 || (n_frames > 0 && !out))
    return fail(c, PQA_EINVAL, "bad argument");
  if (!(c->cfg.features & PQA_FEAT_INTEGRITY)) return fail(c, PQA_ESTATE, "pqa_frame_sad_device needs PQA_FEAT_INTEGRITY");
  for (int p = 0; p < c->n_planes; ++p) {
    if (!anchor_planes[p] || !frames->plane[p]) return fail(c, PQA_EINVAL, "plane %d pointer is null", p);
    char who[16];
    snprintf(who, sizeof who, "plane %d ", p);
    const int64_t row_bytes = (int64_t)c->pw[p] * c->esize;
    int rc = check_device_clip(c, who, anchor_row_pitch[p], 0, row_bytes);
    if (rc == PQA_OK) rc = check_device_clip(c, who, frames->row_pitch[p], frames->frame_pitch[p], row_bytes);
    if (rc != PQA_OK) return rc;
  }
  if (c->cancelled.load()) return fail(c, PQA_ECANCELLED, "cancelled");
  HIPCHK(c, hipSetDevice(c->device));
  for (int done = 0; done < n_frames;) {
    const int n = chunk_len(n_frames, done, c->B);
    pqa_device_clip f = *frames;
    for (int p = 0; p < c->n_planes; ++p) f.plane[p] = (const uint8_t*)frames->plane[p] + (int64_t)done * frames->frame_pitch[p];
    const int rc = frame_sad_launch(c, anchor_planes, anchor_row_pitch, &f, n, out + (size_t)done * 3);
    if (rc != PQA_OK) return rc;
    done += n;
  }
  return PQA_OK;
}

int pqa_frame_sad(pqa_ctx* c, const void* const anchor_planes[3], const int64_t anchor_strides[3], const void* const* frames,
                  const int64_t strides[3], int32_t n_frames, uint64_t* out) {
  if (!c) return PQA_EINVAL;
  if (!anchor_planes || !anchor_strides || n_frames < 0 || (n_frames > 0 && (!frames || !strides || !out)))
    return fail(c, PQA_EINVAL, "bad argument");
  if (!(c->cfg.features & PQA_FEAT_INTEGRITY)) return fail(c, PQA_ESTATE, "pqa_frame_sad needs PQA_FEAT_INTEGRITY");
  for (int p = 0; p < c->n_planes; ++p) {
    const int64_t row_bytes = (int64_t)c->pw[p] * c->esize;
    if (!anchor_planes[p]) return fail(c, PQA_EINVAL, "anchor plane %d pointer is null", p);
    if (anchor_strides[p] < row_bytes) return fail(c, PQA_EINVAL, "plane %d stride smaller than a row", p);
    if (n_frames == 0) continue;
    char who[16];
    snprintf(who, sizeof who, "plane %d ", p);
    const int rc = check_host_frames(c, who, "", frames + p, 3, n_frames, strides[p], (size_t)row_bytes, true);
    if (rc != PQA_OK) return rc;
  }
  if (c->cancelled.load()) return fail(c, PQA_ECANCELLED, "cancelled");
  if (n_frames == 0) return PQA_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const int FB = c->B < 8 ? c->B : 8;   // frames per upload and launch
  if (!c->ig_stage) {   // lazily: a healthy clip never asks for an anchored difference
    size_t off = 0;
    for (int p = 0; p < c->n_planes; ++p) {
      c->ig_stage_off[p] = off;
      off += (size_t)round_up(c->ig_hist_pitch[p] * c->ph[p], 256);
    }
    c->ig_stage_bytes = off;
    for (int p = 0; p < c->n_planes; ++p) {
      const int rc = dev_alloc(c, &c->ig_anchor[p], (size_t)c->ig_hist_pitch[p] * c->ph[p]);
      if (rc != PQA_OK) return rc;
    }
    const int rc = dev_alloc(c, &c->ig_stage, off * (size_t)FB);
    if (rc != PQA_OK) return rc;
  }
  // plain synchronous copies from the caller's (pageable) planes: this call is rare and short, it is not pipelined
  for (int p = 0; p < c->n_planes; ++p)
    HIPCHK(c, hipMemcpy2D(c->ig_anchor[p], c->ig_hist_pitch[p], anchor_planes[p], anchor_strides[p], (size_t)c->pw[p] * c->esize,
                          c->ph[p], hipMemcpyHostToDevice));
  const void* anchor[3] = {c->ig_anchor[0], c->ig_anchor[1], c->ig_anchor[2]};
  for (int done = 0; done < n_frames;) {
    if (c->cancelled.load()) return fail(c, PQA_ECANCELLED, "cancelled");
    const int n = chunk_len(n_frames, done, FB);
    pqa_device_clip f{};
    for (int p = 0; p < c->n_planes; ++p) {
      for (int k = 0; k < n; ++k)
        HIPCHK(c, hipMemcpy2D(c->ig_stage + (size_t)k * c->ig_stage_bytes + c->ig_stage_off[p], c->ig_hist_pitch[p],
                              frames[(size_t)(done + k) * 3 + p], strides[p], (size_t)c->pw[p] * c->esize, c->ph[p],
                              hipMemcpyHostToDevice));
      f.plane[p] = c->ig_stage + c->ig_stage_off[p];
      f.row_pitch[p] = c->ig_hist_pitch[p];
      f.frame_pitch[p] = (int64_t)c->ig_stage_bytes;
    }
    const int rc = frame_sad_launch(c, anchor, c->ig_hist_pitch, &f, n, out + (size_t)done * 3);
    if (rc != PQA_OK) return rc;
    done += n;
  }
  return PQA_OK;
}

// ---- luma statistics ---------------------------------------------------------------------------------------------------
// Launches write their results side by side into luma_out (kLumaOutFrames frames); the host copy and the sync happen once
// per kLumaOutFrames frames, not once per launch.

int pqa_set_luma_gray(pqa_ctx* c, uint32_t mode) {
  if (!c) return PQA_EINVAL;
  if (mode != PQA_GRAY_LUMA && mode != PQA_GRAY_BT601_FULL) return fail(c, PQA_EINVAL, "bad gray mode %u", mode);
  c->luma_gray = mode;
  return PQA_OK;
}

int pqa_luma_stats_device(pqa_ctx* c, const void* luma, int64_t row_pitch, int64_t frame_pitch, int32_t n_frames,
                          uint32_t threshold, uint64_t* out) {
  if (!c) return PQA_EINVAL;
  if (!luma || n_frames < 0 || (n_frames > 0 && !out)) return fail(c, PQA_EINVAL, "bad argument");
  const int chk = check_device_clip(c, "", row_pitch, frame_pitch, INT64_MIN);   // this entry has no rule on the row pitch
  if (chk != PQA_OK) return chk;
  if (c->cancelled.load()) return fail(c, PQA_ECANCELLED, "cancelled");
  HIPCHK(c, hipSetDevice(c->device));
  const int gray_bpc = c->luma_gray == PQA_GRAY_BT601_FULL ? (int)c->cfg.bit_depth : 0;
  for (int done = 0; done < n_frames;) {
    const int group = chunk_len(n_frames, done, kLumaOutFrames);
    hipError_t e = hipSuccess;
    for (int g0 = 0; g0 < group && e == hipSuccess;) {
      const int n = chunk_len(group, g0, c->B);
      const PlaneRun run{(const uint8_t*)luma + (int64_t)(done + g0) * frame_pitch, row_pitch / c->esize, frame_pitch / c->esize};
      e = launch_luma_stats(c->stream, c->elem, run, n, c->pw[0], c->ph[0], threshold, gray_bpc, c->luma_part,
                            c->luma_out + (size_t)g0 * 3);
      g0 += n;
    }
    const int rc = side_finish(c, "luma statistics chunk", e, out + (size_t)done * 3, c->luma_out, (size_t)group * 3 * sizeof(uint64_t));
    if (rc != PQA_OK) return rc;
    done += group;
  }
  return PQA_OK;
}

int pqa_luma_stats(pqa_ctx* c, const void* const* luma_frames, int64_t row_stride, int32_t n_frames, uint32_t threshold,
                   uint64_t* out) {
  if (!c) return PQA_EINVAL;
  if (n_frames < 0 || (n_frames > 0 && (!luma_frames || !out))) return fail(c, PQA_EINVAL, "bad argument");
  const size_t row_bytes = (size_t)c->pw[0] * c->esize;
  int rc = check_host_frames(c, "", "", luma_frames, 1, n_frames, row_stride, row_bytes, false);
  if (rc != PQA_OK) return rc;
  if (c->cancelled.load()) return fail(c, PQA_ECANCELLED, "cancelled");
  HIPCHK(c, hipSetDevice(c->device));
  rc = luma_staging_ensure(c);
  if (rc != PQA_OK) return rc;
  const int h = c->ph[0];
  const size_t frame_bytes = (size_t)c->luma_pitch * h;
  const int gray_bpc = c->luma_gray == PQA_GRAY_BT601_FULL ? (int)c->cfg.bit_depth : 0;
  // Chunks of LB frames alternate between the two halves; every chunk's kernel writes its results next to the previous
  // ones in luma_out: no device-to-host copy sits between the chunks (into the caller's pageable `out` it would block the
  // host until the kernel in front of it is done, and the next chunk could not be packed under that kernel).
  int hf = 0;
  for (int done = 0; done < n_frames;) {
    const int group = chunk_len(n_frames, done, kLumaOutFrames);
    hipError_t e = hipSuccess;
    for (int g0 = 0; g0 < group && e == hipSuccess && !c->cancelled.load(); hf ^= 1) {
      const int n = chunk_len(group, g0, c->LB);
      e = stage_frames(c, hf, luma_frames + done + g0, row_stride, n, row_bytes, h);
      if (e == hipSuccess) {
        const PlaneRun run{c->luma_half[hf].dev, c->luma_pitch / c->esize, (int64_t)(frame_bytes / c->esize)};
        e = launch_luma_stats(c->stream, c->elem, run, n, c->pw[0], h, threshold, gray_bpc, c->luma_part,
                              c->luma_out + (size_t)g0 * 3);
      }
      g0 += n;
    }
    rc = side_finish(c, "luma statistics chunk", e, out + (size_t)done * 3, c->luma_out, (size_t)group * 3 * sizeof(uint64_t));
    if (rc != PQA_OK) return rc;
    done += group;
  }
  return PQA_OK;
}

// ---- temporal alignment (cross_sse.hip) --------------------------------------------------------------------------------

int pqa_cross_sse_device(pqa_ctx* c, const void* ref_luma, int64_t ref_row_pitch, int64_t ref_frame_pitch, int32_t n_ref,
                         const void* dis_luma, int64_t dis_row_pitch, int64_t dis_frame_pitch, int32_t n_dis, int32_t k_lo,
                         int32_t k_hi, uint64_t* out) {
  int rc = xs_check(c, ref_luma, dis_luma, n_ref, n_dis, k_lo, k_hi, out);
  if (rc != PQA_OK) return rc;
  const int es = c->esize;
  const int64_t row_bytes = (int64_t)c->pw[0] * es;
  rc = check_device_clip(c, "cross_sse: ", ref_row_pitch, ref_frame_pitch, row_bytes);
  if (rc == PQA_OK) rc = check_device_clip(c, "cross_sse: ", dis_row_pitch, dis_frame_pitch, row_bytes);
  if (rc != PQA_OK) return rc;
  if (c->cancelled.load()) return fail(c, PQA_ECANCELLED, "cancelled");
  if (n_ref == 0) return PQA_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const int span = k_hi - k_lo + 1;
  const bool mfma = c->xsse_mfma && c->elem == ELEM_U8;
  const int n_tiles = (n_ref + 31) / 32;
  const int per_launch = n_tiles < kXsTilesPerLaunch ? n_tiles : kXsTilesPerLaunch;
  rc = xs_prepare(c, mfma, span, per_launch, n_ref, n_dis);
  if (rc != PQA_OK) return rc;
  const XsseClip ref{ref_luma, ref_row_pitch / es, ref_frame_pitch / es, INT32_MAX, n_ref};
  const XsseClip dis{dis_luma, dis_row_pitch / es, dis_frame_pitch / es, INT32_MAX, n_dis};
  auto* nr = (unsigned long long*)c->side_buf[SIDE_XSSE_NORM_REF];
  auto* nd = (unsigned long long*)c->side_buf[SIDE_XSSE_NORM_DIS];
  auto* dev_out = (unsigned long long*)c->side_buf[SIDE_XSSE_OUT];
  hipError_t e = hipSuccess;
  if (mfma) {
    e = launch_xsse_norms(c->stream, ref, 0, n_ref, c->pw[0], c->ph[0], nr);
    if (e == hipSuccess) e = launch_xsse_norms(c->stream, dis, 0, n_dis, c->pw[0], c->ph[0], nd);
  }
  for (int t0 = 0; t0 < n_tiles && e == hipSuccess; t0 += per_launch)
    e = launch_cross_sse(c->stream, c->elem, mfma, ref, dis, c->pw[0], c->ph[0], k_lo, span, t0, chunk_len(n_tiles, t0, per_launch),
                         c->side_buf[SIDE_XSSE_PART], nr, nd, dev_out);
  return side_finish(c, "cross_sse", e, out, dev_out, (size_t)n_ref * span * sizeof(uint64_t));
}

int pqa_cross_sse(pqa_ctx* c, const void* const* ref_frames, int64_t ref_row_stride, int32_t n_ref,
                  const void* const* dis_frames, int64_t dis_row_stride, int32_t n_dis, int32_t k_lo, int32_t k_hi,
                  uint64_t* out) {
  int rc = xs_check(c, ref_frames, dis_frames, n_ref, n_dis, k_lo, k_hi, out);
  if (rc != PQA_OK) return rc;
  const size_t row_bytes = (size_t)c->pw[0] * c->esize;
  rc = check_host_frames(c, "cross_sse: ", "reference ", ref_frames, 1, n_ref, ref_row_stride, row_bytes, false);
  if (rc == PQA_OK) rc = check_host_frames(c, "cross_sse: ", "captured ", dis_frames, 1, n_dis, dis_row_stride, row_bytes, false);
  if (rc != PQA_OK) return rc;
  if (c->cancelled.load()) return fail(c, PQA_ECANCELLED, "cancelled");
  if (n_ref == 0) return PQA_OK;
  HIPCHK(c, hipSetDevice(c->device));
  rc = luma_staging_ensure(c);
  if (rc != PQA_OK) return rc;
  const int span = k_hi - k_lo + 1, h = c->ph[0], es = c->esize;
  const bool mfma = c->xsse_mfma && c->elem == ELEM_U8;
  rc = xs_prepare(c, mfma, span, 1, n_ref, n_dis);
  const size_t frame_bytes = (size_t)c->luma_pitch * h;
  const int dis_ring = 31 + span;   // the captured frames one reference tile meets
  if (rc == PQA_OK) rc = side_reserve(c, SIDE_XSSE_REF, frame_bytes * 32);
  if (rc == PQA_OK) rc = side_reserve(c, SIDE_XSSE_DIS, frame_bytes * dis_ring);
  if (rc != PQA_OK) return rc;
  const XsseClip ref{c->side_buf[SIDE_XSSE_REF], c->luma_pitch / es, (int64_t)(frame_bytes / es), 32, n_ref};
  const XsseClip dis{c->side_buf[SIDE_XSSE_DIS], c->luma_pitch / es, (int64_t)(frame_bytes / es), dis_ring, n_dis};
  auto* nr = (unsigned long long*)c->side_buf[SIDE_XSSE_NORM_REF];
  auto* nd = (unsigned long long*)c->side_buf[SIDE_XSSE_NORM_DIS];
  auto* dev_out = (unsigned long long*)c->side_buf[SIDE_XSSE_OUT];
  // Every frame crosses PCIe once: reference tile b replaces tile b - 1 in its 32 slots, and the captured window only ever
  // moves forward, so a tile uploads the captured frames between the previous window's end and its own.  Frames travel in
  // chunks of LB that alternate between the two pinned halves, as in pqa_luma_stats; the stream orders a tile's uploads
  // before its kernels and those before the next tile's uploads into the same slots.
  hipError_t e = hipSuccess;
  int hf = 0;
  const auto live = [&] { return e == hipSuccess && !c->cancelled.load(); };
  const auto upload = [&](const void* const* frames, int64_t stride, const XsseClip& clip, int64_t first, int64_t last,
                          unsigned long long* norms) {   // frames first ... last - 1 into their ring slots
    for (int64_t f0 = first; f0 < last && live(); hf ^= 1) {
      const int n = (int)(last - f0 < c->LB ? last - f0 : c->LB);
      e = stage_frames(c, hf, frames + f0, stride, n, row_bytes, h, (uint8_t*)clip.base, clip.ring, f0);
      // the frames of a chunk lie in consecutive slots unless the ring wraps inside it: one norm launch per frame
      for (int f = 0; mfma && f < n && e == hipSuccess; ++f) e = launch_xsse_norms(c->stream, clip, f0 + f, 1, c->pw[0], h, norms);
      f0 += n;
    }
  };
  int64_t dis_done = 0;   // captured frames below it have been uploaded (or skipped: no reference tile meets them)
  const int n_tiles = (n_ref + 31) / 32;
  for (int t = 0; t < n_tiles && live(); ++t) {
    const int64_t r0 = (int64_t)t * 32, r1 = r0 + 32 < n_ref ? r0 + 32 : n_ref;
    int64_t d0 = r0 + k_lo, d1 = r0 + 31 + k_hi + 1;
    d0 = d0 < dis_done ? dis_done : d0;
    d1 = d1 > n_dis ? n_dis : d1;
    upload(ref_frames, ref_row_stride, ref, r0, r1, nr);
    if (d0 < d1) {
      upload(dis_frames, dis_row_stride, dis, d0, d1, nd);
      dis_done = d1;
    }
    if (live())
      e = launch_cross_sse(c->stream, c->elem, mfma, ref, dis, c->pw[0], h, k_lo, span, t, 1, c->side_buf[SIDE_XSSE_PART], nr, nd,
                           dev_out);
  }
  return side_finish(c, "cross_sse", e, out, dev_out, (size_t)n_ref * span * sizeof(uint64_t));
}

// ---- spatial alignment (shift_sse.hip) ---------------------------------------------------------------------------------

int pqa_shift_sse_device(pqa_ctx* c, const void* ref_luma, int64_t ref_row_pitch, int64_t ref_frame_pitch, const void* dis_luma,
                         int64_t dis_row_pitch, int64_t dis_frame_pitch, int32_t n_frames, int32_t radius, uint64_t* out) {
  int rc = sh_check(c, ref_luma, dis_luma, n_frames, radius, out);
  if (rc != PQA_OK) return rc;
  if (n_frames == 0) return PQA_OK;
  const int es = c->esize;
  const int64_t row_bytes = (int64_t)c->pw[0] * es;
  rc = check_device_clip(c, "shift_sse: ", ref_row_pitch, ref_frame_pitch, row_bytes);
  if (rc == PQA_OK) rc = check_device_clip(c, "shift_sse: ", dis_row_pitch, dis_frame_pitch, row_bytes);
  if (rc != PQA_OK) return rc;
  if (c->cancelled.load()) return fail(c, PQA_ECANCELLED, "cancelled");
  HIPCHK(c, hipSetDevice(c->device));
  rc = sh_prepare(c, radius, n_frames);
  if (rc != PQA_OK) return rc;
  const size_t n = (size_t)(2 * radius + 1) * (2 * radius + 1);
  auto* dev_out = (unsigned long long*)c->side_buf[SIDE_SHIFT_OUT];
  hipError_t e = hipSuccess;
  for (int f0 = 0; f0 < n_frames && e == hipSuccess; f0 += kShiftChunk)
    e = launch_shift_sse(c->stream, c->elem, (const uint8_t*)ref_luma + (int64_t)f0 * ref_frame_pitch, ref_row_pitch / es,
                         ref_frame_pitch / es, (const uint8_t*)dis_luma + (int64_t)f0 * dis_frame_pitch, dis_row_pitch / es,
                         dis_frame_pitch / es, chunk_len(n_frames, f0, kShiftChunk), c->pw[0], c->ph[0], radius,
                         c->side_buf[SIDE_SHIFT_PART], (unsigned long long*)c->side_buf[SIDE_SHIFT_ROWSQ], dev_out + (size_t)f0 * n);
  return side_finish(c, "shift_sse", e, out, dev_out, (size_t)n_frames * n * sizeof(uint64_t));
}

int pqa_shift_sse(pqa_ctx* c, const void* const* ref_frames, int64_t ref_row_stride, const void* const* dis_frames,
                  int64_t dis_row_stride, int32_t n_frames, int32_t radius, uint64_t* out) {
  int rc = sh_check(c, ref_frames, dis_frames, n_frames, radius, out);
  if (rc != PQA_OK) return rc;
  if (n_frames == 0) return PQA_OK;
  const size_t row_bytes = (size_t)c->pw[0] * c->esize;
  rc = check_host_frames(c, "shift_sse: ", "", ref_frames, 1, n_frames, ref_row_stride, row_bytes, false);
  if (rc == PQA_OK) rc = check_host_frames(c, "shift_sse: ", "", dis_frames, 1, n_frames, dis_row_stride, row_bytes, false);
  if (rc != PQA_OK) return rc;
  if (c->cancelled.load()) return fail(c, PQA_ECANCELLED, "cancelled");
  HIPCHK(c, hipSetDevice(c->device));
  rc = luma_staging_ensure(c);
  if (rc == PQA_OK) rc = sh_prepare(c, radius, n_frames);   // LB <= kShiftChunk: the workspaces of a full chunk hold every chunk here
  if (rc != PQA_OK) return rc;
  const int h = c->ph[0], es = c->esize;
  const size_t frame_bytes = (size_t)c->luma_pitch * h, n = (size_t)(2 * radius + 1) * (2 * radius + 1);
  auto* dev_out = (unsigned long long*)c->side_buf[SIDE_SHIFT_OUT];
  hipError_t e = hipSuccess;
  // Chunks of LB (<= 8) pairs: the reference frames go through pinned / device half 0, the captured ones through half 1.
  // The stream orders a chunk's kernel before the next chunk's uploads into the same device halves.
  for (int f0 = 0; f0 < n_frames && e == hipSuccess && !c->cancelled.load(); f0 += c->LB) {
    const int m = chunk_len(n_frames, f0, c->LB);
    e = stage_frames(c, 0, ref_frames + f0, ref_row_stride, m, row_bytes, h);
    if (e == hipSuccess) e = stage_frames(c, 1, dis_frames + f0, dis_row_stride, m, row_bytes, h);
    if (e == hipSuccess)
      e = launch_shift_sse(c->stream, c->elem, c->luma_half[0].dev, c->luma_pitch / es, (int64_t)(frame_bytes / es),
                           c->luma_half[1].dev, c->luma_pitch / es, (int64_t)(frame_bytes / es), m, c->pw[0], h, radius,
                           c->side_buf[SIDE_SHIFT_PART], (unsigned long long*)c->side_buf[SIDE_SHIFT_ROWSQ], dev_out + (size_t)f0 * n);
  }
  return side_finish(c, "shift_sse", e, out, dev_out, (size_t)n_frames * n * sizeof(uint64_t));
}

// ---- level alignment (level_stats.hip) ---------------------------------------------------------------------------------

int pqa_level_bins(const pqa_ctx* c) { return c ? 1 << c->cfg.bit_depth : PQA_EINVAL; }

int pqa_level_stats_device(pqa_ctx* c, const void* ref, int64_t ref_row_pitch, int64_t ref_frame_pitch, const void* dis,
                           int64_t dis_row_pitch, int64_t dis_frame_pitch, int32_t n_frames, int32_t plane, uint64_t* out) {
  int rc = lv_check(c, ref, dis, n_frames, plane, out);
  if (rc != PQA_OK) return rc;
  if (n_frames == 0) return PQA_OK;
  const int es = c->esize, bpc = (int)c->cfg.bit_depth;
  const int64_t row_bytes = (int64_t)c->pw[plane] * es;
  rc = check_device_clip(c, "level_stats: ", ref_row_pitch, ref_frame_pitch, row_bytes);
  if (rc == PQA_OK) rc = check_device_clip(c, "level_stats: ", dis_row_pitch, dis_frame_pitch, row_bytes);
  if (rc != PQA_OK) return rc;
  if (c->cancelled.load()) return fail(c, PQA_ECANCELLED, "cancelled");
  HIPCHK(c, hipSetDevice(c->device));
  rc = side_reserve(c, SIDE_LEVEL_OUT, level_out_bytes(bpc, n_frames));
  if (rc != PQA_OK) return rc;
  const size_t n = (size_t)3 << bpc;
  auto* dev_out = (unsigned long long*)c->side_buf[SIDE_LEVEL_OUT];
  hipError_t e = hipSuccess;
  for (int f0 = 0; f0 < n_frames && e == hipSuccess; f0 += kLevelChunk)
    e = launch_level_stats(c->stream, c->elem, bpc, (const uint8_t*)ref + (int64_t)f0 * ref_frame_pitch, ref_row_pitch / es,
                           ref_frame_pitch / es, (const uint8_t*)dis + (int64_t)f0 * dis_frame_pitch, dis_row_pitch / es,
                           dis_frame_pitch / es, chunk_len(n_frames, f0, kLevelChunk), c->pw[plane], c->ph[plane],
                           dev_out + (size_t)f0 * n);
  return side_finish(c, "level_stats", e, out, dev_out, (size_t)n_frames * n * sizeof(uint64_t));
}

int pqa_level_stats(pqa_ctx* c, const void* const* ref_frames, int64_t ref_row_stride, const void* const* dis_frames,
                    int64_t dis_row_stride, int32_t n_frames, int32_t plane, uint64_t* out) {
  int rc = lv_check(c, ref_frames, dis_frames, n_frames, plane, out);
  if (rc != PQA_OK) return rc;
  if (n_frames == 0) return PQA_OK;
  const size_t row_bytes = (size_t)c->pw[plane] * c->esize;
  rc = check_host_frames(c, "level_stats: ", "", ref_frames, 1, n_frames, ref_row_stride, row_bytes, true);
  if (rc == PQA_OK) rc = check_host_frames(c, "level_stats: ", "", dis_frames, 1, n_frames, dis_row_stride, row_bytes, true);
  if (rc != PQA_OK) return rc;
  if (c->cancelled.load()) return fail(c, PQA_ECANCELLED, "cancelled");
  HIPCHK(c, hipSetDevice(c->device));
  const int bpc = (int)c->cfg.bit_depth;
  rc = luma_staging_ensure(c);
  if (rc == PQA_OK) rc = side_reserve(c, SIDE_LEVEL_OUT, level_out_bytes(bpc, n_frames));
  if (rc != PQA_OK) return rc;
  // a chroma plane is no larger than the luma plane, so it travels through the luma staging with the luma pitches
  const int w = c->pw[plane], h = c->ph[plane], es = c->esize;
  const size_t frame_bytes = (size_t)c->luma_pitch * c->ph[0], n = (size_t)3 << bpc;
  auto* dev_out = (unsigned long long*)c->side_buf[SIDE_LEVEL_OUT];
  hipError_t e = hipSuccess;
  // chunks of LB (<= kLevelChunk) pairs, staged as in pqa_shift_sse: reference frames through half 0, captured ones through half 1
  for (int f0 = 0; f0 < n_frames && e == hipSuccess && !c->cancelled.load(); f0 += c->LB) {
    const int m = chunk_len(n_frames, f0, c->LB);
    e = stage_frames(c, 0, ref_frames + f0, ref_row_stride, m, row_bytes, h);
    if (e == hipSuccess) e = stage_frames(c, 1, dis_frames + f0, dis_row_stride, m, row_bytes, h);
    if (e == hipSuccess)
      e = launch_level_stats(c->stream, c->elem, bpc, c->luma_half[0].dev, c->luma_pitch / es, (int64_t)(frame_bytes / es),
                             c->luma_half[1].dev, c->luma_pitch / es, (int64_t)(frame_bytes / es), m, w, h, dev_out + (size_t)f0 * n);
  }
  return side_finish(c, "level_stats", e, out, dev_out, (size_t)n_frames * n * sizeof(uint64_t));
}

// ---- resampler (resample.hip) ------------------------------------------------------------------------------------------

int pqa_resample_device(pqa_ctx* c, const pqa_resample_spec* spec, const void* src, int64_t src_row_pitch, int64_t src_frame_pitch,
                        void* dst, int64_t dst_row_pitch, int64_t dst_frame_pitch, int32_t n_frames) {
  int rc = rs_check(c, spec);
  if (rc != PQA_OK) return rc;
  if (n_frames < 0) return fail(c, PQA_EINVAL, "resample: negative frame count");
  if (n_frames > 0 && (!src || !dst)) return fail(c, PQA_EINVAL, "resample: null plane pointer");
  const int es = c->esize;
  rc = check_device_clip(c, "resample: source ", src_row_pitch, src_frame_pitch, (int64_t)spec->src_width * es);
  if (rc == PQA_OK) rc = check_device_clip(c, "resample: destination ", dst_row_pitch, dst_frame_pitch, (int64_t)spec->dst_width * es);
  if (rc != PQA_OK) return rc;
  int slot = 0;
  rc = rs_tables(c, spec, &slot);   // more than 32 taps: refused before any device call
  if (rc != PQA_OK) return rc;
  if (c->cancelled.load()) return fail(c, PQA_ECANCELLED, "cancelled");
  if (n_frames == 0) return PQA_OK;
  HIPCHK(c, hipSetDevice(c->device));
  hipError_t e = hipSuccess;
  for (int f0 = 0; f0 < n_frames && e == hipSuccess; f0 += kRsChunk)
    e = launch_resample(c->stream, c->elem, (int)c->cfg.bit_depth, c->rs_cache[slot].plan, (const int*)c->side_buf[SIDE_RS_TABLE0 + slot],
                        (const uint8_t*)src + (int64_t)f0 * src_frame_pitch, src_row_pitch / es, src_frame_pitch / es,
                        (int)spec->src_width, (int)spec->src_height, (uint8_t*)dst + (int64_t)f0 * dst_frame_pitch, dst_row_pitch / es,
                        dst_frame_pitch / es, (int)spec->dst_width, (int)spec->dst_height, chunk_len(n_frames, f0, kRsChunk));
  return side_finish(c, "resample", e, nullptr, nullptr, 0);
}

int pqa_resample(pqa_ctx* c, const pqa_resample_spec* spec, const void* const* src_frames, int64_t src_row_stride,
                 void* const* dst_frames, int64_t dst_row_stride, int32_t n_frames) {
  int rc = rs_check(c, spec);
  if (rc != PQA_OK) return rc;
  if (n_frames < 0) return fail(c, PQA_EINVAL, "resample: negative frame count");
  if (n_frames > 0 && (!src_frames || !dst_frames)) return fail(c, PQA_EINVAL, "resample: null frame list");
  const int es = c->esize;
  const int sw = (int)spec->src_width, sh = (int)spec->src_height, dw = (int)spec->dst_width, dh = (int)spec->dst_height;
  const size_t src_row = (size_t)sw * es, dst_row = (size_t)dw * es;
  rc = check_host_frames(c, "resample: ", "source ", src_frames, 1, n_frames, src_row_stride, src_row, true);
  if (rc == PQA_OK) rc = check_host_frames(c, "resample: ", "destination ", (const void* const*)dst_frames, 1, n_frames, dst_row_stride, dst_row, true);
  if (rc != PQA_OK) return rc;
  int slot = 0;
  rc = rs_tables(c, spec, &slot);   // more than 32 taps: refused before any device call
  if (rc != PQA_OK) return rc;
  if (c->cancelled.load()) return fail(c, PQA_ECANCELLED, "cancelled");
  if (n_frames == 0) return PQA_OK;
  HIPCHK(c, hipSetDevice(c->device));
  // A source plane may be larger than the context's: the chunks of kRsChunk planes travel through pinned buffers and device
  // buffers of this entry's own, all grow-only.  Rows are packed 16 bytes apart at least, so the kernel loads and stores
  // four samples at a time.  A chunk is uploaded, resampled, downloaded and copied out before the next one starts.
  const int64_t sp = round_up((int64_t)src_row, 16), dp = round_up((int64_t)dst_row, 16);
  const size_t sf = (size_t)sp * sh, df = (size_t)dp * dh;
  const int chunk = n_frames < kRsChunk ? n_frames : kRsChunk;
  rc = rs_pin_reserve(c, 0, sf * chunk);
  if (rc == PQA_OK) rc = rs_pin_reserve(c, 1, df * chunk);
  if (rc == PQA_OK) rc = side_reserve(c, SIDE_RS_SRC, sf * chunk);
  if (rc == PQA_OK) rc = side_reserve(c, SIDE_RS_DST, df * chunk);
  if (rc != PQA_OK) return rc;
  for (int f0 = 0; f0 < n_frames; f0 += kRsChunk) {
    const int n = chunk_len(n_frames, f0, kRsChunk);
    for (int f = 0; f < n; ++f) copy_plane_rows(c->rs_pin[0] + (size_t)f * sf, sp, (const uint8_t*)src_frames[f0 + f], src_row_stride, src_row, sh);
    hipError_t e = hipMemcpyAsync(c->side_buf[SIDE_RS_SRC], c->rs_pin[0], sf * n, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess)
      e = launch_resample(c->stream, c->elem, (int)c->cfg.bit_depth, c->rs_cache[slot].plan, (const int*)c->side_buf[SIDE_RS_TABLE0 + slot],
                          c->side_buf[SIDE_RS_SRC], sp / es, (int64_t)(sf / es), sw, sh, c->side_buf[SIDE_RS_DST], dp / es,
                          (int64_t)(df / es), dw, dh, n);
    rc = side_finish(c, "resample", e, c->rs_pin[1], c->side_buf[SIDE_RS_DST], df * n);
    if (rc != PQA_OK) return rc;
    for (int f = 0; f < n; ++f)   // row by row: the bytes between a destination row's end and the next row stay as they are
      for (int y = 0; y < dh; ++y)
        memcpy((uint8_t*)dst_frames[f0 + f] + (int64_t)y * dst_row_stride, c->rs_pin[1] + (size_t)f * df + (size_t)y * dp, dst_row);
  }
  return PQA_OK;
}

// ---- registration moments (flow_moments.hip) ---------------------------------------------------------------------------

int pqa_flow_moments_device(pqa_ctx* c, const pqa_flow_spec* spec, const void* ref, int64_t ref_row_pitch, int64_t ref_frame_pitch,
                            const void* dis, int64_t dis_row_pitch, int64_t dis_frame_pitch, int32_t n_frames, int64_t* out) {
  int rc = fl_check(c, spec, ref, dis, n_frames, out);
  if (rc != PQA_OK) return rc;
  const int es = c->esize, w = (int)spec->width, h = (int)spec->height, tile = (int)spec->tile;
  rc = check_device_clip(c, "flow_moments: reference ", ref_row_pitch, ref_frame_pitch, (int64_t)w * es);
  if (rc == PQA_OK) rc = check_device_clip(c, "flow_moments: captured ", dis_row_pitch, dis_frame_pitch, (int64_t)w * es);
  if (rc != PQA_OK) return rc;
  if (c->cancelled.load()) return fail(c, PQA_ECANCELLED, "cancelled");
  if (n_frames == 0) return PQA_OK;
  HIPCHK(c, hipSetDevice(c->device));
  rc = side_reserve(c, SIDE_FLOW_OUT, flow_out_bytes(w, h, tile, n_frames));
  if (rc != PQA_OK) return rc;
  const size_t per_frame = flow_out_bytes(w, h, tile, 1) / sizeof(long long);
  auto* dev_out = (long long*)c->side_buf[SIDE_FLOW_OUT];
  hipError_t e = hipSuccess;
  for (int f0 = 0; f0 < n_frames && e == hipSuccess; f0 += kFlowChunk)
    e = launch_flow_moments(c->stream, c->elem, (int)c->cfg.bit_depth, (const uint8_t*)ref + (int64_t)f0 * ref_frame_pitch,
                            ref_row_pitch / es, ref_frame_pitch / es, (const uint8_t*)dis + (int64_t)f0 * dis_frame_pitch,
                            dis_row_pitch / es, dis_frame_pitch / es, chunk_len(n_frames, f0, kFlowChunk), w, h, tile,
                            dev_out + (size_t)f0 * per_frame);
  return side_finish(c, "flow_moments", e, out, dev_out, flow_out_bytes(w, h, tile, n_frames));
}

int pqa_flow_moments(pqa_ctx* c, const pqa_flow_spec* spec, const void* const* ref_frames, int64_t ref_row_stride,
                     const void* const* dis_frames, int64_t dis_row_stride, int32_t n_frames, int64_t* out) {
  int rc = fl_check(c, spec, ref_frames, dis_frames, n_frames, out);
  if (rc != PQA_OK) return rc;
  const int es = c->esize, w = (int)spec->width, h = (int)spec->height, tile = (int)spec->tile;
  const size_t row_bytes = (size_t)w * es;
  rc = check_host_frames(c, "flow_moments: ", "reference ", ref_frames, 1, n_frames, ref_row_stride, row_bytes, true);
  if (rc == PQA_OK) rc = check_host_frames(c, "flow_moments: ", "captured ", dis_frames, 1, n_frames, dis_row_stride, row_bytes, true);
  if (rc != PQA_OK) return rc;
  if (c->cancelled.load()) return fail(c, PQA_ECANCELLED, "cancelled");
  if (n_frames == 0) return PQA_OK;
  HIPCHK(c, hipSetDevice(c->device));
  // The planes are the call's own size, so they travel as pqa_resample's do: chunks of kFlowChunk pairs through its two
  // grow-only pinned buffers (the reference planes through the first, the captured ones through the second) into device
  // buffers of this entry.  Every chunk's kernel writes its sums behind the previous chunk's; they come back once.  A pinned
  // buffer is packed again only after the stream has drained the chunk before: the entry is short, it is not pipelined.
  const int64_t pitch = round_up((int64_t)row_bytes, 16);
  const size_t fb = (size_t)pitch * h;
  const int chunk = n_frames < kFlowChunk ? n_frames : kFlowChunk;
  rc = rs_pin_reserve(c, 0, fb * chunk);
  if (rc == PQA_OK) rc = rs_pin_reserve(c, 1, fb * chunk);
  if (rc == PQA_OK) rc = side_reserve(c, SIDE_FLOW_REF, fb * chunk);
  if (rc == PQA_OK) rc = side_reserve(c, SIDE_FLOW_DIS, fb * chunk);
  if (rc == PQA_OK) rc = side_reserve(c, SIDE_FLOW_OUT, flow_out_bytes(w, h, tile, n_frames));
  if (rc != PQA_OK) return rc;
  const size_t per_frame = flow_out_bytes(w, h, tile, 1) / sizeof(long long);
  auto* dev_out = (long long*)c->side_buf[SIDE_FLOW_OUT];
  hipError_t e = hipSuccess;
  for (int f0 = 0; f0 < n_frames && e == hipSuccess && !c->cancelled.load(); f0 += kFlowChunk) {
    const int n = chunk_len(n_frames, f0, kFlowChunk);
    if (f0 > 0) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) break;
    for (int f = 0; f < n; ++f) {
      copy_plane_rows(c->rs_pin[0] + (size_t)f * fb, pitch, (const uint8_t*)ref_frames[f0 + f], ref_row_stride, row_bytes, h);
      copy_plane_rows(c->rs_pin[1] + (size_t)f * fb, pitch, (const uint8_t*)dis_frames[f0 + f], dis_row_stride, row_bytes, h);
    }
    e = hipMemcpyAsync(c->side_buf[SIDE_FLOW_REF], c->rs_pin[0], fb * n, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(c->side_buf[SIDE_FLOW_DIS], c->rs_pin[1], fb * n, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess)
      e = launch_flow_moments(c->stream, c->elem, (int)c->cfg.bit_depth, c->side_buf[SIDE_FLOW_REF], pitch / es, (int64_t)(fb / es),
                              c->side_buf[SIDE_FLOW_DIS], pitch / es, (int64_t)(fb / es), n, w, h, tile, dev_out + (size_t)f0 * per_frame);
  }
  return side_finish(c, "flow_moments", e, out, dev_out, flow_out_bytes(w, h, tile, n_frames));
}

// ---- distortion map (tile_moments.hip) -------------------------------------------------------------------------------------

int pqa_tile_moments_device(pqa_ctx* c, const pqa_tile_spec* spec, const void* ref, int64_t ref_row_pitch, int64_t ref_frame_pitch,
                            const void* dis, int64_t dis_row_pitch, int64_t dis_frame_pitch, int32_t n_frames, uint64_t* out) {
  int rc = tl_check(c, spec, ref, dis, n_frames, out);
  if (rc != PQA_OK) return rc;
  const int es = c->esize, w = (int)spec->width, h = (int)spec->height, tile = (int)spec->tile;
  rc = check_device_clip(c, "tile_moments: reference ", ref_row_pitch, ref_frame_pitch, (int64_t)w * es);
  if (rc == PQA_OK) rc = check_device_clip(c, "tile_moments: captured ", dis_row_pitch, dis_frame_pitch, (int64_t)w * es);
  if (rc != PQA_OK) return rc;
  if (c->cancelled.load()) return fail(c, PQA_ECANCELLED, "cancelled");
  if (n_frames == 0) return PQA_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t bytes = tile_out_bytes(w, h, tile, n_frames), per_frame = tile_out_bytes(w, h, tile, 1) / sizeof(uint64_t);
  rc = side_reserve(c, SIDE_TILE_OUT, bytes);
  if (rc != PQA_OK) return rc;
  auto* dev_out = (unsigned long long*)c->side_buf[SIDE_TILE_OUT];
  hipError_t e = hipSuccess;
  for (int f0 = 0; f0 < n_frames && e == hipSuccess; f0 += kTileChunk)
    e = launch_tile_moments(c->stream, c->elem, (int)c->cfg.bit_depth, (const uint8_t*)ref + (int64_t)f0 * ref_frame_pitch,
                            ref_row_pitch / es, ref_frame_pitch / es, (const uint8_t*)dis + (int64_t)f0 * dis_frame_pitch,
                            dis_row_pitch / es, dis_frame_pitch / es, chunk_len(n_frames, f0, kTileChunk), w, h, tile,
                            dev_out + (size_t)f0 * per_frame);
  return side_finish(c, "tile_moments", e, out, dev_out, bytes);
}

int pqa_tile_moments(pqa_ctx* c, const pqa_tile_spec* spec, const void* const* ref_frames, int64_t ref_row_stride,
                     const void* const* dis_frames, int64_t dis_row_stride, int32_t n_frames, uint64_t* out) {
  int rc = tl_check(c, spec, ref_frames, dis_frames, n_frames, out);
  if (rc != PQA_OK) return rc;
  const int es = c->esize, w = (int)spec->width, h = (int)spec->height, tile = (int)spec->tile;
  const size_t row_bytes = (size_t)w * es;
  rc = check_host_frames(c, "tile_moments: ", "reference ", ref_frames, 1, n_frames, ref_row_stride, row_bytes, true);
  if (rc == PQA_OK) rc = check_host_frames(c, "tile_moments: ", "captured ", dis_frames, 1, n_frames, dis_row_stride, row_bytes, true);
  if (rc != PQA_OK) return rc;
  if (n_frames > 0 && (ref_row_stride % es || dis_row_stride % es))
    return fail(c, PQA_EINVAL, "tile_moments: stride is not a multiple of the sample size");
  if (c->cancelled.load()) return fail(c, PQA_ECANCELLED, "cancelled");
  if (n_frames == 0) return PQA_OK;
  HIPCHK(c, hipSetDevice(c->device));
  // The planes travel exactly as pqa_flow_moments' do, through the same buffers: chunks of kTileChunk pairs through the two
  // grow-only pinned buffers of pqa_resample into the two device buffers of pqa_flow_moments (every entry here is synchronous,
  // so no two of them are ever in flight), rows 16 bytes apart at least, so the kernel takes its wide loads.  Every chunk's
  // kernel writes its sums behind the previous chunk's; they come back once.  A pinned buffer is packed again only after the
  // stream has drained the chunk before.
  const int64_t pitch = round_up((int64_t)row_bytes, 16);
  const size_t fb = (size_t)pitch * h;
  const int chunk = n_frames < kTileChunk ? n_frames : kTileChunk;
  const size_t bytes = tile_out_bytes(w, h, tile, n_frames), per_frame = tile_out_bytes(w, h, tile, 1) / sizeof(uint64_t);
  rc = rs_pin_reserve(c, 0, fb * chunk);
  if (rc == PQA_OK) rc = rs_pin_reserve(c, 1, fb * chunk);
  if (rc == PQA_OK) rc = side_reserve(c, SIDE_FLOW_REF, fb * chunk);
  if (rc == PQA_OK) rc = side_reserve(c, SIDE_FLOW_DIS, fb * chunk);
  if (rc == PQA_OK) rc = side_reserve(c, SIDE_TILE_OUT, bytes);
  if (rc != PQA_OK) return rc;
  auto* dev_out = (unsigned long long*)c->side_buf[SIDE_TILE_OUT];
  hipError_t e = hipSuccess;
  for (int f0 = 0; f0 < n_frames && e == hipSuccess && !c->cancelled.load(); f0 += kTileChunk) {
    const int n = chunk_len(n_frames, f0, kTileChunk);
    if (f0 > 0) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) break;
    for (int f = 0; f < n; ++f) {
      copy_plane_rows(c->rs_pin[0] + (size_t)f * fb, pitch, (const uint8_t*)ref_frames[f0 + f], ref_row_stride, row_bytes, h);
      copy_plane_rows(c->rs_pin[1] + (size_t)f * fb, pitch, (const uint8_t*)dis_frames[f0 + f], dis_row_stride, row_bytes, h);
    }
    e = hipMemcpyAsync(c->side_buf[SIDE_FLOW_REF], c->rs_pin[0], fb * n, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(c->side_buf[SIDE_FLOW_DIS], c->rs_pin[1], fb * n, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess)
      e = launch_tile_moments(c->stream, c->elem, (int)c->cfg.bit_depth, c->side_buf[SIDE_FLOW_REF], pitch / es, (int64_t)(fb / es),
                              c->side_buf[SIDE_FLOW_DIS], pitch / es, (int64_t)(fb / es), n, w, h, tile, dev_out + (size_t)f0 * per_frame);
  }
  return side_finish(c, "tile_moments", e, out, dev_out, bytes);
}

// ---- distortion spectrum (band_moments.hip) --------------------------------------------------------------------------------

int pqa_band_sums(void) { return kBandSums; }

int pqa_band_moments_device(pqa_ctx* c, const pqa_band_spec* spec, const void* ref, int64_t ref_row_pitch, int64_t ref_frame_pitch,
                            const void* dis, int64_t dis_row_pitch, int64_t dis_frame_pitch, int32_t n_frames, uint64_t* out) {
  int rc = bd_check(c, spec, ref, dis, n_frames, out);
  if (rc != PQA_OK) return rc;
  const int es = c->esize, w = (int)spec->width, h = (int)spec->height, levels = (int)spec->levels;
  rc = check_device_clip(c, "band_moments: reference ", ref_row_pitch, ref_frame_pitch, (int64_t)w * es);
  if (rc == PQA_OK) rc = check_device_clip(c, "band_moments: captured ", dis_row_pitch, dis_frame_pitch, (int64_t)w * es);
  if (rc != PQA_OK) return rc;
  if (c->cancelled.load()) return fail(c, PQA_ECANCELLED, "cancelled");
  if (n_frames == 0) return PQA_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const int chunk = n_frames < kBandChunk ? n_frames : kBandChunk;
  const size_t bytes = band_out_bytes(levels, n_frames), per_frame = band_out_bytes(levels, 1) / sizeof(uint64_t);
  rc = side_reserve(c, SIDE_BAND_PART, band_part_bytes(w, h, levels, chunk));
  if (rc == PQA_OK) rc = side_reserve(c, SIDE_BAND_OUT, bytes);
  if (rc != PQA_OK) return rc;
  auto* dev_out = (unsigned long long*)c->side_buf[SIDE_BAND_OUT];
  hipError_t e = hipSuccess;
  for (int f0 = 0; f0 < n_frames && e == hipSuccess; f0 += kBandChunk)   // the chunks share the partials: the stream keeps them in order
    e = launch_band_moments(c->stream, c->elem, (int)c->cfg.bit_depth, (const uint8_t*)ref + (int64_t)f0 * ref_frame_pitch,
                            ref_row_pitch / es, ref_frame_pitch / es, (const uint8_t*)dis + (int64_t)f0 * dis_frame_pitch,
                            dis_row_pitch / es, dis_frame_pitch / es, chunk_len(n_frames, f0, kBandChunk), w, h, levels,
                            c->side_buf[SIDE_BAND_PART], dev_out + (size_t)f0 * per_frame);
  return side_finish(c, "band_moments", e, out, dev_out, bytes);
}

int pqa_band_moments(pqa_ctx* c, const pqa_band_spec* spec, const void* const* ref_frames, int64_t ref_row_stride,
                     const void* const* dis_frames, int64_t dis_row_stride, int32_t n_frames, uint64_t* out) {
  int rc = bd_check(c, spec, ref_frames, dis_frames, n_frames, out);
  if (rc != PQA_OK) return rc;
  const int es = c->esize, w = (int)spec->width, h = (int)spec->height, levels = (int)spec->levels;
  const size_t row_bytes = (size_t)w * es;
  rc = check_host_frames(c, "band_moments: ", "reference ", ref_frames, 1, n_frames, ref_row_stride, row_bytes, true);
  if (rc == PQA_OK) rc = check_host_frames(c, "band_moments: ", "captured ", dis_frames, 1, n_frames, dis_row_stride, row_bytes, true);
  if (rc != PQA_OK) return rc;
  if (n_frames > 0 && (ref_row_stride % es || dis_row_stride % es))
    return fail(c, PQA_EINVAL, "band_moments: stride is not a multiple of the sample size");
  if (c->cancelled.load()) return fail(c, PQA_ECANCELLED, "cancelled");
  if (n_frames == 0) return PQA_OK;
  HIPCHK(c, hipSetDevice(c->device));
  // The planes travel exactly as pqa_tile_moments' do, through the same buffers: chunks of kBandChunk pairs through the two
  // grow-only pinned buffers of pqa_resample into the two device buffers of pqa_flow_moments, rows 16 bytes apart at least, so
  // the kernel takes its wide loads.  Every chunk's sums land behind the previous chunk's; they come back once.  A pinned
  // buffer is packed again only after the stream has drained the chunk before.
  const int64_t pitch = round_up((int64_t)row_bytes, 16);
  const size_t fb = (size_t)pitch * h;
  const int chunk = n_frames < kBandChunk ? n_frames : kBandChunk;
  const size_t bytes = band_out_bytes(levels, n_frames), per_frame = band_out_bytes(levels, 1) / sizeof(uint64_t);
  rc = rs_pin_reserve(c, 0, fb * chunk);
  if (rc == PQA_OK) rc = rs_pin_reserve(c, 1, fb * chunk);
  if (rc == PQA_OK) rc = side_reserve(c, SIDE_FLOW_REF, fb * chunk);
  if (rc == PQA_OK) rc = side_reserve(c, SIDE_FLOW_DIS, fb * chunk);
  if (rc == PQA_OK) rc = side_reserve(c, SIDE_BAND_PART, band_part_bytes(w, h, levels, chunk));
  if (rc == PQA_OK) rc = side_reserve(c, SIDE_BAND_OUT, bytes);
  if (rc != PQA_OK) return rc;
  auto* dev_out = (unsigned long long*)c->side_buf[SIDE_BAND_OUT];
  hipError_t e = hipSuccess;
  for (int f0 = 0; f0 < n_frames && e == hipSuccess && !c->cancelled.load(); f0 += kBandChunk) {
    const int n = chunk_len(n_frames, f0, kBandChunk);
    if (f0 > 0) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) break;
    for (int f = 0; f < n; ++f) {
      copy_plane_rows(c->rs_pin[0] + (size_t)f * fb, pitch, (const uint8_t*)ref_frames[f0 + f], ref_row_stride, row_bytes, h);
      copy_plane_rows(c->rs_pin[1] + (size_t)f * fb, pitch, (const uint8_t*)dis_frames[f0 + f], dis_row_stride, row_bytes, h);
    }
    e = hipMemcpyAsync(c->side_buf[SIDE_FLOW_REF], c->rs_pin[0], fb * n, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(c->side_buf[SIDE_FLOW_DIS], c->rs_pin[1], fb * n, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess)
      e = launch_band_moments(c->stream, c->elem, (int)c->cfg.bit_depth, c->side_buf[SIDE_FLOW_REF], pitch / es, (int64_t)(fb / es),
                              c->side_buf[SIDE_FLOW_DIS], pitch / es, (int64_t)(fb / es), n, w, h, levels,
                              c->side_buf[SIDE_BAND_PART], dev_out + (size_t)f0 * per_frame);
  }
  return side_finish(c, "band_moments", e, out, dev_out, bytes);
}

// ---- temporal distortion (temporal_moments.hip) ------------------------------------------------------------------------------

int pqa_temporal_sums(void) { return kTemporalSums; }

int pqa_temporal_moments_device(pqa_ctx* c, const pqa_temporal_spec* spec, const void* ref, int64_t ref_row_pitch,
                                int64_t ref_frame_pitch, const void* dis, int64_t dis_row_pitch, int64_t dis_frame_pitch,
                                int32_t n_frames, uint64_t* out) {
  int rc = tm_check(c, spec, ref, dis, n_frames, out);
  if (rc != PQA_OK) return rc;
  const int es = c->esize, w = (int)spec->width, h = (int)spec->height, tile = (int)spec->tile;
  rc = check_device_clip(c, "temporal_moments: reference ", ref_row_pitch, ref_frame_pitch, (int64_t)w * es);
  if (rc == PQA_OK) rc = check_device_clip(c, "temporal_moments: captured ", dis_row_pitch, dis_frame_pitch, (int64_t)w * es);
  if (rc != PQA_OK) return rc;
  if (c->cancelled.load()) return fail(c, PQA_ECANCELLED, "cancelled");
  if (n_frames <= 1) return PQA_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t bytes = temporal_out_bytes(w, h, tile, n_frames), per_tr = temporal_out_bytes(w, h, tile, 2) / sizeof(uint64_t);
  rc = side_reserve(c, SIDE_TEMPORAL_OUT, bytes);
  if (rc != PQA_OK) return rc;
  auto* dev_out = (unsigned long long*)c->side_buf[SIDE_TEMPORAL_OUT];
  hipError_t e = hipSuccess;
  // transitions t0 + 1 ... t0 + kTemporalChunk a launch: frames t0 ... t0 + kTemporalChunk, the first as predecessor only
  for (int t0 = 0; t0 < n_frames - 1 && e == hipSuccess; t0 += kTemporalChunk)
    e = launch_temporal_moments(c->stream, c->elem, (int)c->cfg.bit_depth, (const uint8_t*)ref + (int64_t)t0 * ref_frame_pitch,
                                ref_row_pitch / es, ref_frame_pitch / es, (const uint8_t*)dis + (int64_t)t0 * dis_frame_pitch,
                                dis_row_pitch / es, dis_frame_pitch / es, chunk_len(n_frames - 1, t0, kTemporalChunk) + 1, w, h, tile,
                                c->temporal_walk, dev_out + (size_t)t0 * per_tr);
  return side_finish(c, "temporal_moments", e, out, dev_out, bytes);
}

int pqa_temporal_moments(pqa_ctx* c, const pqa_temporal_spec* spec, const void* const* ref_frames, int64_t ref_row_stride,
                         const void* const* dis_frames, int64_t dis_row_stride, int32_t n_frames, uint64_t* out) {
  int rc = tm_check(c, spec, ref_frames, dis_frames, n_frames, out);
  if (rc != PQA_OK) return rc;
  const int es = c->esize, w = (int)spec->width, h = (int)spec->height, tile = (int)spec->tile;
  const size_t row_bytes = (size_t)w * es;
  rc = check_host_frames(c, "temporal_moments: ", "reference ", ref_frames, 1, n_frames, ref_row_stride, row_bytes, true);
  if (rc == PQA_OK) rc = check_host_frames(c, "temporal_moments: ", "captured ", dis_frames, 1, n_frames, dis_row_stride, row_bytes, true);
  if (rc != PQA_OK) return rc;
  if (n_frames > 0 && (ref_row_stride % es || dis_row_stride % es))
    return fail(c, PQA_EINVAL, "temporal_moments: stride is not a multiple of the sample size");
  if (c->cancelled.load()) return fail(c, PQA_ECANCELLED, "cancelled");
  if (n_frames <= 1) return PQA_OK;
  HIPCHK(c, hipSetDevice(c->device));
  // The planes travel as pqa_tile_moments' do, through the same buffers, every frame once: chunks of kTemporalChunk pairs through
  // the two grow-only pinned buffers of pqa_resample into the two device buffers of pqa_flow_moments, rows 16 bytes apart at
  // least, so the kernel takes its wide loads.  The device buffers hold one slot more than a chunk: a chunk lands in slots
  // 1 ... n, and before the next chunk's upload overwrites them the last pair is copied to slot 0 on the stream, where it is
  // the predecessor of the next chunk's first.  So the first chunk's launch starts at slot 1 (n - 1 transitions) and every
  // later one at slot 0 (n transitions).  Every launch writes its sums behind the previous one's; they come back once.  A
  // pinned buffer is packed again only after the stream has drained the chunk before.
  const int64_t pitch = round_up((int64_t)row_bytes, 16);
  const size_t fb = (size_t)pitch * h;
  const int chunk = n_frames < kTemporalChunk ? n_frames : kTemporalChunk;
  const size_t bytes = temporal_out_bytes(w, h, tile, n_frames), per_tr = temporal_out_bytes(w, h, tile, 2) / sizeof(uint64_t);
  rc = rs_pin_reserve(c, 0, fb * chunk);
  if (rc == PQA_OK) rc = rs_pin_reserve(c, 1, fb * chunk);
  if (rc == PQA_OK) rc = side_reserve(c, SIDE_FLOW_REF, fb * (chunk + 1));
  if (rc == PQA_OK) rc = side_reserve(c, SIDE_FLOW_DIS, fb * (chunk + 1));
  if (rc == PQA_OK) rc = side_reserve(c, SIDE_TEMPORAL_OUT, bytes);
  if (rc != PQA_OK) return rc;
  auto* dev_out = (unsigned long long*)c->side_buf[SIDE_TEMPORAL_OUT];
  auto* dref = (uint8_t*)c->side_buf[SIDE_FLOW_REF];
  auto* ddis = (uint8_t*)c->side_buf[SIDE_FLOW_DIS];
  hipError_t e = hipSuccess;
  int prev_n = 0;   // frames of the chunk before: its last pair is in slot prev_n
  for (int f0 = 0; f0 < n_frames && e == hipSuccess && !c->cancelled.load(); f0 += kTemporalChunk) {
    const int n = chunk_len(n_frames, f0, kTemporalChunk);
    if (f0 > 0) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) break;
    for (int f = 0; f < n; ++f) {
      copy_plane_rows(c->rs_pin[0] + (size_t)f * fb, pitch, (const uint8_t*)ref_frames[f0 + f], ref_row_stride, row_bytes, h);
      copy_plane_rows(c->rs_pin[1] + (size_t)f * fb, pitch, (const uint8_t*)dis_frames[f0 + f], dis_row_stride, row_bytes, h);
    }
    if (prev_n > 0) {   // the seam: slot prev_n >= 1, so source and destination never overlap
      e = hipMemcpyAsync(dref, dref + (size_t)prev_n * fb, fb, hipMemcpyDeviceToDevice, c->stream);
      if (e == hipSuccess) e = hipMemcpyAsync(ddis, ddis + (size_t)prev_n * fb, fb, hipMemcpyDeviceToDevice, c->stream);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(dref + fb, c->rs_pin[0], fb * n, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(ddis + fb, c->rs_pin[1], fb * n, hipMemcpyHostToDevice, c->stream);
    const size_t first = prev_n > 0 ? 0 : fb;   // the slot of the launch's first frame
    if (e == hipSuccess)
      e = launch_temporal_moments(c->stream, c->elem, (int)c->cfg.bit_depth, dref + first, pitch / es, (int64_t)(fb / es), ddis + first,
                                  pitch / es, (int64_t)(fb / es), n + (prev_n > 0 ? 1 : 0), w, h, tile, c->temporal_walk,
                                  dev_out + (size_t)(f0 > 0 ? f0 - 1 : 0) * per_tr);
    prev_n = n;
  }
  return side_finish(c, "temporal_moments", e, out, dev_out, bytes);
}

// ---- coding-grid detection (edge_profiles.hip) -------------------------------------------------------------------------------

int pqa_edge_sums(void) { return kEdgeSums; }

int pqa_edge_profiles_device(pqa_ctx* c, const pqa_edge_spec* spec, const void* ref, int64_t ref_row_pitch, int64_t ref_frame_pitch,
                             const void* dis, int64_t dis_row_pitch, int64_t dis_frame_pitch, int32_t n_frames, uint64_t* out) {
  int rc = eg_check(c, spec, ref, dis, n_frames, out);
  if (rc != PQA_OK) return rc;
  const int es = c->esize, w = (int)spec->width, h = (int)spec->height;
  rc = check_device_clip(c, "edge_profiles: reference ", ref_row_pitch, ref_frame_pitch, (int64_t)w * es);
  if (rc == PQA_OK) rc = check_device_clip(c, "edge_profiles: captured ", dis_row_pitch, dis_frame_pitch, (int64_t)w * es);
  if (rc != PQA_OK) return rc;
  if (c->cancelled.load()) return fail(c, PQA_ECANCELLED, "cancelled");
  if (n_frames == 0) return PQA_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t bytes = edge_out_bytes(w, h, n_frames), per_frame = edge_out_bytes(w, h, 1) / sizeof(uint64_t);
  rc = side_reserve(c, SIDE_EDGE_OUT, bytes);
  if (rc != PQA_OK) return rc;
  auto* dev_out = (unsigned long long*)c->side_buf[SIDE_EDGE_OUT];
  hipError_t e = hipSuccess;
  for (int f0 = 0; f0 < n_frames && e == hipSuccess; f0 += kEdgeChunk)
    e = launch_edge_profiles(c->stream, c->elem, (int)c->cfg.bit_depth, (const uint8_t*)ref + (int64_t)f0 * ref_frame_pitch,
                             ref_row_pitch / es, ref_frame_pitch / es, (const uint8_t*)dis + (int64_t)f0 * dis_frame_pitch,
                             dis_row_pitch / es, dis_frame_pitch / es, chunk_len(n_frames, f0, kEdgeChunk), w, h,
                             dev_out + (size_t)f0 * per_frame);
  return side_finish(c, "edge_profiles", e, out, dev_out, bytes);
}

int pqa_edge_profiles(pqa_ctx* c, const pqa_edge_spec* spec, const void* const* ref_frames, int64_t ref_row_stride,
                      const void* const* dis_frames, int64_t dis_row_stride, int32_t n_frames, uint64_t* out) {
  int rc = eg_check(c, spec, ref_frames, dis_frames, n_frames, out);
  if (rc != PQA_OK) return rc;
  const int es = c->esize, w = (int)spec->width, h = (int)spec->height;
  const size_t row_bytes = (size_t)w * es;
  rc = check_host_frames(c, "edge_profiles: ", "reference ", ref_frames, 1, n_frames, ref_row_stride, row_bytes, true);
  if (rc == PQA_OK) rc = check_host_frames(c, "edge_profiles: ", "captured ", dis_frames, 1, n_frames, dis_row_stride, row_bytes, true);
  if (rc != PQA_OK) return rc;
  if (n_frames > 0 && (ref_row_stride % es || dis_row_stride % es))
    return fail(c, PQA_EINVAL, "edge_profiles: stride is not a multiple of the sample size");
  if (c->cancelled.load()) return fail(c, PQA_ECANCELLED, "cancelled");
  if (n_frames == 0) return PQA_OK;
  HIPCHK(c, hipSetDevice(c->device));
  // The planes travel exactly as pqa_tile_moments' do, through the same buffers: chunks of kEdgeChunk pairs through the two
  // grow-only pinned buffers of pqa_resample into the two device buffers of pqa_flow_moments, rows 16 bytes apart at least, so
  // the kernel takes its wide loads.  Every chunk's kernel writes its profiles behind the previous chunk's; they come back
  // once.  A pinned buffer is packed again only after the stream has drained the chunk before.
  const int64_t pitch = round_up((int64_t)row_bytes, 16);
  const size_t fb = (size_t)pitch * h;
  const int chunk = n_frames < kEdgeChunk ? n_frames : kEdgeChunk;
  const size_t bytes = edge_out_bytes(w, h, n_frames), per_frame = edge_out_bytes(w, h, 1) / sizeof(uint64_t);
  rc = rs_pin_reserve(c, 0, fb * chunk);
  if (rc == PQA_OK) rc = rs_pin_reserve(c, 1, fb * chunk);
  if (rc == PQA_OK) rc = side_reserve(c, SIDE_FLOW_REF, fb * chunk);
  if (rc == PQA_OK) rc = side_reserve(c, SIDE_FLOW_DIS, fb * chunk);
  if (rc == PQA_OK) rc = side_reserve(c, SIDE_EDGE_OUT, bytes);
  if (rc != PQA_OK) return rc;
  auto* dev_out = (unsigned long long*)c->side_buf[SIDE_EDGE_OUT];
  hipError_t e = hipSuccess;
  for (int f0 = 0; f0 < n_frames && e == hipSuccess && !c->cancelled.load(); f0 += kEdgeChunk) {
    const int n = chunk_len(n_frames, f0, kEdgeChunk);
    if (f0 > 0) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) break;
    for (int f = 0; f < n; ++f) {
      copy_plane_rows(c->rs_pin[0] + (size_t)f * fb, pitch, (const uint8_t*)ref_frames[f0 + f], ref_row_stride, row_bytes, h);
      copy_plane_rows(c->rs_pin[1] + (size_t)f * fb, pitch, (const uint8_t*)dis_frames[f0 + f], dis_row_stride, row_bytes, h);
    }
    e = hipMemcpyAsync(c->side_buf[SIDE_FLOW_REF], c->rs_pin[0], fb * n, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(c->side_buf[SIDE_FLOW_DIS], c->rs_pin[1], fb * n, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess)
      e = launch_edge_profiles(c->stream, c->elem, (int)c->cfg.bit_depth, c->side_buf[SIDE_FLOW_REF], pitch / es, (int64_t)(fb / es),
                               c->side_buf[SIDE_FLOW_DIS], pitch / es, (int64_t)(fb / es), n, w, h, dev_out + (size_t)f0 * per_frame);
  }
  return side_finish(c, "edge_profiles", e, out, dev_out, bytes);
}

// ---- active-picture detection (line_profiles.hip) ------------------------------------------------------------------------

int pqa_line_profiles_device(pqa_ctx* c, const pqa_profile_spec* spec, const void* planes, int64_t row_pitch, int64_t frame_pitch,
                             int32_t n_frames, uint64_t* out) {
  int rc = pr_check(c, spec, planes, n_frames, out);
  if (rc != PQA_OK) return rc;
  const int es = c->esize, w = (int)spec->width, h = (int)spec->height;
  rc = check_device_clip(c, "line_profiles: ", row_pitch, frame_pitch, (int64_t)w * es);
  if (rc != PQA_OK) return rc;
  if (c->cancelled.load()) return fail(c, PQA_ECANCELLED, "cancelled");
  if (n_frames == 0) return PQA_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t bytes = profile_out_bytes(w, h, n_frames), per_frame = profile_out_bytes(w, h, 1) / sizeof(uint64_t);
  rc = side_reserve(c, SIDE_PROF_OUT, bytes);
  if (rc != PQA_OK) return rc;
  auto* dev_out = (unsigned long long*)c->side_buf[SIDE_PROF_OUT];
  hipError_t e = hipSuccess;
  for (int f0 = 0; f0 < n_frames && e == hipSuccess; f0 += kProfChunk)
    e = launch_line_profiles(c->stream, c->elem, (int)c->cfg.bit_depth, (const uint8_t*)planes + (int64_t)f0 * frame_pitch,
                             row_pitch / es, frame_pitch / es, chunk_len(n_frames, f0, kProfChunk), w, h, dev_out + (size_t)f0 * per_frame);
  return side_finish(c, "line_profiles", e, out, dev_out, bytes);
}

int pqa_line_profiles(pqa_ctx* c, const pqa_profile_spec* spec, const void* const* frames, int64_t row_stride, int32_t n_frames,
                      uint64_t* out) {
  int rc = pr_check(c, spec, frames, n_frames, out);
  if (rc != PQA_OK) return rc;
  const int es = c->esize, w = (int)spec->width, h = (int)spec->height;
  const size_t row_bytes = (size_t)w * es;
  rc = check_host_frames(c, "line_profiles: ", "", frames, 1, n_frames, row_stride, row_bytes, true);
  if (rc != PQA_OK) return rc;
  if (c->cancelled.load()) return fail(c, PQA_ECANCELLED, "cancelled");
  if (n_frames == 0) return PQA_OK;
  HIPCHK(c, hipSetDevice(c->device));
  // The planes are the call's own size, so they travel as pqa_flow_moments' do: chunks of kProfChunk planes through the first
  // grow-only pinned buffer of pqa_resample into a device buffer of this entry, rows 16 bytes apart at least, so the kernel
  // takes its wide loads.  Every chunk's kernel writes its profiles behind the previous chunk's; they come back once.  The
  // pinned buffer is packed again only after the stream has drained the chunk before: the entry is short, it is not pipelined.
  const int64_t pitch = round_up((int64_t)row_bytes, 16);
  const size_t fb = (size_t)pitch * h;
  const int chunk = n_frames < kProfChunk ? n_frames : kProfChunk;
  const size_t bytes = profile_out_bytes(w, h, n_frames), per_frame = profile_out_bytes(w, h, 1) / sizeof(uint64_t);
  rc = rs_pin_reserve(c, 0, fb * chunk);
  if (rc == PQA_OK) rc = side_reserve(c, SIDE_PROF_SRC, fb * chunk);
  if (rc == PQA_OK) rc = side_reserve(c, SIDE_PROF_OUT, bytes);
  if (rc != PQA_OK) return rc;
  auto* dev_out = (unsigned long long*)c->side_buf[SIDE_PROF_OUT];
  hipError_t e = hipSuccess;
  for (int f0 = 0; f0 < n_frames && e == hipSuccess && !c->cancelled.load(); f0 += kProfChunk) {
    const int n = chunk_len(n_frames, f0, kProfChunk);
    if (f0 > 0) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) break;
    for (int f = 0; f < n; ++f) copy_plane_rows(c->rs_pin[0] + (size_t)f * fb, pitch, (const uint8_t*)frames[f0 + f], row_stride, row_bytes, h);
    e = hipMemcpyAsync(c->side_buf[SIDE_PROF_SRC], c->rs_pin[0], fb * n, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess)
      e = launch_line_profiles(c->stream, c->elem, (int)c->cfg.bit_depth, c->side_buf[SIDE_PROF_SRC], pitch / es, (int64_t)(fb / es), n,
                               w, h, dev_out + (size_t)f0 * per_frame);
  }
  return side_finish(c, "line_profiles", e, out, dev_out, bytes);
}

// ---- colour-matrix alignment (colour_moments.hip) ------------------------------------------------------------------------

int pqa_colour_sums(void) { return kColourSums; }

int pqa_colour_moments_device(pqa_ctx* c, const pqa_device_clip* ref, const pqa_device_clip* dis, int32_t n_frames, uint32_t lo,
                              uint32_t hi, uint64_t* out) {
  if (!c) return PQA_EINVAL;
  int rc = cl_check(c, "colour_moments", n_frames);
  if (rc != PQA_OK) return rc;
  const uint32_t top = (1u << c->cfg.bit_depth) - 1u;
  if (lo > hi || hi > top) return fail(c, PQA_EINVAL, "colour_moments: mask %u ... %u outside 0 ... %u", lo, hi, top);
  if (n_frames > 0 && (!ref || !dis)) return fail(c, PQA_EINVAL, "colour_moments: null clip pointer");
  if (n_frames > 0 && !out) return fail(c, PQA_EINVAL, "colour_moments: null output pointer");
  if (n_frames == 0) return PQA_OK;
  rc = cl_check_clip(c, "colour_moments: reference ", ref);
  if (rc == PQA_OK) rc = cl_check_clip(c, "colour_moments: captured ", dis);
  if (rc != PQA_OK) return rc;
  if (c->cancelled.load()) return fail(c, PQA_ECANCELLED, "cancelled");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t bytes = (size_t)n_frames * kColourSums * sizeof(uint64_t);
  rc = side_reserve(c, SIDE_COLOUR_OUT, bytes);
  if (rc != PQA_OK) return rc;
  const int es = c->esize;
  auto* dev_out = (unsigned long long*)c->side_buf[SIDE_COLOUR_OUT];
  hipError_t e = hipSuccess;
  for (int f0 = 0; f0 < n_frames && e == hipSuccess; f0 += kColourChunk) {
    PlaneRun r[3], d[3];
    for (int p = 0; p < 3; ++p) {
      r[p] = PlaneRun{(const uint8_t*)ref->plane[p] + (int64_t)f0 * ref->frame_pitch[p], ref->row_pitch[p] / es, ref->frame_pitch[p] / es};
      d[p] = PlaneRun{(const uint8_t*)dis->plane[p] + (int64_t)f0 * dis->frame_pitch[p], dis->row_pitch[p] / es, dis->frame_pitch[p] / es};
    }
    e = launch_colour_moments(c->stream, c->elem, (int)c->cfg.bit_depth, (int)c->cfg.chroma_hshift, (int)c->cfg.chroma_vshift, r, d,
                              chunk_len(n_frames, f0, kColourChunk), c->pw[0], c->ph[0], lo, hi, dev_out + (size_t)f0 * kColourSums);
  }
  return side_finish(c, "colour_moments", e, out, dev_out, bytes);
}

int pqa_colour_moments(pqa_ctx* c, const void* const* ref_frames, const int64_t ref_strides[3], const void* const* dis_frames,
                       const int64_t dis_strides[3], int32_t n_frames, uint32_t lo, uint32_t hi, uint64_t* out) {
  if (!c) return PQA_EINVAL;
  int rc = cl_check(c, "colour_moments", n_frames);
  if (rc != PQA_OK) return rc;
  const uint32_t top = (1u << c->cfg.bit_depth) - 1u;
  if (lo > hi || hi > top) return fail(c, PQA_EINVAL, "colour_moments: mask %u ... %u outside 0 ... %u", lo, hi, top);
  if (n_frames > 0 && (!ref_frames || !dis_frames || !ref_strides || !dis_strides)) return fail(c, PQA_EINVAL, "colour_moments: null frame list");
  if (n_frames > 0 && !out) return fail(c, PQA_EINVAL, "colour_moments: null output pointer");
  if (n_frames == 0) return PQA_OK;
  rc = cl_check_host(c, "colour_moments: ", "reference ", ref_frames, ref_strides, n_frames);
  if (rc == PQA_OK) rc = cl_check_host(c, "colour_moments: ", "captured ", dis_frames, dis_strides, n_frames);
  if (rc != PQA_OK) return rc;
  if (c->cancelled.load()) return fail(c, PQA_ECANCELLED, "cancelled");
  HIPCHK(c, hipSetDevice(c->device));
  // Three planes a frame, so the frames travel as pqa_flow_moments' planes do: chunks of kColourChunk pairs through the two
  // grow-only pinned buffers of pqa_resample (reference frames through the first, captured ones through the second) into
  // device buffers of this entry; every chunk's kernel writes its sums behind the previous chunk's, they come back once.
  const ClLayout L = cl_layout(c);
  const int chunk = n_frames < kColourChunk ? n_frames : kColourChunk;
  const size_t bytes = (size_t)n_frames * kColourSums * sizeof(uint64_t);
  rc = rs_pin_reserve(c, 0, L.bytes * chunk);
  if (rc == PQA_OK) rc = rs_pin_reserve(c, 1, L.bytes * chunk);
  if (rc == PQA_OK) rc = side_reserve(c, SIDE_COLOUR_A, L.bytes * chunk);
  if (rc == PQA_OK) rc = side_reserve(c, SIDE_COLOUR_B, L.bytes * chunk);
  if (rc == PQA_OK) rc = side_reserve(c, SIDE_COLOUR_OUT, bytes);
  if (rc != PQA_OK) return rc;
  auto* dev_out = (unsigned long long*)c->side_buf[SIDE_COLOUR_OUT];
  PlaneRun r[3], d[3];
  cl_runs(c, L, c->side_buf[SIDE_COLOUR_A], r);
  cl_runs(c, L, c->side_buf[SIDE_COLOUR_B], d);
  hipError_t e = hipSuccess;
  for (int f0 = 0; f0 < n_frames && e == hipSuccess && !c->cancelled.load(); f0 += kColourChunk) {
    const int n = chunk_len(n_frames, f0, kColourChunk);
    if (f0 > 0) e = hipStreamSynchronize(c->stream);   // the pinned buffers are packed again only after the chunk before has left them
    if (e != hipSuccess) break;
    cl_pack(c, L, c->rs_pin[0], ref_frames + (size_t)f0 * 3, ref_strides, n);
    cl_pack(c, L, c->rs_pin[1], dis_frames + (size_t)f0 * 3, dis_strides, n);
    e = hipMemcpyAsync(c->side_buf[SIDE_COLOUR_A], c->rs_pin[0], L.bytes * n, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(c->side_buf[SIDE_COLOUR_B], c->rs_pin[1], L.bytes * n, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess)
      e = launch_colour_moments(c->stream, c->elem, (int)c->cfg.bit_depth, (int)c->cfg.chroma_hshift, (int)c->cfg.chroma_vshift, r, d, n,
                                c->pw[0], c->ph[0], lo, hi, dev_out + (size_t)f0 * kColourSums);
  }
  return side_finish(c, "colour_moments", e, out, dev_out, bytes);
}

int pqa_colour_apply_device(pqa_ctx* c, const int32_t m[12], const pqa_device_clip* src, const pqa_device_clip* dst, int32_t n_frames) {
  if (!c) return PQA_EINVAL;
  int rc = cl_check(c, "colour_apply", n_frames);
  if (rc != PQA_OK) return rc;
  if (!m) return fail(c, PQA_EINVAL, "colour_apply: null matrix");
  if (!colour_matrix_ok(m)) return fail(c, PQA_EINVAL, "colour_apply: a matrix entry is out of range (|offset| < 2^28, |gain| < 2^16 in Q14)");
  if (n_frames > 0 && (!src || !dst)) return fail(c, PQA_EINVAL, "colour_apply: null clip pointer");
  if (n_frames == 0) return PQA_OK;
  rc = cl_check_clip(c, "colour_apply: source ", src);
  if (rc == PQA_OK) rc = cl_check_clip(c, "colour_apply: destination ", dst);
  if (rc != PQA_OK) return rc;
  if (c->cancelled.load()) return fail(c, PQA_ECANCELLED, "cancelled");
  HIPCHK(c, hipSetDevice(c->device));
  const int es = c->esize;
  hipError_t e = hipSuccess;
  for (int f0 = 0; f0 < n_frames && e == hipSuccess; f0 += kColourChunk) {
    PlaneRun s[3];
    MutPlaneRun d[3];
    for (int p = 0; p < 3; ++p) {
      s[p] = PlaneRun{(const uint8_t*)src->plane[p] + (int64_t)f0 * src->frame_pitch[p], src->row_pitch[p] / es, src->frame_pitch[p] / es};
      d[p] = MutPlaneRun{(uint8_t*)const_cast<void*>(dst->plane[p]) + (int64_t)f0 * dst->frame_pitch[p], dst->row_pitch[p] / es, dst->frame_pitch[p] / es};
    }
    e = launch_colour_apply(c->stream, c->elem, (int)c->cfg.bit_depth, (int)c->cfg.chroma_hshift, (int)c->cfg.chroma_vshift, m, s, d,
                            chunk_len(n_frames, f0, kColourChunk), c->pw[0], c->ph[0]);
  }
  return side_finish(c, "colour_apply", e, nullptr, nullptr, 0);
}

int pqa_colour_apply(pqa_ctx* c, const int32_t m[12], const void* const* src_frames, const int64_t src_strides[3],
                     void* const* dst_frames, const int64_t dst_strides[3], int32_t n_frames) {
  if (!c) return PQA_EINVAL;
  int rc = cl_check(c, "colour_apply", n_frames);
  if (rc != PQA_OK) return rc;
  if (!m) return fail(c, PQA_EINVAL, "colour_apply: null matrix");
  if (!colour_matrix_ok(m)) return fail(c, PQA_EINVAL, "colour_apply: a matrix entry is out of range (|offset| < 2^28, |gain| < 2^16 in Q14)");
  if (n_frames > 0 && (!src_frames || !dst_frames || !src_strides || !dst_strides)) return fail(c, PQA_EINVAL, "colour_apply: null frame list");
  if (n_frames == 0) return PQA_OK;
  rc = cl_check_host(c, "colour_apply: ", "source ", src_frames, src_strides, n_frames);
  if (rc == PQA_OK) rc = cl_check_host(c, "colour_apply: ", "destination ", (const void* const*)dst_frames, dst_strides, n_frames);
  if (rc != PQA_OK) return rc;
  if (c->cancelled.load()) return fail(c, PQA_ECANCELLED, "cancelled");
  HIPCHK(c, hipSetDevice(c->device));
  // as pqa_resample: a chunk is uploaded, mapped, downloaded and copied out before the next one starts
  const ClLayout L = cl_layout(c);
  const int chunk = n_frames < kColourChunk ? n_frames : kColourChunk;
  rc = rs_pin_reserve(c, 0, L.bytes * chunk);
  if (rc == PQA_OK) rc = rs_pin_reserve(c, 1, L.bytes * chunk);
  if (rc == PQA_OK) rc = side_reserve(c, SIDE_COLOUR_A, L.bytes * chunk);
  if (rc == PQA_OK) rc = side_reserve(c, SIDE_COLOUR_B, L.bytes * chunk);
  if (rc != PQA_OK) return rc;
  PlaneRun s[3], dr[3];
  MutPlaneRun d[3];
  cl_runs(c, L, c->side_buf[SIDE_COLOUR_A], s);
  cl_runs(c, L, c->side_buf[SIDE_COLOUR_B], dr);
  for (int p = 0; p < 3; ++p) d[p] = MutPlaneRun{const_cast<void*>(dr[p].base), dr[p].row_pitch, dr[p].frame_pitch};
  for (int f0 = 0; f0 < n_frames; f0 += kColourChunk) {
    const int n = chunk_len(n_frames, f0, kColourChunk);
    cl_pack(c, L, c->rs_pin[0], src_frames + (size_t)f0 * 3, src_strides, n);
    hipError_t e = hipMemcpyAsync(c->side_buf[SIDE_COLOUR_A], c->rs_pin[0], L.bytes * n, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess)
      e = launch_colour_apply(c->stream, c->elem, (int)c->cfg.bit_depth, (int)c->cfg.chroma_hshift, (int)c->cfg.chroma_vshift, m, s, d, n,
                              c->pw[0], c->ph[0]);
    rc = side_finish(c, "colour_apply", e, c->rs_pin[1], c->side_buf[SIDE_COLOUR_B], L.bytes * n);
    if (rc != PQA_OK) return rc;
    for (int f = 0; f < n; ++f)   // row by row: the bytes between a destination row's end and the next row stay as they are
      for (int p = 0; p < 3; ++p)
        for (int y = 0; y < c->ph[p]; ++y)
          memcpy((uint8_t*)dst_frames[(size_t)(f0 + f) * 3 + p] + (int64_t)y * dst_strides[p],
                 c->rs_pin[1] + (size_t)f * L.bytes + L.off[p] + (size_t)y * L.pitch[p], (size_t)c->pw[p] * c->esize);
  }
  return PQA_OK;
}

}  // extern "C"
