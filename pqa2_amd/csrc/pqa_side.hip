// The one-shot analyses and plane transforms of the C ABI that leave the scoring chain alone: anchored frame differences, luma
// statistics, temporal / spatial / level alignment, the colour moments, Delta E ITP, the spec-driven analyses of planes of the
// call's own size (registration moments, tile / band / temporal moments, edge and line profiles), and the transforms (resampler,
// packed unpack, format and RGB converters, table apply, deinterlacer, mask blend, colour-matrix apply).  Each has an entry for a clip in HBM
// and one for frames in host memory.  Host frames, of the context's size or of the call's own, take one staging path, whose host
// side is host_stage.h: two pinned chunks and two staging buffers.  The analyses share one driver per kind of clip (pair_run) and,
// where a spec names the plane, one checker (spec_check); the transforms share one driver per kind of clip (transform_run);
// pqa_cross_sse, whose two clips differ in length, walks its own tiles over the same pinned chunks, and pqa_frame_sad has the
// runtime copy its frames into the first staging buffer.  Every entry ends in one epilogue (side_finish).
// Declarations: include/pqa_vmaf.h; the context: pqa_ctx.h.
#include "pqa_ctx.h"

#include "ingest.h"

#include <climits>
#include <cstdio>
#include <functional>
#include <type_traits>

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

// ---- the epilogue, the grow-only buffers ----------------------------------------------------------------------------------
// The end of every entry, after its launches (e: the first error among them): the results go to the caller unless
// something failed or the call was cancelled, and the stream is ALWAYS synchronised -- nothing queued on it may still point
// at the pinned chunks or at `out` when the call returns.
int side_finish(pqa_ctx* c, const char* what, hipError_t e, void* out, const void* dev_out, size_t bytes) {
  if (e == hipSuccess && !c->cancelled.load() && bytes) e = hipMemcpyAsync(out, dev_out, bytes, hipMemcpyDeviceToHost, c->stream);
  const hipError_t es = hipStreamSynchronize(c->stream);
  c->side_pin_busy[0] = c->side_pin_busy[1] = false;
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

// one of the two grow-only pinned chunks of the side analyses, with its event
int side_pin_reserve(pqa_ctx* c, int which, size_t bytes) {
  if (!c->side_pin_sent[which]) HIPCHK(c, hipEventCreateWithFlags(&c->side_pin_sent[which], hipEventDisableTiming));
  if (c->side_pin_cap[which] >= bytes) return PQA_OK;
  if (c->side_pin[which]) {
    HIPCHK(c, hipHostFree(c->side_pin[which]));
    c->side_pin[which] = nullptr;
    c->side_pin_cap[which] = 0;
  }
  HIPCHK(c, hipHostMalloc((void**)&c->side_pin[which], bytes, hipHostMallocDefault));
  c->side_pin_cap[which] = bytes;
  return PQA_OK;
}

// A pinned chunk is packed again while the kernels of the chunk before still run: before the pack the host waits only until
// the upload that last read the chunk has left it (pin_wait), which the chunk's event, recorded behind that upload (pin_mark),
// tells.  The stream orders everything else: a kernel before the next upload into the device slots it reads.
hipError_t pin_wait(pqa_ctx* c, int which) {
  if (!c->side_pin_busy[which]) return hipSuccess;
  c->side_pin_busy[which] = false;
  return hipEventSynchronize(c->side_pin_sent[which]);
}
hipError_t pin_mark(pqa_ctx* c, int which) {
  const hipError_t e = hipEventRecord(c->side_pin_sent[which], c->stream);
  c->side_pin_busy[which] = e == hipSuccess;
  return e;
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

// the workspaces of a launch of at most `chunk` frame pairs
int sh_prepare(pqa_ctx* c, int radius, int chunk) {
  const int rc = side_reserve(c, SIDE_SHIFT_PART, shift_part_bytes(c->elem, c->pw[0], c->ph[0], radius, chunk));
  return rc == PQA_OK ? side_reserve(c, SIDE_SHIFT_ROWSQ, shift_rowsq_bytes(c->ph[0], radius, chunk)) : rc;
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

// ---- resampler (resample.hip): argument rules (no device call), tables ------------------------------------------------
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

// ---- the spec-driven analyses of a clip pair (or, pqa_line_profiles, of one clip): planes of the call's own size -----------
// pqa_flow_moments, pqa_tile_moments, pqa_band_moments, pqa_temporal_moments, pqa_edge_profiles and pqa_line_profiles differ
// in their spec, their kernel and what a PairJob names; one checker, one driver for clips in HBM and one for host frames.

// The argument rules, in the order in which they fire (no device call): null spec, struct_size, `rule` (the entry's own, on
// its third field), plane size, negative count, null clips, null out.  dis: the second clip, or the first again when there
// is only one; `out` may be null below out_from frames.
// the two sizes that spec_check holds against 1 ... 8192: the plane's, or (pqa_convert_spec) the luma frame's
template <class Spec>
void spec_sizes(const Spec* sp, uint32_t out[2]) { out[0] = sp->width; out[1] = sp->height; }
void spec_sizes(const pqa_convert_spec* sp, uint32_t out[2]) { out[0] = sp->luma_width; out[1] = sp->luma_height; }

template <class Spec, class Rule>
int spec_check(pqa_ctx* c, const char* who, const Spec* sp, uint32_t min_size, const void* ref, const void* dis, int32_t n_frames,
               const void* out, int out_from, Rule rule) {
  if (!c) return PQA_EINVAL;
  if (!sp) return fail(c, PQA_EINVAL, "%s: null spec", who);
  if (sp->struct_size != sizeof(Spec)) return fail(c, PQA_EINVAL, "%s: bad struct_size %u", who, sp->struct_size);
  const int rc = rule();
  if (rc != PQA_OK) return rc;
  uint32_t sizes[2];
  spec_sizes(sp, sizes);
  for (uint32_t v : sizes)
    if (v < min_size || v > 8192) return fail(c, PQA_EINVAL, "%s: plane size %u outside %u ... 8192", who, v, min_size);
  if (n_frames < 0) return fail(c, PQA_EINVAL, "%s: negative frame count", who);
  if (n_frames > 0 && (!ref || !dis)) return fail(c, PQA_EINVAL, "%s: null clip pointer", who);
  if (n_frames >= out_from && !out) return fail(c, PQA_EINVAL, "%s: null output pointer", who);
  return PQA_OK;
}

struct HostClip {   // a list of frames in host memory, rows of plane p strides[p] bytes apart (one plane: the address of its stride)
  const void* const* at;
  const int64_t* strides;
};
template <class Clip>
constexpr bool kHostFrames = std::is_same<Clip, HostClip>::value;
struct DevClip {   // planes in HBM, pitches in bytes
  const void* at;
  int64_t row_pitch, frame_pitch;
};

// ---- clips in HBM as the launches take them ---------------------------------------------------------------------------------
constexpr int kFrameCap = 32768;   // frames per launch of a transform that has no chunk of its own (a dimension of the grid)

pqa_device_clip one_plane(const void* base, int64_t row_pitch, int64_t frame_pitch) {
  return pqa_device_clip{{base, nullptr, nullptr}, {row_pitch, 0, 0}, {frame_pitch, 0, 0}};
}
// a clip from its frame f0 on: every plane advances by its own frame pitch
pqa_device_clip clip_from(const pqa_device_clip& k, int f0) {
  pqa_device_clip at = k;
  for (int p = 0; p < 3; ++p)
    if (k.plane[p]) at.plane[p] = (const uint8_t*)k.plane[p] + (int64_t)f0 * k.frame_pitch[p];
  return at;
}
// a chunk staged at `base` in layout L
pqa_device_clip staged_clip(const host::ClipLayout& L, const void* base) {
  pqa_device_clip k{};
  for (int p = 0; p < L.n_planes; ++p) {
    k.plane[p] = (const uint8_t*)base + L.off[p];
    k.row_pitch[p] = L.plane[p].pitch;
    k.frame_pitch[p] = (int64_t)L.frame_bytes;
  }
  return k;
}
// PlaneRun[3] or MutPlaneRun[3] (pitches in samples of es bytes) of a clip from its frame f0 on
template <class Run>
void plane_runs(const pqa_device_clip& k, int f0, int es, Run run[3]) {
  const pqa_device_clip at = clip_from(k, f0);
  for (int p = 0; p < 3; ++p) run[p] = Run{const_cast<void*>(at.plane[p]), at.row_pitch[p] / es, at.frame_pitch[p] / es};
}
// launch(f0, n) over n_frames frames in runs of at most cap: stops at the first error and, where `stop` is given, before a run once it is set
template <class Launch>
hipError_t launch_runs(int n_frames, int cap, const std::atomic<int>* stop, Launch launch) {
  hipError_t e = hipSuccess;
  for (int f0 = 0; f0 < n_frames && e == hipSuccess && !(stop && stop->load()); f0 += cap) e = launch(f0, chunk_len(n_frames, f0, cap));
  return e;
}
// A plane in HBM of samples of es bytes (not always the context's): its base and both pitches are whole samples.
bool whole_samples(const void* base, int64_t row_pitch, int64_t frame_pitch, int es) {
  return !(((uintptr_t)base | (uintptr_t)row_pitch | (uintptr_t)frame_pitch) & (uintptr_t)(es - 1));
}
// The rules of the planes of pqa_format_convert_device, pqa_table_apply_device and pqa_mask_blend_device, in their order: every
// plane is whole samples, then every row pitch holds a row.
struct DevPlane {
  const char* kind;   // "source", "destination", "fill"
  const void* base;
  int64_t row_pitch, frame_pitch, row_bytes;
  int es;
};
int check_device_planes(pqa_ctx* c, const char* who, std::initializer_list<DevPlane> planes) {
  for (const DevPlane& p : planes)
    if (!whole_samples(p.base, p.row_pitch, p.frame_pitch, p.es))
      return fail(c, PQA_EINVAL, "%s: %s base or pitch is not a multiple of the sample size", who, p.kind);
  for (const DevPlane& p : planes)
    if (p.row_pitch < p.row_bytes) return fail(c, PQA_EINVAL, "%s: %s pitch smaller than a row", who, p.kind);
  return PQA_OK;
}

// What an analysis asks of a driver.  carry 0: a result per frame.  carry 1 (pqa_temporal_moments): a result per transition,
// so a launch also reads the frame in front of its first transition, and fewer than two frames are no work.
struct PairJob {
  const char* who;   // opens every message
  host::ClipLayout L;   // a frame as the host entry stages it: one plane, or three (pqa_colour_moments, pqa_delta_itp)
  int32_t n_frames;
  int chunk, carry;   // chunk: results per launch
  SideBuf out_buf;
  size_t out_bytes;   // of all results: they come back once
  void* out;
  bool whole_samples = true;       // host frames: refuse a stride that is no multiple of the sample size
  SideBuf part_buf = kSideBufs;    // a workspace of part_bytes that the launches share (pqa_band_moments, pqa_delta_itp)
  size_t part_bytes = 0;
  // what the five oldest entries answer differently, each as it always has:
  bool bottom_up = false;          // host frames: a negative stride passes, and the rows are then copied bottom-up
  bool row_holds = true;           // one-plane clips in HBM: refuse a row pitch smaller than a row (pqa_luma_stats_device: no such rule)
  bool bare = false;               // a rule's message opens with nothing, not with "<who>: " (pqa_luma_stats)
  std::function<int()> prepare;    // reserves the workspaces one part_buf cannot name (pqa_shift_sse)
};

int job_reserve(pqa_ctx* c, const PairJob& j) {
  int rc = j.part_buf != kSideBufs ? side_reserve(c, j.part_buf, j.part_bytes) : PQA_OK;
  if (rc == PQA_OK) rc = side_reserve(c, j.out_buf, j.out_bytes);
  return rc == PQA_OK && j.prepare ? j.prepare() : rc;
}

// Host frames of the context's size travel in chunks of at most 8 and of no more than a batch of the scoring path: the
// per-batch workspaces (luma_part, ig_part) hold that many, and so do kShiftChunk and kLevelChunk.
int ctx_chunk(const pqa_ctx* c) { return c->B < 8 ? c->B : 8; }

// Three-plane clips in HBM, after the entry's own rules.  launch(ref runs, dis runs, n frames, index of the first result) queues
// a kernel; `stop`: launch_runs.
template <class Launch>
int pair_run(pqa_ctx* c, const PairJob& j, const pqa_device_clip& ref, const pqa_device_clip& dis, const std::atomic<int>* stop, Launch launch) {
  HIPCHK(c, hipSetDevice(c->device));
  const int rc = job_reserve(c, j);
  if (rc != PQA_OK) return rc;
  const hipError_t e = launch_runs(j.n_frames, j.chunk, stop, [&](int f0, int n) {
    PlaneRun r[3], d[3];
    plane_runs(ref, f0, c->esize, r);
    plane_runs(dis, f0, c->esize, d);
    return launch(r, d, n, f0);
  });
  return side_finish(c, j.who, e, j.out, c->side_buf[j.out_buf], j.out_bytes);
}

// One-plane clips in HBM (dis null: one clip), with their rules.
template <class Launch>
int pair_run(pqa_ctx* c, const PairJob& j, const DevClip& ref, const DevClip* dis, Launch launch) {
  const int es = c->esize;
  const int64_t row_bytes = (int64_t)j.L.plane[0].row_bytes;
  char who[48];
  const int64_t min_row = j.row_holds ? row_bytes : INT64_MIN;
  snprintf(who, sizeof who, dis ? "%s: reference " : "%s: ", j.who);
  if (j.bare) who[0] = 0;
  int rc = check_device_clip(c, who, ref.row_pitch, ref.frame_pitch, min_row);
  if (rc == PQA_OK && dis) {
    snprintf(who, sizeof who, "%s: captured ", j.who);
    rc = check_device_clip(c, who, dis->row_pitch, dis->frame_pitch, min_row);
  }
  if (rc != PQA_OK) return rc;
  if (c->cancelled.load()) return fail(c, PQA_ECANCELLED, "cancelled");
  if (j.n_frames <= j.carry) return PQA_OK;
  HIPCHK(c, hipSetDevice(c->device));
  rc = job_reserve(c, j);
  if (rc != PQA_OK) return rc;
  const int results = j.n_frames - j.carry;
  const hipError_t e = launch_runs(results, j.chunk, nullptr, [&](int f0, int n) {   // the launches share what they share in stream order
    PlaneRun r[3] = {}, d[3] = {};
    plane_runs(one_plane(ref.at, ref.row_pitch, ref.frame_pitch), f0, es, r);
    if (dis) plane_runs(one_plane(dis->at, dis->row_pitch, dis->frame_pitch), f0, es, d);
    return launch(r, d, n + j.carry, f0);
  });
  return side_finish(c, j.who, e, j.out, c->side_buf[j.out_buf], j.out_bytes);
}

// Host frames (dis null: one clip), with their rules.  The frames are of any size, so they travel in chunks through the two
// grow-only pinned chunks (the reference frames through the first, the captured ones through the second) into the two staging
// buffers (SIDE_STAGE_A, SIDE_STAGE_B) as host_stage.h lays out: packed rows, a chunk launched before the next is packed -- under
// that launch's kernel: the host waits for the uploads out of the pinned chunks only (pin_wait) --, with carry 1 the last pair
// of a chunk kept as predecessor of the next.  Every entry here is synchronous, so no two calls are ever in flight in these
// buffers, and no call reads what another left there.  Every launch writes its results behind the previous one's; they come
// back once.
template <class Launch>
int pair_run(pqa_ctx* c, const PairJob& j, const HostClip& ref, const HostClip* dis, Launch launch) {
  const int es = c->esize, np = j.L.n_planes;
  char who[48];
  snprintf(who, sizeof who, "%s: ", j.who);
  if (j.bare) who[0] = 0;
  int rc = PQA_OK;
  for (const HostClip* k : {&ref, dis})
    for (int p = 0; k && p < np && rc == PQA_OK; ++p)
      rc = check_host_frames(c, who, !dis ? "" : k == &ref ? "reference " : "captured ", k->at + p, np, j.n_frames, k->strides[p], j.L.plane[p].row_bytes, !j.bottom_up);
  if (rc != PQA_OK) return rc;
  if (j.whole_samples && j.n_frames > 0 && (ref.strides[0] % es || (dis && dis->strides[0] % es)))
    return fail(c, PQA_EINVAL, "%s: stride is not a multiple of the sample size", j.who);
  if (c->cancelled.load()) return fail(c, PQA_ECANCELLED, "cancelled");
  if (j.n_frames <= j.carry) return PQA_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t fb = j.L.frame_bytes, slots = (size_t)(j.n_frames < j.chunk ? j.n_frames : j.chunk);
  rc = side_pin_reserve(c, 0, fb * slots);
  if (rc == PQA_OK && (dis || j.n_frames > j.chunk)) rc = side_pin_reserve(c, 1, fb * slots);   // one clip: its chunks alternate
  if (rc == PQA_OK) rc = side_reserve(c, SIDE_STAGE_A, fb * (slots + j.carry));
  if (rc == PQA_OK && dis) rc = side_reserve(c, SIDE_STAGE_B, fb * (slots + j.carry));
  if (rc == PQA_OK) rc = job_reserve(c, j);
  if (rc != PQA_OK) return rc;
  uint8_t* const dev[2] = {(uint8_t*)c->side_buf[SIDE_STAGE_A], dis ? (uint8_t*)c->side_buf[SIDE_STAGE_B] : nullptr};
  const hipError_t e = host::stage_walk(
      j.L, c->side_pin, ref.at, ref.strides, dis ? dis->at : nullptr, dis ? dis->strides : nullptr, j.n_frames, j.chunk, j.carry, c->cancelled,
      [&](int b) { return pin_wait(c, b); },
      [&](int from_slot) {   // from_slot >= 1: no overlap
        hipError_t e = hipSuccess;
        for (int k = 0; k < (dis ? 2 : 1) && e == hipSuccess; ++k)
          e = hipMemcpyAsync(dev[k], dev[k] + (size_t)from_slot * fb, fb, hipMemcpyDeviceToDevice, c->stream);
        return e;
      },
      [&](int b, int k, int slot, int n) {
        const hipError_t e = hipMemcpyAsync(dev[k] + (size_t)slot * fb, c->side_pin[b], fb * n, hipMemcpyHostToDevice, c->stream);
        return e == hipSuccess ? pin_mark(c, b) : e;
      },
      [&](int slot, int n, int out_index) {
        PlaneRun r[3] = {}, d[3] = {};
        plane_runs(staged_clip(j.L, dev[0]), slot, es, r);
        if (dis) plane_runs(staged_clip(j.L, dev[1]), slot, es, d);
        return launch(r, d, n, out_index);
      });
  return side_finish(c, j.who, e, j.out, c->side_buf[j.out_buf], j.out_bytes);
}

// ---- the spec-driven analyses (spec_check, pair_run above) ----------------------------------------------------------------
// Clip is HostClip or DevClip: both entries of an analysis are one body, which checks, sizes its results and names its launch.
// A launch's results lie `at` results into the analysis' output buffer; r and d are its runs of planes (the first of three).

// registration moments (flow_moments.hip); this one lets a stride that is no multiple of the sample size pass
template <class Clip>
int flow_moments(pqa_ctx* c, const pqa_flow_spec* sp, const Clip& ref, const Clip& dis, int32_t n_frames, int64_t* out) {
  const int rc = spec_check(c, "flow_moments", sp, 3, ref.at, dis.at, n_frames, out, 1, [&] {
    return sp->tile > 64 || !flow_tile_ok((int)sp->tile) ? fail(c, PQA_EINVAL, "flow_moments: tile %u is not 8, 16, 32 or 64", sp->tile) : PQA_OK;
  });
  if (rc != PQA_OK) return rc;
  const int w = (int)sp->width, h = (int)sp->height, tile = (int)sp->tile;
  const size_t per_frame = flow_out_bytes(w, h, tile, 1) / sizeof(long long);
  const PairJob j{"flow_moments", host::plane_clip((size_t)w * c->esize, h), n_frames, kFlowChunk, 0, SIDE_FLOW_OUT, flow_out_bytes(w, h, tile, n_frames), out, false};
  return pair_run(c, j, ref, &dis, [&](const PlaneRun* r, const PlaneRun* d, int n, int at) {
    return launch_flow_moments(c->stream, c->elem, (int)c->cfg.bit_depth, r->base, r->row_pitch, r->frame_pitch, d->base, d->row_pitch,
                               d->frame_pitch, n, w, h, tile, (long long*)c->side_buf[SIDE_FLOW_OUT] + (size_t)at * per_frame);
  });
}

// distortion map (tile_moments.hip)
template <class Clip>
int tile_moments(pqa_ctx* c, const pqa_tile_spec* sp, const Clip& ref, const Clip& dis, int32_t n_frames, uint64_t* out) {
  const int rc = spec_check(c, "tile_moments", sp, 1, ref.at, dis.at, n_frames, out, 1, [&] {
    return sp->tile > 64 || !tile_size_ok((int)sp->tile) ? fail(c, PQA_EINVAL, "tile_moments: tile %u is not 8, 16, 32 or 64", sp->tile) : PQA_OK;
  });
  if (rc != PQA_OK) return rc;
  const int w = (int)sp->width, h = (int)sp->height, tile = (int)sp->tile;
  const size_t per_frame = tile_out_bytes(w, h, tile, 1) / sizeof(uint64_t);
  const PairJob j{"tile_moments", host::plane_clip((size_t)w * c->esize, h), n_frames, kTileChunk, 0, SIDE_TILE_OUT, tile_out_bytes(w, h, tile, n_frames), out};
  return pair_run(c, j, ref, &dis, [&](const PlaneRun* r, const PlaneRun* d, int n, int at) {
    return launch_tile_moments(c->stream, c->elem, (int)c->cfg.bit_depth, r->base, r->row_pitch, r->frame_pitch, d->base, d->row_pitch,
                               d->frame_pitch, n, w, h, tile, (unsigned long long*)c->side_buf[SIDE_TILE_OUT] + (size_t)at * per_frame);
  });
}

// distortion spectrum (band_moments.hip); the launches share the workgroups' partial sums of a chunk
template <class Clip>
int band_moments(pqa_ctx* c, const pqa_band_spec* sp, const Clip& ref, const Clip& dis, int32_t n_frames, uint64_t* out) {
  const int rc = spec_check(c, "band_moments", sp, 1, ref.at, dis.at, n_frames, out, 1, [&] {
    return sp->levels > 6 || !band_levels_ok((int)sp->levels) ? fail(c, PQA_EINVAL, "band_moments: %u levels outside 1 ... 6", sp->levels) : PQA_OK;
  });
  if (rc != PQA_OK) return rc;
  const int w = (int)sp->width, h = (int)sp->height, levels = (int)sp->levels;
  const size_t per_frame = band_out_bytes(levels, 1) / sizeof(uint64_t);
  const PairJob j{"band_moments", host::plane_clip((size_t)w * c->esize, h), n_frames, kBandChunk, 0, SIDE_BAND_OUT, band_out_bytes(levels, n_frames), out, true, SIDE_BAND_PART,
                  band_part_bytes(w, h, levels, n_frames < kBandChunk ? n_frames : kBandChunk)};
  return pair_run(c, j, ref, &dis, [&](const PlaneRun* r, const PlaneRun* d, int n, int at) {
    return launch_band_moments(c->stream, c->elem, (int)c->cfg.bit_depth, r->base, r->row_pitch, r->frame_pitch, d->base, d->row_pitch,
                               d->frame_pitch, n, w, h, levels, c->side_buf[SIDE_BAND_PART],
                               (unsigned long long*)c->side_buf[SIDE_BAND_OUT] + (size_t)at * per_frame);
  });
}

// temporal distortion (temporal_moments.hip): a result per transition, so `out` may be null below two frames
template <class Clip>
int temporal_moments(pqa_ctx* c, const pqa_temporal_spec* sp, const Clip& ref, const Clip& dis, int32_t n_frames, uint64_t* out) {
  const int rc = spec_check(c, "temporal_moments", sp, 1, ref.at, dis.at, n_frames, out, 2, [&] {
    return sp->tile > 64 || !tile_size_ok((int)sp->tile) ? fail(c, PQA_EINVAL, "temporal_moments: tile %u is not 8, 16, 32 or 64", sp->tile) : PQA_OK;
  });
  if (rc != PQA_OK) return rc;
  const int w = (int)sp->width, h = (int)sp->height, tile = (int)sp->tile;
  const size_t per_transition = temporal_out_bytes(w, h, tile, 2) / sizeof(uint64_t);
  const PairJob j{"temporal_moments", host::plane_clip((size_t)w * c->esize, h), n_frames, kTemporalChunk, 1, SIDE_TEMPORAL_OUT, temporal_out_bytes(w, h, tile, n_frames), out};
  return pair_run(c, j, ref, &dis, [&](const PlaneRun* r, const PlaneRun* d, int n, int at) {
    return launch_temporal_moments(c->stream, c->elem, (int)c->cfg.bit_depth, r->base, r->row_pitch, r->frame_pitch, d->base, d->row_pitch,
                                   d->frame_pitch, n, w, h, tile, c->temporal_walk,
                                   (unsigned long long*)c->side_buf[SIDE_TEMPORAL_OUT] + (size_t)at * per_transition);
  });
}

// field alignment (field_moments.hip): a result per transition, so `out` may be null below two frames; a plane has a row pair
template <class Clip>
int field_moments(pqa_ctx* c, const pqa_field_spec* sp, const Clip& ref, const Clip& dis, int32_t n_frames, uint64_t* out) {
  const int rc = spec_check(c, "field_moments", sp, 1, ref.at, dis.at, n_frames, out, 2, [&] {
    return sp->height < 2 ? fail(c, PQA_EINVAL, "field_moments: height %u has no row pair", sp->height) : PQA_OK;
  });
  if (rc != PQA_OK) return rc;
  const int w = (int)sp->width, h = (int)sp->height;
  const PairJob j{"field_moments", host::plane_clip((size_t)w * c->esize, h), n_frames, kFieldChunk, 1, SIDE_FIELD_OUT, field_out_bytes(n_frames), out};
  return pair_run(c, j, ref, &dis, [&](const PlaneRun* r, const PlaneRun* d, int n, int at) {
    return launch_field_moments(c->stream, c->elem, (int)c->cfg.bit_depth, r->base, r->row_pitch, r->frame_pitch, d->base, d->row_pitch,
                                d->frame_pitch, n, w, h, (unsigned long long*)c->side_buf[SIDE_FIELD_OUT] + (size_t)at * kFieldSums);
  });
}

// coding-grid detection (edge_profiles.hip)
template <class Clip>
int edge_profiles(pqa_ctx* c, const pqa_edge_spec* sp, const Clip& ref, const Clip& dis, int32_t n_frames, uint64_t* out) {
  const int rc = spec_check(c, "edge_profiles", sp, 1, ref.at, dis.at, n_frames, out, 1, [] { return PQA_OK; });
  if (rc != PQA_OK) return rc;
  const int w = (int)sp->width, h = (int)sp->height;
  const size_t per_frame = edge_out_bytes(w, h, 1) / sizeof(uint64_t);
  const PairJob j{"edge_profiles", host::plane_clip((size_t)w * c->esize, h), n_frames, kEdgeChunk, 0, SIDE_EDGE_OUT, edge_out_bytes(w, h, n_frames), out};
  return pair_run(c, j, ref, &dis, [&](const PlaneRun* r, const PlaneRun* d, int n, int at) {
    return launch_edge_profiles(c->stream, c->elem, (int)c->cfg.bit_depth, r->base, r->row_pitch, r->frame_pitch, d->base, d->row_pitch,
                                d->frame_pitch, n, w, h, (unsigned long long*)c->side_buf[SIDE_EDGE_OUT] + (size_t)at * per_frame);
  });
}

// active-picture detection (line_profiles.hip): one clip; a stride that is no multiple of the sample size passes here too
template <class Clip>
int line_profiles(pqa_ctx* c, const pqa_profile_spec* sp, const Clip& planes, int32_t n_frames, uint64_t* out) {
  const int rc = spec_check(c, "line_profiles", sp, 1, planes.at, planes.at, n_frames, out, 1, [] { return PQA_OK; });
  if (rc != PQA_OK) return rc;
  const int w = (int)sp->width, h = (int)sp->height;
  const size_t per_frame = profile_out_bytes(w, h, 1) / sizeof(uint64_t);
  const PairJob j{"line_profiles", host::plane_clip((size_t)w * c->esize, h), n_frames, kProfChunk, 0, SIDE_PROF_OUT, profile_out_bytes(w, h, n_frames), out, false};
  return pair_run(c, j, planes, (const Clip*)nullptr, [&](const PlaneRun* r, const PlaneRun*, int n, int at) {
    return launch_line_profiles(c->stream, c->elem, (int)c->cfg.bit_depth, r->base, r->row_pitch, r->frame_pitch, n, w, h,
                                (unsigned long long*)c->side_buf[SIDE_PROF_OUT] + (size_t)at * per_frame);
  });
}

// ---- the analyses of a plane of the context's size (pair_run above) ---------------------------------------------------------------
// pqa_luma_stats, pqa_shift_sse and pqa_level_stats are older than spec_check: each has its own rules (sh_check, lv_check, the
// entries' "bad argument") and keeps what it has always answered (PairJob: bottom_up, row_holds, bare).  A launch of the entry
// for clips in HBM takes what it always took; host frames travel ctx_chunk() at a time.
host::ClipLayout ctx_plane(const pqa_ctx* c, int plane) { return host::plane_clip((size_t)c->pw[plane] * c->esize, c->ph[plane]); }

// luma statistics (luma_stats.hip): one clip
template <class Clip>
int luma_stats(pqa_ctx* c, const Clip& luma, int32_t n_frames, uint32_t threshold, uint64_t* out) {
  const int gray_bpc = c->luma_gray == PQA_GRAY_BT601_FULL ? (int)c->cfg.bit_depth : 0;
  PairJob j{"luma_stats", ctx_plane(c, 0), n_frames, kHostFrames<Clip> ? ctx_chunk(c) : c->B, 0, SIDE_LUMA_OUT, (size_t)n_frames * 3 * sizeof(uint64_t), out, false};
  j.bottom_up = j.bare = true;
  j.row_holds = false;
  return pair_run(c, j, luma, (const Clip*)nullptr, [&](const PlaneRun* r, const PlaneRun*, int n, int at) {
    return launch_luma_stats(c->stream, c->elem, *r, n, c->pw[0], c->ph[0], threshold, gray_bpc, c->luma_part,
                             (unsigned long long*)c->side_buf[SIDE_LUMA_OUT] + (size_t)at * 3);
  });
}

// spatial alignment (shift_sse.hip); no frames: PQA_OK before a pitch or a stride is looked at
template <class Clip>
int shift_sse(pqa_ctx* c, const Clip& ref, const Clip& dis, int32_t n_frames, int32_t radius, uint64_t* out) {
  const int rc = sh_check(c, ref.at, dis.at, n_frames, radius, out);
  if (rc != PQA_OK || n_frames == 0) return rc;
  const size_t per_frame = (size_t)(2 * radius + 1) * (2 * radius + 1);
  const int chunk = kHostFrames<Clip> ? ctx_chunk(c) : kShiftChunk;
  PairJob j{"shift_sse", ctx_plane(c, 0), n_frames, chunk, 0, SIDE_SHIFT_OUT, (size_t)n_frames * per_frame * sizeof(uint64_t), out, false};
  j.bottom_up = true;
  j.prepare = [&] { return sh_prepare(c, radius, n_frames < chunk ? n_frames : chunk); };
  return pair_run(c, j, ref, &dis, [&](const PlaneRun* r, const PlaneRun* d, int n, int at) {
    return launch_shift_sse(c->stream, c->elem, r->base, r->row_pitch, r->frame_pitch, d->base, d->row_pitch, d->frame_pitch, n, c->pw[0], c->ph[0],
                            radius, c->side_buf[SIDE_SHIFT_PART], (unsigned long long*)c->side_buf[SIDE_SHIFT_ROWSQ],
                            (unsigned long long*)c->side_buf[SIDE_SHIFT_OUT] + (size_t)at * per_frame);
  });
}

// level alignment (level_stats.hip): a plane of the context, at its own size; no frames: as above
template <class Clip>
int level_stats(pqa_ctx* c, const Clip& ref, const Clip& dis, int32_t n_frames, int32_t plane, uint64_t* out) {
  const int rc = lv_check(c, ref.at, dis.at, n_frames, plane, out);
  if (rc != PQA_OK || n_frames == 0) return rc;
  const int bpc = (int)c->cfg.bit_depth;
  const size_t per_frame = (size_t)3 << bpc;
  const PairJob j{"level_stats", ctx_plane(c, plane), n_frames, kHostFrames<Clip> ? ctx_chunk(c) : kLevelChunk, 0, SIDE_LEVEL_OUT, level_out_bytes(bpc, n_frames), out, false};
  return pair_run(c, j, ref, &dis, [&](const PlaneRun* r, const PlaneRun* d, int n, int at) {
    return launch_level_stats(c->stream, c->elem, bpc, r->base, r->row_pitch, r->frame_pitch, d->base, d->row_pitch, d->frame_pitch, n, c->pw[plane],
                              c->ph[plane], (unsigned long long*)c->side_buf[SIDE_LEVEL_OUT] + (size_t)at * per_frame);
  });
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

// A frame of the context's size, all its planes (three here; pqa_frame_sad: one or three), as the host entries stage it: rows
// 16 bytes apart at least and planes 256, so the kernels take their wide loads.
host::ClipLayout cl_frame(const pqa_ctx* c) {
  const size_t rb[3] = {(size_t)c->pw[0] * c->esize, (size_t)c->pw[1] * c->esize, (size_t)c->pw[2] * c->esize};
  return host::clip_layout(c->n_planes, rb, c->ph, 16, 256);
}

// anchored frame differences (integrity.hip): one clip of whole frames against the anchor planes (pitches in bytes), after the
// entry's own rules; `chunk` frames a launch (ig_part holds a batch)
PairJob sad_job(pqa_ctx* c, int32_t n_frames, int chunk, uint64_t* out) {
  return PairJob{"frame_sad", cl_frame(c), n_frames, chunk, 0, SIDE_SAD_OUT, (size_t)n_frames * 3 * sizeof(uint64_t), out, false};
}
auto sad_launch(pqa_ctx* c, const void* const* anchor, const int64_t* anchor_pitch_bytes) {
  return [=](const PlaneRun* cur, const PlaneRun*, int n, int at) {
    int64_t app[3] = {0, 0, 0};
    for (int p = 0; p < c->n_planes; ++p) app[p] = anchor_pitch_bytes[p] / c->esize;
    return launch_integrity(c->stream, c->elem, cur, anchor, app, c->pw, c->ph, c->n_planes, n, true, c->black_thr, c->ig_part, nullptr, 0, 0, 1,
                            (unsigned long long*)c->side_buf[SIDE_SAD_OUT] + (size_t)at * 3);
  };
}

// ---- the plane transforms: n frames of a source clip to n frames of a destination clip ----------------------------------------
// pqa_resample, pqa_unpack, pqa_format_convert, pqa_rgb_convert, pqa_table_apply, pqa_mask_blend and pqa_colour_apply differ in
// their rules, their layouts and their launch; one driver for clips in HBM and one for host frames, which an entry reaches
// after its rules.  front() queues what the launches read besides the frames (a table, a node grid) in front of the first;
// launch(source, second input, destination, n frames) queues a kernel on clips in HBM (pitches in bytes).
struct TransformJob {
  const char* who;
  int32_t n_frames;
  int cap, chunk;                  // frames per launch of clips in HBM; host frames per chunk
  host::ClipLayout S, D;           // host frames: a source and a destination frame as they are staged
  int dst_step = 1;                // host frames: pointers per destination frame
  bool in_place = false;           // host frames: the launch leaves the result where the source was uploaded (pqa_mask_blend)
  SideBuf side_buf = kSideBufs;    // what front() uploads into, of side_bytes
  size_t side_bytes = 0;
  int per = 1;                     // a windowed launch: destination frames per source frame
};
const auto no_front = [] { return hipSuccess; };
// A launch with a window in time (pqa_deinterlace) is launch(clip, destination, count, t0, m): the outputs of the m source frames
// from the t0-th on of the `count` frames of `clip`, whose neighbours in time it reads and clamps to the clip itself, go to
// `destination`, per frames each.
template <class Launch>
constexpr bool kWindowed = std::is_invocable<Launch, const pqa_device_clip&, const pqa_device_clip&, int, int, int>::value;

template <class Front, class Launch>
int transform_run(pqa_ctx* c, const TransformJob& j, const pqa_device_clip& src, const pqa_device_clip* aux, const pqa_device_clip& dst,
                  Front front, Launch launch) {
  HIPCHK(c, hipSetDevice(c->device));
  const int rc = j.side_buf != kSideBufs ? side_reserve(c, j.side_buf, j.side_bytes) : PQA_OK;
  if (rc != PQA_OK) return rc;
  hipError_t e = front();
  if (e == hipSuccess)
    e = launch_runs(j.n_frames, j.cap, nullptr, [&](int f0, int n) {
      if constexpr (kWindowed<Launch>) return launch(src, clip_from(dst, f0 * j.per), j.n_frames, f0, n);
      else return launch(clip_from(src, f0), aux ? clip_from(*aux, f0) : pqa_device_clip{}, clip_from(dst, f0), n);
    });
  return side_finish(c, j.who, e, nullptr, nullptr, 0);
}

// Host frames travel as host::transform_walk lays out: a chunk goes out through the first of the side analyses' two pinned
// chunks into SIDE_STAGE_A (a second input behind it, into SIDE_STAGE_B), the launch writes SIDE_STAGE_B (in_place: blends
// where the source lies; a second input needs that), and the result comes back through the second pinned chunk and is copied
// out before the next chunk is packed: one side_finish per chunk.  Rows lie 16 bytes apart at least, so the kernels' wide
// paths apply.  Nothing in the staging buffers outlives the call.  A windowed launch (kWindowed; it has no front and no second
// input) travels as host::window_walk lays out instead: SIDE_STAGE_A holds two slots more than a chunk, the last two frames of a
// chunk stay there as the predecessors of the next, and a chunk brings back the outputs of up to a chunk plus one source frames.
template <class Front, class Launch>
int transform_run(pqa_ctx* c, const TransformJob& j, const HostClip& src, const HostClip* aux, const HostClip& dst, Front front, Launch launch) {
  HIPCHK(c, hipSetDevice(c->device));
  constexpr bool windowed = kWindowed<Launch>;   // host::window_walk: two slots of predecessors, a launch one source frame late
  const size_t slots = (size_t)(j.n_frames < j.chunk ? j.n_frames : j.chunk), sb = j.S.frame_bytes * slots,
               db = j.D.frame_bytes * (slots + (windowed ? 1 : 0)) * j.per;
  int rc = side_pin_reserve(c, 0, sb * (aux ? 2 : 1));
  if (rc == PQA_OK) rc = side_pin_reserve(c, 1, db);
  if (rc == PQA_OK && j.side_buf != kSideBufs) rc = side_reserve(c, j.side_buf, j.side_bytes);
  if (rc == PQA_OK) rc = side_reserve(c, SIDE_STAGE_A, sb + (windowed ? 2 * j.S.frame_bytes : 0));
  if (rc == PQA_OK && (aux || !j.in_place)) rc = side_reserve(c, SIDE_STAGE_B, aux ? sb : db);
  if (rc != PQA_OK) return rc;
  void* const a = c->side_buf[SIDE_STAGE_A];
  void* const b = c->side_buf[SIDE_STAGE_B];
  const pqa_device_clip s = staged_clip(j.S, a), x = aux ? staged_clip(j.S, b) : pqa_device_clip{}, d = staged_clip(j.D, j.in_place ? a : b);
  const auto finish = [&](hipError_t e, int n) { return side_finish(c, j.who, e, c->side_pin[1], d.plane[0], j.D.frame_bytes * n); };
  if constexpr (windowed) {
    const size_t fb = j.S.frame_bytes;
    return host::window_walk(
        j.S, j.D, c->side_pin, src.at, src.strides, (void* const*)dst.at, dst.strides, j.dst_step, j.n_frames, j.chunk, j.per,
        [&](int from_slot) { return hipMemcpyAsync(a, (const uint8_t*)a + fb * from_slot, 2 * fb, hipMemcpyDeviceToDevice, c->stream); },
        [&](int slot, int n) { return hipMemcpyAsync((uint8_t*)a + fb * slot, c->side_pin[0], fb * n, hipMemcpyHostToDevice, c->stream); },
        [&](int slot, int count, int t0, int m) { return launch(clip_from(s, slot), d, count, t0, m); }, finish);
  } else {
    return host::transform_walk(
        j.S, j.D, c->side_pin, src.at, src.strides, aux ? aux->at : nullptr, aux ? aux->strides : nullptr, (void* const*)dst.at, dst.strides,
        j.dst_step, j.n_frames, j.chunk,
        [&](int f0, int n) {
          hipError_t e = f0 == 0 ? front() : hipSuccess;
          if (e == hipSuccess) e = hipMemcpyAsync(a, c->side_pin[0], j.S.frame_bytes * n, hipMemcpyHostToDevice, c->stream);
          if (e == hipSuccess && aux) e = hipMemcpyAsync(b, c->side_pin[0] + sb, j.S.frame_bytes * n, hipMemcpyHostToDevice, c->stream);
          return e;
        },
        [&](int n) { return launch(s, x, d, n); }, finish);
  }
}

// The destination rules that pqa_unpack[_device] and pqa_rgb_convert[_device] share, after `cancelled` (no device call).  A
// destination has a luma plane of w samples a row and, or not, two chroma planes of cw; samples of es bytes.  aligned: the name
// of a format whose source must lie on 4 bytes ("v210", "r210"), or null.  *np: 1 or 3.
int packed_dst_check(pqa_ctx* c, const char* who, const char* aligned, const void* src, const pqa_device_clip* dst, int es, int w, int cw, int* np) {
  if (!dst->plane[0]) return fail(c, PQA_EINVAL, "%s: null luma destination", who);
  if (!dst->plane[1] != !dst->plane[2]) return fail(c, PQA_EINVAL, "%s: chroma destinations: both or neither", who);
  if (aligned && ((uintptr_t)src & 3)) return fail(c, PQA_EINVAL, "%s: %s source is not 4-byte aligned", who, aligned);
  *np = dst->plane[1] ? 3 : 1;
  for (int p = 0; p < *np; ++p) {
    if (!whole_samples(dst->plane[p], dst->row_pitch[p], dst->frame_pitch[p], es))
      return fail(c, PQA_EINVAL, "%s: plane %d destination is not made of whole samples", who, p);
    if (dst->row_pitch[p] < (int64_t)(p ? cw : w) * es) return fail(c, PQA_EINVAL, "%s: plane %d destination pitch smaller than a row", who, p);
  }
  return PQA_OK;
}
// whole_strides: refuse a destination stride that is not whole samples (pqa_rgb_convert does, pqa_unpack does not)
int packed_dst_check(pqa_ctx* c, const char* who, const char* aligned, const void* const* src_frames, void* const* dst_planes,
                     const int64_t dst_strides[3], int32_t n_frames, int es, int w, int cw, bool whole_strides, int* np) {
  if (!dst_strides) return fail(c, PQA_EINVAL, "%s: null destination strides", who);
  *np = dst_planes[1] && dst_planes[2] ? 3 : 1;
  if (*np == 1 && (dst_planes[1] || dst_planes[2])) return fail(c, PQA_EINVAL, "%s: chroma destinations: both or neither", who);
  for (int f = 0; f < n_frames; ++f) {   // before anything is queued
    if (!src_frames[f]) return fail(c, PQA_EINVAL, "%s: source frame %d pointer is null", who, f);
    if (aligned && ((uintptr_t)src_frames[f] & 3)) return fail(c, PQA_EINVAL, "%s: %s source frame %d is not 4-byte aligned", who, aligned, f);
    for (int p = 0; p < *np; ++p)
      if (!dst_planes[(size_t)f * 3 + p]) return fail(c, PQA_EINVAL, "%s: destination plane %d of frame %d is null", who, p, f);
  }
  for (int p = 0; p < *np; ++p) {
    if (whole_strides && (dst_strides[p] & (int64_t)(es - 1))) return fail(c, PQA_EINVAL, "%s: plane %d destination is not made of whole samples", who, p);
    if (dst_strides[p] < (int64_t)(p ? cw : w) * es) return fail(c, PQA_EINVAL, "%s: plane %d destination stride smaller than a row", who, p);
  }
  return PQA_OK;
}

// ---- the transforms and the three-plane analyses: the rules an entry pair shares and one body for both (entries below) ------------

// resampler (resample.hip)
template <class Clip>
int resample_run(pqa_ctx* c, const pqa_resample_spec* sp, int slot, const Clip& src, const Clip& dst, int32_t n_frames) {
  const int es = c->esize, sw = (int)sp->src_width, sh = (int)sp->src_height, dw = (int)sp->dst_width, dh = (int)sp->dst_height;
  const TransformJob j{"resample", n_frames, kRsChunk, kRsChunk, host::plane_clip((size_t)sw * es, sh), host::plane_clip((size_t)dw * es, dh)};
  return transform_run(c, j, src, nullptr, dst, no_front, [&](const pqa_device_clip& s, const pqa_device_clip&, const pqa_device_clip& d, int n) {
    return launch_resample(c->stream, c->elem, (int)c->cfg.bit_depth, c->rs_cache[slot].plan, (const int*)c->side_buf[SIDE_RS_TABLE0 + slot],
                           s.plane[0], s.row_pitch[0] / es, s.frame_pitch[0] / es, sw, sh, const_cast<void*>(d.plane[0]), d.row_pitch[0] / es,
                           d.frame_pitch[0] / es, dw, dh, n);
  });
}

// The argument rules both entries share, in spec_check's order (no device call); then the rows of the packed source.
int unpack_check(pqa_ctx* c, const pqa_unpack_spec* sp, const void* src, const void* dst, int32_t n_frames, int64_t src_row,
                 int64_t src_frame) {
  const int rc = spec_check(c, "unpack", sp, 1, src, dst, n_frames, sp, 1, [&] {
    return host::packed_format(sp->format) ? PQA_OK : fail(c, PQA_EINVAL, "unpack: format %u is not a packed capture format (UYVY 3, YUYV 4, V210 5)", sp->format);
  });
  if (rc != PQA_OK || n_frames == 0) return rc;
  const int64_t min_row = host::packed_min_row_bytes(sp->format, (int)sp->width);
  if (src_row < min_row)
    return fail(c, PQA_EINVAL, "unpack: source pitch %lld is smaller than a packed row of %lld bytes", (long long)src_row, (long long)min_row);
  if (sp->format == PQA_SURFACE_V210 && ((src_row | src_frame) & 3)) return fail(c, PQA_EINVAL, "unpack: v210 pitch is not a multiple of 4");
  return PQA_OK;
}

// np: the planes of the destination, 1 or 3
template <class Clip>
int unpack_run(pqa_ctx* c, const pqa_unpack_spec* sp, int np, const Clip& src, const Clip& dst, int32_t n_frames) {
  const int w = (int)sp->width, h = (int)sp->height;
  const TransformJob j{"unpack", n_frames, kFrameCap, kRsChunk, host::packed_layout(sp->format, w, h), host::unpacked_layout(sp->format, w, h, np), 3};
  return transform_run(c, j, src, nullptr, dst, no_front, [&](const pqa_device_clip& s, const pqa_device_clip&, const pqa_device_clip& d, int n) {
    void* const at[3] = {const_cast<void*>(d.plane[0]), const_cast<void*>(d.plane[1]), const_cast<void*>(d.plane[2])};
    return launch_unpack(c->stream, (int)sp->format, s.plane[0], s.row_pitch[0], s.frame_pitch[0], at, d.row_pitch, d.frame_pitch, w, h, n);
  });
}

// The argument rules both entries share, in spec_check's order (no device call).
int convert_check(pqa_ctx* c, const pqa_convert_spec* sp, const void* src, const void* dst, int32_t n_frames) {
  return spec_check(c, "format_convert", sp, 1, src, dst, n_frames, sp, 1, [&] {
    if (sp->flags & ~(uint32_t)PQA_CONVERT_GENERIC) return fail(c, PQA_EINVAL, "format_convert: unknown flag bits %#x", sp->flags);
    for (uint32_t b : {sp->src_bits, sp->dst_bits})
      if (b != 8 && b != 10 && b != 12) return fail(c, PQA_EINVAL, "format_convert: bit depth %u is not 8, 10 or 12", b);
    for (uint8_t s : {sp->src_hshift, sp->src_vshift, sp->dst_hshift, sp->dst_vshift})
      if (s > 2) return fail(c, PQA_EINVAL, "format_convert: chroma shift %u outside 0 ... 2", (unsigned)s);
    for (uint8_t s : {sp->src_hsite, sp->src_vsite, sp->dst_hsite, sp->dst_vsite})
      if (s != PQA_SITE_COSITED && s != PQA_SITE_CENTRE) return fail(c, PQA_EINVAL, "format_convert: siting %u is not PQA_SITE_COSITED or _CENTRE", (unsigned)s);
    return (int)PQA_OK;
  });
}
ConvertLayout convert_side(const pqa_convert_spec* sp, bool dst) {
  return dst ? ConvertLayout{(int)sp->dst_bits, sp->dst_hshift, sp->dst_vshift, sp->dst_hsite, sp->dst_vsite}
             : ConvertLayout{(int)sp->src_bits, sp->src_hshift, sp->src_vshift, sp->src_hsite, sp->src_vsite};
}

struct ConvertPlanes {   // the source and the destination plane of a spec: layouts, bytes of a row, rows
  ConvertLayout S, D;
  size_t src_row, dst_row;
  int src_h, dst_h;
};
ConvertPlanes convert_planes(const pqa_convert_spec* sp) {
  const ConvertLayout S = convert_side(sp, false), D = convert_side(sp, true);
  const int lw = (int)sp->luma_width, lh = (int)sp->luma_height;
  return ConvertPlanes{S, D, (size_t)convert_plane_size(lw, S.hshift) * (S.bits > 8 ? 2 : 1), (size_t)convert_plane_size(lw, D.hshift) * (D.bits > 8 ? 2 : 1),
                       convert_plane_size(lh, S.vshift), convert_plane_size(lh, D.vshift)};
}
template <class Clip>
int convert_run(pqa_ctx* c, const pqa_convert_spec* sp, const ConvertPlanes& P, const Clip& src, const Clip& dst, int32_t n_frames) {
  const TransformJob j{"format_convert", n_frames, kFrameCap, kConvertChunk, host::plane_clip(P.src_row, P.src_h), host::plane_clip(P.dst_row, P.dst_h)};
  return transform_run(c, j, src, nullptr, dst, no_front, [&](const pqa_device_clip& s, const pqa_device_clip&, const pqa_device_clip& d, int n) {
    return launch_format_convert(c->stream, P.S, P.D, (int)sp->luma_width, (int)sp->luma_height, (sp->flags & PQA_CONVERT_GENERIC) != 0, s.plane[0],
                                 s.row_pitch[0], s.frame_pitch[0], const_cast<void*>(d.plane[0]), d.row_pitch[0], d.frame_pitch[0], n);
  });
}

// The argument rules both entries share, in spec_check's order (no device call); then the rows of the packed source.
int rgb_check(pqa_ctx* c, const pqa_rgb_spec* sp, const void* src, const void* dst, int32_t n_frames, int64_t src_row, int64_t src_frame) {
  const int rc = spec_check(c, "rgb_convert", sp, 1, src, dst, n_frames, sp, 1, [&] {
    if (!host::rgb_format(sp->format))
      return fail(c, PQA_EINVAL, "rgb_convert: format %u is not a packed RGB format (BGRA 6, ARGB 7, RGBA 8, ABGR 9, R210 10)", sp->format);
    if (sp->flags & ~(uint32_t)PQA_RGB_GENERIC) return fail(c, PQA_EINVAL, "rgb_convert: unknown flag bits %#x", sp->flags);
    if (sp->dst_bits != 8 && sp->dst_bits != 10) return fail(c, PQA_EINVAL, "rgb_convert: destination bit depth %u is not 8 or 10", sp->dst_bits);
    for (uint32_t s : {sp->hshift, sp->vshift})
      if (s > 1) return fail(c, PQA_EINVAL, "rgb_convert: chroma shift %u outside 0 ... 1", s);
    for (uint32_t s : {sp->hsite, sp->vsite})
      if (s != PQA_SITE_COSITED && s != PQA_SITE_CENTRE) return fail(c, PQA_EINVAL, "rgb_convert: siting %u is not PQA_SITE_COSITED or _CENTRE", s);
    if (!host::rgb_matrix_fits(sp->m, host::rgb_bit_depth(sp->format), (int)sp->hshift, (int)sp->vshift))
      return fail(c, PQA_EINVAL, "rgb_convert: the matrix leaves int32 (extreme |A| times the tap sum %d plus the rounding half reaches 2^31)",
                  1 << (3 * (sp->hshift + sp->vshift)));
    return (int)PQA_OK;
  });
  if (rc != PQA_OK || n_frames == 0) return rc;
  const int64_t min_row = host::rgb_min_row_bytes((int)sp->width);
  if (src_row < min_row)
    return fail(c, PQA_EINVAL, "rgb_convert: source pitch %lld is smaller than a packed row of %lld bytes", (long long)src_row, (long long)min_row);
  if (sp->format == PQA_SURFACE_R210 && ((src_row | src_frame) & 3)) return fail(c, PQA_EINVAL, "rgb_convert: r210 pitch is not a multiple of 4");
  return PQA_OK;
}
ConvertLayout rgb_side(const pqa_rgb_spec* sp) {
  return ConvertLayout{(int)sp->dst_bits, (int)sp->hshift, (int)sp->vshift, (int)sp->hsite, (int)sp->vsite};
}

// np: the planes of the destination, 1 or 3
template <class Clip>
int rgb_run(pqa_ctx* c, const pqa_rgb_spec* sp, int np, const Clip& src, const Clip& dst, int32_t n_frames) {
  const ConvertLayout D = rgb_side(sp);
  const int w = (int)sp->width, h = (int)sp->height;
  const TransformJob j{"rgb_convert", n_frames, kFrameCap, kRgbChunk, host::rgb_layout(w, h),
                       host::converted_layout(w, h, convert_plane_size(w, D.hshift), convert_plane_size(h, D.vshift), D.bits > 8 ? 2 : 1, np), 3};
  return transform_run(c, j, src, nullptr, dst, no_front, [&](const pqa_device_clip& s, const pqa_device_clip&, const pqa_device_clip& d, int n) {
    void* const at[3] = {const_cast<void*>(d.plane[0]), const_cast<void*>(d.plane[1]), const_cast<void*>(d.plane[2])};
    return launch_rgb_convert(c->stream, (int)sp->format, D, (sp->flags & PQA_RGB_GENERIC) != 0, sp->m, s.plane[0], s.row_pitch[0], s.frame_pitch[0], at,
                              d.row_pitch, d.frame_pitch, w, h, n);
  });
}

// The argument rules both entries share, in spec_check's order and then the table's (no device call).
int table_check(pqa_ctx* c, const pqa_table_spec* sp, const void* table, const void* src, const void* dst, int32_t n_frames) {
  const int rc = spec_check(c, "table_apply", sp, 1, src, dst, n_frames, sp, 1, [] { return (int)PQA_OK; });
  if (rc != PQA_OK) return rc;
  if (!table) return fail(c, PQA_EINVAL, "table_apply: null table");
  const unsigned top = (1u << c->cfg.bit_depth) - 1u;
  for (unsigned v = 0; v <= top; ++v) {
    const unsigned t = c->esize == 1 ? ((const uint8_t*)table)[v] : ((const uint16_t*)table)[v];
    if (t > top) return fail(c, PQA_EINVAL, "table_apply: table entry %u is %u, above %u", v, t, top);
  }
  return PQA_OK;
}
// the table onto the stream, in front of the launches that read it; pageable memory: the copy has left `table` on return
hipError_t table_upload(pqa_ctx* c, const void* table) {
  return hipMemcpyAsync(c->side_buf[SIDE_TABLE_LUT], table, ((size_t)c->esize) << c->cfg.bit_depth, hipMemcpyHostToDevice, c->stream);
}

template <class Clip>
int table_run(pqa_ctx* c, const pqa_table_spec* sp, const void* table, const Clip& src, const Clip& dst, int32_t n_frames) {
  const int w = (int)sp->width, h = (int)sp->height;
  const host::ClipLayout P = host::plane_clip((size_t)w * c->esize, h);
  const TransformJob j{"table_apply", n_frames, kFrameCap, kTableChunk, P, P, 1, false, SIDE_TABLE_LUT, (size_t)c->esize << c->cfg.bit_depth};
  return transform_run(c, j, src, nullptr, dst, [&] { return table_upload(c, table); },
                       [&](const pqa_device_clip& s, const pqa_device_clip&, const pqa_device_clip& d, int n) {
                         return launch_table_apply(c->stream, c->elem, (int)c->cfg.bit_depth, c->side_buf[SIDE_TABLE_LUT], s.plane[0], s.row_pitch[0],
                                                   s.frame_pitch[0], const_cast<void*>(d.plane[0]), d.row_pitch[0], d.frame_pitch[0], n, w, h);
                       });
}

// deinterlacer (deinterlace.hip).  The argument rules both entries share, in spec_check's order (no device call); a plane has a
// row of each parity from height 2 on.
int deint_check(pqa_ctx* c, const pqa_deint_spec* sp, const void* src, const void* dst, int32_t n_frames) {
  return spec_check(c, "deinterlace", sp, 1, src, dst, n_frames, sp, 1, [&] {
    if (sp->mode > 1) return fail(c, PQA_EINVAL, "deinterlace: bad mode %u", sp->mode);
    if (sp->first > 1) return fail(c, PQA_EINVAL, "deinterlace: bad first %u", sp->first);
    if (sp->rate > 1) return fail(c, PQA_EINVAL, "deinterlace: bad rate %u", sp->rate);
    return sp->height == 1 ? fail(c, PQA_EINVAL, "deinterlace: height 1 has one field only") : (int)PQA_OK;
  });
}

template <class Clip>
int deint_run(pqa_ctx* c, const pqa_deint_spec* sp, const Clip& src, const Clip& dst, int32_t n_frames) {
  const int w = (int)sp->width, h = (int)sp->height;
  const host::ClipLayout P = host::plane_clip((size_t)w * c->esize, h);
  TransformJob j{"deinterlace", n_frames, kDeintChunk, kDeintChunk, P, P};
  j.per = 1 + (int)sp->rate;
  return transform_run(c, j, src, nullptr, dst, no_front, [&](const pqa_device_clip& s, const pqa_device_clip& d, int count, int t0, int m) {
    return launch_deinterlace(c->stream, c->elem, (int)c->cfg.bit_depth, (int)sp->mode, (int)sp->first, j.per, c->deint_uniform, s.plane[0],
                              s.row_pitch[0], s.frame_pitch[0], count, t0, m, const_cast<void*>(d.plane[0]), d.row_pitch[0], d.frame_pitch[0], w, h);
  });
}

// The argument rules both entries share, in spec_check's order and then the grid's (no device call); bounds: what one pass over the grid tells (kernels.h).
int mask_check(pqa_ctx* c, const pqa_mask_spec* sp, const uint16_t* nodes, const void* src, const void* dst, int32_t n_frames, MaskBounds* bounds) {
  const int rc = spec_check(c, "mask_blend", sp, 1, src, dst, n_frames, sp, 1, [&] {
    if (sp->step_log2_x > (uint32_t)kMaskMaxStep || sp->step_log2_y > (uint32_t)kMaskMaxStep)
      return fail(c, PQA_EINVAL, "mask_blend: steps %u, %u above %d", sp->step_log2_x, sp->step_log2_y, kMaskMaxStep);
    const uint32_t top = (1u << c->cfg.bit_depth) - 1u;
    return sp->fill > top ? fail(c, PQA_EINVAL, "mask_blend: fill %u above %u", sp->fill, top) : (int)PQA_OK;
  });
  if (rc != PQA_OK) return rc;
  if (!nodes) return fail(c, PQA_EINVAL, "mask_blend: null node grid");
  if (!mask_node_bounds(nodes, (int)sp->width, (int)sp->height, (int)sp->step_log2_x, (int)sp->step_log2_y, bounds))
    return fail(c, PQA_EINVAL, "mask_blend: a node is above 256");
  return PQA_OK;
}
size_t mask_node_bytes(const pqa_mask_spec* sp) {
  return (size_t)mask_grid((int)sp->width, (int)sp->step_log2_x) * mask_grid((int)sp->height, (int)sp->step_log2_y) * sizeof(uint16_t);
}
// the grid's rows that hold a non-zero node onto the stream, at their place in the grid, in front of the launches that read
// them; pageable memory: the copy has left `nodes` on return
hipError_t mask_upload(pqa_ctx* c, const pqa_mask_spec* sp, const uint16_t* nodes, const MaskBounds& b) {
  if (!b.rows) return hipSuccess;
  const size_t gx = (size_t)mask_grid((int)sp->width, (int)sp->step_log2_x), first = (size_t)b.row0 * gx;
  return hipMemcpyAsync((uint16_t*)c->side_buf[SIDE_MASK_NODES] + first, nodes + first, (size_t)b.rows * gx * sizeof(uint16_t),
                        hipMemcpyHostToDevice, c->stream);
}

// fill null: the spec's fill value.  Host frames are blended where they were uploaded: the launch covers the mask's rectangle
// only, the rest of a plane comes back as it went.
template <class Clip>
int mask_run(pqa_ctx* c, const pqa_mask_spec* sp, const uint16_t* nodes, const MaskBounds& bounds, const Clip& src, const Clip* fill, const Clip& dst,
             int32_t n_frames) {
  const int w = (int)sp->width, h = (int)sp->height;
  const host::ClipLayout P = host::plane_clip((size_t)w * c->esize, h);
  const TransformJob j{"mask_blend", n_frames, kFrameCap, kMaskChunk, P, P, 1, true, SIDE_MASK_NODES, mask_node_bytes(sp)};
  return transform_run(c, j, src, fill, dst, [&] { return mask_upload(c, sp, nodes, bounds); },
                       [&](const pqa_device_clip& s, const pqa_device_clip& x, const pqa_device_clip& d, int n) {
                         return launch_mask_blend(c->stream, c->elem, (int)c->cfg.bit_depth, (const uint16_t*)c->side_buf[SIDE_MASK_NODES],
                                                  (int)sp->step_log2_x, (int)sp->step_log2_y, sp->fill, bounds, s.plane[0], s.row_pitch[0],
                                                  s.frame_pitch[0], x.plane[0], x.row_pitch[0], x.frame_pitch[0], const_cast<void*>(d.plane[0]),
                                                  d.row_pitch[0], d.frame_pitch[0], n, w, h);
                       });
}

// colour-matrix alignment (colour_moments.hip)
PairJob colour_job(pqa_ctx* c, int32_t n_frames, uint64_t* out) {
  return PairJob{"colour_moments", cl_frame(c), n_frames, kColourChunk, 0, SIDE_COLOUR_OUT, (size_t)n_frames * kColourSums * sizeof(uint64_t), out, false};
}
// a launch's sums lie `at` frames into the output buffer
auto colour_launch(pqa_ctx* c, uint32_t lo, uint32_t hi) {
  return [=](const PlaneRun* r, const PlaneRun* d, int n, int at) {
    return launch_colour_moments(c->stream, c->elem, (int)c->cfg.bit_depth, (int)c->cfg.chroma_hshift, (int)c->cfg.chroma_vshift, r, d, n, c->pw[0],
                                 c->ph[0], lo, hi, (unsigned long long*)c->side_buf[SIDE_COLOUR_OUT] + (size_t)at * kColourSums);
  };
}
template <class Clip>
int colour_apply_run(pqa_ctx* c, const int32_t m[12], const Clip& src, const Clip& dst, int32_t n_frames) {
  const host::ClipLayout L = cl_frame(c);
  const TransformJob j{"colour_apply", n_frames, kColourChunk, kColourChunk, L, L, 3};
  return transform_run(c, j, src, nullptr, dst, no_front, [&](const pqa_device_clip& s, const pqa_device_clip&, const pqa_device_clip& d, int n) {
    PlaneRun sr[3];
    MutPlaneRun dr[3];
    plane_runs(s, 0, c->esize, sr);
    plane_runs(d, 0, c->esize, dr);
    return launch_colour_apply(c->stream, c->elem, (int)c->cfg.bit_depth, (int)c->cfg.chroma_hshift, (int)c->cfg.chroma_vshift, m, sr, dr, n, c->pw[0], c->ph[0]);
  });
}

// the argument rules both entries share, in the order in which they fire (no device call)
int itp_check(pqa_ctx* c, const pqa_itp_spec* sp, int32_t n_frames) {
  if (!sp) return fail(c, PQA_EINVAL, "delta_itp: null spec");
  if (c->n_planes != 3) return fail(c, PQA_EINVAL, "delta_itp needs the chroma planes: n_planes must be 3 (got %d)", c->n_planes);
  if (c->elem != ELEM_U8 && c->elem != ELEM_U16) return fail(c, PQA_EINVAL, "delta_itp: u8 or u16 samples only");
  if (const char* what = itp_spec_error(*sp)) return fail(c, PQA_EINVAL, "delta_itp: %s", what);
  if (n_frames < 0) return fail(c, PQA_EINVAL, "delta_itp: negative frame count");
  return PQA_OK;
}

// the tiles' partial sums of a chunk are the workspace the launches share
PairJob itp_job(pqa_ctx* c, int32_t n_frames, double* out) {
  const int chunk = n_frames < kItpChunk ? n_frames : kItpChunk;
  return PairJob{"delta_itp", cl_frame(c), n_frames, kItpChunk, 0, SIDE_ITP_OUT, (size_t)n_frames * kItpSums * sizeof(double), out, false, SIDE_ITP_PART,
                 (size_t)chunk * itp_tiles(c->pw[1], c->ph[1]) * kItpSums * sizeof(double)};
}
// kernel and epilogue of n staged or resident frame pairs; their rows go `at` frames into the output buffer
auto itp_launch(pqa_ctx* c, const pqa_itp_spec* sp) {
  ItpCoef k;
  itp_prepare(*sp, &k);
  return [=](const PlaneRun* r, const PlaneRun* d, int n, int at) {
    auto* part = (double*)c->side_buf[SIDE_ITP_PART];
    hipError_t e = launch_delta_itp(c->stream, c->elem, k, r, d, n, c->pw[0], c->ph[0], (int)c->cfg.chroma_hshift, (int)c->cfg.chroma_vshift, part);
    if (e == hipSuccess)
      e = launch_delta_itp_finalize(c->stream, part, itp_tiles(c->pw[1], c->ph[1]), n, (double*)c->side_buf[SIDE_ITP_OUT] + (size_t)at * kItpSums);
    return e;
  };
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
  return pair_run(c, sad_job(c, n_frames, c->B, out), *frames, *frames, nullptr, sad_launch(c, anchor_planes, anchor_row_pitch));
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
  for (int p = 0; p < c->n_planes; ++p) {   // lazily: a healthy clip never asks for an anchored difference
    const int rc = c->ig_anchor[p] ? PQA_OK : dev_alloc(c, &c->ig_anchor[p], (size_t)c->ig_hist[p].pitch * c->ph[p]);
    if (rc != PQA_OK) return rc;
  }
  // the anchor: plain synchronous copies from the caller's (pageable) planes, once a call
  for (int p = 0; p < c->n_planes; ++p)
    HIPCHK(c, hipMemcpy2D(c->ig_anchor[p], c->ig_hist[p].pitch, anchor_planes[p], anchor_strides[p], (size_t)c->pw[p] * c->esize,
                          c->ph[p], hipMemcpyHostToDevice));
  const void* const anchor[3] = {c->ig_anchor[0], c->ig_anchor[1], c->ig_anchor[2]};
  const int64_t anchor_pitch[3] = {c->ig_hist[0].pitch, c->ig_hist[1].pitch, c->ig_hist[2].pitch};
  // The frames take the same synchronous copies into SIDE_STAGE_A, laid out as every staged frame is: for whole frames in one
  // or two chunks the runtime's pageable copy is twice as fast as a pack into a pinned chunk and its upload (DESIGN.md,
  // "The pair staging").  A copy has left the caller's plane on return; a chunk's kernel is waited for before the buffer is
  // written again.
  const PairJob j = sad_job(c, n_frames, ctx_chunk(c), out);
  int rc = side_reserve(c, SIDE_STAGE_A, j.L.frame_bytes * (size_t)(n_frames < j.chunk ? n_frames : j.chunk));
  if (rc == PQA_OK) rc = job_reserve(c, j);
  if (rc != PQA_OK) return rc;
  auto* const stage = (uint8_t*)c->side_buf[SIDE_STAGE_A];
  const auto launch = sad_launch(c, anchor, anchor_pitch);
  PlaneRun cur[3];
  plane_runs(staged_clip(j.L, stage), 0, c->esize, cur);
  hipError_t e = hipSuccess;
  for (int f0 = 0; f0 < n_frames && e == hipSuccess && !c->cancelled.load(); f0 += j.chunk) {
    const int n = chunk_len(n_frames, f0, j.chunk);
    if (f0 > 0) e = hipStreamSynchronize(c->stream);
    for (int f = 0; f < n; ++f)
      for (int p = 0; p < c->n_planes && e == hipSuccess; ++p)   // a frame of the list is three pointers whatever n_planes is
        e = hipMemcpy2D(stage + (size_t)f * j.L.frame_bytes + j.L.off[p], j.L.plane[p].pitch, frames[(size_t)(f0 + f) * 3 + p], strides[p],
                        j.L.plane[p].row_bytes, c->ph[p], hipMemcpyHostToDevice);
    if (e == hipSuccess) e = launch(cur, nullptr, n, f0);
  }
  return side_finish(c, j.who, e, out, c->side_buf[j.out_buf], j.out_bytes);
}

// ---- luma statistics ---------------------------------------------------------------------------------------------------

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
  return luma_stats(c, DevClip{luma, row_pitch, frame_pitch}, n_frames, threshold, out);
}

int pqa_luma_stats(pqa_ctx* c, const void* const* luma_frames, int64_t row_stride, int32_t n_frames, uint32_t threshold,
                   uint64_t* out) {
  if (!c) return PQA_EINVAL;
  if (n_frames < 0 || (n_frames > 0 && (!luma_frames || !out))) return fail(c, PQA_EINVAL, "bad argument");
  return luma_stats(c, HostClip{luma_frames, &row_stride}, n_frames, threshold, out);
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
  const int span = k_hi - k_lo + 1, h = c->ph[0], es = c->esize, chunk = ctx_chunk(c);
  const bool mfma = c->xsse_mfma && c->elem == ELEM_U8;
  const host::ClipLayout L = ctx_plane(c, 0);
  const size_t frame_bytes = L.frame_bytes;
  const int dis_ring = 31 + span;   // the captured frames one reference tile meets
  rc = xs_prepare(c, mfma, span, 1, n_ref, n_dis);
  for (int k = 0; k < 2 && rc == PQA_OK; ++k) rc = side_pin_reserve(c, k, frame_bytes * chunk);
  if (rc == PQA_OK) rc = side_reserve(c, SIDE_XSSE_REF, frame_bytes * 32);
  if (rc == PQA_OK) rc = side_reserve(c, SIDE_XSSE_DIS, frame_bytes * dis_ring);
  if (rc != PQA_OK) return rc;
  const XsseClip ref{c->side_buf[SIDE_XSSE_REF], L.plane[0].pitch / es, (int64_t)(frame_bytes / es), 32, n_ref};
  const XsseClip dis{c->side_buf[SIDE_XSSE_DIS], L.plane[0].pitch / es, (int64_t)(frame_bytes / es), dis_ring, n_dis};
  auto* nr = (unsigned long long*)c->side_buf[SIDE_XSSE_NORM_REF];
  auto* nd = (unsigned long long*)c->side_buf[SIDE_XSSE_NORM_DIS];
  auto* dev_out = (unsigned long long*)c->side_buf[SIDE_XSSE_OUT];
  // Every frame crosses PCIe once: reference tile b replaces tile b - 1 in its 32 slots, and the captured window only ever
  // moves forward, so a tile uploads the captured frames between the previous window's end and its own.  Frames travel in
  // chunks that alternate between the two pinned chunks, each packed once its last upload has left it (pin_wait) and so under
  // the uploads of the chunk before; the stream orders a tile's uploads before its kernels and those before the next tile's
  // uploads into the same slots.
  hipError_t e = hipSuccess;
  int pin = 0;
  const auto live = [&] { return e == hipSuccess && !c->cancelled.load(); };
  const auto upload = [&](const void* const* frames, int64_t stride, const XsseClip& clip, int64_t first, int64_t last,
                          unsigned long long* norms) {   // frames first ... last - 1 into their ring slots
    for (int64_t f0 = first; f0 < last && live(); pin ^= 1) {
      const int n = chunk_len((int)last, (int)f0, chunk);
      e = pin_wait(c, pin);
      if (e == hipSuccess) host::pack_clip(c->side_pin[pin], L, frames, &stride, (int)f0, n);
      for (int f = 0; f < n && e == hipSuccess; ++f)   // a ring may wrap inside a chunk: every frame to its own slot
        e = hipMemcpyAsync((uint8_t*)clip.base + (size_t)((f0 + f) % clip.ring) * frame_bytes, c->side_pin[pin] + (size_t)f * frame_bytes, frame_bytes,
                           hipMemcpyHostToDevice, c->stream);
      if (e == hipSuccess) e = pin_mark(c, pin);
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
  return shift_sse(c, DevClip{ref_luma, ref_row_pitch, ref_frame_pitch}, DevClip{dis_luma, dis_row_pitch, dis_frame_pitch}, n_frames, radius, out);
}
int pqa_shift_sse(pqa_ctx* c, const void* const* ref_frames, int64_t ref_row_stride, const void* const* dis_frames,
                  int64_t dis_row_stride, int32_t n_frames, int32_t radius, uint64_t* out) {
  return shift_sse(c, HostClip{ref_frames, &ref_row_stride}, HostClip{dis_frames, &dis_row_stride}, n_frames, radius, out);
}

// ---- level alignment (level_stats.hip) ---------------------------------------------------------------------------------

int pqa_level_bins(const pqa_ctx* c) { return c ? 1 << c->cfg.bit_depth : PQA_EINVAL; }

int pqa_level_stats_device(pqa_ctx* c, const void* ref, int64_t ref_row_pitch, int64_t ref_frame_pitch, const void* dis,
                           int64_t dis_row_pitch, int64_t dis_frame_pitch, int32_t n_frames, int32_t plane, uint64_t* out) {
  return level_stats(c, DevClip{ref, ref_row_pitch, ref_frame_pitch}, DevClip{dis, dis_row_pitch, dis_frame_pitch}, n_frames, plane, out);
}
int pqa_level_stats(pqa_ctx* c, const void* const* ref_frames, int64_t ref_row_stride, const void* const* dis_frames,
                    int64_t dis_row_stride, int32_t n_frames, int32_t plane, uint64_t* out) {
  return level_stats(c, HostClip{ref_frames, &ref_row_stride}, HostClip{dis_frames, &dis_row_stride}, n_frames, plane, out);
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
  return resample_run(c, spec, slot, one_plane(src, src_row_pitch, src_frame_pitch), one_plane(dst, dst_row_pitch, dst_frame_pitch), n_frames);
}

int pqa_resample(pqa_ctx* c, const pqa_resample_spec* spec, const void* const* src_frames, int64_t src_row_stride,
                 void* const* dst_frames, int64_t dst_row_stride, int32_t n_frames) {
  int rc = rs_check(c, spec);
  if (rc != PQA_OK) return rc;
  if (n_frames < 0) return fail(c, PQA_EINVAL, "resample: negative frame count");
  if (n_frames > 0 && (!src_frames || !dst_frames)) return fail(c, PQA_EINVAL, "resample: null frame list");
  const size_t src_row = (size_t)spec->src_width * c->esize, dst_row = (size_t)spec->dst_width * c->esize;
  rc = check_host_frames(c, "resample: ", "source ", src_frames, 1, n_frames, src_row_stride, src_row, true);
  if (rc == PQA_OK) rc = check_host_frames(c, "resample: ", "destination ", (const void* const*)dst_frames, 1, n_frames, dst_row_stride, dst_row, true);
  if (rc != PQA_OK) return rc;
  int slot = 0;
  rc = rs_tables(c, spec, &slot);   // more than 32 taps: refused before any device call
  if (rc != PQA_OK) return rc;
  if (c->cancelled.load()) return fail(c, PQA_ECANCELLED, "cancelled");
  if (n_frames == 0) return PQA_OK;
  return resample_run(c, spec, slot, HostClip{src_frames, &src_row_stride}, HostClip{(const void* const*)dst_frames, &dst_row_stride}, n_frames);
}

// ---- packed capture formats (unpack.hip) -----------------------------------------------------------------------------------

int pqa_unpack_device(pqa_ctx* c, const pqa_unpack_spec* spec, const void* src, int64_t src_row_pitch, int64_t src_frame_pitch,
                      int32_t n_frames, const pqa_device_clip* dst) {
  int rc = unpack_check(c, spec, src, dst, n_frames, src_row_pitch, src_frame_pitch);
  if (rc != PQA_OK) return rc;
  if (c->cancelled.load()) return fail(c, PQA_ECANCELLED, "cancelled");
  if (n_frames == 0) return PQA_OK;
  int np = 0;
  rc = packed_dst_check(c, "unpack", spec->format == PQA_SURFACE_V210 ? "v210" : nullptr, src, dst, host::packed_sample_bytes(spec->format),
                        (int)spec->width, ((int)spec->width + 1) / 2, &np);
  if (rc != PQA_OK) return rc;
  return unpack_run(c, spec, np, one_plane(src, src_row_pitch, src_frame_pitch), *dst, n_frames);
}

int pqa_unpack(pqa_ctx* c, const pqa_unpack_spec* spec, const void* const* src_frames, int64_t src_row_stride, int32_t n_frames,
               void* const* dst_planes, const int64_t dst_strides[3]) {
  int rc = unpack_check(c, spec, src_frames, dst_planes, n_frames, src_row_stride, 0);
  if (rc != PQA_OK) return rc;
  if (c->cancelled.load()) return fail(c, PQA_ECANCELLED, "cancelled");
  if (n_frames == 0) return PQA_OK;
  int np = 0;
  rc = packed_dst_check(c, "unpack", spec->format == PQA_SURFACE_V210 ? "v210" : nullptr, src_frames, dst_planes, dst_strides, n_frames,
                        host::packed_sample_bytes(spec->format), (int)spec->width, ((int)spec->width + 1) / 2, false, &np);
  if (rc != PQA_OK) return rc;
  return unpack_run(c, spec, np, HostClip{src_frames, &src_row_stride}, HostClip{(const void* const*)dst_planes, dst_strides}, n_frames);
}

// ---- pixel-format conversion (format_convert.hip) ---------------------------------------------------------------------------

int pqa_format_convert_device(pqa_ctx* c, const pqa_convert_spec* spec, const void* src, int64_t src_row_pitch, int64_t src_frame_pitch,
                              void* dst, int64_t dst_row_pitch, int64_t dst_frame_pitch, int32_t n_frames) {
  int rc = convert_check(c, spec, src, dst, n_frames);
  if (rc != PQA_OK) return rc;
  const ConvertPlanes P = convert_planes(spec);
  rc = check_device_planes(c, "format_convert", {{"source", src, src_row_pitch, src_frame_pitch, (int64_t)P.src_row, P.S.bits > 8 ? 2 : 1},
                                                 {"destination", dst, dst_row_pitch, dst_frame_pitch, (int64_t)P.dst_row, P.D.bits > 8 ? 2 : 1}});
  if (rc != PQA_OK) return rc;
  if (c->cancelled.load()) return fail(c, PQA_ECANCELLED, "cancelled");
  if (n_frames == 0) return PQA_OK;
  return convert_run(c, spec, P, one_plane(src, src_row_pitch, src_frame_pitch), one_plane(dst, dst_row_pitch, dst_frame_pitch), n_frames);
}

int pqa_format_convert(pqa_ctx* c, const pqa_convert_spec* spec, const void* const* src_frames, int64_t src_row_stride,
                       void* const* dst_frames, int64_t dst_row_stride, int32_t n_frames) {
  int rc = convert_check(c, spec, src_frames, dst_frames, n_frames);
  if (rc != PQA_OK) return rc;
  const ConvertPlanes P = convert_planes(spec);
  rc = check_host_frames(c, "format_convert: ", "source ", src_frames, 1, n_frames, src_row_stride, P.src_row, true);
  if (rc == PQA_OK) rc = check_host_frames(c, "format_convert: ", "destination ", (const void* const*)dst_frames, 1, n_frames, dst_row_stride, P.dst_row, true);
  if (rc != PQA_OK) return rc;
  if (c->cancelled.load()) return fail(c, PQA_ECANCELLED, "cancelled");
  if (n_frames == 0) return PQA_OK;
  return convert_run(c, spec, P, HostClip{src_frames, &src_row_stride}, HostClip{(const void* const*)dst_frames, &dst_row_stride}, n_frames);
}

// ---- packed RGB captures -> Y'CbCr planes (rgb_convert.hip) -------------------------------------------------------------------

int pqa_rgb_convert_device(pqa_ctx* c, const pqa_rgb_spec* spec, const void* src, int64_t src_row_pitch, int64_t src_frame_pitch,
                           int32_t n_frames, const pqa_device_clip* dst) {
  int rc = rgb_check(c, spec, src, dst, n_frames, src_row_pitch, src_frame_pitch);
  if (rc != PQA_OK) return rc;
  if (c->cancelled.load()) return fail(c, PQA_ECANCELLED, "cancelled");
  if (n_frames == 0) return PQA_OK;
  int np = 0;
  rc = packed_dst_check(c, "rgb_convert", spec->format == PQA_SURFACE_R210 ? "r210" : nullptr, src, dst, spec->dst_bits > 8 ? 2 : 1, (int)spec->width,
                        convert_plane_size((int)spec->width, (int)spec->hshift), &np);
  if (rc != PQA_OK) return rc;
  return rgb_run(c, spec, np, one_plane(src, src_row_pitch, src_frame_pitch), *dst, n_frames);
}

int pqa_rgb_convert(pqa_ctx* c, const pqa_rgb_spec* spec, const void* const* src_frames, int64_t src_row_stride, int32_t n_frames,
                    void* const* dst_planes, const int64_t dst_strides[3]) {
  int rc = rgb_check(c, spec, src_frames, dst_planes, n_frames, src_row_stride, 0);
  if (rc != PQA_OK) return rc;
  if (c->cancelled.load()) return fail(c, PQA_ECANCELLED, "cancelled");
  if (n_frames == 0) return PQA_OK;
  int np = 0;
  rc = packed_dst_check(c, "rgb_convert", spec->format == PQA_SURFACE_R210 ? "r210" : nullptr, src_frames, dst_planes, dst_strides, n_frames,
                        spec->dst_bits > 8 ? 2 : 1, (int)spec->width, convert_plane_size((int)spec->width, (int)spec->hshift), true, &np);
  if (rc != PQA_OK) return rc;
  return rgb_run(c, spec, np, HostClip{src_frames, &src_row_stride}, HostClip{(const void* const*)dst_planes, dst_strides}, n_frames);
}

// ---- transfer-curve alignment: planes through an integer table (table_apply.hip) ----------------------------------------------

int pqa_table_apply_device(pqa_ctx* c, const pqa_table_spec* spec, const void* table, const void* src, int64_t src_row_pitch,
                           int64_t src_frame_pitch, void* dst, int64_t dst_row_pitch, int64_t dst_frame_pitch, int32_t n_frames) {
  int rc = table_check(c, spec, table, src, dst, n_frames);
  if (rc != PQA_OK) return rc;
  const int es = c->esize;
  const int64_t row = (int64_t)spec->width * es;
  rc = check_device_planes(c, "table_apply", {{"source", src, src_row_pitch, src_frame_pitch, row, es}, {"destination", dst, dst_row_pitch, dst_frame_pitch, row, es}});
  if (rc != PQA_OK) return rc;
  if (c->cancelled.load()) return fail(c, PQA_ECANCELLED, "cancelled");
  if (n_frames == 0) return PQA_OK;
  return table_run(c, spec, table, one_plane(src, src_row_pitch, src_frame_pitch), one_plane(dst, dst_row_pitch, dst_frame_pitch), n_frames);
}

int pqa_table_apply(pqa_ctx* c, const pqa_table_spec* spec, const void* table, const void* const* src_frames, int64_t src_row_stride,
                    void* const* dst_frames, int64_t dst_row_stride, int32_t n_frames) {
  int rc = table_check(c, spec, table, src_frames, dst_frames, n_frames);
  if (rc != PQA_OK) return rc;
  const size_t row = (size_t)spec->width * c->esize;
  rc = check_host_frames(c, "table_apply: ", "source ", src_frames, 1, n_frames, src_row_stride, row, true);
  if (rc == PQA_OK) rc = check_host_frames(c, "table_apply: ", "destination ", (const void* const*)dst_frames, 1, n_frames, dst_row_stride, row, true);
  if (rc != PQA_OK) return rc;
  if (c->cancelled.load()) return fail(c, PQA_ECANCELLED, "cancelled");
  if (n_frames == 0) return PQA_OK;
  return table_run(c, spec, table, HostClip{src_frames, &src_row_stride}, HostClip{(const void* const*)dst_frames, &dst_row_stride}, n_frames);
}

// ---- deinterlacing: a kept field and an interpolated one (deinterlace.hip) ------------------------------------------------------

int pqa_deint_chunk(void) { return kDeintChunk; }
int pqa_deint_block_bytes(void) { return kDeintColBytes; }
int pqa_deint_block_rows(void) { return kDeintWaves * kDeintBand; }

int pqa_deinterlace_device(pqa_ctx* c, const pqa_deint_spec* spec, const void* src, int64_t src_row_pitch, int64_t src_frame_pitch,
                           void* dst, int64_t dst_row_pitch, int64_t dst_frame_pitch, int32_t n_frames) {
  int rc = deint_check(c, spec, src, dst, n_frames);
  if (rc != PQA_OK) return rc;
  const int es = c->esize;
  const int64_t row = (int64_t)spec->width * es;
  rc = check_device_planes(c, "deinterlace", {{"source", src, src_row_pitch, src_frame_pitch, row, es}, {"destination", dst, dst_row_pitch, dst_frame_pitch, row, es}});
  if (rc != PQA_OK) return rc;
  if (n_frames > 0 && dst == src) return fail(c, PQA_EINVAL, "deinterlace: the destination is the source");
  if (c->cancelled.load()) return fail(c, PQA_ECANCELLED, "cancelled");
  if (n_frames == 0) return PQA_OK;
  return deint_run(c, spec, one_plane(src, src_row_pitch, src_frame_pitch), one_plane(dst, dst_row_pitch, dst_frame_pitch), n_frames);
}

int pqa_deinterlace(pqa_ctx* c, const pqa_deint_spec* spec, const void* const* src_frames, int64_t src_row_stride, void* const* dst_frames,
                    int64_t dst_row_stride, int32_t n_frames) {
  int rc = deint_check(c, spec, src_frames, dst_frames, n_frames);
  if (rc != PQA_OK) return rc;
  const size_t row = (size_t)spec->width * c->esize;
  const int n_out = n_frames * (1 + (int)spec->rate);
  rc = check_host_frames(c, "deinterlace: ", "source ", src_frames, 1, n_frames, src_row_stride, row, true);
  if (rc == PQA_OK) rc = check_host_frames(c, "deinterlace: ", "destination ", (const void* const*)dst_frames, 1, n_out, dst_row_stride, row, true);
  if (rc != PQA_OK) return rc;
  if (n_frames > 0 && (src_row_stride % c->esize || dst_row_stride % c->esize))
    return fail(c, PQA_EINVAL, "deinterlace: stride is not a multiple of the sample size");
  std::vector<const void*> sources(src_frames, src_frames + n_frames);
  std::sort(sources.begin(), sources.end(), std::less<const void*>());   // no in-place form: the window reads rows after they would be written
  for (int k = 0; k < n_out; ++k)
    if (std::binary_search(sources.begin(), sources.end(), (const void*)dst_frames[k], std::less<const void*>()))
      return fail(c, PQA_EINVAL, "deinterlace: destination frame %d is a source frame", k);
  if (c->cancelled.load()) return fail(c, PQA_ECANCELLED, "cancelled");
  if (n_frames == 0) return PQA_OK;
  return deint_run(c, spec, HostClip{src_frames, &src_row_stride}, HostClip{(const void* const*)dst_frames, &dst_row_stride}, n_frames);
}

// ---- overlay masking: planes through a feathered mask (mask_blend.hip) ---------------------------------------------------------

int pqa_mask_blend_device(pqa_ctx* c, const pqa_mask_spec* spec, const uint16_t* nodes, const void* src, int64_t src_row_pitch,
                          int64_t src_frame_pitch, const void* fill, int64_t fill_row_pitch, int64_t fill_frame_pitch, void* dst,
                          int64_t dst_row_pitch, int64_t dst_frame_pitch, int32_t n_frames) {
  MaskBounds bounds;
  int rc = mask_check(c, spec, nodes, src, dst, n_frames, &bounds);
  if (rc != PQA_OK) return rc;
  const int es = c->esize;
  const int64_t row = (int64_t)spec->width * es;
  rc = check_device_planes(c, "mask_blend", {{"source", src, src_row_pitch, src_frame_pitch, row, es}, {"destination", dst, dst_row_pitch, dst_frame_pitch, row, es}});
  if (rc == PQA_OK && fill) rc = check_device_planes(c, "mask_blend", {{"fill", fill, fill_row_pitch, fill_frame_pitch, row, es}});
  if (rc != PQA_OK) return rc;
  if (fill && fill == dst) return fail(c, PQA_EINVAL, "mask_blend: the destination is the fill plane");
  if (c->cancelled.load()) return fail(c, PQA_ECANCELLED, "cancelled");
  if (n_frames == 0) return PQA_OK;
  const pqa_device_clip fill_clip = one_plane(fill, fill_row_pitch, fill_frame_pitch);
  return mask_run(c, spec, nodes, bounds, one_plane(src, src_row_pitch, src_frame_pitch), fill ? &fill_clip : nullptr,
                  one_plane(dst, dst_row_pitch, dst_frame_pitch), n_frames);
}

int pqa_mask_blend(pqa_ctx* c, const pqa_mask_spec* spec, const uint16_t* nodes, const void* const* src_frames, int64_t src_row_stride,
                   const void* const* fill_frames, int64_t fill_row_stride, void* const* dst_frames, int64_t dst_row_stride,
                   int32_t n_frames) {
  MaskBounds bounds;
  int rc = mask_check(c, spec, nodes, src_frames, dst_frames, n_frames, &bounds);
  if (rc != PQA_OK) return rc;
  const size_t row = (size_t)spec->width * c->esize;
  rc = check_host_frames(c, "mask_blend: ", "source ", src_frames, 1, n_frames, src_row_stride, row, true);
  if (rc == PQA_OK) rc = check_host_frames(c, "mask_blend: ", "destination ", (const void* const*)dst_frames, 1, n_frames, dst_row_stride, row, true);
  if (rc == PQA_OK && fill_frames) rc = check_host_frames(c, "mask_blend: ", "fill ", fill_frames, 1, n_frames, fill_row_stride, row, true);
  if (rc != PQA_OK) return rc;
  for (int f = 0; fill_frames && f < n_frames; ++f)
    if (fill_frames[f] == dst_frames[f]) return fail(c, PQA_EINVAL, "mask_blend: destination frame %d is its fill plane", f);
  if (c->cancelled.load()) return fail(c, PQA_ECANCELLED, "cancelled");
  if (n_frames == 0) return PQA_OK;
  const HostClip fill_clip{fill_frames, &fill_row_stride};
  return mask_run(c, spec, nodes, bounds, HostClip{src_frames, &src_row_stride}, fill_frames ? &fill_clip : nullptr,
                  HostClip{(const void* const*)dst_frames, &dst_row_stride}, n_frames);
}

// ---- the spec-driven analyses: flow_moments() ... line_profiles() above ------------------------------------------------------

int pqa_flow_moments_device(pqa_ctx* c, const pqa_flow_spec* spec, const void* ref, int64_t ref_row_pitch, int64_t ref_frame_pitch,
                            const void* dis, int64_t dis_row_pitch, int64_t dis_frame_pitch, int32_t n_frames, int64_t* out) {
  return flow_moments(c, spec, DevClip{ref, ref_row_pitch, ref_frame_pitch}, DevClip{dis, dis_row_pitch, dis_frame_pitch}, n_frames, out);
}
int pqa_flow_moments(pqa_ctx* c, const pqa_flow_spec* spec, const void* const* ref_frames, int64_t ref_row_stride,
                     const void* const* dis_frames, int64_t dis_row_stride, int32_t n_frames, int64_t* out) {
  return flow_moments(c, spec, HostClip{ref_frames, &ref_row_stride}, HostClip{dis_frames, &dis_row_stride}, n_frames, out);
}

int pqa_tile_moments_device(pqa_ctx* c, const pqa_tile_spec* spec, const void* ref, int64_t ref_row_pitch, int64_t ref_frame_pitch,
                            const void* dis, int64_t dis_row_pitch, int64_t dis_frame_pitch, int32_t n_frames, uint64_t* out) {
  return tile_moments(c, spec, DevClip{ref, ref_row_pitch, ref_frame_pitch}, DevClip{dis, dis_row_pitch, dis_frame_pitch}, n_frames, out);
}
int pqa_tile_moments(pqa_ctx* c, const pqa_tile_spec* spec, const void* const* ref_frames, int64_t ref_row_stride,
                     const void* const* dis_frames, int64_t dis_row_stride, int32_t n_frames, uint64_t* out) {
  return tile_moments(c, spec, HostClip{ref_frames, &ref_row_stride}, HostClip{dis_frames, &dis_row_stride}, n_frames, out);
}

int pqa_band_sums(void) { return kBandSums; }
int pqa_band_moments_device(pqa_ctx* c, const pqa_band_spec* spec, const void* ref, int64_t ref_row_pitch, int64_t ref_frame_pitch,
                            const void* dis, int64_t dis_row_pitch, int64_t dis_frame_pitch, int32_t n_frames, uint64_t* out) {
  return band_moments(c, spec, DevClip{ref, ref_row_pitch, ref_frame_pitch}, DevClip{dis, dis_row_pitch, dis_frame_pitch}, n_frames, out);
}
int pqa_band_moments(pqa_ctx* c, const pqa_band_spec* spec, const void* const* ref_frames, int64_t ref_row_stride,
                     const void* const* dis_frames, int64_t dis_row_stride, int32_t n_frames, uint64_t* out) {
  return band_moments(c, spec, HostClip{ref_frames, &ref_row_stride}, HostClip{dis_frames, &dis_row_stride}, n_frames, out);
}

int pqa_temporal_sums(void) { return kTemporalSums; }
int pqa_temporal_moments_device(pqa_ctx* c, const pqa_temporal_spec* spec, const void* ref, int64_t ref_row_pitch,
                                int64_t ref_frame_pitch, const void* dis, int64_t dis_row_pitch, int64_t dis_frame_pitch,
                                int32_t n_frames, uint64_t* out) {
  return temporal_moments(c, spec, DevClip{ref, ref_row_pitch, ref_frame_pitch}, DevClip{dis, dis_row_pitch, dis_frame_pitch}, n_frames, out);
}
int pqa_temporal_moments(pqa_ctx* c, const pqa_temporal_spec* spec, const void* const* ref_frames, int64_t ref_row_stride,
                         const void* const* dis_frames, int64_t dis_row_stride, int32_t n_frames, uint64_t* out) {
  return temporal_moments(c, spec, HostClip{ref_frames, &ref_row_stride}, HostClip{dis_frames, &dis_row_stride}, n_frames, out);
}

int pqa_field_moments_device(pqa_ctx* c, const pqa_field_spec* spec, const void* ref, int64_t ref_row_pitch, int64_t ref_frame_pitch,
                             const void* dis, int64_t dis_row_pitch, int64_t dis_frame_pitch, int32_t n_frames, uint64_t* out) {
  return field_moments(c, spec, DevClip{ref, ref_row_pitch, ref_frame_pitch}, DevClip{dis, dis_row_pitch, dis_frame_pitch}, n_frames, out);
}
int pqa_field_moments(pqa_ctx* c, const pqa_field_spec* spec, const void* const* ref_frames, int64_t ref_row_stride,
                      const void* const* dis_frames, int64_t dis_row_stride, int32_t n_frames, uint64_t* out) {
  return field_moments(c, spec, HostClip{ref_frames, &ref_row_stride}, HostClip{dis_frames, &dis_row_stride}, n_frames, out);
}

int pqa_edge_sums(void) { return kEdgeSums; }
int pqa_edge_profiles_device(pqa_ctx* c, const pqa_edge_spec* spec, const void* ref, int64_t ref_row_pitch, int64_t ref_frame_pitch,
                             const void* dis, int64_t dis_row_pitch, int64_t dis_frame_pitch, int32_t n_frames, uint64_t* out) {
  return edge_profiles(c, spec, DevClip{ref, ref_row_pitch, ref_frame_pitch}, DevClip{dis, dis_row_pitch, dis_frame_pitch}, n_frames, out);
}
int pqa_edge_profiles(pqa_ctx* c, const pqa_edge_spec* spec, const void* const* ref_frames, int64_t ref_row_stride,
                      const void* const* dis_frames, int64_t dis_row_stride, int32_t n_frames, uint64_t* out) {
  return edge_profiles(c, spec, HostClip{ref_frames, &ref_row_stride}, HostClip{dis_frames, &dis_row_stride}, n_frames, out);
}

int pqa_line_profiles_device(pqa_ctx* c, const pqa_profile_spec* spec, const void* planes, int64_t row_pitch, int64_t frame_pitch,
                             int32_t n_frames, uint64_t* out) {
  return line_profiles(c, spec, DevClip{planes, row_pitch, frame_pitch}, n_frames, out);
}
int pqa_line_profiles(pqa_ctx* c, const pqa_profile_spec* spec, const void* const* frames, int64_t row_stride, int32_t n_frames,
                      uint64_t* out) {
  return line_profiles(c, spec, HostClip{frames, &row_stride}, n_frames, out);
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
  return pair_run(c, colour_job(c, n_frames, out), *ref, *dis, nullptr, colour_launch(c, lo, hi));
}

int pqa_colour_moments(pqa_ctx* c, const void* const* ref_frames, const int64_t ref_strides[3], const void* const* dis_frames,
                       const int64_t dis_strides[3], int32_t n_frames, uint32_t lo, uint32_t hi, uint64_t* out) {
  if (!c) return PQA_EINVAL;
  const int rc = cl_check(c, "colour_moments", n_frames);
  if (rc != PQA_OK) return rc;
  const uint32_t top = (1u << c->cfg.bit_depth) - 1u;
  if (lo > hi || hi > top) return fail(c, PQA_EINVAL, "colour_moments: mask %u ... %u outside 0 ... %u", lo, hi, top);
  if (n_frames > 0 && (!ref_frames || !dis_frames || !ref_strides || !dis_strides)) return fail(c, PQA_EINVAL, "colour_moments: null frame list");
  if (n_frames > 0 && !out) return fail(c, PQA_EINVAL, "colour_moments: null output pointer");
  if (n_frames == 0) return PQA_OK;
  const HostClip ref{ref_frames, ref_strides}, dis{dis_frames, dis_strides};
  return pair_run(c, colour_job(c, n_frames, out), ref, &dis, colour_launch(c, lo, hi));   // the frame rules, `cancelled` and the staging
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
  return colour_apply_run(c, m, *src, *dst, n_frames);
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
  return colour_apply_run(c, m, HostClip{src_frames, src_strides}, HostClip{(const void* const*)dst_frames, dst_strides}, n_frames);
}

// ---- Delta E ITP (delta_itp.hip) -----------------------------------------------------------------------------------------

int pqa_itp_sums(void) { return kItpSums; }

int pqa_delta_itp_device(pqa_ctx* c, const pqa_itp_spec* spec, const pqa_device_clip* ref, const pqa_device_clip* dis,
                         int32_t n_frames, double* out) {
  if (!c) return PQA_EINVAL;
  int rc = itp_check(c, spec, n_frames);
  if (rc != PQA_OK) return rc;
  if (n_frames > 0 && (!ref || !dis)) return fail(c, PQA_EINVAL, "delta_itp: null clip pointer");
  if (n_frames > 0 && !out) return fail(c, PQA_EINVAL, "delta_itp: null output pointer");
  if (n_frames == 0) return PQA_OK;
  rc = cl_check_clip(c, "delta_itp: reference ", ref);
  if (rc == PQA_OK) rc = cl_check_clip(c, "delta_itp: captured ", dis);
  if (rc != PQA_OK) return rc;
  if (c->cancelled.load()) return fail(c, PQA_ECANCELLED, "cancelled");
  return pair_run(c, itp_job(c, n_frames, out), *ref, *dis, &c->cancelled, itp_launch(c, spec));
}

int pqa_delta_itp(pqa_ctx* c, const pqa_itp_spec* spec, const void* const* ref_frames, const int64_t ref_strides[3],
                  const void* const* dis_frames, const int64_t dis_strides[3], int32_t n_frames, double* out) {
  if (!c) return PQA_EINVAL;
  const int rc = itp_check(c, spec, n_frames);
  if (rc != PQA_OK) return rc;
  if (n_frames > 0 && (!ref_frames || !dis_frames || !ref_strides || !dis_strides)) return fail(c, PQA_EINVAL, "delta_itp: null frame list");
  if (n_frames > 0 && !out) return fail(c, PQA_EINVAL, "delta_itp: null output pointer");
  if (n_frames == 0) return PQA_OK;
  const HostClip ref{ref_frames, ref_strides}, dis{dis_frames, dis_strides};
  return pair_run(c, itp_job(c, n_frames, out), ref, &dis, itp_launch(c, spec));   // the frame rules, `cancelled` and the staging
}

}  // extern "C"
