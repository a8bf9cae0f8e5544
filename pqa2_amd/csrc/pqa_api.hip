// C ABI of libpqa_vmaf.so: context lifetime, workspaces, batching, the submit paths and their host staging, collect,
// profiling hooks.  The one-shot analyses beside the scoring chain: pqa_side.hip; the pqa_debug_* entries: pqa_debug.hip.
// Declarations and the reference interfaces each entry point replaces: include/pqa_vmaf.h.
#include "pqa_ctx.h"

#include <algorithm>
#include <array>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <mutex>

#include "ingest.h"

using namespace pqa;
using pqa::host::PackPool;
using pqa::host::PackTask;
using pqa::host::PlaneSrc;
using pqa::host::run_pack_task;

static thread_local std::string g_create_error;   // pqa_last_error(NULL): what pqa_create and the pqa_debug_* entries report

int pqa::fail(pqa_ctx* c, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (c) c->err = buf; else g_create_error = buf;
  return code;
}

namespace {

// Staging buffers of the host path outlive their context: pinning 2 x 200 MB (2160p 4:2:0, 8 frames) and releasing it again
// costs ~55 ms per context -- more than scoring a 48-frame 2160p clip -- and the reference's caller makes a fresh analyzer
// per run (app/ui/tabs/analysis_tab.py:588).  One set per process is kept for the next context of the same device and
// size (PQA_STAGING_CACHE=0: off; anything else it holds is released when a differently sized set is parked).
struct StagingSet {
  int device = -1;
  size_t bytes = 0;
  uint8_t* pinned[2] = {nullptr, nullptr};
  uint8_t* dev[2] = {nullptr, nullptr};
};
std::mutex g_staging_mu;
StagingSet g_staging;   // guarded by g_staging_mu; empty when bytes == 0

bool staging_cache_enabled() {
  const char* e = getenv("PQA_STAGING_CACHE");
  return !(e && e[0] == '0');
}

void staging_release(StagingSet& s) {   // caller holds the lock or owns s; the right device must be current
  for (int i = 0; i < 2; ++i) {
    if (s.pinned[i]) hipHostFree(s.pinned[i]);
    if (s.dev[i]) hipFree(s.dev[i]);
    s.pinned[i] = s.dev[i] = nullptr;
  }
  s.bytes = 0;
  s.device = -1;
}

static const char* kProfNames[PQA_PROF_KERNELS] = {
    "vif_stat_s0", "vif_stat_s1", "vif_stat_s2", "vif_stat_s3", "ciede2000", "reserved5",
    "reserved6", "adm_scale_s0", "adm_scale_s1", "adm_scale_s2", "adm_scale_s3", "motion", "sse",
    "ssim", "finalize", "ms_ssim", "float_ssim"};

struct ProfScope {
  pqa_ctx* c;
  ProfEv ev{};
  bool on;
  hipStream_t st;
  ProfScope(pqa_ctx* ctx, int id, int frames, hipStream_t stream)
      : c(ctx), on(ctx->prof && ((ctx->prof_mask >> id) & 1u)), st(stream), ev_id(id), ev_frames(frames) {
    if (c->trace) {
      fprintf(stderr, "[pqa trace] %s queued\n", kProfNames[id]);
      fflush(stderr);
    }
    if (!on) return;
    ev.id = id; ev.frames = frames;
    if (hipEventCreate(&ev.a) != hipSuccess || hipEventCreate(&ev.b) != hipSuccess) { on = false; return; }
    hipEventRecord(ev.a, st);
  }
  ~ProfScope() {
    if (c->trace) {   // the launches of this scope are queued: wait for them and say so, flushed
      const hipError_t e = hipStreamSynchronize(st);
      fprintf(stderr, "[pqa trace] %s done (%d frames)%s%s\n", kProfNames[ev_id], ev_frames, e == hipSuccess ? "" : ": ",
              e == hipSuccess ? "" : hipGetErrorString(e));
      fflush(stderr);
    }
    if (!on) return;
    hipEventRecord(ev.b, st);
    c->evs.push_back(ev);
  }
  int ev_id = 0, ev_frames = 0;
};

void prof_drain(pqa_ctx* c) {
  for (auto& e : c->evs) {
    float ms = 0.0f;
    if (hipEventSynchronize(e.b) == hipSuccess && hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess) {
      c->prof_ms[e.id] += ms;
      c->prof_n[e.id] += 1;
      c->prof_frames[e.id] += e.frames;
    }
    hipEventDestroy(e.a);
    hipEventDestroy(e.b);
  }
  c->evs.clear();
}

// ---- record-ring bookkeeping -----------------------------------------------------------------------
// A slot may be rewritten by the SAME frame index (a re-run) or once its record has been collected; a different
// frame landing on an uncollected record would lose it silently, so that is a call-sequence error.
int check_slots_free(pqa_ctx* c, int64_t first, int n) {
  int64_t f = 0, holder = 0;
  if (!c->ring.can_submit(first, n, &f, &holder))
    return fail(c, PQA_ESTATE,
                "frame %lld would overwrite the uncollected record of frame %lld (result_capacity %d): "
                "collect it first or create the context with a larger result_capacity",
                (long long)f, (long long)holder, c->capacity);
  return PQA_OK;
}

void claim_slots(pqa_ctx* c, int64_t first, int n, uint64_t seq) { c->ring.claim(first, n, seq); }

// Wait until batch `seq` (and, the stream being in order, every earlier one) has written its records.
int wait_batch(pqa_ctx* c, uint64_t seq) {
  if (seq <= c->done_seq) return PQA_OK;
  const int e = (int)(seq % kBatchEvents);
  // the event may meanwhile carry a later batch of the same stream: waiting for that one is still correct
  HIPCHK(c, hipEventSynchronize(c->batch_ev[e]));
  c->done_seq = c->batch_ev_seq[e] > seq ? c->batch_ev_seq[e] : seq;
  return PQA_OK;
}

// ---- the batch: every kernel for n consecutive device-resident frames -------------------------
struct RunPair { PlaneRun ref, dis; };
struct MutRunPair { MutPlaneRun ref{nullptr, 0, 0}, dis{nullptr, 0, 0}; };
struct Pred { const void* base = nullptr; int64_t pitch = 0; };   // a plane in front of the batch, pitch in elements; null: none

PlaneRun clip_run(const pqa_device_clip* clip, int p, int es) {
  return PlaneRun{clip->plane[p], clip->row_pitch[p] / es, clip->frame_pitch[p] / es};
}
PlaneRun run_at(PlaneRun r, int64_t elems, int es) {   // r from `elems` samples further on
  return PlaneRun{(const uint8_t*)r.base + elems * es, r.row_pitch, r.frame_pitch};
}
PlaneRun frames_from(PlaneRun r, int64_t f, int es) { return run_at(r, f * r.frame_pitch, es); }   // the run starting at frame f
RunPair level_in(const Level& L) { return RunPair{{L.ref, L.pitch, L.frame_pitch}, {L.dis, L.pitch, L.frame_pitch}}; }
MutRunPair level_out(const Level& L) { return MutRunPair{{L.ref, L.pitch, L.frame_pitch}, {L.dis, L.pitch, L.frame_pitch}}; }

// One batch as its steps see it: computed once by process_batch.  The counts below the streams are what the chains wrote, for
// the finalize kernel.
struct Batch {
  int64_t first;
  int n, e0, sp_n, k;        // sp_n frames, e0 + i * k, get spatial features (libvmaf n_subsample: index % k == 0)
  int es, w, h, capacity;
  PlaneRun r[3]{}, d[3]{};   // every frame of the reference / the distorted clip, per plane
  PlaneRun rs[3]{}, ds[3]{}; // the frames that get spatial features
  const pqa_device_clip *ref, *dis;
  Pred prev;                 // the caller's reference luma first-1
  hipStream_t st, st_adm, st_misc;
  bool multi, fork_late;
  int vif_np[4], adm_np[4], motion_np;   // partials written per frame
  int n_sse = 0, n_ssim = 0;
  bool sse_a[3] = {false, false, false}, sse_b[3] = {false, false, false}, sse_t[3] = {false, false, false};
  int slot(int64_t f) const { return (int)((first + f) % capacity); }   // the ring slot of frame f of the batch
};

// fork: the ADM chain and the motion/PSNR/SSIM kernels are independent of the VIF chain; on their own
// streams they fill the SIMD time the VALU-bound VIF kernels leave while waiting, and the small deep-scale
// grids overlap instead of running one after another
int fork_streams(pqa_ctx* c, const Batch& b) {
  HIPCHK(c, hipEventRecord(c->fork_ev, b.st));
  HIPCHK(c, hipStreamWaitEvent(b.st_adm, c->fork_ev, 0));
  HIPCHK(c, hipStreamWaitEvent(b.st_misc, c->fork_ev, 0));
  return PQA_OK;
}

int join_streams(pqa_ctx* c, const Batch& b) {
  HIPCHK(c, hipEventRecord(c->join_ev[0], b.st_adm));
  HIPCHK(c, hipEventRecord(c->join_ev[1], b.st_misc));
  HIPCHK(c, hipStreamWaitEvent(b.st, c->join_ev[0], 0));
  HIPCHK(c, hipStreamWaitEvent(b.st, c->join_ev[1], 0));
  return PQA_OK;
}

// One scale of a pyramid walk: reads `in` (w x h, elements `elem`), writes `out` (the next level; null at the last scale).
struct Scale { int s; Elem elem; RunPair in; int w, h; MutRunPair out; };

// One walk down a four-level pyramid: launch(k) queues scale k.s.  `first` is the scale the walk starts at, on the caller's
// planes (scale 0) or on those of lv[first.s]; the levels below hold elements `deep`.
template <typename Launch>
int walk_pyramid(const Level (&lv)[4], Scale first, Elem deep, Launch launch) {
  for (Scale k = first; k.s < 4; ++k.s) {
    k.out = k.s < 3 ? level_out(lv[k.s + 1]) : MutRunPair{};
    const int rc = launch(k);
    if (rc != PQA_OK) return rc;
    if (k.s < 3) {
      const Level& L = lv[k.s + 1];
      k.in = level_in(L);
      k.elem = deep;
      k.w = L.w; k.h = L.h;
    }
  }
  return PQA_OK;
}

// A history plane for plane p of a clip, rows padded to 64 bytes.
int hist_alloc(pqa_ctx* c, HistPlane* hp, int p) {
  hp->pitch = round_up((int64_t)c->pw[p] * c->esize, 64);
  return dev_alloc(c, &hp->base, (size_t)hp->pitch * c->ph[p]);
}

// VIF pyramid (floor halving): f32 planes of scales 1-3, rows padded to 64 B, and the partials of every scale.
int alloc_vif(pqa_ctx* c) {
  const bool on = c->cfg.features & PQA_FEAT_VIF;
  if (on && !c->vif_fixed) HIPCHK(c, vif_march_prepare());
  if (c->vif_fixed) {
    std::vector<uint16_t> lut(32768);
    vif_fixed_log2_table(lut.data());
    PQACHK(dev_alloc(c, &c->vif_lut, lut.size()));
    HIPCHK(c, hipMemcpy(c->vif_lut, lut.data(), lut.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
  }
  int vw = c->pw[0], vh = c->ph[0];
  for (int s = 0; s < 4; ++s) {
    if (s > 0) {
      vw /= 2; vh /= 2;
      Level& V = c->vif_lv[s];
      V.w = vw; V.h = vh; V.pitch = round_up(vw, 16); V.frame_pitch = V.pitch * vh;
      if (on) {
        PQACHK(dev_alloc(c, &V.ref, (size_t)V.frame_pitch * c->B));
        PQACHK(dev_alloc(c, &V.dis, (size_t)V.frame_pitch * c->B));
      }
    }
    if (vw < 2 || vh < 2) return fail(c, PQA_EINVAL, "frame too small for 4 VIF scales");
    c->vif_tiles[s] = vif_tiles_x(s, vw) * vif_tiles_y(vh);
    if (s == 0) {   // scale 0 may run the march kernel, which writes one partial pair per wave segment
      const int mp = vif_march_partials_max(vw, vh);
      c->vif_part_cap0 = c->vif_tiles[0] > mp ? c->vif_tiles[0] : mp;
    }
    if (on && !c->vif_fixed)
      PQACHK(dev_alloc(c, &c->vif_part[s], (size_t)(s == 0 ? c->vif_part_cap0 : c->vif_tiles[s]) * 2 * c->B));
    if (on && c->vif_fixed) PQACHK(dev_alloc(c, &c->vif_fx_part[s], (size_t)c->vif_tiles[s] * kVifFxPartials * c->B));
  }
  return PQA_OK;
}

int run_vif(pqa_ctx* c, Batch& b) {
  if (!(c->cfg.features & PQA_FEAT_VIF) || b.sp_n == 0) return PQA_OK;
  const Scale top{0, c->elem, RunPair{b.rs[0], b.ds[0]}, b.w, b.h, {}};
  if (c->vif_fixed)   // the pyramid buffers hold u16 planes in this mode (same element pitches, half the bytes)
    return walk_pyramid(c->vif_lv, top, ELEM_U16, [&](const Scale& k) -> int {
      ProfScope ps(c, k.s, b.sp_n, b.st);
      HIPCHK(c, launch_vif_fixed(b.st, k.s, (int)c->cfg.bit_depth, k.elem, k.in.ref, k.in.dis, b.sp_n, k.w, k.h,
                                 c->cfg.vif_enhn_gain_limit, c->vif_lut, c->vif_fx_part[k.s], k.out.ref, k.out.dis));
      return PQA_OK;
    });
  return walk_pyramid(c->vif_lv, top, ELEM_F32, [&](const Scale& k) -> int {
    {
      ProfScope ps(c, k.s, b.sp_n, b.st);
      HIPCHK(c, launch_vif_stat(b.st, k.s, k.elem, k.in.ref, k.in.dis, b.sp_n, k.w, k.h, c->inv_scale,
                                (float)c->cfg.vif_enhn_gain_limit, c->cfg.vif_border == PQA_VIF_BORDER_INTEGER, c->vif_part[k.s],
                                k.out.ref, k.out.dis, c->vif_s0_mode, &b.vif_np[k.s], c->vif_uniform,
                                (c->vif_strip_mask >> k.s & 1) ? c->vif_strip_seg : -1));
    }
    // mode 2: the other chains start behind VIF scale 0 (the dominant launch runs alone, its figures stay its own) and
    // overlap VIF scales 1-3 only
    return k.s == 0 && b.fork_late ? fork_streams(c, b) : PQA_OK;
  });
}

// ADM approximation bands (ceil halving): f32 planes of scales 1-3, rows padded to 64 B, and the partials of every scale.
int alloc_adm(pqa_ctx* c) {
  const bool on = c->cfg.features & PQA_FEAT_ADM;
  const int w = c->pw[0], h = c->ph[0], B = c->B;
  if (c->adm_fixed) {
    std::vector<int32_t> lut(65537);
    adm_fixed_div_table(lut.data());
    PQACHK(dev_alloc(c, &c->adm_div_lut, lut.size()));
    HIPCHK(c, hipMemcpy(c->adm_div_lut, lut.data(), lut.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    PQACHK(dev_alloc(c, &c->adm_fx_acc, (size_t)c->capacity * 24));
    HIPCHK(c, hipMemsetAsync(c->adm_fx_acc, 0, (size_t)c->capacity * 24 * sizeof(long long), c->stream));
  }
  int aw = w, ah = h;
  for (int s = 0; s < 4; ++s) {
    if (s > 0) {
      aw = (aw + 1) / 2; ah = (ah + 1) / 2;
      Level& A = c->adm_lv[s];
      A.w = aw; A.h = ah; A.pitch = round_up(aw, 16); A.frame_pitch = A.pitch * ah;
      if (on) {
        PQACHK(dev_alloc(c, &A.ref, (size_t)A.frame_pitch * B));
        PQACHK(dev_alloc(c, &A.dis, (size_t)A.frame_pitch * B));
      }
    }
    const int bw = (aw + 1) / 2, bh = (ah + 1) / 2;  // band size produced at ADM scale s
    c->adm_tiles[s] = adm_tiles_x(bw) * adm_tiles_y(bh);
    const int left = (int)(bw * 0.1 - 0.5), top = (int)(bh * 0.1 - 0.5);
    c->adm_area[s] = (float)((bh - 2 * top) * (bw - 2 * left));
    c->adm_fx[s] = adm_fixed_scale_params(s, bw, bh);
    if (on && !c->adm_fixed) {   // one sextet per tile (adm.hip) or per wave segment (adm_march.hip)
      int mp = adm_march_partials(bw, bh);
      if (s < 2 && adm_pyramid_takes(c->elem, w, h)) { const int pp = adm_pyramid_partials(w, h); mp = pp > mp ? pp : mp; }
      PQACHK(dev_alloc(c, &c->adm_part[s], (size_t)(c->adm_tiles[s] > mp ? c->adm_tiles[s] : mp) * 6 * B));
    }
    if (on && c->adm_fixed) PQACHK(dev_alloc(c, &c->adm_fx_part[s], (size_t)c->adm_tiles[s] * kAdmFxRows * 6 * B));
  }
  return PQA_OK;
}

int run_adm(pqa_ctx* c, Batch& b) {
  if (!(c->cfg.features & PQA_FEAT_ADM) || b.sp_n == 0) return PQA_OK;
  Scale top{0, c->elem, RunPair{b.rs[0], b.ds[0]}, b.w, b.h, {}};
  if (c->adm_fixed)   // the approximation-band buffers hold int32 planes in this mode (same 4-byte elements)
    return walk_pyramid(c->adm_lv, top, ELEM_F32, [&](const Scale& k) -> int {
      ProfScope ps(c, 7 + k.s, b.sp_n, b.st_adm);
      HIPCHK(c, launch_adm_fixed(b.st_adm, k.s, (int)c->cfg.bit_depth, k.elem, k.in.ref, k.in.dis, b.sp_n, k.w, k.h,
                                 c->cfg.adm_enhn_gain_limit, c->adm_div_lut, k.out.ref, k.out.dis, c->adm_fx_part[k.s]));
      return PQA_OK;
    });
  // A caller's plane of 2 GiB and more: launch_adm_march would refuse scale 0 alone; the whole chain goes tiled, so that the
  // records are those of PQA_ADM_MARCH=0 (a context's mode is one for all scales: kernels.h).
  const int64_t span = (b.rs[0].row_pitch > b.ds[0].row_pitch ? b.rs[0].row_pitch : b.ds[0].row_pitch) * b.h * b.es;
  const int adm_mode = span >= (1ll << 31) ? (int)ADM_TILED : c->adm_mode;
  if (adm_mode == ADM_AUTO) {   // scales 0 and 1 in one launch when the geometry allows (adm_pyramid.hip)
    const Level& L2 = c->adm_lv[2];
    hipError_t perr = hipSuccess;
    int np = 0;
    ProfScope ps(c, 7, b.sp_n, b.st_adm);
    if (launch_adm_pyramid(b.st_adm, top.elem, top.in.ref, top.in.dis, b.sp_n, top.w, top.h, c->inv_scale,
                           (float)c->cfg.adm_enhn_gain_limit, level_out(L2).ref, level_out(L2).dis, c->adm_part[0], c->adm_part[1],
                           &np, c->adm_cone, &perr)) {
      HIPCHK(c, perr);
      b.adm_np[0] = b.adm_np[1] = np;
      top = Scale{2, ELEM_F32, level_in(L2), L2.w, L2.h, {}};
    }
  }
  return walk_pyramid(c->adm_lv, top, ELEM_F32, [&](const Scale& k) -> int {
    ProfScope ps(c, 7 + k.s, b.sp_n, b.st_adm);
    HIPCHK(c, launch_adm_scale(b.st_adm, k.s, k.elem, k.in.ref, k.in.dis, b.sp_n, k.w, k.h, c->inv_scale,
                               (float)c->cfg.adm_enhn_gain_limit, k.out.ref, k.out.dis, c->adm_part[k.s], adm_mode, &b.adm_np[k.s],
                               c->adm_cone));
    return PQA_OK;
  });
}

// The frame histories: the feature that reads one, its chain and planes ([slot][np]), the clip (distorted or reference), np.
struct History { uint32_t feature; host::FrameChain* chain; const HistPlane* planes; bool dis; int np; };
std::array<History, 5> histories(pqa_ctx* c) {
  return {{{PQA_FEAT_MOTION, &c->mo_chain, &c->mo_hist, false, 1},
           {PQA_FEAT_XPSNR, &c->xp_chain, c->xp_hist, false, 1},
           {PQA_FEAT_SITI, &c->st_chain[0], &c->st_hist[0], true, 1},
           {PQA_FEAT_SITI, &c->st_chain[1], &c->st_hist[1], false, 1},
           {PQA_FEAT_INTEGRITY, &c->ig_chain, c->ig_hist, true, c->n_planes}}};
}

// Frame `frame` as a chain holds it (planes[slot]), or none.
Pred held(const host::FrameChain& chain, const HistPlane* planes, int64_t frame, int es) {
  const int j = chain.find(frame);
  return j < 0 ? Pred{} : Pred{planes[j].base, planes[j].pitch / es};
}

// Motion: one partial per tile (motion.hip) or per wave segment (motion_march.hip), and the plane its chain keeps.
int alloc_motion(pqa_ctx* c) {
  const int w = c->pw[0], h = c->ph[0];
  c->motion_tiles_n = motion_tiles(w, h);
  if (!(c->cfg.features & PQA_FEAT_MOTION)) return PQA_OK;
  const int mp = motion_march_partials(w, h);
  PQACHK(dev_alloc(c, &c->motion_part, (size_t)(c->motion_tiles_n > mp ? c->motion_tiles_n : mp) * c->B));
  if (c->motion_fixed) PQACHK(dev_alloc(c, &c->motion_fx_part, (size_t)c->motion_tiles_n * c->B));
  return hist_alloc(c, &c->mo_hist, 0);
}

int run_motion(pqa_ctx* c, Batch& b) {
  if (!(c->cfg.features & PQA_FEAT_MOTION)) return PQA_OK;
  // reference luma in front of the batch: the caller's halo, the armed halo, or the last frame of the previous batch
  const Pred p0 = b.prev.base ? b.prev : held(c->mo_chain, &c->mo_hist, b.first - 1, b.es);
  ProfScope ps(c, 11, b.n, b.st_misc);
  if (c->motion_fixed)
    HIPCHK(c, launch_motion_fixed(b.st_misc, (int)c->cfg.bit_depth, c->elem, b.r[0], p0.base, p0.pitch, b.n, b.w, b.h,
                                  c->motion_fx_part));
  else
    HIPCHK(c, launch_motion(b.st_misc, c->elem, b.r[0], p0.base, p0.pitch, b.n, b.w, b.h, c->inv_scale, c->motion_part,
                            c->motion_mode, &b.motion_np));
  return PQA_OK;
}

int alloc_psnr_ssim(pqa_ctx* c) {
  const uint32_t feat = c->cfg.features;
  for (int p = 0; p < c->n_planes; ++p) {
    if (feat & PQA_FEAT_PSNR) {
      PQACHK(dev_alloc(c, &c->sse_part[p], (size_t)kSseBlocksPerPlane * c->B));
      PQACHK(dev_alloc(c, &c->sse_part_b[p], (size_t)kSseBlocksPerPlane * c->B));
    }
    if (feat & PQA_FEAT_SSIM) {
      c->ssim_tiles_n[p] = ssim_tiles(c->pw[p], c->ph[p]);
      const int ww = (c->pw[p] >> 2) - 1, wh = (c->ph[p] >> 2) - 1;
      c->ssim_norm[p] = (ww > 0 && wh > 0) ? 1.0 / ((double)ww * wh) : 0.0;
      PQACHK(dev_alloc(c, &c->ssim_part[p], (size_t)(c->ssim_tiles_n[p] ? c->ssim_tiles_n[p] : 1) * c->B));
      PQACHK(dev_alloc(c, &c->sse_tile_part[p], (size_t)(c->ssim_tiles_n[p] ? c->ssim_tiles_n[p] : 1) * c->B));
    }
  }
  return PQA_OK;
}

int run_psnr_ssim(pqa_ctx* c, Batch& b) {
  const uint32_t feat = c->cfg.features;
  const int es = b.es;
  const bool both = (feat & PQA_FEAT_PSNR) && (feat & PQA_FEAT_SSIM);
  if (feat & PQA_FEAT_PSNR) {
    b.n_sse = c->n_planes;
    ProfScope ps(c, 12, b.n, b.st_misc);
    for (int p = 0; p < c->n_planes; ++p) {
      const PlaneRun a = b.d[p], r = b.r[p];
      const int pw = c->pw[p], ph = c->ph[p];
      if (both && c->ssim_tiles_n[p] > 0) {
        // the SSIM kernel delivers the squared error of the 4-aligned part; only remainder strips are left
        b.sse_t[p] = true;
        const int w4 = (pw >> 2) << 2, h4 = (ph >> 2) << 2;
        if (w4 < pw) {
          HIPCHK(c, launch_sse(b.st_misc, c->elem, run_at(a, w4, es), run_at(r, w4, es), b.n, pw - w4, ph, c->sse_part[p]));
          b.sse_a[p] = true;
        }
        if (h4 < ph) {
          HIPCHK(c, launch_sse(b.st_misc, c->elem, run_at(a, h4 * a.row_pitch, es), run_at(r, h4 * r.row_pitch, es), b.n, w4,
                               ph - h4, c->sse_part_b[p]));
          b.sse_b[p] = true;
        }
      } else {
        HIPCHK(c, launch_sse(b.st_misc, c->elem, a, r, b.n, pw, ph, c->sse_part[p]));
        b.sse_a[p] = true;
      }
    }
  }
  if (feat & PQA_FEAT_SSIM) {
    b.n_ssim = c->n_planes;
    ProfScope ps(c, 13, b.n, b.st_misc);
    for (int p = 0; p < c->n_planes; ++p)
      HIPCHK(c, launch_ssim(b.st_misc, c->elem, b.d[p], b.r[p], b.n, c->pw[p], c->ph[p], (1 << c->cfg.bit_depth) - 1,
                            c->ssim_part[p], b.sse_t[p] ? c->sse_tile_part[p] : nullptr));
  }
  return PQA_OK;
}

// The partials of the luma statistics, the extension rings of the blocks whose features are on (NaN until a batch writes a
// row) and the record ring (zeros).  The last part of pqa_create: every fill the parts have queued is done when it returns.
int alloc_rings(pqa_ctx* c) {
  try {
    c->ring.init(c->capacity);
  } catch (...) {
    return fail(c, PQA_ENOMEM, "out of host memory");
  }
  PQACHK(dev_alloc(c, &c->luma_part, (size_t)kLumaBlocks * 3 * c->B));
  PQACHK(dev_alloc(c, &c->records, (size_t)c->capacity * PQA_RECORD_DOUBLES));
  for (int i = 0; i < kExtBlocks; ++i) {
    if (!(c->cfg.features & kExtBlock[i].features)) continue;
    PQACHK(dev_alloc(c, &c->ext[i], (size_t)c->capacity * kExtBlock[i].doubles));
    HIPCHK(c, launch_ext_fill_nan(c->stream, c->ext[i], 0, c->capacity, c->capacity, kExtBlock[i].doubles));
  }
  HIPCHK(c, hipMemsetAsync(c->records, 0, (size_t)c->capacity * PQA_RECORD_DOUBLES * sizeof(double), c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return PQA_OK;
}

// The blocks written on the frames that get spatial features only: with n_subsample > 1 the rows of the batch are NaN first.
int fill_ext_nan(pqa_ctx* c, Batch& b) {
  for (int i = 0; b.k > 1 && i < kExtBlocks; ++i)
    if (kExtBlock[i].spatial && c->ext[i])
      HIPCHK(c, launch_ext_fill_nan(b.st_misc, c->ext[i], b.slot(0), b.n, c->capacity, kExtBlock[i].doubles));
  return PQA_OK;
}

int alloc_ssim_family(pqa_ctx* c) {
  const uint32_t feat = c->cfg.features;
  const int w = c->pw[0], h = c->ph[0], B = c->B;
  // MS-SSIM scales 1..4 hold ~5.3 bytes per luma sample and frame (22 MB per 2160p frame): the pyramid is walked ssf_sb
  // frames at a time, at most 320 MiB of planes
  size_t per_frame = 0;
  int sw = w, sh = h;
  for (int j = 0; j < kMsScales; ++j) {
    Level& L = c->ms_lv[j];
    L.w = sw; L.h = sh;
    if (j > 0) { L.pitch = round_up(sw, 16); L.frame_pitch = L.pitch * sh; per_frame += (size_t)L.frame_pitch * 2 * sizeof(float); }
    c->ms_tiles[j] = ssf_tiles(sw, sh);
    sw = (sw + 1) / 2; sh = (sh + 1) / 2;
  }
  c->ssf_sb = B;
  if ((feat & PQA_FEAT_MS_SSIM) && per_frame) {
    const int64_t sb = (int64_t)(320ll << 20) / (int64_t)per_frame;
    c->ssf_sb = (int)(sb < 1 ? 1 : sb < B ? sb : B);
  }
  const int SB = c->ssf_sb;
  for (int j = 0; (feat & PQA_FEAT_MS_SSIM) && j < kMsScales; ++j) {
    Level& L = c->ms_lv[j];
    if (j > 0) {
      PQACHK(dev_alloc(c, &L.ref, (size_t)L.frame_pitch * SB));
      PQACHK(dev_alloc(c, &L.dis, (size_t)L.frame_pitch * SB));
    }
    PQACHK(dev_alloc(c, &c->ms_part[j], (size_t)c->ms_tiles[j] * 4 * SB));
  }
  if (feat & PQA_FEAT_FLOAT_SSIM) {
    c->fs_box = ssf_decimation(w, h);
    c->fs_tiles = ssf_tiles((w + c->fs_box - 1) / c->fs_box, (h + c->fs_box - 1) / c->fs_box);
    PQACHK(dev_alloc(c, &c->fs_part, (size_t)c->fs_tiles * 4 * SB));
  }
  return PQA_OK;
}

// The SSIM family, ssf_sb frames at a time (the MS-SSIM pyramid is sized for that many).
int run_ssim_family(pqa_ctx* c, Batch& b) {
  const bool fs = c->cfg.features & PQA_FEAT_FLOAT_SSIM, ms = c->cfg.features & PQA_FEAT_MS_SSIM;
  if (!fs && !ms) return PQA_OK;
  const hipStream_t st = b.st_misc;
  for (int s0 = 0; s0 < b.sp_n; s0 += c->ssf_sb) {
    const int m = b.sp_n - s0 < c->ssf_sb ? b.sp_n - s0 : c->ssf_sb;
    const PlaneRun r0 = frames_from(b.rs[0], s0, b.es), d0 = frames_from(b.ds[0], s0, b.es);
    SsfFinalizeArgs sa{};
    sa.n_frames = m;
    sa.ext = c->ext[BLK_MAIN];
    sa.ext_stride = PQA_EXT_DOUBLES;
    sa.slot_base = b.slot(b.e0 + (int64_t)s0 * b.k);
    sa.slot_step = b.k;
    sa.capacity = c->capacity;
    if (fs) {
      sa.fs_part = c->fs_part; sa.fs_tiles = c->fs_tiles;
      const int dw = (b.w + c->fs_box - 1) / c->fs_box, dh = (b.h + c->fs_box - 1) / c->fs_box;
      sa.fs_norm = 1.0 / ((double)(dw - 10) * (dh - 10));
      ProfScope ps(c, 16, m, st);
      HIPCHK(c, launch_ssf_map(st, c->elem, r0, d0, m, b.w, b.h, c->fs_box, c->inv_scale, c->fs_part));
      if (!ms) HIPCHK(c, launch_ssf_finalize(st, sa));
    }
    if (ms) {
      ProfScope ps(c, 15, m, st);
      RunPair cur{r0, d0};
      Elem ce = c->elem;
      for (int j = 0; j < kMsScales; ++j) {
        const Level& L = c->ms_lv[j];
        sa.ms_part[j] = c->ms_part[j]; sa.ms_tiles[j] = c->ms_tiles[j];
        sa.ms_norm[j] = 1.0 / ((double)(L.w - 10) * (L.h - 10));
        if (j == 0) {   // scale 0 writes scale 1's planes in the same launch (the caller's pair is read once)
          const MutRunPair N = level_out(c->ms_lv[1]);
          HIPCHK(c, launch_ssf_map(st, ce, cur.ref, cur.dis, m, L.w, L.h, 1, c->inv_scale, c->ms_part[0], N.ref, N.dis));
        } else {
          HIPCHK(c, launch_ssf_map(st, ce, cur.ref, cur.dis, m, L.w, L.h, 1, c->inv_scale, c->ms_part[j]));
        }
        if (j + 1 < kMsScales) {
          const MutRunPair N = level_out(c->ms_lv[j + 1]);
          if (j > 0) HIPCHK(c, launch_ssf_down(st, ce, cur.ref, cur.dis, m, L.w, L.h, c->inv_scale, N.ref, N.dis));
          cur = level_in(c->ms_lv[j + 1]);
          ce = ELEM_F32;
        }
      }
      HIPCHK(c, launch_ssf_finalize(st, sa));
    }
  }
  return PQA_OK;
}

int alloc_ciede(pqa_ctx* c) {
  c->ciede_tiles_n = ciede_tiles(c->pw[1], c->ph[1]);
  return dev_alloc(c, &c->ciede_part, (size_t)c->ciede_tiles_n * c->B);
}

// CIEDE2000 on Y, U, V of the frames that get spatial features; the epilogue writes slots 20 / 21 of their rows only.
int run_ciede(pqa_ctx* c, Batch& b) {
  if (!(c->cfg.features & PQA_FEAT_CIEDE) || b.sp_n == 0) return PQA_OK;
  CiedeFinalizeArgs ca{};
  ca.n_frames = b.sp_n;
  ca.ext = c->ext[BLK_MAIN];
  ca.ext_stride = PQA_EXT_DOUBLES;
  ca.slot_base = b.slot(b.e0);
  ca.slot_step = b.k;
  ca.capacity = c->capacity;
  ca.partials = c->ciede_part;
  ca.n_tiles = c->ciede_tiles_n;
  ca.norm = 1.0 / ((double)b.w * b.h);
  ProfScope ps(c, 4, b.sp_n, b.st_misc);
  HIPCHK(c, launch_ciede(b.st_misc, c->elem, b.rs, b.ds, b.sp_n, b.w, b.h, (int)c->cfg.chroma_hshift, (int)c->cfg.chroma_vshift,
                         (int)c->cfg.bit_depth, c->ciede_part));
  HIPCHK(c, launch_ciede_finalize(b.st_misc, ca));
  return PQA_OK;
}

// CAMBI's work planes: 7 bytes per sample of the five scales (~77 MB per 2160p frame), at most ~512 MiB per pass.
int alloc_cambi(pqa_ctx* c) {
  c->cambi_prm = cambi_params(c->pw[0], c->ph[0]);
  const CambiParams& cp = c->cambi_prm;
  HIPCHK(c, cambi_prepare(cp, (int)c->cfg.bit_depth));
  const int64_t per_frame = cp.off[kCambiScales] * 7 + (int64_t)cp.chunk[kCambiScales] * 8;
  const int64_t sb = (int64_t)(512ll << 20) / per_frame;
  c->cambi_sb = (int)(sb < 1 ? 1 : sb < c->B ? sb : c->B);
  const size_t SB = (size_t)c->cambi_sb;
  PQACHK(dev_alloc(c, &c->cambi_wk.plane, (size_t)cp.off[kCambiScales] * SB));
  PQACHK(dev_alloc(c, &c->cambi_wk.mask, (size_t)cp.off[kCambiScales] * SB));
  PQACHK(dev_alloc(c, &c->cambi_wk.cmap, (size_t)cp.off[kCambiScales] * SB));
  PQACHK(dev_alloc(c, &c->cambi_wk.hist, (size_t)kCambiScales * 2048 * SB));
  PQACHK(dev_alloc(c, &c->cambi_wk.sel, (size_t)kCambiScales * 4 * SB));
  return dev_alloc(c, &c->cambi_wk.partials, (size_t)cp.chunk[kCambiScales] * SB);
}

// CAMBI of the distorted (and, FULL_REF, the reference) luma, cambi_sb frames at a time; slots 22 / 23 of their rows.
int run_cambi(pqa_ctx* c, Batch& b) {
  if (!(c->cfg.features & PQA_FEAT_CAMBI)) return PQA_OK;
  for (int s0 = 0; s0 < b.sp_n; s0 += c->cambi_sb) {
    const int m = b.sp_n - s0 < c->cambi_sb ? b.sp_n - s0 : c->cambi_sb;
    const int slot_base = b.slot(b.e0 + (int64_t)s0 * b.k);
    HIPCHK(c, launch_cambi(b.st_misc, c->elem, frames_from(b.ds[0], s0, b.es), m, b.w, b.h, (int)c->cfg.bit_depth, c->cambi_prm,
                           c->cambi_wk, c->ext[BLK_MAIN], PQA_EXT_DOUBLES, PQA_EXT_CAMBI, slot_base, b.k, c->capacity));
    if (c->cfg.features & PQA_FEAT_CAMBI_FULL_REF)
      HIPCHK(c, launch_cambi(b.st_misc, c->elem, frames_from(b.rs[0], s0, b.es), m, b.w, b.h, (int)c->cfg.bit_depth, c->cambi_prm,
                             c->cambi_wk, c->ext[BLK_MAIN], PQA_EXT_DOUBLES, PQA_EXT_CAMBI_SOURCE, slot_base, b.k, c->capacity));
  }
  return PQA_OK;
}

int alloc_psnr_hvs(pqa_ctx* c) {
  HIPCHK(c, psnr_hvs_prepare());
  psnr_hvs_geometry(c->pw, c->ph, &c->phv_geo);
  return dev_alloc(c, &c->phv_part, (size_t)c->phv_geo.tile0[3] * c->B);
}

// PSNR-HVS on Y, Cb, Cr of the frames that get spatial features, into slots 0..6 of their rows of the second block.
int run_psnr_hvs(pqa_ctx* c, Batch& b) {
  if (!(c->cfg.features & PQA_FEAT_PSNR_HVS) || b.sp_n == 0) return PQA_OK;
  PsnrHvsFinalizeArgs pa{};
  pa.n_frames = b.sp_n;
  pa.ext2 = c->ext[BLK_PSNR_HVS];
  pa.ext_stride = PQA_EXT2_DOUBLES;
  pa.slot_base = b.slot(b.e0);
  pa.slot_step = b.k;
  pa.capacity = c->capacity;
  pa.partials = c->phv_part;
  for (int p = 0; p < 4; ++p) pa.tile0[p] = c->phv_geo.tile0[p];
  for (int p = 0; p < 3; ++p) pa.blocks[p] = c->phv_geo.nbx[p] * c->phv_geo.nby[p];
  pa.peak = (double)((1 << c->cfg.bit_depth) - 1);
  HIPCHK(c, launch_psnr_hvs(b.st_misc, c->elem, b.rs, b.ds, b.sp_n, c->phv_geo, c->phv_part));
  HIPCHK(c, launch_psnr_hvs_finalize(b.st_misc, pa));
  return PQA_OK;
}

int alloc_xpsnr(pqa_ctx* c) {
  xpsnr_geometry(c->pw[0], c->ph[0], c->pw[1], c->ph[1], c->n_planes, (int)c->cfg.bit_depth, &c->xp_geo);
  PQACHK(dev_alloc(c, &c->xp_blk, (size_t)c->xp_geo.n_blk * kXpBlockVals * c->B));
  PQACHK(dev_alloc(c, &c->xp_w, (size_t)c->xp_geo.n_blk * c->B));
  for (int j = 0; j < 2; ++j) PQACHK(hist_alloc(c, &c->xp_hist[j], 0));
  return PQA_OK;
}

// XPSNR on every frame: its predecessors come from the batch, the caller's halo, the kept pair or the armed history.
int run_xpsnr(pqa_ctx* c, Batch& b) {
  if (!(c->cfg.features & PQA_FEAT_XPSNR)) return PQA_OK;
  const Pred h1 = b.prev.base ? b.prev : held(c->xp_chain, c->xp_hist, b.first - 1, b.es);
  const Pred h2 = held(c->xp_chain, c->xp_hist, b.first - 2, b.es);
  XpFinalizeArgs xa{};
  xa.n_frames = b.n;
  xa.blk = c->xp_blk;
  xa.wbuf = c->xp_w;
  xa.ext3 = c->ext[BLK_XPSNR];
  xa.ext_stride = PQA_EXT3_DOUBLES;
  xa.slot_base = b.slot(0);
  xa.capacity = c->capacity;
  xa.g = c->xp_geo;
  HIPCHK(c, launch_xpsnr_blocks(b.st_misc, c->elem, b.r, b.d, b.n, h1.base, h1.pitch, h2.base, h2.pitch,
                                (c->cfg.features & PQA_FEAT_XPSNR_HFR) != 0, c->xp_geo, c->xp_blk));
  HIPCHK(c, launch_xpsnr_finalize(b.st_misc, xa));
  return PQA_OK;
}

int alloc_siti(pqa_ctx* c) {
  PQACHK(dev_alloc(c, &c->st_part, (size_t)siti_partials(c->pw[0], c->ph[0]) * 2 * 4 * c->B));
  for (int z = 0; z < 2; ++z) PQACHK(hist_alloc(c, &c->st_hist[z], 0));
  return PQA_OK;
}

// SI / TI of both clips on every frame; frame first-1 of each clip: the caller's halo (reference), the kept or the armed
// plane; none at a chain start.
int run_siti(pqa_ctx* c, Batch& b) {
  const uint32_t feat = c->cfg.features;
  if (!(feat & PQA_FEAT_SITI)) return PQA_OK;
  const Pred p[2] = {held(c->st_chain[0], &c->st_hist[0], b.first - 1, b.es),
                     b.prev.base ? b.prev : held(c->st_chain[1], &c->st_hist[1], b.first - 1, b.es)};
  const void* sp0[2] = {p[0].base, p[1].base};
  const int64_t spp[2] = {p[0].pitch, p[1].pitch};
  const PlaneRun sc[2] = {b.d[0], b.r[0]};
  const bool sfull[2] = {(feat & PQA_FEAT_SITI_DIS_FULL) != 0, (feat & PQA_FEAT_SITI_REF_FULL) != 0};
  HIPCHK(c, launch_siti(b.st_misc, c->elem, sc, sp0, spp, sfull, 2, b.n, b.w, b.h, c->st_part, c->ext[BLK_SITI], PQA_EXT4_DOUBLES, b.slot(0),
                        c->capacity, nullptr));
  return PQA_OK;
}

int alloc_integrity(pqa_ctx* c) {
  PQACHK(dev_alloc(c, &c->ig_part, (size_t)c->B * 3 * kIntegrityBlocks * 2));
  for (int p = 0; p < c->n_planes; ++p) PQACHK(hist_alloc(c, &c->ig_hist[p], p));
  return PQA_OK;
}

// SAD of every plane of the distorted frames against their predecessors, and the black count; frame first-1: the kept or the
// armed planes, none at a chain start.
int run_integrity(pqa_ctx* c, Batch& b) {
  if (!(c->cfg.features & PQA_FEAT_INTEGRITY)) return PQA_OK;
  const bool have = c->ig_chain.find(b.first - 1) == 0;
  const void* ip0[3] = {nullptr, nullptr, nullptr};
  int64_t ipp[3] = {0, 0, 0};
  for (int p = 0; have && p < c->n_planes; ++p) {
    ip0[p] = c->ig_hist[p].base;
    ipp[p] = c->ig_hist[p].pitch / b.es;
  }
  HIPCHK(c, launch_integrity(b.st_misc, c->elem, b.d, ip0, ipp, c->pw, c->ph, c->n_planes, b.n, false, c->black_thr, c->ig_part,
                             c->ext[BLK_INTEGRITY], PQA_EXT5_DOUBLES, b.slot(0), c->capacity, nullptr));
  return PQA_OK;
}

int run_finalize(pqa_ctx* c, Batch& b) {
  const uint32_t feat = c->cfg.features;
  FinalizeArgs fa{};
  for (int s = 0; s < 4; ++s) {
    fa.vif_part[s] = c->vif_part[s]; fa.vif_tiles[s] = c->vif_fixed ? c->vif_tiles[s] : b.vif_np[s];
    fa.vif_fx_part[s] = c->vif_fixed ? c->vif_fx_part[s] : nullptr;
    fa.adm_part[s] = c->adm_part[s]; fa.adm_tiles[s] = c->adm_fixed ? c->adm_tiles[s] : b.adm_np[s]; fa.adm_area[s] = c->adm_area[s];
    fa.adm_fx_part[s] = c->adm_fixed ? c->adm_fx_part[s] : nullptr;
    fa.adm_fx_tiles_x[s] = adm_tiles_x(c->adm_fx[s].band_w);
    fa.adm_fx_top[s] = c->adm_fx[s].top; fa.adm_fx_bottom[s] = c->adm_fx[s].bottom;
    fa.adm_fx_num_shift[s] = c->adm_fx[s].num_row_shift; fa.adm_fx_den_shift[s] = c->adm_fx[s].den_row_shift;
  }
  fa.motion_part = c->motion_part;
  fa.motion_tiles = c->motion_fixed ? c->motion_tiles_n : b.motion_np;
  fa.motion_norm = (double)c->inv_scale / ((double)b.w * b.h);
  fa.motion_fx_part = c->motion_fixed ? c->motion_fx_part : nullptr;
  fa.motion_wh = (unsigned)b.w * (unsigned)b.h;
  for (int p = 0; p < 3; ++p) {
    fa.sse_part[p] = c->sse_part[p];
    fa.sse_use_a[p] = b.sse_a[p] ? 1 : 0;
    fa.sse_part_b[p] = b.sse_b[p] ? c->sse_part_b[p] : nullptr;
    fa.sse_tile_part[p] = b.sse_t[p] ? c->sse_tile_part[p] : nullptr;
    fa.ssim_part[p] = c->ssim_part[p]; fa.ssim_tiles[p] = c->ssim_tiles_n[p]; fa.ssim_norm[p] = c->ssim_norm[p];
  }
  fa.adm_fx_acc = c->adm_fx_acc;
  fa.records = c->records;
  fa.record_stride = PQA_RECORD_DOUBLES;
  fa.capacity = c->capacity;
  // one launch over `frames` rows from slot_base on, every step-th, for the features of `on`
  const auto finalize_rows = [&](int frames, int slot_base, int step, uint32_t on) {
    fa.n_frames = frames;
    fa.slot_base = slot_base; fa.slot_step = step;
    fa.has_vif = !!(on & PQA_FEAT_VIF); fa.has_adm = !!(on & PQA_FEAT_ADM); fa.has_motion = !!(on & PQA_FEAT_MOTION);
    fa.n_sse_planes = (on & PQA_FEAT_PSNR) ? b.n_sse : 0; fa.n_ssim_planes = (on & PQA_FEAT_SSIM) ? b.n_ssim : 0;
    return launch_finalize(b.st, fa);
  };
  const uint32_t spatial = PQA_FEAT_VIF | PQA_FEAT_ADM;
  ProfScope ps(c, 14, b.n, b.st);
  if (b.k > 1) {   // the spatial features on their frames, the others on every frame
    if (b.sp_n > 0 && (feat & spatial)) HIPCHK(c, finalize_rows(b.sp_n, b.slot(b.e0), b.k, feat & spatial));
    HIPCHK(c, finalize_rows(b.n, b.slot(0), 1, feat & ~spatial));
  } else {
    HIPCHK(c, finalize_rows(b.n, b.slot(0), 1, feat));
  }
  return PQA_OK;
}

// The caller's host plane p (rows `stride` bytes apart) into a history plane, before it is armed; the stream is idle.
hipError_t hist_arm(pqa_ctx* c, const HistPlane& dst, const void* src, int64_t stride, int p) {
  return hipMemcpy2D(dst.base, dst.pitch, src, stride, (size_t)c->pw[p] * c->esize, c->ph[p], hipMemcpyHostToDevice);
}

// A keep copy: plane p of a device frame (pitch in bytes) into a history plane, on the main stream.
hipError_t hist_keep(pqa_ctx* c, const HistPlane& dst, const void* src, int64_t src_pitch, int p) {
  return hipMemcpy2DAsync(dst.base, dst.pitch, src, src_pitch, (size_t)c->pw[p] * c->esize, c->ph[p], hipMemcpyDeviceToDevice,
                          c->stream);
}

// What a chain's end() asks for: frames of the first np planes of `clip`, or the caller's prev plane, into planes[slot][np].
int keep_chain(pqa_ctx* c, const Batch& b, host::FrameChain& chain, const HistPlane* planes, const pqa_device_clip* clip,
               int np) {
  host::FrameChain::Copy cp[host::FrameChain::kMaxDepth];
  const int m = chain.end(b.first, b.n, b.prev.base != nullptr, cp);
  for (int i = 0; i < m; ++i)
    for (int p = 0; p < np; ++p) {
      const bool from_prev = cp[i].src == host::FrameChain::kFromPrev;
      const void* src = from_prev ? b.prev.base : (const uint8_t*)clip->plane[p] + (int64_t)cp[i].src * clip->frame_pitch[p];
      HIPCHK(c, hist_keep(c, planes[cp[i].slot * np + p], src, from_prev ? b.prev.pitch * b.es : clip->row_pitch[p], p));
    }
  return PQA_OK;
}

// The last frames of this batch, kept so that the next one continues the chains (behind the join: this batch's kernels have
// read the old planes; behind the batch event: pqa_collect does not wait for these copies).
int keep_histories(pqa_ctx* c, const Batch& b) {
  for (const History& h : histories(c))
    if (c->cfg.features & h.feature) PQACHK(keep_chain(c, b, *h.chain, h.planes, h.dis ? b.dis : b.ref, h.np));
  return PQA_OK;
}

// The rows of a plane the kernels read where it lies (`who`: "reference plane 1", "halo"; plane p of the context, row pitch in
// bytes): no row pitch below a row, and a span (row pitch x rows) the kernels can address.  The VIF, ADM and motion kernels
// form unsigned 32-bit byte offsets from the plane's base (pqa_device.h), so a span ends at 2^32 - 1; from 2^31 on their
// launchers go tiled by themselves.  The siti kernel stops at 2^31 and has no partner.  Every other feature's kernels add
// 64-bit row offsets to a pointer.  No device call.
int check_plane_rows(pqa_ctx* c, const char* who, int p, int64_t row_pitch) {
  const int64_t row = (int64_t)c->pw[p] * c->esize, rows = c->ph[p];
  if (row_pitch < row)
    return fail(c, PQA_EINVAL, "%s: row pitch %lld is below a row of %lld bytes", who, (long long)row_pitch, (long long)row);
  if (row_pitch > ((1ll << 32) - 1) / rows)
    return fail(c, PQA_EINVAL, "%s spans %lld rows of pitch %lld: the limit of a plane is 2^32 - 1 bytes (32-bit offsets)", who,
                (long long)rows, (long long)row_pitch);
  if (p == 0 && (c->cfg.features & PQA_FEAT_SITI) && row_pitch > ((1ll << 31) - 1) / rows)
    return fail(c, PQA_EINVAL, "siti: %s spans %lld rows of pitch %lld: the limit of its kernel is 2^31 - 1 bytes", who,
                (long long)rows, (long long)row_pitch);
  return PQA_OK;
}

int process_batch(pqa_ctx* c, int64_t first, int n, const pqa_device_clip* ref, const pqa_device_clip* dis,
                  const void* prev, int64_t prev_pitch_bytes) {
  const uint32_t feat = c->cfg.features;
  const int es = c->esize;
  int rc = PQA_OK;
  for (int p = 0; p < c->n_planes; ++p) {
    if (ref->row_pitch[p] % es || dis->row_pitch[p] % es || ref->frame_pitch[p] % es || dis->frame_pitch[p] % es)
      return fail(c, PQA_EINVAL, "plane %d pitch is not a multiple of the sample size", p);
    if (!ref->plane[p] || !dis->plane[p]) return fail(c, PQA_EINVAL, "plane %d pointer is null", p);
    char who[32];
    snprintf(who, sizeof who, "reference plane %d", p);
    if ((rc = check_plane_rows(c, who, p, ref->row_pitch[p])) != PQA_OK) return rc;
    snprintf(who, sizeof who, "distorted plane %d", p);
    if ((rc = check_plane_rows(c, who, p, dis->row_pitch[p])) != PQA_OK) return rc;
  }
  if (prev && (feat & (PQA_FEAT_MOTION | PQA_FEAT_XPSNR | PQA_FEAT_SITI))) {
    if (prev_pitch_bytes % es) return fail(c, PQA_EINVAL, "halo pitch is not a multiple of the sample size");
    if ((rc = check_plane_rows(c, "halo plane", 0, prev_pitch_bytes)) != PQA_OK) return rc;
  }
  if ((rc = check_slots_free(c, first, n)) != PQA_OK) return rc;
  c->started = true;

  Batch b{};
  b.first = first; b.n = n; b.es = es; b.w = c->pw[0]; b.h = c->ph[0]; b.capacity = c->capacity;
  b.ref = ref; b.dis = dis;
  if (prev) b.prev = Pred{prev, prev_pitch_bytes / es};
  // frames that get spatial features (libvmaf n_subsample: index % k == 0)
  b.k = c->k_sub; b.e0 = 0; b.sp_n = n;
  if (b.k > 1) {
    b.e0 = (int)((b.k - first % b.k) % b.k);
    b.sp_n = b.e0 < n ? (n - b.e0 + b.k - 1) / b.k : 0;
  }
  for (int p = 0; p < c->n_planes; ++p) {
    b.r[p] = clip_run(ref, p, es);
    b.d[p] = clip_run(dis, p, es);
    b.rs[p] = frames_from(b.r[p], b.e0, es); b.rs[p].frame_pitch *= b.k;
    b.ds[p] = frames_from(b.d[p], b.e0, es); b.ds[p].frame_pitch *= b.k;
  }
  // (with EVERY kernel event-timed -- the breakdown pass of bench.py -- the chains stay on one stream, so that a kernel's
  // figure is its own and not its share of a crowded device; a subset mask, as in the timed region, changes nothing)
  b.multi = c->multi_stream && !(c->prof && c->prof_mask == 0xffffffffu);
  b.st = c->stream;
  b.st_adm = b.multi ? c->aux[0] : b.st; b.st_misc = b.multi ? c->aux[1] : b.st;
  b.fork_late = b.multi && c->multi_stream == 2 && (feat & PQA_FEAT_VIF) && !c->vif_fixed && b.sp_n > 0;   // run_vif forks
  for (int s = 0; s < 4; ++s) { b.vif_np[s] = c->vif_tiles[s]; b.adm_np[s] = c->adm_tiles[s]; }
  b.motion_np = c->motion_tiles_n;
  // the frames in front of this batch: armed planes are bound, a batch that does not continue a chain starts one (the chain
  // of a feature that is off is never read)
  for (const History& h : histories(c)) h.chain->begin(first);

  // the VIF chain on the main stream, the ADM chain on the second, everything else in this order on the third
  static int (*const kSteps[])(pqa_ctx*, Batch&) = {run_vif,   run_adm,   run_motion,   run_psnr_ssim, fill_ext_nan, run_ssim_family,
                                                    run_ciede, run_cambi, run_psnr_hvs, run_xpsnr,     run_siti,     run_integrity};
  if (b.multi && !b.fork_late && (rc = fork_streams(c, b)) != PQA_OK) return rc;
  for (const auto step : kSteps)
    if ((rc = step(c, b)) != PQA_OK) return rc;
  if (b.multi && (rc = join_streams(c, b)) != PQA_OK) return rc;
  if ((rc = run_finalize(c, b)) != PQA_OK) return rc;
  {  // the records of this batch are complete here: one event per batch, so pqa_collect waits for ITS batch only
    const uint64_t seq = c->batch_seq + 1;
    const int e = (int)(seq % kBatchEvents);
    HIPCHK(c, hipEventRecord(c->batch_ev[e], b.st));
    c->batch_ev_seq[e] = seq;
    c->batch_seq = seq;
    claim_slots(c, first, n, seq);
  }
  return keep_histories(c, b);
}

// One side of a frame pair as the library lays it out itself: pqa_ctx::slot.
host::ClipLayout slot_layout(const pqa_ctx* c) {
  size_t rb[3] = {0, 0, 0};
  for (int p = 0; p < c->n_planes; ++p) rb[p] = (size_t)c->pw[p] * c->esize;
  return host::clip_layout(c->n_planes, rb, c->ph, 64, 256);
}

// The frames of layout L that lie frame_pitch bytes apart from `base` on, as the kernels take a clip.
pqa_device_clip clip_at(const void* base, const host::ClipLayout& L, int64_t frame_pitch) {
  pqa_device_clip d{};
  for (int p = 0; p < L.n_planes; ++p) {
    d.plane[p] = (const uint8_t*)base + L.off[p];
    d.row_pitch[p] = L.plane[p].pitch;
    d.frame_pitch[p] = frame_pitch;
  }
  return d;
}
// side sd of the slots at `base` (a staging half's device copy, surf_dev)
pqa_device_clip slot_clip(const pqa_ctx* c, const uint8_t* base, int sd) {
  return clip_at(base + sd * c->slot.frame_bytes, c->slot, (int64_t)c->slot_bytes());
}

// ---- the staging halves (pqa::Half) ------------------------------------------------------------
// The copy stream and a pair's events, made by whichever host path comes first.
int ensure_copy_path(pqa_ctx* c, Half (&pair)[2]) {
  if (!c->copy_stream) HIPCHK(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
  for (Half& H : pair) {
    if (!H.copied) HIPCHK(c, hipEventCreateWithFlags(&H.copied, hipEventDisableTiming));
    if (!H.computed) HIPCHK(c, hipEventCreateWithFlags(&H.computed, hipEventDisableTiming));
  }
  return PQA_OK;
}

hipError_t half_alloc(Half& H, size_t bytes) {
  hipError_t e = hipHostMalloc((void**)&H.pinned, bytes, hipHostMallocDefault);
  if (e == hipSuccess) e = hipMalloc((void**)&H.dev, bytes);
  if (e == hipSuccess) H.cap = bytes;
  return e;
}

void half_free(Half& H) {   // nothing reads it any more; the right device is current
  if (H.pinned) hipHostFree(H.pinned);
  if (H.dev) hipFree(H.dev);
  H.pinned = H.dev = nullptr;
  H.cap = 0;
}

// Before the host packs `bytes` into H: the upload that last read the pinned buffer has passed; a half too small is replaced
// by a larger one once the kernels that last read its device copy are through; the next upload waits for those kernels.
int half_claim(pqa_ctx* c, Half& H, size_t bytes) {
  if (H.copied_pending) {
    HIPCHK(c, hipEventSynchronize(H.copied));
    H.copied_pending = false;
  }
  if (H.cap < bytes) {
    if (H.computed_pending) {
      HIPCHK(c, hipEventSynchronize(H.computed));
      H.computed_pending = false;
    }
    half_free(H);
    HIPCHK(c, half_alloc(H, bytes));
  }
  if (H.computed_pending) {
    HIPCHK(c, hipStreamWaitEvent(c->copy_stream, H.computed, 0));
    H.computed_pending = false;
  }
  return PQA_OK;
}

std::array<Half*, 4> all_halves(pqa_ctx* c) { return {{&c->half[0], &c->half[1], &c->chunk_half[0], &c->chunk_half[1]}}; }

// H's uploads are queued: the kernels wait for them.
int half_sent(pqa_ctx* c, Half& H) {
  HIPCHK(c, hipEventRecord(H.copied, c->copy_stream));
  H.copied_pending = true;
  HIPCHK(c, hipStreamWaitEvent(c->stream, H.copied, 0));
  return PQA_OK;
}

// The kernels that read H's device copy are queued.
int half_launched(pqa_ctx* c, Half& H) {
  HIPCHK(c, hipEventRecord(H.computed, c->stream));
  H.computed_pending = true;
  return PQA_OK;
}

int ensure_staging(pqa_ctx* c) {
  if (c->staging_ready) return PQA_OK;
  const size_t half_bytes = c->slot_bytes() * c->HB;
  bool reused = false;
  if (staging_cache_enabled()) {
    std::lock_guard<std::mutex> g(g_staging_mu);
    if (g_staging.bytes == half_bytes && g_staging.device == c->device) {
      for (int i = 0; i < 2; ++i) {
        c->half[i].pinned = g_staging.pinned[i];
        c->half[i].dev = g_staging.dev[i];
        c->half[i].cap = half_bytes;
        g_staging.pinned[i] = g_staging.dev[i] = nullptr;
      }
      g_staging.bytes = 0;
      g_staging.device = -1;
      reused = true;
    }
  }
  PQACHK(ensure_copy_path(c, c->half));
  if (!reused) {
    // Pinning costs ~40 us per MiB (a 2160p 4:2:0 half of 8 frame pairs: 8 ms): only the first half is needed before
    // the first frame can be packed; the second is pinned by a helper thread while the first one fills.
    HIPCHK(c, half_alloc(c->half[0], half_bytes));
    const auto pin_second = [c, half_bytes] {
      const hipError_t e = hipSetDevice(c->device);
      c->pin_err = e == hipSuccess ? half_alloc(c->half[1], half_bytes) : e;
    };
    try {
      c->pin_thread = std::thread(pin_second);
    } catch (...) {   // no thread to be had: pin it here
      pin_second();
    }
  }
  c->staging_ready = true;
  return PQA_OK;
}

// Before half i is touched: the helper thread that pins the second half has to be done with it (joining it also makes
// its writes to half[1] visible here).
int staging_half_ready(pqa_ctx* c, int i) {
  if (i == 0) return PQA_OK;
  if (c->pin_thread.joinable()) c->pin_thread.join();
  if (c->pin_err != hipSuccess)
    return fail(c, c->pin_err == hipErrorOutOfMemory ? PQA_ENOMEM : PQA_EDEVICE, "pinning the second staging half failed: %s",
                hipGetErrorString(c->pin_err));
  return PQA_OK;
}

int flush_pending(pqa_ctx* c) {
  if (c->pending == 0) return PQA_OK;
  Half& H = c->half[c->cur_half];
  PQACHK(half_sent(c, H));
  const pqa_device_clip r = slot_clip(c, H.dev, 0), d = slot_clip(c, H.dev, 1);
  const int n = c->pending;
  PQACHK(check_slots_free(c, c->pending_first, n));   // PQA_ESTATE: nothing launched, the packed frames stay pending (collect, then flush again)
  c->pending = 0;
  PQACHK(process_batch(c, c->pending_first, n, &r, &d, nullptr, 0));
  PQACHK(half_launched(c, H));
  c->cur_half ^= 1;
  return PQA_OK;
}

// The helpers that pack large frames, made on first use (a context of small frames never starts a thread).
void ensure_pack_pool(pqa_ctx* c) {
  if (c->pack_pool_tried) return;
  c->pack_pool_tried = true;
  // threads packing a frame, the caller included.  Default 8: plain host buffers reach the PCIe ceiling with 4, frames
  // read from files (pread out of the page cache) or out of a memory-mapped file scale further (2160p through
  // analyze_videos: 880 frames/s with 4, 1 370 with 8; beyond that the box's noise decides, profiles/r04o_pack_threads.txt)
  const char* e = getenv("PQA_PACK_THREADS");
  int n = e ? atoi(e) : 8;
  const int hw = (int)std::thread::hardware_concurrency();
  if (hw > 0 && n > hw) n = hw;
  if (n > 1) {
    try { c->pack_pool.reset(new PackPool(n - 1)); } catch (...) { c->pack_pool.reset(); }   // serial packing then
  }
}

// n consecutive frame pairs (frame k's planes lie k * frame_step[side] bytes after src's; memory sources: n == 1) into
// staging slots and onto the copy stream.  A run is cut into chunks that fit the current staging half; within a chunk the
// helpers pack frame k + 1 while the caller queues the upload of frame k (PackPool::run_frames): one fork / join per
// chunk, the link busy from the first completed frame on.
int submit_run(pqa_ctx* c, int64_t first_index, int n_frames, const PlaneSrc (&src)[2][3], const int64_t (&frame_step)[2]) {
  if (c->cancelled.load()) return fail(c, PQA_ECANCELLED, "cancelled");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t slot_bytes = c->slot_bytes();
  int rc = PQA_OK;
  int done = 0;
  while (done < n_frames) {
    const int64_t frame_index = first_index + done;
    if (c->cancelled.load()) return fail(c, PQA_ECANCELLED, "cancelled");
    if (c->pending > 0 && frame_index != c->pending_first + c->pending) {
      rc = flush_pending(c);  // non-consecutive index starts a new run: the pending frames claim their slots first
      if (rc != PQA_OK) return rc;
    }
    rc = ensure_staging(c);
    if (rc != PQA_OK) return rc;
    int m = n_frames - done;
    if (m > c->HB - c->pending) m = c->HB - c->pending;
    if (m > PackPool::kMaxFrames) m = PackPool::kMaxFrames;
    // before anything is packed (the caller can collect and retry): against the claimed slots, and against the frames still
    // pending in this run (consecutive indices: they collide only when the run is as long as the ring)
    rc = check_slots_free(c, frame_index, m);
    if (rc != PQA_OK) return rc;
    if (c->pending + m > c->capacity)
      return fail(c, PQA_ESTATE, "more pending frames than result_capacity %d", c->capacity);
    rc = staging_half_ready(c, c->cur_half);   // the second half is pinned by a helper thread while the first one fills
    if (rc != PQA_OK) return rc;
    Half& H = c->half[c->cur_half];
    if (c->pending == 0) {   // the first frames into this half
      c->pending_first = frame_index;
      PQACHK(half_claim(c, H, H.cap));
    }
    const int slot0 = c->pending;
    // Pack into the pinned slots in ~1 MiB tasks (a 2160p 4:2:0 pair is 25 MB: one core's memcpy / pread, not PCIe, would
    // bound this path), drained by the caller and a few persistent helpers.
    bool ok = true;
    hipError_t copy_err = hipSuccess;
    const auto upload = [&](int k) {   // frame k of the chunk is complete in its pinned slot: queue its copy
      const size_t off = (size_t)(slot0 + k) * slot_bytes;
      copy_err = hipMemcpyAsync(H.dev + off, H.pinned + off, slot_bytes, hipMemcpyHostToDevice, c->copy_stream);
      return copy_err == hipSuccess;
    };
    try {  // no exception may cross the C ABI: if the task list or the helpers cannot be made, that is PQA_ENOMEM below
      c->pack_tasks.clear();
      static const unsigned task_bytes = [] { const char* e = getenv("PQA_PACK_TASK_KB"); const int kb = e ? atoi(e) : 0; return (unsigned)(kb > 0 ? kb : 1024) << 10; }();
      for (int k = 0; k < m; ++k)
        for (int side = 0; side < 2; ++side)
          host::pack_frame_tasks(c->pack_tasks, c->slot, H.pinned + (size_t)(slot0 + k) * slot_bytes + side * c->slot.frame_bytes,
                                 src[side], frame_step[side], done + k, k, task_bytes);
      if (slot_bytes >= (4u << 20)) ensure_pack_pool(c);
      if (c->pack_pool && slot_bytes >= (4u << 20)) {
        ok = c->pack_pool->run_frames(c->pack_tasks.data(), (int)c->pack_tasks.size(), m, upload);
      } else {
        int k_done = 0;
        for (size_t i = 0; i < c->pack_tasks.size() && ok; ++i) {
          ok = run_pack_task(c->pack_tasks[i]);
          if (ok && (i + 1 == c->pack_tasks.size() || c->pack_tasks[i + 1].frame != c->pack_tasks[i].frame)) ok = upload(k_done++);
        }
      }
    } catch (...) {
      return fail(c, PQA_ENOMEM, "out of host memory while staging frame %lld", (long long)frame_index);
    }
    if (copy_err != hipSuccess) return fail(c, PQA_EDEVICE, "hipMemcpyAsync failed: %s", hipGetErrorString(copy_err));
    if (!ok)   // nothing of this chunk becomes pending: its slots are simply packed again by the next submit
      return fail(c, PQA_EINVAL, "frame %lld%s: short read from a file source (truncated file or bad plane offset)",
                  (long long)frame_index, m > 1 ? " (or one of the frames after it in this run)" : "");
    c->pending += m;
    done += m;
    if (c->pending == c->HB) {
      rc = flush_pending(c);
      if (rc != PQA_OK) return rc;
    }
  }
  return PQA_OK;
}

int submit_one(pqa_ctx* c, int64_t frame_index, const PlaneSrc (&src)[2][3]) {
  const int64_t no_step[2] = {0, 0};
  return submit_run(c, frame_index, 1, src, no_step);
}

// ---- pqa_create, in parts -----------------------------------------------------------------------
// What a configuration must satisfy, the first failing rule reported; no device call.
int check_config(const pqa_config* cfg) {
  if (cfg->struct_size != sizeof(pqa_config)) return fail(nullptr, PQA_EINVAL, "pqa_config.struct_size mismatch");
  if (cfg->width < 16 || cfg->height < 16 || cfg->width > 16384 || cfg->height > 16384)
    return fail(nullptr, PQA_EINVAL, "unsupported frame size %ux%u (16..16384)", cfg->width, cfg->height);
  if (cfg->bit_depth != 8 && cfg->bit_depth != 10 && cfg->bit_depth != 12)
    return fail(nullptr, PQA_EINVAL, "unsupported bit depth %u (8, 10, 12)", cfg->bit_depth);
  if (cfg->n_planes != 1 && cfg->n_planes != 3) return fail(nullptr, PQA_EINVAL, "n_planes must be 1 or 3");
  if (cfg->chroma_hshift > 2 || cfg->chroma_vshift > 2) return fail(nullptr, PQA_EINVAL, "bad chroma shift");
  if ((cfg->features & ~(uint32_t)PQA_FEAT_KNOWN) || cfg->features == 0)
    return fail(nullptr, PQA_EINVAL, "bad feature mask 0x%x", cfg->features);
  if (cfg->features & PQA_FEAT_FLOAT_SSIM) {   // the decimated plane must hold one 11 x 11 window
    const int f = ssf_decimation((int)cfg->width, (int)cfg->height);
    if (ssf_tiles(((int)cfg->width + f - 1) / f, ((int)cfg->height + f - 1) / f) == 0)
      return fail(nullptr, PQA_EINVAL, "frame %ux%u too small for float_ssim (decimated by %d it must be >= 11x11)", cfg->width,
                  cfg->height, f);
  }
  if (cfg->features & PQA_FEAT_MS_SSIM) {      // the 5th scale must hold one 11 x 11 window
    int sw = (int)cfg->width, sh = (int)cfg->height;
    for (int j = 1; j < kMsScales; ++j) { sw = (sw + 1) / 2; sh = (sh + 1) / 2; }
    if (ssf_tiles(sw, sh) == 0)
      return fail(nullptr, PQA_EINVAL, "frame %ux%u too small for float_ms_ssim (5th scale %dx%d, needs >= 11x11: w, h >= 161)",
                  cfg->width, cfg->height, sw, sh);
  }
  if ((cfg->features & PQA_FEAT_CIEDE) && cfg->n_planes != 3)
    return fail(nullptr, PQA_EINVAL, "ciede2000 needs the chroma planes: n_planes must be 3 (got %u)", cfg->n_planes);
  if ((cfg->features & PQA_FEAT_CAMBI_FULL_REF) && !(cfg->features & PQA_FEAT_CAMBI))
    return fail(nullptr, PQA_EINVAL, "cambi full reference (PQA_FEAT_CAMBI_FULL_REF) needs PQA_FEAT_CAMBI");
  if ((cfg->features & PQA_FEAT_CAMBI) && cfg->bit_depth != 8 && cfg->bit_depth != 10)
    return fail(nullptr, PQA_EINVAL, "cambi supports bit depth 8 or 10 (got %u)", cfg->bit_depth);
  if ((cfg->features & PQA_FEAT_PSNR_HVS) && cfg->n_planes != 3)
    return fail(nullptr, PQA_EINVAL, "psnr_hvs needs the chroma planes: n_planes must be 3 (got %u)", cfg->n_planes);
  if ((cfg->features & PQA_FEAT_PSNR_HVS) &&
      (((cfg->width + (1u << cfg->chroma_hshift) - 1) >> cfg->chroma_hshift) < 8 ||
       ((cfg->height + (1u << cfg->chroma_vshift) - 1) >> cfg->chroma_vshift) < 8))
    return fail(nullptr, PQA_EINVAL, "psnr_hvs needs every plane >= 8x8 (frame %ux%u, chroma shifts %u, %u)", cfg->width,
                cfg->height, cfg->chroma_hshift, cfg->chroma_vshift);
  if ((cfg->features & PQA_FEAT_XPSNR_HFR) && !(cfg->features & PQA_FEAT_XPSNR))
    return fail(nullptr, PQA_EINVAL, "xpsnr second-order term (PQA_FEAT_XPSNR_HFR) needs PQA_FEAT_XPSNR");
  if (cfg->features & PQA_FEAT_XPSNR) {
    XpsnrGeometry g{};
    xpsnr_geometry((int)cfg->width, (int)cfg->height, (int)((cfg->width + (1u << cfg->chroma_hshift) - 1) >> cfg->chroma_hshift),
                   (int)((cfg->height + (1u << cfg->chroma_vshift) - 1) >> cfg->chroma_vshift), (int)cfg->n_planes,
                   (int)cfg->bit_depth, &g);
    if (g.bv == 2 && ((cfg->width | cfg->height) & 1))
      return fail(nullptr, PQA_EINVAL, "xpsnr needs an even width and height above 2048x1152 (its 2x2 activity; got %ux%u)",
                  cfg->width, cfg->height);
    if (g.nc_blk > g.n_blk || (cfg->n_planes == 3 && g.nc_blk == 0) || g.bsx + 4 > kXpLdsCols)
      return fail(nullptr, PQA_EINVAL, "xpsnr: unsupported block grid for %ux%u (chroma shifts %u, %u)", cfg->width,
                  cfg->height, cfg->chroma_hshift, cfg->chroma_vshift);
  }
  if ((cfg->features & (PQA_FEAT_SITI_REF_FULL | PQA_FEAT_SITI_DIS_FULL)) && !(cfg->features & PQA_FEAT_SITI))
    return fail(nullptr, PQA_EINVAL, "siti range bits (PQA_FEAT_SITI_REF_FULL / _DIS_FULL) need PQA_FEAT_SITI");
  if ((cfg->features & PQA_FEAT_SITI) && cfg->bit_depth != 8 && cfg->bit_depth != 10)
    return fail(nullptr, PQA_EINVAL, "siti supports bit depth 8 or 10 (got %u)", cfg->bit_depth);
  if (cfg->vif_border > PQA_VIF_BORDER_INTEGER || (cfg->fixed_point & ~(uint32_t)PQA_FIXED_ALL))
    return fail(nullptr, PQA_EINVAL, "bad vif_border %u / fixed_point 0x%x", cfg->vif_border, cfg->fixed_point);
  return PQA_OK;
}

// The environment switches, read once per context.
void read_switches(pqa_ctx* c) {
  // PQA_MULTI_STREAM=1: the ADM chain and the motion / PSNR / SSIM kernels on their own streams beside the VIF chain.
  // With the ADM march kernel (memory-bound at scales 0 / 1) that is worth +2 ... +4 % at 2160p (profiles/r04h_batch_sweep.txt,
  // r04j_prio.txt) -- but a kernel's launch then lasts as long as its share of a crowded device allows (VIF scale 0: 1.23 ms
  // instead of 0.76), so the per-kernel figures stop describing the kernels; stream priorities changed nothing.  Off by default.
  const char* e = getenv("PQA_MULTI_STREAM");
  c->multi_stream = (e && e[0] == '1') ? 1 : (e && e[0] == '2') ? 2 : 0;
  const char* t = getenv("PQA_TRACE");
  c->trace = t && t[0] == '1';
  const char* v = getenv("PQA_VIF_MFMA");   // 0: VALU kernels only (the march kernel's test partner); default: march kernel
  c->vif_s0_mode = (v && v[0] == '0') ? VIF_S0_VALU : VIF_S0_AUTO;
  const char* vu = getenv("PQA_VIF_UNIFORM");   // 0: every wave takes the general VIF statistic (test partner of the all-high fast path)
  c->vif_uniform = !(vu && vu[0] == '0');
  // PQA_VIF_STRIP: 0 = vif_stat_kernel at every scale (the strip kernel's test partner); a number = the scales that may run
  // the strip kernel as a bit mask (2: scale 1, 6: scales 1 and 2, 14: scales 1-3; per-scale A/B runs and the tests); default:
  // scale 1, the one scale at which the strip kernel measured faster.
  // PQA_VIF_STRIP_SEG=n: segments of n tile rows whatever the launch size (small test frames cross segment boundaries).
  const char* vs = getenv("PQA_VIF_STRIP");
  if (vs && vs[0]) c->vif_strip_mask = atoi(vs) & 0xe;
  const char* vg = getenv("PQA_VIF_STRIP_SEG");
  c->vif_strip_seg = vg ? std::max(0, atoi(vg)) : 0;
  const char* am = getenv("PQA_ADM_MARCH");  // 0: the LDS-tiled ADM kernel (A/B partner of the march kernel)
  const char* ap = getenv("PQA_ADM_PYRAMID");  // 0: the march kernel one scale per launch (test partner of the pyramid kernel)
  c->adm_mode = (am && am[0] == '0') ? ADM_TILED : (ap && ap[0] == '0') ? ADM_MARCH : ADM_AUTO;
  const char* ac = getenv("PQA_ADM_CONE");  // 0: the march kernels compute the whole approximation band (test partner of the cone, adm_need.h)
  c->adm_cone = !(ac && ac[0] == '0');
  const char* mm = getenv("PQA_MOTION_MARCH");  // 0: the LDS-tiled motion kernel (test partner of the march kernel)
  c->motion_mode = (mm && mm[0] == '0') ? MOTION_TILED : MOTION_AUTO;
  const char* xm = getenv("PQA_XSSE_MFMA");  // 0: the plain-VALU cross-SSE kernel for 8-bit clips too (test partner of the MFMA kernel)
  c->xsse_mfma = !(xm && xm[0] == '0');
  const char* tw = getenv("PQA_TEMPORAL_WALK");  // 1: a workgroup of the temporal moments walks through time (A/B partner of a workgroup per transition)
  c->temporal_walk = tw && tw[0] == '1';
  const char* du = getenv("PQA_DEINT_UNIFORM");  // 0: every wave of the deinterlacer takes the general path (test partner of the still-picture fast path)
  c->deint_uniform = !(du && du[0] == '0');
}

// The context's own streams and the events of a batch.
int create_streams(pqa_ctx* c) {
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
  c->stream = c->own_stream;
  for (int i = 0; i < 2; ++i) {
    HIPCHK(c, hipStreamCreateWithFlags(&c->aux[i], hipStreamNonBlocking));
    HIPCHK(c, hipEventCreateWithFlags(&c->join_ev[i], hipEventDisableTiming));
  }
  HIPCHK(c, hipEventCreateWithFlags(&c->fork_ev, hipEventDisableTiming));
  for (int i = 0; i < kBatchEvents; ++i) HIPCHK(c, hipEventCreateWithFlags(&c->batch_ev[i], hipEventDisableTiming));
  return PQA_OK;
}

// ---- what the submit and history entries share ------------------------------------------------
// The rules of a run of n_frames that need no device call: a cancelled context takes none (pqa_submit_fd_run: submit_run says so
// itself, after this), and the records of one call must not overwrite each other.
int run_admit(pqa_ctx* c, int n_frames, bool check_cancel = true) {
  if (check_cancel && c->cancelled.load()) return fail(c, PQA_ECANCELLED, "cancelled");
  if (n_frames > c->capacity)
    return fail(c, PQA_ESTATE, "%d frames in one call exceed result_capacity %d (records would overwrite each other)",
                n_frames, c->capacity);
  return PQA_OK;
}

// ... and what follows an entry's own argument rules: the pending host frames go first, and the slots of the WHOLE run must
// be free before anything is copied, unpacked or launched.
int run_begin(pqa_ctx* c, int64_t first_index, int n_frames) {
  HIPCHK(c, hipSetDevice(c->device));
  PQACHK(flush_pending(c));
  return check_slots_free(c, first_index, n_frames);
}

// What a launch of a run scores: the two clips and the reference luma in front of them (null: none, or what the chains hold).
struct LaunchInput {
  pqa_device_clip ref{}, dis{};
  const void* prev = nullptr;
  int64_t prev_pitch = 0;   // bytes
};

// n_frames device-resident frames from first_index on in equal launches (host::launch_size; records do not depend on how a
// run is cut): input(done, n, &in) fills in frames done ... done + n - 1 of the run, queueing whatever brings them there.
template <class Input>
int launch_run(pqa_ctx* c, int64_t first_index, int n_frames, Input input) {
  const int per = host::launch_size(n_frames, c->B);
  for (int done = 0; done < n_frames;) {
    if (c->cancelled.load()) return fail(c, PQA_ECANCELLED, "cancelled");
    const int n = n_frames - done < per ? n_frames - done : per;
    LaunchInput in;
    PQACHK(input(done, n, &in));
    PQACHK(process_batch(c, first_index + done, n, &in.ref, &in.dis, in.prev, in.prev_pitch));
    done += n;
  }
  return PQA_OK;
}

pqa_device_clip clip_from(const pqa_device_clip& clip, int n_planes, int64_t f) {   // the clip from frame f on
  pqa_device_clip d = clip;
  for (int p = 0; p < n_planes; ++p) d.plane[p] = (const uint8_t*)clip.plane[p] + f * clip.frame_pitch[p];
  return d;
}

// What the history-arming entries share: the pending host frames go first; then `restart` when there is nothing to arm (a chain
// start), else `arm` on an idle stream.
template <class Restart, class Arm>
int arm_histories(pqa_ctx* c, bool have, Restart restart, Arm arm) {
  HIPCHK(c, hipSetDevice(c->device));
  PQACHK(flush_pending(c));
  if (!have) {
    restart();
    return PQA_OK;
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return arm();
}

}  // namespace

// ================================================================================================
extern "C" {

const char* pqa_version(void) { return "pqa_vmaf 0.2.0 (gfx950; libvmaf-float VIF/ADM/motion, FFmpeg psnr/ssim; VIF scale 0 on the f16 matrix cores)"; }
int pqa_record_doubles(void) { return PQA_RECORD_DOUBLES; }
int pqa_ext_doubles(void) { return PQA_EXT_DOUBLES; }
int pqa_ext2_doubles(void) { return PQA_EXT2_DOUBLES; }
int pqa_ext3_doubles(void) { return PQA_EXT3_DOUBLES; }
int pqa_ext4_doubles(void) { return PQA_EXT4_DOUBLES; }
int pqa_ext5_doubles(void) { return PQA_EXT5_DOUBLES; }

void pqa_config_init(pqa_config* cfg, uint32_t width, uint32_t height) {
  if (!cfg) return;
  memset(cfg, 0, sizeof *cfg);
  cfg->struct_size = sizeof *cfg;
  cfg->width = width; cfg->height = height;
  cfg->bit_depth = 8;
  cfg->n_planes = 1;
  cfg->chroma_hshift = cfg->chroma_vshift = 1;
  cfg->features = PQA_FEAT_VMAF;
  cfg->max_batch = 0;  // auto
  cfg->result_capacity = 16384;
  cfg->n_subsample = 1;
  cfg->vif_enhn_gain_limit = 100.0;
  cfg->adm_enhn_gain_limit = 100.0;
}

int pqa_create(const pqa_config* cfg, pqa_ctx** out) {
  if (!cfg || !out) return fail(nullptr, PQA_EINVAL, "null argument");
  *out = nullptr;
  PQACHK(check_config(cfg));
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(nullptr, PQA_EDEVICE, "no HIP device visible (this library has no CPU fallback)");
  if (cfg->device < 0 || cfg->device >= ndev) return fail(nullptr, PQA_EINVAL, "device %d out of range (%d)", cfg->device, ndev);

  pqa_ctx* c = new (std::nothrow) pqa_ctx();
  if (!c) return fail(nullptr, PQA_ENOMEM, "out of host memory");
  c->cfg = *cfg;
  c->device = cfg->device;
  if (cfg->max_batch) {
    c->B = (int)cfg->max_batch;
  } else {  // auto: about 1.5 GiB of luma per launch (2160p -> 97, 1080p -> 256): every launch pays a ramp and a tail, and the
            // deep scales are rounds of few, long-lived waves -- 32 -> 96 frames per launch measured +3 % at 2160p
            // (profiles/r06h_batch.txt); the workspace that goes with it is 43.5 MB per 2160p frame, 4.2 GB of the 288
    const int64_t per_frame = 2ll * cfg->width * cfg->height * (cfg->bit_depth > 8 ? 2 : 1);
    c->B = (int)((1536ll << 20) / per_frame);
    if (c->B < 8) c->B = 8;
  }
  if (c->B > 256) c->B = 256;
  c->HB = c->B < 8 ? c->B : 8;  // the host path is PCIe-bound: small pinned halves, same kernels
  c->capacity = cfg->result_capacity ? (int)cfg->result_capacity : 16384;
  if (c->capacity < c->B) c->capacity = c->B;
  c->k_sub = cfg->n_subsample > 1 ? (int)cfg->n_subsample : 1;
  if (c->cfg.vif_enhn_gain_limit <= 0) c->cfg.vif_enhn_gain_limit = 100.0;
  if (c->cfg.adm_enhn_gain_limit <= 0) c->cfg.adm_enhn_gain_limit = 100.0;
  c->elem = cfg->bit_depth > 8 ? ELEM_U16 : ELEM_U8;
  c->esize = cfg->bit_depth > 8 ? 2 : 1;
  c->inv_scale = 1.0f / (float)(1 << (cfg->bit_depth - 8));
  c->n_planes = (int)cfg->n_planes;
  c->pw[0] = (int)cfg->width; c->ph[0] = (int)cfg->height;
  for (int p = 1; p < 3; ++p) {
    c->pw[p] = (int)((cfg->width + (1u << cfg->chroma_hshift) - 1) >> cfg->chroma_hshift);
    c->ph[p] = (int)((cfg->height + (1u << cfg->chroma_vshift) - 1) >> cfg->chroma_vshift);
  }
  c->slot = slot_layout(c);
  c->vif_fixed = (cfg->features & PQA_FEAT_VIF) && (cfg->fixed_point & PQA_FIXED_VIF);
  c->motion_fixed = (cfg->features & PQA_FEAT_MOTION) && (cfg->fixed_point & PQA_FIXED_MOTION);
  c->adm_fixed = (cfg->features & PQA_FEAT_ADM) && (cfg->fixed_point & PQA_FIXED_ADM);
  // blackdetect's default pixel_black_th = 0.10 on a limited-range clip: 37 / 151 / 606
  const double f = (double)(1 << (cfg->bit_depth - 8));
  c->black_thr = (uint32_t)(16.0 * f + 0.10 * 219.0 * f);
  read_switches(c);
  // each part for the contexts with one of its feature bits (0: all); the streams first, alloc_rings last: it waits for the fills
  static const struct { uint32_t features; int (*make)(pqa_ctx*); } kParts[] = {
      {0, create_streams}, {0, alloc_vif}, {0, alloc_adm}, {0, alloc_motion}, {0, alloc_psnr_ssim},
      {PQA_FEAT_FLOAT_SSIM | PQA_FEAT_MS_SSIM, alloc_ssim_family}, {PQA_FEAT_CIEDE, alloc_ciede}, {PQA_FEAT_CAMBI, alloc_cambi},
      {PQA_FEAT_PSNR_HVS, alloc_psnr_hvs}, {PQA_FEAT_XPSNR, alloc_xpsnr}, {PQA_FEAT_SITI, alloc_siti},
      {PQA_FEAT_INTEGRITY, alloc_integrity}, {0, alloc_rings}};
  for (const auto& part : kParts) {
    if (part.features && !(cfg->features & part.features)) continue;
    if (const int rc = part.make(c); rc != PQA_OK) {
      g_create_error = c->err;
      pqa_destroy(c);
      return rc;
    }
  }
  *out = c;
  return PQA_OK;
}

void pqa_destroy(pqa_ctx* c) {
  if (!c) return;
  if (c->pin_thread.joinable()) c->pin_thread.join();
  hipSetDevice(c->device);
  if (c->stream) hipStreamSynchronize(c->stream);
  if (c->copy_stream) hipStreamSynchronize(c->copy_stream);
  for (int i = 0; i < 2; ++i) if (c->aux[i]) hipStreamSynchronize(c->aux[i]);
  prof_drain(c);
  for (void* p : c->allocs) hipFree(p);
  // park the fixed halves for the next context (everything using them has been synchronised above) ...
  if (c->staging_ready && staging_cache_enabled() && c->half[0].pinned && c->half[0].dev && c->half[1].pinned && c->half[1].dev) {
    std::lock_guard<std::mutex> g(g_staging_mu);
    if (g_staging.bytes) {           // one set per process: the older one goes
      if (g_staging.device != c->device) hipSetDevice(g_staging.device);
      staging_release(g_staging);
      hipSetDevice(c->device);
    }
    g_staging.device = c->device;
    g_staging.bytes = c->slot_bytes() * (size_t)c->HB;
    for (int i = 0; i < 2; ++i) {
      g_staging.pinned[i] = c->half[i].pinned;
      g_staging.dev[i] = c->half[i].dev;
      c->half[i].pinned = c->half[i].dev = nullptr;
    }
  }
  for (Half* H : all_halves(c)) {   // ... and release what every half still holds
    half_free(*H);
    if (H->copied) hipEventDestroy(H->copied);
    if (H->computed) hipEventDestroy(H->computed);
  }
  for (void* b : c->side_buf)
    if (b) hipFree(b);
  for (uint8_t* b : c->side_pin)
    if (b) hipHostFree(b);
  for (hipEvent_t e : c->side_pin_sent)
    if (e) hipEventDestroy(e);
  if (c->copy_stream) hipStreamDestroy(c->copy_stream);
  for (int i = 0; i < 2; ++i) {
    if (c->aux[i]) hipStreamDestroy(c->aux[i]);
    if (c->join_ev[i]) hipEventDestroy(c->join_ev[i]);
  }
  if (c->fork_ev) hipEventDestroy(c->fork_ev);
  for (int i = 0; i < kBatchEvents; ++i) if (c->batch_ev[i]) hipEventDestroy(c->batch_ev[i]);
  if (c->own_stream) hipStreamDestroy(c->own_stream);
  delete c;
}

int pqa_set_stream(pqa_ctx* c, void* hip_stream) {
  if (!c) return PQA_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->done_seq = c->batch_seq;
  c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
  return PQA_OK;
}

int pqa_submit_device(pqa_ctx* c, int64_t first_index, int32_t n_frames, const pqa_device_clip* ref,
                      const pqa_device_clip* dis, const void* prev_ref_luma, int64_t prev_row_pitch) {
  if (!c) return PQA_EINVAL;
  if (!ref || !dis || n_frames < 0 || first_index < 0) return fail(c, PQA_EINVAL, "bad argument");
  PQACHK(run_admit(c, n_frames));
  PQACHK(run_begin(c, first_index, n_frames));
  return launch_run(c, first_index, n_frames, [&](int done, int, LaunchInput* in) -> int {
    in->ref = clip_from(*ref, c->n_planes, done);
    in->dis = clip_from(*dis, c->n_planes, done);
    // the halo: the caller's in front of the run, the reference frame before the launch inside it
    in->prev = done == 0 ? prev_ref_luma : (const uint8_t*)ref->plane[0] + (int64_t)(done - 1) * ref->frame_pitch[0];
    in->prev_pitch = done == 0 ? prev_row_pitch : ref->row_pitch[0];
    return PQA_OK;
  });
}

namespace {
// does a surface / packed format fit a context of bpc bits?
bool surface_fits(uint32_t format, int bpc) {
  if (host::packed_format(format)) return host::packed_bit_depth(format) == bpc;
  return format == (bpc <= 8 ? (uint32_t)PQA_SURFACE_NV12 : (uint32_t)PQA_SURFACE_P01X);
}

// the rules of a packed clip's rows (`who`: "surface", "reference clip"); no device call
int check_packed_rows(pqa_ctx* c, const char* who, uint32_t format, const void* base, int64_t row_pitch, int64_t frame_pitch) {
  const int64_t min_row = host::packed_min_row_bytes(format, c->pw[0]);
  if (row_pitch < min_row)
    return fail(c, PQA_EINVAL, "%s: packed row pitch %lld is smaller than a row of %lld bytes", who, (long long)row_pitch, (long long)min_row);
  if (format == PQA_SURFACE_V210 && (((uintptr_t)base | (uintptr_t)row_pitch | (uintptr_t)frame_pitch) & 3))
    return fail(c, PQA_EINVAL, "%s: v210 base and pitches must be multiples of 4", who);
  return PQA_OK;
}

// n packed frames -> the planes of side sd of the surf_dev slots (luma only in a luma-only context)
hipError_t unpack_to_slots(pqa_ctx* c, int sd, uint32_t format, const void* src, int64_t row_pitch, int64_t frame_pitch, int n,
                           pqa_device_clip* out) {
  *out = slot_clip(c, c->surf_dev, sd);
  void* dst[3] = {nullptr, nullptr, nullptr};
  for (int p = 0; p < c->n_planes; ++p) dst[p] = (void*)out->plane[p];
  return launch_unpack(c->stream, (int)format, src, row_pitch, frame_pitch, dst, out->row_pitch, out->frame_pitch, c->pw[0], c->ph[0], n);
}

int ensure_surf_dev(pqa_ctx* c) {
  if (c->surf_dev) return PQA_OK;
  HIPCHK(c, hipMalloc((void**)&c->surf_dev, c->slot_bytes() * (size_t)c->B));
  c->allocs.push_back(c->surf_dev);
  return PQA_OK;
}
}  // namespace

int pqa_submit_surfaces(pqa_ctx* c, int64_t first_index, int32_t n_frames, const pqa_surface_clip* ref,
                        const pqa_surface_clip* dis, const pqa_surface_clip* prev_ref) {
  if (!c) return PQA_EINVAL;
  if (!ref || !dis || n_frames < 0 || first_index < 0) return fail(c, PQA_EINVAL, "bad argument");
  PQACHK(run_admit(c, n_frames));
  const int bpc = (int)c->cfg.bit_depth;
  const pqa_surface_clip* all[3] = {ref, dis, prev_ref};
  bool any_packed = false, any_decoder = false;
  for (int i = 0; i < 3; ++i) {
    const pqa_surface_clip* s = all[i];
    if (!s) continue;
    if (s->struct_size != sizeof(pqa_surface_clip)) return fail(c, PQA_EINVAL, "pqa_surface_clip.struct_size mismatch");
    if (!surface_fits(s->format, bpc))
      return fail(c, PQA_EINVAL,
                  "surface format %u does not fit a %d-bit context (NV12, UYVY, YUYV for 8 bit; P01X above, V210 for 10 bit)",
                  s->format, bpc);
    if (host::packed_format(s->format)) {
      if (!s->luma) return fail(c, PQA_EINVAL, "surface luma pointer / pitch");
      const int rc = check_packed_rows(c, "surface", s->format, s->luma, s->luma_row_pitch, s->luma_frame_pitch);
      if (rc != PQA_OK) return rc;
      if (i < 2) any_packed = true;
      continue;
    }
    if (i < 2) any_decoder = true;
    if (!s->luma || s->luma_row_pitch < (int64_t)c->pw[0] * c->esize || s->luma_row_pitch % c->esize)
      return fail(c, PQA_EINVAL, "surface luma pointer / pitch");
    // an NV12 luma plane is scored where it lies: the rules of pqa_submit_device, before anything is unpacked (the halo's
    // where a feature in the mask reads it, as in process_batch)
    if (bpc <= 8 && (i < 2 || (c->cfg.features & (PQA_FEAT_MOTION | PQA_FEAT_XPSNR | PQA_FEAT_SITI)))) {
      static const char* const kWho[3] = {"reference surface luma", "distorted surface luma", "halo surface luma"};
      const int rc = check_plane_rows(c, kWho[i], 0, s->luma_row_pitch);
      if (rc != PQA_OK) return rc;
    }
    if (i < 2 && c->n_planes == 3 &&
        (!s->chroma || s->chroma_row_pitch < (int64_t)c->pw[1] * 2 * c->esize || s->chroma_row_pitch % c->esize))
      return fail(c, PQA_EINVAL, "surface chroma pointer / pitch");
  }
  if (c->n_planes == 3 && any_decoder && (c->cfg.chroma_hshift != 1 || c->cfg.chroma_vshift != 1))
    return fail(c, PQA_EINVAL, "decoder surfaces are 4:2:0: the context's chroma shifts must be 1, 1");
  if (c->n_planes == 3 && any_packed && (c->cfg.chroma_hshift != 1 || c->cfg.chroma_vshift != 0))
    return fail(c, PQA_EINVAL, "packed capture formats are 4:2:2: the context's chroma shifts must be 1, 0");
  PQACHK(run_begin(c, first_index, n_frames));
  const bool shift_luma = bpc > 8;   // of a decoder surface
  const int shift = 16 - bpc;
  // Unpacked planes go to a device buffer of B slots.  One buffer is enough: unpack and scoring run on the same stream,
  // so the next batch's unpack starts when this batch's kernels are done.
  const bool stage = shift_luma || c->n_planes == 3 || any_packed;
  if (stage) PQACHK(ensure_surf_dev(c));
  const bool prev_packed = prev_ref && host::packed_format(prev_ref->format);
  const bool prev_staged = prev_ref && (prev_packed || shift_luma);   // not usable where it lies
  // prev_ref's luma, unpacked / shifted down, into a plane of the device
  const auto stage_prev = [&](uint8_t* dst, int64_t pitch) -> hipError_t {
    if (!prev_packed)
      return launch_ingest_shift16(c->stream, prev_ref->luma, prev_ref->luma_row_pitch, 0, dst, pitch, 0, c->pw[0], c->ph[0], shift, 1);
    void* planes[3] = {dst, nullptr, nullptr};
    const int64_t rp[3] = {pitch, 0, 0}, fp[3] = {0, 0, 0};
    return launch_unpack(c->stream, (int)prev_ref->format, prev_ref->luma, prev_ref->luma_row_pitch, 0, planes, rp, fp, c->pw[0], c->ph[0], 1);
  };
  if (prev_staged && (c->cfg.features & PQA_FEAT_MOTION)) {   // the halo frame goes where a previous batch would have left it
    HIPCHK(c, stage_prev(c->mo_hist.base, c->mo_hist.pitch));
    c->mo_chain.arm(1);
  }
  // xpsnr's and siti's reference frame first-1 likewise, into a plane of its own
  const bool shift_prev = prev_staged && (c->cfg.features & (PQA_FEAT_XPSNR | PQA_FEAT_SITI));
  const int64_t shift_prev_pitch = round_up((int64_t)c->pw[0] * c->esize, 64);
  if (shift_prev) {
    if (!c->xp_prev) {
      HIPCHK(c, hipMalloc((void**)&c->xp_prev, (size_t)shift_prev_pitch * c->ph[0]));
      c->allocs.push_back(c->xp_prev);
    }
    HIPCHK(c, stage_prev(c->xp_prev, shift_prev_pitch));
  }
  const pqa_surface_clip* side[2] = {ref, dis};
  return launch_run(c, first_index, n_frames, [&](int done, int n, LaunchInput* in) -> int {
    pqa_device_clip* out[2] = {&in->ref, &in->dis};
    for (int sd = 0; sd < 2; ++sd) {
      const pqa_surface_clip* s = side[sd];
      const uint8_t* luma = (const uint8_t*)s->luma + (int64_t)done * s->luma_frame_pitch;
      if (host::packed_format(s->format)) {   // a packed clip is never scored in place
        HIPCHK(c, unpack_to_slots(c, sd, s->format, luma, s->luma_row_pitch, s->luma_frame_pitch, n, out[sd]));
        continue;
      }
      const pqa_device_clip slots = stage ? slot_clip(c, c->surf_dev, sd) : pqa_device_clip{};   // where this side's planes are staged
      *out[sd] = slots;
      if (shift_luma) {
        HIPCHK(c, launch_ingest_shift16(c->stream, luma, s->luma_row_pitch, s->luma_frame_pitch, (void*)slots.plane[0], slots.row_pitch[0],
                                        slots.frame_pitch[0], c->pw[0], c->ph[0], shift, n));
      } else {   // NV12 luma: scored in place
        out[sd]->plane[0] = luma; out[sd]->row_pitch[0] = s->luma_row_pitch; out[sd]->frame_pitch[0] = s->luma_frame_pitch;
      }
      if (c->n_planes == 3) {
        const uint8_t* uv = (const uint8_t*)s->chroma + (int64_t)done * s->chroma_frame_pitch;
        if (slots.row_pitch[1] != slots.row_pitch[2]) return fail(c, PQA_EINVAL, "internal: U and V staging pitches differ");
        HIPCHK(c, launch_ingest_deinterleave(c->stream, c->esize, uv, s->chroma_row_pitch, s->chroma_frame_pitch, (void*)slots.plane[1],
                                             (void*)slots.plane[2], slots.row_pitch[1], slots.frame_pitch[1], c->pw[1], c->ph[1],
                                             shift_luma ? shift : 0, n));
      }
    }
    // the halo of the first launch: an NV12 luma plane is usable as it is; an unpacked / shifted one was armed above, and is
    // the frame xpsnr and siti look back to
    if (done == 0 && prev_ref && !prev_staged) { in->prev = prev_ref->luma; in->prev_pitch = prev_ref->luma_row_pitch; }
    if (done == 0 && shift_prev) { in->prev = c->xp_prev; in->prev_pitch = shift_prev_pitch; }
    return PQA_OK;
  });
}

namespace {
// one side of pqa_submit_packed: the argument rules (no device call) and how a chunk of it is staged
int host_clip_check(pqa_ctx* c, const char* who, const pqa_host_clip* h, int n_frames, host::ClipLayout* L) {
  if (h->struct_size != sizeof(pqa_host_clip)) return fail(c, PQA_EINVAL, "submit_packed: %s clip: pqa_host_clip.struct_size mismatch", who);
  const bool packed = host::packed_format(h->format);
  if (!packed && h->format != PQA_SURFACE_PLANAR)
    return fail(c, PQA_EINVAL, "submit_packed: %s clip: format %u is neither planar nor a packed capture format", who, h->format);
  if (packed && host::packed_bit_depth(h->format) != (int)c->cfg.bit_depth)
    return fail(c, PQA_EINVAL, "submit_packed: %s clip: format %u does not fit a %d-bit context (UYVY, YUYV: 8 bit; V210: 10 bit)", who,
                h->format, (int)c->cfg.bit_depth);
  if (n_frames > 0 && !h->frames) return fail(c, PQA_EINVAL, "submit_packed: %s clip: null frame list", who);
  if (packed) {
    char name[48];
    snprintf(name, sizeof name, "submit_packed: %s clip", who);
    for (int f = 0; f < n_frames; ++f) {
      if (!h->frames[f]) return fail(c, PQA_EINVAL, "%s: frame %d pointer is null", name, f);
      const int rc = check_packed_rows(c, name, h->format, h->frames[f], h->strides[0], 0);
      if (rc != PQA_OK) return rc;
    }
    *L = host::packed_layout(h->format, c->pw[0], c->ph[0]);
    return PQA_OK;
  }
  for (int p = 0; p < c->n_planes; ++p)
    if (n_frames > 0 && (h->strides[p] < 0 || (size_t)h->strides[p] < c->slot.plane[p].row_bytes))
      return fail(c, PQA_EINVAL, "submit_packed: %s clip: plane %d stride smaller than a row", who, p);
  for (int64_t i = 0; i < (int64_t)n_frames * c->n_planes; ++i)
    if (!h->frames[i]) return fail(c, PQA_EINVAL, "submit_packed: %s clip: plane pointer %lld is null", who, (long long)i);
  *L = c->slot;   // planar frames are staged as the other host paths stage them
  return PQA_OK;
}

}  // namespace

int pqa_submit_packed(pqa_ctx* c, int64_t first_index, int32_t n_frames, const pqa_host_clip* ref, const pqa_host_clip* dis) {
  if (!c) return PQA_EINVAL;
  if (!ref || !dis || n_frames < 0 || first_index < 0) return fail(c, PQA_EINVAL, "bad argument");
  PQACHK(run_admit(c, n_frames));
  const pqa_host_clip* side[2] = {ref, dis};
  host::ClipLayout L[2];
  bool any_packed = false;
  for (int sd = 0; sd < 2; ++sd) {
    PQACHK(host_clip_check(c, sd ? "captured" : "reference", side[sd], n_frames, &L[sd]));
    any_packed = any_packed || host::packed_format(side[sd]->format);
  }
  if (c->n_planes == 3 && any_packed && (c->cfg.chroma_hshift != 1 || c->cfg.chroma_vshift != 0))
    return fail(c, PQA_EINVAL, "packed capture formats are 4:2:2: the context's chroma shifts must be 1, 0");
  PQACHK(run_begin(c, first_index, n_frames));
  if (n_frames == 0) return PQA_OK;
  const int chunk = n_frames < c->HB ? n_frames : c->HB;
  if (any_packed) PQACHK(ensure_surf_dev(c));
  PQACHK(ensure_copy_path(c, c->chunk_half));
  // Chunks alternate between the two halves: chunk k + 1 is packed while chunk k is uploaded, and uploaded (on the copy stream)
  // while the kernels of chunk k run (on the context's stream).
  for (int f0 = 0; f0 < n_frames; f0 += chunk) {
    if (c->cancelled.load()) return fail(c, PQA_ECANCELLED, "cancelled");
    const int m = n_frames - f0 < chunk ? n_frames - f0 : chunk;
    Half& H = c->chunk_half[c->cur_chunk_half];
    const size_t bytes[2] = {L[0].frame_bytes * (size_t)m, L[1].frame_bytes * (size_t)m};
    const size_t at[2] = {0, (size_t)round_up((int64_t)bytes[0], 256)};   // the captured chunk lies behind the reference chunk
    PQACHK(half_claim(c, H, at[1] + bytes[1]));
    // large frames are packed in ~1 MiB tasks by the pack pool of the pqa_submit path, small ones here, the captured chunk
    // under the upload of the reference chunk; memory sources cannot come up short
    size_t side_tasks[3] = {0, 0, 0};   // side sd's tasks: [side_tasks[sd], side_tasks[sd + 1])
    bool pooled = false;
    try {   // no exception may cross the C ABI
      c->pack_tasks.clear();
      for (int sd = 0; sd < 2; ++sd) {
        host::pack_clip_tasks(c->pack_tasks, H.pinned + at[sd], L[sd], side[sd]->frames, side[sd]->strides, f0, m, 1u << 20);
        side_tasks[sd + 1] = c->pack_tasks.size();
      }
      if (L[0].frame_bytes + L[1].frame_bytes >= (4u << 20)) {
        ensure_pack_pool(c);
        pooled = c->pack_pool && c->pack_pool->run(c->pack_tasks.data(), (int)c->pack_tasks.size());
      }
    } catch (...) {
      return fail(c, PQA_ENOMEM, "out of host memory while staging frame %lld", (long long)(first_index + f0));
    }
    for (int sd = 0; sd < 2; ++sd) {
      for (size_t i = side_tasks[sd]; !pooled && i < side_tasks[sd + 1]; ++i) run_pack_task(c->pack_tasks[i]);
      HIPCHK(c, hipMemcpyAsync(H.dev + at[sd], H.pinned + at[sd], bytes[sd], hipMemcpyHostToDevice, c->copy_stream));
    }
    PQACHK(half_sent(c, H));
    c->cur_chunk_half ^= 1;
    const int rc = launch_run(c, first_index + f0, m, [&](int done, int n, LaunchInput* in) -> int {
      pqa_device_clip* out[2] = {&in->ref, &in->dis};
      for (int sd = 0; sd < 2; ++sd) {
        const uint8_t* base = H.dev + at[sd] + (size_t)done * L[sd].frame_bytes;
        if (host::packed_format(side[sd]->format))
          HIPCHK(c, unpack_to_slots(c, sd, side[sd]->format, base, L[sd].plane[0].pitch, (int64_t)L[sd].frame_bytes, n, out[sd]));
        else   // planar planes are scored where they were uploaded
          *out[sd] = clip_at(base, L[sd], (int64_t)L[sd].frame_bytes);
      }
      return PQA_OK;   // no halo: the chains continue
    });
    if (rc != PQA_OK) {   // whatever was queued still reads the half
      std::string why;
      why.swap(c->err);
      half_launched(c, H);
      why.swap(c->err);
      return rc;
    }
    PQACHK(half_launched(c, H));
  }
  // the caller's buffers are free: everything was copied into the pinned chunks above
  return PQA_OK;
}

int pqa_submit(pqa_ctx* c, int64_t frame_index, const void* const ref_planes[3], const int64_t ref_strides[3],
               const void* const dis_planes[3], const int64_t dis_strides[3]) {
  if (!c) return PQA_EINVAL;
  if (!ref_planes || !dis_planes || !ref_strides || !dis_strides || frame_index < 0)
    return fail(c, PQA_EINVAL, "bad argument");
  PlaneSrc src[2][3];
  for (int p = 0; p < c->n_planes; ++p) {
    if (!ref_planes[p] || !dis_planes[p]) return fail(c, PQA_EINVAL, "plane %d pointer is null", p);
    const size_t row_bytes = (size_t)c->pw[p] * c->esize;
    if ((size_t)ref_strides[p] < row_bytes || (size_t)dis_strides[p] < row_bytes)
      return fail(c, PQA_EINVAL, "plane %d stride smaller than a row", p);
    src[0][p] = PlaneSrc{(const uint8_t*)ref_planes[p], ref_strides[p], -1, 0};
    src[1][p] = PlaneSrc{(const uint8_t*)dis_planes[p], dis_strides[p], -1, 0};
  }
  return submit_one(c, frame_index, src);
}

int pqa_submit_fd(pqa_ctx* c, int64_t frame_index, int ref_fd, const int64_t ref_plane_offsets[3], int dis_fd,
                  const int64_t dis_plane_offsets[3]) {
  if (!c) return PQA_EINVAL;
  if (ref_fd < 0 || dis_fd < 0 || !ref_plane_offsets || !dis_plane_offsets || frame_index < 0)
    return fail(c, PQA_EINVAL, "bad argument");
  PlaneSrc src[2][3];
  for (int p = 0; p < c->n_planes; ++p) {
    if (ref_plane_offsets[p] < 0 || dis_plane_offsets[p] < 0) return fail(c, PQA_EINVAL, "plane %d file offset is negative", p);
    const int64_t row_bytes = (int64_t)c->pw[p] * c->esize;   // planes lie packed in the file: rows row_bytes apart
    src[0][p] = PlaneSrc{nullptr, row_bytes, ref_fd, ref_plane_offsets[p]};
    src[1][p] = PlaneSrc{nullptr, row_bytes, dis_fd, dis_plane_offsets[p]};
  }
  return submit_one(c, frame_index, src);
}

int pqa_submit_fd_run(pqa_ctx* c, int64_t first_index, int32_t n_frames, int ref_fd, const int64_t ref_plane_offsets[3],
                      int64_t ref_frame_stride, int dis_fd, const int64_t dis_plane_offsets[3], int64_t dis_frame_stride) {
  if (!c) return PQA_EINVAL;
  if (ref_fd < 0 || dis_fd < 0 || !ref_plane_offsets || !dis_plane_offsets || first_index < 0 || n_frames < 0 ||
      ref_frame_stride < 0 || dis_frame_stride < 0)
    return fail(c, PQA_EINVAL, "bad argument");
  PQACHK(run_admit(c, n_frames, false));   // the length of the run first; submit_run refuses a cancelled context
  PlaneSrc src[2][3];
  for (int p = 0; p < c->n_planes; ++p) {
    if (ref_plane_offsets[p] < 0 || dis_plane_offsets[p] < 0) return fail(c, PQA_EINVAL, "plane %d file offset is negative", p);
    const int64_t row_bytes = (int64_t)c->pw[p] * c->esize;   // planes lie packed in the file: rows row_bytes apart
    src[0][p] = PlaneSrc{nullptr, row_bytes, ref_fd, ref_plane_offsets[p]};
    src[1][p] = PlaneSrc{nullptr, row_bytes, dis_fd, dis_plane_offsets[p]};
  }
  const int64_t step[2] = {ref_frame_stride, dis_frame_stride};
  return submit_run(c, first_index, n_frames, src, step);
}

namespace {
// pqa_set_motion_halo / pqa_set_ref_history: motion's halo from prev[0], xpsnr's history from prev[0..n_prev)
int set_history(pqa_ctx* c, const void* const* prev, int n_prev, int64_t row_stride) {
  const bool mot = c->cfg.features & PQA_FEAT_MOTION, xp = c->cfg.features & PQA_FEAT_XPSNR;
  const bool si = c->cfg.features & PQA_FEAT_SITI;
  if (!mot && !xp && !si) return PQA_OK;
  return arm_histories(
      c, n_prev > 0,
      [&] {
        c->mo_chain.restart();
        c->xp_chain.restart();
        c->st_chain[1].restart();
      },
      [&]() -> int {
        if (mot) {
          HIPCHK(c, hist_arm(c, c->mo_hist, prev[0], row_stride, 0));
          c->mo_chain.arm(1);
        }
        if (xp) {
          for (int j = 0; j < n_prev; ++j) HIPCHK(c, hist_arm(c, c->xp_hist[j], prev[j], row_stride, 0));
          c->xp_chain.arm(n_prev);
        }
        if (si) {
          HIPCHK(c, hist_arm(c, c->st_hist[1], prev[0], row_stride, 0));
          c->st_chain[1].arm(1);
        }
        return PQA_OK;
      });
}
}  // namespace

int pqa_set_motion_halo(pqa_ctx* c, const void* prev_ref_luma_host, int64_t row_stride) {
  if (!c) return PQA_EINVAL;
  return set_history(c, &prev_ref_luma_host, prev_ref_luma_host ? 1 : 0, row_stride);
}

int pqa_set_ref_history(pqa_ctx* c, const void* const* prev_luma_host, int32_t n_prev, int64_t row_stride) {
  if (!c) return PQA_EINVAL;
  if (n_prev < 0 || n_prev > 2 || (n_prev > 0 && !prev_luma_host))
    return fail(c, PQA_EINVAL, "pqa_set_ref_history: bad argument (n_prev %d)", n_prev);
  for (int j = 0; j < n_prev; ++j)
    if (!prev_luma_host[j]) return fail(c, PQA_EINVAL, "pqa_set_ref_history: plane %d is null", j);
  if (n_prev > 0 && row_stride < (int64_t)c->pw[0] * c->esize)
    return fail(c, PQA_EINVAL, "pqa_set_ref_history: row stride %lld smaller than a row", (long long)row_stride);
  return set_history(c, prev_luma_host, n_prev, row_stride);
}

int pqa_set_dis_history(pqa_ctx* c, const void* prev_dis_luma_host, int64_t row_stride) {
  if (!c) return PQA_EINVAL;
  if (!(c->cfg.features & PQA_FEAT_SITI)) return PQA_OK;
  if (prev_dis_luma_host && row_stride < (int64_t)c->pw[0] * c->esize)
    return fail(c, PQA_EINVAL, "pqa_set_dis_history: row stride %lld smaller than a row", (long long)row_stride);
  return arm_histories(
      c, prev_dis_luma_host != nullptr, [&] { c->st_chain[0].restart(); },   // a chain start of the distorted clip
      [&]() -> int {
        HIPCHK(c, hist_arm(c, c->st_hist[0], prev_dis_luma_host, row_stride, 0));
        c->st_chain[0].arm(1);
        return PQA_OK;
      });
}

int pqa_set_dis_history_planes(pqa_ctx* c, const void* const planes[3], const int64_t strides[3]) {
  if (!c) return PQA_EINVAL;
  const bool ig = c->cfg.features & PQA_FEAT_INTEGRITY, si = c->cfg.features & PQA_FEAT_SITI;
  if (!ig && !si) return PQA_OK;
  if (planes) {
    if (!strides) return fail(c, PQA_EINVAL, "pqa_set_dis_history_planes: null strides");
    for (int p = 0; p < (ig ? c->n_planes : 1); ++p) {
      if (!planes[p]) return fail(c, PQA_EINVAL, "pqa_set_dis_history_planes: plane %d is null", p);
      if (strides[p] < (int64_t)c->pw[p] * c->esize)
        return fail(c, PQA_EINVAL, "pqa_set_dis_history_planes: plane %d stride %lld smaller than a row", p, (long long)strides[p]);
    }
  }
  if (si) PQACHK(pqa_set_dis_history(c, planes ? planes[0] : nullptr, planes ? strides[0] : 0));   // what it arms
  if (!ig) return PQA_OK;
  return arm_histories(
      c, planes != nullptr, [&] { c->ig_chain.restart(); },
      [&]() -> int {
        for (int p = 0; p < c->n_planes; ++p) HIPCHK(c, hist_arm(c, c->ig_hist[p], planes[p], strides[p], p));
        c->ig_chain.arm(1);
        return PQA_OK;
      });
}

int pqa_set_black_threshold(pqa_ctx* c, uint32_t threshold) {
  if (!c) return PQA_EINVAL;
  if (threshold >= (1u << c->cfg.bit_depth))
    return fail(c, PQA_EINVAL, "black threshold %u above the largest %u-bit sample", threshold, c->cfg.bit_depth);
  if (c->started || c->pending > 0)
    return fail(c, PQA_ESTATE, "pqa_set_black_threshold: legal before the first submit and after pqa_reset only");
  c->black_thr = threshold;
  return PQA_OK;
}

int pqa_flush(pqa_ctx* c) {
  if (!c) return PQA_EINVAL;
  if (c->cancelled.load()) return fail(c, PQA_ECANCELLED, "cancelled");
  HIPCHK(c, hipSetDevice(c->device));
  return flush_pending(c);
}

int pqa_sync(pqa_ctx* c) {
  if (!c) return PQA_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  int rc = c->cancelled.load() ? PQA_OK : flush_pending(c);
  if (rc != PQA_OK) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->done_seq = c->batch_seq;
  prof_drain(c);
  if (c->cancelled.load()) return fail(c, PQA_ECANCELLED, "cancelled");
  return PQA_OK;
}

int pqa_collect(pqa_ctx* c, int64_t first_index, int32_t count, double* records) {
  return pqa_collect_ext5(c, first_index, count, records, nullptr, nullptr, nullptr, nullptr, nullptr);
}

int pqa_collect_ext(pqa_ctx* c, int64_t first_index, int32_t count, double* records, double* ext) {
  return pqa_collect_ext5(c, first_index, count, records, ext, nullptr, nullptr, nullptr, nullptr);
}

int pqa_collect_ext2(pqa_ctx* c, int64_t first_index, int32_t count, double* records, double* ext, double* ext2) {
  return pqa_collect_ext5(c, first_index, count, records, ext, ext2, nullptr, nullptr, nullptr);
}

int pqa_collect_ext3(pqa_ctx* c, int64_t first_index, int32_t count, double* records, double* ext, double* ext2,
                     double* ext3) {
  return pqa_collect_ext5(c, first_index, count, records, ext, ext2, ext3, nullptr, nullptr);
}

int pqa_collect_ext4(pqa_ctx* c, int64_t first_index, int32_t count, double* records, double* ext, double* ext2,
                     double* ext3, double* ext4) {
  return pqa_collect_ext5(c, first_index, count, records, ext, ext2, ext3, ext4, nullptr);
}

int pqa_collect_ext5(pqa_ctx* c, int64_t first_index, int32_t count, double* records, double* ext, double* ext2,
                     double* ext3, double* ext4, double* ext5) {
  if (!c) return PQA_EINVAL;
  if (count < 0 || first_index < 0 || (count > 0 && !records)) return fail(c, PQA_EINVAL, "bad argument");
  if (count > c->capacity) return fail(c, PQA_ESTATE, "count %d exceeds result_capacity %d", count, c->capacity);
  if (c->cancelled.load()) return fail(c, PQA_ECANCELLED, "cancelled");
  HIPCHK(c, hipSetDevice(c->device));
  int rc = flush_pending(c);  // a partial host batch holding requested frames has to be launched first
  if (rc != PQA_OK) return rc;
  // every requested frame must be the one its ring slot holds (never submitted / overwritten -> PQA_ESTATE);
  // then wait for the youngest batch among them only -- later batches keep running under the host's work
  uint64_t need = 0;
  {
    int64_t bad = 0, holder = 0;
    bool never = false;
    if (!c->ring.collectable(first_index, count, &need, &bad, &never, &holder)) {
      if (never) return fail(c, PQA_ESTATE, "frame %lld was never submitted", (long long)bad);
      return fail(c, PQA_ESTATE, "frame %lld was never submitted, or its record was overwritten by frame %lld",
                  (long long)bad, (long long)holder);
    }
  }
  rc = wait_batch(c, need);
  if (rc != PQA_OK) return rc;
  if (c->cancelled.load()) return fail(c, PQA_ECANCELLED, "cancelled");
  const size_t rec_bytes = PQA_RECORD_DOUBLES * sizeof(double);
  double* const outs[kExtBlocks] = {ext, ext2, ext3, ext4, ext5};
  int64_t row = first_index % c->capacity;
  int done = 0;
  while (done < count) {
    const int n = (int)((c->capacity - row) < (count - done) ? (c->capacity - row) : (count - done));
    HIPCHK(c, hipMemcpy(records + (size_t)done * PQA_RECORD_DOUBLES, c->records + (size_t)row * PQA_RECORD_DOUBLES,
                        n * rec_bytes, hipMemcpyDeviceToHost));
    if (c->adm_fixed) {
      // integer_adm.c's scalar epilogue (six cube roots per scale) on the host, with the libm libvmaf would use:
      // the integer accumulators are exact, so are the resulting adm num / den
      std::vector<long long> acc;
      try {
        acc.resize((size_t)n * 24);
      } catch (...) {
        return fail(c, PQA_ENOMEM, "out of host memory");
      }
      HIPCHK(c, hipMemcpy(acc.data(), c->adm_fx_acc + (size_t)row * 24, acc.size() * sizeof(long long),
                          hipMemcpyDeviceToHost));
      for (int f = 0; f < n; ++f)
        for (int s = 0; s < 4; ++s) {
          double* rec = records + (size_t)(done + f) * PQA_RECORD_DOUBLES;
          adm_fixed_epilogue(c->adm_fx[s], &acc[(size_t)f * 24 + s * 6], &rec[PQA_REC_ADM_NUM + s], &rec[PQA_REC_ADM_DEN + s]);
        }
    }
    for (int i = 0; i < kExtBlocks; ++i) {   // an extension ring has the record ring's slots
      if (!outs[i]) continue;
      const size_t doubles = kExtBlock[i].doubles;
      double* dst = outs[i] + (size_t)done * doubles;
      if (c->ext[i])
        HIPCHK(c, hipMemcpy(dst, c->ext[i] + (size_t)row * doubles, (size_t)n * doubles * sizeof(double), hipMemcpyDeviceToHost));
      else   // a context without the features of this block: nothing it runs has a slot there
        std::fill(dst, dst + (size_t)n * doubles, __builtin_nan(""));
    }
    done += n;
    row = 0;
  }
  c->ring.mark_collected(first_index, count);
  return PQA_OK;
}

int pqa_cancel(pqa_ctx* c) {
  if (!c) return PQA_EINVAL;
  c->cancelled.store(1);
  return PQA_OK;
}

int pqa_reset(pqa_ctx* c) {
  if (!c) return PQA_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->copy_stream) HIPCHK(c, hipStreamSynchronize(c->copy_stream));
  for (Half* H : all_halves(c)) H->copied_pending = H->computed_pending = false;   // both streams are idle
  c->cancelled.store(0);
  c->done_seq = c->batch_seq;
  c->ring.reset();
  c->pending = 0;
  for (const History& h : histories(c)) h.chain->restart();
  c->started = false;
  c->err.clear();
  return PQA_OK;
}

const char* pqa_last_error(const pqa_ctx* c) { return c ? c->err.c_str() : g_create_error.c_str(); }

int pqa_profile_enable(pqa_ctx* c, int on) {
  if (!c) return PQA_EINVAL;
  prof_drain(c);
  c->prof = on != 0;
  c->prof_mask = (on == 1 || on == 0) ? 0xffffffffu : (uint32_t)on >> 1;  // on = 1: all; on = (mask << 1): subset
  if (on) {
    memset(c->prof_ms, 0, sizeof c->prof_ms);
    memset(c->prof_n, 0, sizeof c->prof_n);
    memset(c->prof_frames, 0, sizeof c->prof_frames);
  }
  return PQA_OK;
}

int pqa_profile_read(pqa_ctx* c, int kernel_id, double* total_ms, uint64_t* launches, uint64_t* frames) {
  if (!c || kernel_id < 0 || kernel_id >= PQA_PROF_KERNELS) return PQA_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  prof_drain(c);
  if (total_ms) *total_ms = c->prof_ms[kernel_id];
  if (launches) *launches = c->prof_n[kernel_id];
  if (frames) *frames = c->prof_frames[kernel_id];
  return PQA_OK;
}

const char* pqa_profile_kernel_name(int kernel_id) {
  return (kernel_id >= 0 && kernel_id < PQA_PROF_KERNELS) ? kProfNames[kernel_id] : "";
}

}  // extern "C"
