// The context behind the C ABI and what its three host units share: pqa_api.hip (context lifetime, the submit paths, collect,
// profiling), pqa_side.hip (the one-shot analyses that leave the scoring chain alone) and pqa_debug.hip (the pqa_debug_*
// entries).  Private to the library: callers see include/pqa_vmaf.h only.  What needs no device lives in headers of its own:
// host_pack.h, host_ring.h, host_stage.h, host_chain.h (these four tests/host_harness.cpp drives on the CPU) and host_packed.h.
#pragma once
#include "../../include/pqa_vmaf.h"

#include <atomic>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "host_chain.h"
#include "host_pack.h"
#include "host_ring.h"
#include "host_packed.h"
#include "host_stage.h"
#include "kernels.h"

namespace pqa {

struct Level {
  int w = 0, h = 0;
  int64_t pitch = 0, frame_pitch = 0;  // elements (float)
  float* ref = nullptr;
  float* dis = nullptr;
};

// A plane a feature keeps on the device in front of the next batch; which frame it holds: the host::FrameChain beside it.
struct HistPlane {
  uint8_t* base = nullptr;
  int64_t pitch = 0;  // bytes
};

// One half of a double-buffered host staging path: a pinned buffer and its device copy, of `cap` bytes each, filled in turn
// with the other half.  Uploads run on pqa_ctx::copy_stream, kernels on pqa_ctx::stream; three steps keep the two apart
// (half_claim, half_sent, half_launched in pqa_api.hip).  copied: the upload out of `pinned` is through -- the host may pack it
// again and the kernels may read `dev`; computed: the kernels that read `dev` are through -- the next upload may overwrite it.
struct Half {
  uint8_t* pinned = nullptr;
  uint8_t* dev = nullptr;
  size_t cap = 0;
  hipEvent_t copied = nullptr, computed = nullptr;
  bool copied_pending = false, computed_pending = false;
};

struct ProfEv {
  hipEvent_t a, b;
  int id, frames;
};

constexpr int kBatchEvents = 64;  // ring of per-batch completion events

// The extension record blocks: rings of [capacity][doubles] beside the record ring, pqa_ctx::ext below.  A block exists in a
// context whose feature mask has one of its bits (pqa_create allocates and NaN-fills it; collecting hands out NaN rows
// for the others).  `spatial`: written on the frames that get spatial features only, so with n_subsample > 1 a batch fills
// its rows with NaN first (fill_ext_nan).  A new block is one row here and one in _native.EXT_BLOCKS.
struct ExtBlock { int doubles; uint32_t features; bool spatial; };
enum { BLK_MAIN = 0, BLK_PSNR_HVS, BLK_XPSNR, BLK_SITI, BLK_INTEGRITY, kExtBlocks };   // in the order the collect entry points take them
constexpr ExtBlock kExtBlock[kExtBlocks] = {
    {PQA_EXT_DOUBLES, PQA_FEAT_FLOAT_SSIM | PQA_FEAT_MS_SSIM | PQA_FEAT_CIEDE | PQA_FEAT_CAMBI, true},   // ssim_family, ciede, cambi
    {PQA_EXT2_DOUBLES, PQA_FEAT_PSNR_HVS, true},     // psnr_hvs.hip
    {PQA_EXT3_DOUBLES, PQA_FEAT_XPSNR, false},       // xpsnr.hip
    {PQA_EXT4_DOUBLES, PQA_FEAT_SITI, false},        // siti.hip
    {PQA_EXT5_DOUBLES, PQA_FEAT_INTEGRITY, false},   // integrity.hip
};

// The grow-only device buffers of the side analyses, pqa_ctx::side_buf below (side_reserve, pqa_side.hip).
enum SideBuf {
  // The one pair of staging buffers for host frames, of the context's size or the call's own (pair_run, transform_run): an analysis
  // uploads a chunk of reference frames into A and of captured frames into B; a transform uploads a chunk of source frames into A
  // and writes the result into B (pqa_mask_blend: blends in A, the fill planes lie in B); pqa_frame_sad copies a chunk of frames into A.  Every such entry is synchronous and
  // leaves with the stream drained, and none reads what a call before it left there, so they all share the pair.
  SIDE_STAGE_A = 0, SIDE_STAGE_B,
  SIDE_SAD_OUT,                                                                // pqa_frame_sad[_device], integrity.hip: the sums
  SIDE_LUMA_OUT,                                                               // pqa_luma_stats[_device], luma_stats.hip: the sums
  SIDE_XSSE_PART, SIDE_XSSE_NORM_REF, SIDE_XSSE_NORM_DIS, SIDE_XSSE_OUT,       // pqa_cross_sse[_device], cross_sse.hip
  SIDE_XSSE_REF, SIDE_XSSE_DIS,                                                // pqa_cross_sse: its two rings of uploaded frames
  SIDE_SHIFT_PART, SIDE_SHIFT_ROWSQ, SIDE_SHIFT_OUT,                           // pqa_shift_sse[_device], shift_sse.hip
  SIDE_LEVEL_OUT,                                                              // pqa_level_stats[_device], level_stats.hip
  SIDE_RS_TABLE0, SIDE_RS_TABLE1, SIDE_RS_TABLE2, SIDE_RS_TABLE3,              // pqa_resample[_device], resample.hip: cached tables
  SIDE_FLOW_OUT,                                                               // pqa_flow_moments[_device], flow_moments.hip: the sums
  SIDE_COLOUR_OUT,                                                             // pqa_colour_moments[_device], colour_moments.hip: the sums
  SIDE_PROF_OUT,                                                               // pqa_line_profiles[_device], line_profiles.hip: the profiles
  SIDE_TILE_OUT,                                                               // pqa_tile_moments[_device], tile_moments.hip: the sums
  SIDE_BAND_PART, SIDE_BAND_OUT,                                               // pqa_band_moments[_device], band_moments.hip: the workgroups' partial sums of a chunk, the sums
  SIDE_TEMPORAL_OUT,                                                           // pqa_temporal_moments[_device], temporal_moments.hip: the sums
  SIDE_FIELD_OUT,                                                              // pqa_field_moments[_device], field_moments.hip: the sums
  SIDE_EDGE_OUT,                                                               // pqa_edge_profiles[_device], edge_profiles.hip: the profiles
  SIDE_TABLE_LUT,                                                              // pqa_table_apply[_device], table_apply.hip: the table
  SIDE_ITP_PART, SIDE_ITP_OUT,                                                 // pqa_delta_itp[_device], delta_itp.hip: the tiles' partial sums of a chunk, the sums
  SIDE_MASK_NODES,                                                             // pqa_mask_blend[_device], mask_blend.hip: the node grid
  kSideBufs
};

// A resampling the context has the device tables of (side_buf[SIDE_RS_TABLE0 + slot]): what pqa_resample was asked for last.
constexpr int kRsCached = 4;
struct RsCached {
  bool valid = false;
  pqa_resample_spec spec{};
  ResamplePlan plan;   // `words` is emptied once it is uploaded
};

}  // namespace pqa

struct pqa_ctx {
  pqa_config cfg{};
  int device = 0;
  hipStream_t own_stream = nullptr, stream = nullptr, copy_stream = nullptr;
  hipStream_t aux[2] = {nullptr, nullptr};  // ADM and motion/PSNR/SSIM chains run beside the VIF chain
  hipEvent_t fork_ev = nullptr, join_ev[2] = {nullptr, nullptr};
  pqa::Elem elem = pqa::ELEM_U8;
  int esize = 1;
  float inv_scale = 1.0f;
  int pw[3] = {0, 0, 0}, ph[3] = {0, 0, 0};
  int n_planes = 1;
  int B = 8, HB = 8, capacity = 16384, k_sub = 1;  // B: frames per launch; HB: frames per host-staging half
  pqa::Level vif_lv[4], adm_lv[4];
  double* vif_part[4] = {};
  long long* vif_fx_part[4] = {};  // fixed-point VIF: int64 partials instead of (num, den) doubles
  uint16_t* vif_lut = nullptr;     // integer_vif.c's log2 table, entries 32768..65535
  bool vif_fixed = false, motion_fixed = false, adm_fixed = false;
  long long* adm_fx_part[4] = {};   // fixed-point ADM: per-row int64 partials
  long long* adm_fx_acc = nullptr;  // [capacity][4][6] ring of accumulators, finished on the host in pqa_collect
  int32_t* adm_div_lut = nullptr;
  pqa::AdmFxScale adm_fx[4] = {};
  unsigned long long* motion_fx_part = nullptr;
  int vif_tiles[4] = {};
  int vif_part_cap0 = 0;   // partial pairs per frame the scale-0 buffer holds (tiled kernels or the march kernel)
  double* adm_part[4] = {};
  int adm_tiles[4] = {};
  float adm_area[4] = {};
  double* motion_part = nullptr;
  int motion_tiles_n = 0;
  unsigned long long* sse_part[3] = {};
  unsigned long long* sse_part_b[3] = {};
  unsigned long long* sse_tile_part[3] = {};
  double* ssim_part[3] = {};
  int ssim_tiles_n[3] = {};
  double ssim_norm[3] = {};
  double* records = nullptr;
  double* ext[pqa::kExtBlocks] = {};   // the extension rings beside `records` (pqa::kExtBlock); null: no feature of the block is on
  // The opt-in features below allocate nothing unless one of their bits is set (the alloc_* functions of pqa_api.hip).
  // SSIM family (PQA_FEAT_FLOAT_SSIM / PQA_FEAT_MS_SSIM; ssim_family.hip)
  pqa::Level ms_lv[pqa::kMsScales];            // MS-SSIM scales 1..4: f32 planes for ssf_sb frames
  double* ms_part[pqa::kMsScales] = {};   // [ssf_sb][tiles][4] per scale
  int ms_tiles[pqa::kMsScales] = {};
  double* fs_part = nullptr;         // float_ssim: [ssf_sb][tiles][4]
  int fs_tiles = 0, fs_box = 1;
  int ssf_sb = 0;                    // frames per pass through the pyramid (bounds its memory at 2160p)
  // CIEDE2000 (PQA_FEAT_CIEDE; ciede.hip)
  double* ciede_part = nullptr;      // [B][ciede_tiles]
  int ciede_tiles_n = 0;
  // CAMBI (PQA_FEAT_CAMBI; cambi.hip)
  pqa::CambiParams cambi_prm{};
  pqa::CambiWork cambi_wk{};
  int cambi_sb = 0;                  // frames per pass (bounds the work planes at 2160p)
  // PSNR-HVS (PQA_FEAT_PSNR_HVS; psnr_hvs.hip)
  pqa::PsnrHvsGeometry phv_geo{};
  double* phv_part = nullptr;        // [B][phv_geo.tile0[3]]
  // XPSNR (PQA_FEAT_XPSNR; xpsnr.hip)
  pqa::XpsnrGeometry xp_geo{};
  unsigned long long* xp_blk = nullptr;   // [B][xp_geo.n_blk][kXpBlockVals]
  double* xp_w = nullptr;                 // [B][xp_geo.n_blk] weights
  pqa::HistPlane xp_hist[2];              // reference luma planes the chain keeps (the last two of the last batch)
  pqa::host::FrameChain xp_chain{2};      // ... and which frames they are; pqa_set_ref_history arms them
  uint8_t* xp_prev = nullptr;        // pqa_submit_surfaces: its shifted prev_ref (allocated on first use)
  // SI / TI (PQA_FEAT_SITI; siti.hip)
  double* st_part = nullptr;         // [B][2][siti_partials][4]
  pqa::HistPlane st_hist[2];              // the last luma plane of each clip's chain (0: distorted, 1: reference)
  pqa::host::FrameChain st_chain[2];      // pqa_set_dis_history / the reference history arm them
  // capture integrity (PQA_FEAT_INTEGRITY; integrity.hip)
  unsigned long long* ig_part = nullptr;      // [B][3][kIntegrityBlocks][2]
  pqa::HistPlane ig_hist[3];              // the planes of the last distorted frame of the chain
  pqa::host::FrameChain ig_chain;         // one index for the three; pqa_set_dis_history_planes arms them
  uint32_t black_thr = 0;                     // pqa_set_black_threshold
  bool started = false;                       // a batch was launched since pqa_create / pqa_reset
  // pqa_frame_sad (allocated on first use)
  uint8_t* ig_anchor[3] = {nullptr, nullptr, nullptr};  // the anchor frame's planes (pitches: those of ig_hist)
  unsigned long long* luma_part = nullptr;
  uint32_t luma_gray = PQA_GRAY_LUMA;
  bool xsse_mfma = true;             // PQA_XSSE_MFMA, read once in pqa_create (8-bit clips; deeper clips always take the VALU path)
  bool deint_uniform = true;         // PQA_DEINT_UNIFORM, read once in pqa_create: 0 = no still-picture fast path in deinterlace.hip (test partner; the same integers)
  bool temporal_walk = false;        // PQA_TEMPORAL_WALK, read once in pqa_create: 1 takes the walking form of temporal_moments.hip (A/B partner; the same integers)
  pqa::RsCached rs_cache[pqa::kRsCached];   // pqa_resample[_device]: the tables of the last few (filter, geometry, window)
  int rs_next = 0;                          // the slot the next new table replaces
  // The side analyses' two grow-only pinned chunks (side_pin_reserve, pqa_side.hip), of any frame size: all their host frames go
  // through these (but pqa_frame_sad's, which the runtime copies).  An analysis of a clip pair packs a chunk of reference frames into the first and of captured frames into the
  // second; an analysis of one clip and pqa_cross_sse pack their chunks into the two in turn; a transform packs its source chunk
  // (pqa_mask_blend: the fill planes behind it) into the first and takes the result back through the second.
  uint8_t* side_pin[2] = {nullptr, nullptr};
  size_t side_pin_cap[2] = {0, 0};
  hipEvent_t side_pin_sent[2] = {nullptr, nullptr};   // recorded behind the upload that last read a chunk; the chunk is packed again once it has passed
  bool side_pin_busy[2] = {false, false};             // such an upload may be in flight
  void* side_buf[pqa::kSideBufs] = {};    // the side analyses' grow-only device buffers (SideBuf above), allocated on first use; all host staging shares SIDE_STAGE_A / _B
  size_t side_cap[pqa::kSideBufs] = {};   // their sizes in bytes
  // motion continuity: the last reference luma of the chain; pqa_set_motion_halo / pqa_set_ref_history arm it
  pqa::HistPlane mo_hist;
  pqa::host::FrameChain mo_chain;
  // One side of a frame pair as the library lays it out itself (pinned staging, its device copy, unpacked decoder surfaces):
  // rows padded to 64 bytes, planes to 256; the distorted side lies slot.frame_bytes behind the reference side.
  pqa::host::ClipLayout slot;
  size_t slot_bytes() const { return 2 * slot.frame_bytes; }
  // host staging.  half: the fixed halves of HB slots of the pqa_submit path (frames stay pending until a half is full or
  // flushed); chunk_half: the grow-only halves of pqa_submit_packed, a chunk of reference frames as the caller has them and the
  // captured chunk behind it at a 256-byte boundary (a packed frame can be larger than a slot).  Both upload on copy_stream.
  pqa::Half half[2], chunk_half[2];
  int cur_half = 0, cur_chunk_half = 0, pending = 0;
  int64_t pending_first = 0;
  bool staging_ready = false;
  std::thread pin_thread;            // pins the second staging half while the first one fills (ensure_staging)
  hipError_t pin_err = hipSuccess;   // its result; read after joining it (staging_half_ready)
  uint8_t* surf_dev = nullptr;   // pqa_submit_surfaces, pqa_submit_packed: B slots of unpacked planes (device only, allocated on first use)
  std::unique_ptr<pqa::host::PackPool> pack_pool;
  bool pack_pool_tried = false;
  std::vector<pqa::host::PackTask> pack_tasks;
  // record-ring bookkeeping (host side): which frame a slot holds, whether it was collected, and the batch that
  // writes it.  Lets pqa_collect wait for ITS batch only and makes the PQA_ESTATE promises of the header real.
  pqa::host::RecordRing ring;             // host_ring.h
  hipEvent_t batch_ev[pqa::kBatchEvents] = {};
  uint64_t batch_ev_seq[pqa::kBatchEvents] = {};  // sequence number last recorded into each event
  uint64_t batch_seq = 0;            // batches launched so far (the next batch gets batch_seq + 1)
  uint64_t done_seq = 0;             // every batch <= done_seq is known to be complete
  std::atomic<int> cancelled{0};
  std::string err;
  std::vector<void*> allocs;
  // profiling
  int multi_stream = 0;              // 0 one stream; 1 three streams from the start of a batch; 2 three streams behind VIF scale 0
  int vif_s0_mode = pqa::VIF_S0_AUTO;   // PQA_VIF_MFMA, read once in pqa_create
  int vif_uniform = 1;                  // PQA_VIF_UNIFORM, read once in pqa_create: 0 = no all-high fast path in the VIF statistic
  int vif_strip_mask = 0x2;             // PQA_VIF_STRIP, read once in pqa_create: bit s = scale s may run the strip kernel (0 = none; default: scale 1)
  int vif_strip_seg = 0;                // PQA_VIF_STRIP_SEG, read once in pqa_create: tile rows per segment; 0 = vif_strip_shape's rule
  int adm_mode = pqa::ADM_AUTO;        // PQA_ADM_MARCH, read once in pqa_create
  bool adm_cone = true;                // PQA_ADM_CONE, read once in pqa_create: approximation bands only inside the dependency cone
  int motion_mode = pqa::MOTION_AUTO;   // PQA_MOTION_MARCH, read once in pqa_create
  bool trace = false;   // PQA_TRACE=1: synchronise after every launch and name it on stderr (localises a stall)
  bool prof = false;
  uint32_t prof_mask = 0xffffffffu;
  std::vector<pqa::ProfEv> evs;
  double prof_ms[PQA_PROF_KERNELS] = {};
  uint64_t prof_n[PQA_PROF_KERNELS] = {}, prof_frames[PQA_PROF_KERNELS] = {};
};

namespace pqa {

// sets pqa_last_error (of the context, or of the calling thread when c is null) and returns code; defined in pqa_api.hip
int fail(pqa_ctx* c, int code, const char* fmt, ...);

#define HIPCHK(c, expr)                                                                          \
  do {                                                                                           \
    hipError_t e_ = (expr);                                                                      \
    if (e_ != hipSuccess)                                                                        \
      return pqa::fail((c), e_ == hipErrorOutOfMemory ? PQA_ENOMEM : PQA_EDEVICE, "%s failed: %s", #expr, \
                  hipGetErrorString(e_));                                                        \
  } while (0)

// a call that has set the error itself: its code goes up
#define PQACHK(expr)                   \
  do {                                 \
    const int rc_ = (expr);            \
    if (rc_ != PQA_OK) return rc_;     \
  } while (0)

template <typename T>
int dev_alloc(pqa_ctx* c, T** out, size_t count) {
  void* p = nullptr;
  if (count == 0) count = 1;
  HIPCHK(c, hipMalloc(&p, count * sizeof(T)));
  c->allocs.push_back(p);
  *out = (T*)p;
  return PQA_OK;
}

}  // namespace pqa
