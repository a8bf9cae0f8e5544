// Host-side launch interface of the gfx950 feature kernels.  All pointers are device pointers,
// pitches are in ELEMENTS of the plane's sample type.  Every launcher is asynchronous on `stream`
// and allocates nothing (workspaces come from the context), so a caller may capture them in a
// hipGraph.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

struct pqa_itp_spec;   // include/pqa_vmaf.h

namespace pqa {

enum Elem : int { ELEM_U8 = 0, ELEM_U16 = 1, ELEM_F32 = 2 };

// A run of equally-shaped planes: frame f lives at base + f * frame_pitch.
struct PlaneRun {
  const void* base;
  int64_t row_pitch;    // elements
  int64_t frame_pitch;  // elements
};

struct MutPlaneRun {
  void* base;
  int64_t row_pitch;
  int64_t frame_pitch;
};

// ---- VIF ------------------------------------------------------------------------------------
// Tile geometry of the statistic kernel at a scale (filter widths 17/9/5/3).
int vif_tile_w(int scale);
constexpr int kVifTileH = 8;
inline int vif_tiles_x(int scale, int w) { return (w + vif_tile_w(scale) - 1) / vif_tile_w(scale); }
inline int vif_tiles_y(int h) { return (h + kVifTileH - 1) / kVifTileH; }

// partials: [n_frames][tiles][2] doubles (num, den), tiles = tiles_x * tiles_y.
// border101: 0 = vif_tools.c border rule (high edge repeated), 1 = integer_vif.c padding (reflect-101).
// For scale < 3 the same launch also produces the next scale's input (fused decimation): the planes are
// filtered with the next scale's kernel and even samples kept -> next_ref / next_dis, (w/2 x h/2) f32.
// *n_partials (nullable) receives the number of (num, den) pairs per frame the launch wrote: vif_tiles_x * vif_tiles_y for
// the tiled kernels, one per wave segment for the march kernel of scale 0 (vif_march.hip); the finalize stage sums that many.
// s0_mode: which kernel scale 0 runs (read once per context from PQA_VIF_MFMA in pqa_create: A/B runs and the tests that
// compare the paths): VIF_S0_AUTO = the march kernel (8-, 10- and 12-bit clips);
// VIF_S0_VALU = VALU only.
// uniform: 1 = a wave whose pixels are all inside the image and all in the log branch (sigma1_sq >= sigma_nsq) takes the
// statistic without its other branch (same bits); 0 = every wave takes the general statistic (PQA_VIF_UNIFORM=0, read in
// pqa_create: the test partner).
// strip_seg: scales 1-3 on f32 planes, the strip kernel (a workgroup marches down `segment` tile rows of one tile column; same
// tiles, same partial slots, same bits): 0 = where vif_strip_shape's rule finds the launch large enough, n > 0 = segments of
// n tile rows whatever the launch (PQA_VIF_STRIP_SEG: tests cross segment boundaries on small frames), < 0 = the tiled kernel
// (PQA_VIF_STRIP=0, the test partner; or a scale outside PQA_VIF_STRIP's mask).
enum : int { VIF_S0_VALU = 0, VIF_S0_AUTO = 1 };
hipError_t launch_vif_stat(hipStream_t stream, int scale, Elem elem, PlaneRun ref, PlaneRun dis, int n_frames,
                           int w, int h, float inv_scale, float gain_limit, int border101, double* partials,
                           MutPlaneRun next_ref, MutPlaneRun next_dis, int s0_mode = VIF_S0_AUTO, int* n_partials = nullptr,
                           int uniform = 1, int strip_seg = 0);
// {strips (tile columns), tile rows, tile rows per segment, segments per strip} of a launch of n_frames w x h planes at `scale`
// under strip_seg; segment 0 = the tiled kernel runs.  Host arithmetic only.
void vif_strip_shape(int scale, int w, int h, int n_frames, int strip_seg, int* out4);
// Scale 0 (8-, 10-, 12-bit clips: `bits`), both filter passes on the f16 matrix cores (vif_march.hip).  vif_march_prepare uploads its tap
// table once per device (pqa_create does; synchronous, idempotent; a device that does not keep f16 denormals -- probed once,
// the operand encoding leans on them -- gets no table and scale 0 stays on the VALU kernel); launch_vif_s0_march returns false when it cannot take
// the planes (no table, pitches the stores cannot take, planes of 2 GiB and more) and launch_vif_stat then falls back to the tiled kernels.
// vif_march_partials: *n_partials of a w x h frame (one pair per wave: four stripes a workgroup x segments);
// vif_march_partials_max: its upper bound (workspace sizing).
hipError_t vif_march_prepare();
int vif_march_partials(int w, int h);
int vif_march_partials_max(int w, int h);
// host: the per-lane tap-matrix fragments the march kernel reads ([fragment][lane 0..63][8 f16 bit patterns]) -- no device
// needed; returns the number of fragments, 0 when a tap does not split exactly, -(halfwords needed) when `out` is too small
int vif_march_table(uint16_t* out, int capacity_halfwords);
// {16-column stripes, 16-row blocks, blocks per segment, segments, pass-1 MFMAs per block, pass-2 MFMAs per block} of a w x h frame
void vif_march_shape(int w, int h, int* out6);
bool launch_vif_s0_march(hipStream_t stream, Elem elem, int bits, PlaneRun ref, PlaneRun dis, int n_frames, int w, int h, float gain_limit,
                         int border101, double* partials, MutPlaneRun next_ref, MutPlaneRun next_dis, int* n_partials,
                         hipError_t* err, int uniform = 1);
// Fixed-point VIF (integer_vif.c arithmetic, vif_fixed.hip): same tiling; partials are [n_frames][tiles][8] int64
// {num_log, den_log, x, x2, n_log, den_non_log, num_non_log, -}; next_ref / next_dis are u16 planes (w/2 x h/2).
// elem: scale 0 reads the caller's samples (ELEM_U8 at 8 bit, ELEM_U16 above), deeper scales ELEM_U16.
constexpr int kVifFxPartials = 8;
void vif_fixed_log2_table(uint16_t* out32768);  // host: entry i = round(log2f(32768 + i) * 2048)
hipError_t launch_vif_fixed(hipStream_t stream, int scale, int bit_depth, Elem elem, PlaneRun ref, PlaneRun dis,
                            int n_frames, int w, int h, double gain_limit, const uint16_t* log2_lut,
                            long long* partials, MutPlaneRun next_ref, MutPlaneRun next_dis);

// ---- ADM ------------------------------------------------------------------------------------
constexpr int kAdmTileW = 60, kAdmTileH = 14;  // 126 input columns (one per lane), 16 halo'd rows = 8 row pairs
inline int adm_tiles_x(int band_w) { return (band_w + kAdmTileW - 1) / kAdmTileW; }
inline int adm_tiles_y(int band_h) { return (band_h + kAdmTileH - 1) / kAdmTileH; }

// One ADM scale: db2 DWT of (w x h) planes -> decouple -> CSF -> contrast masking.
// partials: [n_frames][tiles][6] doubles (num h,v,d cube sums; den h,v,d cube sums).
// ll_ref/ll_dis receive the approximation band (ceil(w/2) x ceil(h/2)) for the next scale
// (base may be null at the last scale).
// mode (read once per context from PQA_ADM_MARCH / PQA_ADM_PYRAMID in pqa_create): ADM_AUTO = the march kernel (adm_march.hip: one partial
// sextet per wave segment), ADM_TILED = the LDS-tiled kernel (adm.hip: one per 60 x 14 tile; A/B partner, and the fallback
// for planes of 2 GiB and more).  *n_partials (nullable) receives the number of sextets per frame the launch wrote.
// cone (PQA_ADM_CONE, read once per context; the march kernels only): outside libvmaf's window the approximation band is
// computed and stored only where a deeper scale can read it (adm_need.h); false = the whole band (test partner).  The tiled
// kernel writes and reads whole bands; it never reads a band a march kernel wrote: a context's mode is one for all scales,
// and the 2 GiB fallback goes tiled from the LARGER scale down (a band too large for the march kernel is the output of a
// scale whose input was too large as well).
enum : int { ADM_TILED = 0, ADM_AUTO = 1, ADM_MARCH = 2 };   // ADM_MARCH: the march kernel, one scale per launch (no pyramid)
hipError_t launch_adm_scale(hipStream_t stream, int scale, Elem elem, PlaneRun ref, PlaneRun dis, int n_frames,
                            int w, int h, float inv_scale, float gain_limit, MutPlaneRun ll_ref,
                            MutPlaneRun ll_dis, double* partials, int mode = ADM_AUTO, int* n_partials = nullptr,
                            bool cone = true);
// The march kernel (adm_march.hip).  adm_march_partials: sextets per frame it writes for a band_w x band_h band (workspace
// sizing; a function of the geometry only).  launch_adm_march returns false when it cannot take the planes.
// n_frames = 0 (here, in launch_adm_pyramid and in launch_motion_march): *n_partials is filled and nothing is launched.
int adm_march_partials(int band_w, int band_h);
bool launch_adm_march(hipStream_t stream, int scale, Elem elem, PlaneRun ref, PlaneRun dis, int n_frames, int w, int h,
                      float inv_scale, float gain_limit, MutPlaneRun ll_ref, MutPlaneRun ll_dis, double* partials,
                      int* n_partials, bool cone, hipError_t* err);
// Scales 0 and 1 in ONE launch (adm_pyramid.hip): scale 0's approximation band stays in registers; partials0 / partials1
// receive one sextet per wave segment each (the same count, *n_partials), ll_ref / ll_dis the approximation band of SCALE 1
// (w/4 x h/4: the input of scale 2).  adm_pyramid_takes: u8 / u16 planes whose width and height are multiples of 4 and >= 128;
// launch_adm_pyramid returns false when it cannot take the planes (the caller then runs one scale per launch).
bool adm_pyramid_takes(Elem elem, int w, int h);
int adm_pyramid_partials(int w, int h);
bool launch_adm_pyramid(hipStream_t stream, Elem elem, PlaneRun ref, PlaneRun dis, int n_frames, int w, int h, float inv_scale,
                        float gain_limit, MutPlaneRun ll_ref, MutPlaneRun ll_dis, double* partials0, double* partials1,
                        int* n_partials, bool cone, hipError_t* err);
float adm_dwt_quant_step(int lambda, int theta);   // Watson model step (adm_tools.h dwt_quant_step), theta 1 = h/v, 2 = d

// Fixed-point ADM (integer_adm.c arithmetic, adm_fixed.hip).  Same tiling as launch_adm_scale; the approximation
// bands handed to the next scale are int32 planes (4-byte elements: pass them on as ELEM_F32-sized runs).
// partials: [n_frames][tiles][kAdmFxRows][6] int64 per-row sums {num h,v,d, den h,v,d} (row 0 and 15 = halo, zero).
constexpr int kAdmFxRows = kAdmTileH + 2;
struct AdmFxScale {           // per-scale constants of the fixed-point path, shared by kernel, finalize and host epilogue
  int scale, band_w, band_h;
  int left, top, right, bottom;
  float rf[3];
  uint32_t i_rf[3];
  int cm_shift_sq[3], cm_shift_sub[3], cm_shift_cub[3], cm_final_q[3];
  int den_shift_sq, den_shift_cub, den_final_q;
  int num_row_shift, den_row_shift;
};
AdmFxScale adm_fixed_scale_params(int scale, int band_w, int band_h);
void adm_fixed_div_table(int32_t* out65537);  // host: div_lookup of integer_adm.c (2^30 / i, odd-symmetric)
// host: {num_scale, den_scale} from the six integer accumulators, as adm_cm / adm_csf_den_scale finish them
void adm_fixed_epilogue(const AdmFxScale& p, const long long acc[6], double* num_out, double* den_out);
hipError_t launch_adm_fixed(hipStream_t stream, int scale, int bit_depth, Elem elem, PlaneRun ref, PlaneRun dis,
                            int n_frames, int w, int h, double gain_limit, const int32_t* div_lut,
                            MutPlaneRun ll_ref, MutPlaneRun ll_dis, long long* partials);

// ---- motion ---------------------------------------------------------------------------------
constexpr int kMotionTileW = 252, kMotionTileH = 16;
inline int motion_tiles(int w, int h) {
  return ((w + kMotionTileW - 1) / kMotionTileW) * ((h + kMotionTileH - 1) / kMotionTileH);
}
// SAD of the 5-tap-blurred reference luma of frame f against frame f-1.  Frame 0 of the run uses
// `prev0` (may be null: then its partials are zero).  partials: [n_frames][tiles] doubles.
// mode (PQA_MOTION_MARCH, read once per context): MOTION_AUTO = the march kernel (motion_march.hip: one partial per wave
// segment), MOTION_TILED = the LDS-tiled kernel (motion.hip: one per 252 x 16 tile; test partner and fallback for planes of
// 2 GiB and more).  *n_partials (nullable) receives the number of partials per frame the launch wrote.
enum : int { MOTION_TILED = 0, MOTION_AUTO = 1 };
hipError_t launch_motion(hipStream_t stream, Elem elem, PlaneRun ref, const void* prev0, int64_t prev0_row_pitch,
                         int n_frames, int w, int h, float inv_scale, double* partials, int mode = MOTION_AUTO,
                         int* n_partials = nullptr);
int motion_march_partials(int w, int h);   // partials per frame of the march kernel (workspace sizing; geometry only)
bool launch_motion_march(hipStream_t stream, Elem elem, PlaneRun ref, const void* prev0, int64_t prev0_row_pitch, int n_frames,
                         int w, int h, double* partials, int* n_partials, hipError_t* err);
// Fixed-point motion (integer_motion.c arithmetic, motion_fixed.hip): partials are [n_frames][tiles] uint64 SADs of
// the Q8 blurred planes.
hipError_t launch_motion_fixed(hipStream_t stream, int bit_depth, Elem elem, PlaneRun ref, const void* prev0,
                               int64_t prev0_row_pitch, int n_frames, int w, int h, unsigned long long* partials);

// ---- PSNR (FFmpeg psnr filter) and SSIM (FFmpeg ssim filter) ----------------------------------
constexpr int kSseBlocksPerPlane = 256;
// partials: [n_frames][kSseBlocksPerPlane] uint64 SSE of the (w x h) rectangle starting at a.base / b.base
hipError_t launch_sse(hipStream_t stream, Elem elem, PlaneRun a, PlaneRun b, int n_frames, int w, int h,
                      unsigned long long* partials);

constexpr int kSsimTileBW = 32, kSsimTileBH = 8;  // tile = 32 x 8 windows (4x4-block grid)
inline int ssim_tiles(int w, int h) {
  const int ww = (w >> 2) - 1, wh = (h >> 2) - 1;
  if (ww < 1 || wh < 1) return 0;
  return ((ww + kSsimTileBW - 1) / kSsimTileBW) * ((wh + kSsimTileBH - 1) / kSsimTileBH);
}
// main = distorted, ref = reference (order of the filter's inputs).  partials: [n_frames][tiles] doubles.
// sse_partials (nullable): [n_frames][tiles] uint64 -- the squared error of the 4*(w>>2) x 4*(h>>2) part of the
// plane falls out of the block sums the SSIM needs anyway (ss - 2*s12), so PSNR costs no second pass; the
// right / bottom remainder strips (w or h not a multiple of 4) are left to launch_sse.
hipError_t launch_ssim(hipStream_t stream, Elem elem, PlaneRun main, PlaneRun ref, int n_frames, int w, int h,
                       int max_value, double* partials, unsigned long long* sse_partials);

// ---- luma statistics (white bookend-frame detection, the step before the scoring path) ----------
constexpr int kLumaBlocks = 128;
// out: [n_frames][3] uint64 = {sum, sum of squares, count(sample > threshold)}; partials: [n_frames][kLumaBlocks][3].
// gray_bit_depth 0: statistics of the samples as they are; 8/10/12: of gray = clamp(round((Y - 16 s) * 255 / (219 s)), 0, 255),
// s = 2^(bpc - 8) -- the limited -> full range expansion behind cv2's BGR2GRAY --, threshold in those 8-bit units.
hipError_t launch_luma_stats(hipStream_t stream, Elem elem, PlaneRun luma, int n_frames, int w, int h,
                             unsigned threshold, int gray_bit_depth, unsigned long long* partials,
                             unsigned long long* out);
void luma_gray_map(int bit_depth, float* a, float* b);   // the f32 (scale, offset) pair the kernel applies

// ---- finalize -------------------------------------------------------------------------------
// Fixed-order reduction of every partial array of a batch into per-frame records.
struct FinalizeArgs {
  int n_frames;
  int has_vif, has_adm, has_motion, n_sse_planes, n_ssim_planes;
  const double* vif_part[4];   int vif_tiles[4];
  const long long* vif_fx_part[4];            // non-null: fixed-point VIF partials (kVifFxPartials int64 per tile)
  const double* adm_part[4];   int adm_tiles[4];   float adm_area[4];  // cropped-window area per scale
  const long long* adm_fx_part[4];            // non-null: fixed-point ADM per-row partials
  int adm_fx_tiles_x[4], adm_fx_top[4], adm_fx_bottom[4], adm_fx_num_shift[4], adm_fx_den_shift[4];
  long long* adm_fx_acc;                      // [capacity][4][6] ring: the six accumulators per frame and scale
  const double* motion_part;   int motion_tiles;   double motion_norm;  // 2^-(bpc-8) / (w*h)
  const unsigned long long* motion_fx_part;   // non-null: fixed-point motion SAD partials
  unsigned motion_wh;                         // w * h, for normalize_and_scale_sad()
  const unsigned long long* sse_part[3];      // [n_frames][kSseBlocksPerPlane]: whole plane, or the right strip
  const unsigned long long* sse_part_b[3];    // nullable: bottom strip
  const unsigned long long* sse_tile_part[3]; // nullable: [n_frames][ssim_tiles] from the SSIM kernel
  int sse_use_a[3];                           // 1 when sse_part holds data for this batch
  const double* ssim_part[3];  int ssim_tiles[3];  double ssim_norm[3]; // 1/(windows)
  double* records;             // [capacity][record_stride] ring
  int slot_base, slot_step, capacity;  // record row of batch frame f = (slot_base + f*slot_step) % capacity
  int record_stride;
};
hipError_t launch_finalize(hipStream_t stream, const FinalizeArgs& args);

// ---- SSIM family: libvmaf float_ssim / float_ms_ssim (ssim_family.hip) ---------------------------------------------------
constexpr int kSsfTileW = 64, kSsfTileH = 32;   // output tile of the map kernel
constexpr int kMsScales = 5;
// tiles of the (w - 10) x (h - 10) SSIM map of a w x h plane (0: the map is empty)
int ssf_tiles(int w, int h);
// float_ssim's decimation factor: max(1, round(min(w, h) / 256))
int ssf_decimation(int w, int h);
// One SSIM map (11 x 11 Gaussian, valid region).  box > 1: the map is formed on the box-decimated planes
// (ceil(src_w / box) x ceil(src_h / box), float_ssim); box == 1: on the planes themselves (u8 / u16 samples are scaled by
// inv_scale, f32 planes are taken as they are).  partials: [n_frames][ssf_tiles][4] doubles {sum l, sum c, sum s, sum l*c*s}.
// down_ref / down_dis (base non-null; box == 1 and u8 / u16 planes only): the same launch also writes the next MS-SSIM scale,
// as launch_ssf_down would, bit for bit.
hipError_t launch_ssf_map(hipStream_t stream, Elem elem, PlaneRun ref, PlaneRun dis, int n_frames, int src_w, int src_h,
                          int box, float inv_scale, double* partials, MutPlaneRun down_ref = MutPlaneRun{nullptr, 0, 0},
                          MutPlaneRun down_dis = MutPlaneRun{nullptr, 0, 0});
// 9/7 low-pass and 2:1 decimation of a w x h plane pair into ceil(w/2) x ceil(h/2) f32 planes (next MS-SSIM scale).
hipError_t launch_ssf_down(hipStream_t stream, Elem elem, PlaneRun ref, PlaneRun dis, int n_frames, int w, int h,
                           float inv_scale, MutPlaneRun out_ref, MutPlaneRun out_dis);
// Per-frame epilogue into the extension ring (PQA_EXT_* layout): tile sums in a fixed order, means, the MS-SSIM product in
// double.  A null fs_part / ms_part[0] leaves that feature's slots NaN.
struct SsfFinalizeArgs {
  int n_frames;
  double* ext;                 // [capacity][ext_stride] ring
  int ext_stride;
  int slot_base, slot_step, capacity;   // ring row of batch frame f = (slot_base + f * slot_step) % capacity
  const double* fs_part;   int fs_tiles;   double fs_norm;      // 1 / map pixels
  const double* ms_part[kMsScales];   int ms_tiles[kMsScales];   double ms_norm[kMsScales];
};
hipError_t launch_ssf_finalize(hipStream_t stream, const SsfFinalizeArgs& args);
// NaN into n_rows consecutive ring rows starting at slot_base (frames that get no spatial features, fresh rings)
hipError_t launch_ext_fill_nan(hipStream_t stream, double* ext, int slot_base, int n_rows, int capacity, int stride);

// ---- CIEDE2000: libvmaf ciede (ciede.hip) ------------------------------------------------------------------------------
constexpr int kCiedeTileW = 64, kCiedeTileH = 4;    // chroma samples per workgroup tile: a chroma row per wave
// tiles of a cw x ch chroma plane (one double partial each)
int ciede_tiles(int cw, int ch);
// Sum of the CIEDE2000 differences of every luma pixel of w x h frames (planes Y, U, V of u8 / u16 samples at bit_depth;
// chroma ceil(w / 2^hshift) x ceil(h / 2^vshift), upsampled by replication).  partials: [n_frames][ciede_tiles] doubles.
hipError_t launch_ciede(hipStream_t stream, Elem elem, const PlaneRun ref[3], const PlaneRun dis[3], int n_frames, int w,
                        int h, int hshift, int vshift, int bit_depth, double* partials);
// Per-frame epilogue: fixed-order sum of the partials, mean (x norm = 1 / (w h)) and 45 - 20 log10(mean) in double, into
// slots PQA_EXT_CIEDE_MEAN_DE / PQA_EXT_CIEDE2000 of the extension ring; the other slots of the row are left alone.
struct CiedeFinalizeArgs {
  int n_frames;
  double* ext;
  int ext_stride;
  int slot_base, slot_step, capacity;   // ring row of batch frame f = (slot_base + f * slot_step) % capacity
  const double* partials;
  int n_tiles;
  double norm;
};
hipError_t launch_ciede_finalize(hipStream_t stream, const CiedeFinalizeArgs& args);
// The kernel's CIEDE2000 device function on n Lab pairs [n][6] (f32, device pointers) -> de_out[n] (pqa_debug_ciede2000).
hipError_t launch_ciede_debug(hipStream_t stream, const float* lab_pairs, int n, float* de_out);

// ---- Delta E ITP, ITU-R BT.2124 (delta_itp.hip) ---------------------------------------------------------------------------
constexpr int kItpSums = 8;      // per frame: sum dE, sum dI^2, sum dT^2, sum dP^2, max dE, pixels above the threshold, pixels, sum I of the reference
constexpr int kItpChunk = 8;     // frame pairs per launch of the entries
// A pqa_itp_spec as the kernels take it: both matrices rewritten about the neutral axis (the head of delta_itp.hip).
//   R' = gy Y + cu (Cb - u0) + cv (Cr - v0) + o    L = ls G + lr (R - G) + lb (B - G)    (one entry per row)
struct ItpCoef {
  int transfer;
  float u0, v0;
  float gy[3], cu[3], cv[3], o[3];
  float ls[3], lr[3], lb[3];
  float peak, gamma_m1, threshold;   // gamma_m1: the HLG system gamma - 1 at `peak`
};
void itp_prepare(const pqa_itp_spec& spec, ItpCoef* coef);
// what is wrong with a spec (the argument rules of pqa_delta_itp; no device call), or null
const char* itp_spec_error(const pqa_itp_spec& spec);
// tiles of a cw x ch chroma plane (the 64 x 4 tile of ciede_kernel; kItpSums doubles each)
int itp_tiles(int cw, int ch);
// The partial sums of every tile of n_frames frame pairs (planes Y, Cb, Cr of u8 / u16 samples; chroma ceil(w / 2^hshift) x
// ceil(h / 2^vshift), upsampled by replication) into partials[n_frames][itp_tiles][kItpSums]; then, per frame, their fixed-order
// sums into out[n_frames][kItpSums].
hipError_t launch_delta_itp(hipStream_t stream, Elem elem, const ItpCoef& coef, const PlaneRun ref[3], const PlaneRun dis[3],
                            int n_frames, int w, int h, int hshift, int vshift, double* partials);
hipError_t launch_delta_itp_finalize(hipStream_t stream, const double* partials, int n_tiles, int n_frames, double* out);
// The kernel's device function on n code triples [n][3] = (Y, Cb, Cr) (f32, device pointers) -> itp_out[n][3] = (720 I, 360 Ct,
// 720 Cp) (pqa_debug_itp).
hipError_t launch_delta_itp_debug(hipStream_t stream, const ItpCoef& coef, const float* yuv, int n, float* itp_out);

// ---- CAMBI: libvmaf cambi banding index (cambi.hip) --------------------------------------------------------------------
constexpr int kCambiScales = 5, kCambiDiffs = 4;
constexpr int kCambiParamInts = 22;   // pqa_debug_cambi_params: ws, r, piw, T, tvi[4], weights[4], (w_s, h_s)[5]
// The host-built tables of a w x h frame (definition: tests/cambi_ref.py CONST).
struct CambiParams {
  int ws, r, piw, mask_t;
  int tvi[kCambiDiffs];        // tvi_for_diff[d], d = 1..4
  int weights[kCambiDiffs];    // contrast weights
  int sw[kCambiScales], sh[kCambiScales];
  int64_t off[kCambiScales + 1];     // scale s's samples start at off[s] of a frame's [off[5]] work planes
  int chunk[kCambiScales + 1];       // pooling chunks of scale s: [chunk[s], chunk[s + 1])
  int topk[kCambiScales];            // k = clamp((int)(0.6 N), 1, N)
};
CambiParams cambi_params(int w, int h);
// Once per context before launch_cambi: lets the c-value kernel of this size and bit depth have its LDS (> 64 KiB at 10 bit).
hipError_t cambi_prepare(const CambiParams& prm, int bit_depth);
// Work planes of cambi_sb frames, allocated by the context when PQA_FEAT_CAMBI is set.
struct CambiWork {
  uint16_t* plane;    // [sb][off[5]]  10-bit samples per scale (mode-filtered at s > 0)
  uint8_t* mask;      // [sb][off[5]]
  float* cmap;        // [sb][off[5]]  c-values
  uint32_t* hist;     // [sb][5][2048] radix-select histograms
  int32_t* sel;       // [sb][5][4]    radix-select state
  double* partials;   // [sb][chunk[5]]
};
// CAMBI of the luma of n_frames frames (u8 / u16 samples at bit_depth 8 or 10) into slot `slot` of the extension ring
// rows (slot_base + f * slot_step) % capacity; the other slots of the rows are left alone.  n_frames <= the sb of `wk`.
// wk.cmap then holds each frame's c-values of scales 0..4 at offsets prm.off[s] (pqa_debug_cambi_cmap reads them).
hipError_t launch_cambi(hipStream_t stream, Elem elem, PlaneRun luma, int n_frames, int w, int h, int bit_depth,
                        const CambiParams& prm, const CambiWork& wk, double* ext, int ext_stride, int slot, int slot_base,
                        int slot_step, int capacity);

// ---- PSNR-HVS: libvmaf psnr_hvs (psnr_hvs.hip) ----------------------------------------------------------------------------
constexpr int kPhvTileRows = 4;       // block rows per workgroup (32 blocks side by side, eight lanes each)
constexpr int kPhvTableFloats = 384;  // pqa_debug_psnr_hvs_tables: CSF[3][64], M[3][64]
// Blocks and workgroups of the three planes: plane p owns workgroups [tile0[p], tile0[p + 1]).
struct PsnrHvsGeometry {
  int nbx[3], nby[3], tiles_x[3], tile0[4];
};
void psnr_hvs_geometry(const int pw[3], const int ph[3], PsnrHvsGeometry* g);
// The CSF tables (f32) and the mask tables M = (0.3885746225901003 * CSF)^2 as libvmaf stores them: out[kPhvTableFloats].
void psnr_hvs_tables(float* out);
// The kernel's od_bin_fdct8x8 (its own __host__ __device__ function) on n row-major 8 x 8 int32 blocks, on the host.
void psnr_hvs_fdct8x8_host(const int32_t* in, int32_t* out, int n);
// Once per process before launch_psnr_hvs: uploads the tables to constant memory.
hipError_t psnr_hvs_prepare();
// Block error sums of the Y, Cb, Cr planes of n_frames frames (u8 / u16 samples) -> partials [n_frames][geo.tile0[3]]
// doubles.  block_err (nullable, debug): frame 0's per-block sums of plane dbg_plane, [nby][nbx] f32.
hipError_t launch_psnr_hvs(hipStream_t stream, Elem elem, const PlaneRun ref[3], const PlaneRun dis[3], int n_frames,
                           const PsnrHvsGeometry& geo, double* partials, float* block_err = nullptr, int dbg_plane = 0);
// Per-frame epilogue: fixed-order sums per plane, mse_p = sum / (64 blocks_p), 10 log10(peak^2 / mse) (+inf at 0) and the
// 0.8 / 0.1 / 0.1 combination, into slots PQA_EXT2_PSNR_HVS_* of the ext2 ring; slot PQA_EXT2_RESERVED is left alone.
struct PsnrHvsFinalizeArgs {
  int n_frames;
  double* ext2;
  int ext_stride;
  int slot_base, slot_step, capacity;   // ring row of batch frame f = (slot_base + f * slot_step) % capacity
  const double* partials;
  int tile0[4];
  int blocks[3];
  double peak;                          // 2^bpc - 1
};
hipError_t launch_psnr_hvs_finalize(hipStream_t stream, const PsnrHvsFinalizeArgs& args);

// ---- XPSNR: FFmpeg's xpsnr filter (xpsnr.hip) --------------------------------------------------------------------------
constexpr int kXpStrip = 16;          // block rows per LDS strip (even: 2 x 2 groups never straddle two strips)
constexpr int kXpLdsCols = 732;       // the widest block (b = 728 at 16384 x 16384) plus the 2-column halo on each side
constexpr int kXpBlockVals = 5;       // per block: luma sse, sa, ta, then the SSE of chroma block k of U and V
constexpr unsigned long long kXpGamma = 2;   // XPSNR_GAMMA: the temporal term's weight
// The frame's block grids (vf_xpsnr.c get_wsse).  plain (b < 4): one block per plane and WSSE = SSE.
struct XpsnrGeometry {
  int W, H, Wc, Hc, n_planes, bit_depth;
  int b, bv, smooth, plain;
  int bsx, bsy, w_blk, h_blk, n_blk;      // luma blocks (bsx = bsy = b unless plain)
  int cbx, cby, cw_blk, ch_blk, nc_blk;   // chroma blocks: (b * Wc) / W x (b * Hc) / H
  double A;                               // sqrt(16 * 2^(2d - 9) / sqrt(max(1e-5, W H / (3840 * 2160))))
};
void xpsnr_geometry(int w, int h, int wc, int hc, int n_planes, int bit_depth, XpsnrGeometry* g);
// Exact block sums of n_frames frames (u8 / u16 samples): out[n_frames][geo.n_blk][kXpBlockVals].  Frame f's predecessors
// are frames f - 1 and f - 2 of the run; h1 / h2 (nullptr: zero planes; row pitches in elements) stand for frames -1 and -2.
hipError_t launch_xpsnr_blocks(hipStream_t stream, Elem elem, const PlaneRun ref[3], const PlaneRun dis[3], int n_frames,
                               const void* h1, int64_t h1_pitch, const void* h2, int64_t h2_pitch, bool hfr,
                               const XpsnrGeometry& geo, unsigned long long* out);
// Per frame: weights (into wbuf [n_frames][geo.n_blk]), smoothing, WSSE and dB into slots 0..5 of ring row
// (slot_base + f) % capacity of ext3; the reserved slots are left alone.
struct XpFinalizeArgs {
  int n_frames;
  const unsigned long long* blk;
  double* wbuf;
  double* ext3;
  int ext_stride, slot_base, capacity;
  XpsnrGeometry g;
};
hipError_t launch_xpsnr_finalize(hipStream_t stream, const XpFinalizeArgs& args);

// ---- SI / TI: FFmpeg's siti filter (siti.hip) ----------------------------------------------------------------------------
constexpr int kSitiSegRows = 128;     // rows per wave segment (bounds the int32 sum of m^2 per lane: 128 * 1023^2 < 2^31)
// wave partials per frame and clip of a w x h luma plane (4 doubles each)
int siti_partials(int w, int h);
// SI and TI of n_frames frames of n_clips clips (clip 0: distorted, clip 1: reference; u8 / u16 luma, 8 or 10 bit):
// frame f's predecessor is frame f - 1 of the run; prev0[z] (nullptr: a chain start, TI 0; row pitch in elements) stands
// for frame -1 of clip z.  full[z]: clip z is full range (no conversion).  partials: [n_frames][2][siti_partials(w, h)][4].
// SI / TI of clip z go to slots 2z / 2z + 1 of ring row (slot_base + f) % capacity of ext4; the other slots are left alone.
// gmap (nullable, test hook): the (w - 2) x (h - 2) gradient map of frame 0 of clip 0.
hipError_t launch_siti(hipStream_t stream, Elem elem, const PlaneRun clip[2], const void* const prev0[2],
                       const int64_t prev0_pitch[2], const bool full[2], int n_clips, int n_frames, int w, int h,
                       double* partials, double* ext4, int ext_stride, int slot_base, int capacity, float* gmap);

// ---- capture integrity: what FFmpeg's freezedetect / blackdetect / scdet reduce a frame to (integrity.hip) --------------
constexpr int kIntegrityBlocks = 128;   // workgroups per frame and plane (512 waves, a wave per row at a time)
// Exact per-plane SAD of n_frames frames of n_planes planes (pw x ph samples each, u8 / u16) and the number of luma samples
// <= black_threshold.  anchor false: frame f against frame f - 1 of the run, frame 0 against prev0 (all nullptr: a chain
// start, no SAD for frame 0; row pitches in elements); anchor true: every frame against prev0.
// partials: [n_frames][3][kIntegrityBlocks][2] uint64.  ext5 (nullable): ring row (slot_base + f) % capacity gets the SADs in
// slots 0..2 (NaN at a chain start and for planes >= n_planes), the black count in slot 3 and NaN in slots 4..ext_stride-1.
// out (nullable): [n_frames][3] uint64 SADs.
hipError_t launch_integrity(hipStream_t stream, Elem elem, const PlaneRun cur[3], const void* const prev0[3],
                            const int64_t prev0_pitch[3], const int pw[3], const int ph[3], int n_planes, int n_frames,
                            bool anchor, unsigned black_threshold, unsigned long long* partials, double* ext5,
                            int ext_stride, int slot_base, int capacity, unsigned long long* out);

// ---- temporal alignment: banded cross-frame SSE (cross_sse.hip) ----------------------------------------------------------
// D[i][c] = sum over luma pixels of (ref_i - dis_{i + k_lo + c})^2, exact uint64; UINT64_MAX where i + k_lo + c is outside
// [0, dis.n).  Frame f of a clip lives at base + (f % ring) * frame_pitch (a clip that lies whole in memory: ring >= n).
struct XsseClip {
  const void* base;
  int64_t row_pitch, frame_pitch;   // elements
  int ring;                         // frames the buffer holds
  int64_t n;                        // frames of the clip
};
constexpr int kXsseSegsPerWave = 64;   // 128-pixel row segments per wave: 8192 pixels in an i32 accumulator (limit 131071)
constexpr int kXsseNormBlocks = 16;    // workgroups per frame of the sum of centred squares
constexpr int kXsseValuBlocks = 64;    // row groups per (frame, offset) of the VALU path
int xsse_dis_tiles(int span);          // captured 32-frame tiles one reference tile meets
int xsse_blocks(int w, int h);         // workgroups per tile pair of the MFMA path
size_t xsse_part_bytes(bool mfma, int w, int h, int span, int n_tiles);   // workspace of one launch over n_tiles reference tiles
// 8-bit only: norm_part[(first + f) * kXsseNormBlocks + b], f < count = partial sums of (x - 128)^2 of frames first ...
hipError_t launch_xsse_norms(hipStream_t stream, const XsseClip& clip, int64_t first, int count, int w, int h,
                             unsigned long long* norm_part);
// Rows 32 tile0 ... 32 (tile0 + n_tiles) - 1 (those below ref.n) of out[ref.n][span].  mfma: 8-bit samples on
// v_mfma_i32_32x32x32_i8, needs the norm partials of every frame it touches (indexed by clip frame number); otherwise plain
// VALU integers (u8 / u16), norm_ref / norm_dis unused.  Both write the same integers.
hipError_t launch_cross_sse(hipStream_t stream, Elem elem, bool mfma, const XsseClip& ref, const XsseClip& dis, int w, int h,
                            int k_lo, int span, int tile0, int n_tiles, void* part, const unsigned long long* norm_ref,
                            const unsigned long long* norm_dis, unsigned long long* out);

// ---- spatial alignment: shifted-window luma SSE (shift_sse.hip) ----------------------------------------------------------
// out[f][j][i] = sum over the window R <= x < w - R, R <= y < h - R of (ref_f[y][x] - dis_f[y + j - R][x + i - R])^2, exact
// uint64, for n_frames pairs (frame f at base + f * frame_pitch, pitches in elements).  part / rowsq: workspaces of
// shift_part_bytes / shift_rowsq_bytes for the same (elem, w, h, R, n_frames).
constexpr int kShiftMaxRadius = 16;
constexpr int kShiftChunk = 8;   // frame pairs per launch of the two entries
size_t shift_part_bytes(Elem elem, int w, int h, int R, int n_frames);
size_t shift_rowsq_bytes(int h, int R, int n_frames);
hipError_t launch_shift_sse(hipStream_t stream, Elem elem, const void* ref, int64_t ref_row_pitch, int64_t ref_frame_pitch,
                            const void* dis, int64_t dis_row_pitch, int64_t dis_frame_pitch, int n_frames, int w, int h, int R,
                            void* part, unsigned long long* rowsq, unsigned long long* out);

// ---- level alignment: per-level transfer table (level_stats.hip) ---------------------------------------------------------
// out[f][v][0 / 1 / 2] = count / sum of dis / sum of dis^2 over the pixels of frame pair f whose reference sample is v (above
// L - 1: bin L - 1), L = 2^bit_depth, exact uint64, for n_frames pairs of one w x h plane (frame f at base + f * frame_pitch,
// pitches in elements).  out: device memory of level_out_bytes(bit_depth, n_frames), zeroed by the launch.
constexpr int kLevelChunk = 8;   // frame pairs per launch of the two entries
size_t level_out_bytes(int bit_depth, int n_frames);
hipError_t launch_level_stats(hipStream_t stream, Elem elem, int bit_depth, const void* ref, int64_t ref_row_pitch,
                              int64_t ref_frame_pitch, const void* dis, int64_t dis_row_pitch, int64_t dis_frame_pitch,
                              int n_frames, int w, int h, unsigned long long* out);

// ---- exact-integer polyphase resampler (resample.hip) ---------------------------------------------------------------------
// One axis of the filter: destination sample i reads the source samples first[i] ... first[i] + taps - 1 with the int16
// coefficients coeff[i][0 .. taps) (scale 2^14, a row sums to 16384, zero-padded; edge replication folded in).  Built on the
// host in double; resample_table returns 0, or -1 when the arguments are out of range, a row needs
// more than kRsMaxTaps taps or its sum of |q| reaches 32768.  filter: PQA_RESAMPLE_*; x0_q16 / ext_q16: the source window.
constexpr int kRsMaxTaps = 32;
constexpr int kRsChunk = 8;   // frames per launch of the two entries
struct ResampleTable {
  std::vector<int32_t> first;
  std::vector<int16_t> coeff;   // [n_dst][taps]
  int taps = 0;
};
int resample_table(int filter, int n_src, int n_dst, int64_t x0_q16, int64_t ext_q16, ResampleTable* out);
// What the kernel reads for a pair of tables: `words` is uploaded as it is (first / coefficient pairs of both axes, the
// source footprint of every tile column and tile row); the rest sizes the launch.
struct ResamplePlan {
  std::vector<int32_t> words;
  size_t off_first_h = 0, off_coef_h = 0, off_first_v = 0, off_coef_v = 0, off_tile_h = 0, off_tile_v = 0;   // in words
  int wpad = 0, ph = 0, pv = 0, th = 0, mid_rows = 0, sw = 0;
  size_t lds_bytes = 0;
};
void resample_plan(const ResampleTable& th, const ResampleTable& tv, int dst_w, int dst_h, ResamplePlan* plan);
// n_frames planes of src_w x src_h -> dst_w x dst_h (frame f at base + f * frame_pitch, pitches in elements; samples of
// `bits` bits).  dev_words: plan.words in device memory.  Reads no source sample outside the plane, writes no byte outside
// the dst_w samples of a destination row.
hipError_t launch_resample(hipStream_t stream, Elem elem, int bits, const ResamplePlan& plan, const int* dev_words, const void* src,
                           int64_t src_row_pitch, int64_t src_frame_pitch, int src_w, int src_h, void* dst, int64_t dst_row_pitch,
                           int64_t dst_frame_pitch, int dst_w, int dst_h, int n_frames);

// ---- sub-pixel registration: tile-wise gradient moments (flow_moments.hip) ------------------------------------------------
// out[f][j][i][0..5] = sum over the counted pixels (1 <= x <= w - 2, 1 <= y <= h - 2) of tile (i, j) = (x / tile, y / tile) of
// gx^2, gx gy, gy^2, gx dt, gy dt, dt^2 (gx, gy: Sobel of ref + dis; dt: 3 x 3 binomial of dis - ref), exact int64, for n_frames
// pairs of one w x h plane (3 ... 8192 each way; frame f at base + f * frame_pitch, pitches in elements; samples of `bits`
// bits).  tile: 8, 16, 32 or 64.  out: device memory of flow_out_bytes(); every entry is written.
constexpr int kFlowChunk = 8;   // frame pairs per launch of the two entries
bool flow_tile_ok(int tile);
size_t flow_out_bytes(int w, int h, int tile, int n_frames);
hipError_t launch_flow_moments(hipStream_t stream, Elem elem, int bits, const void* ref, int64_t ref_row_pitch,
                               int64_t ref_frame_pitch, const void* dis, int64_t dis_row_pitch, int64_t dis_frame_pitch,
                               int n_frames, int w, int h, int tile, long long* out);

// ---- colour-matrix alignment: cross-plane moments and the matrix apply (colour_moments.hip) ---------------------------------
// Both work on the chroma grid ceil(w / 2^hshift) x ceil(h / 2^vshift) of w x h frames (shifts 0 or 1; u8 / u16 samples of
// `bit_depth` bits, a sample above 2^bit_depth - 1 is read as that); plane p of frame f at base + f * frame_pitch, pitches in
// elements.  Definitions, bounds and the widening interval: the head of colour_moments.hip.
// out[f][28]: the upper triangle, row-major, of the sum over the unmasked chroma samples of z z^T, z = (1, SYr, Ur, Vr, SYd,
// Ud, Vd), exact uint64; device memory of n_frames * 28 words, zeroed by the launch.
constexpr int kColourSums = 28;
constexpr int kColourChunk = 8;                  // frames / frame pairs per launch of the entries
constexpr int64_t kColourMaxGain = 1 << 16;      // |m[r][1..3]| below it (Q14: gains below 4)
constexpr int64_t kColourMaxOffset = 1 << 28;    // |m[r][0]| below it (Q14 code values)
bool colour_shift_ok(int hshift, int vshift);
bool colour_matrix_ok(const int32_t m[12]);
int colour_flush_steps(int bit_depth, int hshift, int vshift);   // row steps between two widenings of a lane's int32 partials
hipError_t launch_colour_moments(hipStream_t stream, Elem elem, int bit_depth, int hshift, int vshift, const PlaneRun ref[3],
                                 const PlaneRun dis[3], int n_frames, int w, int h, unsigned lo, unsigned hi,
                                 unsigned long long* out);
// dst = the frame through m[3][4] (Q14, column 0 the offset); reads no sample outside a source plane, writes none outside the
// plane sizes of dst.
hipError_t launch_colour_apply(hipStream_t stream, Elem elem, int bit_depth, int hshift, int vshift, const int32_t m[12],
                               const PlaneRun src[3], const MutPlaneRun dst[3], int n_frames, int w, int h);

// ---- active-picture detection: row and column profiles (line_profiles.hip) ---------------------------------------------------
// out[f][y][0 / 1] = sum / sum of squares of row y, then out[f][h + x][0 / 1] of column x, exact uint64, for n_frames planes
// of w x h samples (1 ... 8192 each way; frame f at base + f * frame_pitch, pitches in elements; u8 / u16 samples of
// `bit_depth` bits, a sample above 2^bit_depth - 1 is read as that).  out: device memory of profile_out_bytes(), zeroed by
// the launch.  A workgroup reads a stripe of kProfStripe columns by a band of kProfBand rows once for both profiles.
constexpr int kProfStripe = 1024;   // columns of a workgroup: 64 lanes of 16
constexpr int kProfBand = 64;       // rows of a workgroup: 16 a wave
constexpr int kProfChunk = 8;       // frames per launch of the two entries
size_t profile_out_bytes(int w, int h, int n_frames);
int profile_flush_rows(int bit_depth);   // rows between two widenings of a lane's uint32 column sums
hipError_t launch_line_profiles(hipStream_t stream, Elem elem, int bit_depth, const void* base, int64_t row_pitch,
                                int64_t frame_pitch, int n_frames, int w, int h, unsigned long long* out);

// ---- distortion map: tile-wise second-order statistics of a frame pair (tile_moments.hip) ------------------------------------
// out[f][j][i][0..5] = sum r, sum d, sum r^2, sum d^2, sum r d, sum |d - r| over the pixels of tile (i, j) of `tile` x `tile`
// pixels (8, 16, 32 or 64; edge tiles hold the pixels that exist), exact uint64, for n_frames plane pairs of w x h samples
// (1 ... 8192 each way; frame f at base + f * frame_pitch, pitches in elements; u8 / u16 samples of `bits` bits, a sample above
// 2^bits - 1 is read as that).  out: device memory of tile_out_bytes(); every word is written, nothing needs zeroing.
constexpr int kTileSums = 6;    // sums a tile
constexpr int kTileChunk = 8;   // frame pairs per launch of the two entries
bool tile_size_ok(int tile);
size_t tile_out_bytes(int w, int h, int tile, int n_frames);
hipError_t launch_tile_moments(hipStream_t stream, Elem elem, int bits, const void* ref, int64_t ref_row_pitch,
                               int64_t ref_frame_pitch, const void* dis, int64_t dis_row_pitch, int64_t dis_frame_pitch,
                               int n_frames, int w, int h, int tile, unsigned long long* out);

// ---- distortion spectrum: second moments of the Haar octave bands of a frame pair (band_moments.hip) --------------------------
// out[f][l-1][o][0..2] = sum r_o^2, sum d_o^2, sum r_o d_o (the last as int64) over the coefficients of level l = 1 ... levels
// and orientation o (0 H, 1 V, 2 D, 3 A) of the unnormalised Haar transform whose 2^l x 2^l support lies inside the plane, exact,
// for n_frames plane pairs of w x h samples (1 ... 8192 each way; frame f at base + f * frame_pitch, pitches in elements; u8 /
// u16 samples of `bits` bits, a sample above 2^bits - 1 is read as that).  part: device memory of band_part_bytes() for the
// workgroups' partial sums; out: device memory of band_out_bytes(); every word of both is written, nothing needs zeroing.
constexpr int kBandSums = 3;    // sums a band
constexpr int kBandChunk = 8;   // frame pairs per launch of the two entries
bool band_levels_ok(int levels);
size_t band_out_bytes(int levels, int n_frames);
size_t band_part_bytes(int w, int h, int levels, int n_frames);
hipError_t launch_band_moments(hipStream_t stream, Elem elem, int bits, const void* ref, int64_t ref_row_pitch,
                               int64_t ref_frame_pitch, const void* dis, int64_t dis_row_pitch, int64_t dis_frame_pitch,
                               int n_frames, int w, int h, int levels, void* part, unsigned long long* out);

// ---- temporal distortion: tile-wise second-order statistics of the frame differences of a clip pair (temporal_moments.hip) ----
// With a = R_k - R_{k-1}, b = D_k - D_{k-1}, e = D_k - R_k (signed) for the transitions k = 1 ... n_frames - 1:
// out[k-1][j][i][0..6] = sum a, sum b, sum a^2, sum b^2, sum a b, sum a e, sum e^2 over the pixels of tile (i, j) of `tile` x
// `tile` pixels (8, 16, 32 or 64; edge tiles hold the pixels that exist), exact (words 0, 1, 4, 5 as int64), for n_frames plane
// pairs of w x h samples (1 ... 8192 each way; frame f at base + f * frame_pitch, pitches in elements; u8 / u16 samples of
// `bits` bits, a sample above 2^bits - 1 is read as that).  out: device memory of temporal_out_bytes(); every word is written,
// nothing needs zeroing.  n_frames <= 1 launches nothing.  walk: the A/B partner in which a workgroup walks through the launch's
// transitions with its block of the previous pair in registers, instead of a workgroup per transition; the same integers.
constexpr int kTemporalSums = 7;    // sums a tile
constexpr int kTemporalChunk = 8;   // frame pairs per launch of the two entries (the host entry keeps one more as predecessor)
size_t temporal_out_bytes(int w, int h, int tile, int n_frames);
hipError_t launch_temporal_moments(hipStream_t stream, Elem elem, int bits, const void* ref, int64_t ref_row_pitch,
                                   int64_t ref_frame_pitch, const void* dis, int64_t dis_row_pitch, int64_t dis_frame_pitch,
                                   int n_frames, int w, int h, int tile, bool walk, unsigned long long* out);

// ---- field alignment: field-against-field squared errors of a clip pair (field_moments.hip) ----------------------------------
// With E(A, p, B, q) = sum over the row pairs i < h / 2 and the columns of (A[2 i + p][x] - B[2 i + q][x])^2, for the transitions
// k = 1 ... n_frames - 1: out[k-1][2 p + q] = E(D_k, p, R_k, q), out[k-1][4 + 2 p + q] = E(D_k, p, R_{k-1}, q),
// out[k-1][8 + 2 p + q] = E(D_{k-1}, p, R_k, q), out[k-1][12] = E(D_k, 0, D_k, 1), out[k-1][13] = E(R_k, 0, R_k, 1), exact
// uint64, for n_frames plane pairs of w x h samples (w 1 ... 8192, h 2 ... 8192; the last row of an odd height is not counted;
// frame f at base + f * frame_pitch, pitches in elements; u8 / u16 samples of `bits` bits, a sample above 2^bits - 1 is read as
// that).  out: device memory of field_out_bytes(), zeroed by the launch.  n_frames <= 1 launches nothing.  A workgroup reads a
// block of kFieldCols columns by kFieldRows rows of the four planes of a transition.
constexpr int kFieldSums = 14;    // words a transition
constexpr int kFieldChunk = 8;    // frame pairs per launch of the two entries (the host entry keeps one more as predecessor)
constexpr int kFieldCols = 128;   // columns of a workgroup's block
constexpr int kFieldRows = 128;   // rows of a workgroup's block: 64 row pairs
size_t field_out_bytes(int n_frames);
hipError_t launch_field_moments(hipStream_t stream, Elem elem, int bits, const void* ref, int64_t ref_row_pitch,
                                int64_t ref_frame_pitch, const void* dis, int64_t dis_row_pitch, int64_t dis_frame_pitch,
                                int n_frames, int w, int h, unsigned long long* out);

// ---- coding-grid detection: gradient energy per line of a frame pair (edge_profiles.hip) -------------------------------------
// With a / b the difference of a sample of the reference / captured plane and its upper neighbour (row line y = 1 ... h - 1,
// summed over x) or its left neighbour (column line x = 1 ... w - 1, summed over y): out[f][y][0..2] = sum a^2, sum b^2,
// sum a b (the last as int64) of row line y, then out[f][h + x][0..2] of column line x; line 0 of each axis is zero.  Exact, for
// n_frames plane pairs of w x h samples (1 ... 8192 each way; frame f at base + f * frame_pitch, pitches in elements; u8 / u16
// samples of `bits` bits, a sample above 2^bits - 1 is read as that).  out: device memory of edge_out_bytes(), zeroed by the
// launch.  A workgroup reads a stripe of kEdgeStripe columns by a band of kEdgeBand rows (and the row above each wave's run).
constexpr int kEdgeStripe = 1024;   // columns of a workgroup: 64 lanes of 16
constexpr int kEdgeBand = 64;       // rows of a workgroup: a run of 16 consecutive rows a wave
constexpr int kEdgeSums = 3;        // sums a line
constexpr int kEdgeChunk = 8;       // frame pairs per launch of the two entries
size_t edge_out_bytes(int w, int h, int n_frames);
// rows between two widenings of a lane's 32-bit column sums: floor((2^32 - 1) / top^2), signed floor((2^31 - 1) / top^2)
int edge_flush_rows(int bit_depth, bool is_signed);
hipError_t launch_edge_profiles(hipStream_t stream, Elem elem, int bits, const void* ref, int64_t ref_row_pitch,
                                int64_t ref_frame_pitch, const void* dis, int64_t dis_row_pitch, int64_t dis_frame_pitch,
                                int n_frames, int w, int h, unsigned long long* out);

// ---- pixel-format conversion: chroma layout, siting and depth in one pass (format_convert.hip) ----------------------------------
// n_frames planes of one kind of a luma_w x luma_h frame (1 ... 8192 each way) go from the layout `src` to the layout `dst`:
// chroma shifts 0 ... 2, siting per axis (kSiteCosited / kSiteCentre, void where the shift is 0), samples of 8 / 10 / 12 bits
// (u8 at 8 bit, otherwise u16; a source sample above 2^bits - 1 is read as that).  Definition (triangle taps in exact integers,
// one rounding that carries the depth change): the head of format_convert.hip.  Frame f at base + f * frame_pitch, pitches in
// BYTES.  generic: the general kernel whatever the layout (the fast paths' test partner; the same integers).  Reads no source
// sample outside the plane, writes no byte outside the samples of a destination row.  hipErrorInvalidValue, before any launch,
// on a layout or size out of range, more than 65535 frames, a side that is not made of whole samples or a pitch below a row.
constexpr int kSiteCosited = 0, kSiteCentre = 1;   // the PQA_SITE_* values
constexpr int kConvertChunk = 8;                   // frames per chunk of the host entry
struct ConvertLayout {
  int bits, hshift, vshift, hsite, vsite;
};
inline int convert_plane_size(int luma, int shift) { return (luma + (1 << shift) - 1) >> shift; }
hipError_t launch_format_convert(hipStream_t stream, const ConvertLayout& src, const ConvertLayout& dst, int luma_w, int luma_h,
                                 bool generic, const void* src_planes, int64_t src_row_pitch, int64_t src_frame_pitch, void* dst_planes,
                                 int64_t dst_row_pitch, int64_t dst_frame_pitch, int n_frames);

// ---- packed RGB captures -> Y'CbCr planes: unpack, matrix, range, depth, subsampling, siting in one pass (rgb_convert.hip) ----
// n_frames packed frames of w x h pixels (1 ... 8192 each way; format: host::FMT_BGRA ... FMT_R210, 4 bytes a pixel) become the
// planes dst[0..2] = Y, U, V of the layout `dst` (bits 8 / 10, chroma shifts 0 / 1, siting per axis; chroma planes of
// convert_plane_size() samples; u8 at 8 bit, otherwise u16) through the Q14 matrix m[3][4], column 0 the offset.  dst[1] and
// dst[2] both null: luma only.  Definition, the int32 bound and the fast paths: the head of rgb_convert.hip.  Frame f at
// base + f * frame_pitch, pitches in BYTES.  generic: the general kernel whatever the layout (the fast paths' test partner; the
// same integers).  Reads no source row beyond 4 * w bytes, writes no byte outside the samples of a destination row.
// hipErrorInvalidValue, before any launch, on a format, layout or size out of range, more than 65535 frames, a matrix beyond
// host::rgb_matrix_fits, one chroma destination of two, an r210 base or pitch that is no multiple of 4, a destination that is not
// made of whole samples or a pitch below a row.
constexpr int kRgbChunk = 8;   // frames per chunk of the host entry
hipError_t launch_rgb_convert(hipStream_t stream, int format, const ConvertLayout& dst, bool generic, const int32_t m[12],
                              const void* src, int64_t src_row_pitch, int64_t src_frame_pitch, void* const dst_planes[3],
                              const int64_t dst_row_pitch[3], const int64_t dst_frame_pitch[3], int w, int h, int n_frames);

// ---- transfer-curve alignment: planes through an integer table (table_apply.hip) ---------------------------------------------
// dst[y][x] = table[min(src[y][x], L - 1)], L = 2^bit_depth, for n_frames planes of w x h samples (1 ... 8192 each way; u8 at
// 8 bit, otherwise u16).  table: L entries of the sample type in DEVICE memory, 16-byte aligned; any table, monotone or not.
// Frame f at base + f * frame_pitch, pitches in BYTES; dst may be exactly src.  Reads no source byte past a row's last sample,
// writes no destination byte past it.  hipErrorInvalidValue, before any launch, on a null pointer, a size or depth out of
// range, more than 65535 frames, a side that is not made of whole samples or a pitch below a row.
constexpr int kTableChunk = 8;   // frames per chunk of the host entry
hipError_t launch_table_apply(hipStream_t stream, Elem elem, int bit_depth, const void* table, const void* src, int64_t src_row_pitch,
                              int64_t src_frame_pitch, void* dst, int64_t dst_row_pitch, int64_t dst_frame_pitch, int n_frames, int w,
                              int h);

// ---- deinterlacing: a kept field and a motion-adaptive interpolated one (deinterlace.hip) ---------------------------------------
// Output planes of the source frames t0 ... t0 + n - 1 of a clip of `count` planes of w x h samples at `src` (w 1 ... 8192,
// h 2 ... 8192; u8 at 8 bit, otherwise u16, a source sample above 2^bits - 1 is read as that); the neighbours t - 1 and t + 1
// are clamped to 0 ... count - 1 by the kernel.  per 1: one output a source frame, the field of parity `first` kept; per 2: two,
// `first` and then 1 - first.  mode 0 intra, 1 adaptive; the arithmetic heads deinterlace.hip.  dst: n * per planes, the first
// one that of t0.  Frame f at base + f * frame_pitch, pitches in BYTES; dst may not overlap src.  uniform: the still-picture fast
// path (the same integers).  A workgroup writes kDeintColBytes bytes of kDeintWaves * kDeintBand rows.  Reads no source byte past
// a row's last sample, writes no destination byte past it.  hipErrorInvalidValue, before any launch, on a null pointer, a size,
// depth, mode, parity or rate out of range, t0 ... t0 + n - 1 outside the clip, more than 32767 frames, a side that is not made
// of whole samples or a pitch below a row.
constexpr int kDeintChunk = 8;          // source frames per launch of the two entries
constexpr int kDeintColBytes = 1024;    // bytes of a row a wave marches down: 64 lanes of 16
constexpr int kDeintBand = 16;          // rows of a wave's band
constexpr int kDeintWaves = 4;          // bands of a workgroup, one below the other
hipError_t launch_deinterlace(hipStream_t stream, Elem elem, int bit_depth, int mode, int first, int per, bool uniform, const void* src,
                              int64_t src_row_pitch, int64_t src_frame_pitch, int count, int t0, int n, void* dst, int64_t dst_row_pitch,
                              int64_t dst_frame_pitch, int w, int h);

// ---- overlay masking: planes through a feathered mask (mask_blend.hip) ---------------------------------------------------------
// dst = (src (256 - a) + fill a + 128) >> 8 for n_frames planes of w x h samples (1 ... 8192 each way; u8 at 8 bit, otherwise
// u16), a interpolated from a grid of nodes 0 ... 256 that lie 1 << sx by 1 << sy samples apart (0 ... kMaskMaxStep each),
// mask_grid(w, sx) columns by mask_grid(h, sy) rows of uint16 in DEVICE memory; the definition heads mask_blend.hip.  fill: a
// plane of the same geometry with pitches of its own, or null for fill_const (at most 2^bit_depth - 1).  Frame f at base +
// f * frame_pitch, pitches in BYTES.  Of the grid only the rows bounds.row0 ... are read, at their place in it.  dst may be
// exactly src (same base and pitches): then only bounds.rect, the samples with a > 0 as mask_node_bounds gives them, is
// launched (x0 >= x1: nothing is); otherwise the whole plane is written.
// Reads no source byte past a row's last sample, writes no destination byte past it.  hipErrorInvalidValue, before any launch,
// on a null pointer, a size, depth, step or fill out of range, more than 65535 frames, a side that is not made of whole
// samples, a pitch below a row or dst == fill.
constexpr int kMaskChunk = 8;     // frames per chunk of the host entry
constexpr int kMaskMaxStep = 6;
inline int mask_grid(int size, int step_log2) { return ((size + (1 << step_log2) - 1) >> step_log2) + 1; }
// What the host learns from one pass over a grid.  rect = {x0, y0, x1, y1}: the bounding rectangle of the samples on which a
// non-zero node weighs (x0 >= x1: there is none).  The node rows row0 ... row0 + rows - 1 hold every non-zero node: only they
// need to be in device memory.
struct MaskBounds {
  int rect[4];
  int row0, rows;
};
bool mask_node_bounds(const uint16_t* nodes, int w, int h, int sx, int sy, MaskBounds* bounds);   // false: a node above 256
hipError_t launch_mask_blend(hipStream_t stream, Elem elem, int bit_depth, const uint16_t* nodes, int sx, int sy, unsigned fill_const,
                             const MaskBounds& bounds, const void* src, int64_t src_row_pitch, int64_t src_frame_pitch, const void* fill,
                             int64_t fill_row_pitch, int64_t fill_frame_pitch, void* dst, int64_t dst_row_pitch, int64_t dst_frame_pitch,
                             int n_frames, int w, int h);

}  // namespace pqa
