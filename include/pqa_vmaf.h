/*
 * pqa_vmaf.h -- C ABI of the MI355X-native VMAF feature engine (libpqa_vmaf.so).
 *
 * Drop-in boundary.  In the reference (yoseph007/PQA2) the whole scoring hot path is three child
 * processes started by VMAFAnalyzer.analyze_videos():
 *     subprocess.Popen([ffmpeg, ..., "-lavfi", "libvmaf=..."])      app/vmaf_analyzer.py:406-419,446
 *     subprocess.run([ffmpeg, ..., "-lavfi", "psnr=stats_file=..."]) app/vmaf_analyzer.py:1027-1045
 *     subprocess.run([ffmpeg, ..., "-lavfi", "ssim=stats_file=..."]) app/vmaf_analyzer.py:1057-1075
 * This library sits where those calls are: the host feeds decoded planes, the library returns one
 * fixed-size feature record per frame, and the host (Python, as in the reference) applies the
 * bundled models/vmaf_*.json SVM, pools, and writes the libvmaf-format JSON / stats files that
 * _parse_vmaf_results (app/vmaf_analyzer.py:628-964) reads back.  INTEGRATION.md shows the binding.
 *
 * Conventions: plain C, no exceptions cross the boundary.  Every function returns PQA_OK (0) or a
 * negative pqa_status; pqa_last_error() explains the most recent failure.  The caller owns every
 * buffer it passes in; the library owns all device memory it allocates.  A context is
 * single-threaded (mirrors VMAFAnalyzer._process_lock, app/vmaf_analyzer.py:29,251); the only call
 * legal from another thread is pqa_cancel() (mirrors terminate_analysis, app/vmaf_analyzer.py:139).
 * One context per GPU.
 */
#ifndef PQA_VMAF_H
#define PQA_VMAF_H

#include <stddef.h>
#include <stdint.h>

#if defined(__GNUC__)
#define PQA_API __attribute__((visibility("default")))
#else
#define PQA_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef enum pqa_status {
  PQA_OK = 0,
  PQA_EINVAL = -1,     /* bad argument / unsupported geometry */
  PQA_EDEVICE = -2,    /* HIP runtime failure (text in pqa_last_error) */
  PQA_ENOMEM = -3,     /* host or device allocation failed */
  PQA_ECANCELLED = -4, /* pqa_cancel() was called; pqa_reset() re-arms the context */
  PQA_ESTATE = -5      /* call sequence error: collecting a frame that was never submitted (or whose record a
                          later frame has replaced), or submitting a frame whose ring slot still holds the
                          UNCOLLECTED record of a different frame (result_capacity too small for the caller's
                          collect cadence).  Nothing is launched or overwritten when this is returned. */
} pqa_status;

/* feature mask: which extractors run per frame */
enum {
  PQA_FEAT_VIF = 1u << 0,    /* libvmaf float VIF, 4 scales        (libvmaf= call site, :377-419) */
  PQA_FEAT_ADM = 1u << 1,    /* libvmaf float ADM, 4 scales        (same call site)               */
  PQA_FEAT_MOTION = 1u << 2, /* libvmaf motion (SAD of blurred ref) (same call site)              */
  PQA_FEAT_PSNR = 1u << 3,   /* FFmpeg psnr filter: per-plane SSE   (:1027-1034)                  */
  /* A plane narrower or lower than 8 samples holds no 8 x 8 window (a chroma plane of a small frame at a chroma shift of
   * 2, e.g. 5 x 5 for 19 x 19): no SSIM is computed for it and its PQA_REC_SSIM slot is exactly 0.0, as vf_ssim.c's
   * ssim_plane returns for it; the plane's SSE (PQA_FEAT_PSNR) is unaffected. */
  PQA_FEAT_SSIM = 1u << 4,   /* FFmpeg ssim filter: per-plane SSIM  (:1057-1064)                  */
  PQA_FEAT_VMAF = PQA_FEAT_VIF | PQA_FEAT_ADM | PQA_FEAT_MOTION,
  PQA_FEAT_ALL = PQA_FEAT_VMAF | PQA_FEAT_PSNR | PQA_FEAT_SSIM,  /* stays 31: the features of the 24-double record */
  /* libvmaf's SSIM family (`feature=name=float_ssim` / `float_ms_ssim`, the filter's ssim=1 / ms_ssim=1): luma only, f32,
   * results in the EXTENSION record (PQA_EXT_*, pqa_collect_ext), never in the 24-double record.  Both run on the frames
   * that get VIF / ADM (n_subsample); the extension slots of the other frames hold NaN.  Geometry limits: float_ssim needs
   * the decimated plane (ceil(w / f) x ceil(h / f), f = max(1, round(min(w, h) / 256))) to be >= 11 in both directions,
   * float_ms_ssim needs its 5th scale (ceil-halved four times) >= 11, i.e. w, h >= 161; pqa_create returns PQA_EINVAL
   * naming the feature otherwise (float_ssim fits every size pqa_create accepts, w, h >= 16).  Definition and its unpinned items: DESIGN.md sections 1 and 5. */
  PQA_FEAT_FLOAT_SSIM = 1u << 5,
  PQA_FEAT_MS_SSIM = 1u << 6,
  /* bit 7 stays unassigned (tests use it as the unknown bit pqa_create rejects) */
  /* libvmaf's ciede (`feature=name=ciede`, log key ciede2000): CIEDE2000 colour difference of every luma pixel, chroma
   * upsampled by replication, results in extension slots PQA_EXT_CIEDE2000 / PQA_EXT_CIEDE_MEAN_DE on the frames that get
   * VIF / ADM (n_subsample).  Needs n_planes = 3 (PQA_EINVAL naming ciede2000 otherwise); any chroma subsampling.
   * Definition and its unpinned items: DESIGN.md sections 1 and 5. */
  PQA_FEAT_CIEDE = 1u << 8,
  /* libvmaf's cambi banding index (`feature=name=cambi`): CAMBI of the distorted luma in extension slot PQA_EXT_CAMBI;
   * with PQA_FEAT_CAMBI_FULL_REF also CAMBI of the reference luma in PQA_EXT_CAMBI_SOURCE (cambi_full_reference =
   * max(cambi - cambi_source, 0) is formed by the caller).  Frames that get VIF / ADM only (n_subsample).  Luma only, any
   * n_planes, bit depth 8 or 10 (PQA_EINVAL naming cambi at 12 bit); FULL_REF without PQA_FEAT_CAMBI is PQA_EINVAL.
   * Every frame size pqa_create accepts is defined (the window grows with w + h).  Definition and its unpinned items:
   * DESIGN.md sections 1 and 5; its host-built tables: pqa_debug_cambi_params. */
  PQA_FEAT_CAMBI = 1u << 9,
  PQA_FEAT_CAMBI_FULL_REF = 1u << 10,
  /* libvmaf's psnr_hvs (`feature=name=psnr_hvs`): per plane, 8x8 blocks at a step of 7, Daala's integer DCT, contrast
   * masking and CSF weighting; psnr_hvs_y / _cb / _cr, psnr_hvs and the three plane MSEs in the SECOND extension record
   * (PQA_EXT2_*, pqa_collect_ext2) on the frames that get VIF / ADM (n_subsample).  Needs n_planes = 3 (PQA_EINVAL naming
   * psnr_hvs otherwise) and every plane >= 8 x 8; any chroma subsampling, 8, 10 and 12 bit.  Definition and its unpinned
   * items: DESIGN.md sections 1 and 5; its tables: pqa_debug_psnr_hvs_tables. */
  PQA_FEAT_PSNR_HVS = 1u << 11,
  /* FFmpeg's xpsnr filter (libavfilter/vf_xpsnr.c, FFmpeg >= 7.0): PSNR with per-block weights from the reference's
   * spatial and temporal activity; XPSNR y / u / v and the three WSSE values in the THIRD extension record (PQA_EXT3_*,
   * pqa_collect_ext3) on EVERY frame, like psnr / ssim, whatever n_subsample is.  The temporal term reads the previous one
   * (first order) or two (PQA_FEAT_XPSNR_HFR: second order, for integer frame rates >= 32) reference frames of the chain:
   * the frames before it in the batch, the pair the context keeps from its previous batch, or the history armed with
   * pqa_set_ref_history; zero planes at a chain start.  n_planes 1 or 3, any chroma subsampling, 8, 10 and 12 bit.
   * PQA_EINVAL naming xpsnr for an odd width or height when w * h > 2048 * 1152 (2 x 2 activity), and for
   * PQA_FEAT_XPSNR_HFR without PQA_FEAT_XPSNR.  Definition and its unpinned items: DESIGN.md sections 1 and 5; its block
   * sums: pqa_debug_xpsnr_blocks. */
  PQA_FEAT_XPSNR = 1u << 12,
  PQA_FEAT_XPSNR_HFR = 1u << 13,
  /* FFmpeg's siti filter (libavfilter/vf_siti.c): ITU-T P.910 spatial (SI: standard deviation of the 3 x 3 Sobel
   * magnitude over the interior pixels) and temporal (TI: standard deviation of the frame difference) information of the
   * distorted and of the reference luma, in the FOURTH extension record (PQA_EXT4_*, pqa_collect_ext4) on EVERY frame,
   * whatever n_subsample is.  Limited-range samples are mapped to full range first; PQA_FEAT_SITI_REF_FULL /
   * PQA_FEAT_SITI_DIS_FULL say that clip's samples are full range already.  TI reads the previous frame of each clip:
   * the frame before it in the batch, the plane the context keeps from its previous batch, the caller's halo (reference)
   * or the history armed with pqa_set_ref_history / pqa_set_dis_history; TI = 0 at a chain start.  8 and 10 bit only
   * (PQA_EINVAL naming siti for 12 bit, and for a range bit without PQA_FEAT_SITI); any n_planes and chroma subsampling
   * (luma only).  Definition and its unpinned items: DESIGN.md sections 1 and 5; its gradient map: pqa_debug_siti_plane. */
  PQA_FEAT_SITI = 1u << 14,
  PQA_FEAT_SITI_REF_FULL = 1u << 15,
  PQA_FEAT_SITI_DIS_FULL = 1u << 16,
  /* Capture integrity of the DISTORTED clip: the per-frame quantities FFmpeg's freezedetect, blackdetect and scdet filters
   * reduce a frame to (libavfilter/vf_freezedetect.c, vf_blackdetect.c, vf_scdet.c), in the FIFTH extension record
   * (PQA_EXT5_*, pqa_collect_ext5) on EVERY frame, whatever n_subsample is: the exact sum of absolute differences of
   * every plane against the previous distorted frame, and the number of luma samples <= the black threshold
   * (pqa_set_black_threshold).  The previous frame is the frame before it in the batch, the planes the context keeps from
   * its previous batch, or the history armed with pqa_set_dis_history_planes; no SAD (NaN) at a chain start.  8, 10 and
   * 12 bit, n_planes 1 or 3, any chroma subsampling.  freezedetect's anchored differences: pqa_frame_sad.  The filters'
   * host state machines: pqa2_amd/integrity.py; definition and its unpinned items: DESIGN.md sections 1 and 5. */
  PQA_FEAT_INTEGRITY = 1u << 17,
  PQA_FEAT_KNOWN = PQA_FEAT_ALL | PQA_FEAT_FLOAT_SSIM | PQA_FEAT_MS_SSIM | PQA_FEAT_CIEDE | PQA_FEAT_CAMBI |
                   PQA_FEAT_CAMBI_FULL_REF | PQA_FEAT_PSNR_HVS | PQA_FEAT_XPSNR | PQA_FEAT_XPSNR_HFR | PQA_FEAT_SITI |
                   PQA_FEAT_SITI_REF_FULL | PQA_FEAT_SITI_DIS_FULL | PQA_FEAT_INTEGRITY  /* what pqa_create accepts */
};

/* One record = PQA_RECORD_DOUBLES 8-byte slots per frame. */
enum {
  PQA_REC_VIF_NUM = 0,  /* [4] vif numerator per scale                                        */
  PQA_REC_VIF_DEN = 4,  /* [4] vif denominator per scale     (vif_scale_s = num/den)           */
  PQA_REC_ADM_NUM = 8,  /* [4] adm numerator per scale                                        */
  PQA_REC_ADM_DEN = 12, /* [4] adm denominator per scale     (adm2 = sum num / sum den)        */
  PQA_REC_MOTION = 16,  /*     motion_i (motion2 is a host-side min over neighbours)           */
  PQA_REC_SSIM = 17,    /* [3] FFmpeg ssim Y, U, V                                            */
  PQA_REC_SSE = 20,     /* [3] FFmpeg psnr SSE Y, U, V: uint64 bit-cast into the slot (exact)   */
  PQA_REC_RESERVED = 23,
  PQA_RECORD_DOUBLES = 24
};

/* One EXTENSION record = PQA_EXT_DOUBLES slots per frame, kept beside the record ring (same slots, capacity and wrap) when
 * the context runs PQA_FEAT_FLOAT_SSIM, PQA_FEAT_MS_SSIM, PQA_FEAT_CIEDE or PQA_FEAT_CAMBI.  Slots of a feature the context
 * does not run, and of frames that get no spatial features (n_subsample), are NaN. */
enum {
  PQA_EXT_FLOAT_SSIM = 0,     /*     float_ssim: mean of l*c*s over the (decimated) map                */
  PQA_EXT_FLOAT_SSIM_LCS = 1, /* [3] its means of l, c, s                                               */
  PQA_EXT_MS_SSIM = 4,        /*     float_ms_ssim = l4^0.1333 * prod_j c_j^w_j * s_j^w_j (in double)    */
  PQA_EXT_MS_SSIM_L = 5,      /* [5] mean of l per scale 0..4                                           */
  PQA_EXT_MS_SSIM_C = 10,     /* [5] mean of c per scale                                                */
  PQA_EXT_MS_SSIM_S = 15,     /* [5] mean of s per scale                                                */
  PQA_EXT_RESERVED = 20,      /*     first slot after the SSIM family                                   */
  PQA_EXT_CIEDE2000 = 20,     /*     ciede2000 = 45 - 20 log10(mean dE00), in double (+inf at mean 0)     */
  PQA_EXT_CIEDE_MEAN_DE = 21, /*     the frame's mean CIEDE2000 dE00 over its luma pixels                  */
  PQA_EXT_CAMBI = 22,         /*     cambi of the distorted luma                                        */
  PQA_EXT_CAMBI_SOURCE = 23,  /*     cambi of the reference luma (PQA_FEAT_CAMBI_FULL_REF; NaN without)   */
  PQA_EXT_DOUBLES = 24
};

/* The SECOND extension record = PQA_EXT2_DOUBLES slots per frame, kept beside the record ring (same slots, capacity and
 * wrap) when the context runs PQA_FEAT_PSNR_HVS; read with pqa_collect_ext2.  Frames that get no spatial features
 * (n_subsample) hold NaN, and so does the reserved slot. */
enum {
  PQA_EXT2_PSNR_HVS_Y = 0,    /*     psnr_hvs_y = 10 log10(max^2 / mse_Y), max = 2^bpc - 1 (+inf at mse 0)   */
  PQA_EXT2_PSNR_HVS_CB = 1,   /*     psnr_hvs_cb                                                        */
  PQA_EXT2_PSNR_HVS_CR = 2,   /*     psnr_hvs_cr                                                        */
  PQA_EXT2_PSNR_HVS = 3,      /*     psnr_hvs = 10 log10(max^2 / (0.8 mse_Y + 0.1 (mse_Cb + mse_Cr)))     */
  PQA_EXT2_PSNR_HVS_MSE = 4,  /* [3] mse_Y, mse_Cb, mse_Cr                                               */
  PQA_EXT2_RESERVED = 7,
  PQA_EXT2_DOUBLES = 8
};

/* The THIRD extension record = PQA_EXT3_DOUBLES slots per frame, kept beside the record ring (same slots, capacity and
 * wrap) when the context runs PQA_FEAT_XPSNR; read with pqa_collect_ext3.  Every submitted frame gets its row; slots of
 * planes the context does not have (n_planes 1) and the reserved slots hold NaN. */
enum {
  PQA_EXT3_XPSNR_Y = 0,     /*     XPSNR y = 10 log10(w h (2^bpc - 1)^2 / WSSE_Y) (+inf at WSSE 0)          */
  PQA_EXT3_XPSNR_U = 1,     /*     XPSNR u (chroma plane size)                                            */
  PQA_EXT3_XPSNR_V = 2,     /*     XPSNR v                                                                */
  PQA_EXT3_WSSE = 3,        /* [3] WSSE Y, U, V: integers, exact as doubles                                 */
  PQA_EXT3_RESERVED = 6,    /* [2]                                                                        */
  PQA_EXT3_DOUBLES = 8
};

/* The FOURTH extension record = PQA_EXT4_DOUBLES slots per frame, kept beside the record ring (same slots, capacity and
 * wrap) when the context runs PQA_FEAT_SITI; read with pqa_collect_ext4.  Every submitted frame gets its row; the
 * reserved slots hold NaN. */
enum {
  PQA_EXT4_SI = 0,          /* SI of the distorted luma                                                    */
  PQA_EXT4_TI = 1,          /* TI of the distorted luma (0 at a chain start and on a repeated frame)       */
  PQA_EXT4_SI_SOURCE = 2,   /* SI of the reference luma                                                    */
  PQA_EXT4_TI_SOURCE = 3,   /* TI of the reference luma                                                    */
  PQA_EXT4_RESERVED = 4,    /* [4]                                                                         */
  PQA_EXT4_DOUBLES = 8
};

/* The FIFTH extension record = PQA_EXT5_DOUBLES slots per frame, kept beside the record ring (same slots, capacity and
 * wrap) when the context runs PQA_FEAT_INTEGRITY; read with pqa_collect_ext5.  Every submitted frame gets its row; the
 * values are integers, exact as doubles; the reserved slots hold NaN. */
enum {
  PQA_EXT5_SAD_PREV = 0,    /* [3] sum |dis_i - dis_{i-1}| of Y, U, V; NaN at a chain start / where there is no plane */
  PQA_EXT5_BLACK_COUNT = 3, /* luma samples of dis_i with value <= the black threshold                              */
  PQA_EXT5_RESERVED = 4,    /* [4]                                                                                   */
  PQA_EXT5_DOUBLES = 8
};

typedef struct pqa_config {
  uint32_t struct_size;        /* sizeof(pqa_config), for ABI growth                              */
  int32_t device;              /* HIP device ordinal                                              */
  uint32_t width, height;      /* luma size, both >= 16                                           */
  uint32_t bit_depth;          /* 8, 10 or 12 (samples > 8 bit are little-endian uint16)          */
  uint32_t n_planes;           /* 1 = luma only, 3 = Y,U,V (needed for chroma PSNR/SSIM)          */
  uint32_t chroma_hshift;      /* log2 horizontal chroma subsampling (4:2:0 -> 1)                 */
  uint32_t chroma_vshift;      /* log2 vertical chroma subsampling   (4:2:0 -> 1)                 */
  uint32_t features;           /* PQA_FEAT_* mask                                                 */
  uint32_t max_batch;          /* frames per kernel launch (0 -> auto: ~1.5 GiB of luma, 8..256)   */
  uint32_t result_capacity;    /* records kept on the device, ring indexed by frame_index
                                  (0 -> default 16384)                                            */
  uint32_t n_subsample;        /* libvmaf n_subsample (:379): VIF/ADM on frames i % k == 0 only;
                                  motion on every frame (0/1 -> every frame)                      */
  double vif_enhn_gain_limit;  /* 100.0 default; 1.0 for *neg models (feature_opts_dicts)         */
  double adm_enhn_gain_limit;  /* 100.0 default; 1.0 for *neg models                              */
  uint32_t vif_border;         /* PQA_VIF_BORDER_*: which libvmaf extractor's VIF padding to follow  */
  uint32_t fixed_point;        /* PQA_FIXED_* mask: extractors to run in libvmaf's fixed-point arithmetic
                                  instead of f32 (0 = none: the fast path, the default)              */
} pqa_config;

/* libvmaf has two VIF extractors with different image-border handling.  `model=version=vmaf_v0.6.1`
 * (app/vmaf_analyzer.py:377) names VMAF_integer_feature_vif_* (models/vmaf_v0.6.1.json:31-38), i.e.
 * integer_vif.c, which pads by reflect-101 on all four edges; the vmaf_float_* models name float_vif
 * (vif_tools.c), which repeats the edge sample at the bottom/right edge.  The arithmetic here is f32 in
 * both cases (DESIGN.md "float vs fixed-point" quantifies the residual); this selects the border only.
 * pqa_config.fixed_point goes the whole way per extractor: PQA_FIXED_VIF = integer_vif.c (Q16 taps, Q8 means,
 * 2048-step log2 table, integer accumulators; implies the integer border), PQA_FIXED_MOTION = integer_motion.c
 * (Q8 blurred planes, integer SAD), PQA_FIXED_ADM = integer_adm.c (Q15 db2, int16/int32 bands, reciprocal table,
 * shifted cube accumulators; the six cube roots per scale are taken on the host inside pqa_collect).
 * Bit-identical to oracle/vmaf_int_oracle.c; slower than the f32 path (DESIGN.md section 3 has the numbers). */
enum { PQA_FIXED_VIF = 1, PQA_FIXED_MOTION = 2, PQA_FIXED_ADM = 4, PQA_FIXED_ALL = 7 };
enum {
  PQA_VIF_BORDER_FLOAT = 0,   /* vif_tools.c:   index -i -> i,  n-1+i -> n-i    */
  PQA_VIF_BORDER_INTEGER = 1  /* integer_vif.c: index -i -> i,  n-1+i -> n-1-i  */
};

/* A clip already resident in device memory (HBM): frame f of plane p starts at
 * plane[p] + f * frame_pitch[p]; rows are row_pitch[p] bytes apart.  Pitches are in BYTES. */
typedef struct pqa_device_clip {
  const void* plane[3];
  int64_t row_pitch[3];
  int64_t frame_pitch[3];
} pqa_device_clip;

typedef struct pqa_ctx pqa_ctx;

/* Library / record introspection. */
PQA_API const char* pqa_version(void);
PQA_API int pqa_record_doubles(void);
PQA_API int pqa_ext_doubles(void);
PQA_API int pqa_ext2_doubles(void);
PQA_API int pqa_ext3_doubles(void);
PQA_API int pqa_ext4_doubles(void);
PQA_API int pqa_ext5_doubles(void);

/* Fill cfg with defaults (8-bit 4:2:0, PQA_FEAT_VMAF, gain limits 100). */
PQA_API void pqa_config_init(pqa_config* cfg, uint32_t width, uint32_t height);

/* Create / destroy.  Replaces process start-up of the ffmpeg child (app/vmaf_analyzer.py:446). */
PQA_API int pqa_create(const pqa_config* cfg, pqa_ctx** out);
PQA_API void pqa_destroy(pqa_ctx* ctx);

/* Run all work of this context on an existing HIP stream (e.g. torch's current stream).
 * NULL restores the context's own stream. */
PQA_API int pqa_set_stream(pqa_ctx* ctx, void* hip_stream);

/* Submit one decoded frame pair from HOST memory.  planes[p] / strides[p] (bytes) for p < n_planes.
 * The library copies into pinned staging, uploads on a copy stream and launches kernels once
 * max_batch frames are pending (or at pqa_collect / pqa_flush).  Frames must arrive in increasing,
 * consecutive frame_index order within a clip; motion of the first submitted frame is 0 unless
 * pqa_set_motion_halo() supplied its predecessor.
 * Replaces one frame's worth of the libvmaf/psnr/ssim filter graph input. */
PQA_API int pqa_submit(pqa_ctx* ctx, int64_t frame_index, const void* const ref_planes[3], const int64_t ref_strides[3],
               const void* const dis_planes[3], const int64_t dis_strides[3]);

/* The same for a frame pair that lies in two FILES as packed planes (rows width * sample-size bytes apart, no padding --
 * raw .yuv and .y4m payloads): plane p of the reference frame starts at byte ref_plane_offsets[p] of ref_fd, likewise for
 * the distorted clip.  The library reads (pread) straight into its pinned staging with its packing threads -- one copy out
 * of the page cache and no page faults, against mapping the file and copying from the mapping.  The descriptors are only
 * read, never closed, and their file positions are not moved.  A short read (truncated file, bad offset) is PQA_EINVAL.
 * This is the shape of the reference's inputs: two files (app/vmaf_analyzer.py:411-419, `-i distorted -i reference`). */
PQA_API int pqa_submit_fd(pqa_ctx* ctx, int64_t frame_index, int ref_fd, const int64_t ref_plane_offsets[3], int dis_fd,
                          const int64_t dis_plane_offsets[3]);

/* n_frames CONSECUTIVE frame pairs of two such files in one call: frame first_index + k has plane p at byte
 * ref_plane_offsets[p] + k * ref_frame_stride of ref_fd (a .y4m payload: stride = frame bytes + 6 for "FRAME\n"; raw .yuv:
 * the frame bytes), likewise for the distorted clip.  Same results as n_frames calls of pqa_submit_fd; inside the call the
 * packing threads read frame k + 1 while frame k is on its way to the device -- one wake-up of the threads per staging half
 * (8 frames) instead of one per frame, which is what lets a 2160p clip approach the PCIe rate.  n_frames may be any number
 * up to result_capacity; a caller that reports progress or polls for cancellation submits in runs of a few frames.
 * A short read anywhere in a run is PQA_EINVAL and none of the frames of the staging half it occurred in is submitted. */
PQA_API int pqa_submit_fd_run(pqa_ctx* ctx, int64_t first_index, int32_t n_frames, int ref_fd,
                              const int64_t ref_plane_offsets[3], int64_t ref_frame_stride, int dis_fd,
                              const int64_t dis_plane_offsets[3], int64_t dis_frame_stride);

/* Submit n_frames consecutive frame pairs that are ALREADY in device memory (no copies).  "Already" includes ordering:
 * the context's kernels run on its own stream (or the one given to pqa_set_stream), so whatever produced the frames must be
 * complete -- or on that same stream -- before this call; the same holds for pqa_submit_surfaces and
 * pqa_luma_stats_device.
 * prev_ref_luma (nullable, device pointer, prev_row_pitch bytes) is the reference luma of frame
 * first_index-1 -- the one-frame halo a frame-sharded rank needs for motion.  When NULL the context
 * continues from the last frame it saw if that was first_index-1, else motion(first_index) = 0.
 * The rules of a plane that is scored where it lies (PQA_EINVAL before anything is launched; the context stays usable), with
 * es the sample size, plane p being pw x ph samples and its span = row_pitch x ph bytes:
 *   - pointers are not NULL; row and frame pitches are multiples of es (a frame pitch may be anything else: 0, negative,
 *     smaller than a frame when frames interleave inside the rows);
 *   - row_pitch >= pw * es: no negative, zero or overlapping rows;
 *   - span < 2^32: the VIF, ADM and motion kernels address a plane with unsigned 32-bit byte offsets from its base.  A plane
 *     cut out of a wider buffer with a larger span must be copied first.  From 2^31 bytes on those features run on their
 *     tiled kernels (the march kernels take planes below 2 GiB), with the same results to rounding;
 *   - with PQA_FEAT_SITI in the mask, the luma span < 2^31: the siti kernel has no such partner;
 *   - prev_ref_luma, where a feature in the mask reads it (motion, xpsnr, siti), follows the rules of luma plane 0 with
 *     prev_row_pitch.
 * pqa_submit_surfaces applies the same rules to an NV12 luma plane, which is scored in place. */
PQA_API int pqa_submit_device(pqa_ctx* ctx, int64_t first_index, int32_t n_frames, const pqa_device_clip* ref,
                      const pqa_device_clip* dis, const void* prev_ref_luma, int64_t prev_row_pitch);

/* Decoder surfaces in device memory: what a hardware decoder (VCN through rocDecode / VA-API) writes and what a drop-in
 * that keeps decode on the GPU hands over instead of the planes ffmpeg would feed libvmaf (app/vmaf_analyzer.py:415-416
 * names the two inputs).  NV12: 8-bit Y plane + ONE plane of interleaved U,V pairs at half
 * resolution in both directions.  P01X: the same layout with 16-bit little-endian samples whose value sits in the UPPER
 * bit_depth bits (P010 for a 10-bit context, P012 for a 12-bit one).  Frame f's planes start at luma + f * luma_frame_pitch
 * and chroma + f * chroma_frame_pitch; pitches in BYTES.  chroma may be NULL when the context has n_planes == 1.
 *
 * Packed capture formats: what a capture card delivers (the reference's default pixel format for DeckLink devices is
 * uyvy422, app/options_manager.py:78; v210 is the card's 10-bit format).  All three are 4:2:2: with cw = ceil(w / 2) the
 * chroma planes are cw x h, chroma shifts (1, 0).  For a packed clip luma / luma_row_pitch / luma_frame_pitch describe the
 * PACKED frames and the chroma fields are ignored.
 *   PQA_SURFACE_UYVY, 8 bit: macropixel k of a row is the four bytes U_k, Y_2k, V_k, Y_2k+1; a row holds cw macropixels (the
 *     last Y of an odd-width row is present and never used).  Minimum row pitch 4 * cw bytes.
 *   PQA_SURFACE_YUYV, 8 bit (YUY2): the same with the bytes Y_2k, U_k, Y_2k+1, V_k.
 *   PQA_SURFACE_V210, 10 bit: a row is groups of 6 pixels in four little-endian 32-bit words, three 10-bit components per
 *     word in bits 0-9, 10-19, 20-29 (bits 30-31 are undefined and influence nothing):
 *         w0 = U0 | Y0 << 10 | V0 << 20     w1 = Y1 | U1 << 10 | Y2 << 20
 *         w2 = V1 | Y3 << 10 | U2 << 20     w3 = Y4 | V2 << 10 | Y5 << 20
 *     ceil(w / 6) groups per row (components beyond w / cw in the last group are present and never used).  Minimum row
 *     pitch 16 * ceil(w / 6) bytes; base and pitches are multiples of 4.  Files pad rows to ((w + 47) / 48) * 128 bytes.
 *     The unpacked samples are LSB-aligned uint16 0 ... 1023.
 * A format fits a context when the bit depths agree: NV12 / UYVY / YUYV 8, V210 10, P01X 10 or 12.  No row is read beyond
 * its minimum bytes: a caller's last row may end at the end of its allocation.
 * PQA_SURFACE_PLANAR names planar planes in pqa_host_clip (pqa_submit_packed) only.
 *
 * Packed RGB captures: what a card delivers from an HDMI source or a 4:4:4 chain (FFmpeg's bgra, argb, rgba, abgr and r210).
 * A pixel is 4 bytes in every format; minimum row pitch 4 * w bytes.
 *   PQA_SURFACE_BGRA / _ARGB / _RGBA / _ABGR, 8 bit: the four bytes of a pixel in that order.  The A byte influences nothing
 *     (bgr0 / 0rgb are the same bytes).  Files do not pad rows.
 *   PQA_SURFACE_R210, 10 bit: a pixel is one BIG-endian 32-bit word, R in bits 29-20, G in 19-10, B in 9-0; bits 31-30 are
 *     undefined and influence nothing.  Base and pitches are multiples of 4.  Files pad rows to ((w + 63) / 64) * 256 bytes.
 * As for the packed 4:2:2 formats no row is read beyond its minimum bytes and no destination row is written beyond its samples.
 * The RGB values are accepted by pqa_rgb_convert / pqa_rgb_convert_device ONLY: pqa_submit_surfaces, pqa_submit_packed and
 * pqa_unpack refuse them as they refuse any unknown format. */
enum { PQA_SURFACE_PLANAR = 0, PQA_SURFACE_NV12 = 1, PQA_SURFACE_P01X = 2, PQA_SURFACE_UYVY = 3, PQA_SURFACE_YUYV = 4, PQA_SURFACE_V210 = 5,
       PQA_SURFACE_BGRA = 6, PQA_SURFACE_ARGB = 7, PQA_SURFACE_RGBA = 8, PQA_SURFACE_ABGR = 9, PQA_SURFACE_R210 = 10 };
typedef struct pqa_surface_clip {
  uint32_t struct_size;        /* sizeof(pqa_surface_clip) */
  uint32_t format;             /* PQA_SURFACE_* */
  const void* luma;
  const void* chroma;
  int64_t luma_row_pitch, luma_frame_pitch;
  int64_t chroma_row_pitch, chroma_frame_pitch;
} pqa_surface_clip;

/* Submit n_frames consecutive frame pairs held as decoder surfaces.  An NV12 luma plane is scored where it lies;
 * interleaved chroma is split into planes and 16-bit samples are shifted down on the way (device-side, into the
 * context's own staging; nothing crosses PCIe).  The context must be 4:2:0 (chroma shifts 1, 1) when n_planes == 3.
 * prev_ref (nullable) carries, as its frame 0, the reference frame first_index-1 -- the motion halo of a frame-sharded
 * rank; NULL continues from the last frame the context saw, as pqa_submit_device does.  Same record semantics as the
 * other submit calls.
 * Each of ref, dis and prev_ref may instead be a packed capture clip (PQA_SURFACE_UYVY / _YUYV / _V210, chosen per side): it
 * is unpacked on the device into the context's own staging (unpack.hip; never scored in place), and the records are
 * bit-identical to a planar submission of the same samples.  With n_planes == 3 a packed side needs the context's chroma
 * shifts to be (1, 0) and an NV12 / P01X side (1, 1), so the two kinds mix only in a luma-only context (n_planes == 1:
 * no chroma is decoded).  PQA_EINVAL, before any device call, on a format that does not fit the context's bit depth, a
 * row pitch below the format's minimum, or a v210 base / pitch that is not a multiple of 4. */
PQA_API int pqa_submit_surfaces(pqa_ctx* ctx, int64_t first_index, int32_t n_frames, const pqa_surface_clip* ref,
                                const pqa_surface_clip* dis, const pqa_surface_clip* prev_ref);

/* A clip in HOST memory for pqa_submit_packed.  format PQA_SURFACE_PLANAR: frames[] holds n_frames * n_planes plane
 * pointers, frame-major (frame f's plane p at frames[f * n_planes + p]), rows strides[p] bytes apart as in pqa_submit.
 * A packed format (PQA_SURFACE_UYVY / _YUYV / _V210, fitting the context's bit depth): frames[] holds n_frames pointers
 * to packed frames, rows strides[0] bytes apart. */
typedef struct pqa_host_clip {
  uint32_t struct_size;        /* sizeof(pqa_host_clip) */
  uint32_t format;             /* PQA_SURFACE_PLANAR or a packed format */
  const void* const* frames;
  int64_t strides[3];
} pqa_host_clip;

/* Submit n_frames consecutive frame pairs from HOST memory where either side (independently) is a packed capture clip.
 * The packed bytes are copied into pinned memory as they are, cross PCIe once and are unpacked in device memory: nothing is
 * de-interleaved on the host, and a v210 frame moves 8/3 bytes per pixel where its planar form moves 4.  Frames pending
 * from pqa_submit are flushed first, as pqa_submit_surfaces does; the frames then travel in chunks of at most 8 through
 * grow-only pinned and device buffers of this entry's own (two alternating sets, allocated on first use, so that a chunk is
 * copied and uploaded while the kernels of the chunk before run).  Synchronous on the host side: on
 * return the caller's buffers are free, the kernels are queued and the records are collected as usual.  With
 * n_planes == 3 the context must be 4:2:2 (chroma shifts 1, 0) when a side is packed.  PQA_EINVAL, before any device
 * call, on a null pointer, a struct_size or format mismatch, or a stride below a row (v210: no multiple of 4);
 * PQA_ESTATE, before anything is copied, when a record slot of the run is still uncollected. */
PQA_API int pqa_submit_packed(pqa_ctx* ctx, int64_t first_index, int32_t n_frames, const pqa_host_clip* ref,
                              const pqa_host_clip* dis);

/* Host-memory variant of the halo for the pqa_submit path.  pqa_set_motion_halo(c, p, s) is
 * pqa_set_ref_history(c, &p, 1, s); p == NULL restarts the chain (n_prev = 0). */
PQA_API int pqa_set_motion_halo(pqa_ctx* ctx, const void* prev_ref_luma_host, int64_t row_stride);

/* The reference history in front of the next submitted frame (call it before that frame, e.g. frames a-1 and a-2 of a
 * frame-sharded rank that starts at a): prev_luma_host[0] is the luma of reference frame first-1, prev_luma_host[1] that
 * of first-2 (rows row_stride bytes apart), n_prev of them (0, 1 or 2; a missing one is a zero plane, as at a chain
 * start).  It arms motion's halo from prev_luma_host[0] exactly as pqa_set_motion_halo does, and PQA_FEAT_XPSNR's
 * temporal history from both; n_prev = 0 restarts the chain.  PQA_EINVAL on n_prev outside 0..2 or a null plane. */
PQA_API int pqa_set_ref_history(pqa_ctx* ctx, const void* const* prev_luma_host, int32_t n_prev, int64_t row_stride);

/* The distorted clip's luma in front of the next submitted frame (frame a-1 of a frame-sharded rank that starts at a; rows
 * row_stride bytes apart): PQA_FEAT_SITI's TI of the distorted clip continues from it.  NULL restarts the distorted chain
 * (TI 0 on the next frame).  The reference side arrives through pqa_set_motion_halo / pqa_set_ref_history.  A no-op
 * without PQA_FEAT_SITI. */
PQA_API int pqa_set_dis_history(pqa_ctx* ctx, const void* prev_dis_luma_host, int64_t row_stride);

/* The distorted clip's frame in front of the next submitted frame with ALL its planes (frame a-1 of a frame-sharded rank
 * that starts at a; planes[p] has rows strides[p] bytes apart, p < n_planes): PQA_FEAT_INTEGRITY's differences continue
 * from it.  It also arms what pqa_set_dis_history arms (from planes[0]).  planes == NULL restarts both chains.  A no-op
 * without PQA_FEAT_INTEGRITY and PQA_FEAT_SITI. */
PQA_API int pqa_set_dis_history_planes(pqa_ctx* ctx, const void* const planes[3], const int64_t strides[3]);

/* The integer sample value at or below which a luma sample counts as black (PQA_EXT5_BLACK_COUNT).  Default: FFmpeg
 * blackdetect's pixel_black_th = 0.10 on a limited-range clip, trunc(16 f + 0.10 * 219 f), f = 2^(bit_depth - 8): 37 /
 * 151 / 606 at 8 / 10 / 12 bit.  Legal before the first submit and after pqa_reset (PQA_ESTATE otherwise); PQA_EINVAL
 * above the largest sample value.  pqa_reset keeps the value. */
PQA_API int pqa_set_black_threshold(pqa_ctx* ctx, uint32_t threshold);

/* freezedetect's anchored differences, synchronously: out[f * 3 + p] = sum |frame_f[p] - anchor[p]| over plane p, exact,
 * for n_frames frames in HOST memory against one anchor frame (frames[f * 3 + p]: plane p of frame f, rows strides[p] bytes
 * apart; anchor_planes[p] rows anchor_strides[p] bytes apart; p < n_planes, out is 0 for the other planes).  n_frames
 * need not fit max_batch.  Needs PQA_FEAT_INTEGRITY (PQA_ESTATE otherwise).  Independent of the scoring chain. */
PQA_API int pqa_frame_sad(pqa_ctx* ctx, const void* const anchor_planes[3], const int64_t anchor_strides[3],
                          const void* const* frames, const int64_t strides[3], int32_t n_frames, uint64_t* out);

/* The same for a clip in DEVICE memory (frames: n_frames frames, pitches in bytes) against an anchor frame in device
 * memory (anchor_planes[p] rows anchor_row_pitch[p] bytes apart). */
PQA_API int pqa_frame_sad_device(pqa_ctx* ctx, const void* const anchor_planes[3], const int64_t anchor_row_pitch[3],
                                 const pqa_device_clip* frames, int32_t n_frames, uint64_t* out);

/* Launch whatever pqa_submit has pending (partial batch). */
PQA_API int pqa_flush(pqa_ctx* ctx);

/* Copy `count` records starting at frame first_index into records[count][PQA_RECORD_DOUBLES].  Launches a pending
 * partial batch, then waits only for the batch that produced the youngest requested record (one completion event
 * per batch): batches submitted later keep running while the caller works on these records (SVM, pooling).
 * Frames that were never submitted, or whose record has been replaced, give PQA_ESTATE.  A collected record's ring
 * slot becomes free for frame index + k * result_capacity.  Replaces reading the libvmaf JSON log / stats files. */
PQA_API int pqa_collect(pqa_ctx* ctx, int64_t first_index, int32_t count, double* records);

/* pqa_collect with the extension records: exactly its contract (the same waits, the same PQA_ESTATE rules; the frames are
 * marked collected), and in addition ext[count][PQA_EXT_DOUBLES] receives the extension rows of the same frames.  ext may
 * be NULL.  A context that runs none of PQA_FEAT_FLOAT_SSIM, PQA_FEAT_MS_SSIM, PQA_FEAT_CIEDE, PQA_FEAT_CAMBI returns
 * all-NaN rows.
 * pqa_collect(c, f, n, r) is pqa_collect_ext(c, f, n, r, NULL). */
PQA_API int pqa_collect_ext(pqa_ctx* ctx, int64_t first_index, int32_t count, double* records, double* ext);

/* pqa_collect_ext with the second extension record as well: exactly its contract, and in addition
 * ext2[count][PQA_EXT2_DOUBLES] receives the ext2 rows of the same frames.  ext and ext2 may be NULL.  A context without
 * PQA_FEAT_PSNR_HVS returns all-NaN ext2 rows. */
PQA_API int pqa_collect_ext2(pqa_ctx* ctx, int64_t first_index, int32_t count, double* records, double* ext, double* ext2);

/* pqa_collect_ext2 with the third extension record as well: ext3[count][PQA_EXT3_DOUBLES] receives the ext3 rows of the
 * same frames.  ext, ext2 and ext3 may be NULL.  A context without PQA_FEAT_XPSNR returns all-NaN ext3 rows. */
PQA_API int pqa_collect_ext3(pqa_ctx* ctx, int64_t first_index, int32_t count, double* records, double* ext, double* ext2,
                             double* ext3);

/* pqa_collect_ext3 with the fourth extension record as well: ext4[count][PQA_EXT4_DOUBLES] receives the ext4 rows of the
 * same frames.  ext, ext2, ext3 and ext4 may be NULL.  A context without PQA_FEAT_SITI returns all-NaN ext4 rows. */
PQA_API int pqa_collect_ext4(pqa_ctx* ctx, int64_t first_index, int32_t count, double* records, double* ext, double* ext2,
                             double* ext3, double* ext4);

/* pqa_collect_ext4 with the fifth extension record as well: ext5[count][PQA_EXT5_DOUBLES] receives the ext5 rows of the
 * same frames.  ext .. ext5 may be NULL.  A context without PQA_FEAT_INTEGRITY returns all-NaN ext5 rows. */
PQA_API int pqa_collect_ext5(pqa_ctx* ctx, int64_t first_index, int32_t count, double* records, double* ext, double* ext2,
                             double* ext3, double* ext4, double* ext5);

/* Wait for all submitted work without collecting. */
PQA_API int pqa_sync(pqa_ctx* ctx);

/* Thread-safe: makes every later (and the current, between batches) submit/collect return
 * PQA_ECANCELLED.  Mirrors VMAFAnalyzer.terminate_analysis (app/vmaf_analyzer.py:139-151). */
PQA_API int pqa_cancel(pqa_ctx* ctx);

/* Clear the cancel flag and the motion / xpsnr / siti / integrity continuity state (start of a new clip). */
PQA_API int pqa_reset(pqa_ctx* ctx);

/* Text of the most recent failure on this context (ctx == NULL: last pqa_create failure). */
PQA_API const char* pqa_last_error(const pqa_ctx* ctx);

/* Per-frame luma statistics of a device-resident clip: out[n_frames][3] (host) = {sum, sum of squares,
 * count(sample > threshold)}, exact integers.  mean / std / white-pixel ratio follow in float64 on the host.
 * Replaces the cv2 loops np.mean(gray) / np.std(gray) / np.sum(gray > threshold) of the reference's white
 * bookend-frame detection (app/bookend_alignment.py:796-800, 902-904, 998-1020; app/reference_analyzer.py:
 * 127-144) -- the step that runs right before analyze_videos.  n_frames <= max_batch per call is NOT required
 * (the call loops).  Synchronous. */
PQA_API int pqa_luma_stats_device(pqa_ctx* ctx, const void* luma, int64_t row_pitch, int64_t frame_pitch,
                                  int32_t n_frames, uint32_t threshold, uint64_t* out);

/* The same statistics for frames in HOST memory: luma_frames[i] points at frame i's luma plane (rows row_stride bytes
 * apart; the frames need not be contiguous -- a detector samples every k-th frame of a memory-mapped clip).  Frames
 * are packed into pinned staging and uploaded in chunks while the previous chunk's kernel runs.  out[n_frames][3] as
 * above.  This is what pqa2_amd.bookend.detect() drives.  Synchronous. */
PQA_API int pqa_luma_stats(pqa_ctx* ctx, const void* const* luma_frames, int64_t row_stride, int32_t n_frames,
                           uint32_t threshold, uint64_t* out);

/* Temporal alignment: the banded cross-frame SSE of two clips, synchronously.
 *     D[i][c] = sum over luma pixels of (ref_i - dis_{i+k})^2,  k = k_lo + c,  0 <= i < n_ref,  0 <= c <= k_hi - k_lo
 *     D[i][c] = UINT64_MAX where i + k is outside [0, n_dis)
 * Exact uint64 sums; k > 0 means the capture is late (captured frame i + k shows reference frame i).  out (host) is
 * [n_ref][k_hi - k_lo + 1].  Any context: its width, height and bit depth (8, 10, 12) are used, no feature bit is needed,
 * device buffers are allocated on first use.  Independent of the scoring chain: a call between two pqa_submit calls changes
 * no record.  PQA_EINVAL on a null pointer, a negative frame count, k_lo > k_hi, a span above 129 or |k| > 64 (checked
 * before any device call); n_ref == 0 succeeds and writes nothing.  8-bit clips run on the i8 matrix cores, deeper ones (and
 * 8-bit ones with PQA_XSSE_MFMA=0 in the environment at pqa_create) on plain integer VALU code: the same integers.
 * pqa2_amd/align.py turns D into an offset and a frame map; definition, tiling and overflow rule: DESIGN.md section 5.
 *
 * pqa_cross_sse_device: both clips in device memory (frame f at luma + f * frame_pitch, rows row_pitch BYTES apart), under
 * the ordering contract of pqa_submit_device. */
PQA_API int pqa_cross_sse_device(pqa_ctx* ctx, const void* ref_luma, int64_t ref_row_pitch, int64_t ref_frame_pitch,
                                 int32_t n_ref, const void* dis_luma, int64_t dis_row_pitch, int64_t dis_frame_pitch,
                                 int32_t n_dis, int32_t k_lo, int32_t k_hi, uint64_t* out);

/* The same for frames in HOST memory: ref_frames[i] / dis_frames[j] point at luma planes (rows *_row_stride bytes apart; the
 * frames need not be contiguous, as for pqa_luma_stats).  Frames go through the pinned staging of pqa_luma_stats, and the
 * band is walked one 32-frame reference tile at a time over a device window of 31 + span captured frames, so every frame
 * is uploaded once, whatever the span. */
PQA_API int pqa_cross_sse(pqa_ctx* ctx, const void* const* ref_frames, int64_t ref_row_stride, int32_t n_ref,
                          const void* const* dis_frames, int64_t dis_row_stride, int32_t n_dis, int32_t k_lo, int32_t k_hi,
                          uint64_t* out);

/* Spatial alignment: the shifted-window luma SSE of n_frames frame pairs, synchronously.  For a search radius R = radius,
 * 0 <= R <= 16, on frames with W > 2R and H > 2R:
 *     S[f][j][i] = sum_{y=R}^{H-R-1} sum_{x=R}^{W-R-1} (ref_f[y][x] - dis_f[y + dy][x + dx])^2,  dy = j - R,  dx = i - R
 * Exact uint64 sums; the summed reference window is the same for every shift, so all entries count (W - 2R)(H - 2R) pixels.
 * dx > 0 means the captured picture is displaced to the right, dy > 0 down.  out (host) is [n_frames][2R + 1][2R + 1]; frame
 * f pairs reference frame f with captured frame f.  Any context: its width, height and bit depth (8, 10, 12) are used, no
 * feature bit is needed, device buffers are allocated on first use, grow only and are freed with the context.  Independent
 * of the scoring chain: a call between two pqa_submit calls changes no record.  PQA_EINVAL on a null pointer, a negative
 * frame count, a radius outside 0 ... 16 or a frame not larger than 2R in either direction (checked before any device call);
 * n_frames == 0 succeeds and writes nothing.  pqa2_amd/align.py (best_shift) turns S into a shift; definition, tiling and
 * overflow rule: DESIGN.md section 5.
 *
 * pqa_shift_sse_device: both clips in device memory (frame f at luma + f * frame_pitch, rows row_pitch BYTES apart), under
 * the ordering contract of pqa_submit_device. */
PQA_API int pqa_shift_sse_device(pqa_ctx* ctx, const void* ref_luma, int64_t ref_row_pitch, int64_t ref_frame_pitch,
                                 const void* dis_luma, int64_t dis_row_pitch, int64_t dis_frame_pitch, int32_t n_frames,
                                 int32_t radius, uint64_t* out);

/* The same for frames in HOST memory: ref_frames[f] / dis_frames[f] point at luma planes (rows *_row_stride bytes apart; the
 * frames need not be contiguous, as for pqa_luma_stats).  Frames go through the pinned staging of pqa_luma_stats in chunks
 * of 8 pairs. */
PQA_API int pqa_shift_sse(pqa_ctx* ctx, const void* const* ref_frames, int64_t ref_row_stride, const void* const* dis_frames,
                          int64_t dis_row_stride, int32_t n_frames, int32_t radius, uint64_t* out);

/* Level alignment: the per-level transfer table of n_frames frame pairs of one plane, synchronously.  With L =
 * pqa_level_bins(ctx) = 2^bit_depth and v = 0 ... L - 1:
 *     T[f][v][0] = number of pixels of pair f with ref == v
 *     T[f][v][1] = sum of dis over those pixels          T[f][v][2] = sum of dis^2 over those pixels
 * Exact uint64.  A reference sample above L - 1 (a 16-bit container can hold one) is counted in bin L - 1; its captured
 * partner enters the sums as it is.  out (host) is [n_frames][L][3].  plane 0 / 1 / 2 selects the context's luma or chroma
 * plane size (chroma from chroma_shift).  Any context, no feature bit; the device table is allocated on first use, grows only
 * and is freed with the context.  Independent of the scoring chain: a call between two pqa_submit calls changes no record.
 * PQA_EINVAL on a null pointer, a negative frame count, plane < 0 or plane >= n_planes (checked before any device call);
 * n_frames == 0 succeeds and writes nothing.  pqa2_amd/align.py (best_levels, level_lut) turns T into a gain / offset and
 * a correction table; kernel and accumulator bounds: DESIGN.md section 5.
 *
 * pqa_level_stats_device: both clips in device memory (frame f at base + f * frame_pitch, rows row_pitch BYTES apart), under
 * the ordering contract of pqa_submit_device. */
PQA_API int pqa_level_stats_device(pqa_ctx* ctx, const void* ref, int64_t ref_row_pitch, int64_t ref_frame_pitch,
                                   const void* dis, int64_t dis_row_pitch, int64_t dis_frame_pitch, int32_t n_frames,
                                   int32_t plane, uint64_t* out);

/* The same for frames in HOST memory: ref_frames[f] / dis_frames[f] point at planes of the selected size (rows *_row_stride
 * bytes apart; the frames need not be contiguous).  Frames go through the pinned staging of pqa_luma_stats in chunks of 8
 * pairs. */
PQA_API int pqa_level_stats(pqa_ctx* ctx, const void* const* ref_frames, int64_t ref_row_stride, const void* const* dis_frames,
                            int64_t dis_row_stride, int32_t n_frames, int32_t plane, uint64_t* out);

/* L, the number of levels of the table above: 2^bit_depth of the context. */
PQA_API int pqa_level_bins(const pqa_ctx* ctx);

/* Resampling: n_frames planes of src_width x src_height samples become planes of dst_width x dst_height, synchronously, with
 * one separable polyphase filter in exact integers -- what scoring a clip against a reference of another size needs first.
 * Samples are u8 in an 8-bit context, otherwise little-endian u16 of the context's bit depth b (a sample above 2^b - 1 is
 * read as 2^b - 1).  The plane sizes are those of the spec, independent of the context's width and height (each 1 ... 8192):
 * a chroma plane is resampled as a plane of its own size.  The source window (x0, y0, w, h), in source samples as signed
 * Q16 integers, is what the destination plane shows: a whole-plane resize is (0, 0, src_width, src_height); a sub-pixel
 * shift is dst = src size, (w, h) = the size, (x0, y0) = the shift.  Per axis (n_src -> n_dst, window x0, ext), in double:
 *     step = ext / n_dst, stretch = max(1, step), S = s * stretch, centre of destination sample i: c = x0 + (i + 0.5) step - 0.5,
 *     taps j = ceil(c - S) ... floor(c + S) with the weights k((j - c) / stretch), normalised to sum 1,
 *     q = floor(w * 16384 + 0.5), the remainder 16384 - sum q added to the largest q (the first of equals),
 *     every tap folded onto clamp(j, 0, n_src - 1) (edge replication).
 * k and s: PQA_RESAMPLE_BILINEAR max(0, 1 - |t|), 1; PQA_RESAMPLE_BICUBIC Keys' cubic with a = -0.6, 2;
 * PQA_RESAMPLE_LANCZOS3 sinc(t) sinc(t / 3), 3.  The horizontal pass runs first: acc = sum q_h * src (int32),
 * mid = (acc + 2^(b-1)) >> b (signed, not clamped), acc2 = sum q_v * mid, out = clamp((acc2 + 2^(27-b)) >> (28 - b), 0, 2^b - 1);
 * all shifts arithmetic.  Identity returns the source; a whole-sample window returns the edge-replicated crop; a constant
 * plane stays constant.  Coefficient quantisation and the intermediate rounding are this library's own, not swscale's.
 * Any context, no feature bit; tables and buffers are made on first use, grow only, are kept for the last four (filter,
 * geometry, window) and freed with the context.  Independent of the scoring chain: a call between two pqa_submit calls
 * changes no record.  PQA_EINVAL, before any device call, on a null pointer, a bad struct_size or filter, a size outside
 * 1 ... 8192, a non-positive window, a row pitch shorter than a row (or, in device memory, no multiple of the sample size),
 * a negative frame count, or a destination sample that needs more than 32 taps (Lanczos beyond 5.3x down, bicubic beyond
 * 8x down).  n_frames == 0 succeeds and writes nothing.  Bytes between the end of a destination row and the next row are
 * never written.  Kernel, tiling and overflow bounds: DESIGN.md section 5.
 *
 * pqa_resample: frames in HOST memory (src_frames[f] / dst_frames[f] point at planes, rows *_row_stride bytes apart; the
 * frames need not be contiguous).  They travel in chunks of 8 through pinned buffers of this entry's own.
 * pqa_resample_device: both clips in device memory (frame f at base + f * frame_pitch, rows row_pitch BYTES apart), under
 * the ordering contract of pqa_submit_device; the resampled planes can go straight into pqa_submit_device. */
enum { PQA_RESAMPLE_BILINEAR = 0, PQA_RESAMPLE_BICUBIC = 1, PQA_RESAMPLE_LANCZOS3 = 2 };
typedef struct pqa_resample_spec {
  uint32_t struct_size, filter;
  uint32_t src_width, src_height, dst_width, dst_height; /* of THIS plane, 1 ... 8192 */
  int64_t x0_q16, y0_q16, w_q16, h_q16;                  /* source window; w, h > 0 */
} pqa_resample_spec;
PQA_API int pqa_resample(pqa_ctx* ctx, const pqa_resample_spec* spec, const void* const* src_frames, int64_t src_row_stride,
                         void* const* dst_frames, int64_t dst_row_stride, int32_t n_frames);
PQA_API int pqa_resample_device(pqa_ctx* ctx, const pqa_resample_spec* spec, const void* src, int64_t src_row_pitch,
                                int64_t src_frame_pitch, void* dst, int64_t dst_row_pitch, int64_t dst_frame_pitch,
                                int32_t n_frames);

/* Packed capture frames -> planes, synchronously: n_frames frames of width x height in one of the packed formats above
 * (PQA_SURFACE_UYVY / _YUYV / _V210) become a Y plane of width x height and U, V planes of ceil(width / 2) x height samples
 * (u8; v210: LSB-aligned u16).  The planes are the same integers a planar file of the clip holds, so there is nothing to
 * pin.  Any context, no feature bit; the size and the sample format are the call's own (each size 1 ... 8192), independent
 * of the context's.  This is how the side analyses of resident clips, pqa_resample or pqa_submit_device get planes from a
 * packed capture.  No source row is read beyond the format's minimum row bytes and no destination row is written beyond
 * its samples.  PQA_EINVAL, before any device call, on a null spec, a bad struct_size or format, a size outside 1 ... 8192,
 * a negative frame count, a null source or luma destination, a row pitch below a row, a v210 base / pitch that is not a
 * multiple of 4, or a destination that is not made of whole samples.  n_frames == 0 succeeds and writes nothing.
 *
 * pqa_unpack_device: both clips in device memory under the ordering contract of pqa_submit_device; the planes of dst are
 * WRITTEN (its pointers are const only because the struct is shared).  dst->plane[1] and dst->plane[2] both NULL: luma only,
 * no chroma is decoded.
 * pqa_unpack: frames in HOST memory (src_frames[f]: a packed frame, rows src_row_stride bytes apart; dst_planes[f * 3 + p]:
 * plane p of frame f, rows dst_strides[p] bytes apart; dst_planes[f * 3 + 1] and [f * 3 + 2] NULL in frame 0: luma only).
 * They travel in chunks of 8 through the pinned buffers of pqa_resample and device buffers of this entry's own. */
typedef struct pqa_unpack_spec {
  uint32_t struct_size, format; /* sizeof(pqa_unpack_spec); PQA_SURFACE_UYVY / _YUYV / _V210 */
  uint32_t width, height;       /* of the luma plane, 1 ... 8192 */
} pqa_unpack_spec;
PQA_API int pqa_unpack_device(pqa_ctx* ctx, const pqa_unpack_spec* spec, const void* src, int64_t src_row_pitch,
                              int64_t src_frame_pitch, int32_t n_frames, const pqa_device_clip* dst);
PQA_API int pqa_unpack(pqa_ctx* ctx, const pqa_unpack_spec* spec, const void* const* src_frames, int64_t src_row_stride,
                       int32_t n_frames, void* const* dst_planes, const int64_t dst_strides[3]);

/* Pixel-format conversion, synchronously: n_frames planes of ONE kind (luma, or a chroma plane) change their chroma layout,
 * chroma siting and sample depth in one pass with one rounding -- what scoring a 4:2:2 capture (uyvy422, yuyv422, v210) against
 * a yuv420p master needs first, where ffmpeg would insert swscale.  The plane belongs to a frame of luma_width x luma_height
 * (each 1 ... 8192).  A layout is (hshift, vshift), each 0 ... 2 (the nine the library accepts); a luma plane is 0, 0 -> 0, 0.
 * A plane has ceil(luma >> shift) samples along an axis.  Siting per axis and side: PQA_SITE_COSITED or PQA_SITE_CENTRE,
 * ignored where the shift is 0.  src_bits, dst_bits: 8, 10 or 12; samples are u8 at 8 bit, otherwise little-endian u16; a
 * source sample above 2^src_bits - 1 is read as 2^src_bits - 1.
 * Per axis, positions in HALF luma samples, F = 1 << shift: sample k of a plane sits at P(k) = 2 F k + (centre ? F - 1 : 0);
 * W = max(F_src, F_dst); destination sample i takes every source sample j with the weight w = 2 W - |P_src(j) - P_dst(i)| where
 * that is positive (a triangle of half-width W luma samples), j folded onto clamp(j, 0, n_src - 1) (edge replication).  The
 * weights of a destination sample sum to S = 2 W^2 / F_src, a power of two of at most 32, over at most 8 taps.  4:2:2 -> 4:2:0
 * vertically centred: [1 3 3 1] / 8 at rows 2i - 1 ... 2i + 2, co-sited [1 2 1] / 4; 4:2:0 centred -> 4:2:2: [3 1] / 4 and
 * [1 3] / 4 alternating; identity [2] / 2.  Both axes share one rounding, which carries the depth change:
 *     acc = sum_y sum_x w_y w_x s (at most 1024 * 4095, int32), t = log2(S_x S_y), d = dst_bits - src_bits,
 *     t > d: out = min((acc + 2^(t-d-1)) >> (t - d), 2^dst_bits - 1); otherwise out = acc << (d - t).
 * Identity returns the source; a constant plane c becomes c << d (d < 0: min((c + 2^(-d-1)) >> -d, max)); a plane linear in
 * the luma position stays linear in the interior; 10 -> 8 bit of 1023 gives 255.  Triangle and rounding are this library's
 * own, not swscale's; the distance to swscale is not pinned.  PQA_CONVERT_GENERIC in flags: the general kernel whatever the
 * layout (the test partner of the fast paths; the same integers).
 * Any context, no feature bit, no record, no profile id; sizes and sample formats are the call's own, independent of the
 * context's and of the scoring chain: a call between two pqa_submit calls changes no record.  PQA_EINVAL, before any device
 * call, on a null pointer, a bad struct_size, unknown flag bits, a bad depth, shift or site value, a size outside 1 ... 8192,
 * a negative frame count, a row pitch below a row or, in device memory, a base or pitch that is no multiple of the sample
 * size.  n_frames == 0 succeeds and writes nothing.  No source row is read beyond its samples and no destination byte beyond
 * a row's samples is written.  Kernel and fast paths: DESIGN.md section 5.
 *
 * pqa_format_convert: frames in HOST memory (src_frames[f] / dst_frames[f] point at planes, rows *_row_stride bytes apart; the
 * frames need not be contiguous).  They travel in chunks of 8 through the pinned buffers of pqa_resample and device buffers
 * of this entry's own, grow-only and freed with the context.
 * pqa_format_convert_device: both clips in device memory (frame f at base + f * frame_pitch, rows row_pitch BYTES apart), under
 * the ordering contract of pqa_submit_device; the converted planes can go straight into pqa_submit_device. */
enum { PQA_SITE_COSITED = 0, PQA_SITE_CENTRE = 1 };
enum { PQA_CONVERT_GENERIC = 1 }; /* flags: the general path whatever the layout (test partner; same integers) */
typedef struct pqa_convert_spec {
  uint32_t struct_size, flags;
  uint32_t src_bits, dst_bits;                            /* 8, 10, 12 */
  uint32_t luma_width, luma_height;                       /* of the frame the plane belongs to, 1 ... 8192 */
  uint8_t src_hshift, src_vshift, dst_hshift, dst_vshift; /* 0 ... 2 */
  uint8_t src_hsite, src_vsite, dst_hsite, dst_vsite;     /* PQA_SITE_* */
} pqa_convert_spec;
PQA_API int pqa_format_convert(pqa_ctx* ctx, const pqa_convert_spec* spec, const void* const* src_frames, int64_t src_row_stride,
                               void* const* dst_frames, int64_t dst_row_stride, int32_t n_frames);
PQA_API int pqa_format_convert_device(pqa_ctx* ctx, const pqa_convert_spec* spec, const void* src, int64_t src_row_pitch,
                                      int64_t src_frame_pitch, void* dst, int64_t dst_row_pitch, int64_t dst_frame_pitch,
                                      int32_t n_frames);

/* Packed RGB frames -> Y'CbCr planes, synchronously: n_frames frames of width x height pixels in one of the packed RGB formats
 * above become a Y plane of width x height and U, V planes of ceil(width >> hshift) x ceil(height >> vshift) samples (u8 at
 * dst_bits 8, LSB-aligned little-endian u16 at 10) -- unpack, colour matrix, range, depth, chroma subsampling and siting in one
 * pass with ONE rounding, where ffmpeg would insert swscale.  Integers only:
 *   m[3][4] (m[4 c + k]) is Q14, column 0 the offset in Q14 units, columns 1-3 multiply R, G, B (pqa_colour_apply's layout).
 *   A_c(x, y) = m[c][0] + m[c][1] R + m[c][2] G + m[c][3] B                                      (exact, no rounding)
 *   Y(x, y)   = clamp((A_0 + 2^13) >> 14, 0, 2^dst_bits - 1)                                    (>> arithmetic, i.e. floor)
 *   C_c       = clamp((My A_c Mx^T + 2^(t-1)) >> t, 0, 2^dst_bits - 1), c = 1, 2, t = 14 + log2(Sx Sy)
 * where Mx, My are the tap matrices pqa_format_convert applies to a 4:4:4 plane (source shift 0, edge replication folded in):
 * an axis of shift 0 is the identity (S = 1); an axis of shift 1 is [1 2 1] / 4 around luma sample 2i (PQA_SITE_COSITED; as
 * [2 4 2] / 8) or [1 3 3 1] / 8 on the luma samples 2i - 1 ... 2i + 2 (PQA_SITE_CENTRE), S = 8.  Taps-then-matrix and
 * matrix-then-taps are the same integers.  4:2:0 "left" is hsite COSITED, vsite CENTRE.
 * Bound: a call is valid only if, for every row c, the extreme of |A_c| over the source cube [0, 2^sb - 1]^3 (sb = 8, r210: 10),
 * times Sx Sy, plus the rounding half 2^(t-1), stays below 2^31 -- this is what lets the kernel work in int32.  Every matrix of
 * pqa2_amd.rgb.conversion_matrix meets it at dst_bits 8 and 10; 12-bit destinations are not accepted.
 * Coefficients and taps are this library's own, not swscale's; the distance to swscale is not pinned.  PQA_RGB_GENERIC in
 * flags: the general kernel whatever the layout (the test partner of the fast paths 4:4:4, 4:2:2 co-sited and 4:2:0 left; the
 * same integers).
 * Any context, no feature bit, no record; the size is the call's own, independent of the context's: a call between two
 * pqa_submit calls changes no record.  PQA_EINVAL, before any device call, on a null pointer, a bad struct_size, a format that
 * is not a packed RGB format, unknown flag bits, a dst_bits other than 8 or 10, a shift above 1, a bad site value, a size outside
 * 1 ... 8192, a negative frame count, a source pitch below 4 * width, an r210 base or pitch that is not a multiple of 4, a
 * destination that is not made of whole samples or whose pitch is below a row, chroma destinations given as one of two, or a
 * matrix beyond the bound.  n_frames == 0 succeeds and writes nothing.
 *
 * pqa_rgb_convert_device: both clips in device memory under the ordering contract of pqa_unpack_device; the planes of dst are
 * WRITTEN (its pointers are const only because the struct is shared).  dst->plane[1] and dst->plane[2] both NULL: luma only, no
 * chroma work at all.
 * pqa_rgb_convert: frames in HOST memory (src_frames[f]: a packed frame, rows src_row_stride bytes apart; dst_planes[f * 3 + p]:
 * plane p of frame f, rows dst_strides[p] bytes apart; dst_planes[1] and [2] NULL in frame 0: luma only).  They travel in chunks
 * of 8 through the pinned buffers of pqa_resample and device buffers of this entry's own. */
enum { PQA_RGB_GENERIC = 1 }; /* flags: the general path whatever the layout (test partner; same integers) */
typedef struct pqa_rgb_spec {
  uint32_t struct_size, format;          /* sizeof(pqa_rgb_spec); PQA_SURFACE_BGRA ... _R210 */
  uint32_t width, height;                /* 1 ... 8192 */
  uint32_t dst_bits;                     /* 8 or 10 */
  uint32_t hshift, vshift, hsite, vsite; /* destination chroma layout; shifts 0 / 1, PQA_SITE_* */
  uint32_t flags;                        /* PQA_RGB_GENERIC */
  int32_t m[12];                         /* Q14, column 0 the offset */
} pqa_rgb_spec;
PQA_API int pqa_rgb_convert_device(pqa_ctx* ctx, const pqa_rgb_spec* spec, const void* src, int64_t src_row_pitch,
                                   int64_t src_frame_pitch, int32_t n_frames, const pqa_device_clip* dst);
PQA_API int pqa_rgb_convert(pqa_ctx* ctx, const pqa_rgb_spec* spec, const void* const* src_frames, int64_t src_row_stride,
                            int32_t n_frames, void* const* dst_planes, const int64_t dst_strides[3]);

/* Transfer-curve alignment: n_frames planes through an integer table, synchronously -- the correction that undoes a gamma
 * mismatch, a contrast enhancer or a black-stretch curve once pqa2_amd/align.py (best_curve, curve_lut) has turned the table
 * of pqa_level_stats into a monotone curve and its inverse.  Planes of width x height samples (the spec's, independent of the
 * context's width and height; each 1 ... 8192), u8 in an 8-bit context, otherwise little-endian u16.  table: a HOST pointer to
 * L = pqa_level_bins(ctx) entries of the sample type, none above 2^bit_depth - 1, and
 *     dst[y][x] = table[min(src[y][x], L - 1)].
 * Any table, monotone or not.  The destination may be exactly the source (same base and pitches).
 * Any context, no feature bit, no record, no profile id; independent of the scoring chain: a call between two pqa_submit
 * calls changes no record.  PQA_EINVAL, before any device call, on a null pointer, a bad struct_size, a size outside
 * 1 ... 8192, a negative frame count, a row pitch below a row, in device memory a base or pitch that is no multiple of the
 * sample size, or a table entry above 2^bit_depth - 1.  n_frames == 0 succeeds and writes nothing.  No source byte past a
 * row's last sample is read and no destination byte past it is written.  Kernel: DESIGN.md section 5.
 *
 * pqa_table_apply: frames in HOST memory (src_frames[f] / dst_frames[f] point at planes, rows *_row_stride bytes apart; the
 * frames need not be contiguous).  They travel in chunks of 8 through the pinned buffers of pqa_resample and device buffers
 * of this entry's own, grow-only and freed with the context.
 * pqa_table_apply_device: both clips in device memory (frame f at base + f * frame_pitch, rows row_pitch BYTES apart), under
 * the ordering contract of pqa_submit_device; the mapped planes can go straight into pqa_submit_device. */
typedef struct pqa_table_spec {
  uint32_t struct_size;   /* sizeof(pqa_table_spec) */
  uint32_t width, height; /* of this plane, 1 ... 8192 */
} pqa_table_spec;
PQA_API int pqa_table_apply(pqa_ctx* ctx, const pqa_table_spec* spec, const void* table, const void* const* src_frames,
                            int64_t src_row_stride, void* const* dst_frames, int64_t dst_row_stride, int32_t n_frames);
PQA_API int pqa_table_apply_device(pqa_ctx* ctx, const pqa_table_spec* spec, const void* table, const void* src, int64_t src_row_pitch,
                                   int64_t src_frame_pitch, void* dst, int64_t dst_row_pitch, int64_t dst_frame_pitch,
                                   int32_t n_frames);

/* Deinterlacing: the planes of an interlaced clip to progressive ones, synchronously, in exact integers -- what lets a capture
 * that really is interlaced (1080i: two moments in time a frame) be scored against a progressive master.  One field of a source
 * frame is kept and the other interpolated: from the kept field alone (mode 0, intra) or motion-adaptively from the fields before
 * and after it (mode 1, adaptive; the w3fdif taps inside yadif's temporal clamp that FFmpeg ships as bwdif -- the arithmetic as
 * this library states it heads pqa2_amd/csrc/deinterlace.hip and is restated in tests/deinterlace_ref.py; parity with FFmpeg is
 * not pinned).  first: the parity of the rows whose field comes first in time.  rate 0 (frame): output t keeps the field `first`
 * of source frame t; rate 1 (field): outputs 2 t and 2 t + 1 keep the fields first and 1 - first of source frame t.  A source
 * frame before the first is the first and one after the last is the last.  Planes of width x height samples (the spec's,
 * independent of the context's), u8 in an 8-bit context, otherwise little-endian u16; a sample above 2^bit_depth - 1 is read as
 * that.  n_frames counts SOURCE frames; dst holds n_frames or 2 n_frames planes.
 * Any context, no feature bit, no record, no profile id; independent of the scoring chain: a call between two pqa_submit
 * calls changes no record.  PQA_EINVAL, before any device call, on a null pointer, a bad struct_size, a mode, first or rate
 * above 1, a width outside 1 ... 8192 or a height outside 2 ... 8192, a negative frame count, a row pitch that is negative or
 * below a row, a base or pitch that is no multiple of the sample size, or a destination that is the source (there is no in-place
 * form).  n_frames == 0 succeeds and writes nothing.  No source byte past a row's last sample is read and no destination byte
 * past it is written.  Kernel: DESIGN.md section 5.
 *
 * pqa_deinterlace: frames in HOST memory (src_frames[f] / dst_frames[k] point at planes, rows *_row_stride bytes apart).  Every
 * source frame crosses PCIe once: the frames travel in chunks of 8 and the last two of a chunk stay in device memory as the
 * predecessors of the next.
 * pqa_deinterlace_device: both clips in device memory (frame f at base + f * frame_pitch, rows row_pitch BYTES apart), under
 * the ordering contract of pqa_submit_device. */
typedef struct pqa_deint_spec {
  uint32_t struct_size;   /* sizeof(pqa_deint_spec) */
  uint32_t width, height; /* of this plane: width 1 ... 8192, height 2 ... 8192 */
  uint32_t mode;          /* 0 intra, 1 adaptive */
  uint32_t first;         /* 0 top field first, 1 bottom field first */
  uint32_t rate;          /* 0 frame: n_frames outputs, 1 field: 2 n_frames outputs */
} pqa_deint_spec;
PQA_API int pqa_deinterlace(pqa_ctx* ctx, const pqa_deint_spec* spec, const void* const* src_frames, int64_t src_row_stride,
                            void* const* dst_frames, int64_t dst_row_stride, int32_t n_frames);
PQA_API int pqa_deinterlace_device(pqa_ctx* ctx, const pqa_deint_spec* spec, const void* src, int64_t src_row_pitch,
                                   int64_t src_frame_pitch, void* dst, int64_t dst_row_pitch, int64_t dst_frame_pitch,
                                   int32_t n_frames);
/* what the binding states of the kernel: source frames a launch, bytes of a row and rows of a workgroup's block */
PQA_API int pqa_deint_chunk(void);
PQA_API int pqa_deint_block_bytes(void);
PQA_API int pqa_deint_block_rows(void);

/* Overlay masking: n_frames planes of one clip through a feathered mask, synchronously, in exact integers -- the correction that
 * takes a burnt-in overlay (a channel logo, a clock, a timecode, an OSD) out of the scores once pqa2_amd/distortion.py
 * (persistent_regions, overlay_mask) has found it: both clips are blended towards one flat value there, or the captured clip
 * towards the reference's own samples.  Planes of width x height samples (the spec's, independent of the context's width and
 * height; each 1 ... 8192), u8 in an 8-bit context, otherwise little-endian u16.
 * nodes: a HOST pointer to a grid A[gy][gx] of uint16, each 0 ... 256, whose nodes lie Gx = 1 << step_log2_x and
 * Gy = 1 << step_log2_y samples apart (steps 0 ... 6, the call's own, so that luma at step 3 and 4:2:0 chroma at step 2 share
 * one grid): gx = ((width + Gx - 1) >> step_log2_x) + 1 columns, gy rows likewise.  For sample (x, y), i = x >> step_log2_x,
 * fx = x & (Gx - 1), j = y >> step_log2_y, fy = y & (Gy - 1):
 *     a   = (A[j][i] (Gx - fx)(Gy - fy) + A[j][i+1] fx (Gy - fy) + A[j+1][i] (Gx - fx) fy + A[j+1][i+1] fx fy
 *            + ((Gx Gy) >> 1)) >> (step_log2_x + step_log2_y)
 *     dst = (src (256 - a) + fill a + 128) >> 8
 * fill: the spec's constant (at most 2^bit_depth - 1), or with a fill plane the sample of that plane at (x, y); the fill plane
 * has the geometry of src and a base and pitches of its own.  a = 0 returns src exactly, a = 256 returns fill exactly.  u16:
 * where a > 0 a source sample above 2^bit_depth - 1 is read as 2^bit_depth - 1, and so is every fill sample; where a = 0 the
 * source sample is copied as it is.
 * The destination may be exactly the source (same base and pitches): then only the bounding rectangle of the samples with
 * a > 0 is read and written.  Otherwise the whole plane is written.  The destination may not be the fill plane.
 * Any context, no feature bit, no record, no profile id; independent of the scoring chain: a call between two pqa_submit
 * calls changes no record.  PQA_EINVAL, before any device call, on a null pointer, a bad struct_size, a size outside
 * 1 ... 8192, a step above 6, a node above 256, a fill above 2^bit_depth - 1, a negative frame count, a row pitch below a
 * row, in device memory a base or pitch that is no multiple of the sample size, or a destination equal to the fill plane.
 * n_frames == 0 succeeds and writes nothing.  No source byte past a row's last sample is read and no destination byte past it
 * is written.  Kernel: DESIGN.md section 5.
 *
 * pqa_mask_blend: frames in HOST memory (src_frames[f] / fill_frames[f] / dst_frames[f] point at planes, rows *_row_stride
 * bytes apart; fill_frames null: the constant).  They travel in chunks of 8 through the pinned buffers of pqa_resample and
 * device buffers of this entry's own, grow-only and freed with the context.
 * pqa_mask_blend_device: the clips in device memory (frame f at base + f * frame_pitch, rows row_pitch BYTES apart; fill null:
 * the constant), under the ordering contract of pqa_submit_device; the blended planes can go straight into pqa_submit_device. */
typedef struct pqa_mask_spec {
  uint32_t struct_size;              /* sizeof(pqa_mask_spec) */
  uint32_t width, height;            /* of this plane, 1 ... 8192 */
  uint32_t step_log2_x, step_log2_y; /* 0 ... 6 */
  uint32_t fill;                     /* the constant fill, at most 2^bit_depth - 1 (checked with a fill plane too, then unused) */
} pqa_mask_spec;
PQA_API int pqa_mask_blend(pqa_ctx* ctx, const pqa_mask_spec* spec, const uint16_t* nodes, const void* const* src_frames,
                           int64_t src_row_stride, const void* const* fill_frames, int64_t fill_row_stride, void* const* dst_frames,
                           int64_t dst_row_stride, int32_t n_frames);
PQA_API int pqa_mask_blend_device(pqa_ctx* ctx, const pqa_mask_spec* spec, const uint16_t* nodes, const void* src, int64_t src_row_pitch,
                                  int64_t src_frame_pitch, const void* fill, int64_t fill_row_pitch, int64_t fill_frame_pitch, void* dst,
                                  int64_t dst_row_pitch, int64_t dst_frame_pitch, int32_t n_frames);

/* Sub-pixel registration: the tile-wise gradient moments of n_frames frame pairs of one plane, synchronously -- the
 * Lucas-Kanade normal equations of every tile, from which pqa2_amd/align.py (solve_geometry, register) estimates a sub-pixel
 * shift and a scale factor per axis and drives the source window of pqa_resample.  Planes of width x height samples (the
 * spec's, independent of the context's width and height; each 3 ... 8192), u8 in an 8-bit context, otherwise u16 of the
 * context's bit depth b (a sample above 2^b - 1 is read as 2^b - 1).  With r = ref, d = dis, a = r + d, e = d - r, at every
 * pixel 1 <= x <= W - 2, 1 <= y <= H - 2:
 *     gx = (a[y-1][x+1] + 2 a[y][x+1] + a[y+1][x+1]) - (a[y-1][x-1] + 2 a[y][x-1] + a[y+1][x-1])
 *     gy = (a[y+1][x-1] + 2 a[y+1][x] + a[y+1][x+1]) - (a[y-1][x-1] + 2 a[y-1][x] + a[y-1][x+1])
 *     dt = sum_{j,i in -1..1} w_j w_i e[y+j][x+i],  w = (1, 2, 1)
 * Tile (i, j) of size T = tile (8, 16, 32 or 64) owns the counted pixels with x / T = i, y / T = j; the grid is
 * tx = ceil(W / T) by ty = ceil(H / T), and
 *     out[f][j][i][0..5] = sum gx^2, sum gx gy, sum gy^2, sum gx dt, sum gy dt, sum dt^2
 * Exact int64, no floating point anywhere; a tile with no counted pixel is all zeros.  out (host) is [n_frames][ty][tx][6].
 * The signs are those of pqa_shift_sse: a captured picture displaced to the right by dx > 0 gives sum gx dt of the sign of
 * -dx sum gx^2.  Any context, no feature bit; buffers are made on first use, grow only and are freed with the context.
 * Independent of the scoring chain: a call between two pqa_submit calls changes no record.  PQA_EINVAL, before any device
 * call, on a null pointer, a bad struct_size, a tile other than 8 / 16 / 32 / 64, a size outside 3 ... 8192, a row pitch
 * shorter than a row (or, in device memory, a pitch that is no multiple of the sample size), or a negative frame count.
 * n_frames == 0 succeeds and writes nothing.  Kernel and accumulator bounds: DESIGN.md section 5.
 *
 * pqa_flow_moments: frames in HOST memory (ref_frames[f] / dis_frames[f] point at planes, rows *_row_stride bytes apart; the
 * frames need not be contiguous).  They travel in chunks of 8 pairs through the pinned buffers of pqa_resample.
 * pqa_flow_moments_device: both clips in device memory (frame f at base + f * frame_pitch, rows row_pitch BYTES apart), under
 * the ordering contract of pqa_submit_device. */
typedef struct pqa_flow_spec {
  uint32_t struct_size;
  uint32_t width, height; /* of THIS plane, 3 ... 8192 */
  uint32_t tile;          /* 8, 16, 32 or 64 */
} pqa_flow_spec;
PQA_API int pqa_flow_moments(pqa_ctx* ctx, const pqa_flow_spec* spec, const void* const* ref_frames, int64_t ref_row_stride,
                             const void* const* dis_frames, int64_t dis_row_stride, int32_t n_frames, int64_t* out);
PQA_API int pqa_flow_moments_device(pqa_ctx* ctx, const pqa_flow_spec* spec, const void* ref, int64_t ref_row_pitch,
                                    int64_t ref_frame_pitch, const void* dis, int64_t dis_row_pitch, int64_t dis_frame_pitch,
                                    int32_t n_frames, int64_t* out);

/* Active-picture detection: the row and column profiles of n_frames planes of ONE clip, synchronously -- what
 * pqa2_amd/align.py (active_picture, common_window) finds letterbox and pillarbox bars with.  Planes of width x height samples
 * (the spec's, independent of the context's width and height; each 1 ... 8192), u8 in an 8-bit context, otherwise u16 of the
 * context's bit depth b (a sample above 2^b - 1 is read as 2^b - 1):
 *     rows[f][y][0] = sum_x v[y][x]     rows[f][y][1] = sum_x v[y][x]^2
 *     cols[f][x][0] = sum_y v[y][x]     cols[f][x][1] = sum_y v[y][x]^2
 * Exact uint64, no floating point anywhere; every sample is read once for both profiles.  out (host) is
 * [n_frames][height + width][2]: the rows of a frame first, then its columns.  The profile of a window of rows is that of
 * planes whose base pointer and height select the window.  Any context, no feature bit; buffers are made on first use, grow
 * only and are freed with the context.  Independent of the scoring chain: a call between two pqa_submit calls changes no
 * record.  PQA_EINVAL, before any device call, on a null pointer, a bad struct_size, a size outside 1 ... 8192, a row pitch
 * shorter than a row (or, in device memory, a pitch that is no multiple of the sample size), or a negative frame count.
 * n_frames == 0 succeeds and writes nothing.  Kernel and accumulator bounds: DESIGN.md section 5.
 *
 * pqa_line_profiles: frames in HOST memory (frames[f] points at a plane, rows row_stride bytes apart; the frames need not be
 * contiguous).  They travel in chunks of 8 through the first pinned buffer of pqa_resample.
 * pqa_line_profiles_device: the clip in device memory (frame f at planes + f * frame_pitch, rows row_pitch BYTES apart), under
 * the ordering contract of pqa_submit_device. */
typedef struct pqa_profile_spec {
  uint32_t struct_size;
  uint32_t width, height; /* of THIS plane, 1 ... 8192 */
} pqa_profile_spec;
PQA_API int pqa_line_profiles(pqa_ctx* ctx, const pqa_profile_spec* spec, const void* const* frames, int64_t row_stride,
                              int32_t n_frames, uint64_t* out);
PQA_API int pqa_line_profiles_device(pqa_ctx* ctx, const pqa_profile_spec* spec, const void* planes, int64_t row_pitch,
                                     int64_t frame_pitch, int32_t n_frames, uint64_t* out);

/* Distortion map: the tile-wise second-order statistics of n_frames frame pairs of one plane, synchronously -- what
 * pqa2_amd/distortion.py turns into a tile PSNR, a block SSIM, a list of localised defects and of persistent regions (a
 * burnt-in logo or clock).  Planes of width x height samples (the spec's, independent of the context's width and height;
 * each 1 ... 8192), u8 in an 8-bit context, otherwise u16 of the context's bit depth b (a sample above 2^b - 1 is read as
 * 2^b - 1).  With r = ref, d = dis, tile (i, j) of size T = tile (8, 16, 32 or 64) owns the pixels with x / T = i,
 * y / T = j; the grid is tx = ceil(W / T) by ty = ceil(H / T), edge tiles hold the pixels that exist, and
 *     out[f][j][i][0..5] = sum r, sum d, sum r^2, sum d^2, sum r d, sum |d - r|
 * Exact uint64, no floating point anywhere; the squared error of a tile is sum r^2 - 2 sum r d + sum d^2.  out (host) is
 * [n_frames][ty][tx][6].  Any context, no feature bit; buffers are made on first use, grow only and are freed with the
 * context.  Independent of the scoring chain: a call between two pqa_submit calls changes no record.  PQA_EINVAL, before any
 * device call, on a null pointer, a bad struct_size, a tile other than 8 / 16 / 32 / 64, a size outside 1 ... 8192, a row
 * pitch that is negative, shorter than a row or no multiple of the sample size, or a negative frame count.  n_frames == 0
 * succeeds and writes nothing.  Kernel and accumulator bounds: DESIGN.md section 5.
 *
 * pqa_tile_moments: frames in HOST memory (ref_frames[f] / dis_frames[f] point at planes, rows *_row_stride bytes apart; the
 * frames need not be contiguous).  They travel in chunks of 8 pairs through the pinned buffers of pqa_resample.
 * pqa_tile_moments_device: both clips in device memory (frame f at base + f * frame_pitch, rows row_pitch BYTES apart), under
 * the ordering contract of pqa_submit_device. */
typedef struct pqa_tile_spec {
  uint32_t struct_size;
  uint32_t width, height; /* of THIS plane, 1 ... 8192 */
  uint32_t tile;          /* 8, 16, 32 or 64 */
} pqa_tile_spec;
PQA_API int pqa_tile_moments(pqa_ctx* ctx, const pqa_tile_spec* spec, const void* const* ref_frames, int64_t ref_row_stride,
                             const void* const* dis_frames, int64_t dis_row_stride, int32_t n_frames, uint64_t* out);
PQA_API int pqa_tile_moments_device(pqa_ctx* ctx, const pqa_tile_spec* spec, const void* ref, int64_t ref_row_pitch,
                                    int64_t ref_frame_pitch, const void* dis, int64_t dis_row_pitch, int64_t dis_frame_pitch,
                                    int32_t n_frames, uint64_t* out);

/* Distortion spectrum: the second moments of the Haar octave bands of n_frames frame pairs of one plane, synchronously -- what
 * pqa2_amd/spectrum.py turns into a gain, a detail loss and an added noise per octave and orientation: WHAT KIND of difference
 * the clips have, where the distortion map says where.  Planes of width x height samples (the spec's, independent of the
 * context's; each 1 ... 8192), u8 in an 8-bit context, otherwise u16 of the context's bit depth b (a sample above 2^b - 1 is
 * read as 2^b - 1).  A_0 is the plane; for l = 1 ... L = levels (1 ... 6), W_l = floor(W / 2^l), H_l = floor(H / 2^l),
 * 0 <= i < W_l, 0 <= j < H_l and a = A_{l-1}[2j][2i], b = A_{l-1}[2j][2i+1], c = A_{l-1}[2j+1][2i], e = A_{l-1}[2j+1][2i+1]:
 *     A_l = a + b + c + e    H_l = a - b + c - e    V_l = a + b - c - e    D_l = a - b - c + e
 * the unnormalised Haar transform: nothing is divided or rounded, and a coefficient exists only where its whole 2^l x 2^l
 * support lies inside the plane (the last odd row or column of a level is ignored at that level and deeper).  With r_o, d_o
 * the coefficients of the reference and the captured plane,
 *     out[f][l-1][o][0..2] = sum r_o^2, sum d_o^2, sum r_o d_o        o: 0 H, 1 V, 2 D, 3 A
 * over the level's W_l H_l coefficients, exact; the third is an int64 stored in the word as two's complement.  A level with
 * W_l = 0 or H_l = 0 is all zeros.  Every sum is at most (2^b - 1)^2 W H 4^l < 2^62.  out (host) is [n_frames][L][4][3];
 * pqa_band_sums() is 3.  No floating point anywhere.  Any context, no feature bit; buffers are made on first use, grow only and
 * are freed with the context.  Independent of the scoring chain: a call between two pqa_submit calls changes no record.
 * PQA_EINVAL, before any device call, on a null pointer, a bad struct_size, levels outside 1 ... 6, a size outside
 * 1 ... 8192, a row pitch that is negative, shorter than a row or no multiple of the sample size, or a negative frame count.
 * n_frames == 0 succeeds and writes nothing.  Kernel and accumulator bounds: DESIGN.md section 5.
 *
 * pqa_band_moments: frames in HOST memory (ref_frames[f] / dis_frames[f] point at planes, rows *_row_stride bytes apart; the
 * frames need not be contiguous).  They travel in chunks of 8 pairs through the pinned buffers of pqa_resample.
 * pqa_band_moments_device: both clips in device memory (frame f at base + f * frame_pitch, rows row_pitch BYTES apart), under
 * the ordering contract of pqa_submit_device. */
typedef struct pqa_band_spec {
  uint32_t struct_size;
  uint32_t width, height; /* of THIS plane, 1 ... 8192 */
  uint32_t levels;        /* L, 1 ... 6 */
} pqa_band_spec;
PQA_API int pqa_band_moments(pqa_ctx* ctx, const pqa_band_spec* spec, const void* const* ref_frames, int64_t ref_row_stride,
                             const void* const* dis_frames, int64_t dis_row_stride, int32_t n_frames, uint64_t* out);
PQA_API int pqa_band_moments_device(pqa_ctx* ctx, const pqa_band_spec* spec, const void* ref, int64_t ref_row_pitch,
                                    int64_t ref_frame_pitch, const void* dis, int64_t dis_row_pitch, int64_t dis_frame_pitch,
                                    int32_t n_frames, uint64_t* out);
PQA_API int pqa_band_sums(void);

/* Temporal distortion: the tile-wise second-order statistics of the frame DIFFERENCES of n_frames frame pairs of one plane,
 * synchronously -- what pqa2_amd/temporal.py turns into a temporal gain, a blend weight, a temporal loss and noise and a list
 * of pops: whether the MOTION of the captured clip is wrong, where the distortion map and spectrum say whether its pictures
 * are.  Planes of width x height samples (the spec's, independent of the context's width and height; each 1 ... 8192), u8 in an
 * 8-bit context, otherwise u16 of the context's bit depth b (a sample above 2^b - 1 is read as 2^b - 1).  With R_f the
 * reference and D_f the captured plane of frame f, for every transition k = 1 ... n_frames - 1 and every pixel
 *     a = R_k - R_{k-1}    b = D_k - D_{k-1}    e = D_k - R_k        (signed integers)
 * tile (i, j) of size T = tile (8, 16, 32 or 64) owns the pixels with x / T = i, y / T = j; the grid is tx = ceil(W / T) by
 * ty = ceil(H / T), edge tiles hold the pixels that exist, and
 *     out[k-1][j][i][0..6] = sum a, sum b, sum a^2, sum b^2, sum a b, sum a e, sum e^2
 * Exact, no floating point anywhere: words 0, 1, 4 and 5 are int64 stored in the word as two's complement, words 2, 3 and 6
 * uint64; every sum is below 4095^2 * 4096 < 2^36 in magnitude.  out (host) is [max(n_frames - 1, 0)][ty][tx][7];
 * pqa_temporal_sums() is 7.  Any context, no feature bit; buffers are made on first use, grow only and are freed with the
 * context.  Independent of the scoring chain: a call between two pqa_submit calls changes no record.  PQA_EINVAL, before any
 * device call, on a null pointer, a bad struct_size, a tile other than 8 / 16 / 32 / 64, a size outside 1 ... 8192, a row
 * pitch that is negative, shorter than a row or no multiple of the sample size, or a negative frame count.  n_frames of 0 or 1
 * succeeds and writes nothing.  Kernel and accumulator bounds: DESIGN.md section 5.  PQA_TEMPORAL_WALK=1 in the environment at
 * pqa_create selects the kernel's other traversal (a workgroup walks through time; the A/B partner): the same integers.
 *
 * pqa_temporal_moments: frames in HOST memory (ref_frames[f] / dis_frames[f] point at planes, rows *_row_stride bytes apart;
 * the frames need not be contiguous).  They travel in chunks of 8 pairs through the pinned buffers of pqa_resample, every
 * frame once: the last pair of a chunk stays on the device as the predecessor of the next chunk's first.
 * pqa_temporal_moments_device: both clips in device memory (frame f at base + f * frame_pitch, rows row_pitch BYTES apart),
 * under the ordering contract of pqa_submit_device. */
typedef struct pqa_temporal_spec {
  uint32_t struct_size;
  uint32_t width, height; /* of THIS plane, 1 ... 8192 */
  uint32_t tile;          /* 8, 16, 32 or 64 */
} pqa_temporal_spec;
PQA_API int pqa_temporal_moments(pqa_ctx* ctx, const pqa_temporal_spec* spec, const void* const* ref_frames,
                                 int64_t ref_row_stride, const void* const* dis_frames, int64_t dis_row_stride, int32_t n_frames,
                                 uint64_t* out);
PQA_API int pqa_temporal_moments_device(pqa_ctx* ctx, const pqa_temporal_spec* spec, const void* ref, int64_t ref_row_pitch,
                                        int64_t ref_frame_pitch, const void* dis, int64_t dis_row_pitch, int64_t dis_frame_pitch,
                                        int32_t n_frames, uint64_t* out);
PQA_API int pqa_temporal_sums(void);

/* Field alignment: the field-against-field squared errors of n_frames frame pairs of one plane, synchronously -- what
 * pqa2_amd/fields.py turns into the field structure of a capture: a progressive programme carried over an interlaced link
 * comes back with one field taken from the neighbouring frame, with both fields in the wrong line positions, or with one
 * field dropped and the other line-doubled, and a full-reference tool can tell which from exact sums.  Planes of width x
 * height samples (the spec's, independent of the context's width and height; width 1 ... 8192, height 2 ... 8192), u8 in an
 * 8-bit context, otherwise u16 of the context's bit depth b (a sample above 2^b - 1 is read as 2^b - 1).  With R_f the
 * reference and D_f the captured plane of frame f, h2 = floor(height / 2) row pairs (the last row of an odd-height plane is
 * counted nowhere) and
 *     E(A, p, B, q) = sum_{i < h2} sum_{x < width} (A[2 i + p][x] - B[2 i + q][x])^2        p, q in {0, 1}
 * every transition k = 1 ... n_frames - 1 has 14 words:
 *     out[k-1][2 p + q]     = E(D_k, p, R_k, q)        captured field p against reference field q of the same frame
 *     out[k-1][4 + 2 p + q] = E(D_k, p, R_{k-1}, q)    the captured field shows the PREVIOUS reference frame (offset -1)
 *     out[k-1][8 + 2 p + q] = E(D_{k-1}, p, R_k, q)    the previous captured frame's field shows THIS reference frame (offset +1)
 *     out[k-1][12]          = E(D_k, 0, D_k, 1)        comb of the captured frame
 *     out[k-1][13]          = E(R_k, 0, R_k, 1)        comb of the reference frame
 * So captured frame t and parity p have six candidates (q, j), j the reference frame minus the captured frame: j = 0 in record
 * t - 1, word 2 p + q; j = -1 in record t - 1, word 4 + 2 p + q; j = +1 in record t, word 8 + 2 p + q; all six exist for
 * t = 1 ... n_frames - 2.  Exact uint64, no floating point anywhere; every word is below 4096 * 8192 * 4095^2 < 2^50.  out
 * (host) is [max(n_frames - 1, 0)][14].  Any context, no feature bit; buffers are made on first use, grow only and are freed
 * with the context.  Independent of the scoring chain: a call between two pqa_submit calls changes no record.  PQA_EINVAL,
 * before any device call, on a null pointer, a bad struct_size, a height below 2, a size above 8192 or a width of 0, a row
 * pitch that is negative, shorter than a row or no multiple of the sample size, or a negative frame count.  n_frames of 0 or 1
 * succeeds and writes nothing (out may then be null).  Kernel and accumulator bounds: DESIGN.md section 5.
 *
 * pqa_field_moments: frames in HOST memory (ref_frames[f] / dis_frames[f] point at planes, rows *_row_stride bytes apart; the
 * frames need not be contiguous).  They travel in chunks of 8 pairs through the pinned buffers of pqa_resample, every frame
 * once: the last pair of a chunk stays on the device as the predecessor of the next chunk's first.
 * pqa_field_moments_device: both clips in device memory (frame f at base + f * frame_pitch, rows row_pitch BYTES apart),
 * under the ordering contract of pqa_submit_device. */
typedef struct pqa_field_spec {
  uint32_t struct_size;
  uint32_t width, height; /* of THIS plane: width 1 ... 8192, height 2 ... 8192 */
} pqa_field_spec;
PQA_API int pqa_field_moments(pqa_ctx* ctx, const pqa_field_spec* spec, const void* const* ref_frames, int64_t ref_row_stride,
                              const void* const* dis_frames, int64_t dis_row_stride, int32_t n_frames, uint64_t* out);
PQA_API int pqa_field_moments_device(pqa_ctx* ctx, const pqa_field_spec* spec, const void* ref, int64_t ref_row_pitch,
                                     int64_t ref_frame_pitch, const void* dis, int64_t dis_row_pitch, int64_t dis_frame_pitch,
                                     int32_t n_frames, uint64_t* out);

/* Coding-grid detection: the gradient energy per LINE of n_frames frame pairs of one plane, synchronously -- what
 * pqa2_amd/grid.py turns into the period and phase of a block grid: the one artefact an encoder leg leaves and no other leg
 * does, which neither the tile moments (per tile) nor the band moments (per octave) localise.  Planes of width x height samples
 * (the spec's, independent of the context's width and height; each 1 ... 8192), u8 in an 8-bit context, otherwise u16 of the
 * context's bit depth b (a sample above 2^b - 1 is read as 2^b - 1).  With R the reference and D the captured plane of a frame:
 *     column line x = 1 ... W - 1, the boundary between the columns x - 1 and x:
 *         a = R[y][x] - R[y][x-1]   b = D[y][x] - D[y][x-1]   cols[x] = (sum_y a^2, sum_y b^2, sum_y a b)
 *     row line y = 1 ... H - 1, the boundary between the rows y - 1 and y:
 *         a = R[y][x] - R[y-1][x]   b = D[y][x] - D[y-1][x]   rows[y] = (sum_x a^2, sum_x b^2, sum_x a b)
 * and line 0 of each axis is zero (a 1-wide or 1-high plane gives zeros on that axis).  out (host) is [n_frames][H + W][3],
 * the H row lines first, then the W column lines.  Exact, no floating point anywhere: words 0 and 1 are uint64, word 2 is int64
 * stored in the word as two's complement (as pqa_temporal_moments does); every sum is below 8192 * 4095^2 < 2^37 in magnitude.
 * pqa_edge_sums() is 3.  Any context, no feature bit; buffers are made on first use, grow only and are freed with the context.
 * Independent of the scoring chain: a call between two pqa_submit calls changes no record.  PQA_EINVAL, before any device
 * call, on a null pointer, a bad struct_size, a size outside 1 ... 8192, a row pitch that is negative, shorter than a row or no
 * multiple of the sample size, or a negative frame count.  n_frames == 0 succeeds and writes nothing.  Kernel and accumulator
 * bounds: DESIGN.md section 5.
 *
 * pqa_edge_profiles: frames in HOST memory (ref_frames[f] / dis_frames[f] point at planes, rows *_row_stride bytes apart; the
 * frames need not be contiguous).  They travel in chunks of 8 pairs through the pinned buffers of pqa_resample.
 * pqa_edge_profiles_device: both clips in device memory (frame f at base + f * frame_pitch, rows row_pitch BYTES apart), under
 * the ordering contract of pqa_submit_device. */
typedef struct pqa_edge_spec {
  uint32_t struct_size;
  uint32_t width, height; /* of THIS plane, 1 ... 8192 */
} pqa_edge_spec;
PQA_API int pqa_edge_profiles(pqa_ctx* ctx, const pqa_edge_spec* spec, const void* const* ref_frames, int64_t ref_row_stride,
                              const void* const* dis_frames, int64_t dis_row_stride, int32_t n_frames, uint64_t* out);
PQA_API int pqa_edge_profiles_device(pqa_ctx* ctx, const pqa_edge_spec* spec, const void* ref, int64_t ref_row_pitch,
                                     int64_t ref_frame_pitch, const void* dis, int64_t dis_row_pitch, int64_t dis_frame_pitch,
                                     int32_t n_frames, uint64_t* out);
PQA_API int pqa_edge_sums(void);

/* Colour-matrix alignment: the cross-plane moments of n_frames frame pairs, synchronously -- what a capture chain that decodes
 * Y'CbCr with one matrix and encodes with another (BT.709 through a BT.601 leg) leaves behind, which no single-plane
 * measurement sees.  Works on the chroma grid of the context: chroma_shift = (hs, vs), s = 2^(hs + vs), chroma planes of
 * ceil(width / 2^hs) x ceil(height / 2^vs) samples.  For every chroma sample c,
 *     z(c) = (1, SYr, Ur, Vr, SYd, Ud, Vd)
 * with SY the integer sum of the 2^hs x 2^vs luma samples c covers, luma coordinates clamped to the plane (a partial edge
 * block of an odd-sized frame still has s terms); nothing is divided.  out[f][28], 28 = pqa_colour_sums(), is the upper
 * triangle of sum_c z z^T, row-major ((0,0), (0,1) ... (0,6), (1,1) ... (6,6)), exact uint64; entry 0 is the number of samples
 * that entered.  Mask: a sample enters only if every captured luma sample feeding SYd, Ud and Vd all lie in [lo, hi] -- the
 * chain clips after it converts, and clipped samples bias a linear fit; lo = 0, hi = 2^bit_depth - 1 keeps everything;
 * reference samples are never masked.  Samples are u8 in an 8-bit context, otherwise u16 of the context's bit depth b (a
 * sample above 2^b - 1 is read as 2^b - 1).  Any context with n_planes == 3 and chroma shifts of 0 or 1, no feature bit;
 * buffers are made on first use, grow only and are freed with the context.  Independent of the scoring chain: a call between
 * two pqa_submit calls changes no record.  PQA_EINVAL, before any device call, on a null pointer, a negative frame count,
 * n_planes != 3, a chroma shift above 1, lo > hi, hi > 2^b - 1, a row pitch shorter than a row (or, in device memory, a pitch
 * that is no multiple of the sample size).  n_frames == 0 succeeds and writes nothing.  pqa2_amd/align.py (best_colour,
 * colour_correction) turns the sums into the 3 x 4 map and its inverse; kernel and accumulator bounds: DESIGN.md section 5.
 *
 * pqa_colour_moments: frames in HOST memory, laid out as for pqa_frame_sad (frames[f * 3 + p]: plane p of frame f, rows
 * strides[p] bytes apart).  They travel in chunks of 8 pairs through the pinned buffers of pqa_resample.
 * pqa_colour_moments_device: both clips in device memory (pitches in BYTES), under the ordering contract of pqa_submit_device. */
PQA_API int pqa_colour_sums(void);
PQA_API int pqa_colour_moments_device(pqa_ctx* ctx, const pqa_device_clip* ref, const pqa_device_clip* dis, int32_t n_frames,
                                      uint32_t lo, uint32_t hi, uint64_t* out);
PQA_API int pqa_colour_moments(pqa_ctx* ctx, const void* const* ref_frames, const int64_t ref_strides[3],
                               const void* const* dis_frames, const int64_t dis_strides[3], int32_t n_frames, uint32_t lo,
                               uint32_t hi, uint64_t* out);

/* The matrix apply: every frame of src through the 3 x 4 integer matrix m (row-major, Q14; column 0 is the offset in Q14 code
 * values) into planes of the same sizes, synchronously.  With top = 2^bit_depth - 1 and c = (x >> hs, y >> vs):
 *     Y'(x, y) = clamp((m[0] + m[1] Y(x, y) + m[2] U(c) + m[3] V(c) + 2^13) >> 14, 0, top)
 *     U'(c)    = clamp((m[4] s + m[5] SY(c) + s m[6] U(c) + s m[7] V(c) + s 2^13) >> (14 + hs + vs), 0, top)
 * and V' like U' with m[8 ... 11]; >> is an arithmetic shift.  Chroma is read by replication for luma, luma as the clamped
 * block sum for chroma: both as in the moments above.  The identity (m[1] = m[6] = m[11] = 16384, the rest 0) returns the
 * source.  Same contexts, staging, independence and argument rules as the moments; in addition PQA_EINVAL on a null matrix or
 * an entry out of range: |m[r][0]| < 2^28 (an offset below 2^14 code values), |m[r][1 ... 3]| < 2^16 (gains below 4).  The
 * destination of pqa_colour_apply_device is written (its plane pointers are const only because the struct is shared); it
 * may be the source. */
PQA_API int pqa_colour_apply_device(pqa_ctx* ctx, const int32_t m[12], const pqa_device_clip* src, const pqa_device_clip* dst,
                                    int32_t n_frames);
PQA_API int pqa_colour_apply(pqa_ctx* ctx, const int32_t m[12], const void* const* src_frames, const int64_t src_strides[3],
                             void* const* dst_frames, const int64_t dst_strides[3], int32_t n_frames);

/* Delta E ITP (ITU-R BT.2124): the colour difference of n_frames frame pairs in ICtCp (BT.2100), synchronously -- the one
 * colour metric here that means something on a PQ or HLG clip (PQA_FEAT_CIEDE decodes every clip as BT.709 / sRGB).  For every
 * luma pixel, for the reference and the captured frame (chroma read by replication):
 *     (Y, Cb, Cr, 1) in code values  -- yuv_to_rgb -->  R'G'B'  -- transfer -->  display light F in cd/m2
 *     F  -- rgb_to_lms -->  LMS / 10000, clamped at 0  -- ST 2084 inverse EOTF -->  L'M'S'  -- BT.2100 -->  (I, Ct, Cp)
 * and dE = sqrt(dI^2 + dT^2 + dP^2) with dI = 720 (I_ref - I_dis), dT = 360 (Ct_ref - Ct_dis), dP = 720 (Cp_ref - Cp_dis); 1 is
 * about one just-noticeable difference.  Transfers: PQA_ITP_PQ, the ST 2084 EOTF of R'G'B' clamped to [0, 1]; PQA_ITP_HLG, the
 * BT.2100 HLG inverse OETF of max(E', 0) and the OOTF F = peak Ys^(gamma - 1) E, gamma = 1.2 + 0.42 log10(peak / 1000), Ys =
 * 0.2627 R + 0.6780 G + 0.0593 B; PQA_ITP_BT1886, F = peak max(E', 0)^2.4.  The matrices are the caller's (pqa2_amd/itp.py
 * builds them from the matrix coefficients, range, depth and primaries); a neutral sample -- chroma at the point where the
 * three rows of yuv_to_rgb agree -- has Ct = Cp = 0 exactly when the rows of each matrix agree on it to within f32 rounding.
 * out[f][8], 8 = pqa_itp_sums(), doubles: sum of dE, sum of dI^2, sum of dT^2, sum of dP^2, max dE, the number of pixels with dE >
 * threshold, the number of pixels (width x height), the sum of I of the reference.  f32 per pixel, the hardware log2 / exp2;
 * errors: DESIGN.md section 5.  A frame's row does not depend on the number of frames of the call, on pitches or on alignment.
 * Samples are u8 in an 8-bit context, otherwise u16.  Any context with n_planes == 3, every chroma layout it accepts, no feature
 * bit; buffers are made on first use, grow only and are freed with the context.  Independent of the scoring chain: a call
 * between two pqa_submit calls changes no record.  PQA_EINVAL, before any device call, on a null pointer, n_planes != 3, an
 * unknown transfer, a coefficient that is not finite, peak <= 0 (or not finite) for HLG / BT.1886, a threshold that is
 * negative or not finite, a negative frame count, a row pitch shorter than a row (or, in device memory, a pitch that is no
 * multiple of the sample size).  n_frames == 0 succeeds and writes nothing.
 *
 * pqa_delta_itp: frames in HOST memory, laid out as for pqa_colour_moments; they travel in chunks of 8 pairs through the pinned
 * buffers of pqa_resample.  pqa_delta_itp_device: both clips in device memory (pitches in BYTES), under the ordering contract
 * of pqa_submit_device. */
enum { PQA_ITP_PQ = 0, PQA_ITP_HLG = 1, PQA_ITP_BT1886 = 2 };
typedef struct pqa_itp_spec {
  uint32_t transfer;    /* PQA_ITP_PQ 0, PQA_ITP_HLG 1, PQA_ITP_BT1886 2 */
  float yuv_to_rgb[12]; /* rows of [Y Cb Cr 1] in code values -> R'G'B', nominal range 0..1 */
  float rgb_to_lms[9];  /* linear display light in cd/m2 -> LMS / 10000 */
  float peak;           /* Lw, cd/m2: HLG and BT.1886; ignored for PQ */
  float threshold;      /* dE above which a pixel is counted */
} pqa_itp_spec;
PQA_API int pqa_itp_sums(void);
PQA_API int pqa_delta_itp_device(pqa_ctx* ctx, const pqa_itp_spec* spec, const pqa_device_clip* ref, const pqa_device_clip* dis,
                                 int32_t n_frames, double* out);
PQA_API int pqa_delta_itp(pqa_ctx* ctx, const pqa_itp_spec* spec, const void* const* ref_frames, const int64_t ref_strides[3],
                          const void* const* dis_frames, const int64_t dis_strides[3], int32_t n_frames, double* out);

/* What "gray" means to the two luma-statistics calls above.  PQA_GRAY_LUMA (default): the luma samples as they are.
 * PQA_GRAY_BT601_FULL: gray = clamp(round((Y - 16 s) * 255 / (219 s)), 0, 255), s = 2^(bit_depth - 8) -- what the
 * reference's cv2.cvtColor(frame, cv2.COLOR_BGR2GRAY) sees for a limited-range clip (cv2.VideoCapture has expanded it to
 * full-range BGR; with BT.601 on both legs the chroma terms cancel).  The statistics are then those of that 8-bit gray for
 * every bit depth, and `threshold` is in its units: the absolute constants of the reference's rules (180 / 200 / 220 / 230 /
 * 240, app/bookend_alignment.py:818-852, app/reference_analyzer.py:134) mean what they mean there. */
enum { PQA_GRAY_LUMA = 0, PQA_GRAY_BT601_FULL = 1 };
PQA_API int pqa_set_luma_gray(pqa_ctx* ctx, uint32_t mode);

/* Measurement hooks (bench.py): HIP-event timing of individual kernels on the context's stream.
 * kernel ids: 0..3 vif_stat scale s (each also produces the next scale's planes), 4 ciede2000 (its kernel and epilogue),
 * 5..6 reserved,
 * 7..10 adm scale s,
 * 11 motion, 12 sse, 13 ssim, 14 finalize, 15 ms_ssim (all five scales, their decimations and the extension epilogue),
 * 16 float_ssim.
 * pqa_profile_enable(ctx, 0) stops, (ctx, 1) times every kernel, (ctx, mask << 1) only the kernels whose bit
 * is set in mask (event records between kernels are not free: ~10 % of a step when every kernel is timed). */
enum { PQA_PROF_KERNELS = 17 };
PQA_API int pqa_profile_enable(pqa_ctx* ctx, int on);
PQA_API int pqa_profile_read(pqa_ctx* ctx, int kernel_id, double* total_ms, uint64_t* launches, uint64_t* frames);
PQA_API const char* pqa_profile_kernel_name(int kernel_id);

/* Test hook (no device needed): the per-lane tap-matrix fragments of the scale-0 VIF kernel, [fragment][lane 0..63][8 f16 bit
 * patterns], so that a CPU test can replay both matrix passes in numpy against a direct convolution (tests/test_host.py).
 * Returns the number of fragments, or -(halfwords needed) when `out` is too small. */
PQA_API int pqa_debug_vif_march_table(uint16_t* out, int32_t capacity_halfwords);

/* Test / measurement hook (no device needed): how the scale-0 VIF kernel cuts a width x height frame into waves, and what a
 * 16 x 16 block costs on the matrix cores: out6 = {16-column stripes, 16-row blocks, blocks per segment, segments per stripe,
 * first-pass MFMAs per block, second-pass MFMAs per block}.  A wave = one stripe x one segment; a segment repeats one block
 * of the first pass.  bench.py prices `roofline.mfma` with it instead of mirroring the rule. */
PQA_API int pqa_debug_vif_march_shape(uint32_t width, uint32_t height, int32_t* out6);

/* Test / measurement hook: how the context runs VIF scale 1, 2 or 3 for a launch of n_frames frames, under the switches it
 * read at pqa_create (PQA_VIF_STRIP, PQA_VIF_STRIP_SEG): out4 = {strips (tile columns), tile rows, tile rows per segment,
 * segments per strip}.  A workgroup of the strip kernel marches down one segment of one strip; tile rows per segment = 0
 * means the tiled kernel runs there (one workgroup per tile).  PQA_EINVAL on a null pointer, another scale or n_frames = 0. */
PQA_API int pqa_debug_vif_strip_shape(pqa_ctx* ctx, uint32_t scale, uint32_t n_frames, int32_t* out4);

/* Test hook (host only): where the ADM march kernels compute anything at all for a width x height frame -- the dependency
 * cone of libvmaf's 10 % accumulation windows (pqa2_amd/csrc/adm_need.h; PQA_ADM_CONE=0 at pqa_create computes whole bands
 * instead).  out20 = per ADM scale 0 .. 3 {row lo, row hi, column lo, column hi} of the coefficient positions (half-open),
 * then {row lo, row hi, column lo, column hi} of the input samples they read.  PQA_EINVAL on a null pointer or a size of
 * 0 or above 65536. */
PQA_API int pqa_debug_adm_need(uint32_t width, uint32_t height, int32_t* out20);

/* Test hook (host only): per frame of width x height at bit_depth, what the context's workspace sizing functions return for
 * the four march kernels ("sized") and the number of partial slots a launch of each writes ("written": the launcher's own
 * count, from a launch of no frames; 0 where the launcher does not take such planes).  out (cap >= PQA_PARTIAL_COUNT_INTS) =
 *   [0] sized, [1] written: the scale-0 VIF march kernel (vif_march_partials_max; pairs of doubles),
 *   [2 + 2 s] sized, [3 + 2 s] written: the ADM march kernel at scale s = 0 .. 3 (adm_march_partials; sextets),
 *   [10] sized (0 where the context does not size for it), [11] written: the ADM pyramid kernel (adm_pyramid_partials),
 *   [12] sized, [13] written: the motion march kernel (motion_march_partials; doubles).
 * PQA_EINVAL on a null or short output, a size outside 16 .. 16384 or a bit depth other than 8, 10, 12. */
enum { PQA_PARTIAL_COUNT_INTS = 14 };
PQA_API int pqa_debug_partial_counts(uint32_t width, uint32_t height, uint32_t bit_depth, int32_t* out, int32_t cap);

/* Test hook (needs a device): the CIEDE2000 device function of the PQA_FEAT_CIEDE kernel on n Lab pairs
 * lab_pairs[n][6] = {L1, a1, b1, L2, a2, b2}: the inputs are converted to f32, de_out[n] receives the f32 results widened.
 * PQA_EDEVICE without a device (text in pqa_last_error(NULL)), PQA_EINVAL on a null pointer or n < 0. */
PQA_API int pqa_debug_ciede2000(const double* lab_pairs, int32_t n, double* de_out);

/* Test hook (needs a device): the ICtCp device function of the pqa_delta_itp kernel on n code triples yuv_triples[n][3] =
 * {Y, Cb, Cr} (f32): itp_out[n][3] receives (720 I, 360 Ct, 720 Cp) as f32.  The spec's threshold is not read.  PQA_EDEVICE
 * without a device (text in pqa_last_error(NULL)), PQA_EINVAL on a null pointer, n < 0 or a spec pqa_delta_itp refuses. */
PQA_API int pqa_debug_itp(const pqa_itp_spec* spec, const float* yuv_triples, int32_t n, float* itp_out);

/* Test hook (no device needed): the host-built tables the PQA_FEAT_CAMBI kernels use at w x h and bit_depth (8 or 10):
 * out[PQA_CAMBI_PARAM_INTS] = {adjusted window size, r, pixels_in_window, mask threshold, tvi_for_diff[1..4],
 * contrast weights[4], (w_s, h_s) of scales 0..4}.  PQA_EINVAL on a null pointer, cap < PQA_CAMBI_PARAM_INTS, a size
 * pqa_create rejects or another bit depth. */
enum { PQA_CAMBI_PARAM_INTS = 22 };
PQA_API int pqa_debug_cambi_params(uint32_t w, uint32_t h, uint32_t bit_depth, int32_t* out, int32_t cap);

/* Test hook (needs a device): the PQA_FEAT_CAMBI kernels on one w x h luma plane in host memory (u8 at bit_depth 8, u16 at
 * 10; rows row_pitch_bytes apart).  cmap[cap] receives the c-values of scales 0..4, each w_s x h_s row-major, one after
 * another (sum of w_s h_s floats; PQA_EINVAL when cap is smaller); *score (nullable) the frame's cambi.  PQA_EINVAL on a
 * null pointer or a size / depth pqa_create rejects for cambi, PQA_EDEVICE without a device. */
PQA_API int pqa_debug_cambi_cmap(const void* luma, int64_t row_pitch_bytes, uint32_t w, uint32_t h, uint32_t bit_depth,
                                 float* cmap, int64_t cap, double* score);

/* Test hook (no device needed): the PQA_FEAT_PSNR_HVS kernel's od_bin_fdct8x8 (its own host / device function) on n
 * row-major 8 x 8 int32 blocks in[n][64] -> out[n][64] (row i = vertical frequency i).  PQA_EINVAL on a null pointer or
 * n < 0. */
PQA_API int pqa_debug_psnr_hvs_dct8x8(const int32_t* in, int32_t* out, int32_t n);

/* Test hook (no device needed): out[PQA_PSNR_HVS_TABLE_FLOATS] = the CSF tables of Y, Cb, Cr ([3][8][8] f32), then the
 * mask tables M = (0.3885746225901003 CSF)^2 ([3][8][8]).  PQA_EINVAL on a null pointer or a smaller cap. */
enum { PQA_PSNR_HVS_TABLE_FLOATS = 384 };
PQA_API int pqa_debug_psnr_hvs_tables(float* out, int32_t cap);

/* Test hook (needs a device): the PQA_FEAT_PSNR_HVS kernel on one w x h plane pair in host memory (u8 at bit_depth 8, u16
 * above; rows row_pitch_bytes apart) with the tables of plane_kind (0 = Y, 1 = Cb, 2 = Cr).  block_err receives the
 * per-block error sums, [(h - 1) / 7][(w - 1) / 7] f32 row-major; *mse (nullable) the plane's mse.  PQA_EINVAL on a null
 * pointer, a plane under 8 x 8, a bad depth, pitch or kind, PQA_EDEVICE without a device. */
PQA_API int pqa_debug_psnr_hvs_plane(const void* ref, const void* dis, int64_t row_pitch_bytes, uint32_t w, uint32_t h,
                                     uint32_t bit_depth, uint32_t plane_kind, float* block_err, double* mse);

/* Test hook (needs a device): the PQA_FEAT_XPSNR kernels on one w x h luma plane (u8 at bit_depth 8, u16 above; rows
 * row_pitch_bytes apart) with ref_m1 / ref_m2 (nullable: zero planes) as the reference frames one and two before it and
 * hfr selecting the second-order temporal term.  out receives [blocks][3] = {sse, sa, ta} per luma block in raster
 * order, blocks = ceil(w / b) * ceil(h / b) (one block covering the plane when b < 4, with sa = ta = 0); *wsse (nullable)
 * the plane's WSSE.  PQA_EINVAL on a null pointer, a bad size, depth or pitch, PQA_EDEVICE without a device. */
PQA_API int pqa_debug_xpsnr_blocks(const void* ref, const void* ref_m1, const void* ref_m2, const void* dis,
                                   int64_t row_pitch_bytes, uint32_t w, uint32_t h, uint32_t bit_depth, int32_t hfr,
                                   uint64_t* out, double* wsse);

/* Test hook (needs a device): the PQA_FEAT_SITI kernels on one w x h luma plane cur (u8 at bit_depth 8, u16 at 10; rows
 * row_pitch_bytes apart) with prev (nullable: a chain start) as the frame before it; full_range != 0: no range
 * conversion.  gmap (nullable) receives the (w - 2) x (h - 2) gradient map in raster order, si_ti[0] / si_ti[1] the SI
 * and TI.  w, h >= 3.  PQA_EINVAL on a null pointer, a bad size, depth or pitch, PQA_EDEVICE without a device. */
PQA_API int pqa_debug_siti_plane(const void* cur, const void* prev, int64_t row_pitch_bytes, uint32_t w, uint32_t h,
                                 uint32_t bit_depth, int32_t full_range, float* gmap, double* si_ti);

/* Test hook (no device needed): one axis of the pqa_resample tables.  Destination sample i of n_dst reads the source samples
 * first[i] ... first[i] + *taps - 1 of n_src with the coefficients coeff[i * cap_taps + 0 ... *taps) (scale 2^14, a row sums
 * to 16384; zero from the row's last tap to cap_taps); x0_q16 / ext_q16: the source window of this axis.  *taps: the longest
 * row (at most 32; rows are cut to their non-zero span).  PQA_EINVAL on a null pointer, a bad filter, a size outside
 * 1 ... 8192, a non-positive window, a row of more than 32 taps, or cap_taps < *taps (*taps is set then). */
PQA_API int pqa_debug_resample_table(uint32_t filter, int32_t n_src, int32_t n_dst, int64_t x0_q16, int64_t ext_q16,
                                     int32_t* first, int16_t* coeff, int32_t cap_taps, int32_t* taps);

/* Test hook (needs a device, no context): the two colour kernels on ONE frame pair of any size, 1 ... 16384 each way -- also the
 * sizes no context accepts.  ref / dis: packed planes Y, U, V (rows width * sample-size bytes apart; chroma planes of
 * ceil(w / 2^hshift) x ceil(h / 2^vshift)).  sums28 (nullable) receives pqa_colour_moments' 28 sums of the pair under the mask
 * lo ... hi; with m (nullable) the packed planes applied[3] receive dis through pqa_colour_apply's matrix.  PQA_EINVAL on a
 * null pointer, a bad size, depth, shift, mask or matrix, PQA_EDEVICE without a device. */
PQA_API int pqa_debug_colour(uint32_t bit_depth, uint32_t hshift, uint32_t vshift, uint32_t w, uint32_t h,
                             const void* const ref[3], const void* const dis[3], uint32_t lo, uint32_t hi, uint64_t* sums28,
                             const int32_t* m, void* const applied[3]);

#ifdef __cplusplus
}
#endif
#endif /* PQA_VMAF_H */
