"""ctypes binding of libpqa_vmaf.so (include/pqa_vmaf.h).  No fallback: if the HIP extension is
missing or fails to load, importing callers get a loud ImportError/RuntimeError."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
# PQA_LIB_PATH: load another build of the SAME library (tools/build_variant.sh) -- A/B parity and timing runs only
LIB_PATH = os.environ.get("PQA_LIB_PATH") or os.path.join(_HERE, "csrc", "libpqa_vmaf.so")

PQA_OK, PQA_EINVAL, PQA_EDEVICE, PQA_ENOMEM, PQA_ECANCELLED, PQA_ESTATE = 0, -1, -2, -3, -4, -5
FEAT_VIF, FEAT_ADM, FEAT_MOTION, FEAT_PSNR, FEAT_SSIM = 1, 2, 4, 8, 16
FEAT_VMAF = FEAT_VIF | FEAT_ADM | FEAT_MOTION
FEAT_ALL = FEAT_VMAF | FEAT_PSNR | FEAT_SSIM   # stays 31: the features of the 24-double record
FEAT_FLOAT_SSIM, FEAT_MS_SSIM = 32, 64          # libvmaf float_ssim / float_ms_ssim: results in the extension record
FEAT_CIEDE = 256                                # libvmaf ciede (ciede2000): results in the extension record (bit 7 unassigned)
FEAT_CAMBI, FEAT_CAMBI_FULL_REF = 512, 1024          # libvmaf cambi of the distorted (and reference) luma: extension record
FEAT_PSNR_HVS = 2048                            # libvmaf psnr_hvs: results in the second extension record (pqa_collect_ext2)
FEAT_XPSNR, FEAT_XPSNR_HFR = 4096, 8192              # FFmpeg xpsnr (second-order temporal term): third extension record
FEAT_SITI, FEAT_SITI_REF_FULL, FEAT_SITI_DIS_FULL = 16384, 32768, 65536   # FFmpeg siti (full-range clips): fourth ext. record
FEAT_INTEGRITY = 131072                         # FFmpeg freezedetect / blackdetect / scdet reductions: fifth extension record
FEAT_KNOWN = (FEAT_ALL | FEAT_FLOAT_SSIM | FEAT_MS_SSIM | FEAT_CIEDE | FEAT_CAMBI | FEAT_CAMBI_FULL_REF | FEAT_PSNR_HVS
              | FEAT_XPSNR | FEAT_XPSNR_HFR | FEAT_SITI | FEAT_SITI_REF_FULL | FEAT_SITI_DIS_FULL
              | FEAT_INTEGRITY)
VIF_BORDER_FLOAT, VIF_BORDER_INTEGER = 0, 1  # pqa_config.vif_border (include/pqa_vmaf.h)
FIXED_VIF, FIXED_MOTION, FIXED_ADM, FIXED_ALL = 1, 2, 4, 7   # pqa_config.fixed_point mask
REC_VIF_NUM, REC_VIF_DEN, REC_ADM_NUM, REC_ADM_DEN, REC_MOTION, REC_SSIM, REC_SSE = 0, 4, 8, 12, 16, 17, 20
RECORD_DOUBLES = 24
# extension record (pqa_collect_ext): float_ssim, its l/c/s means, float_ms_ssim, per-scale l/c/s means; NaN where not run
EXT_FLOAT_SSIM, EXT_FLOAT_SSIM_LCS, EXT_MS_SSIM, EXT_MS_SSIM_L, EXT_MS_SSIM_C, EXT_MS_SSIM_S, EXT_RESERVED = 0, 1, 4, 5, 10, 15, 20
EXT_CIEDE2000, EXT_CIEDE_MEAN_DE = 20, 21   # ciede2000 = 45 - 20 log10(mean dE00), and the mean itself
EXT_CAMBI, EXT_CAMBI_SOURCE = 22, 23         # cambi of the distorted luma, and of the reference luma (FULL_REF; NaN without)
CAMBI_PARAM_INTS = 22                        # pqa_debug_cambi_params
PARTIAL_COUNT_INTS = 14                      # pqa_debug_partial_counts
EXT_DOUBLES = 24
# second extension record (pqa_collect_ext2): psnr_hvs_y / _cb / _cr, psnr_hvs, the three plane MSEs; NaN where not run
EXT2_PSNR_HVS_Y, EXT2_PSNR_HVS_CB, EXT2_PSNR_HVS_CR, EXT2_PSNR_HVS, EXT2_PSNR_HVS_MSE, EXT2_RESERVED = 0, 1, 2, 3, 4, 7
EXT2_DOUBLES = 8
# third extension record (pqa_collect_ext3): XPSNR y / u / v, the three WSSE values; NaN where not run / no such plane
EXT3_XPSNR_Y, EXT3_XPSNR_U, EXT3_XPSNR_V, EXT3_WSSE, EXT3_RESERVED = 0, 1, 2, 3, 6
EXT3_DOUBLES = 8
# fourth extension record (pqa_collect_ext4): SI / TI of the distorted, then of the reference luma; NaN where not run
EXT4_SI, EXT4_TI, EXT4_SI_SOURCE, EXT4_TI_SOURCE, EXT4_RESERVED = 0, 1, 2, 3, 4
EXT4_DOUBLES = 8
# fifth extension record (pqa_collect_ext5): exact SAD of Y / U / V against the previous distorted frame (NaN at a chain
# start / no such plane), the number of luma samples <= the black threshold
EXT5_SAD_PREV, EXT5_BLACK_COUNT, EXT5_RESERVED = 0, 3, 4
EXT5_DOUBLES = 8
# the extension record blocks, in the order pqa_collect_ext5 takes them: (name, doubles per frame, the feature bits that own
# it).  The one place on this side where a block is declared (pqa_ctx.h has the library's table); collect_blocks, score_files
# and finish_records go by index into it.
EXT_BLOCKS = (
    ("ext", EXT_DOUBLES, FEAT_FLOAT_SSIM | FEAT_MS_SSIM | FEAT_CIEDE | FEAT_CAMBI),
    ("ext2", EXT2_DOUBLES, FEAT_PSNR_HVS),
    ("ext3", EXT3_DOUBLES, FEAT_XPSNR),
    ("ext4", EXT4_DOUBLES, FEAT_SITI),
    ("ext5", EXT5_DOUBLES, FEAT_INTEGRITY),
)
PSNR_HVS_TABLE_FLOATS = 384                  # pqa_debug_psnr_hvs_tables: CSF[3][8][8], then M[3][8][8]
PROF_KERNELS = 17
GRAY_LUMA, GRAY_BT601_FULL = 0, 1   # pqa_set_luma_gray

# every symbol include/pqa_vmaf.h declares
EXPORTS = [
    "pqa_version", "pqa_record_doubles", "pqa_ext_doubles", "pqa_ext2_doubles", "pqa_ext3_doubles", "pqa_ext4_doubles", "pqa_ext5_doubles", "pqa_config_init", "pqa_create", "pqa_destroy", "pqa_set_stream",
    "pqa_submit", "pqa_submit_fd", "pqa_submit_fd_run", "pqa_submit_device", "pqa_submit_surfaces", "pqa_submit_packed", "pqa_set_motion_halo", "pqa_set_ref_history", "pqa_set_dis_history", "pqa_set_dis_history_planes", "pqa_set_black_threshold", "pqa_frame_sad", "pqa_frame_sad_device", "pqa_flush", "pqa_collect", "pqa_collect_ext", "pqa_collect_ext2", "pqa_collect_ext3", "pqa_collect_ext4", "pqa_collect_ext5", "pqa_sync",
    "pqa_cancel", "pqa_reset", "pqa_last_error", "pqa_luma_stats_device", "pqa_luma_stats", "pqa_cross_sse_device", "pqa_cross_sse", "pqa_shift_sse_device", "pqa_shift_sse", "pqa_level_stats_device", "pqa_level_stats", "pqa_level_bins", "pqa_resample", "pqa_resample_device", "pqa_unpack", "pqa_unpack_device", "pqa_format_convert", "pqa_format_convert_device", "pqa_rgb_convert", "pqa_rgb_convert_device", "pqa_table_apply", "pqa_table_apply_device", "pqa_deinterlace", "pqa_deinterlace_device", "pqa_deint_chunk", "pqa_deint_block_bytes", "pqa_deint_block_rows", "pqa_mask_blend", "pqa_mask_blend_device", "pqa_flow_moments", "pqa_flow_moments_device", "pqa_line_profiles", "pqa_line_profiles_device", "pqa_tile_moments", "pqa_tile_moments_device", "pqa_band_moments", "pqa_band_moments_device", "pqa_band_sums", "pqa_temporal_moments", "pqa_temporal_moments_device", "pqa_temporal_sums", "pqa_field_moments", "pqa_field_moments_device", "pqa_edge_profiles", "pqa_edge_profiles_device", "pqa_edge_sums", "pqa_colour_sums", "pqa_colour_moments", "pqa_colour_moments_device", "pqa_colour_apply", "pqa_colour_apply_device", "pqa_itp_sums", "pqa_delta_itp", "pqa_delta_itp_device", "pqa_set_luma_gray",
    "pqa_profile_enable",
    "pqa_profile_read", "pqa_profile_kernel_name", "pqa_debug_vif_march_table", "pqa_debug_vif_march_shape", "pqa_debug_vif_strip_shape", "pqa_debug_adm_need",
    "pqa_debug_partial_counts",
    "pqa_debug_ciede2000", "pqa_debug_itp", "pqa_debug_cambi_params", "pqa_debug_cambi_cmap", "pqa_debug_psnr_hvs_dct8x8",
    "pqa_debug_psnr_hvs_tables", "pqa_debug_psnr_hvs_plane", "pqa_debug_xpsnr_blocks", "pqa_debug_siti_plane",
    "pqa_debug_resample_table", "pqa_debug_colour",
]


class PqaConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("device", C.c_int32), ("width", C.c_uint32), ("height", C.c_uint32),
        ("bit_depth", C.c_uint32), ("n_planes", C.c_uint32), ("chroma_hshift", C.c_uint32),
        ("chroma_vshift", C.c_uint32), ("features", C.c_uint32), ("max_batch", C.c_uint32),
        ("result_capacity", C.c_uint32), ("n_subsample", C.c_uint32),
        ("vif_enhn_gain_limit", C.c_double), ("adm_enhn_gain_limit", C.c_double),
        ("vif_border", C.c_uint32), ("fixed_point", C.c_uint32),
    ]


class PqaDeviceClip(C.Structure):
    _fields_ = [("plane", C.c_void_p * 3), ("row_pitch", C.c_int64 * 3), ("frame_pitch", C.c_int64 * 3)]


SURFACE_NV12, SURFACE_P01X = 1, 2
# packed capture formats (4:2:2; UYVY / YUYV 8 bit, V210 10 bit); PLANAR: planar planes in a PqaHostClip only
SURFACE_PLANAR, SURFACE_UYVY, SURFACE_YUYV, SURFACE_V210 = 0, 3, 4, 5
PACKED_FORMATS = {"uyvy422": SURFACE_UYVY, "yuyv422": SURFACE_YUYV, "v210": SURFACE_V210}
PACKED_BIT_DEPTH = {SURFACE_UYVY: 8, SURFACE_YUYV: 8, SURFACE_V210: 10}
# packed RGB captures (4 bytes a pixel; r210 10 bit): pqa_rgb_convert only
SURFACE_BGRA, SURFACE_ARGB, SURFACE_RGBA, SURFACE_ABGR, SURFACE_R210 = 6, 7, 8, 9, 10


class PqaSurfaceClip(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("format", C.c_uint32), ("luma", C.c_void_p), ("chroma", C.c_void_p),
                ("luma_row_pitch", C.c_int64), ("luma_frame_pitch", C.c_int64),
                ("chroma_row_pitch", C.c_int64), ("chroma_frame_pitch", C.c_int64)]


class PqaHostClip(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("format", C.c_uint32), ("frames", C.POINTER(C.c_void_p)), ("strides", C.c_int64 * 3)]


class PqaUnpackSpec(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("format", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32)]


SITE_COSITED, SITE_CENTRE = 0, 1     # PQA_SITE_*: where a subsampled chroma sample sits along an axis
CONVERT_GENERIC = 1                  # pqa_convert_spec.flags: the general kernel whatever the layout
CONVERT_BIT_DEPTHS = (8, 10, 12)
RGB_GENERIC = 1                      # pqa_rgb_spec.flags: the general kernel whatever the layout
RGB_BIT_DEPTHS = (8, 10)             # pqa_rgb_spec.dst_bits


class PqaRgbSpec(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("format", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32),
                ("dst_bits", C.c_uint32), ("hshift", C.c_uint32), ("vshift", C.c_uint32), ("hsite", C.c_uint32), ("vsite", C.c_uint32),
                ("flags", C.c_uint32), ("m", C.c_int32 * 12)]


class PqaTableSpec(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32)]


class PqaDeintSpec(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("mode", C.c_uint32),
                ("first", C.c_uint32), ("rate", C.c_uint32)]


DEINT_MODES = {"intra": 0, "adaptive": 1}          # pqa_deint_spec.mode
DEINT_RATES = {"frame": 0, "field": 1}             # pqa_deint_spec.rate
DEINT_CHUNK = 8                                    # source frames a launch of deinterlace.hip (kernels.h; pqa_deint_chunk())
DEINT_BLOCK_BYTES, DEINT_BLOCK_ROWS = 1024, 64     # bytes of a row / rows a workgroup there writes (pqa_deint_block_*())


MASK_MAX_STEP, MASK_FULL = 6, 256     # pqa_mask_spec: the largest step_log2, the node value that is all fill


class PqaMaskSpec(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("step_log2_x", C.c_uint32),
                ("step_log2_y", C.c_uint32), ("fill", C.c_uint32)]


class PqaConvertSpec(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("src_bits", C.c_uint32), ("dst_bits", C.c_uint32),
                ("luma_width", C.c_uint32), ("luma_height", C.c_uint32),
                ("src_hshift", C.c_uint8), ("src_vshift", C.c_uint8), ("dst_hshift", C.c_uint8), ("dst_vshift", C.c_uint8),
                ("src_hsite", C.c_uint8), ("src_vsite", C.c_uint8), ("dst_hsite", C.c_uint8), ("dst_vsite", C.c_uint8)]


RESAMPLE_BILINEAR, RESAMPLE_BICUBIC, RESAMPLE_LANCZOS3 = 0, 1, 2
RESAMPLE_FILTERS = {"bilinear": RESAMPLE_BILINEAR, "bicubic": RESAMPLE_BICUBIC, "lanczos": RESAMPLE_LANCZOS3}
RESAMPLE_MAX_TAPS = 32


class PqaResampleSpec(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("filter", C.c_uint32), ("src_width", C.c_uint32), ("src_height", C.c_uint32),
                ("dst_width", C.c_uint32), ("dst_height", C.c_uint32), ("x0_q16", C.c_int64), ("y0_q16", C.c_int64),
                ("w_q16", C.c_int64), ("h_q16", C.c_int64)]


FLOW_TILES = (8, 16, 32, 64)
COLOUR_SUMS = 28                                   # pqa_colour_sums(): the upper triangle of a 7 x 7 matrix
COLOUR_Q = 14                                      # pqa_colour_apply: the matrix is Q14
COLOUR_MAX_GAIN, COLOUR_MAX_OFFSET = 1 << 16, 1 << 28   # its entries lie strictly inside (-limit, limit)


class PqaFlowSpec(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("tile", C.c_uint32)]


class PqaProfileSpec(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32)]


PROFILE_STRIPE, PROFILE_BAND = 1024, 64            # columns / rows a workgroup of line_profiles.hip reads (kernels.h)


class PqaTileSpec(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("tile", C.c_uint32)]


TILE_SUMS, TILE_CHUNK = 6, 8                       # sums a tile / frame pairs a launch of tile_moments.hip (kernels.h)


class PqaBandSpec(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("levels", C.c_uint32)]


BAND_SUMS, BAND_CHUNK = 3, 8                       # sums a band / frame pairs a launch of band_moments.hip (kernels.h)


class PqaTemporalSpec(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("tile", C.c_uint32)]


TEMPORAL_SUMS, TEMPORAL_CHUNK = 7, 8               # sums a tile / frame pairs a chunk of temporal_moments.hip (kernels.h)
TEMPORAL_SIGNED = (0, 1, 4, 5)                     # the words of a tile that are int64: sum a, sum b, sum a b, sum a e


class PqaFieldSpec(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32)]


FIELD_SUMS, FIELD_CHUNK = 14, 8                    # words a transition / frame pairs a chunk of field_moments.hip (kernels.h)
FIELD_COLS, FIELD_ROWS = 128, 128                  # columns / rows of a workgroup's block there


class PqaEdgeSpec(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32)]


EDGE_STRIPE, EDGE_BAND = 1024, 64                  # columns / rows a workgroup of edge_profiles.hip reads (kernels.h)
EDGE_SUMS, EDGE_CHUNK = 3, 8                       # sums a line (the third is int64) / frame pairs a launch


ITP_PQ, ITP_HLG, ITP_BT1886 = 0, 1, 2                # pqa_itp_spec.transfer
ITP_SUMS, ITP_CHUNK = 8, 8                         # pqa_itp_sums(): doubles a frame / frame pairs a launch


class PqaItpSpec(C.Structure):
    _fields_ = [("transfer", C.c_uint32), ("yuv_to_rgb", C.c_float * 12), ("rgb_to_lms", C.c_float * 9), ("peak", C.c_float),
                ("threshold", C.c_float)]


class PqaError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"pqa error {code}: {msg}")
        self.code = code


class PqaCancelled(PqaError):
    pass


def build(force: bool = False) -> str:
    """Compile libpqa_vmaf.so for gfx950 in-tree with hipcc (cross-compiles without a GPU)."""
    script = os.path.join(_HERE, "csrc", "build.sh")
    if force:
        for f in os.listdir(os.path.join(_HERE, "csrc")):
            if f.endswith(".o"):
                os.remove(os.path.join(_HERE, "csrc", f))
    r = subprocess.run(["bash", script], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc build failed:\n{r.stdout}\n{r.stderr}")
    return LIB_PATH


_lib = None


def load():
    """Load the HIP extension.  Raises ImportError (never falls back) when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: the MI355X HIP extension is not built (run `python -c 'import "
            f"__graft_entry__ as g; g.build()'` or pqa2_amd/csrc/build.sh).  There is no CPU fallback.")
    # torch wheels bundle their own libamdhip64.so (same SONAME).  Import torch FIRST so that the one HIP
    # runtime in this process is torch's: device pointers and streams are then shared between torch
    # (memory, RCCL) and the kernels.  Loading ours first would leave torch unable to see the GPU.
    try:
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - torch-less consumers use the system ROCm runtime
        pass
    lib = C.CDLL(LIB_PATH)
    missing = [s for s in EXPORTS if not hasattr(lib, s)]
    if missing:
        raise ImportError(f"{LIB_PATH} lacks symbols {missing}")
    vp, i32, i64, dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    lib.pqa_version.restype = C.c_char_p
    lib.pqa_record_doubles.restype = C.c_int
    lib.pqa_config_init.argtypes = [C.POINTER(PqaConfig), C.c_uint32, C.c_uint32]
    lib.pqa_config_init.restype = None
    lib.pqa_create.argtypes = [C.POINTER(PqaConfig), C.POINTER(vp)]
    lib.pqa_destroy.argtypes = [vp]
    lib.pqa_destroy.restype = None
    lib.pqa_set_stream.argtypes = [vp, vp]
    lib.pqa_submit.argtypes = [vp, i64, C.POINTER(vp * 3), C.POINTER(i64 * 3), C.POINTER(vp * 3), C.POINTER(i64 * 3)]
    lib.pqa_submit_fd.argtypes = [vp, i64, C.c_int, C.POINTER(i64 * 3), C.c_int, C.POINTER(i64 * 3)]
    lib.pqa_submit_fd_run.argtypes = [vp, i64, i32, C.c_int, C.POINTER(i64 * 3), i64, C.c_int, C.POINTER(i64 * 3), i64]
    lib.pqa_submit_device.argtypes = [vp, i64, i32, C.POINTER(PqaDeviceClip), C.POINTER(PqaDeviceClip), vp, i64]
    lib.pqa_submit_surfaces.argtypes = [vp, i64, i32, C.POINTER(PqaSurfaceClip), C.POINTER(PqaSurfaceClip),
                                        C.POINTER(PqaSurfaceClip)]
    lib.pqa_submit_packed.argtypes = [vp, i64, i32, C.POINTER(PqaHostClip), C.POINTER(PqaHostClip)]
    lib.pqa_set_motion_halo.argtypes = [vp, vp, i64]
    lib.pqa_flush.argtypes = [vp]
    lib.pqa_collect.argtypes = [vp, i64, i32, vp]
    lib.pqa_collect_ext.argtypes = [vp, i64, i32, vp, vp]
    lib.pqa_ext_doubles.restype = C.c_int
    lib.pqa_collect_ext2.argtypes = [vp, i64, i32, vp, vp, vp]
    lib.pqa_ext2_doubles.restype = C.c_int
    lib.pqa_collect_ext3.argtypes = [vp, i64, i32, vp, vp, vp, vp]
    lib.pqa_ext3_doubles.restype = C.c_int
    lib.pqa_set_ref_history.argtypes = [vp, vp, i32, i64]
    lib.pqa_collect_ext4.argtypes = [vp, i64, i32, vp, vp, vp, vp, vp]
    lib.pqa_ext4_doubles.restype = C.c_int
    lib.pqa_set_dis_history.argtypes = [vp, vp, i64]
    lib.pqa_collect_ext5.argtypes = [vp, i64, i32, vp, vp, vp, vp, vp, vp]
    lib.pqa_ext5_doubles.restype = C.c_int
    lib.pqa_set_dis_history_planes.argtypes = [vp, C.POINTER(vp * 3), C.POINTER(i64 * 3)]
    lib.pqa_set_black_threshold.argtypes = [vp, C.c_uint32]
    lib.pqa_frame_sad.argtypes = [vp, C.POINTER(vp * 3), C.POINTER(i64 * 3), C.POINTER(vp), C.POINTER(i64 * 3), i32, vp]
    lib.pqa_frame_sad_device.argtypes = [vp, C.POINTER(vp * 3), C.POINTER(i64 * 3), C.POINTER(PqaDeviceClip), i32, vp]
    lib.pqa_sync.argtypes = [vp]
    lib.pqa_cancel.argtypes = [vp]
    lib.pqa_luma_stats_device.argtypes = [vp, vp, i64, i64, i32, C.c_uint32, vp]
    lib.pqa_luma_stats.argtypes = [vp, C.POINTER(vp), i64, i32, C.c_uint32, vp]
    lib.pqa_cross_sse_device.argtypes = [vp, vp, i64, i64, i32, vp, i64, i64, i32, i32, i32, vp]
    lib.pqa_cross_sse.argtypes = [vp, C.POINTER(vp), i64, i32, C.POINTER(vp), i64, i32, i32, i32, vp]
    lib.pqa_shift_sse_device.argtypes = [vp, vp, i64, i64, vp, i64, i64, i32, i32, vp]
    lib.pqa_shift_sse.argtypes = [vp, C.POINTER(vp), i64, C.POINTER(vp), i64, i32, i32, vp]
    lib.pqa_level_stats_device.argtypes = [vp, vp, i64, i64, vp, i64, i64, i32, i32, vp]
    lib.pqa_level_stats.argtypes = [vp, C.POINTER(vp), i64, C.POINTER(vp), i64, i32, i32, vp]
    lib.pqa_level_bins.argtypes = [vp]
    lib.pqa_resample.argtypes = [vp, C.POINTER(PqaResampleSpec), C.POINTER(vp), i64, C.POINTER(vp), i64, i32]
    lib.pqa_resample_device.argtypes = [vp, C.POINTER(PqaResampleSpec), vp, i64, i64, vp, i64, i64, i32]
    lib.pqa_unpack_device.argtypes = [vp, C.POINTER(PqaUnpackSpec), vp, i64, i64, i32, C.POINTER(PqaDeviceClip)]
    lib.pqa_format_convert.argtypes = [vp, C.POINTER(PqaConvertSpec), C.POINTER(vp), i64, C.POINTER(vp), i64, i32]
    lib.pqa_format_convert_device.argtypes = [vp, C.POINTER(PqaConvertSpec), vp, i64, i64, vp, i64, i64, i32]
    lib.pqa_rgb_convert_device.argtypes = [vp, C.POINTER(PqaRgbSpec), vp, i64, i64, i32, C.POINTER(PqaDeviceClip)]
    lib.pqa_rgb_convert.argtypes = [vp, C.POINTER(PqaRgbSpec), C.POINTER(vp), i64, i32, C.POINTER(vp), C.POINTER(i64 * 3)]
    lib.pqa_table_apply.argtypes = [vp, C.POINTER(PqaTableSpec), vp, C.POINTER(vp), i64, C.POINTER(vp), i64, i32]
    lib.pqa_table_apply_device.argtypes = [vp, C.POINTER(PqaTableSpec), vp, vp, i64, i64, vp, i64, i64, i32]
    lib.pqa_deinterlace.argtypes = [vp, C.POINTER(PqaDeintSpec), C.POINTER(vp), i64, C.POINTER(vp), i64, i32]
    lib.pqa_deinterlace_device.argtypes = [vp, C.POINTER(PqaDeintSpec), vp, i64, i64, vp, i64, i64, i32]
    for fn in (lib.pqa_deint_chunk, lib.pqa_deint_block_bytes, lib.pqa_deint_block_rows):
        fn.argtypes, fn.restype = [], C.c_int
    lib.pqa_mask_blend.argtypes = [vp, C.POINTER(PqaMaskSpec), vp, C.POINTER(vp), i64, C.POINTER(vp), i64, C.POINTER(vp), i64, i32]
    lib.pqa_mask_blend_device.argtypes = [vp, C.POINTER(PqaMaskSpec), vp, vp, i64, i64, vp, i64, i64, vp, i64, i64, i32]
    lib.pqa_unpack.argtypes = [vp, C.POINTER(PqaUnpackSpec), C.POINTER(vp), i64, i32, C.POINTER(vp), C.POINTER(i64 * 3)]
    lib.pqa_flow_moments.argtypes = [vp, C.POINTER(PqaFlowSpec), C.POINTER(vp), i64, C.POINTER(vp), i64, i32, vp]
    lib.pqa_flow_moments_device.argtypes = [vp, C.POINTER(PqaFlowSpec), vp, i64, i64, vp, i64, i64, i32, vp]
    lib.pqa_line_profiles.argtypes = [vp, C.POINTER(PqaProfileSpec), C.POINTER(vp), i64, i32, vp]
    lib.pqa_line_profiles_device.argtypes = [vp, C.POINTER(PqaProfileSpec), vp, i64, i64, i32, vp]
    lib.pqa_tile_moments.argtypes = [vp, C.POINTER(PqaTileSpec), C.POINTER(vp), i64, C.POINTER(vp), i64, i32, vp]
    lib.pqa_tile_moments_device.argtypes = [vp, C.POINTER(PqaTileSpec), vp, i64, i64, vp, i64, i64, i32, vp]
    lib.pqa_band_moments.argtypes = [vp, C.POINTER(PqaBandSpec), C.POINTER(vp), i64, C.POINTER(vp), i64, i32, vp]
    lib.pqa_band_moments_device.argtypes = [vp, C.POINTER(PqaBandSpec), vp, i64, i64, vp, i64, i64, i32, vp]
    lib.pqa_temporal_moments.argtypes = [vp, C.POINTER(PqaTemporalSpec), C.POINTER(vp), i64, C.POINTER(vp), i64, i32, vp]
    lib.pqa_temporal_moments_device.argtypes = [vp, C.POINTER(PqaTemporalSpec), vp, i64, i64, vp, i64, i64, i32, vp]
    lib.pqa_temporal_sums.argtypes = []
    lib.pqa_field_moments.argtypes = [vp, C.POINTER(PqaFieldSpec), C.POINTER(vp), i64, C.POINTER(vp), i64, i32, vp]
    lib.pqa_field_moments_device.argtypes = [vp, C.POINTER(PqaFieldSpec), vp, i64, i64, vp, i64, i64, i32, vp]
    lib.pqa_temporal_sums.restype = C.c_int
    lib.pqa_edge_profiles.argtypes = [vp, C.POINTER(PqaEdgeSpec), C.POINTER(vp), i64, C.POINTER(vp), i64, i32, vp]
    lib.pqa_edge_profiles_device.argtypes = [vp, C.POINTER(PqaEdgeSpec), vp, i64, i64, vp, i64, i64, i32, vp]
    lib.pqa_edge_sums.argtypes = []
    lib.pqa_edge_sums.restype = C.c_int
    lib.pqa_band_sums.argtypes = []
    lib.pqa_band_sums.restype = C.c_int
    lib.pqa_colour_sums.argtypes = []
    lib.pqa_colour_sums.restype = C.c_int
    lib.pqa_colour_moments_device.argtypes = [vp, C.POINTER(PqaDeviceClip), C.POINTER(PqaDeviceClip), i32, C.c_uint32, C.c_uint32, vp]
    lib.pqa_colour_moments.argtypes = [vp, C.POINTER(vp), C.POINTER(i64 * 3), C.POINTER(vp), C.POINTER(i64 * 3), i32, C.c_uint32, C.c_uint32, vp]
    lib.pqa_colour_apply_device.argtypes = [vp, C.POINTER(i32 * 12), C.POINTER(PqaDeviceClip), C.POINTER(PqaDeviceClip), i32]
    lib.pqa_colour_apply.argtypes = [vp, C.POINTER(i32 * 12), C.POINTER(vp), C.POINTER(i64 * 3), C.POINTER(vp), C.POINTER(i64 * 3), i32]
    lib.pqa_itp_sums.argtypes = []
    lib.pqa_itp_sums.restype = C.c_int
    lib.pqa_delta_itp_device.argtypes = [vp, C.POINTER(PqaItpSpec), C.POINTER(PqaDeviceClip), C.POINTER(PqaDeviceClip), i32, vp]
    lib.pqa_delta_itp.argtypes = [vp, C.POINTER(PqaItpSpec), C.POINTER(vp), C.POINTER(i64 * 3), C.POINTER(vp), C.POINTER(i64 * 3), i32, vp]
    lib.pqa_debug_itp.argtypes = [C.POINTER(PqaItpSpec), vp, i32, vp]
    lib.pqa_debug_colour.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(vp * 3), C.POINTER(vp * 3),
                                     C.c_uint32, C.c_uint32, vp, C.POINTER(i32 * 12), C.POINTER(vp * 3)]
    lib.pqa_debug_resample_table.argtypes = [C.c_uint32, i32, i32, i64, i64, vp, vp, i32, C.POINTER(i32)]
    lib.pqa_set_luma_gray.argtypes = [vp, C.c_uint32]
    lib.pqa_reset.argtypes = [vp]
    lib.pqa_last_error.argtypes = [vp]
    lib.pqa_last_error.restype = C.c_char_p
    lib.pqa_profile_enable.argtypes = [vp, C.c_int]
    lib.pqa_profile_read.argtypes = [vp, C.c_int, C.POINTER(dbl), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.pqa_debug_vif_march_table.argtypes = [vp, i32]
    lib.pqa_debug_vif_march_shape.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(i32 * 6)]
    lib.pqa_debug_vif_strip_shape.argtypes = [vp, C.c_uint32, C.c_uint32, C.POINTER(i32 * 4)]
    lib.pqa_debug_adm_need.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(i32 * 20)]
    lib.pqa_debug_partial_counts.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(i32 * PARTIAL_COUNT_INTS), i32]
    lib.pqa_debug_ciede2000.argtypes = [vp, i32, vp]
    lib.pqa_debug_cambi_params.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, vp, i32]
    lib.pqa_debug_cambi_cmap.argtypes = [vp, C.c_int64, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_int64, vp]
    lib.pqa_debug_psnr_hvs_dct8x8.argtypes = [vp, vp, i32]
    lib.pqa_debug_psnr_hvs_tables.argtypes = [vp, i32]
    lib.pqa_debug_psnr_hvs_plane.argtypes = [vp, vp, C.c_int64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp]
    lib.pqa_debug_xpsnr_blocks.argtypes = [vp, vp, vp, vp, C.c_int64, C.c_uint32, C.c_uint32, C.c_uint32, i32, vp, vp]
    lib.pqa_debug_siti_plane.argtypes = [vp, vp, C.c_int64, C.c_uint32, C.c_uint32, C.c_uint32, i32, vp, vp]
    lib.pqa_profile_kernel_name.argtypes = [C.c_int]
    lib.pqa_profile_kernel_name.restype = C.c_char_p
    assert lib.pqa_record_doubles() == RECORD_DOUBLES
    assert lib.pqa_ext_doubles() == EXT_DOUBLES
    assert lib.pqa_ext2_doubles() == EXT2_DOUBLES
    assert lib.pqa_ext3_doubles() == EXT3_DOUBLES
    assert lib.pqa_ext4_doubles() == EXT4_DOUBLES
    assert lib.pqa_ext5_doubles() == EXT5_DOUBLES
    assert lib.pqa_colour_sums() == COLOUR_SUMS
    assert lib.pqa_itp_sums() == ITP_SUMS
    _lib = lib
    return lib
