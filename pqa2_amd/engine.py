"""FeatureEngine: thin Python owner of one pqa_ctx (one per GPU).

Frames go in as numpy planes (host path, `submit`) or as a torch CUDA tensor that already holds a
whole clip in HBM (`submit_resident`); per-frame feature records come back as a [n, 24] float64
array.  All arithmetic happens in the HIP kernels behind the C ABI (include/pqa_vmaf.h).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _native as N


_PARKED = {}   # at most one entry: configuration bytes -> (library, context) parked by FeatureEngine.release()


def _take_parked(key):
    hit = _PARKED.pop(key, None)
    return hit[1] if hit else None


def clear_parked():
    """Destroy the context FeatureEngine.release() parked (also runs at interpreter exit)."""
    while _PARKED:
        _, (lib, ctx) = _PARKED.popitem()
        try:
            lib.pqa_destroy(ctx)
        except Exception:
            pass


def _park(lib, key, ctx):
    clear_parked()            # one per process: whatever was parked before goes
    if not _PARKED_HOOK:
        import atexit
        atexit.register(clear_parked)
        _PARKED_HOOK.append(True)
    _PARKED[key] = (lib, C.c_void_p(ctx.value))


_PARKED_HOOK = []


def _tiles_out(n, sp, sums, dtype=np.uint64):
    t = sp.tile if sp.tile in N.FLOW_TILES else 64     # a bad tile is the library's to refuse
    return np.zeros((max(int(n), 0), -(-sp.height // t), -(-sp.width // t), sums), dtype)


def _lines_out(n, sp, sums):
    return np.zeros((max(int(n), 0), sp.height + sp.width, sums), np.uint64)


def _bands_out(n, sp):
    lv = sp.levels if 1 <= sp.levels <= 6 else 1      # a bad count is the library's to refuse
    return np.zeros((max(int(n), 0), lv, 4, N.BAND_SUMS), np.uint64)


# The spec-driven analyses, pqa_<name> and pqa_<name>_device: (spec class, its third field, the zeroed result of n frames)
_ANALYSES = {
    "flow_moments": (N.PqaFlowSpec, "tile", lambda n, sp: _tiles_out(n, sp, 6, np.int64)),
    "tile_moments": (N.PqaTileSpec, "tile", lambda n, sp: _tiles_out(n, sp, N.TILE_SUMS)),
    "band_moments": (N.PqaBandSpec, "levels", _bands_out),
    "temporal_moments": (N.PqaTemporalSpec, "tile", lambda n, sp: _tiles_out(int(n) - 1, sp, N.TEMPORAL_SUMS)),
    "line_profiles": (N.PqaProfileSpec, None, lambda n, sp: _lines_out(n, sp, 2)),
    "field_moments": (N.PqaFieldSpec, None, lambda n, sp: np.zeros((max(int(n) - 1, 0), N.FIELD_SUMS), np.uint64)),
    "edge_profiles": (N.PqaEdgeSpec, None, lambda n, sp: _lines_out(n, sp, N.EDGE_SUMS)),
}


class FeatureEngine:
    def __init__(self, width: int, height: int, bit_depth: int = 8, n_planes: int = 1,
                 chroma_shift=(1, 1), features: int = N.FEAT_VMAF, device: int = 0, max_batch: int = 0,
                 result_capacity: int = 16384, n_subsample: int = 1,
                 vif_enhn_gain_limit: float = 100.0, adm_enhn_gain_limit: float = 100.0,
                 vif_border: int = N.VIF_BORDER_FLOAT, fixed_point: int = 0, reuse: bool = False):
        self.lib = N.load()
        cfg = N.PqaConfig()
        self.lib.pqa_config_init(C.byref(cfg), width, height)
        cfg.device = device
        cfg.bit_depth = bit_depth
        cfg.n_planes = n_planes
        cfg.chroma_hshift, cfg.chroma_vshift = chroma_shift
        self.chroma_shift = (int(chroma_shift[0]), int(chroma_shift[1]))
        cfg.features = features
        cfg.max_batch = max_batch
        cfg.result_capacity = result_capacity
        cfg.n_subsample = n_subsample
        cfg.vif_enhn_gain_limit = vif_enhn_gain_limit
        cfg.adm_enhn_gain_limit = adm_enhn_gain_limit
        cfg.vif_border = vif_border
        cfg.fixed_point = int(fixed_point)
        self.cfg = cfg
        self.width, self.height, self.bit_depth, self.n_planes = width, height, bit_depth, n_planes
        self.dtype = np.uint8 if bit_depth <= 8 else np.dtype("<u2")
        self._ctx = C.c_void_p()
        self.luma_gray = N.GRAY_LUMA   # mirror of the context's sticky gray mode (pqa_set_luma_gray)
        self._key = bytes(cfg)         # every field of the configuration: what a parked context must match
        parked = _take_parked(self._key) if reuse else None
        if parked is not None:         # a context release() parked: same configuration, back to its initial state
            self._ctx = parked
            if self.lib.pqa_reset(self._ctx) == N.PQA_OK and self.lib.pqa_set_luma_gray(self._ctx, N.GRAY_LUMA) == N.PQA_OK:
                return
            self.lib.pqa_destroy(self._ctx)
            self._ctx = C.c_void_p()
        rc = self.lib.pqa_create(C.byref(cfg), C.byref(self._ctx))
        if rc != N.PQA_OK:
            raise N.PqaError(rc, (self.lib.pqa_last_error(None) or b"").decode())

    # -- lifetime ----------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_ctx", None) is not None and self._ctx.value:
            self.lib.pqa_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def release(self):
        """Like close(), but a healthy context is PARKED for the next FeatureEngine(..., reuse=True) of the very same
        configuration instead of being destroyed (the reference's caller makes a fresh analyzer per run,
        app/ui/tabs/analysis_tab.py:588: creating and destroying a 2160p context costs ~7 ms of a 180 ms analysis).  One
        context per process is kept; it is destroyed when another one is parked, by clear_parked(), or at interpreter exit.
        PQA_CONTEXT_CACHE=0 turns parking off.  Call only after a successful run: a context that reported an error is closed."""
        if getattr(self, "_ctx", None) is None or not self._ctx.value:
            return
        if os.environ.get("PQA_CONTEXT_CACHE", "1") == "0":
            return self.close()
        _park(self.lib, self._key, self._ctx)
        self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc: int):
        if rc == N.PQA_OK:
            return
        msg = (self.lib.pqa_last_error(self._ctx) or b"").decode()
        raise (N.PqaCancelled if rc == N.PQA_ECANCELLED else N.PqaError)(rc, msg)

    # -- marshalling: planes going in, planes coming out, clips in HBM -------------------------
    @staticmethod
    def _host_planes(frames, dtype, what, shapes=None, k=None, step=None):
        """(arrays kept alive, pointer array, row stride of every plane kind as a c_int64 triple) of planes in host memory:
        a list of planes (k None) or of frames of k planes, whose pointers lie `step` (default k) apart in the array.  The one
        rule: the planes are handed over as they lie only if every one of them is 2-D, has `dtype`, a unit column stride and
        a POSITIVE row stride equal to that of the same plane kind in the first frame; otherwise all become packed copies.
        Then the sizes: shapes[p] is the (height, width) a plane of kind p must have, None for the first frame's (shapes
        None: 2-D is all that is asked); `what` is the ValueError's text, formatted with i (frame), p (plane), got, want.
        No frames: an array of one null pointer and the row bytes of shapes[p], 0 where there is none."""
        dtype = np.dtype(dtype)
        arrs = [[np.asarray(f)] if k is None else [np.asarray(f[p]) for p in range(k)] for f in frames]
        k = k or 1
        if not all(a.ndim == 2 and a.dtype == dtype and a.strides[1] == a.itemsize and 0 < a.strides[0] == arrs[0][p].strides[0]
                   for f in arrs for p, a in enumerate(f)):
            arrs = [[np.ascontiguousarray(a, dtype=dtype) for a in f] for f in arrs]
        want = [None if shapes is None else arrs[0][p].shape if arrs and shapes[p] is None else shapes[p] for p in range(k)]
        step = step or k
        ptrs = (C.c_void_p * max(len(arrs) * step, 1))()
        for i, f in enumerate(arrs):
            for p, a in enumerate(f):
                if a.ndim != 2 or (want[p] is not None and a.shape != tuple(want[p])):
                    raise ValueError(what.format(i=i, p=p, got=a.shape, want=want[p]))
                ptrs[i * step + p] = a.ctypes.data
        strides = [arrs[0][p].strides[0] if arrs else (int(want[p][1]) * dtype.itemsize if want[p] is not None else 0) for p in range(k)]
        return [a for f in arrs for a in f], ptrs, (C.c_int64 * 3)(*strides)

    @staticmethod
    def _outputs(n, shapes, dtype, planes=None):
        """(new arrays, frame by frame; their pointer array; the row bytes of every plane kind as a c_int64 triple) of n output
        frames that hold the first `planes` (default: all) of the plane kinds `shapes`; one kind: a pointer a frame, more: three"""
        planes, step = planes or len(shapes), 1 if len(shapes) == 1 else 3
        out = [np.empty(shapes[p], dtype) for _ in range(n) for p in range(planes)]
        ptrs = (C.c_void_p * max(n * step, 1))()
        for j, o in enumerate(out):
            ptrs[j // planes * step + j % planes] = o.ctypes.data
        return out, ptrs, (C.c_int64 * 3)(*[int(s[1]) * np.dtype(dtype).itemsize for s in shapes])

    @staticmethod
    def _device_clip(ptrs, row_pitch, frame_pitch, count=3):
        """the pqa_device_clip of the first `count` planes of a clip in HBM (0 or None: a null plane)"""
        d = N.PqaDeviceClip()
        for p in range(count):
            d.plane[p], d.row_pitch[p], d.frame_pitch[p] = ptrs[p] or None, row_pitch[p], frame_pitch[p]
        return d

    # -- host path ---------------------------------------------------------------------------
    def submit(self, index: int, ref_planes, dis_planes):
        """ref_planes / dis_planes: sequences of 2-D numpy arrays (Y[,U,V]) of this engine's dtype."""
        keep_r, rp, rs = self._planes(ref_planes)
        keep_d, dp, ds = self._planes(dis_planes)
        self._check(self.lib.pqa_submit(self._ctx, index, C.byref(rp), C.byref(rs), C.byref(dp), C.byref(ds)))

    def submit_file(self, index: int, ref_fd: int, ref_offsets, dis_fd: int, dis_offsets):
        """A frame pair lying in two files as packed planes (pqa_submit_fd): *_offsets = byte offset of each plane."""
        S = C.c_int64 * 3
        ro, do = S(), S()
        for p in range(self.n_planes):
            ro[p], do[p] = int(ref_offsets[p]), int(dis_offsets[p])
        self._check(self.lib.pqa_submit_fd(self._ctx, index, int(ref_fd), C.byref(ro), int(dis_fd), C.byref(do)))

    def submit_file_run(self, first_index: int, n_frames: int, ref_fd: int, ref_offsets, ref_frame_stride: int,
                        dis_fd: int, dis_offsets, dis_frame_stride: int):
        """n_frames consecutive frame pairs of two files (pqa_submit_fd_run): frame first_index + k has plane p at
        *_offsets[p] + k * *_frame_stride.  The library pipelines reading and upload inside the call."""
        ro = (C.c_int64 * 3)(*[int(x) for x in list(ref_offsets) + [0] * (3 - len(ref_offsets))])
        do = (C.c_int64 * 3)(*[int(x) for x in list(dis_offsets) + [0] * (3 - len(dis_offsets))])
        self._check(self.lib.pqa_submit_fd_run(self._ctx, int(first_index), int(n_frames), int(ref_fd), C.byref(ro),
                                               int(ref_frame_stride), int(dis_fd), C.byref(do), int(dis_frame_stride)))

    def set_motion_halo(self, prev_ref_luma: np.ndarray | None):
        if prev_ref_luma is None:
            self._check(self.lib.pqa_set_motion_halo(self._ctx, None, 0))
            return
        a = np.ascontiguousarray(prev_ref_luma, dtype=self.dtype)
        self._check(self.lib.pqa_set_motion_halo(self._ctx, a.ctypes.data, a.strides[0]))

    def set_ref_history(self, prev_ref_lumas):
        """The reference luma planes in front of the next submitted frame: [frame first-1, frame first-2] (at most two;
        an empty list restarts the chain).  Arms motion's halo from the first and xpsnr's temporal history from both
        (pqa_set_ref_history)."""
        planes = [np.ascontiguousarray(p, dtype=self.dtype) for p in prev_ref_lumas]
        if len(planes) > 2:
            raise ValueError("set_ref_history takes at most two planes")
        ptrs = (C.c_void_p * 2)(*([p.ctypes.data for p in planes] + [None] * (2 - len(planes))))
        stride = planes[0].strides[0] if planes else 0
        self._check(self.lib.pqa_set_ref_history(self._ctx, ptrs, len(planes), stride))

    def set_dis_history(self, prev_dis_luma: np.ndarray | None):
        """The distorted luma plane in front of the next submitted frame (frame first-1), from which siti's TI of the
        distorted clip continues; None restarts that chain (pqa_set_dis_history)."""
        if prev_dis_luma is None:
            self._check(self.lib.pqa_set_dis_history(self._ctx, None, 0))
            return
        a = np.ascontiguousarray(prev_dis_luma, dtype=self.dtype)
        self._check(self.lib.pqa_set_dis_history(self._ctx, a.ctypes.data, a.strides[0]))

    def _planes(self, planes):
        """(keep-alive arrays, pointer triple, stride triple) of the first n_planes planes of a frame."""
        return self._host_planes([planes], self.dtype, "a frame needs 2-D planes", k=self.n_planes, step=3)

    def set_dis_history_planes(self, prev_dis_planes):
        """Every plane of the distorted frame in front of the next submitted frame (frame first-1): the integrity
        feature's differences continue from it, and so does siti's TI of the distorted clip; None restarts both chains
        (pqa_set_dis_history_planes)."""
        if prev_dis_planes is None:
            self._check(self.lib.pqa_set_dis_history_planes(self._ctx, None, None))
            return
        keep, pp, ss = self._planes(prev_dis_planes)
        self._check(self.lib.pqa_set_dis_history_planes(self._ctx, C.byref(pp), C.byref(ss)))

    def set_black_threshold(self, threshold: int):
        """The integer sample value at or below which a luma sample counts as black (pqa_set_black_threshold); legal
        before the first submit and after reset()."""
        self._check(self.lib.pqa_set_black_threshold(self._ctx, int(threshold)))

    def frame_sad(self, anchor_planes, frames) -> np.ndarray:
        """[n, 3] uint64: the exact SAD of every plane of each frame in `frames` (sequences of Y[,U,V] numpy planes in
        host memory) against the anchor frame's (pqa_frame_sad; synchronous, 0 for planes the engine does not have)."""
        n = len(frames)
        out = np.zeros((n, 3), np.uint64)
        if n == 0:
            return out
        keep_a, ap, as_ = self._planes(anchor_planes)
        keep, ptrs, strides = self._host_planes(frames, self.dtype, "a frame needs 2-D planes", k=self.n_planes, step=3)
        self._check(self.lib.pqa_frame_sad(self._ctx, C.byref(ap), C.byref(as_), ptrs, C.byref(strides), n, out.ctypes.data))
        return out

    def frame_sad_resident(self, anchor_ptrs, anchor_row_pitch, frame_ptrs, row_pitch, frame_pitch, n_frames: int) -> np.ndarray:
        """[n, 3] uint64 like frame_sad() for a clip in HBM (frame_ptrs: device addresses of frame 0's planes) against an
        anchor frame in HBM; pitches in bytes per plane (pqa_frame_sad_device)."""
        out = np.zeros((n_frames, 3), np.uint64)
        ap, as_ = (C.c_void_p * 3)(*anchor_ptrs[:self.n_planes]), (C.c_int64 * 3)(*anchor_row_pitch[:self.n_planes])
        d = self._device_clip(frame_ptrs, row_pitch, frame_pitch, self.n_planes)
        self._check(self.lib.pqa_frame_sad_device(self._ctx, C.byref(ap), C.byref(as_), C.byref(d), n_frames, out.ctypes.data))
        return out

    # -- device-resident path ------------------------------------------------------------------
    def submit_resident(self, first_index: int, n_frames: int, ref_ptrs, dis_ptrs, row_pitch, frame_pitch,
                        prev_ref_luma_ptr: int = 0, prev_row_pitch: int = 0):
        """ref_ptrs/dis_ptrs: device addresses of frame 0's planes; pitches in bytes per plane."""
        r = self._device_clip(ref_ptrs, row_pitch, frame_pitch, self.n_planes)
        d = self._device_clip(dis_ptrs, row_pitch, frame_pitch, self.n_planes)
        self._check(self.lib.pqa_submit_device(self._ctx, first_index, n_frames, C.byref(r), C.byref(d),
                                               prev_ref_luma_ptr or None, prev_row_pitch))

    @staticmethod
    def surface_clip(fmt: int, luma_ptr: int, luma_row_pitch: int, luma_frame_pitch: int, chroma_ptr: int = 0,
                     chroma_row_pitch: int = 0, chroma_frame_pitch: int = 0) -> "N.PqaSurfaceClip":
        """A clip of decoder surfaces in device memory (NV12 / P010 / P012; pitches in bytes)."""
        s = N.PqaSurfaceClip()
        s.struct_size = C.sizeof(N.PqaSurfaceClip)
        s.format = fmt
        s.luma, s.chroma = luma_ptr or None, chroma_ptr or None
        s.luma_row_pitch, s.luma_frame_pitch = luma_row_pitch, luma_frame_pitch
        s.chroma_row_pitch, s.chroma_frame_pitch = chroma_row_pitch, chroma_frame_pitch
        return s

    def submit_surfaces(self, first_index: int, n_frames: int, ref: "N.PqaSurfaceClip", dis: "N.PqaSurfaceClip",
                        prev_ref: "N.PqaSurfaceClip | None" = None):
        """Frames as a hardware decoder leaves them (pqa_submit_surfaces): NV12 luma is scored in place, interleaved
        chroma is split and 16-bit samples are shifted down on the device."""
        self._check(self.lib.pqa_submit_surfaces(self._ctx, first_index, n_frames, C.byref(ref), C.byref(dis),
                                                 C.byref(prev_ref) if prev_ref is not None else None))

    # -- packed capture formats ----------------------------------------------------------------
    @staticmethod
    def _packed_format(fmt) -> int:
        """PQA_SURFACE_* of a packed format given by name ("uyvy422", "yuyv422", "v210") or by constant"""
        f = N.PACKED_FORMATS.get(fmt, fmt) if isinstance(fmt, str) else fmt
        if f not in N.PACKED_BIT_DEPTH:
            raise ValueError(f"packed format must be one of {sorted(N.PACKED_FORMATS)}, not {fmt!r}")
        return int(f)

    @staticmethod
    def _unpack_spec(fmt: int, shape):
        sp = N.PqaUnpackSpec()
        sp.struct_size, sp.format = C.sizeof(N.PqaUnpackSpec), fmt
        sp.width, sp.height = max(0, int(shape[1])), max(0, int(shape[0]))
        return sp

    def unpack(self, frames, fmt, shape, luma_only: bool = False):
        """A list of (Y, U, V) -- or (Y,) with luma_only -- per frame: packed capture frames in HOST memory unpacked on the
        GPU (pqa_unpack).  frames: 2-D uint8 arrays of packed rows (the rows of a frame may be padded; v210: 4-byte
        aligned); fmt: "uyvy422", "yuyv422" or "v210"; shape = (height, width) of the luma plane.  Y is height x width, U and
        V are height x ceil(width / 2); uint8, v210: uint16 values 0 ... 1023.  The size is the call's own."""
        f = self._packed_format(fmt)
        keep, sptr, ss = self._host_planes(frames, np.uint8, "unpack needs 2-D arrays of packed rows of one size", [None])
        sp = self._unpack_spec(f, shape)
        h, w = int(shape[0]), int(shape[1])
        n, cw, k = len(keep), (w + 1) // 2, 1 if luma_only else 3
        out, dptr, ds = self._outputs(n, [(h, w), (h, cw), (h, cw)], np.uint16 if N.PACKED_BIT_DEPTH[f] > 8 else np.uint8, k)
        self._check(self.lib.pqa_unpack(self._ctx, C.byref(sp), sptr, ss[0], n, dptr, C.byref(ds)))
        return [tuple(out[i * k:(i + 1) * k]) for i in range(n)]

    def unpack_resident(self, fmt, shape, src_ptr: int, src_row_pitch: int, src_frame_pitch: int, n_frames: int, dst_ptrs,
                        dst_row_pitch, dst_frame_pitch):
        """The same for frames in HBM (device pointers, pitches in bytes; pqa_unpack_device): n_frames packed frames at
        src_ptr become the planes at dst_ptrs = (Y, U, V) or (Y,) for luma only.  Nothing crosses PCIe; the planes can go
        straight into submit_resident or any *_resident analysis."""
        sp = self._unpack_spec(self._packed_format(fmt), shape)
        d = self._device_clip(dst_ptrs, dst_row_pitch, dst_frame_pitch, len(dst_ptrs))
        self._check(self.lib.pqa_unpack_device(self._ctx, C.byref(sp), src_ptr or None, src_row_pitch, src_frame_pitch, int(n_frames),
                                               C.byref(d)))

    # -- pixel-format conversion ---------------------------------------------------------------
    @staticmethod
    def _convert_spec(luma_shape, src, dst, generic: bool):
        """the pqa_convert_spec of planes of a luma_shape = (height, width) frame; src / dst = (hshift, vshift, hsite, vsite, bits)"""
        sp = N.PqaConvertSpec()
        sp.struct_size, sp.flags = C.sizeof(N.PqaConvertSpec), N.CONVERT_GENERIC if generic else 0
        sp.luma_width, sp.luma_height = max(0, int(luma_shape[1])), max(0, int(luma_shape[0]))
        # a value the library must refuse still has to fit its field
        sp.src_hshift, sp.src_vshift, sp.src_hsite, sp.src_vsite = (int(v) & 0xFF for v in src[:4])
        sp.dst_hshift, sp.dst_vshift, sp.dst_hsite, sp.dst_vsite = (int(v) & 0xFF for v in dst[:4])
        sp.src_bits, sp.dst_bits = max(0, int(src[4])), max(0, int(dst[4]))
        return sp

    @staticmethod
    def convert_plane_shape(luma_shape, hshift: int, vshift: int):
        """(rows, samples a row) of a plane of chroma shifts (hshift, vshift) in a frame of luma_shape = (height, width)"""
        return -(-int(luma_shape[0]) >> vshift), -(-int(luma_shape[1]) >> hshift)

    def format_convert(self, frames, luma_shape, src, dst, generic: bool = False):
        """A list of 2-D arrays: every plane of `frames` (planes of ONE kind, of a frame of luma_shape = (height, width), in HOST
        memory) converted from the layout src = (hshift, vshift, hsite, vsite, bits) to dst = (...) in one pass with one
        rounding (pqa_format_convert; definition: include/pqa_vmaf.h).  Shifts 0 ... 2, sitings N.SITE_COSITED / N.SITE_CENTRE
        (void where the shift is 0), bits 8 / 10 / 12 (uint8 at 8 bit, else uint16).  A luma plane is (0, 0, *, *, bits) on both
        sides: a depth change only.  generic: the general kernel whatever the layout (the same integers).  Sizes and sample
        formats are the call's own, not this context's."""
        sp = self._convert_spec(luma_shape, src, dst, generic)
        sdt = np.uint8 if int(src[4]) <= 8 else np.dtype("<u2")
        ddt = np.uint8 if int(dst[4]) <= 8 else np.dtype("<u2")
        src_shape = self.convert_plane_shape(luma_shape, int(src[0]) & 3, int(src[1]) & 3)
        keep, sptr, ss = self._host_planes(frames, sdt, f"format_convert needs 2-D planes of {src_shape[0]} x {src_shape[1]} samples", [src_shape])
        out, dptr, ds = self._outputs(len(keep), [self.convert_plane_shape(luma_shape, int(dst[0]) & 3, int(dst[1]) & 3)], ddt)
        self._check(self.lib.pqa_format_convert(self._ctx, C.byref(sp), sptr, ss[0], dptr, ds[0], len(keep)))
        return out

    def format_convert_resident(self, luma_shape, src, dst, src_ptr: int, src_row_pitch: int, src_frame_pitch: int, dst_ptr: int,
                                dst_row_pitch: int, dst_frame_pitch: int, n_frames: int, generic: bool = False):
        """The same for planes in HBM (device pointers, pitches in bytes; pqa_format_convert_device): n_frames planes at
        src_ptr become the planes at dst_ptr.  Nothing crosses PCIe; the result can go into submit_resident."""
        sp = self._convert_spec(luma_shape, src, dst, generic)
        self._check(self.lib.pqa_format_convert_device(self._ctx, C.byref(sp), src_ptr or None, src_row_pitch, src_frame_pitch,
                                                       dst_ptr or None, dst_row_pitch, dst_frame_pitch, int(n_frames)))

    # -- packed RGB captures -------------------------------------------------------------------
    @staticmethod
    def _rgb_spec(fmt, shape, dst, m, generic: bool):
        """the pqa_rgb_spec of frames of shape = (height, width); dst = (hshift, vshift, hsite, vsite, bits); m: 12 Q14 integers"""
        from . import rgb as R
        if isinstance(fmt, str) and fmt not in R.FORMATS:
            raise ValueError(f"unknown packed RGB format {fmt!r} (one of {', '.join(R.FORMATS)})")
        sp = N.PqaRgbSpec()
        sp.struct_size, sp.format = C.sizeof(N.PqaRgbSpec), R.FORMATS[fmt] if isinstance(fmt, str) else max(0, int(fmt))
        sp.width, sp.height = max(0, int(shape[1])), max(0, int(shape[0]))
        # a value the library must refuse still has to fit its field
        sp.hshift, sp.vshift, sp.hsite, sp.vsite = (int(v) & 0xFFFFFFFF for v in dst[:4])
        sp.dst_bits, sp.flags = max(0, int(dst[4])), N.RGB_GENERIC if generic else 0
        if len(m) != 12:
            raise ValueError("rgb_convert needs a matrix of 12 integers (rows of offset, R, G, B in Q14)")
        for k, v in enumerate(m):
            sp.m[k] = int(v)
        return sp

    def rgb_convert(self, frames, fmt, shape, dst, m, luma_only: bool = False, generic: bool = False):
        """A list of [Y, U, V] -- or [Y] with luma_only -- per frame: packed RGB frames in HOST memory converted on the GPU
        (pqa_rgb_convert; definition: include/pqa_vmaf.h).  frames: 2-D uint8 arrays of packed rows (the rows of a frame may be
        padded; r210: 4-byte aligned); fmt: "bgra", "argb", "rgba", "abgr" or "r210"; shape = (height, width) in pixels;
        dst = (hshift, vshift, hsite, vsite, bits), shifts 0 / 1, sitings N.SITE_COSITED / N.SITE_CENTRE, bits 8 / 10 (uint8,
        else uint16); m: the Q14 matrix (pqa2_amd.rgb.conversion_matrix).  generic: the general kernel whatever the layout
        (the same integers).  The size is the call's own, not this context's."""
        sp = self._rgb_spec(fmt, shape, dst, m, generic)
        keep, sptr, ss = self._host_planes(frames, np.uint8, "rgb_convert needs 2-D arrays of packed rows of one size", [None])
        h, w = int(shape[0]), int(shape[1])
        chroma = self.convert_plane_shape((h, w), int(dst[0]) & 1, int(dst[1]) & 1)
        n, k = len(keep), 1 if luma_only else 3
        out, dptr, ds = self._outputs(n, [(h, w), chroma, chroma], np.uint16 if int(dst[4]) > 8 else np.uint8, k)
        self._check(self.lib.pqa_rgb_convert(self._ctx, C.byref(sp), sptr, ss[0], n, dptr, C.byref(ds)))
        return [out[i * k:(i + 1) * k] for i in range(n)]

    def rgb_convert_resident(self, fmt, shape, dst, m, src_ptr: int, src_row_pitch: int, src_frame_pitch: int, n_frames: int, dst_ptrs,
                             dst_row_pitch, dst_frame_pitch, generic: bool = False):
        """The same for frames in HBM (device pointers, pitches in bytes; pqa_rgb_convert_device): n_frames packed frames at
        src_ptr become the planes at dst_ptrs = (Y, U, V) or (Y,) for luma only.  Nothing crosses PCIe; the planes can go
        straight into submit_resident or any *_resident analysis."""
        sp = self._rgb_spec(fmt, shape, dst, m, generic)
        d = self._device_clip(dst_ptrs, dst_row_pitch, dst_frame_pitch, len(dst_ptrs))
        self._check(self.lib.pqa_rgb_convert_device(self._ctx, C.byref(sp), src_ptr or None, src_row_pitch, src_frame_pitch, int(n_frames),
                                                    C.byref(d)))

    def _host_clip(self, side, keep):
        """the pqa_host_clip of one side of submit_packed: (frames, format name or None)"""
        frames, fmt = side
        h = N.PqaHostClip()
        h.struct_size = C.sizeof(N.PqaHostClip)
        if fmt is None or fmt == "planar":
            h.format = N.SURFACE_PLANAR
            arrs, ptrs, h.strides = self._host_planes(frames, self.dtype, "a frame needs 2-D planes", k=self.n_planes)
        else:
            h.format = self._packed_format(fmt)
            arrs, ptrs, h.strides = self._host_planes(frames, np.uint8, "submit_packed needs 2-D arrays of packed rows of one size", [None])
        keep += arrs
        keep.append(ptrs)
        h.frames = C.cast(ptrs, C.POINTER(C.c_void_p))
        return h

    def submit_packed(self, first_index: int, ref, dis):
        """Consecutive frame pairs from HOST memory where either side is a packed capture clip (pqa_submit_packed).  Each
        side is (frames, format): format "uyvy422", "yuyv422" or "v210" with frames = 2-D uint8 arrays of packed rows, or
        None for planar frames (sequences of Y[,U,V] planes as submit() takes them).  The packed bytes cross PCIe as they
        are and are unpacked on the GPU; on return the arrays may be reused."""
        if len(ref[0]) != len(dis[0]):
            raise ValueError("submit_packed needs as many reference as captured frames")
        keep = []
        r, d = self._host_clip(ref, keep), self._host_clip(dis, keep)
        self._check(self.lib.pqa_submit_packed(self._ctx, int(first_index), len(ref[0]), C.byref(r), C.byref(d)))

    def set_luma_gray(self, mode: int):
        """N.GRAY_LUMA: statistics of the luma samples; N.GRAY_BT601_FULL: of the limited -> full range gray the
        reference's cv2 path sees (8-bit units for every bit depth; thresholds in those units)."""
        self._check(self.lib.pqa_set_luma_gray(self._ctx, int(mode)))
        self.luma_gray = int(mode)

    def luma_stats_resident(self, luma_ptr: int, row_pitch: int, frame_pitch: int, n_frames: int,
                            threshold: int) -> np.ndarray:
        """[n,3] uint64 {sum, sum of squares, count(sample > threshold)} per frame of a clip in HBM."""
        out = np.zeros((n_frames, 3), np.uint64)
        self._check(self.lib.pqa_luma_stats_device(self._ctx, luma_ptr, row_pitch, frame_pitch, n_frames,
                                                   int(threshold), out.ctypes.data))
        return out

    def luma_stats(self, luma_frames, threshold: int) -> np.ndarray:
        """[n,3] uint64 {sum, sum of squares, count(sample > threshold)} for luma planes in HOST memory (a list of 2-D
        arrays of this engine's dtype with one common row stride; they are packed and uploaded by the library)."""
        n = len(luma_frames)
        out = np.zeros((n, 3), np.uint64)
        if n == 0:
            return out
        keep, ptrs, stride = self._luma_list(luma_frames, "luma")
        self._check(self.lib.pqa_luma_stats(self._ctx, ptrs, stride, n, int(threshold), out.ctypes.data))
        return out

    # -- temporal alignment ------------------------------------------------------------------
    def _luma_list(self, frames, what: str, shape=None):
        """(arrays kept alive, ctypes pointer array, common row stride) of luma planes (or planes of `shape`) in host memory"""
        arrs, ptrs, strides = self._host_planes(frames, self.dtype, what + " frame {i} is {got}, engine is {want}",
                                                [shape or (self.height, self.width)])
        return arrs, ptrs, strides[0]

    def cross_sse(self, ref_lumas, dis_lumas, k_lo: int, k_hi: int) -> np.ndarray:
        """[n_ref, k_hi - k_lo + 1] uint64: D[i][c] = sum (ref_i - dis_{i + k_lo + c})^2 over the luma plane, exact;
        UINT64_MAX where i + k_lo + c is no captured frame (pqa_cross_sse).  Luma planes in HOST memory (lists of 2-D
        arrays); every frame is uploaded once.  align.best_offset / align.frame_map read the result."""
        n_ref, n_dis = len(ref_lumas), len(dis_lumas)
        out = np.zeros((n_ref, max(int(k_hi) - int(k_lo) + 1, 1)), np.uint64)
        keep_r, rp, rs = self._luma_list(ref_lumas, "reference")
        keep_d, dp, ds = self._luma_list(dis_lumas, "captured")
        self._check(self.lib.pqa_cross_sse(self._ctx, rp, rs, n_ref, dp, ds, n_dis, int(k_lo), int(k_hi), out.ctypes.data))
        del keep_r, keep_d
        return out

    def cross_sse_resident(self, ref_ptr: int, ref_row_pitch: int, ref_frame_pitch: int, n_ref: int, dis_ptr: int,
                           dis_row_pitch: int, dis_frame_pitch: int, n_dis: int, k_lo: int, k_hi: int) -> np.ndarray:
        """The same for two clips in HBM (device pointers, pitches in bytes; pqa_cross_sse_device)."""
        out = np.zeros((n_ref, max(int(k_hi) - int(k_lo) + 1, 1)), np.uint64)
        self._check(self.lib.pqa_cross_sse_device(self._ctx, ref_ptr, ref_row_pitch, ref_frame_pitch, n_ref, dis_ptr,
                                                  dis_row_pitch, dis_frame_pitch, n_dis, int(k_lo), int(k_hi),
                                                  out.ctypes.data))
        return out

    # -- spatial alignment -------------------------------------------------------------------
    def shift_sse(self, ref_frames, dis_frames, radius: int) -> np.ndarray:
        """[n, 2R + 1, 2R + 1] uint64: S[f][j][i] = sum over the window R <= x < W - R, R <= y < H - R of
        (ref_f[y][x] - dis_f[y + j - R][x + i - R])^2, exact (pqa_shift_sse).  Luma planes in HOST memory (two lists of 2-D
        arrays of equal length).  align.best_shift reads the result."""
        n, R = len(ref_frames), int(radius)
        if len(dis_frames) != n:
            raise ValueError("shift_sse needs as many captured as reference frames")
        side = 2 * R + 1 if 0 <= R <= 16 else 1
        out = np.zeros((n, side, side), np.uint64)
        keep_r, rp, rs = self._luma_list(ref_frames, "reference")
        keep_d, dp, ds = self._luma_list(dis_frames, "captured")
        self._check(self.lib.pqa_shift_sse(self._ctx, rp, rs, dp, ds, n, R, out.ctypes.data))
        del keep_r, keep_d
        return out

    def shift_sse_resident(self, ref_ptr: int, ref_row_pitch: int, ref_frame_pitch: int, dis_ptr: int, dis_row_pitch: int,
                           dis_frame_pitch: int, n_frames: int, radius: int) -> np.ndarray:
        """The same for two clips in HBM (device pointers, pitches in bytes; pqa_shift_sse_device)."""
        R = int(radius)
        side = 2 * R + 1 if 0 <= R <= 16 else 1
        out = np.zeros((max(int(n_frames), 0), side, side), np.uint64)
        self._check(self.lib.pqa_shift_sse_device(self._ctx, ref_ptr, ref_row_pitch, ref_frame_pitch, dis_ptr, dis_row_pitch,
                                                  dis_frame_pitch, int(n_frames), R, out.ctypes.data))
        return out

    # -- level alignment ---------------------------------------------------------------------
    def plane_shape(self, plane: int):
        """(height, width) of plane 0 / 1 / 2 of this context in samples (chroma from chroma_shift, rounded up)"""
        if plane == 0:
            return (self.height, self.width)
        hs, vs = self.chroma_shift
        return ((self.height + (1 << vs) - 1) >> vs, (self.width + (1 << hs) - 1) >> hs)

    def _own_shape(self, name, frames, shape=None):
        """(height, width) of the planes of a call that brings its own size: `shape`, else the first frame's, else this context's"""
        if shape is None:
            shape = np.shape(frames[0]) if len(frames) else (self.height, self.width)
        if len(shape) != 2:
            raise ValueError(f"{name} needs 2-D planes")
        return tuple(int(v) for v in shape)

    def level_stats(self, ref_frames, dis_frames, plane: int = 0) -> np.ndarray:
        """[n, L, 3] uint64, L = 2^bit_depth: T[f][v] = (count, sum of dis, sum of dis^2) over the pixels of pair f whose
        reference sample is v, exact (pqa_level_stats).  Planes in HOST memory (two lists of 2-D arrays of equal length,
        each of the size of `plane` of this context).  align.best_levels reads the result."""
        n, plane = len(ref_frames), int(plane)
        if len(dis_frames) != n:
            raise N.PqaError(N.PQA_EINVAL, "level_stats needs as many captured as reference frames")
        out = np.zeros((n, 1 << self.bit_depth, 3), np.uint64)
        shape = self.plane_shape(plane) if 0 <= plane < self.n_planes else None   # a bad plane is the library's to refuse
        keep_r, rp, rs = self._luma_list(ref_frames if shape else [], "reference", shape)
        keep_d, dp, ds = self._luma_list(dis_frames if shape else [], "captured", shape)
        self._check(self.lib.pqa_level_stats(self._ctx, rp, rs, dp, ds, n, plane, out.ctypes.data))
        del keep_r, keep_d
        return out

    def level_stats_resident(self, ref_ptr: int, ref_row_pitch: int, ref_frame_pitch: int, dis_ptr: int, dis_row_pitch: int,
                             dis_frame_pitch: int, n_frames: int, plane: int = 0) -> np.ndarray:
        """The same for two clips in HBM (device pointers, pitches in bytes; pqa_level_stats_device)."""
        out = np.zeros((max(int(n_frames), 0), 1 << self.bit_depth, 3), np.uint64)
        self._check(self.lib.pqa_level_stats_device(self._ctx, ref_ptr, ref_row_pitch, ref_frame_pitch, dis_ptr, dis_row_pitch,
                                                    dis_frame_pitch, int(n_frames), int(plane), out.ctypes.data))
        return out

    def _table(self, table):
        """(array kept alive, pointer) of a table of L = 2^bit_depth entries of this engine's sample type; an entry the type
        cannot hold is refused here, one above 2^bit_depth - 1 by the library"""
        t = np.asarray(table)
        if t.shape != (1 << self.bit_depth,) or t.dtype.kind not in "ui":
            raise ValueError(f"table_apply needs a table of {1 << self.bit_depth} integers")
        if t.size and (int(t.min()) < 0 or int(t.max()) > np.iinfo(self.dtype).max):
            raise N.PqaError(N.PQA_EINVAL, "table_apply: a table entry does not fit the sample type")
        t = np.ascontiguousarray(t, dtype=self.dtype)
        return t, t.ctypes.data

    def table_apply(self, frames, table, plane: int | None = 0):
        """A list of new 2-D arrays: every plane of `frames` (HOST memory) through the integer table, out = table[min(sample,
        L - 1)], L = 2^bit_depth (pqa_table_apply; definition: include/pqa_vmaf.h).  Any table of L entries none of which
        exceeds 2^bit_depth - 1, monotone or not; align.curve_lut makes the one that undoes a transfer curve.  The planes have
        the size of `plane` of this context, or with plane=None any one size of their own."""
        shape = self._own_shape("table_apply", frames, None if plane is None else self.plane_shape(int(plane)))
        keep_t, tp = self._table(table)
        sp = self._plane_spec(N.PqaTableSpec, shape)
        keep, sptr, sstride = self._luma_list(frames, "source", shape)
        out, dptr, ds = self._outputs(len(keep), [shape], self.dtype)
        self._check(self.lib.pqa_table_apply(self._ctx, C.byref(sp), tp, sptr, sstride, dptr, ds[0], len(keep)))
        del keep, keep_t
        return out

    def table_apply_resident(self, table, shape, src_ptr: int, src_row_pitch: int, src_frame_pitch: int, dst_ptr: int,
                             dst_row_pitch: int, dst_frame_pitch: int, n_frames: int):
        """The same for n_frames planes of `shape` = (height, width) in HBM (device pointers, pitches in bytes;
        pqa_table_apply_device); dst may be exactly src.  Nothing but the table crosses PCIe; the result can go into
        submit_resident."""
        keep_t, tp = self._table(table)
        sp = self._plane_spec(N.PqaTableSpec, shape)
        self._check(self.lib.pqa_table_apply_device(self._ctx, C.byref(sp), tp, src_ptr or None, src_row_pitch, src_frame_pitch,
                                                    dst_ptr or None, dst_row_pitch, dst_frame_pitch, int(n_frames)))
        del keep_t

    # -- deinterlacing -----------------------------------------------------------------------
    def _deint_spec(self, shape, mode, first, rate):
        """pqa_deint_spec of planes of `shape` = (height, width); a mode or rate by name, a field parity 0 / 1"""
        if mode not in N.DEINT_MODES:
            raise ValueError(f"deinterlace mode {mode!r} is none of {sorted(N.DEINT_MODES)}")
        if rate not in N.DEINT_RATES:
            raise ValueError(f"deinterlace rate {rate!r} is none of {sorted(N.DEINT_RATES)}")
        if first not in (0, 1):
            raise ValueError(f"deinterlace first {first!r} is neither 0 (top field first) nor 1")
        return self._plane_spec(N.PqaDeintSpec, shape, mode=N.DEINT_MODES[mode], first=first, rate=N.DEINT_RATES[rate])

    def deinterlace(self, frames, mode: str = "adaptive", first: int = 0, rate: str = "frame", shape=None):
        """A list of new 2-D arrays: the planes of an interlaced clip (HOST memory, in time order) deinterlaced in exact
        integers (pqa_deinterlace; definition: include/pqa_vmaf.h).  mode "intra" interpolates the dropped field from the kept
        one, "adaptive" from the fields before and after it where the picture is still; first: the parity of the rows that
        come first in time (0: top field first); rate "frame": one output a source frame, the field `first` kept; "field":
        two, `first` and then the other.  The planes have any one size of their own (`shape`, or the first frame's), at least
        two rows; every source frame is uploaded once."""
        shape = self._own_shape("deinterlace", frames, shape)
        sp = self._deint_spec(shape, mode, first, rate)
        keep, sptr, sstride = self._luma_list(frames, "source", shape)
        out, dptr, ds = self._outputs(len(keep) * (1 + sp.rate), [shape], self.dtype)
        self._check(self.lib.pqa_deinterlace(self._ctx, C.byref(sp), sptr, sstride, dptr, ds[0], len(keep)))
        del keep
        return out

    def deinterlace_resident(self, shape, src_ptr: int, src_row_pitch: int, src_frame_pitch: int, dst_ptr: int, dst_row_pitch: int,
                             dst_frame_pitch: int, n_frames: int, mode: str = "adaptive", first: int = 0, rate: str = "frame"):
        """The same for n_frames SOURCE planes of `shape` = (height, width) in HBM (device pointers, pitches in bytes;
        pqa_deinterlace_device); dst holds n_frames planes, or 2 n_frames at rate "field", and may not be src.  Nothing crosses
        PCIe; the result can go into submit_resident."""
        sp = self._deint_spec(shape, mode, first, rate)
        self._check(self.lib.pqa_deinterlace_device(self._ctx, C.byref(sp), src_ptr or None, src_row_pitch, src_frame_pitch,
                                                    dst_ptr or None, dst_row_pitch, dst_frame_pitch, int(n_frames)))

    # -- overlay masking ---------------------------------------------------------------------
    def _mask(self, nodes, steps, fill, shape):
        """(node grid kept alive, its pointer, pqa_mask_spec) of a mask over planes of `shape` = (height, width): nodes a 2-D
        array of integers 0 ... 256 with the rows and columns include/pqa_vmaf.h asks of steps = (step_log2_x, step_log2_y); a
        value uint16 cannot hold is refused here, one above 256 by the library"""
        sx, sy = (int(v) for v in steps)
        g = np.asarray(nodes)
        if g.ndim != 2 or g.dtype.kind not in "ui":
            raise ValueError("mask_blend needs a 2-D grid of integer nodes")
        if g.size and (int(g.min()) < 0 or int(g.max()) > 0xffff):
            raise N.PqaError(N.PQA_EINVAL, "mask_blend: a node does not fit uint16")
        if 0 <= sx <= N.MASK_MAX_STEP and 0 <= sy <= N.MASK_MAX_STEP and 1 <= shape[0] <= 8192 and 1 <= shape[1] <= 8192:
            want = (((shape[0] + (1 << sy) - 1) >> sy) + 1, ((shape[1] + (1 << sx) - 1) >> sx) + 1)
            if g.shape != want:   # the library cannot see the size of what the pointer points at
                raise ValueError(f"mask_blend needs a grid of {want} nodes for planes of {tuple(shape)} at steps {(sx, sy)}, not {g.shape}")
        g = np.ascontiguousarray(g, dtype=np.uint16)
        sp = self._plane_spec(N.PqaMaskSpec, shape, step_log2_x=sx, step_log2_y=sy, fill=0 if fill is None else fill)
        return g, g.ctypes.data, sp

    def mask_blend(self, frames, nodes, steps, fill, plane: int | None = 0):
        """A list of new 2-D arrays: every plane of `frames` (HOST memory) through the feathered mask of `nodes` (integers
        0 ... 256, `steps` = (step_log2_x, step_log2_y) samples apart as powers of two), out = (src (256 - a) + fill a + 128)
        >> 8 with a interpolated from the four nodes around a sample (pqa_mask_blend; definition: include/pqa_vmaf.h).  fill:
        an integer of at most 2^bit_depth - 1, or a list of as many planes as `frames` whose samples are the fill.
        distortion.overlay_mask makes the grid.  The planes have the size of `plane` of this context, or with plane=None any
        one size of their own."""
        shape = self._own_shape("mask_blend", frames, None if plane is None else self.plane_shape(int(plane)))
        const = isinstance(fill, (int, np.integer))
        if not const and len(fill) != len(frames):
            raise ValueError("mask_blend needs as many fill planes as frames")
        keep_g, gp, sp = self._mask(nodes, steps, fill if const else 0, shape)
        keep, sptr, sstride = self._luma_list(frames, "source", shape)
        keep_f, fptr, fstride = (None, None, 0) if const else self._luma_list(fill, "fill", shape)
        out, dptr, ds = self._outputs(len(keep), [shape], self.dtype)
        self._check(self.lib.pqa_mask_blend(self._ctx, C.byref(sp), gp, sptr, sstride, fptr, fstride, dptr, ds[0], len(keep)))
        del keep, keep_f, keep_g
        return out

    def mask_blend_resident(self, nodes, steps, fill, shape, src_ptr: int, src_row_pitch: int, src_frame_pitch: int, dst_ptr: int,
                            dst_row_pitch: int, dst_frame_pitch: int, n_frames: int, fill_ptr: int = 0, fill_row_pitch: int = 0,
                            fill_frame_pitch: int = 0):
        """The same for n_frames planes of `shape` = (height, width) in HBM (device pointers, pitches in bytes;
        pqa_mask_blend_device).  fill: the constant; with fill_ptr the fill plane in HBM instead.  dst may be exactly src --
        then only the bounding rectangle of the mask is read and written -- but not the fill plane.  Nothing but the node grid
        crosses PCIe; the result can go into submit_resident."""
        keep_g, gp, sp = self._mask(nodes, steps, fill, shape)
        self._check(self.lib.pqa_mask_blend_device(self._ctx, C.byref(sp), gp, src_ptr or None, src_row_pitch, src_frame_pitch,
                                                   fill_ptr or None, fill_row_pitch, fill_frame_pitch, dst_ptr or None,
                                                   dst_row_pitch, dst_frame_pitch, int(n_frames)))
        del keep_g

    # -- resampling --------------------------------------------------------------------------
    def _resample_spec(self, src_shape, dst_shape, filter, window):
        """the pqa_resample_spec of planes src_shape -> dst_shape ((height, width) each); window = (x0, y0, w, h) in source
        samples, rounded to Q16 (None: the whole plane)"""
        if filter not in N.RESAMPLE_FILTERS:
            raise ValueError(f"resample filter must be one of {sorted(N.RESAMPLE_FILTERS)}, not {filter!r}")
        x0, y0, ww, wh = window if window is not None else (0, 0, src_shape[1], src_shape[0])
        sp = N.PqaResampleSpec()
        sp.struct_size, sp.filter = C.sizeof(N.PqaResampleSpec), N.RESAMPLE_FILTERS[filter]
        sp.src_width, sp.src_height, sp.dst_width, sp.dst_height = (max(0, int(v)) for v in (src_shape[1], src_shape[0], dst_shape[1], dst_shape[0]))
        sp.x0_q16, sp.y0_q16, sp.w_q16, sp.h_q16 = (int(round(v * 65536)) for v in (x0, y0, ww, wh))
        return sp

    def resample(self, frames, dst_shape, filter: str = "bicubic", window=None):
        """A list of 2-D arrays of dst_shape = (height, width): every plane of `frames` (2-D arrays of one size, which need
        not be this context's) resized with the exact-integer polyphase filter "bilinear", "bicubic" or "lanczos"
        (pqa_resample; definition: include/pqa_vmaf.h).  window = (x0, y0, w, h) in source samples is what the result
        shows (default: the whole plane); a fractional (x0, y0) with dst_shape = the source's is a sub-pixel shift.  Planes
        in HOST memory; samples of this context's bit depth."""
        src_shape = np.shape(frames[0]) if len(frames) else (int(dst_shape[0]), int(dst_shape[1]))
        keep, sptr, ss = self._host_planes(frames, self.dtype, "resample needs 2-D planes of one size", [src_shape])
        sp = self._resample_spec(src_shape, dst_shape, filter, window)
        out, dptr, ds = self._outputs(len(keep), [(sp.dst_height, sp.dst_width)], self.dtype)
        self._check(self.lib.pqa_resample(self._ctx, C.byref(sp), sptr, ss[0], dptr, ds[0], len(keep)))
        return out

    def resample_resident(self, src_ptr: int, src_row_pitch: int, src_frame_pitch: int, src_shape, dst_ptr: int,
                          dst_row_pitch: int, dst_frame_pitch: int, dst_shape, n_frames: int, filter: str = "bicubic", window=None):
        """The same for planes in HBM (device pointers, pitches in bytes; pqa_resample_device): n_frames planes of src_shape
        at src_ptr become planes of dst_shape at dst_ptr.  Nothing crosses PCIe; the result can go into submit_resident."""
        sp = self._resample_spec(src_shape, dst_shape, filter, window)
        self._check(self.lib.pqa_resample_device(self._ctx, C.byref(sp), src_ptr, src_row_pitch, src_frame_pitch, dst_ptr,
                                                 dst_row_pitch, dst_frame_pitch, int(n_frames)))

    # -- the spec-driven analyses: planes of the call's own size -------------------------------
    @staticmethod
    def _plane_spec(cls, shape, **third):
        """the spec `cls` of planes of `shape` = (height, width); `third`: its third field (tile or levels)"""
        sp = cls()
        sp.struct_size = C.sizeof(cls)
        sp.height, sp.width = (max(0, int(v)) for v in (shape[0], shape[1]))
        for name, v in third.items():
            setattr(sp, name, max(0, int(v)))
        return sp

    @staticmethod
    def _spec(name, shape, third=None):
        """the spec of the analysis `name` (a row of _ANALYSES) over planes of `shape` = (height, width); third: its tile or levels"""
        cls, field, _ = _ANALYSES[name]
        return FeatureEngine._plane_spec(cls, shape, **({field: third} if field else {}))

    # the names the argument tests of the raw entries build a spec by
    _flow_spec = staticmethod(lambda shape, tile: FeatureEngine._spec("flow_moments", shape, tile))
    _tile_spec = staticmethod(lambda shape, tile: FeatureEngine._spec("tile_moments", shape, tile))
    _band_spec = staticmethod(lambda shape, levels: FeatureEngine._spec("band_moments", shape, levels))
    _temporal_spec = staticmethod(lambda shape, tile: FeatureEngine._spec("temporal_moments", shape, tile))
    _profile_spec = staticmethod(lambda shape: FeatureEngine._spec("line_profiles", shape))
    _field_spec = staticmethod(lambda shape: FeatureEngine._spec("field_moments", shape))
    _edge_spec = staticmethod(lambda shape: FeatureEngine._spec("edge_profiles", shape))

    def _plane_call(self, name, lists, shape, third=None):
        """(out, spec) of pqa_<name> over planes in host memory.  lists: (reference frames, captured frames) or (frames,);
        shape: (height, width) or None for the first frame's; third: the tile or levels of the spec."""
        n = len(lists[0])
        if len(lists[-1]) != n:
            raise ValueError(f"{name} needs as many captured as reference frames")
        shape = self._own_shape(name, lists[0], shape)
        sp = self._spec(name, shape, third)
        out = _ANALYSES[name][2](n, sp)
        keep, args = [], []
        for frames, what in zip(lists, ("reference", "captured") if len(lists) == 2 else ("profile",)):
            arrs, ptrs, stride = self._luma_list(frames, what, shape)
            keep.append(arrs)
            args += [ptrs, stride]
        self._check(getattr(self.lib, "pqa_" + name)(self._ctx, C.byref(sp), *args, n, out.ctypes.data))
        del keep
        return out, sp

    def _plane_call_resident(self, name, clips, shape, n_frames, third=None):
        """(out, spec) of pqa_<name>_device; clips: (pointer, row pitch, frame pitch) of every clip, flat"""
        sp = self._spec(name, shape, third)
        out = _ANALYSES[name][2](n_frames, sp)
        self._check(getattr(self.lib, f"pqa_{name}_device")(self._ctx, C.byref(sp), *clips, int(n_frames), out.ctypes.data))
        return out, sp

    @staticmethod
    def _profile_split(out, sp):
        return out[:, :sp.height], out[:, sp.height:]

    # -- sub-pixel registration ----------------------------------------------------------------
    def flow_moments(self, ref_frames, dis_frames, tile: int = 32) -> np.ndarray:
        """[n, ty, tx, 6] int64: per tile of `tile` x `tile` pixels (8, 16, 32 or 64) the sums of gx^2, gx gy, gy^2, gx dt,
        gy dt, dt^2 over the pixels 1 <= x <= W - 2, 1 <= y <= H - 2 (gx, gy: Sobel of ref + dis; dt: 3 x 3 binomial of
        dis - ref), exact (pqa_flow_moments; definition: include/pqa_vmaf.h).  Planes in HOST memory: two lists of 2-D arrays
        of equal length and one size, which need not be this context's (3 ... 8192 each way); samples of this context's bit
        depth.  align.solve_geometry reads the sum over the frames."""
        return self._plane_call("flow_moments", (ref_frames, dis_frames), None, tile)[0]

    def flow_moments_resident(self, ref_ptr: int, ref_row_pitch: int, ref_frame_pitch: int, dis_ptr: int, dis_row_pitch: int,
                              dis_frame_pitch: int, shape, n_frames: int, tile: int = 32) -> np.ndarray:
        """The same for two clips of planes of `shape` = (height, width) in HBM (device pointers, pitches in bytes;
        pqa_flow_moments_device)."""
        return self._plane_call_resident("flow_moments", (ref_ptr, ref_row_pitch, ref_frame_pitch, dis_ptr, dis_row_pitch, dis_frame_pitch),
                                         shape, n_frames, tile)[0]

    # -- distortion map ------------------------------------------------------------------------
    def tile_moments(self, ref_frames, dis_frames, tile: int = 32) -> np.ndarray:
        """[n, ty, tx, 6] uint64: per tile of `tile` x `tile` pixels (8, 16, 32 or 64; edge tiles hold the pixels that exist)
        the sums of r, d, r^2, d^2, r d and |d - r| (r: reference, d: captured), exact (pqa_tile_moments; definition:
        include/pqa_vmaf.h).  Planes in HOST memory: two lists of 2-D arrays of equal length and one size, which need not be
        this context's (1 ... 8192 each way); samples of this context's bit depth.  distortion.tile_metrics and
        distortion.find_defects read the result."""
        return self._plane_call("tile_moments", (ref_frames, dis_frames), None, tile)[0]

    def tile_moments_resident(self, ref_ptr: int, ref_row_pitch: int, ref_frame_pitch: int, dis_ptr: int, dis_row_pitch: int,
                              dis_frame_pitch: int, shape, n_frames: int, tile: int = 32) -> np.ndarray:
        """The same for two clips of planes of `shape` = (height, width) in HBM (device pointers, pitches in bytes;
        pqa_tile_moments_device)."""
        return self._plane_call_resident("tile_moments", (ref_ptr, ref_row_pitch, ref_frame_pitch, dis_ptr, dis_row_pitch, dis_frame_pitch),
                                         shape, n_frames, tile)[0]

    # -- distortion spectrum -------------------------------------------------------------------
    def band_moments(self, ref_frames, dis_frames, levels: int = 4) -> np.ndarray:
        """[n, L, 4, 3] uint64: per level l = 1 ... L = `levels` (1 ... 6) and orientation (0 H, 1 V, 2 D, 3 A) of the
        unnormalised Haar transform the sums of r^2, d^2 and r d over the level's coefficients (r: reference, d: captured; the
        last is an int64: .view(np.int64)), exact (pqa_band_moments; definition: include/pqa_vmaf.h).  Planes in HOST memory:
        two lists of 2-D arrays of equal length and one size, which need not be this context's (1 ... 8192 each way); samples
        of this context's bit depth.  spectrum.band_table and spectrum.summary read the result."""
        return self._plane_call("band_moments", (ref_frames, dis_frames), None, levels)[0]

    def band_moments_resident(self, ref_ptr: int, ref_row_pitch: int, ref_frame_pitch: int, dis_ptr: int, dis_row_pitch: int,
                              dis_frame_pitch: int, shape, n_frames: int, levels: int = 4) -> np.ndarray:
        """The same for two clips of planes of `shape` = (height, width) in HBM (device pointers, pitches in bytes;
        pqa_band_moments_device)."""
        return self._plane_call_resident("band_moments", (ref_ptr, ref_row_pitch, ref_frame_pitch, dis_ptr, dis_row_pitch, dis_frame_pitch),
                                         shape, n_frames, levels)[0]

    # -- temporal distortion -------------------------------------------------------------------
    def temporal_moments(self, ref_frames, dis_frames, tile: int = 32) -> np.ndarray:
        """[n - 1, ty, tx, 7] uint64: per transition k = 1 ... n - 1 and tile of `tile` x `tile` pixels (8, 16, 32 or 64; edge
        tiles hold the pixels that exist) the sums of a, b, a^2, b^2, a b, a e and e^2 with a = R_k - R_{k-1},
        b = D_k - D_{k-1}, e = D_k - R_k (R: reference, D: captured), exact (pqa_temporal_moments; definition:
        include/pqa_vmaf.h).  Words 0, 1, 4 and 5 (N.TEMPORAL_SIGNED) are int64: read them through .view(np.int64).  Planes in
        HOST memory: two lists of 2-D arrays of equal length and one size, which need not be this context's (1 ... 8192 each
        way); samples of this context's bit depth.  Fewer than two frames give an empty result.  temporal.frame_table and
        temporal.summary read the result."""
        return self._plane_call("temporal_moments", (ref_frames, dis_frames), None, tile)[0]

    def temporal_moments_resident(self, ref_ptr: int, ref_row_pitch: int, ref_frame_pitch: int, dis_ptr: int, dis_row_pitch: int,
                                  dis_frame_pitch: int, shape, n_frames: int, tile: int = 32) -> np.ndarray:
        """The same for two clips of planes of `shape` = (height, width) in HBM (device pointers, pitches in bytes;
        pqa_temporal_moments_device)."""
        return self._plane_call_resident("temporal_moments", (ref_ptr, ref_row_pitch, ref_frame_pitch, dis_ptr, dis_row_pitch, dis_frame_pitch),
                                         shape, n_frames, tile)[0]

    # -- active-picture detection --------------------------------------------------------------
    def line_profiles(self, frames, shape=None):
        """(rows [n, H, 2], cols [n, W, 2]) uint64: per row and per column of every plane the sum of its samples and the sum
        of their squares, exact (pqa_line_profiles; definition: include/pqa_vmaf.h).  Planes in HOST memory: a list of 2-D
        arrays (views are fine) of `shape` = (height, width), default the first frame's, which need not be this context's
        (1 ... 8192 each way); samples of this context's bit depth.  align.active_picture reads the result."""
        return self._profile_split(*self._plane_call("line_profiles", (frames,), shape))

    def line_profiles_resident(self, ptr: int, row_pitch: int, frame_pitch: int, shape, n_frames: int):
        """The same for n_frames planes of `shape` = (height, width) in HBM (device pointer, pitches in bytes;
        pqa_line_profiles_device)."""
        return self._profile_split(*self._plane_call_resident("line_profiles", (ptr, row_pitch, frame_pitch), shape, n_frames))

    # -- field alignment -------------------------------------------------------------------------
    def field_moments(self, ref_frames, dis_frames, shape=None) -> np.ndarray:
        """[n - 1, 14] uint64: per transition k = 1 ... n - 1 the squared errors of field against field, E(A, p, B, q) summed
        over the row pairs: words 2 p + q: captured field p of frame k against reference field q of frame k; 4 + 2 p + q:
        against reference frame k - 1; 8 + 2 p + q: captured frame k - 1 against reference frame k; 12 / 13: the comb of the
        captured / reference frame k, exact (pqa_field_moments; definition: include/pqa_vmaf.h).  Planes in HOST memory: two
        lists of 2-D arrays (views are fine) of equal length and of `shape` = (height, width), default the first frame's,
        which need not be this context's (width 1 ... 8192, height 2 ... 8192); samples of this context's bit depth.  Fewer
        than two frames give an empty result.  fields.segments and fields.summary read the result."""
        return self._plane_call("field_moments", (ref_frames, dis_frames), shape)[0]

    def field_moments_resident(self, ref_ptr: int, ref_row_pitch: int, ref_frame_pitch: int, dis_ptr: int, dis_row_pitch: int,
                               dis_frame_pitch: int, shape, n_frames: int) -> np.ndarray:
        """The same for two clips of planes of `shape` = (height, width) in HBM (device pointers, pitches in bytes;
        pqa_field_moments_device)."""
        return self._plane_call_resident("field_moments", (ref_ptr, ref_row_pitch, ref_frame_pitch, dis_ptr, dis_row_pitch, dis_frame_pitch),
                                         shape, n_frames)[0]

    # -- coding-grid detection -----------------------------------------------------------------
    def edge_profiles(self, ref_frames, dis_frames, shape=None):
        """(rows [n, H, 3], cols [n, W, 3]) uint64: per row line y (the boundary between the rows y - 1 and y) and per column
        line x (between the columns x - 1 and x) of every frame pair the sums of a^2, b^2 and a b, with a / b the difference
        of a reference / captured sample across the line, exact (pqa_edge_profiles; definition: include/pqa_vmaf.h).  Line 0
        of each axis is zero; word 2 is int64: read it through .view(np.int64).  Planes in HOST memory: two lists of 2-D arrays
        (views are fine) of equal length and of `shape` = (height, width), default the first frame's, which need not be this
        context's (1 ... 8192 each way); samples of this context's bit depth.  grid.summary reads the result."""
        return self._profile_split(*self._plane_call("edge_profiles", (ref_frames, dis_frames), shape))

    def edge_profiles_resident(self, ref_ptr: int, ref_row_pitch: int, ref_frame_pitch: int, dis_ptr: int, dis_row_pitch: int,
                               dis_frame_pitch: int, shape, n_frames: int):
        """The same for two clips of planes of `shape` = (height, width) in HBM (device pointers, pitches in bytes;
        pqa_edge_profiles_device)."""
        return self._profile_split(*self._plane_call_resident("edge_profiles", (ref_ptr, ref_row_pitch, ref_frame_pitch, dis_ptr, dis_row_pitch,
                                                                                dis_frame_pitch), shape, n_frames))

    # -- colour-matrix alignment ---------------------------------------------------------------
    def _frame_list(self, frames, what: str):
        """(arrays kept alive, ctypes pointer array [n * 3], stride triple) of frames [Y, U, V] in host memory: packed copies
        unless every plane already has this engine's dtype, unit column stride and one row stride per plane kind"""
        return self._host_planes(frames, self.dtype, what + " frame {i} plane {p} is {got}, engine is {want}",
                                 [self.plane_shape(p) for p in range(3)], k=3)

    def _colour_mask(self, lo, hi):
        top = (1 << self.bit_depth) - 1
        return (1 if lo is None else int(lo)), (top - 1 if hi is None else int(hi))

    def colour_moments(self, ref_frames, dis_frames, lo=None, hi=None) -> np.ndarray:
        """[n, 28] uint64: per frame pair the upper triangle, row-major, of the sum of z z^T over the chroma grid, z = (1, SYr, Ur,
        Vr, SYd, Ud, Vd), SY = the sum of the luma samples under a chroma sample, exact (pqa_colour_moments; definition:
        include/pqa_vmaf.h).  A chroma sample enters only if every captured sample it reads lies in lo ... hi (default 1 ...
        top - 1: clipped samples stay out; 0 and top keep everything).  Frames [Y, U, V] in HOST memory (two lists of equal
        length); needs n_planes == 3.  align.best_colour reads the result."""
        n = len(ref_frames)
        if len(dis_frames) != n:
            raise ValueError("colour_moments needs as many captured as reference frames")
        if self.n_planes != 3:
            raise N.PqaError(N.PQA_EINVAL, "colour_moments needs the chroma planes: n_planes must be 3")
        lo, hi = self._colour_mask(lo, hi)
        out = np.zeros((n, N.COLOUR_SUMS), np.uint64)
        keep_r, rp, rs = self._frame_list(ref_frames, "reference")
        keep_d, dp, ds = self._frame_list(dis_frames, "captured")
        self._check(self.lib.pqa_colour_moments(self._ctx, rp, C.byref(rs), dp, C.byref(ds), n, lo, hi, out.ctypes.data))
        del keep_r, keep_d
        return out

    def colour_moments_resident(self, ref_ptrs, dis_ptrs, row_pitch, frame_pitch, n_frames: int, lo=None, hi=None) -> np.ndarray:
        """The same for two clips in HBM (ref_ptrs / dis_ptrs: device addresses of frame 0's planes; pitches in bytes per
        plane, common to both clips; pqa_colour_moments_device)."""
        lo, hi = self._colour_mask(lo, hi)
        out = np.zeros((max(int(n_frames), 0), N.COLOUR_SUMS), np.uint64)
        r, d = self._device_clip(ref_ptrs, row_pitch, frame_pitch), self._device_clip(dis_ptrs, row_pitch, frame_pitch)
        self._check(self.lib.pqa_colour_moments_device(self._ctx, C.byref(r), C.byref(d), int(n_frames), lo, hi, out.ctypes.data))
        return out

    def colour_apply(self, frames, m):
        """A list of frames [Y, U, V]: every frame of `frames` through the 3 x 4 integer matrix m (12 values, Q14; column 0 the
        offset: align.colour_correction / align.colour_matrix_q14), planes of the same sizes (pqa_colour_apply; definition:
        include/pqa_vmaf.h).  Frames in HOST memory; needs n_planes == 3."""
        if self.n_planes != 3:
            raise N.PqaError(N.PQA_EINVAL, "colour_apply needs the chroma planes: n_planes must be 3")
        mm = (C.c_int32 * 12)(*[int(v) for v in np.asarray(m).reshape(12)])
        keep, sp, ss = self._frame_list(frames, "source")
        n = len(frames)
        out, dp, ds = self._outputs(n, [self.plane_shape(p) for p in range(3)], self.dtype)
        self._check(self.lib.pqa_colour_apply(self._ctx, C.byref(mm), sp, C.byref(ss), dp, C.byref(ds), n))
        del keep
        return [out[3 * i:3 * i + 3] for i in range(n)]

    def colour_apply_resident(self, m, src_ptrs, dst_ptrs, row_pitch, frame_pitch, n_frames: int):
        """The same for a clip in HBM into planes in HBM (device addresses of frame 0's planes; pitches in bytes per plane,
        common to both; pqa_colour_apply_device).  Nothing crosses PCIe; the result can go into submit_resident."""
        mm = (C.c_int32 * 12)(*[int(v) for v in np.asarray(m).reshape(12)])
        s, d = self._device_clip(src_ptrs, row_pitch, frame_pitch), self._device_clip(dst_ptrs, row_pitch, frame_pitch)
        self._check(self.lib.pqa_colour_apply_device(self._ctx, C.byref(mm), C.byref(s), C.byref(d), int(n_frames)))

    # -- Delta E ITP ---------------------------------------------------------------------------
    def delta_itp(self, ref_frames, dis_frames, spec) -> np.ndarray:
        """[n, 8] float64: per frame pair the sums of the BT.2124 colour difference in ICtCp -- sum dE, sum dI^2, sum dT^2, sum
        dP^2, max dE, pixels above the threshold, pixels, the reference's sum of I (pqa_delta_itp; definition:
        include/pqa_vmaf.h).  `spec`: itp.spec(...) (transfer, the two matrices, peak, threshold).  Frames [Y, Cb, Cr] in HOST
        memory (two lists of equal length); needs n_planes == 3.  itp.summary reads the result."""
        from . import itp as ITP
        n = len(ref_frames)
        if len(dis_frames) != n:
            raise ValueError("delta_itp needs as many captured as reference frames")
        if self.n_planes != 3:
            raise N.PqaError(N.PQA_EINVAL, "delta_itp needs the chroma planes: n_planes must be 3")
        sp = spec if isinstance(spec, N.PqaItpSpec) else ITP.native_spec(spec)
        out = np.zeros((n, N.ITP_SUMS), np.float64)
        keep_r, rp, rs = self._frame_list(ref_frames, "reference")
        keep_d, dp, ds = self._frame_list(dis_frames, "captured")
        self._check(self.lib.pqa_delta_itp(self._ctx, C.byref(sp), rp, C.byref(rs), dp, C.byref(ds), n, out.ctypes.data))
        del keep_r, keep_d
        return out

    def delta_itp_resident(self, ref_ptrs, dis_ptrs, row_pitch, frame_pitch, n_frames: int, spec) -> np.ndarray:
        """The same for two clips in HBM (ref_ptrs / dis_ptrs: device addresses of frame 0's planes; pitches in bytes per
        plane, common to both clips; pqa_delta_itp_device)."""
        from . import itp as ITP
        sp = spec if isinstance(spec, N.PqaItpSpec) else ITP.native_spec(spec)
        out = np.zeros((max(int(n_frames), 0), N.ITP_SUMS), np.float64)
        r, d = self._device_clip(ref_ptrs, row_pitch, frame_pitch), self._device_clip(dis_ptrs, row_pitch, frame_pitch)
        self._check(self.lib.pqa_delta_itp_device(self._ctx, C.byref(sp), C.byref(r), C.byref(d), int(n_frames), out.ctypes.data))
        return out

    # -- results -----------------------------------------------------------------------------
    def collect(self, first_index: int, count: int) -> np.ndarray:
        out = np.zeros((count, N.RECORD_DOUBLES), np.float64)
        self._check(self.lib.pqa_collect(self._ctx, first_index, count, out.ctypes.data))
        return out

    def collect_blocks(self, first_index: int, count: int, blocks=()):
        """(records [count, 24], {i: rows [count, width of block i]}): collect() plus the rows of the same frames in the
        extension blocks asked for (indices into N.EXT_BLOCKS; NaN where the context does not run the block's features).
        One pqa_collect_ext5 call with NULL for every other block: nothing is allocated or copied for those."""
        out = np.zeros((count, N.RECORD_DOUBLES), np.float64)
        got = {i: np.zeros((count, N.EXT_BLOCKS[i][1]), np.float64) for i in sorted(set(blocks))}
        ptrs = [got[i].ctypes.data if i in got else None for i in range(len(N.EXT_BLOCKS))]
        self._check(self.lib.pqa_collect_ext5(self._ctx, first_index, count, out.ctypes.data, *ptrs))
        return out, got

    def _collect_first(self, first_index: int, count: int, n_blocks: int):
        out, got = self.collect_blocks(first_index, count, range(n_blocks))
        return (out, *(got[i] for i in range(n_blocks)))

    # (records, ext, ..., extN): the first N blocks of N.EXT_BLOCKS, as pqa_collect_ext ... pqa_collect_ext5 hand them out
    def collect_ext(self, first_index: int, count: int):
        return self._collect_first(first_index, count, 1)

    def collect_ext2(self, first_index: int, count: int):
        return self._collect_first(first_index, count, 2)

    def collect_ext3(self, first_index: int, count: int):
        return self._collect_first(first_index, count, 3)

    def collect_ext4(self, first_index: int, count: int):
        return self._collect_first(first_index, count, 4)

    def collect_ext5(self, first_index: int, count: int):
        return self._collect_first(first_index, count, 5)

    def flush(self):
        self._check(self.lib.pqa_flush(self._ctx))

    def sync(self):
        self._check(self.lib.pqa_sync(self._ctx))

    def cancel(self):
        self.lib.pqa_cancel(self._ctx)

    def reset(self):
        self._check(self.lib.pqa_reset(self._ctx))

    # -- measurement ---------------------------------------------------------------------------
    def profile_enable(self, on=True):
        """True: time every kernel; False: stop; an iterable of kernel ids: time only those (event records
        between kernels are not free, so the bench times just the dominant kernel inside its timed region)."""
        if on is True:
            code = 1
        elif not on:
            code = 0
        else:
            mask = 0
            for k in on:
                mask |= 1 << int(k)
            code = mask << 1
        self._check(self.lib.pqa_profile_enable(self._ctx, code))

    def profile_read(self) -> dict:
        out = {}
        for k in range(N.PROF_KERNELS):
            ms, n, fr = C.c_double(), C.c_uint64(), C.c_uint64()
            self._check(self.lib.pqa_profile_read(self._ctx, k, C.byref(ms), C.byref(n), C.byref(fr)))
            out[self.lib.pqa_profile_kernel_name(k).decode()] = {"ms": ms.value, "launches": n.value, "frames": fr.value}
        return out


def sse_from_records(rec: np.ndarray) -> np.ndarray:
    """[n,3] uint64 SSE (Y,U,V) bit-cast out of the record slots."""
    return np.ascontiguousarray(rec[:, N.REC_SSE:N.REC_SSE + 3]).view(np.uint64)
