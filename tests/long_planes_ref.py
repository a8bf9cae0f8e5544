"""Frames at the size limits of pqa_create (16 ... 16384 samples each way): the clips, the oracle values and the library's own
partial counts that tests/test_long_planes_ref.py (CPU) and tests/test_gpu_long_planes.py (GPU) share.

A 16384 x 16 frame has 262 144 pixels, so it costs what a 512 x 512 frame costs, yet it holds the largest stripe, segment and
partial-slot counts and the largest column / row offsets any kernel forms.  The content is synth.make_clip's (sinusoids,
texture, blur + noise + block quantisation) with the sample extremes written into the last 16 columns or rows of the long
axis: the far end of the plane then carries the largest values the kernels hold, and an error there is not a rounding
error.  Three frames: frame 1 changes the far end against frame 0 (motion sees it), frame 2 is make_clip's own.

No GPU imports.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from pqa2_amd import synth

N_FRAMES = 3
MAX_BATCH = 2          # three frames at batch 2: a partial batch and a motion carry
FAR = 16               # columns / rows at the far end of the long axis that hold the extremes

# (width, height, bit depth): the four 262k-pixel sizes (odd ones: mirrored last row / column), then the two the ADM pyramid
# kernel takes (multiples of 4, >= 128 each way)
SMALL = [(16384, 16, 8), (16, 16384, 8), (16384, 17, 10), (17, 16384, 12)]
PYRAMID = [(16384, 128, 8), (128, 16384, 10)]
SIZES = SMALL + PYRAMID

N_FEAT = 17
FEATURES = ([f"vif_num_s{s}" for s in range(4)] + [f"vif_den_s{s}" for s in range(4)] +
            [f"adm_num_s{s}" for s in range(4)] + [f"adm_den_s{s}" for s in range(4)] + ["motion"])

REL_TOL = 5e-5         # tests/test_gpu_parity.py's bar; the rule max(REL_TOL, 4 x rel32) leaves it unchanged here, because ...
REL32_MAX = 1e-5       # ... the f32 oracle stays this close to f64 on every size (tests/test_long_planes_ref.py asserts it)
MOTION_ATOL = 2e-5


def far_end(plane: np.ndarray, lo: int, hi: int) -> np.ndarray:
    """The view of `plane` that is columns / rows [n - FAR + lo, n - FAR + hi) of its long axis, the whole short axis."""
    h, w = plane.shape
    if w >= h:
        return plane[:, w - FAR + lo:w - FAR + hi]
    return plane[h - FAR + lo:h - FAR + hi, :]


@functools.lru_cache(maxsize=None)
def clip(w: int, h: int, bpc: int):
    """(refs, diss): N_FRAMES luma planes each, read-only, built once."""
    refs, diss = synth.make_clip(w, h, N_FRAMES, bpc, chroma=False)
    refs, diss = [r[0] for r in refs], [d[0] for d in diss]
    top = (1 << bpc) - 1
    # frame 0: 0 against top (the largest difference), then top against top (the largest products)
    far_end(refs[0], 0, 8)[...] = 0
    far_end(diss[0], 0, 8)[...] = top
    far_end(refs[0], 8, 16)[...] = top
    far_end(diss[0], 8, 16)[...] = top
    # frame 1: the other way round, so that the reference changes by the whole range between frames 0 and 1
    far_end(refs[1], 0, 8)[...] = top
    far_end(diss[1], 0, 8)[...] = 0
    far_end(refs[1], 8, 16)[...] = 0
    far_end(diss[1], 8, 16)[...] = 0
    for p in refs + diss:
        p.setflags(write=False)
    return refs, diss


_ORACLE = {}   # (precision, w, h, bpc, border101) -> [N_FRAMES, 17], computed once and never modified


def oracle_features(orc, w: int, h: int, bpc: int, vif_border101: bool = False) -> np.ndarray:
    key = (orc.precision, w, h, bpc, vif_border101)
    if key not in _ORACLE:
        refs, diss = clip(w, h, bpc)
        e = orc.clip_features_mt(refs, diss, bpc, threads=N_FRAMES, vif_border101=vif_border101)
        e.setflags(write=False)
        _ORACLE[key] = e
    return _ORACLE[key]


_INT_ORACLE = {}


def int_oracle_features(w: int, h: int, bpc: int) -> np.ndarray:
    """[N_FRAMES, 17] of the fixed-point restatement (oracle/vmaf_int_oracle.c)."""
    if (w, h, bpc) not in _INT_ORACLE:
        from oracle.int_oracle import IntOracle
        refs, diss = clip(w, h, bpc)
        e = IntOracle().clip_features_mt(refs, diss, bpc, threads=N_FRAMES)
        e.setflags(write=False)
        _INT_ORACLE[w, h, bpc] = e
    return _INT_ORACLE[w, h, bpc]


def rel_features(got: np.ndarray, want: np.ndarray) -> np.ndarray:
    """[n, 16] relative distance of the VIF / ADM doubles."""
    return np.abs(got[:, :16] - want[:, :16]) / np.maximum(np.abs(want[:, :16]), 1e-12)


# ---- the library's own counts (host arithmetic: the library loads without a GPU) ----------------------------------------
COUNT_NAMES = (["vif_march_sized", "vif_march_written"] +
               [f"adm_march_{kind}_s{s}" for s in range(4) for kind in ("sized", "written")] +
               ["adm_pyramid_sized", "adm_pyramid_written", "motion_march_sized", "motion_march_written"])


def partial_counts(w: int, h: int, bpc: int) -> dict:
    """What the context's sizing functions return and what the launchers themselves report to write (a launch of no frames)."""
    from pqa2_amd import _native as N
    out = (C.c_int32 * N.PARTIAL_COUNT_INTS)()
    rc = N.load().pqa_debug_partial_counts(w, h, bpc, C.byref(out), N.PARTIAL_COUNT_INTS)
    assert rc == N.PQA_OK, (w, h, bpc, rc)
    assert len(COUNT_NAMES) == N.PARTIAL_COUNT_INTS
    return dict(zip(COUNT_NAMES, (int(v) for v in out)))
