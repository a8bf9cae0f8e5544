"""Inputs for the chroma-layout tests (tests/test_gpu_chroma_layouts.py, tests/test_chroma_layouts_ref.py): the nine
(chroma_hshift, chroma_vshift) pairs pqa_create accepts, the localized ciede2000 construction (a frame pair that differs
in one 8 x 8 luma patch, so the frame's dE00 sum is the patch's own), its geometries and patch origins, two deliberate
mutations of the restatement that stand for the errors the construction must catch, and random planes with a bounded
offset for the FFmpeg PSNR / SSIM kernels.  Everything is numpy on the host; the restatement is tests/ciede_ref.py."""
from __future__ import annotations

import functools

import numpy as np

from tests import ciede_ref as R

LAYOUTS = [(hs, vs) for hs in range(3) for vs in range(3)]
# the ciede_kernel<T, HS, VS> instantiations no other test runs: the ones with a rolled pixel loop or a vertical-only break
NEVER_RUN = [(2, 2), (2, 1), (2, 0), (1, 2), (0, 1), (0, 2)]
PATCH = 8                   # luma patch edge
PAIR_TOL = 2e-5             # tests/test_gpu_ciede.py's bound on the device function per pair, applied per changed pixel


def chroma_size(w, h, hs, vs):
    return (w + (1 << hs) - 1) >> hs, (h + (1 << vs) - 1) >> vs


def dtype_of(bpc):
    return np.uint8 if bpc == 8 else np.uint16


def depths(hs, vs):
    return (8, 10, 12) if (hs, vs) in NEVER_RUN else (8, 10)


def seam_size(hs, vs):
    """More than two 64 x 4 chroma-sample workgroup tiles each way; the last chroma column covers one luma pixel, the last
    chroma row one luma row (vertical shift 0 or 1) or three (shift 2)."""
    return (128 << hs) + 5, (16 << vs) + 3


def geometries(hs, vs):
    """[(w, h, [patch origins])]: the seam size with the four corners, a patch across a tile seam both ways and two
    patches clipped by the frame's end; 19 x 19 and 18 x 18 (one partial tile; at shift 2 the last chroma sample covers
    3 and 2 luma pixels) with the first and a clipped last patch."""
    w, h = seam_size(hs, vs)
    out = [(w, h, [(0, 0), (w - PATCH, 0), (0, h - PATCH), (w - PATCH, h - PATCH),
                   ((64 << hs) - 4, max(0, (4 << vs) - 4)), (w - 3, h - 3), (w - 1, h - 1)])]
    for s in (19, 18):
        out.append((s, s, [(0, 0), (s - 3, s - 3)]))
    return out


def cases(hs, vs):
    """Every (w, h, bpc, origin) of one layout."""
    return [(w, h, bpc, o) for (w, h, origins) in geometries(hs, vs) for bpc in depths(hs, vs) for o in origins]


@functools.lru_cache(maxsize=None)
def patch_pair(w, h, bpc, hs, vs, origin):
    """(ref planes, dis planes, changed): a random textured reference (luma 16 s .. 235 s, chroma 64 s .. 191 s,
    s = 2^(bpc - 8)) and a copy that differs only in the 8 x 8 luma patch at `origin`, clipped to the frame: Y raised by
    20 s .. 59 s (held at full scale), the chroma samples under the patch moved by 10 s .. 39 s, U up and V down.
    `changed` marks the luma pixels whose inputs differ (the patch and whatever else its chroma samples cover).  The
    arrays are shared between callers: treat them as read-only."""
    x0, y0 = origin
    rng = np.random.default_rng([w, h, bpc, hs, vs, x0, y0])
    s = 1 << (bpc - 8)
    top = (1 << bpc) - 1
    dt = dtype_of(bpc)
    cw, ch = chroma_size(w, h, hs, vs)
    ref = [rng.integers(16 * s, 235 * s + 1, (h, w)), rng.integers(64 * s, 191 * s + 1, (ch, cw)),
           rng.integers(64 * s, 191 * s + 1, (ch, cw))]
    dis = [p.copy() for p in ref]
    x1, y1 = min(x0 + PATCH, w), min(y0 + PATCH, h)
    assert 0 <= x0 < x1 and 0 <= y0 < y1
    dis[0][y0:y1, x0:x1] = np.minimum(dis[0][y0:y1, x0:x1] + rng.integers(20 * s, 59 * s + 1, (y1 - y0, x1 - x0)), top)
    cys, cxs = slice(y0 >> vs, ((y1 - 1) >> vs) + 1), slice(x0 >> hs, ((x1 - 1) >> hs) + 1)
    shape = dis[1][cys, cxs].shape
    dis[1][cys, cxs] += rng.integers(10 * s, 39 * s + 1, shape)
    dis[2][cys, cxs] -= rng.integers(10 * s, 39 * s + 1, shape)
    ref, dis = [p.astype(dt) for p in ref], [p.astype(dt) for p in dis]
    changed = ref[0] != dis[0]
    for p in (1, 2):
        changed |= R.upsample(ref[p] != dis[p], w, h, hs, vs)
    for p in ref + dis + [changed]:
        p.setflags(write=False)
    return ref, dis, changed


def patch_de(ref, dis, bpc, hs, vs, dtype=np.float64):
    """The frame's dE00 map in f64 storage (evaluated in `dtype`)."""
    return R.frame_de(ref, dis, bpc, hs, vs, dtype).astype(np.float64)


def min_hue_distance(ref, dis, changed, bpc, hs, vs):
    """Smallest distance (degrees) of a changed pixel's hue pair from the 180-degree jump of the mean-hue rule."""
    lr, ld = R.yuv_to_lab(*ref, bpc, hs, vs), R.yuv_to_lab(*dis, bpc, hs, vs)
    return float(R.hue_delta_from_180(*lr, *ld)[changed].min())


def bound(n_changed, want):
    return PAIR_TOL * (n_changed + want)


# ---- two wrong kernels, restated: what the construction has to notice -------------------------------------------------
def _full_res(planes, w, h, hs, vs):
    return [np.asarray(planes[0]), R.upsample(planes[1], w, h, hs, vs), R.upsample(planes[2], w, h, hs, vs)]


def mutant_last_column_sum(ref, dis, bpc, hs, vs):
    """dE00 sum of a kernel whose last luma column reads chroma column cx - 1."""
    h, w = ref[0].shape
    cx = (w - 1) >> hs
    out = []
    for planes in (ref, dis):
        f = _full_res(planes, w, h, hs, vs)
        for p in (1, 2):
            f[p] = f[p].copy()
            f[p][:, w - 1] = R.upsample(planes[p][:, cx - 1:cx], 1, h, 0, vs)[:, 0]
        out.append(f)
    return float(R.frame_de(out[0], out[1], bpc, 0, 0).sum())


def mutant_no_break_sum(ref, dis, bpc, hs, vs):
    """dE00 sum of a kernel without the horizontal `break`: the last chroma sample counts (1 << hs) luma pixels, the
    missing ones taken as copies of the last luma column."""
    h, w = ref[0].shape
    pad = (chroma_size(w, h, hs, vs)[0] << hs) - w
    out = []
    for planes in (ref, dis):
        f = _full_res([np.pad(planes[0], ((0, 0), (0, pad)), mode="edge"), planes[1], planes[2]], w + pad, h, hs, vs)
        out.append(f)
    return float(R.frame_de(out[0], out[1], bpc, 0, 0).sum())


def touches_last_column(w, origin):
    return origin[0] + PATCH >= w


def no_break_pad(w, hs):
    return (((w + (1 << hs) - 1) >> hs) << hs) - w


# ---- FFmpeg PSNR / SSIM ---------------------------------------------------------------------------------------------
PSNR_SSIM_CASES = [(19, 19, 8), (45, 39, 8), (150, 86, 8), (45, 39, 10), (45, 41, 8), (45, 39, 12), (150, 86, 12)]


def offset_pair(w, h, bpc, hs, vs, seed, n=1):
    """n frames of random samples over the whole range and copies offset by up to +-9 s per sample (clipped)."""
    rng = np.random.default_rng([seed, w, h, bpc, hs, vs])
    s = 1 << (bpc - 8)
    top = (1 << bpc) - 1
    dt = dtype_of(bpc)
    cw, ch = chroma_size(w, h, hs, vs)
    refs, diss = [], []
    for _ in range(n):
        ref = [rng.integers(0, top + 1, shp) for shp in ((h, w), (ch, cw), (ch, cw))]
        dis = [np.clip(p + rng.integers(-9 * s, 9 * s + 1, p.shape), 0, top) for p in ref]
        refs.append([p.astype(dt) for p in ref])
        diss.append([p.astype(dt) for p in dis])
    return refs, diss
