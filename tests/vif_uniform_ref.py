"""Clips and float64 premises for the wave-uniform fast path of the VIF statistic (tests/test_vif_uniform.py on the CPU,
tests/test_gpu_vif_uniform.py on the GPU).  TEST INFRASTRUCTURE.

The kernels take a shortened statistic when every pixel of a wave is inside the image and at or above sigma_nsq = 2
(vif_march.hip pass2: the wave's 16 x 16 block; vif.hip vif_hstat: the 4-column segments of a wave's lanes, 8 rows).  The
clips here hold all three kinds of wave -- all-high, all-low, mixed -- at sizes where some waves are partly outside the
image; the CPU test counts them in float64 with a margin, so that the GPU comparison cannot pass by never leaving one path.
"""
import functools

import numpy as np

from oracle import np_restatement as R

SIZES = ((272, 272), (264, 250))   # 17 x 17 full blocks and three march segments; a partial last stripe / block row / tiles
SEAM = 100                         # column of the flat | noise seam: not a multiple of 16
BAR = 40                           # rows of the flat bars
PATCH = (112, 96, 32)              # x, y, side of the noise patch
HIGH, LOW = 4.0, 1.0               # float64 margins around sigma_nsq = 2: a pixel counts as high above 4, as low below 1
SEED = 20240917
KINDS = ("flat", "noise", "seam", "straddle", "bars", "patch", "dis_flat")


def _mid(bpc):
    return 128 << (bpc - 8)


@functools.lru_cache(maxsize=None)
def clip(w, h, bpc):
    """(refs, diss): one frame per entry of KINDS.  dis = gain x (ref - mid) + mid + noise, clipped (noise over flat
    reference regions too, so that the low branch sums something other than 1); the last frame's dis is flat where its
    reference is textured."""
    rng = np.random.default_rng(SEED + 1000 * bpc + w)
    dt = np.uint8 if bpc <= 8 else np.uint16
    peak, mid, unit = (1 << bpc) - 1, _mid(bpc), 1 << (bpc - 8)
    flat = np.full((h, w), mid, np.int64)
    noise = lambda: rng.integers(0, peak + 1, (h, w))
    refs = []
    refs.append(flat.copy())
    refs.append(noise())
    f = flat.copy(); f[:, SEAM:] = noise()[:, SEAM:]; refs.append(f)
    refs.append(mid + unit * rng.integers(-2, 3, (h, w)))
    f = noise(); f[:BAR] = mid; f[-BAR:] = mid; refs.append(f)
    f = flat.copy(); x, y, s = PATCH; f[y:y + s, x:x + s] = noise()[y:y + s, x:x + s]; refs.append(f)
    refs.append(noise())
    diss = []
    for k, r in enumerate(refs):
        if KINDS[k] == "dis_flat":
            d = flat.copy()
        else:
            d = np.rint(0.9 * (r - mid) + mid).astype(np.int64) + unit * rng.integers(-6, 7, (h, w))
        diss.append(np.clip(d, 0, peak).astype(dt))
    refs = [np.clip(r, 0, peak).astype(dt) for r in refs]
    for a in refs + diss:
        a.setflags(write=False)
    return tuple(refs), tuple(diss)


def sigma1_sq(ref_plane, bpc, scale):
    """float64 sigma1_sq of the reference at VIF scale 0 or 1 (libvmaf's filters and border rule)."""
    x = R.picture_copy(ref_plane, bpc)
    for s, n in enumerate((17, 9)[:scale + 1]):
        f = R.gaussian_taps(n)
        if s > 0:
            x = R._sep(x, f)[::2, ::2][: x.shape[0] // 2, : x.shape[1] // 2]
    mu = R._sep(x, f)
    return R._sep(x * x, f) - mu * mu


def _kind(v):
    hi, lo = v > HIGH, v < LOW
    if hi.all():
        return "high"
    if lo.all():
        return "low"
    if hi.any() and lo.any():
        return "mixed"
    return "margin"


def block_kinds(s1):
    """Kinds of the full 16 x 16 blocks of a scale-0 plane (the march kernel's waves that lie inside the image)."""
    h, w = s1.shape
    return [_kind(s1[y:y + 16, x:x + 16]) for y in range(0, h - 15, 16) for x in range(0, w - 15, 16)]


def wave_kinds_s1(s1):
    """Kinds of the waves of vif_stat_kernel<., 9, 248, 5> whose pixels all lie inside a scale-1 plane narrower than one 248-
    column tile: tile rows of 8; wave v of a workgroup holds the 4-column segments 2 a + (v & 1) + 8 b + 32 (v >> 1),
    a, b = 0..3 (vif_hstat's lane map)."""
    h, w = s1.shape
    assert w <= 248
    out = []
    for y in range(0, h - 7, 8):
        for v in range(4):
            segs = [2 * a + (v & 1) + 8 * b + 32 * (v >> 1) for a in range(4) for b in range(4)]
            segs = [s for s in segs if s < 62]
            if not segs or any(4 * s + 4 > w for s in segs):
                continue
            out.append(_kind(np.concatenate([s1[y:y + 8, 4 * s:4 * s + 4] for s in segs], axis=1)))
    return out


@functools.lru_cache(maxsize=None)
def census(w, h, bpc):
    """({kind: count} over the clip at scale 0, the same over the waves of scale 1)."""
    refs, _ = clip(w, h, bpc)
    c0 = {k: 0 for k in ("high", "low", "mixed", "margin")}
    c1 = dict(c0)
    for r in refs:
        for k in block_kinds(sigma1_sq(r, bpc, 0)):
            c0[k] += 1
        for k in wave_kinds_s1(sigma1_sq(r, bpc, 1)):
            c1[k] += 1
    return c0, c1
