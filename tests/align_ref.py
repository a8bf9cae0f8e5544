"""numpy restatement of the banded cross-frame SSE (pqa_cross_sse, csrc/cross_sse.hip) and the clip generator its tests
share.  Test infrastructure only.

    D[i][c] = sum over luma pixels of (ref_i - dis_{i+k})^2,  k = k_lo + c;  UINT64_MAX where i + k is no captured frame"""
import numpy as np

SENTINEL = np.uint64((1 << 64) - 1)


def cross_sse(ref_lumas, dis_lumas, k_lo, k_hi):
    """[n_ref, k_hi - k_lo + 1] uint64 by direct int64 subtraction"""
    n_ref, n_dis, span = len(ref_lumas), len(dis_lumas), k_hi - k_lo + 1
    out = np.full((n_ref, span), SENTINEL, np.uint64)
    for i in range(n_ref):
        r = np.asarray(ref_lumas[i]).astype(np.int64)
        for c in range(span):
            j = i + k_lo + c
            if 0 <= j < n_dis:
                d = r - np.asarray(dis_lumas[j]).astype(np.int64)
                out[i, c] = np.uint64(int((d * d).sum()))
    return out


def shown(n, offset, repeats=(), drops=()):
    """the reference frame every captured frame shows (None: a frame in front of the reference's first picture): the
    reference without `drops`, delayed by `offset` frames (offset < 0: its first -offset frames are missing), then every
    captured frame number in `repeats` (ascending) repeats the frame before it"""
    seq = [None] * max(0, offset) + [r for r in range(max(0, -offset), n) if r not in set(drops)]
    for j in sorted(repeats):
        seq.insert(j, seq[j - 1])
    return seq


def planted_clip(w, h, bpc, n, offset, repeats=(), drops=(), seed=0):
    """(ref_lumas, dis_lumas): n reference frames of independent uniform noise; the capture is the reference re-timed
    (shown()), plus noise of -1 / 0 / +1 per sample, clipped.  Frames in front of the reference are noise of their own."""
    rng = np.random.default_rng(seed)
    dt = np.uint8 if bpc == 8 else np.uint16
    top = (1 << bpc) - 1
    ref = [rng.integers(0, top + 1, (h, w)).astype(dt) for _ in range(n)]
    dis = []
    for r in shown(n, offset, repeats, drops):
        base = rng.integers(0, top + 1, (h, w)) if r is None else ref[r].astype(np.int64)
        dis.append(np.clip(base + rng.integers(-1, 2, (h, w)), 0, top).astype(dt))
    return ref, dis


# the planted clips the GPU tests use: name -> (arguments of planted_clip, (k_lo, k_hi) of the test's band)
GPU_CLIPS = {
    "smallest": (dict(w=16, h=16, bpc=8, n=3, offset=0, seed=11), (-1, 1)),
    "tails": (dict(w=50, h=18, bpc=8, n=5, offset=2, seed=12), (-2, 3)),
    "tile_edge": (dict(w=48, h=32, bpc=8, n=40, offset=5, seed=13), (-9, 9)),
    "depth10": (dict(w=50, h=18, bpc=10, n=5, offset=-1, seed=14), (-2, 3)),
    "depth12": (dict(w=50, h=18, bpc=12, n=5, offset=1, seed=15), (-2, 3)),
    "end_to_end": (dict(w=64, h=48, bpc=8, n=24, offset=3, repeats=(26,), seed=16), (-8, 8)),
}


def gpu_clip(name):
    args, band = GPU_CLIPS[name]
    ref, dis = planted_clip(**args)
    return ref, dis, band
