"""Numpy restatement of the per-level transfer table (pqa_level_stats, csrc/level_stats.hip) and the seeded inputs of the
level alignment tests.  Not a test module.

    T[f][v][0] = number of pixels with ref == v,  T[f][v][1] = sum of dis over them,  T[f][v][2] = sum of dis^2 over them

for v = 0 ... L - 1, L = 2^bit_depth: the counts by np.bincount, the sums by np.add.at on int64 (bincount's weights would
be float64), so every entry is an exact integer (a 12-bit 2160p frame stays below 2^47).
The clamped-bin rule: a reference sample above L - 1 (a 16-bit container can hold one) is counted in bin L - 1; its
captured partner enters the sums as it is."""
import numpy as np


def level_stats(ref_frames, dis_frames, bit_depth: int) -> np.ndarray:
    L = 1 << bit_depth
    out = np.zeros((len(ref_frames), L, 3), np.uint64)
    for f, (r, d) in enumerate(zip(ref_frames, dis_frames)):
        r, d = np.asarray(r).astype(np.int64).ravel(), np.asarray(d).astype(np.int64).ravel()
        assert r.shape == d.shape
        b = np.minimum(r, L - 1)
        out[f, :, 0] = np.bincount(b, minlength=L)
        for k, wt in ((1, d), (2, d * d)):
            acc = np.zeros(L, np.int64)
            np.add.at(acc, b, wt)
            out[f, :, k] = acc.astype(np.uint64)
    return out


def table_sse(T) -> list:
    """sum_v (T2 - 2 v T1 + v^2 T0) of every frame, in Python ints: the squared error of the pair"""
    T = np.asarray(T)
    return [sum(int(T[f, v, 2]) - 2 * v * int(T[f, v, 1]) + v * v * int(T[f, v, 0]) for v in range(T.shape[1]))
            for f in range(T.shape[0])]


def random_pair(seed: int, n: int, w: int, h: int, bpc: int = 8):
    """n independent random reference and captured frames"""
    rng = np.random.default_rng(seed)
    dt = np.uint8 if bpc == 8 else np.uint16
    ref = [rng.integers(0, 1 << bpc, (h, w)).astype(dt) for _ in range(n)]
    dis = [rng.integers(0, 1 << bpc, (h, w)).astype(dt) for _ in range(n)]
    return ref, dis


def smooth_field(seed: int, w: int, h: int, lo: int, hi: int, t: int = 0, bpc: int = 8) -> np.ndarray:
    """a smooth field plus noise that fills lo ... hi (both reached), as samples of `bpc` bits"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    f = np.sin((xx + 3 * t) / 23.0) * np.cos((yy - 2 * t) / 17.0) + 0.6 * np.sin((xx + yy) / 41.0 + t) + rng.normal(0, 0.08, (h, w))
    f = (f - f.min()) / (f.max() - f.min())
    return np.round(lo + f * (hi - lo)).astype(np.uint8 if bpc == 8 else np.uint16)


def apply_map(plane: np.ndarray, a: float, b: float, bpc: int = 8, sigma: float = 0.0, seed: int = 0) -> np.ndarray:
    """the capture of `plane` under dis = a * ref + b: optional Gaussian noise, rounded to nearest and clipped to the range"""
    v = a * plane.astype(np.float64) + b
    if sigma:
        v = v + np.random.default_rng(seed).normal(0, sigma, plane.shape)
    return np.clip(np.floor(v + 0.5), 0, (1 << bpc) - 1).astype(plane.dtype)


# the five cases of the solver tests: name -> (reference range, generating a, generating b, expected kind, mismatch)
L2F = (255.0 / 219.0, -16.0 * 255.0 / 219.0)
F2L = (219.0 / 255.0, 16.0)
CASES = {
    "a_identity": ((0, 255), 1.0, 0.0, "identity", False),
    "b_limited_expanded": ((16, 235), L2F[0], L2F[1], "limited_to_full", True),
    "c_full_compressed": ((0, 255), F2L[0], F2L[1], "full_to_limited", True),
    "d_full_expanded_clipped": ((0, 255), L2F[0], L2F[1], "limited_to_full", True),
    "e_gain_offset": ((0, 255), 0.9, 7.0, "affine", True),
}


def case_pair(name: str, noise: bool, w: int = 320, h: int = 180, seed: int = 11):
    (lo, hi), a, b, _, _ = CASES[name]
    ref = smooth_field(seed, w, h, lo, hi)
    return ref, apply_map(ref, a, b, 8, 2.0 if noise else 0.0, seed + 1)


def apply_lut(plane: np.ndarray, lut: np.ndarray) -> np.ndarray:
    return np.take(lut, plane)
