"""Restatement of the band moments (pqa_band_moments, csrc/band_moments.hip) with Python ints, and of the split of
pqa2_amd/spectrum.py in fractions.Fraction.  A_0 is the plane (a sample above 2^bit_depth - 1 is read as that); for
l = 1 ... L, W_l = W >> l, H_l = H >> l and a b / c e the 2 x 2 parents of A_{l-1}:
    A_l = a + b + c + e    H_l = a - b + c - e    V_l = a + b - c - e    D_l = a - b - c + e
out[f][l-1][o][k], o: 0 H, 1 V, 2 D, 3 A, k: 0 sum r_o^2, 1 sum d_o^2, 2 sum r_o d_o (int64 in the word).  The coefficients
are formed in int64 arrays (|coefficient| <= 4095 * 4^6 < 2^24, products below 2^48); every sum is taken over Python ints."""
from fractions import Fraction

import numpy as np

H, V, D, A = range(4)


def haar_levels(plane, levels: int, bit_depth: int = 8):
    """[(H_l, V_l, D_l, A_l)] for l = 1 ... levels as int64 arrays of H_l x W_l (possibly empty)"""
    a0 = np.minimum(np.asarray(plane).astype(np.int64), (1 << bit_depth) - 1)
    out = []
    for _ in range(levels):
        h2, w2 = a0.shape[0] // 2, a0.shape[1] // 2
        a, b = a0[0:2 * h2:2, 0:2 * w2:2], a0[0:2 * h2:2, 1:2 * w2:2]
        c, e = a0[1:2 * h2:2, 0:2 * w2:2], a0[1:2 * h2:2, 1:2 * w2:2]
        out.append((a - b + c - e, a + b - c - e, a - b - c + e, a + b + c + e))
        a0 = out[-1][A]
    return out


def _isum(x) -> int:
    """the sum of an int64 array as a Python int: rows in int64 (a row of 4096 products below 2^48 stays below 2^60)"""
    return sum(int(v) for v in x.sum(axis=1, dtype=np.int64)) if x.size else 0


def band_moments(ref_frames, dis_frames, levels: int = 4, bit_depth: int = 8) -> np.ndarray:
    """[n, L, 4, 3] uint64 of two lists of 2-D planes of one size"""
    out = np.zeros((len(ref_frames), levels, 4, 3), np.uint64)
    for f, (rf, df) in enumerate(zip(ref_frames, dis_frames)):
        rl, dl = haar_levels(rf, levels, bit_depth), haar_levels(df, levels, bit_depth)
        for l in range(levels):
            for o in range(4):
                r, d = rl[l][o], dl[l][o]
                for k, s in enumerate((_isum(r * r), _isum(d * d), _isum(r * d))):
                    out[f, l, o, k] = np.uint64(s % (1 << 64))
    return out


def band_moments_loops(ref, dis, levels: int, bit_depth: int = 8):
    """the same for one pair with plain loops over Python ints: [L][4][3] (signed)"""
    top = (1 << bit_depth) - 1
    ar = [[min(int(v), top) for v in row] for row in np.asarray(ref)]
    ad = [[min(int(v), top) for v in row] for row in np.asarray(dis)]
    out = []
    for _ in range(levels):
        hl, wl = len(ar) // 2, (len(ar[0]) // 2 if ar else 0)
        sums = [[0, 0, 0] for _ in range(4)]
        nr, nd = [], []
        for j in range(hl):
            nr.append([])
            nd.append([])
            for i in range(wl):
                co = []
                for x in (ar, ad):
                    a, b, c, e = x[2 * j][2 * i], x[2 * j][2 * i + 1], x[2 * j + 1][2 * i], x[2 * j + 1][2 * i + 1]
                    co.append((a - b + c - e, a + b - c - e, a - b - c + e, a + b + c + e))
                for o in range(4):
                    sums[o][0] += co[0][o] * co[0][o]
                    sums[o][1] += co[1][o] * co[1][o]
                    sums[o][2] += co[0][o] * co[1][o]
                nr[-1].append(co[0][A])
                nd[-1].append(co[1][A])
        out.append(sums)
        ar, ad = nr, nd
    return out


def signed(M):
    """the moments as Python ints in an object array, the cross sums read as int64"""
    M = np.asarray(M)
    S = M.astype(object)
    S[..., 2] = M[..., 2].view(np.int64).astype(object)
    return S


def split(rr: int, dd: int, rd: int):
    """(gain, err, loss, noise) of one band as Fractions; gain None and everything noise when the reference band is empty"""
    err = Fraction(rr - 2 * rd + dd)
    if rr == 0:
        return None, err, Fraction(0), err
    g = Fraction(rd, rr)
    return g, err, (1 - g) ** 2 * rr, dd - g * g * rr


def h_blur(plane):
    """([1 2 1] + 2) >> 2 along the rows with edge replication"""
    p = np.asarray(plane).astype(np.int64)
    q = np.pad(p, ((0, 0), (1, 1)), mode="edge")
    return ((q[:, :-2] + 2 * q[:, 1:-1] + q[:, 2:] + 2) >> 2).astype(np.asarray(plane).dtype)


def noise_plane(seed: int, w: int, h: int, bpc: int = 8):
    return np.random.default_rng(seed).integers(0, 1 << bpc, (h, w)).astype(np.uint8 if bpc == 8 else np.uint16)


def add_noise(plane, seed: int, amp: int = 8, bpc: int = 8):
    rng = np.random.default_rng(seed)
    p = np.asarray(plane)
    return np.clip(p.astype(np.int64) + rng.integers(-amp, amp + 1, p.shape), 0, (1 << bpc) - 1).astype(p.dtype)


def random_pairs(seed: int, n: int, w: int, h: int, bpc: int = 8):
    rng = np.random.default_rng(seed)
    dt = np.uint8 if bpc == 8 else np.uint16
    return ([rng.integers(0, 1 << bpc, (h, w)).astype(dt) for _ in range(n)],
            [rng.integers(0, 1 << bpc, (h, w)).astype(dt) for _ in range(n)])
