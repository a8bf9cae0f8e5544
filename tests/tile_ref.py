"""Numpy restatement of the tile moments (pqa_tile_moments, csrc/tile_moments.hip) and of the block SSIM of
pqa2_amd/distortion.py.  Moments: per tile of T x T pixels (edge tiles hold the pixels that exist) the sums of r, d, r^2, d^2,
r d and |d - r|, uint64; a sample above 2^bit_depth - 1 is read as that.  Metrics: evaluated in fractions.Fraction."""
from fractions import Fraction

import numpy as np


def tile_moments(ref_frames, dis_frames, tile: int = 32, bit_depth: int = 8) -> np.ndarray:
    """[n, ty, tx, 6] uint64 of two lists of 2-D planes of one size"""
    top = (1 << bit_depth) - 1
    if not ref_frames:
        return np.zeros((0, 0, 0, 6), np.uint64)
    h, w = np.shape(ref_frames[0])
    ty, tx = -(-h // tile), -(-w // tile)
    out = np.zeros((len(ref_frames), ty, tx, 6), np.uint64)
    for f, (rf, df) in enumerate(zip(ref_frames, dis_frames)):
        r = np.minimum(np.asarray(rf).astype(np.int64), top)
        d = np.minimum(np.asarray(df).astype(np.int64), top)
        for k, v in enumerate((r, d, r * r, d * d, r * d, np.abs(d - r))):
            pad = np.zeros((ty * tile, tx * tile), np.uint64)      # zeros add nothing to a sum
            pad[:h, :w] = v.astype(np.uint64)
            out[f, :, :, k] = pad.reshape(ty, tile, tx, tile).sum(axis=(1, 3), dtype=np.uint64)
    return out


def tile_sse(M) -> np.ndarray:
    """[..., ty, tx] tile SSE as Python ints in an object array: sum r^2 - 2 sum r d + sum d^2"""
    M = np.asarray(M).astype(object)
    return M[..., 2] + M[..., 3] - 2 * M[..., 4]


def counts(width: int, height: int, tile: int):
    ty, tx = -(-height // tile), -(-width // tile)
    return [[min(tile, height - j * tile) * min(tile, width - i * tile) for i in range(tx)] for j in range(ty)]


def block_metrics(m, n: int, bit_depth: int):
    """(mse, mad, ssim) of one tile as Fractions: m = its six sums, n = its pixels.  SSIM is the block form
    ((2 ur ud + C1)(2 srd + C2)) / ((ur^2 + ud^2 + C1)(sr^2 + sd^2 + C2)) with biased variances, C1 = (top / 100)^2,
    C2 = (3 top / 100)^2."""
    sr, sd, srr, sdd, srd, sad = (int(v) for v in m)
    top = (1 << bit_depth) - 1
    c1, c2 = Fraction(top, 100) ** 2, Fraction(3 * top, 100) ** 2
    ur, ud = Fraction(sr, n), Fraction(sd, n)
    vr, vd, cov = Fraction(srr, n) - ur * ur, Fraction(sdd, n) - ud * ud, Fraction(srd, n) - ur * ud
    ssim = ((2 * ur * ud + c1) * (2 * cov + c2)) / ((ur * ur + ud * ud + c1) * (vr + vd + c2))
    return Fraction(srr + sdd - 2 * srd, n), Fraction(sad, n), ssim


def psnr_of(mse: np.ndarray, bit_depth: int) -> np.ndarray:
    """the PSNR of an array of MSE values in float64, capped as the project caps psnr_y: 6 b + 12 dB"""
    top = float((1 << bit_depth) - 1)
    mse = np.asarray(mse, np.float64)
    with np.errstate(divide="ignore"):
        db = np.where(mse > 0, 10.0 * np.log10(top * top / np.where(mse > 0, mse, 1.0)), np.inf)
    return np.minimum(db, 6.0 * bit_depth + 12.0)


def random_pairs(seed: int, n: int, w: int, h: int, bpc: int = 8, noise: int | None = None):
    """n plane pairs of w x h: uniform noise over the whole code range; the captured planes independent noise too, or with
    `noise` the reference plus uniform noise of that amplitude"""
    rng = np.random.default_rng(seed)
    dt = np.uint8 if bpc == 8 else np.uint16
    ref = [rng.integers(0, 1 << bpc, (h, w)).astype(dt) for _ in range(n)]
    if noise is None:
        dis = [rng.integers(0, 1 << bpc, (h, w)).astype(dt) for _ in range(n)]
    else:
        dis = [np.clip(r.astype(np.int64) + rng.integers(-noise, noise + 1, r.shape), 0, (1 << bpc) - 1).astype(dt) for r in ref]
    return ref, dis
