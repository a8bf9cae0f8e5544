"""Numpy restatement of the temporal moments (pqa_temporal_moments, csrc/temporal_moments.hip) in int64, and of nothing else.
With R_f / D_f the reference / captured plane of frame f (a sample above 2^bit_depth - 1 is read as that) and, per pixel of
transition k = 1 ... n - 1, a = R_k - R_{k-1}, b = D_k - D_{k-1}, e = D_k - R_k: per tile of T x T pixels (edge tiles hold the
pixels that exist) the sums of a, b, a^2, b^2, a b, a e and e^2; words 0, 1, 4, 5 are int64 stored in the uint64 word."""
import numpy as np

SUMS = 7
SIGNED = (0, 1, 4, 5)


def temporal_moments(ref_frames, dis_frames, tile: int = 32, bit_depth: int = 8) -> np.ndarray:
    """[max(n - 1, 0), ty, tx, 7] uint64 of two lists of 2-D planes of one size"""
    top = (1 << bit_depth) - 1
    n = len(ref_frames)
    if n == 0:
        return np.zeros((0, 0, 0, SUMS), np.uint64)
    h, w = np.shape(ref_frames[0])
    ty, tx = -(-h // tile), -(-w // tile)
    out = np.zeros((max(n - 1, 0), ty, tx, SUMS), np.int64)
    R = [np.minimum(np.asarray(f).astype(np.int64), top) for f in ref_frames]
    D = [np.minimum(np.asarray(f).astype(np.int64), top) for f in dis_frames]
    for k in range(1, n):
        a, b, e = R[k] - R[k - 1], D[k] - D[k - 1], D[k] - R[k]
        for m, v in enumerate((a, b, a * a, b * b, a * b, a * e, e * e)):
            pad = np.zeros((ty * tile, tx * tile), np.int64)      # zeros add nothing to a sum
            pad[:h, :w] = v
            out[k - 1, :, :, m] = pad.reshape(ty, tile, tx, tile).sum(axis=(1, 3), dtype=np.int64)
    return out.view(np.uint64)


def signed(M) -> np.ndarray:
    """the moments as int64: every word is below 2^36 in magnitude, so the view is the value"""
    return np.ascontiguousarray(M).view(np.int64)
