"""Numpy restatement of the edge profiles (pqa_edge_profiles, csrc/edge_profiles.hip) in int64, and of nothing else.  With R / D
the reference / captured plane of a frame (a sample above 2^bit_depth - 1 is read as that): column line x = 1 ... W - 1 holds
the sums over y of a^2, b^2 and a b with a = R[y][x] - R[y][x-1], b = D[y][x] - D[y][x-1]; row line y = 1 ... H - 1 the sums
over x with a = R[y][x] - R[y-1][x], b likewise; line 0 of each axis is zero; word 2 is int64 stored in the uint64 word."""
import numpy as np

SUMS = 3


def edge_profiles(ref_frames, dis_frames, bpc: int = 8):
    """(rows [n, H, 3], cols [n, W, 3]) uint64 of two lists of 2-D planes of one size"""
    top = (1 << bpc) - 1
    n = len(ref_frames)
    if n == 0:
        return np.zeros((0, 0, SUMS), np.uint64), np.zeros((0, 0, SUMS), np.uint64)
    h, w = np.shape(ref_frames[0])
    rows, cols = np.zeros((n, h, SUMS), np.int64), np.zeros((n, w, SUMS), np.int64)
    for f in range(n):
        R = np.minimum(np.asarray(ref_frames[f]).astype(np.int64), top)
        D = np.minimum(np.asarray(dis_frames[f]).astype(np.int64), top)
        a, b = R[:, 1:] - R[:, :-1], D[:, 1:] - D[:, :-1]
        for m, v in enumerate((a * a, b * b, a * b)):
            cols[f, 1:, m] = v.sum(axis=0, dtype=np.int64)
        a, b = R[1:] - R[:-1], D[1:] - D[:-1]
        for m, v in enumerate((a * a, b * b, a * b)):
            rows[f, 1:, m] = v.sum(axis=1, dtype=np.int64)
    return rows.view(np.uint64), cols.view(np.uint64)


def random_frames(n: int, h: int, w: int, bpc: int = 8, seed: int = 0, over: bool = False) -> list:
    """n planes of h x w samples of the full range of the bit depth (over: of the u16 container, above top too)"""
    rng = np.random.default_rng(seed)
    hi = 1 << (16 if over and bpc > 8 else bpc)
    return [rng.integers(0, hi, (h, w)).astype(np.uint8 if bpc == 8 else np.uint16) for _ in range(n)]
