"""Numpy restatement of the table apply (pqa_table_apply, csrc/table_apply.hip) and the seeded inputs of the transfer-curve
tests.  Not a test module.

    out[y][x] = table[min(plane[y][x], L - 1)],  L = 2^bit_depth

for any table of L entries of the sample type, monotone or not: numpy.take behind the clamp a 16-bit container needs."""
import numpy as np


def table_apply(plane: np.ndarray, table: np.ndarray, bit_depth: int) -> np.ndarray:
    L = 1 << bit_depth
    table = np.asarray(table)
    assert table.shape == (L,) and int(table.max()) < L
    return np.take(table, np.minimum(np.asarray(plane), L - 1)).astype(plane.dtype)


def gamma_capture(ref: np.ndarray, gamma: float, bpc: int = 8, sigma: float = 0.0, seed: int = 5) -> np.ndarray:
    """the capture top * (ref / top)^gamma of `ref`: optional Gaussian noise, rounded to nearest and clipped to the range"""
    top = (1 << bpc) - 1
    v = top * (ref.astype(np.float64) / top) ** gamma
    if sigma:
        v = v + np.random.default_rng(seed).normal(0, sigma, ref.shape)
    return np.clip(np.floor(v + 0.5), 0, top).astype(ref.dtype)


def mse(a: np.ndarray, b: np.ndarray) -> float:
    return float(((a.astype(np.int64) - b.astype(np.int64)) ** 2).mean())


def hand_table(bit_depth: int, rows) -> np.ndarray:
    """T[1][L][3] from {level: (count, sum of dis, sum of dis^2)}; a missing sum of squares is filled in as that of `count`
    equal samples when the mean is whole, else as count * ceil(mean)^2 (only its being large enough matters)"""
    T = np.zeros((1, 1 << bit_depth, 3), np.uint64)
    for v, row in rows.items():
        c, s = row[0], row[1]
        m = -(-s // c)
        T[0, v] = (c, s, row[2] if len(row) > 2 else c * m * m)
    return T
