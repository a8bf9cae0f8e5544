"""numpy restatement of the exact-integer resampler (pqa_resample; include/pqa_vmaf.h): the coefficient
table of one axis as a dense integer matrix, and the two integer passes with their rounding shifts."""
import math

import numpy as np

FILTERS = {"bilinear": 0, "bicubic": 1, "lanczos": 2}
SUPPORT = (1.0, 2.0, 3.0)
Q16 = 65536


def q16(v):
    """a source coordinate or extent as the signed Q16 integer the library takes"""
    return int(round(v * Q16))


def _sinc(t):
    if t == 0.0:
        return 1.0
    u = math.pi * t
    return math.sin(u) / u


def kernel(filt, t):
    x = abs(t)
    if filt == 0:
        return 1.0 - x if x < 1.0 else 0.0
    if filt == 1:
        a = -0.6
        if x <= 1.0:
            return (a + 2.0) * x * x * x - (a + 3.0) * x * x + 1.0
        if x < 2.0:
            return a * x * x * x - 5.0 * a * x * x + 8.0 * a * x - 4.0 * a
        return 0.0
    return _sinc(t) * _sinc(t / 3.0) if x < 3.0 else 0.0


def weights(filt, n_dst, x0_q16, ext_q16, i):
    """(first tap j0, the normalised double weights of destination sample i) before quantisation and folding"""
    x0, ext = x0_q16 / Q16, ext_q16 / Q16
    step = ext / n_dst
    stretch = max(1.0, step)
    S = SUPPORT[filt] * stretch
    c = x0 + (i + 0.5) * step - 0.5
    j0, j1 = math.ceil(c - S), math.floor(c + S)
    w = [kernel(filt, (j - c) / stretch) for j in range(j0, j1 + 1)]
    total = 0.0
    for v in w:
        total += v
    return j0, [v / total for v in w]


def table(filt, n_src, n_dst, x0_q16=0, ext_q16=None, quantise=True):
    """the [n_dst, n_src] matrix of one axis: int64 coefficients at scale 2^14 (rows sum to 16384), or with quantise=False
    the float64 weights they are rounded from; edge replication is folded in"""
    filt = FILTERS.get(filt, filt)
    ext_q16 = n_src * Q16 if ext_q16 is None else ext_q16
    out = np.zeros((n_dst, n_src), np.int64 if quantise else np.float64)
    for i in range(n_dst):
        j0, w = weights(filt, n_dst, x0_q16, ext_q16, i)
        if quantise:
            w = [math.floor(v * 16384.0 + 0.5) for v in w]
            w[w.index(max(w))] += 16384 - sum(w)     # the first of equals
        for t, v in enumerate(w):
            out[i, min(max(j0 + t, 0), n_src - 1)] += v
    return out


def dense(first, coeff, n_src):
    """the library's own table (pqa_debug_resample_table: first [n_dst], coeff [n_dst, taps]) as the same dense matrix"""
    n_dst, taps = coeff.shape
    out = np.zeros((n_dst, n_src + taps), np.int64)
    for i in range(n_dst):
        out[i, first[i]:first[i] + taps] = coeff[i]
    assert not out[:, n_src:].any()
    return out[:, :n_src]


def apply(src, table_h, table_v, b):
    """src [h, w] -> [table_v rows, table_h rows]: the horizontal pass first, both in int64 with the two rounding shifts"""
    s = np.asarray(src).astype(np.int64)
    acc = s @ np.asarray(table_h, np.int64).T
    mid = (acc + (1 << (b - 1))) >> b
    assert np.abs(mid).max() < 32768
    acc2 = np.asarray(table_v, np.int64) @ mid
    assert np.abs(acc2).max() < 2 ** 31
    out = np.clip((acc2 + (1 << (27 - b))) >> (28 - b), 0, (1 << b) - 1)
    return out.astype(np.uint8 if b == 8 else np.uint16)


def apply_float(src, table_h, table_v, b):
    """the same filter in float64 with unquantised weights; one rounding, at the end"""
    out = np.asarray(table_v, np.float64) @ np.asarray(src, np.float64) @ np.asarray(table_h, np.float64).T
    return np.clip(np.floor(out + 0.5), 0, (1 << b) - 1).astype(np.uint8 if b == 8 else np.uint16)


def resize(src, dst_shape, filt, b, window=None):
    """a whole plane through the restatement's own tables; window = (x0, y0, w, h) in source samples"""
    h, w = src.shape
    x0, y0, ww, wh = window if window is not None else (0, 0, w, h)
    return apply(src, table(filt, w, dst_shape[1], q16(x0), q16(ww)), table(filt, h, dst_shape[0], q16(y0), q16(wh)), b)


def replicated_crop(src, x0, y0):
    """src moved by whole samples: out[y][x] = src[clamp(y + y0)][clamp(x + x0)]"""
    h, w = src.shape
    return src[np.clip(np.arange(h) + y0, 0, h - 1)][:, np.clip(np.arange(w) + x0, 0, w - 1)]


def noise(seed, w, h, b):
    """independent uniform noise over the full sample range, with a row of 0 and a row of 2^b - 1"""
    rng = np.random.default_rng(seed)
    p = rng.integers(0, 1 << b, (h, w)).astype(np.uint8 if b == 8 else np.uint16)
    p[h // 3] = 0
    p[(2 * h) // 3] = (1 << b) - 1
    return p


def psnr(a, b, peak=255.0):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 10.0 * math.log10(peak * peak / mse)
