"""numpy / Python-int restatement of the colour-matrix alignment kernels (csrc/colour_moments.hip; include/pqa_vmaf.h:
pqa_colour_moments, pqa_colour_apply) and the seeded clips of tests/test_colour.py and tests/test_gpu_colour.py.  A frame is a
list [Y, U, V] of 2-D arrays; chroma planes are ceil(w / 2^hs) x ceil(h / 2^vs)."""
import numpy as np


def chroma_shape(w, h, hs, vs):
    return (-(-h // (1 << vs)), -(-w // (1 << hs)))


def dtype_of(bit_depth):
    return np.uint8 if bit_depth <= 8 else np.dtype("<u2")


def _blocks(Y, hs, vs):
    """[2^vs][2^hs] arrays on the chroma grid: the luma samples under every chroma sample, coordinates clamped to the plane"""
    h, w = Y.shape
    ch, cw = chroma_shape(w, h, hs, vs)
    ys = np.minimum((np.arange(ch)[:, None] << vs), h - 1), np.arange(cw)[None, :] << hs
    return [[Y[np.minimum(ys[0] + j, h - 1), np.minimum(ys[1] + i, w - 1)] for i in range(1 << hs)] for j in range(1 << vs)]


def block_sum(Y, hs, vs, top=None):
    """SY on the chroma grid (int64)"""
    Y = np.asarray(Y).astype(np.int64)
    if top is not None:
        Y = np.minimum(Y, top)
    return sum(b for row in _blocks(Y, hs, vs) for b in row)


def colour_moments(ref_frames, dis_frames, bit_depth, hs, vs, lo=None, hi=None):
    """[n, 28] uint64: per frame pair the upper triangle, row-major, of the sum of z z^T over the unmasked chroma samples, z =
    (1, SYr, Ur, Vr, SYd, Ud, Vd); a sample enters only if every captured luma sample under it, Ud and Vd lie in lo ... hi
    (default 1 ... top - 1); samples above top are read as top"""
    top = (1 << bit_depth) - 1
    lo, hi = (1 if lo is None else lo), (top - 1 if hi is None else hi)
    out = np.zeros((len(ref_frames), 28), np.uint64)
    for f, (r, d) in enumerate(zip(ref_frames, dis_frames)):
        r = [np.minimum(np.asarray(p).astype(np.int64), top) for p in r]
        d = [np.minimum(np.asarray(p).astype(np.int64), top) for p in d]
        keep = (d[1] >= lo) & (d[1] <= hi) & (d[2] >= lo) & (d[2] <= hi)
        for row in _blocks(d[0], hs, vs):
            for b in row:
                keep &= (b >= lo) & (b <= hi)
        z = [keep.astype(np.int64), block_sum(r[0], hs, vs), r[1], r[2], block_sum(d[0], hs, vs), d[1], d[2]]
        z = [z[0]] + [v * z[0] for v in z[1:]]
        e = 0
        for i in range(7):
            for j in range(i, 7):
                out[f, e] = int((z[i] * z[j]).sum())
                e += 1
    return out


def apply(planes, m, bit_depth, hs, vs):
    """[Y', U', V'] of one frame through the Q14 matrix m[12] (rows: offset, gains of Y, U, V), as pqa_colour_apply:
    Y' = clamp((m0 + m1 Y + m2 U(c) + m3 V(c) + 2^13) >> 14, 0, top), U' = clamp((m4 s + m5 SY + s m6 U + s m7 V + s 2^13) >>
    (14 + hs + vs), 0, top), V' with m8 ... m11"""
    top = (1 << bit_depth) - 1
    m = [int(v) for v in np.asarray(m).reshape(12)]
    Y, U, V = (np.minimum(np.asarray(p).astype(np.int64), top) for p in planes)
    h, w = Y.shape
    cy, cx = np.arange(h)[:, None] >> vs, np.arange(w)[None, :] >> hs
    s = 1 << (hs + vs)
    y2 = np.clip((m[0] + m[1] * Y + m[2] * U[cy, cx] + m[3] * V[cy, cx] + 8192) >> 14, 0, top)
    sy = block_sum(Y, hs, vs)
    u2 = np.clip((m[4] * s + m[5] * sy + s * m[6] * U + s * m[7] * V + s * 8192) >> (14 + hs + vs), 0, top)
    v2 = np.clip((m[8] * s + m[9] * sy + s * m[10] * U + s * m[11] * V + s * 8192) >> (14 + hs + vs), 0, top)
    dt = dtype_of(bit_depth)
    return [y2.astype(dt), u2.astype(dt), v2.astype(dt)]


def convert(planes, A, b, bit_depth, hs, vs, noise=None, clip=True):
    """One frame through the map dis = A ref + b (Fractions or floats; pqa2_amd.align.named_colour_map), as a capture chain
    would: luma converted per pixel with replicated chroma, chroma from the block MEAN of the luma; `noise` (sigma, rng)
    adds Gaussian noise before rounding; rounded half up and clipped to 0 ... top.  clip=False: float planes, not rounded."""
    top = (1 << bit_depth) - 1
    A = [[float(v) for v in r] for r in A]
    b = [float(v) for v in b]
    Y, U, V = (np.asarray(p).astype(np.float64) for p in planes)
    h, w = Y.shape
    cy, cx = np.arange(h)[:, None] >> vs, np.arange(w)[None, :] >> hs
    ym = sum(bk for row in _blocks(Y, hs, vs) for bk in row) / (1 << (hs + vs))
    out = [b[0] + A[0][0] * Y + A[0][1] * U[cy, cx] + A[0][2] * V[cy, cx],
           b[1] + A[1][0] * ym + A[1][1] * U + A[1][2] * V,
           b[2] + A[2][0] * ym + A[2][1] * U + A[2][2] * V]
    if noise is not None:
        sigma, rng = noise
        out = [p + rng.normal(0.0, sigma, p.shape) for p in out]
    if not clip:
        return out
    return [np.clip(np.floor(p + 0.5), 0, top).astype(dtype_of(bit_depth)) for p in out]


def _field(rng, h, w, lo, hi, cell):
    """a textured field in lo ... hi: bilinear blobs of `cell` pixels plus fine noise"""
    gh, gw = h // cell + 2, w // cell + 2
    g = rng.uniform(0.0, 1.0, (gh, gw))
    yy, xx = np.arange(h)[:, None] / cell, np.arange(w)[None, :] / cell
    y0, x0 = yy.astype(int), xx.astype(int)
    fy, fx = yy - y0, xx - x0
    v = (g[y0, x0] * (1 - fy) * (1 - fx) + g[y0, x0 + 1] * (1 - fy) * fx + g[y0 + 1, x0] * fy * (1 - fx) + g[y0 + 1, x0 + 1] * fy * fx)
    v = 0.85 * v + 0.15 * rng.uniform(0.0, 1.0, (h, w))
    return lo + (hi - lo) * v


def clip(seed, w, h, bit_depth, hs, vs, n=4, full_range=False, margin=0.16, chroma_margin=0.04):
    """n frames [Y, U, V] of a seeded synthetic clip: textured luma and two independent chroma fields, luma kept `margin` and chroma
    `chroma_margin` of the range away from its ends, so that a matrix conversion between the standards clips next to nothing"""
    rng = np.random.default_rng(seed)
    f = 1 << (bit_depth - 8)
    top = (1 << bit_depth) - 1
    (ylo, yhi), (clo, chi) = ((0, top), (0, top)) if full_range else ((16 * f, 235 * f), (16 * f, 240 * f))
    ym, cm = margin * (yhi - ylo), chroma_margin * (chi - clo)
    ch, cw = chroma_shape(w, h, hs, vs)
    dt = dtype_of(bit_depth)
    out = []
    for _ in range(n):
        out.append([np.floor(_field(rng, h, w, ylo + ym, yhi - ym, 6) + 0.5).astype(dt),
                    np.floor(_field(rng, ch, cw, clo + cm, chi - cm, 5) + 0.5).astype(dt),
                    np.floor(_field(rng, ch, cw, clo + cm, chi - cm, 7) + 0.5).astype(dt)])
    return out


def noise_frames(seed, w, h, bit_depth, hs, vs, n=1):
    """n frames of uniform noise over the whole code range"""
    rng = np.random.default_rng(seed)
    top = (1 << bit_depth) - 1
    ch, cw = chroma_shape(w, h, hs, vs)
    dt = dtype_of(bit_depth)
    return [[rng.integers(0, top + 1, (h, w)).astype(dt), rng.integers(0, top + 1, (ch, cw)).astype(dt),
             rng.integers(0, top + 1, (ch, cw)).astype(dt)] for _ in range(n)]


def plane_sse(a, b):
    return [int(((np.asarray(x).astype(np.int64) - np.asarray(y).astype(np.int64)) ** 2).sum()) for x, y in zip(a, b)]
