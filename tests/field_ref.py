"""The field moments restated in numpy / Python ints (csrc/field_moments.hip, include/pqa_vmaf.h: pqa_field_moments), and the
clips the field tests are built from.

    E(A, p, B, q) = sum over the row pairs i < H // 2 and the columns of (A[2 i + p][x] - B[2 i + q][x])^2

    out[k-1][2 p + q] = E(D_k, p, R_k, q)    out[k-1][4 + 2 p + q] = E(D_k, p, R_{k-1}, q)    out[k-1][8 + 2 p + q] = E(D_{k-1}, p, R_k, q)
    out[k-1][12] = E(D_k, 0, D_k, 1)         out[k-1][13] = E(R_k, 0, R_k, 1)

A u16 sample above top = 2^bits - 1 is read as top; the last row of an odd-height plane is counted nowhere."""
import numpy as np

SUMS = 14


def _E(A, p, B, q):
    h2 = A.shape[0] // 2
    d = A[p:2 * h2:2] - B[q:2 * h2:2]
    return int((d * d).sum())     # below 2^50: exact in int64


def field_moments(ref, dis, bits=8):
    top = (1 << bits) - 1
    R = [np.minimum(np.asarray(f).astype(np.int64), top) for f in ref]
    D = [np.minimum(np.asarray(f).astype(np.int64), top) for f in dis]
    out = np.zeros((max(len(R) - 1, 0), SUMS), np.uint64)
    for k in range(1, len(R)):
        for p in (0, 1):
            for q in (0, 1):
                out[k - 1, 2 * p + q] = _E(D[k], p, R[k], q)
                out[k - 1, 4 + 2 * p + q] = _E(D[k], p, R[k - 1], q)
                out[k - 1, 8 + 2 * p + q] = _E(D[k - 1], p, R[k], q)
        out[k - 1, 12] = _E(D[k], 0, D[k], 1)
        out[k - 1, 13] = _E(R[k], 0, R[k], 1)
    return out


def random_pairs(seed, n, w, h, bits=8, noise=20):
    """n reference planes of uniform noise and captured planes `noise` around them"""
    rng = np.random.default_rng(seed)
    top = (1 << bits) - 1
    dt = np.uint8 if bits == 8 else np.uint16
    ref = [rng.integers(0, top + 1, (h, w)).astype(dt) for _ in range(n)]
    dis = [np.clip(r.astype(np.int64) + rng.integers(-noise, noise + 1, r.shape), 0, top).astype(dt) for r in ref]
    return ref, dis


# ---- clips -------------------------------------------------------------------------------------------------------------------
def _smooth(a, k=5):
    """k x k box mean of a float plane (valid part)"""
    c = np.cumsum(np.cumsum(np.pad(a, ((1, 0), (1, 0))), axis=0), axis=1)
    return (c[k:, k:] - c[:-k, k:] - c[k:, :-k] + c[:-k, :-k]) / (k * k)


def moving_planes(seed, n, w, h, step=3, wobble=3, dtype=np.uint8):
    """n planes of w x h: smoothed noise that moves `step` pixels a frame, with a vertical wobble of `wobble` lines (every
    other frame is that many lines lower); step = wobble = 0: a static clip"""
    rng = np.random.default_rng(seed)
    base = _smooth(rng.integers(0, 256, (h + wobble + 4, w + step * n + 4)).astype(np.float64))
    base = np.clip((base - 128.0) * 4.0 + 128.0, 0, 255).round().astype(dtype)
    return [base[wobble * (t % 2):wobble * (t % 2) + h, step * t:step * t + w].copy() for t in range(n)]


def moving_clip(seed, n, w=64, h=48, step=3, wobble=3):
    """n frames [Y, U, V] of a 4:2:0 clip whose three planes all move"""
    planes = [moving_planes(seed + p, n, w >> (p > 0), h >> (p > 0), step, wobble) for p in range(3)]
    return [[planes[p][t] for p in range(3)] for t in range(n)]


def with_noise(frames, seed, amp=2):
    """the progressive capture of a clip: every sample moved by at most `amp`"""
    rng = np.random.default_rng(seed)
    return [[np.clip(p.astype(np.int64) + rng.integers(-amp, amp + 1, p.shape), 0, 255).astype(p.dtype) for p in f] for f in frames]


def field_late(frames, parity, first=0):
    """from frame `first` on, the rows of `parity` of every plane come from the previous frame (offset -1); frame 0 keeps its own"""
    out = []
    for t, f in enumerate(frames):
        g = [p.copy() for p in f]
        if t >= max(first, 1):
            for dst, src in zip(g, frames[t - 1]):
                dst[parity::2] = src[parity::2]
        out.append(g)
    return out


def fields_swapped(frames):
    """rows 2 i and 2 i + 1 of every plane change places (even heights)"""
    out = []
    for f in frames:
        g = [p.copy() for p in f]
        for dst, src in zip(g, f):
            dst[0::2], dst[1::2] = src[1::2], src[0::2]
        out.append(g)
    return out


def line_down(frames):
    """the picture one line lower: row y shows row y - 1, row 0 stays"""
    return [[np.concatenate([p[:1], p[:-1]]) for p in f] for f in frames]


def top_doubled(frames):
    """the bottom field dropped and the top field line-doubled: row 2 i + 1 shows row 2 i"""
    out = []
    for f in frames:
        g = [p.copy() for p in f]
        for dst, src in zip(g, f):
            dst[1::2] = src[0::2][:len(dst[1::2])]
        out.append(g)
    return out


def lumas(frames):
    return [f[0] for f in frames]
