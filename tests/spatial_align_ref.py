"""Numpy restatement of the shifted-window luma SSE (pqa_shift_sse, csrc/shift_sse.hip) and the seeded clips of the spatial
alignment tests.  Not a test module.

    S[f][j][i] = sum_{y=R}^{H-R-1} sum_{x=R}^{W-R-1} (ref_f[y][x] - dis_f[y + dy][x + dx])^2,  dy = j - R,  dx = i - R

by slicing, in int64 (a 12-bit 2160p frame stays below 2^48).  Reference and capture of the random clips are independent,
so swapped operands give other numbers; sign and transpose are pinned by shifted_pair()."""
import numpy as np


def shift_sse(ref_frames, dis_frames, R: int) -> np.ndarray:
    n = len(ref_frames)
    out = np.zeros((n, 2 * R + 1, 2 * R + 1), np.uint64)
    for f in range(n):
        r, d = np.asarray(ref_frames[f]).astype(np.int64), np.asarray(dis_frames[f]).astype(np.int64)
        h, w = r.shape
        assert w > 2 * R and h > 2 * R and d.shape == r.shape
        win = r[R:h - R, R:w - R]
        for j in range(2 * R + 1):
            for i in range(2 * R + 1):
                e = win - d[j:j + h - 2 * R, i:i + w - 2 * R]
                out[f, j, i] = int((e * e).sum())
    return out


def random_pair(seed: int, n: int, w: int, h: int, bpc: int = 8):
    """n independent random reference and captured frames"""
    rng = np.random.default_rng(seed)
    dt = np.uint8 if bpc == 8 else np.uint16
    ref = [rng.integers(0, 1 << bpc, (h, w)).astype(dt) for _ in range(n)]
    dis = [rng.integers(0, 1 << bpc, (h, w)).astype(dt) for _ in range(n)]
    return ref, dis


def shift_plane(plane: np.ndarray, dx: int, dy: int, rng, top: int) -> np.ndarray:
    """the picture displaced by (dx, dy) -- out[y + dy][x + dx] = plane[y][x] -- with fresh random samples in the border the
    displaced picture does not cover"""
    h, w = plane.shape
    out = rng.integers(0, top + 1, (h, w)).astype(plane.dtype)
    ys, yd = (slice(0, h - dy), slice(dy, h)) if dy >= 0 else (slice(-dy, h), slice(0, h + dy))
    xs, xd = (slice(0, w - dx), slice(dx, w)) if dx >= 0 else (slice(-dx, w), slice(0, w + dx))
    out[yd, xd] = plane[ys, xs]
    return out


def shifted_pair(seed: int, n: int, w: int, h: int, dx: int, dy: int, bpc: int = 8):
    """n random reference frames and the same pictures displaced by (dx, dy)"""
    rng = np.random.default_rng(seed)
    dt = np.uint8 if bpc == 8 else np.uint16
    ref = [rng.integers(0, 1 << bpc, (h, w)).astype(dt) for _ in range(n)]
    dis = [shift_plane(r, dx, dy, rng, (1 << bpc) - 1) for r in ref]
    return ref, dis


def natural_planes(seed: int, n: int, w: int, h: int, hshift: int = 0, vshift: int = 0, mono: bool = True):
    """n frames of smooth moving content with noise (8 bit): [Y] or [Y, U, V] plane lists"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    frames = []
    for t in range(n):
        lum = 128 + 60 * np.sin((xx + 3 * t) / 7.0) * np.cos((yy - 2 * t) / 5.0) + 30 * np.sin((xx * yy) / 97.0 + t)
        lum = np.clip(lum + rng.normal(0, 6, lum.shape), 0, 255).astype(np.uint8)
        planes = [lum]
        if not mono:
            ch, cw = -(-h >> vshift), -(-w >> hshift)
            cy, cx = np.mgrid[0:ch, 0:cw].astype(np.float64)
            for ph in (0.0, 1.3):
                c = 128 + 50 * np.sin((cx + t) / 3.0 + ph) * np.cos((cy + 2 * t) / 4.0 + ph)
                planes.append(np.clip(c + rng.normal(0, 5, c.shape), 0, 255).astype(np.uint8))
        frames.append(planes)
    return frames
