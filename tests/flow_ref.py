"""numpy restatement of the registration moments (pqa_flow_moments, csrc/flow_moments.hip; include/pqa_vmaf.h) and the seeded
captures of the registration tests.  Not a test module.

With r = ref, d = dis, a = r + d, e = d - r, at every pixel 1 <= x <= W - 2, 1 <= y <= H - 2:

    gx = Sobel-x of a,  gy = Sobel-y of a,  dt = (1 2 1) x (1 2 1) of e
    out[f][j][i][0..5] = sum over the pixels of tile (x // T, y // T) of gx^2, gx gy, gy^2, gx dt, gy dt, dt^2

in int64 (a 64 x 64 tile at 12 bit stays below 2^45); moments_exact is the same in Python ints."""
import numpy as np

from tests import resample_ref as R


def _fields(ref, dis, bits):
    top = (1 << bits) - 1
    r = np.minimum(np.asarray(ref).astype(np.int64), top)
    d = np.minimum(np.asarray(dis).astype(np.int64), top)
    assert r.shape == d.shape and r.ndim == 2 and min(r.shape) >= 3
    a, e = r + d, d - r
    gx = (a[:-2, 2:] + 2 * a[1:-1, 2:] + a[2:, 2:]) - (a[:-2, :-2] + 2 * a[1:-1, :-2] + a[2:, :-2])
    gy = (a[2:, :-2] + 2 * a[2:, 1:-1] + a[2:, 2:]) - (a[:-2, :-2] + 2 * a[:-2, 1:-1] + a[:-2, 2:])
    dt = sum(wj * wi * e[j:j + e.shape[0] - 2, i:i + e.shape[1] - 2] for j, wj in enumerate((1, 2, 1)) for i, wi in enumerate((1, 2, 1)))
    return gx, gy, dt           # [H - 2, W - 2]: entry (y - 1, x - 1) belongs to pixel (x, y)


def moments(ref_frames, dis_frames, tile, bits=8):
    """[n, ty, tx, 6] int64"""
    n = len(ref_frames)
    assert len(dis_frames) == n and tile in (8, 16, 32, 64)
    if n == 0:
        return np.zeros((0, 0, 0, 6), np.int64)
    h, w = np.shape(ref_frames[0])
    ty, tx = -(-h // tile), -(-w // tile)
    out = np.zeros((n, ty, tx, 6), np.int64)
    jj = (np.arange(1, h - 1) // tile)[:, None] * tx + (np.arange(1, w - 1) // tile)[None, :]
    for f in range(n):
        gx, gy, dt = _fields(ref_frames[f], dis_frames[f], bits)
        for m, prod in enumerate((gx * gx, gx * gy, gy * gy, gx * dt, gy * dt, dt * dt)):
            acc = np.zeros(ty * tx, np.int64)
            np.add.at(acc, jj.ravel(), prod.ravel())
            out[f, :, :, m] = acc.reshape(ty, tx)
    return out


def moments_exact(ref, dis, tile, bits=8):
    """one frame pair in Python ints: [ty][tx][6] nested lists (no 64-bit wrap can hide in it)"""
    gx, gy, dt = (v.tolist() for v in _fields(ref, dis, bits))
    h, w = np.shape(ref)
    out = [[[0] * 6 for _ in range(-(-w // tile))] for _ in range(-(-h // tile))]
    for y in range(1, h - 1):
        for x in range(1, w - 1):
            a, b, c = gx[y - 1][x - 1], gy[y - 1][x - 1], dt[y - 1][x - 1]
            o = out[y // tile][x // tile]
            for m, v in enumerate((a * a, a * b, b * b, a * c, b * c, c * c)):
                o[m] += v
    return out


def restatements(bits=8):
    """(moments, resample) as align.register takes them, on the numpy restatements"""
    def mom(r, d, tile):
        return moments(r, d, tile, bits)

    def res(planes, dst_shape, filt, window):
        return [R.resize(np.asarray(p), dst_shape, filt, bits, window) for p in planes]
    return mom, res


def capture(plane, dx, dy, sx, sy, noise=0, seed=0, filt="lanczos", bits=8):
    """`plane` as a capture chain with the map X_dis = n/2 + s (X_ref - n/2) + d would show it: the capture's sample X_dis
    shows the reference's X_ref, so it is the reference read through the INVERSE map's window (a Lanczos warp by default),
    plus uniform noise of +-noise"""
    h, w = plane.shape
    isx, isy = 1.0 / sx, 1.0 / sy
    idx, idy = -dx / sx, -dy / sy
    win = (idx + w * (1 - isx) / 2, idy + h * (1 - isy) / 2, w * isx, h * isy)
    out = R.resize(plane, (h, w), filt, bits, win).astype(np.int64)
    if noise:
        out = out + np.random.default_rng(seed).integers(-noise, noise + 1, out.shape)
    return np.clip(out, 0, (1 << bits) - 1).astype(plane.dtype)


def window_of(dx, dy, sx, sy, w, h):
    """the float window (x0, y0, w, h) of the same-size resample that undoes the map (dx, dy, sx, sy) on a w x h plane"""
    return (dx + w * (1 - sx) / 2, dy + h * (1 - sy) / 2, w * sx, h * sy)
