"""numpy restatement of the packed RGB -> Y'CbCr conversion (include/pqa_vmaf.h, pqa_rgb_convert; kernel: csrc/rgb_convert.hip).
Integer arithmetic only, int64.  A destination layout is (hshift, vshift, hsite, vsite, bits) as FeatureEngine.rgb_convert takes it;
m is 12 integers, rows (offset, R, G, B) in Q14.  The taps are format_convert_ref's, from a 4:4:4 plane."""
import numpy as np

from tests import format_convert_ref as FR

BYTE_ORDER = {"bgra": (2, 1, 0, 3), "argb": (1, 2, 3, 0), "rgba": (0, 1, 2, 3), "abgr": (3, 2, 1, 0)}   # the byte of R, G, B, A
BIT_DEPTH = {"bgra": 8, "argb": 8, "rgba": 8, "abgr": 8, "r210": 10}
FORMATS = tuple(BIT_DEPTH)


def file_stride(fmt: str, w: int) -> int:
    return (w + 63) // 64 * 256 if fmt == "r210" else 4 * w


def pack(fmt, r, g, b, stride=None, seed=0, ones=False) -> np.ndarray:
    """[h, stride] uint8: the packed rows of the planes r, g, b.  The A bytes / r210's bits 31-30 are random, or all ones with
    `ones`; the bytes of a row behind 4 * w are random."""
    r, g, b = (np.asarray(p).astype(np.uint32) for p in (r, g, b))
    h, w = r.shape
    stride = 4 * w if stride is None else int(stride)
    rng = np.random.default_rng(seed)
    out = rng.integers(0, 256, (h, stride), dtype=np.uint8)
    px = out[:, :4 * w].reshape(h, w, 4)
    if fmt == "r210":
        top = np.full((h, w), 3, np.uint32) if ones else rng.integers(0, 4, (h, w)).astype(np.uint32)
        word = (top << 30) | (r << 20) | (g << 10) | b
        for k in range(4):   # big-endian
            px[..., k] = (word >> (24 - 8 * k)) & 0xFF
    else:
        ro, go, bo, ao = BYTE_ORDER[fmt]
        px[..., ro], px[..., go], px[..., bo] = r, g, b
        px[..., ao] = 255 if ones else rng.integers(0, 256, (h, w))
    return out


def unpack(packed, fmt, w):
    """(R, G, B) int64 of packed rows"""
    px = np.asarray(packed)[:, :4 * w].reshape(-1, w, 4).astype(np.int64)
    if fmt == "r210":
        word = (px[..., 0] << 24) | (px[..., 1] << 16) | (px[..., 2] << 8) | px[..., 3]
        return (word >> 20) & 1023, (word >> 10) & 1023, word & 1023
    ro, go, bo, _ = BYTE_ORDER[fmt]
    return px[..., ro], px[..., go], px[..., bo]


def axis(luma: int, shift: int, site: int):
    """(tap matrix from a 4:4:4 plane, its weight sum): shift 0 is the identity with S = 1"""
    if shift == 0:
        return np.eye(luma, dtype=np.int64), 1
    return FR.axis_matrix(luma, 0, shift, 0, site), FR.weight_sum(0, shift)


def _rows(mat, plane):
    """mat @ plane in int64, row by row over the few columns a row of a tap matrix uses (numpy has no fast int64 matmul)"""
    out = np.empty((mat.shape[0], plane.shape[1]), np.int64)
    for i in range(mat.shape[0]):
        nz = np.flatnonzero(mat[i])
        out[i] = mat[i, nz] @ plane[nz]
    return out


def convert(packed, fmt, w, h, m, dst, luma_only=False):
    """[Y, U, V] (or [Y]) of one packed frame: section 2 of the definition, matrix first, then the taps, one rounding"""
    hs, vs, hsite, vsite, bits = (int(v) for v in dst)
    m = np.asarray([int(v) for v in m], np.int64).reshape(3, 4)
    r, g, b = unpack(np.asarray(packed)[:h], fmt, w)
    a = [m[c, 0] + m[c, 1] * r + m[c, 2] * g + m[c, 3] * b for c in range(3)]
    top, dt = (1 << bits) - 1, np.uint8 if bits <= 8 else np.uint16
    out = [np.clip((a[0] + (1 << 13)) >> 14, 0, top).astype(dt)]
    if luma_only:
        return out
    mx, sx = axis(w, hs, hsite)
    my, sy = axis(h, vs, vsite)
    t = 14 + (sx * sy).bit_length() - 1
    for c in (1, 2):
        acc = _rows(mx, _rows(my, a[c]).T).T   # My A Mx^T
        assert np.abs(acc).max() + (1 << (t - 1)) < 1 << 31   # the bound of the ABI: int32 is enough
        out.append(np.clip((acc + (1 << (t - 1))) >> t, 0, top).astype(dt))
    return out
