"""numpy restatement of the packed capture formats (include/pqa_vmaf.h, PQA_SURFACE_UYVY / _YUYV / _V210), written from the
format description, not from the kernel (pqa2_amd/csrc/unpack.hip) or the library's own reader (pqa2_amd/yuvio.py).

cw = ceil(w / 2): the chroma planes of these 4:2:2 formats are cw x h.
  uyvy422  macropixel k of a row = the bytes U_k, Y_2k, V_k, Y_2k+1; minimum row 4 * cw bytes
  yuyv422  the same with the bytes Y_2k, U_k, Y_2k+1, V_k
  v210     groups of 6 pixels in four little-endian 32-bit words, 10-bit components at bits 0, 10, 20:
           w0 = U0 Y0 V0, w1 = Y1 U1 Y2, w2 = V1 Y3 U2, w3 = Y4 V2 Y5; minimum row 16 * ceil(w / 6) bytes; files pad rows to
           ((w + 47) / 48) * 128 bytes
pack_* fill everything the format leaves undefined -- row padding, the unused last Y of an odd width, the components beyond
w / cw in the last v210 group, bits 30-31 of every v210 word -- from `fill` (a byte pattern generator), never with zeros, so
that a decoder that lets them through is caught."""
import numpy as np

FORMATS = ("uyvy422", "yuyv422", "v210")
BIT_DEPTH = {"uyvy422": 8, "yuyv422": 8, "v210": 10}
DTYPE = {"uyvy422": np.uint8, "yuyv422": np.uint8, "v210": np.uint16}


def chroma_width(w):
    return (w + 1) // 2


def min_row_bytes(fmt, w):
    return 16 * ((w + 5) // 6) if fmt == "v210" else 4 * chroma_width(w)


def file_stride(fmt, w):
    return ((w + 47) // 48) * 128 if fmt == "v210" else min_row_bytes(fmt, w)


def _junk(shape, seed):
    """a deterministic non-zero byte pattern"""
    n = int(np.prod(shape))
    return ((np.arange(n, dtype=np.uint32) * 37 + 101 + seed * 13) % 255 + 1).astype(np.uint8).reshape(shape)


# where the components of a v210 group sit: (word, bit) of Y0..Y5, U0..U2, V0..V2
_V210_Y = ((0, 10), (1, 0), (1, 20), (2, 10), (3, 0), (3, 20))
_V210_U = ((0, 0), (1, 10), (2, 20))
_V210_V = ((0, 20), (2, 0), (3, 10))


def pack(fmt, y, u, v, stride=None, seed=0, ones=True):
    """(h, stride) uint8: the planes y (h x w), u, v (h x cw) as packed rows `stride` bytes apart (default: the minimum).
    ones: v210's bits 30-31 are set (False: taken from the junk pattern)."""
    y, u, v = (np.asarray(a) for a in (y, u, v))
    h, w = y.shape
    cw = chroma_width(w)
    assert u.shape == (h, cw) and v.shape == (h, cw), (y.shape, u.shape, v.shape)
    row = min_row_bytes(fmt, w)
    stride = row if stride is None else stride
    assert stride >= row
    out = _junk((h, stride), seed)
    if fmt in ("uyvy422", "yuyv422"):
        yo, uo = (1, 0) if fmt == "uyvy422" else (0, 1)
        m = out[:, :4 * cw].reshape(h, cw, 4)
        m[:, :, uo] = u
        m[:, :, uo + 2] = v
        m[:, :, yo] = y[:, 0::2]
        m[:, :w // 2, yo + 2] = y[:, 1::2]       # an odd width leaves the last macropixel's second Y as junk
        return out
    assert fmt == "v210"
    g = (w + 5) // 6
    junk16 = (_junk((h, 6 * g), seed + 1).astype(np.uint32) * 4 + 3) & 1023
    yy, uu, vv = junk16.copy(), junk16[:, :3 * g].copy(), junk16[:, 3 * g:].copy()
    yy[:, :w], uu[:, :cw], vv[:, :cw] = y, u, v
    words = np.zeros((h, g, 4), np.uint32)
    for comp, where in ((yy.reshape(h, g, 6), _V210_Y), (uu.reshape(h, g, 3), _V210_U), (vv.reshape(h, g, 3), _V210_V)):
        for i, (wd, bit) in enumerate(where):
            words[:, :, wd] |= (comp[:, :, i].astype(np.uint32) & 1023) << bit
    top = np.uint32(3) if ones else (_junk((h, g, 4), seed + 2).astype(np.uint32) & 3)
    words |= top << 30
    out[:, :16 * g] = words.reshape(h, 4 * g).astype("<u4").view(np.uint8).reshape(h, 16 * g)
    return out


def unpack(fmt, packed, w):
    """(y, u, v) of the packed rows `packed` ((h, stride) uint8) of a w-wide frame"""
    packed = np.asarray(packed)
    h = packed.shape[0]
    cw = chroma_width(w)
    if fmt in ("uyvy422", "yuyv422"):
        yo, uo = (1, 0) if fmt == "uyvy422" else (0, 1)
        m = packed[:, :4 * cw].reshape(h, cw, 4)
        y = np.empty((h, 2 * cw), np.uint8)
        y[:, 0::2], y[:, 1::2] = m[:, :, yo], m[:, :, yo + 2]
        return y[:, :w].copy(), m[:, :, uo].copy(), m[:, :, uo + 2].copy()
    assert fmt == "v210"
    g = (w + 5) // 6
    words = np.ascontiguousarray(packed[:, :16 * g]).view("<u4").reshape(h, g, 4).astype(np.uint32)
    pick = lambda where: np.stack([(words[:, :, wd] >> bit) & 1023 for wd, bit in where], axis=2).reshape(h, -1).astype(np.uint16)
    return pick(_V210_Y)[:, :w].copy(), pick(_V210_U)[:, :cw].copy(), pick(_V210_V)[:, :cw].copy()


def random_planes(fmt, w, h, seed, extremes=True):
    """planes of uniform noise in the format's range; the first samples of every plane are the extremes 0 and max"""
    rng = np.random.default_rng(seed)
    top = (1 << BIT_DEPTH[fmt]) - 1
    cw = chroma_width(w)
    planes = [rng.integers(0, top + 1, (h, n), dtype=np.uint16).astype(DTYPE[fmt]) for n in (w, cw, cw)]
    if extremes:
        for p in planes:
            p[0, 0], p[-1, -1] = 0, top
            p[0, -1], p[-1, 0] = top, 0
    return planes
