"""Packed RGB captures (bgra, argb, rgba, abgr, r210): file geometry, a numpy unpack and the named R'G'B' -> Y'CbCr matrices in
the Q14 integers pqa_rgb_convert takes (include/pqa_vmaf.h has the formats and the definition; csrc/rgb_convert.hip the kernel).
Everything here is exact: the matrices are derived in Fractions and rounded once."""
from __future__ import annotations

from fractions import Fraction

import numpy as np

from . import _native as N
from .align import COLOUR_STANDARDS

Q = 14
FORMATS = {"bgra": N.SURFACE_BGRA, "argb": N.SURFACE_ARGB, "rgba": N.SURFACE_RGBA, "abgr": N.SURFACE_ABGR, "r210": N.SURFACE_R210}
BIT_DEPTH = {"bgra": 8, "argb": 8, "rgba": 8, "abgr": 8, "r210": 10}
BYTE_ORDER = {"bgra": (2, 1, 0), "argb": (1, 2, 3), "rgba": (0, 1, 2), "abgr": (3, 2, 1)}   # the byte of R, G, B in a pixel
RANGES = ("full", "limited")


def _name(fmt) -> str:
    if fmt not in FORMATS:
        raise ValueError(f"unknown packed RGB format {fmt!r} (one of {', '.join(FORMATS)})")
    return fmt


def row_bytes(fmt: str, width: int) -> int:
    """the bytes of a row that hold pixels"""
    _name(fmt)
    return 4 * int(width)


def file_stride(fmt: str, width: int) -> int:
    """rows of a headerless file: r210 pads to 64 pixels (256 bytes), the 8-bit formats do not pad"""
    return (int(width) + 63) // 64 * 256 if _name(fmt) == "r210" else 4 * int(width)


def unpack_rgb(fmt: str, rows: np.ndarray, width: int):
    """(R, G, B) of packed rows (2-D uint8, at least row_bytes() a row): uint8, r210: uint16 values 0 ... 1023"""
    _name(fmt)
    rows = np.asarray(rows, np.uint8)
    px = rows[:, :4 * int(width)].reshape(rows.shape[0], int(width), 4)
    if fmt == "r210":
        word = (px[..., 0].astype(np.uint32) << 24) | (px[..., 1].astype(np.uint32) << 16) | (px[..., 2].astype(np.uint32) << 8) | px[..., 3]
        return tuple(((word >> s) & 0x3FF).astype(np.uint16) for s in (20, 10, 0))
    return tuple(np.ascontiguousarray(px[..., k]) for k in BYTE_ORDER[fmt])


def default_matrix(height: int) -> str:
    """what an untagged capture is taken for: BT.601 up to 576 lines, BT.709 above ("bt2020" only on request)"""
    return "bt601" if int(height) <= 576 else "bt709"


def default_range(fmt: str) -> str:
    """what the cards deliver: full-range R'G'B' in the 8-bit formats, limited (64 ... 940) in r210"""
    return "limited" if _name(fmt) == "r210" else "full"


def conversion_matrix(standard: str, src_bits: int, rgb_full: bool, dst_bits: int, yuv_full: bool):
    """int[12], rows (offset, gains of R, G, B) of Y', Cb, Cr in Q14, every entry rounded to nearest once:
    Y' = Kr R + Kg G + Kb B, Cb = (B - Y') / (2 (1 - Kb)), Cr = (R - Y') / (2 (1 - Kr)) on R'G'B' normalised from
    [0, 2^sb - 1] (full) or [16, 235] 2^(sb-8) (limited), to Y 16 + 219, C 128 +- 112 times 2^(db-8) (limited) or Y 0 ... 2^db - 1,
    C 2^(db-1) +- (2^db - 1) / 2 (full).  A chroma row whose rounded gains do not sum to zero gets its gain of largest magnitude
    adjusted so that they do: greys stay exactly neutral."""
    if standard not in COLOUR_STANDARDS:
        raise ValueError(f"unknown colour standard {standard!r} (one of {', '.join(COLOUR_STANDARDS)})")
    sb, db = int(src_bits), int(dst_bits)
    kr, kb = COLOUR_STANDARDS[standard]
    kg = 1 - kr - kb
    e = [[kr, kg, kb],
         [-kr / (2 * (1 - kb)), -kg / (2 * (1 - kb)), Fraction(1, 2)],
         [Fraction(1, 2), -kg / (2 * (1 - kr)), -kb / (2 * (1 - kr))]]
    lo, hi = (Fraction(0), Fraction((1 << sb) - 1)) if rgb_full else (Fraction(16 << (sb - 8)), Fraction(235 << (sb - 8)))
    if yuv_full:
        base, span = [Fraction(0), Fraction(1 << (db - 1)), Fraction(1 << (db - 1))], [Fraction((1 << db) - 1)] * 3
    else:
        f = 1 << (db - 8)
        base, span = [Fraction(16 * f), Fraction(128 * f), Fraction(128 * f)], [Fraction(219 * f), Fraction(224 * f), Fraction(224 * f)]
    half, out = Fraction(1, 2), []
    for c in range(3):
        gains = [span[c] * e[c][j] / (hi - lo) for j in range(3)]
        row = [((base[c] - sum(gains) * lo) * (1 << Q) + half).__floor__()] + [(g * (1 << Q) + half).__floor__() for g in gains]
        if c and sum(row[1:]):
            k = max((1, 2, 3), key=lambda j: abs(row[j]))
            row[k] -= sum(row[1:])
        out += row
    return out


def matrix_fits(m, src_bits: int, hshift: int, vshift: int) -> bool:
    """the bound of pqa_rgb_convert: for every row, the extreme of |A| over the source cube times the tap sum Sx Sy (8 an axis of
    shift 1), plus the rounding half, stays below 2^31 -- what makes int32 legal in the kernel"""
    top, s = (1 << int(src_bits)) - 1, 1 << (3 * (int(hshift) + int(vshift)))
    for c in range(3):
        row = [int(v) for v in m[4 * c:4 * c + 4]]
        hi = row[0] + sum(max(v, 0) for v in row[1:]) * top
        lo = row[0] + sum(min(v, 0) for v in row[1:]) * top
        if max(abs(hi), abs(lo)) * s + (s << (Q - 1)) >= 1 << 31:
            return False
    return True
