"""The premises of the packed RGB conversion without a GPU: the named matrices (pqa2_amd/rgb.py), the int32 bound, and the numpy
restatement tests/rgb_ref.py held against published code values and against the existing restatement of pqa_format_convert."""
import itertools

import numpy as np
import pytest

from pqa2_amd import rgb
from pqa2_amd.align import COLOUR_STANDARDS
from tests import format_convert_ref as FR
from tests import rgb_ref as R

ALL = list(itertools.product(sorted(COLOUR_STANDARDS), (8, 10), (True, False), (8, 10), (True, False)))
BARS = [(1, 1, 1), (1, 1, 0), (0, 1, 1), (0, 1, 0), (1, 0, 1), (1, 0, 0), (0, 0, 1), (0, 0, 0)]   # White Yellow Cyan Green Magenta Red Blue Black


def _float_matrix(std, sb, rgb_full, db, yuv_full):
    """a second derivation, in floats, through the normalised signals: code -> E'RGB -> E'Y, E'Cb, E'Cr -> code"""
    kr, kb = (float(v) for v in COLOUR_STANDARDS[std])
    kg = 1.0 - kr - kb
    lo, hi = (0.0, 2.0 ** sb - 1) if rgb_full else (16.0 * 2 ** (sb - 8), 235.0 * 2 ** (sb - 8))
    out = []
    for c in range(3):
        def code(r, g, b):
            er, eg, eb = ((v - lo) / (hi - lo) for v in (r, g, b))
            ey = kr * er + kg * eg + kb * eb
            e = (ey, (eb - ey) / (2 * (1 - kb)), (er - ey) / (2 * (1 - kr)))[c]
            if yuv_full:
                return e * (2.0 ** db - 1) + (0.0 if c == 0 else 2.0 ** (db - 1))
            return (219.0 * e + 16.0 if c == 0 else 224.0 * e + 128.0) * 2 ** (db - 8)
        off = code(0, 0, 0)
        out += [off, code(1, 0, 0) - off, code(0, 1, 0) - off, code(0, 0, 1) - off]
    return [v * 16384 for v in out]


@pytest.mark.parametrize("std,sb,rgb_full,db,yuv_full", ALL)
def test_conversion_matrix_against_a_float_derivation(std, sb, rgb_full, db, yuv_full):
    m = rgb.conversion_matrix(std, sb, rgb_full, db, yuv_full)
    assert len(m) == 12 and all(isinstance(v, int) for v in m)
    for got, want in zip(m, _float_matrix(std, sb, rgb_full, db, yuv_full)):
        assert abs(got - want) <= 1 + 1e-6, (got, want)
    assert sum(m[5:8]) == 0 and sum(m[9:12]) == 0            # greys stay exactly neutral


def test_the_pinned_bt709_matrix():
    assert rgb.conversion_matrix("bt709", 8, True, 8, False) == [262144, 2991, 10064, 1016, 2097152, -1649, -5547, 7196, 2097152, 7196, -6536, -660]
    with pytest.raises(ValueError):
        rgb.conversion_matrix("bt470", 8, True, 8, False)
    assert "bt2020" in COLOUR_STANDARDS
    assert (rgb.default_matrix(480), rgb.default_matrix(576), rgb.default_matrix(577), rgb.default_matrix(1080)) == ("bt601", "bt601", "bt709", "bt709")


def _bars(fmt, m, dst_bits, on, off):
    r, g, b = (np.array([[on if bar[k] else off for bar in BARS]]) for k in range(3))
    y, u, v = R.convert(R.pack(fmt, r, g, b), fmt, 8, 1, m, (0, 0, 0, 0, dst_bits))
    return [(int(y[0, i]), int(u[0, i]), int(v[0, i])) for i in range(8)]


BARS8 = [(235, 128, 128), (219, 16, 138), (188, 154, 16), (173, 42, 26), (78, 214, 230), (63, 102, 240), (32, 240, 118), (16, 128, 128)]
BARS10 = [(940, 512, 512), (877, 64, 553), (754, 615, 64), (691, 167, 105), (313, 857, 919), (250, 409, 960), (127, 960, 471), (64, 512, 512)]


def test_colour_bars_give_the_published_code_values():
    for fmt in ("bgra", "argb", "rgba", "abgr"):
        assert _bars(fmt, rgb.conversion_matrix("bt709", 8, True, 8, False), 8, 255, 0) == BARS8
    assert _bars("r210", rgb.conversion_matrix("bt709", 10, False, 10, False), 10, 940, 64) == BARS10
    assert _bars("r210", rgb.conversion_matrix("bt709", 10, False, 8, False), 8, 940, 64) == BARS8
    assert _bars("bgra", rgb.conversion_matrix("bt601", 8, True, 8, False), 8, 255, 0)[5] == (81, 90, 240)


@pytest.mark.parametrize("w,h", [(13, 11), (1, 1), (2, 5), (16, 3)])
def test_selection_matrix_equals_the_existing_restatement(w, h):
    """m[c] = 2^14 on one component, offset 0: convert() is format_convert_ref.convert of that component's plane"""
    rng = np.random.default_rng(w * 7 + h)
    for fmt in ("abgr", "r210"):
        bits = R.BIT_DEPTH[fmt]
        planes = rng.integers(0, 1 << bits, (3, h, w))
        packed = R.pack(fmt, *planes, seed=3)
        m = [0] * 12
        m[1] = m[4 + 2] = m[8 + 3] = 1 << 14
        for hs, vs, hsite, vsite in itertools.product((0, 1), (0, 1), (0, 1), (0, 1)):
            got = R.convert(packed, fmt, w, h, m, (hs, vs, hsite, vsite, bits))
            dt = np.uint8 if bits == 8 else np.uint16
            assert np.array_equal(got[0], planes[0].astype(dt))
            for c in (1, 2):
                want = FR.convert(planes[c].astype(dt), (h, w), (0, 0, 0, 0, bits), (hs, vs, hsite, vsite, bits))
                assert got[c].dtype == want.dtype and np.array_equal(got[c], want), (fmt, hs, vs, hsite, vsite, c)


def test_pack_and_unpack_agree():
    rng = np.random.default_rng(1)
    for fmt in R.FORMATS:
        bits = R.BIT_DEPTH[fmt]
        planes = rng.integers(0, 1 << bits, (3, 5, 70))
        for ones in (False, True):
            packed = R.pack(fmt, *planes, stride=R.file_stride(fmt, 70), seed=2, ones=ones)
            assert packed.shape == (5, rgb.file_stride(fmt, 70)) and rgb.row_bytes(fmt, 70) == 280
            for got, mine, want in zip(R.unpack(packed, fmt, 70), rgb.unpack_rgb(fmt, packed, 70), planes):
                assert np.array_equal(got, want) and np.array_equal(mine, want)
    assert rgb.file_stride("r210", 70) == 512 and rgb.file_stride("r210", 64) == 256 and rgb.file_stride("bgra", 70) == 280
    with pytest.raises(ValueError):
        rgb.row_bytes("rgb24", 70)


@pytest.mark.parametrize("std,sb,rgb_full,db,yuv_full", ALL)
def test_matrix_fits(std, sb, rgb_full, db, yuv_full):
    m = rgb.conversion_matrix(std, sb, rgb_full, db, yuv_full)
    for hs, vs in itertools.product((0, 1), (0, 1)):
        assert rgb.matrix_fits(m, sb, hs, vs)
    if db == 10:   # (2^10 - 1) 2^14 is 2^24: times 4 and the tap sum 64 it is 2^32
        assert not rgb.matrix_fits([4 * v for v in m], sb, 1, 1)
    # the bound is the one the restatement asserts: at the cube's corners, with all 64 weights on them
    corners = np.array(list(itertools.product((0, (1 << sb) - 1), repeat=3)))
    a = np.array(m).reshape(3, 4)
    ext = np.abs(a[:, :1] + a[:, 1:] @ corners.T).max()
    assert ext * 64 + (1 << 19) < 1 << 31
