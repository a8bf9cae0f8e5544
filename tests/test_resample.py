"""The resampler's host side without a GPU: the coefficient tables the library builds (pqa_debug_resample_table) against the
numpy restatement (tests/resample_ref.py), their invariants and the tap limit, and the restatement's own properties --
constant, identity, whole-sample windows, and what the integer arithmetic costs against the same filter in float64."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import resample_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILTERS = ("bilinear", "bicubic", "lanczos")


@pytest.fixture(scope="module")
def lib():
    from pqa2_amd import _native as N
    if not os.path.exists(N.LIB_PATH):
        N.build()
    return N.load()


def lib_table(lib, filt, n_src, n_dst, x0_q16=0, ext_q16=None, cap=32):
    """(rc, first [n_dst], coeff [n_dst, cap], taps) of the library"""
    ext_q16 = n_src * R.Q16 if ext_q16 is None else ext_q16
    first = np.full(n_dst, -1, np.int32)
    coeff = np.full((n_dst, cap), 77, np.int16)
    taps = C.c_int32(-1)
    rc = lib.pqa_debug_resample_table(R.FILTERS[filt], n_src, n_dst, x0_q16, ext_q16, first.ctypes.data, coeff.ctypes.data, cap,
                                      C.byref(taps))
    return rc, first, coeff, taps.value


# (n_dst, n_src, x0): up- and downscales by whole and broken ratios, and two sub-sample shifts
CASES = [(1920, 1280, 0.0), (64, 47, 0.0), (48, 64, 0.0), (480, 1920, 0.0), (100, 399, 0.0), (64, 64, 0.25), (64, 64, -0.5)]


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("n_dst,n_src,x0", CASES)
def test_table_matches_the_restatement(lib, filt, n_dst, n_src, x0):
    rc, first, coeff, taps = lib_table(lib, filt, n_src, n_dst, R.q16(x0))
    assert rc == 0 and 1 <= taps <= 32
    assert not coeff[:, taps:].any()
    assert (first >= 0).all() and (first + taps <= n_src + 32).all()
    got = R.dense(first, coeff, n_src)           # asserts that no coefficient lies past the source
    want = R.table(filt, n_src, n_dst, R.q16(x0))
    assert (got.sum(axis=1) == 16384).all() and (want.sum(axis=1) == 16384).all()
    assert np.abs(got - want).max() <= 2
    assert (got != want).any(axis=1).sum() <= n_dst // 100      # a last-bit libm difference at a quantisation tie, no more
    assert np.abs(got).sum(axis=1).max() < 32768
    for i in range(n_dst):                                     # rows are cut to their non-zero span
        nz = np.flatnonzero(got[i])
        assert first[i] == nz[0] and nz[-1] - nz[0] < taps


@pytest.mark.parametrize("filt", FILTERS)
def test_identity_and_whole_sample_windows_are_single_taps(lib, filt):
    for x0 in (0, 3, -2, 70):
        rc, first, coeff, taps = lib_table(lib, filt, 64, 64, x0 * R.Q16)
        assert rc == 0 and taps == 1
        assert (coeff[:, 0] == 16384).all() and np.array_equal(first, np.clip(np.arange(64) + x0, 0, 63))
        assert np.array_equal(R.dense(first, coeff, 64), R.table(filt, 64, 64, x0 * R.Q16))


def test_tap_limit_and_argument_rules(lib):
    from pqa2_amd import _native as N
    assert lib_table(lib, "lanczos", 600, 100)[0] == N.PQA_EINVAL          # 6x down: 36 taps
    assert lib_table(lib, "lanczos", 530, 100)[0] == 0 and lib_table(lib, "lanczos", 530, 100)[3] <= 32
    assert lib_table(lib, "bicubic", 800, 100)[0] == 0 and lib_table(lib, "bicubic", 800, 100)[3] == 32
    assert lib_table(lib, "bicubic", 900, 100)[0] == N.PQA_EINVAL
    assert lib_table(lib, "bilinear", 8192, 1)[0] == N.PQA_EINVAL
    rc, _, coeff, taps = lib_table(lib, "bicubic", 128, 64, cap=4)         # a short coefficient array: refused, *taps is set
    assert rc == N.PQA_EINVAL and taps == 8 and (coeff == 77).all()
    first, co, t = np.zeros(4, np.int32), np.zeros((4, 32), np.int16), C.c_int32()
    for args in ((3, 4, 4, 0, 4 * R.Q16), (0, 0, 4, 0, 4 * R.Q16), (0, 4, 0, 0, 4 * R.Q16), (0, 4, 4, 0, 0), (0, 4, 4, 0, -5),
                 (0, 8193, 4, 0, 4 * R.Q16)):
        assert lib.pqa_debug_resample_table(*args, first.ctypes.data, co.ctypes.data, 32, C.byref(t)) == N.PQA_EINVAL
    assert lib.pqa_debug_resample_table(0, 4, 4, 0, 4 * R.Q16, None, co.ctypes.data, 32, C.byref(t)) == N.PQA_EINVAL
    assert lib.pqa_debug_resample_table(0, 4, 4, 0, 4 * R.Q16, first.ctypes.data, co.ctypes.data, 32, None) == N.PQA_EINVAL


def test_magnitude_bound_over_the_ratios(lib):
    """sum |q| of a row stays below 32768 -- what keeps the intermediate in int16 -- from 8x up to 4x down"""
    worst = {}
    for filt in ("bicubic", "lanczos"):
        for n_dst in (512, 400, 171, 128, 100, 64, 37, 25, 16):
            rc, first, coeff, _ = lib_table(lib, filt, 64, n_dst)
            assert rc == 0
            worst[filt] = max(worst.get(filt, 0), int(np.abs(coeff.astype(np.int64)).sum(axis=1).max()))
    print("largest sum |q|:", worst)
    assert max(worst.values()) < 32768


# ---- the restatement itself --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("b", [8, 10, 12])
def test_constant_identity_and_whole_sample_window(filt, b):
    top = (1 << b) - 1
    for v in (0, 1, top // 2, top):
        flat = np.full((9, 11), v, np.uint16)
        for shape in ((9, 11), (20, 31), (4, 5)):
            assert (R.resize(flat, shape, filt, b) == v).all()
        assert (R.resize(flat, (9, 11), filt, b, window=(0.3, -0.7, 11, 9)) == v).all()
    src = R.noise(b, 23, 17, b)
    assert np.array_equal(R.resize(src, src.shape, filt, b), src)
    for x0, y0 in ((3, 2), (-4, 1), (0, -3), (30, 30)):
        assert np.array_equal(R.resize(src, src.shape, filt, b, window=(x0, y0, 23, 17)), R.replicated_crop(src, x0, y0))


def test_integer_round_trip_against_float64():
    """Luma of the 352 x 288 golden clip, bicubic, down by 2 then up by 2, PSNR against the original: the integer path (int14
    coefficients, the intermediate rounded to 14 - 8 = 6 fractional bits) against the same two tables unquantised in float64
    with one rounding per resize.  Measured: float64 37.6384 dB, integer 37.6357 dB, a gap of 0.0027 dB; the two results
    differ in 0.80 % of the samples, by one level.  The bound is on the arithmetic, not on the filter: what the filter
    loses is in both figures."""
    from pqa2_amd.yuvio import open_video
    src = np.asarray(open_video(os.path.join(ROOT, "tests", "golden", "clips", "c352x288_8_ref.y4m")).frame(0)[0])
    h, w = src.shape
    got, ref = [], []
    for quantise, fn, out in ((True, R.apply, got), (False, R.apply_float, ref)):
        down = [R.table("bicubic", n, n // 2, quantise=quantise) for n in (w, h)]
        up = [R.table("bicubic", n // 2, n, quantise=quantise) for n in (w, h)]
        small = fn(src, down[0], down[1], 8)
        assert small.shape == (h // 2, w // 2)
        out.append(fn(small, up[0], up[1], 8))
    p_int, p_float = R.psnr(got[0], src), R.psnr(ref[0], src)
    diff = np.abs(got[0].astype(int) - ref[0].astype(int))
    print(f"round trip: float64 {p_float:.4f} dB, integer {p_int:.4f} dB, gap {p_float - p_int:.4f} dB, "
          f"{(diff != 0).mean() * 100:.2f} % of samples differ, max {diff.max()}")
    assert 20.0 < p_float < 60.0
    assert abs(p_float - p_int) <= 0.05
