"""adm_need (pqa2_amd/csrc/adm_need.h, through pqa_debug_adm_need): the ranges the ADM march kernels compute anything in
are EXACTLY the hull of a brute-force propagation of libvmaf's windows through the pyramid.

Brute force, per axis (the 2-D sets are products of the two axes: window, box and DWT footprint all are): a boolean mask per
scale starts from the scale's accumulation window (adm_window in oracle/vmaf_oracle.c), is dilated by the 3-wide masking box
with the box's mirror (-1 -> 1, n -> n - 1), and is united with what the mask of the next scale reads through the four-tap
DWT: coefficient j reads positions 2j - 1 .. 2j + 2 of the band above with mirror1's fold (-1 -> 1, n -> n - 1, n + 1 -> n - 2).
The last scale owes no band.  Equality is required (no slack): a range that is too small loses a coefficient the result
needs, one that is too large computes what nobody reads."""
import ctypes as C

import numpy as np
import pytest

from pqa2_amd import _native as N

GEOMETRIES = [(128, 128), (256, 256), (576, 324), (1280, 720), (1920, 1080), (3840, 2160), (1726, 250), (250, 1726)]


def _mirror1(i, n):
    i = -i if i < 0 else i
    i = 2 * n - i - 1 if i >= n else i
    return min(max(i, 0), n - 1)


def _hull(mask):
    idx = np.flatnonzero(mask)
    return (int(idx[0]), int(idx[-1]) + 1)


def brute_axis(n):
    """hulls of the needed positions per scale 0 .. 3, and of the input samples, along an axis of n samples"""
    lens = []
    m = n
    for _ in range(4):
        m = (m + 1) // 2
        lens.append(m)
    masks = [None] * 4
    for s in (3, 2, 1, 0):
        ln = lens[s]
        lo = int(ln * 0.1 - 0.5)
        mask = np.zeros(ln, bool)
        for i in range(lo, ln - lo):            # the window, dilated by the box
            for f in (-1, 0, 1):
                mask[_mirror1(i + f, ln)] = True
        if s < 3:                               # what the next scale's needed coefficients read
            for j in np.flatnonzero(masks[s + 1]):
                for t in range(2 * j - 1, 2 * j + 3):
                    mask[_mirror1(t, ln)] = True
        masks[s] = mask
    inp = np.zeros(n, bool)
    for j in np.flatnonzero(masks[0]):
        for t in range(2 * j - 1, 2 * j + 3):
            inp[_mirror1(t, n)] = True
    return [_hull(mk) for mk in masks], _hull(inp), masks


def need(lib, w, h):
    out = (C.c_int32 * 20)()
    assert lib.pqa_debug_adm_need(w, h, C.byref(out)) == N.PQA_OK
    v = list(out)
    rows = [(v[4 * s], v[4 * s + 1]) for s in range(4)]
    cols = [(v[4 * s + 2], v[4 * s + 3]) for s in range(4)]
    return rows, cols, (v[16], v[17]), (v[18], v[19])


@pytest.fixture(scope="module")
def lib():
    return N.load()


@pytest.mark.parametrize("w,h", GEOMETRIES)
def test_ranges_equal_the_brute_force_hull(lib, w, h):
    rows, cols, in_rows, in_cols = need(lib, w, h)
    brows, bin_rows, rmasks = brute_axis(h)
    bcols, bin_cols, cmasks = brute_axis(w)
    print(f"{w}x{h}: rows {rows} of input {in_rows}; columns {cols} of input {in_cols}")
    assert rows == brows and in_rows == bin_rows
    assert cols == bcols and in_cols == bin_cols
    # the needed sets have no holes: a range describes them completely
    for mk in rmasks + cmasks:
        lo, hi = _hull(mk)
        assert mk[lo:hi].all()


def test_figures_at_2160p(lib):
    rows, cols, in_rows, in_cols = need(lib, 3840, 2160)
    assert rows[1] == (45, 495) and cols[1] == (85, 875)
    assert in_rows == (177, 1983) and in_cols == (337, 3503)


def test_small_frames_keep_whole_bands(lib):
    rows, cols, in_rows, in_cols = need(lib, 256, 256)
    assert rows == cols == [(0, 128), (0, 64), (0, 32), (0, 16)]   # (scale 3: window [1, 15) of 16, dilated by the box)
    assert in_rows == in_cols == (0, 256)


def test_bad_arguments(lib):
    out = (C.c_int32 * 20)()
    assert lib.pqa_debug_adm_need(0, 128, C.byref(out)) == N.PQA_EINVAL
    assert lib.pqa_debug_adm_need(128, 70000, C.byref(out)) == N.PQA_EINVAL
    assert lib.pqa_debug_adm_need(128, 128, None) == N.PQA_EINVAL
