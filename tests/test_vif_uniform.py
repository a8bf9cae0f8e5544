"""CPU premises of tests/test_gpu_vif_uniform.py: the clips really hold waves of every kind, so that the bit-equality of
the all-high fast path with the general statistic is checked on waves that take it, on all-low and mixed waves that must not,
and on the edges between them."""
import numpy as np
import pytest

from tests import vif_uniform_ref as U

CASES = [(w, h, bpc) for (w, h) in U.SIZES for bpc in (8, 10, 12)]


@pytest.mark.parametrize("w,h,bpc", CASES)
def test_clip_holds_every_kind_of_wave(w, h, bpc):
    c0, c1 = U.census(w, h, bpc)
    print(f"{w}x{h} {bpc}-bit  scale 0 blocks {c0}  scale 1 waves {c1}")
    for kind in ("high", "low", "mixed"):
        assert c0[kind] >= 8, (kind, c0)      # 16 x 16 blocks of the march kernel, float64 with the margin 4 / 1 around 2
        assert c1[kind] >= 1, (kind, c1)      # waves of the scale-1 tiles


@pytest.mark.parametrize("w,h,bpc", CASES)
def test_straddle_frame_straddles_pixel_by_pixel(w, h, bpc):
    refs, _ = U.clip(w, h, bpc)
    s1 = U.sigma1_sq(refs[U.KINDS.index("straddle")], bpc, 0)
    both = [(b < 2.0).any() and (b >= 2.0).any()
            for y in range(0, h - 15, 16) for x in range(0, w - 15, 16) for b in [s1[y:y + 16, x:x + 16]]]
    print(f"{w}x{h} {bpc}-bit  blocks with both sides of sigma_nsq: {sum(both)} of {len(both)}")
    assert sum(both) >= len(both) // 2


def test_sizes_leave_partial_waves():
    """272 x 272 is whole blocks only; 264 x 250 ends in a partial stripe and a partial block row, and its scale-1 plane in a
    partial tile row: the waves that must NOT take a fast path on the strength of their inside pixels."""
    (w0, h0), (w1, h1) = U.SIZES
    assert w0 % 16 == 0 and h0 % 16 == 0 and h0 // 16 > 16
    assert w1 % 16 and h1 % 16 and (h1 // 2) % 8 and (w1 // 2) % 4 == 0 and U.SEAM % 16


def test_dis_is_flat_under_texture_once():
    refs, diss = U.clip(*U.SIZES[0], 8)
    k = U.KINDS.index("dis_flat")
    assert np.ptp(diss[k]) == 0 and np.ptp(refs[k]) > 200
