"""The premises of the deinterlacer's restatement (tests/deinterlace_ref.py), which the GPU tests compare bit for bit against:
a static clip comes back exactly, a sample reaches four rows and no other column, the half-static noise clip takes every branch,
no intermediate leaves int32, and deinterlacing is worth it on a clip that moves."""
import itertools

import numpy as np
import pytest

from tests import deinterlace_ref as dr
from tests import field_ref


@pytest.mark.parametrize("first", [0, 1])
@pytest.mark.parametrize("rate", ["frame", "field"])
def test_static_clip_comes_back_exactly(first, rate):
    prog = field_ref.moving_planes(3, 8, 40, 23, step=0, wobble=0)
    assert all(np.array_equal(p, prog[0]) for p in prog)
    woven = dr.interlace(prog, first)
    out = dr.deinterlace(woven, "adaptive", first, rate)
    assert len(out) == len(woven) * (2 if rate == "field" else 1)
    for k in list(range(len(out)))[:2] + list(range(len(out)))[-2:]:   # the clip's first and last frame: clamped neighbours
        assert np.array_equal(out[k], prog[0]), k


@pytest.mark.parametrize("which", [0, 1, 2])
def test_reach_is_four_rows_and_the_own_column(which):
    h, w, y0, x0 = 25, 9, 12, 4
    changed = 0
    for first, rate in itertools.product((0, 1), dr.RATES):
        rng = np.random.default_rng(7)   # noise: on a flat clip the temporal clamp rejects a lone sample of P or N altogether
        flat = [rng.integers(0, 200, (h, w)).astype(np.uint8) for _ in range(3)]
        lit = [f.copy() for f in flat]
        lit[which][y0, x0] = 255
        a, b = dr.deinterlace(flat, "adaptive", first, rate), dr.deinterlace(lit, "adaptive", first, rate)
        per = len(a) // 3
        for k in range(per, 2 * per):       # the outputs of the middle frame
            ys, xs = np.nonzero(a[k] != b[k])
            changed += ys.size
            assert set(xs) <= {x0} and all(abs(int(y) - y0) <= 4 for y in ys), (first, rate, k, ys, xs)
    assert changed      # the clamp may reject a lone sample in one setting, not in all four


@pytest.mark.parametrize("bits", [8, 10, 12])
def test_half_static_noise_takes_every_branch(bits):
    stats = {}
    dr.deinterlace(dr.half_static_clip(11, bits), "adaptive", 0, "field", bits, stats)
    share = {k: stats[k] / stats["samples"] for k in ("still", "temporal", "spatial", "clamp")}
    print(bits, {k: round(v, 3) for k, v in share.items()})
    assert all(v >= 0.10 for v in share.values()), share


@pytest.mark.parametrize("bits", [8, 12])
def test_extremes_stay_inside_int32(bits):
    planes = dr.extreme_planes(bits)
    stats = {}
    for trio in itertools.product(planes, repeat=3):
        for first in (0, 1):
            dr.deinterlace(list(trio), "adaptive", first, "field", bits, stats)
            dr.deinterlace(list(trio), "intra", first, "field", bits, stats)
    print(bits, stats["peak"])
    assert stats["peak"] < 2 ** 31
    assert stats["peak"] < 2 ** 26      # the bound the kernel's header states


def test_adaptive_fields_beat_the_woven_frames_by_3_db():
    prog = field_ref.moving_planes(5, 16, 96, 64, step=3, wobble=0)
    woven = dr.interlace(prog, 0)
    assert len(woven) == 8
    fields = dr.deinterlace(woven, "adaptive", 0, "field")
    intra = dr.deinterlace(woven, "intra", 0, "field")
    as_is = np.mean([dr.psnr(woven[t // 2], prog[t]) for t in range(16)])
    adaptive = np.mean([dr.psnr(fields[t], prog[t]) for t in range(16)])
    spatial = np.mean([dr.psnr(intra[t], prog[t]) for t in range(16)])
    print(f"woven {as_is:.2f} dB, adaptive {adaptive:.2f} dB, intra {spatial:.2f} dB")
    assert adaptive >= as_is + 3.0
    assert adaptive > spatial


@pytest.mark.parametrize("h", [2, 3, 4, 5])
def test_small_heights_are_defined(h):
    rng = np.random.default_rng(h)
    frames = [rng.integers(0, 256, (h, 3)).astype(np.uint8) for _ in range(3)]
    for mode, first, rate in itertools.product(dr.MODES, (0, 1), dr.RATES):
        out = dr.deinterlace(frames, mode, first, rate)
        assert all(o.shape == (h, 3) for o in out)
