"""The ADM march kernels compute the approximation band only inside the dependency cone of the deeper scales' windows
(pqa2_amd/csrc/adm_need.h).  That removes work and keeps every surviving operation in its place, so the ADM slots of a
record must be bit-identical to those of the whole-band run (PQA_ADM_CONE=0, read once at pqa_create), nothing outside the
cone may be read, and the usual bars against the oracle and the LDS-tiled kernel hold unchanged.

Shapes (width x height; the pyramid kernel takes sizes that are multiples of 4 and >= 128, in segments of 32 scale-1 rows
and stripes of 60 scale-1 columns):
  256 x 256    the cone is the whole band
  256 x 576    scale-1 rows clamp inside a segment, nothing vanishes
  256 x 1728   scale-1 needed rows start at 33: pyramid segment 0 vanishes
  2880 x 256   scale-1 needed columns start at 61: stripe 0 and the last stripe vanish (the EDGE instances)
  250 x 1726   not a multiple of 4: the one-scale march at all four scales, regions 0 and 2 shortened"""
import ctypes as C
import os

import numpy as np
import pytest

from pqa2_amd import _native as N

pytestmark = pytest.mark.gpu

REL_TOL = 5e-5   # tests/test_gpu_configs.py: f32 kernels against the f32 restatement
SHAPES = [(256, 256), (256, 576), (256, 1728), (2880, 256), (250, 1726)]
ADM = slice(8, 16)
_clips = {}


def clip(w, h, bpc, seed=0, n=2):
    """n frame pairs of seeded noise on a gradient (made once per shape and depth, never modified)"""
    key = (w, h, bpc, seed, n)
    if key not in _clips:
        rng = np.random.default_rng(1000 * seed + w + 7 * h + bpc)
        peak = (1 << bpc) - 1
        y, x = np.mgrid[0:h, 0:w]
        out = []
        for i in range(n):
            base = 0.15 + 0.6 * ((x + 2 * y + 13 * i) % (w + h)) / (w + h)
            ref = base + 0.08 * rng.standard_normal((h, w))
            dis = ref + 0.04 * rng.standard_normal((h, w)) + 0.02 * np.sin(x / 9.0)
            dt = np.uint8 if bpc == 8 else np.uint16
            out.append((np.clip(ref * peak + 0.5, 0, peak).astype(dt), np.clip(dis * peak + 0.5, 0, peak).astype(dt)))
        for r, d in out:
            r.setflags(write=False)
            d.setflags(write=False)
        _clips[key] = out
    return _clips[key]


def bright_clip(w, h, bpc, n=2):
    """checkerboard of black and peak white against its inverse: approximation bands far from any natural content's"""
    peak = (1 << bpc) - 1
    y, x = np.mgrid[0:h, 0:w]
    dt = np.uint8 if bpc == 8 else np.uint16
    a = ((((x // 3) + (y // 5)) & 1) * peak).astype(dt)
    return [(a, (peak - a).astype(dt))] * n


def score(w, h, bpc, clips, **env):
    """ADM record slots of the frames of `clips` (a list of clips scored one after the other on ONE context)"""
    from pqa2_amd.engine import FeatureEngine
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        with FeatureEngine(w, h, bit_depth=bpc, features=N.FEAT_ADM, max_batch=2) as eng:
            got, at = [], 0
            for frames in clips:
                for i, (r, d) in enumerate(frames):
                    eng.submit(at + i, [r], [d])
                got.append(eng.collect(at, len(frames))[:, ADM].copy())
                at += len(frames)
            return got
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def need(w, h):
    out = (C.c_int32 * 20)()
    assert N.load().pqa_debug_adm_need(w, h, C.byref(out)) == N.PQA_OK
    v = list(out)
    return [(v[4 * s], v[4 * s + 1]) for s in range(4)], [(v[4 * s + 2], v[4 * s + 3]) for s in range(4)]


def test_each_shape_is_the_case_it_stands_for():
    seg, stripe = 32, 60   # adm_pyramid.hip: scale-1 rows per segment, scale-1 columns per stripe
    rows, cols = need(256, 256)
    assert rows == cols == [(0, 128), (0, 64), (0, 32), (0, 16)]
    rows, cols = need(256, 576)
    lo, hi = rows[1]
    assert 0 < lo < seg and 144 - hi > 0 and (144 - 1) // seg == (hi - 1) // seg   # clamps inside the first and the last segment
    assert cols[1] == (0, 64)
    rows, cols = need(256, 1728)
    assert rows[1][0] == 33 and rows[1][0] >= seg                 # segment 0 holds no needed row
    assert (rows[1][1] - 1) // seg < (432 - 1) // seg             # nor does the last one
    rows, cols = need(2880, 256)
    assert cols[1][0] == 61 and cols[1][0] >= stripe              # stripe 0 holds no needed column
    assert (cols[1][1] - 1) // stripe < (720 - 1) // stripe       # nor does the last one
    assert rows[1] == (0, 64)
    rows, cols = need(250, 1726)
    assert 250 % 4 and all(rows[s][0] > 0 and rows[s][1] < n for s, n in zip(range(3), (863, 432, 216)))


@pytest.mark.parametrize("bpc", [8, 10])
@pytest.mark.parametrize("w,h", SHAPES)
def test_cone_is_bit_identical_to_whole_bands(w, h, bpc):
    frames = clip(w, h, bpc)
    cone, = score(w, h, bpc, [frames])
    whole, = score(w, h, bpc, [frames], PQA_ADM_CONE="0")
    assert np.all(np.isfinite(cone)) and np.all(cone[:, 4:] > 0)
    assert np.array_equal(cone.view(np.uint64), whole.view(np.uint64)), (np.abs(cone - whole) / np.abs(whole)).max()


@pytest.mark.parametrize("w,h", [(256, 1728), (2880, 256), (250, 1726)])
def test_nothing_outside_the_cone_is_read(w, h):
    """The bands a bright clip left behind lie exactly where the cone says nobody looks: the test clip scored after it on
    the same context equals the test clip on a fresh context."""
    frames = clip(w, h, 8)
    fresh, = score(w, h, 8, [frames])
    _, after = score(w, h, 8, [bright_clip(w, h, 8), frames])
    assert np.array_equal(after.view(np.uint64), fresh.view(np.uint64))


def test_oracle_parity(oracle32):
    w, h = 256, 1728
    frames = clip(w, h, 8)
    got, = score(w, h, 8, [frames])
    exp = oracle32.clip_features([r for r, _ in frames], [d for _, d in frames], 8)[:, ADM]
    rel = np.abs(got - exp) / np.abs(exp)
    print("max rel", rel.max())
    assert rel.max() < REL_TOL, rel.max()


def test_tiled_partner():
    w, h = 256, 1728
    frames = clip(w, h, 8)
    cone, = score(w, h, 8, [frames])
    tiled, = score(w, h, 8, [frames], PQA_ADM_MARCH="0")
    assert not np.array_equal(cone.view(np.uint64), tiled.view(np.uint64)), "PQA_ADM_MARCH=0 did not change the path"
    rel = np.abs(cone - tiled) / np.maximum(np.abs(tiled), 1e-30)
    assert rel.max() < 1e-6, rel.max()
