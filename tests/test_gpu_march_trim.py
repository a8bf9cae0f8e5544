"""The trimmed march kernels (fused f16 lo pieces in the VIF scale-0 split, DPP-fused taps and the peeled row weight in the
motion march, signed-byte sample conversion in the ADM pyramid) against their partner kernels and the oracle, on the
smallest shapes at which each trim can go wrong and on the content that reaches its corner cases.

Shapes (width x height):
  272 x 272   17 x 17 blocks of 16 x 16: a partial 4-stripe group at VIF scale 0; motion: a fast stripe between two edge
              stripes, three segments of 128 / 128 / 16 rows
  264 x 250   a partial block column and a partial block row; motion: 250 = 128 + 122 rows, the last segment no multiple
              of 4 (its last step keeps the row weight)
  130 x 262   motion: edge stripes only, segments of 128 / 128 / 6 rows
  256 x 264   ADM pyramid (sizes that are multiples of 4, 128 or more): fast and edge stripes, two segments

Bars are the ones of the tests that own the switches (tests/test_gpu_configs.py, tests/test_gpu_parity.py): 2e-6 between the
VIF scale-0 paths, 1e-6 between the march and the tiled ADM / motion kernels, 5e-5 relative for VIF / ADM and 2e-5 for
motion against the oracle."""
import os
import zlib

import numpy as np
import pytest

from pqa2_amd import _native as N
from pqa2_amd import synth

pytestmark = pytest.mark.gpu

REL_TOL = 5e-5          # VIF / ADM num and den against the oracle
VIF_PATHS_REL = 2e-6    # march kernel against the VALU kernel
TILED_REL = 1e-6        # ADM / motion march against the LDS-tiled kernels
MOTION_TOL = 2e-5       # motion against the oracle, relative to max(1, motion)
N_FRAMES = 3
_oracle_cache = {}


def _dtype(bpc):
    return np.uint8 if bpc == 8 else np.uint16


def _run(w, h, bpc, refs, diss, features, prev=None, **env):
    """[n, 17] records; `prev`: the reference luma in front of frame 0 (device-resident submit with a halo frame)"""
    from pqa2_amd.engine import FeatureEngine
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        with FeatureEngine(w, h, bit_depth=bpc, features=features, max_batch=2) as eng:
            if prev is None:
                for i, (r, d) in enumerate(zip(refs, diss)):
                    eng.submit(i, [r], [d])
            else:
                import torch
                es = 1 if bpc == 8 else 2
                view = (lambda a: a) if bpc == 8 else (lambda a: a.view(np.int16))
                R = torch.from_numpy(view(np.stack(refs))).cuda()
                D = torch.from_numpy(view(np.stack(diss))).cuda()
                P = torch.from_numpy(view(np.ascontiguousarray(prev))).cuda()
                torch.cuda.synchronize()
                eng.submit_resident(0, len(refs), [R.data_ptr()], [D.data_ptr()], [w * es], [w * h * es],
                                    prev_ref_luma_ptr=P.data_ptr(), prev_row_pitch=w * es)
            return eng.collect(0, len(refs))[:, :17]
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _oracle(orc, key, refs, diss, bpc, prev=None):
    """the oracle's records of a clip, computed once per clip"""
    if key not in _oracle_cache:
        _oracle_cache[key] = orc.clip_features(refs, diss, bpc, prev_ref=prev)
    return _oracle_cache[key]


def _rel(a, b, floor):
    return float((np.abs(a - b) / np.maximum(np.abs(b), floor)).max())


# ---- VIF scale 0: the split's lo pieces ---------------------------------------------------------------------------------
def _vif_clip(kind, w, h, bpc):
    """(A first version's textured clip was white noise of sigma 20 on a gradient: there the two scale-0 kernels, whose
    decimated planes differ in the last bit, sat 2.1e-5 apart at 272 x 272 -- the VALU kernel 2.2e-5 from the oracle, the march
    kernel 3.3e-6 -- with the split's pieces unfused, that is in the arithmetic of the kernels before the trims: noise at
    every pixel leaves a large share of the few coefficients of the deep scales at the statistic's thresholds.  That measures
    the content, not the split.)"""
    rng = np.random.default_rng(zlib.crc32(repr((kind, w, h, bpc)).encode()))
    peak, dt = (1 << bpc) - 1, _dtype(bpc)
    y, x = np.mgrid[0:h, 0:w]
    refs, diss = [], []
    for i in range(N_FRAMES):
        if kind == "near_black":     # samples 0 .. 3: the first pass's outputs are tiny, their lo pieces f16 denormals
            r, d = rng.integers(0, 4, (h, w)), rng.integers(0, 4, (h, w))
        elif kind == "flat_grey":    # mid-grey: after the mean offset the mean planes are exactly 0
            r, d = np.full((h, w), (peak + 1) // 2), np.full((h, w), (peak + 1) // 2 + i)
        elif kind == "checker":      # 0 / peak: the largest values every plane of the split sees
            r = ((x + y + i) & 1) * peak
            d = peak - r
        else:                        # textured: the project's synthetic clip (band-limited texture on sinusoids against a
            #                          blurred, block-quantised, noisy copy), the content of the test that owns the 2e-6 bar
            (r,), (d,) = synth.make_pair(w, h, i, bpc, chroma=False)
        refs.append(np.asarray(r).astype(dt))
        diss.append(np.asarray(d).astype(dt))
    return refs, diss


@pytest.mark.parametrize("bpc", [8, 10, 12])
@pytest.mark.parametrize("kind", ["near_black", "flat_grey", "textured", "checker"])
@pytest.mark.parametrize("w,h", [(272, 272), (264, 250)])
def test_split_march_kernel_matches_valu_kernel_and_oracle(oracle32, w, h, kind, bpc):
    refs, diss = _vif_clip(kind, w, h, bpc)
    march = _run(w, h, bpc, refs, diss, N.FEAT_VIF)[:, :8]
    valu = _run(w, h, bpc, refs, diss, N.FEAT_VIF, PQA_VIF_MFMA="0")[:, :8]
    exp = _oracle(oracle32, ("vif", kind, w, h, bpc), refs, diss, bpc)[:, :8]
    paths, orc = _rel(march, valu, 1e-30), _rel(march, exp, 1e-12)
    print(f"\n{w}x{h} {bpc}-bit {kind}: march vs VALU {paths:.3e}, march vs oracle {orc:.3e}, VALU vs oracle {_rel(valu, exp, 1e-12):.3e}; "
          f"march vs VALU per record slot {(np.abs(march - valu) / np.maximum(np.abs(valu), 1e-30)).max(axis=0).tolist()}")
    assert np.all(np.isfinite(march))
    if kind != "flat_grey":   # (on flat frames every sum is exact on both paths: equal bits are what they should give)
        assert not np.array_equal(march.view(np.uint64), valu.view(np.uint64)), "PQA_VIF_MFMA=0 did not change the path"
    assert paths < VIF_PATHS_REL
    assert orc < REL_TOL


# ---- motion: DPP-fused taps, peeled row weight ---------------------------------------------------------------------------
def _motion_clip(kind, w, h, bpc):
    rng = np.random.default_rng(zlib.crc32(repr((kind, w, h, bpc)).encode()))
    peak, dt = (1 << bpc) - 1, _dtype(bpc)
    first = rng.integers(0, peak + 1, (h, w)).astype(dt)
    if kind == "noise":
        refs = [first] + [rng.integers(0, peak + 1, (h, w)).astype(dt) for _ in range(N_FRAMES - 1)]
    else:   # "last_rows": frame 1 differs from frame 0 in the last row of segment 0 only, frame 2 from frame 1 in the
        #     image's last row only: what the blur spreads over five rows meets the first and last steps of a segment
        second = first.copy()
        second[127] = peak - second[127]
        third = second.copy()
        third[h - 1] = peak - third[h - 1]
        refs = [first, second, third]
    prev = rng.integers(0, peak + 1, (h, w)).astype(dt)
    return refs, prev


@pytest.mark.parametrize("bpc", [8, 10])
@pytest.mark.parametrize("kind", ["noise", "last_rows"])
@pytest.mark.parametrize("w,h", [(272, 272), (264, 250), (130, 262)])
def test_motion_march_matches_tiled_kernel_and_oracle(oracle32, w, h, kind, bpc):
    refs, prev = _motion_clip(kind, w, h, bpc)
    # (motion reads the reference only; the distorted clip is the reference)
    for halo in (None, "other", "same"):
        p = None if halo is None else (prev if halo == "other" else refs[0])
        march = _run(w, h, bpc, refs, refs, N.FEAT_MOTION, prev=p)[:, 16]
        tiled = _run(w, h, bpc, refs, refs, N.FEAT_MOTION, prev=p, PQA_MOTION_MARCH="0")[:, 16]
        exp = _oracle(oracle32, ("motion", kind, w, h, bpc, halo), refs, refs, bpc, prev=p)[:, 16]
        paths = _rel(march, tiled, 1e-30)
        orc = float((np.abs(march - exp) / np.maximum(1.0, np.abs(exp))).max())
        print(f"\n{w}x{h} {bpc}-bit {kind}, halo {halo}: motion {march.tolist()}; march vs tiled {paths:.3e}, vs oracle {orc:.3e}")
        if kind == "noise":   # (a clip that moves in one row only may well sum to the same bits on both paths)
            assert not np.array_equal(march[1:].view(np.uint64), tiled[1:].view(np.uint64)), "PQA_MOTION_MARCH=0 did not change the path"
        assert paths < TILED_REL
        assert orc < MOTION_TOL
        if halo != "other":
            assert march[0] == 0.0 and tiled[0] == 0.0     # no frame in front, or the same frame: motion 0, exactly
        else:
            assert march[0] > 0.0
        assert np.all(march[1:] > 0.0)


# ---- ADM pyramid: signed-byte conversion --------------------------------------------------------------------------------
def _adm_clip(kind, w, h):
    rng = np.random.default_rng(7 if kind == "ramp" else 11)
    y, x = np.mgrid[0:h, 0:w]
    refs, diss = [], []
    for i in range(N_FRAMES):
        r = ((x + 3 * y + 5 * i) % 256).astype(np.uint8)
        d = ((x + 3 * y + 5 * i + (7 * x + 13 * y) % 5) % 256).astype(np.uint8)
        if kind == "shuffled":   # the same values, every row group of four columns somewhere else
            r = rng.permutation(r.reshape(-1)).reshape(h, w)
            d = np.clip(r.astype(np.int16) + rng.integers(-9, 10, (h, w)), 0, 255).astype(np.uint8)
            d.reshape(-1)[:256] = rng.permutation(256)
        for p in (r, d):   # every byte value, in every lane position of the four-sample loads
            assert all(np.unique(p[:, k::4]).size == 256 for k in range(4))
        refs.append(r)
        diss.append(d)
    return refs, diss


@pytest.mark.parametrize("kind", ["ramp", "shuffled"])
def test_adm_pyramid_signed_bytes_match_tiled_kernel_and_oracle(oracle32, kind):
    w, h = 256, 264
    refs, diss = _adm_clip(kind, w, h)
    march = _run(w, h, 8, refs, diss, N.FEAT_ADM)[:, 8:16]
    tiled = _run(w, h, 8, refs, diss, N.FEAT_ADM, PQA_ADM_MARCH="0")[:, 8:16]
    single = _run(w, h, 8, refs, diss, N.FEAT_ADM, PQA_ADM_PYRAMID="0")[:, 8:16]
    exp = _oracle(oracle32, ("adm", kind), refs, diss, 8)[:, 8:16]
    paths, orc = _rel(march, tiled, 1e-30), _rel(march, exp, 1e-12)
    print(f"\n{w}x{h} {kind}: pyramid vs tiled {paths:.3e}, vs one scale per launch {_rel(march, single, 1e-30):.3e}, vs oracle {orc:.3e}")
    assert not np.array_equal(march.view(np.uint64), tiled.view(np.uint64)), "PQA_ADM_MARCH=0 did not change the path"
    assert paths < TILED_REL
    assert _rel(march, single, 1e-30) < TILED_REL
    assert orc < REL_TOL
