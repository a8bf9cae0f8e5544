"""Parity at the frame-size limits: planes 16384 samples long, 16 to 128 samples across (tests/long_planes_ref.py; premises
pinned on the CPU by tests/test_long_planes_ref.py).

pqa_create takes 16 ... 16384 samples each way.  A 16384 x 16 frame costs what 512 x 512 costs and holds the largest stripe,
segment and partial-slot counts and the largest column / row offsets the kernels form; the sample extremes sit in its last 16
columns / rows.  Three frames at max_batch = 2: a partial batch and a motion carry.

  1. float features against the f64 oracle at REL_TOL (the f32 oracle is within 1e-5 of f64 on these sizes, so the rule
     max(REL_TOL, 4 x rel32) leaves the bar where it is), motion at MOTION_ATOL + 5e-6 x value; then under every kernel
     switch, with the agreement bounds of the tests that own the switch: 2e-6 between the VIF scale-0 paths
     (test_gpu_configs.py), 1e-6 between the ADM / motion march and tiled kernels and with / without the ADM pyramid
     (test_gpu_configs.py), bit-equality between the VIF strip and tiled kernels (test_gpu_vif_strip.py), with / without the
     ADM cone (test_gpu_adm_cone.py) and with / without the VIF fast paths (test_gpu_vif_uniform.py); the integer VIF border;
  2. the fixed-point kernels, bit-equal to IntOracle;
  3. the FFmpeg PSNR / SSIM kernels on three 4:2:0 planes: SSE exact, SSIM 1e-9;
  4. far-end localisation: a whole-frame sum dilutes one wrong stripe of 1024, so the patch frames of
     tests/localized_ref.py at 16384 x 48 and 48 x 16384, first two placements, the two at coordinate 8192, the two at the far end, at
     test_gpu_localized.py's bar;
  5. the extension features, each against the restatement and at the tolerance of its own test file.
"""
import functools

import numpy as np
import pytest

from tests import localized_ref as L
from tests import long_planes_ref as LP
from tests.test_gpu_localized import CONFIGS as LOCALIZED_CONFIGS
from tests.test_gpu_localized import _check_against_oracle, _check_premises
from tests.test_gpu_vif_strip import _switches          # None = the library's default, whatever the caller's environment says

pytestmark = pytest.mark.gpu

VIF_PATHS_REL = 2e-6      # test_vif_mfma_path_matches_valu_path_and_oracle
MARCH_TILED_REL = 1e-6    # test_adm_and_motion_march_kernels_match_the_tiled_kernels_and_the_oracle

DEFAULTS = {k: None for k in ("PQA_VIF_MFMA", "PQA_ADM_MARCH", "PQA_MOTION_MARCH", "PQA_ADM_PYRAMID", "PQA_VIF_STRIP",
                              "PQA_VIF_STRIP_SEG", "PQA_ADM_CONE", "PQA_VIF_UNIFORM")}


def _id(s):
    return f"{s[0]}x{s[1]}_{s[2]}bit"


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _run(size, env=None, **kw):
    """[N_FRAMES, 17] records of the size's clip; env: kernel switches, read at pqa_create."""
    from pqa2_amd.engine import FeatureEngine
    w, h, bpc = size
    refs, diss = LP.clip(w, h, bpc)
    with _switches(dict(DEFAULTS, **(env or {}))):
        eng = FeatureEngine(w, h, bit_depth=bpc, max_batch=LP.MAX_BATCH, **kw)
    with eng:
        for i in range(LP.N_FRAMES):
            eng.submit(i, [refs[i]], [diss[i]])
        return np.ascontiguousarray(eng.collect(0, LP.N_FRAMES)[:, :LP.N_FEAT])


@functools.lru_cache(maxsize=None)
def _default(size):
    got = _run(size)
    got.setflags(write=False)
    return got


def _check_oracle(got, want, label):
    """The float bar; prints the worst distance per feature."""
    assert np.all(np.isfinite(got)), label
    rel = LP.rel_features(got, want)
    worst = rel.max(axis=0)
    d_motion = np.abs(got[:, 16] - want[:, 16])
    print(f"\n{label}: worst |gpu - f64| / |f64| per feature (bar {LP.REL_TOL:.0e}); motion |d| {d_motion.max():.2e} "
          f"(values {want[:, 16].round(4).tolist()})")
    for name, r in zip(LP.FEATURES, worst):
        print(f"  {name:11s} {r:.2e}")
    assert rel.max() < LP.REL_TOL, (label, LP.FEATURES[int(worst.argmax())], float(rel.max()))
    assert np.all(d_motion < LP.MOTION_ATOL + 5e-6 * want[:, 16]), (label, got[:, 16], want[:, 16])
    assert got[0, 16] == 0.0


def _rel(a, b):
    return float((np.abs(a - b) / np.maximum(np.abs(b), 1e-30)).max())


# ---- 1. float features ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", LP.SIZES, ids=_id)
def test_float_features_against_the_oracle(oracle64, size):
    _check_oracle(_default(size), LP.oracle_features(oracle64, *size), _id(size))


@pytest.mark.parametrize("size", LP.SIZES, ids=_id)
def test_integer_vif_border(oracle64, size):
    from pqa2_amd import _native as N
    want = LP.oracle_features(oracle64, *size, vif_border101=True)
    plain = LP.oracle_features(oracle64, *size)
    assert np.abs(want[:, :8] - plain[:, :8]).max() > 0 and np.array_equal(want[:, 8:], plain[:, 8:])
    _check_oracle(_run(size, vif_border=N.VIF_BORDER_INTEGER), want, f"{_id(size)} / integer border")


@pytest.mark.parametrize("size", LP.SIZES, ids=_id)
def test_vif_scale0_valu_path(oracle64, size):
    march, valu = _default(size), _run(size, {"PQA_VIF_MFMA": "0"})
    assert not np.array_equal(_bits(march[:, :8]), _bits(valu[:, :8])), "PQA_VIF_MFMA=0 did not change the path"
    assert np.array_equal(_bits(march[:, 8:]), _bits(valu[:, 8:]))
    print(f"\n{_id(size)}: march against VALU {_rel(march[:, :8], valu[:, :8]):.2e}")
    assert _rel(march[:, :8], valu[:, :8]) < VIF_PATHS_REL
    _check_oracle(valu, LP.oracle_features(oracle64, *size), f"{_id(size)} / PQA_VIF_MFMA=0")


@pytest.mark.parametrize("size", LP.SIZES, ids=_id)
def test_adm_and_motion_tiled_kernels(oracle64, size):
    march, tiled = _default(size), _run(size, {"PQA_ADM_MARCH": "0", "PQA_MOTION_MARCH": "0"})
    assert not np.array_equal(_bits(march[:, 8:16]), _bits(tiled[:, 8:16])), "PQA_ADM_MARCH=0 did not change the path"
    assert not np.array_equal(_bits(march[1:, 16]), _bits(tiled[1:, 16])), "PQA_MOTION_MARCH=0 did not change the path"
    assert np.array_equal(_bits(march[:, :8]), _bits(tiled[:, :8]))
    print(f"\n{_id(size)}: march against tiled, ADM {_rel(march[:, 8:16], tiled[:, 8:16]):.2e} "
          f"motion {_rel(march[1:, 16], tiled[1:, 16]):.2e}")
    assert _rel(march[:, 8:16], tiled[:, 8:16]) < MARCH_TILED_REL and _rel(march[1:, 16], tiled[1:, 16]) < MARCH_TILED_REL
    _check_oracle(tiled, LP.oracle_features(oracle64, *size), f"{_id(size)} / PQA_ADM_MARCH=0 PQA_MOTION_MARCH=0")


@pytest.mark.parametrize("size", LP.SIZES, ids=_id)
def test_adm_one_scale_per_launch(oracle64, size):
    auto, single = _default(size), _run(size, {"PQA_ADM_PYRAMID": "0"})
    print(f"\n{_id(size)}: pyramid against one scale per launch {_rel(auto[:, 8:16], single[:, 8:16]):.2e}")
    assert _rel(auto[:, 8:16], single[:, 8:16]) < MARCH_TILED_REL
    if size in LP.PYRAMID:         # scales 0 and 1 come from another kernel (measured 8e-11 and 2e-10 apart): the switch works
        assert not np.array_equal(_bits(auto[:, 8:16]), _bits(single[:, 8:16])), "PQA_ADM_PYRAMID=0 did not change the path"
    else:                          # the pyramid kernel does not take the frame: the very same launches either way
        assert np.array_equal(_bits(auto), _bits(single))
    assert np.array_equal(_bits(auto[:, :8]), _bits(single[:, :8])) and np.array_equal(_bits(auto[:, 16]), _bits(single[:, 16]))
    _check_oracle(single, LP.oracle_features(oracle64, *size), f"{_id(size)} / PQA_ADM_PYRAMID=0")


@pytest.mark.parametrize("size", LP.SIZES, ids=_id)
def test_vif_strip_kernel_equals_the_tiled_kernel(oracle64, size):
    tiled = _run(size, {"PQA_VIF_STRIP": "0"})
    strip = _run(size, {"PQA_VIF_STRIP": "14", "PQA_VIF_STRIP_SEG": "3"})     # every scale marches, three tile rows a segment
    assert np.array_equal(_bits(strip), _bits(tiled)), (strip - tiled)
    _check_oracle(strip, LP.oracle_features(oracle64, *size), f"{_id(size)} / PQA_VIF_STRIP_SEG=3")


@pytest.mark.parametrize("size", LP.SIZES, ids=_id)
@pytest.mark.parametrize("switch", ["PQA_ADM_CONE", "PQA_VIF_UNIFORM"])
def test_cone_and_uniform_switches_change_no_bit(size, switch):
    off = _run(size, {switch: "0"})
    assert np.array_equal(_bits(off), _bits(_default(size))), (switch, off - _default(size))


# ---- 2. fixed point --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", LP.SMALL + [(16384, 128, 8)], ids=_id)
def test_fixed_point_is_bit_exact(size):
    from pqa2_amd import _native as N
    want = LP.int_oracle_features(*size)
    got = _run(size, fixed_point=N.FIXED_ALL)
    bad = np.argwhere(_bits(got) != _bits(want))
    assert bad.size == 0, [(int(i), LP.FEATURES[f], got[i, f], want[i, f]) for i, f in bad[:6]]


# ---- 3. FFmpeg PSNR / SSIM --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(16384, 16), (16, 16384)])
def test_psnr_ssim_three_planes(oracle32, w, h):
    from pqa2_amd import _native as N
    from pqa2_amd import synth
    from pqa2_amd.engine import FeatureEngine, sse_from_records
    n = 2
    refs, diss = synth.make_clip(w, h, n, 8, chroma=True)
    for p in range(3):     # the extremes at the far end of every plane: the largest block sums
        LP.far_end(refs[0][p], 8, 16)[...] = 0
        LP.far_end(diss[0][p], 8, 16)[...] = 255
        LP.far_end(refs[1][p], 8, 16)[...] = 255
        LP.far_end(diss[1][p], 8, 16)[...] = 255
    with FeatureEngine(w, h, n_planes=3, features=N.FEAT_PSNR | N.FEAT_SSIM, max_batch=LP.MAX_BATCH) as eng:
        for i in range(n):
            eng.submit(i, refs[i], diss[i])
        rec = eng.collect(0, n)
    sse = sse_from_records(rec)
    for i in range(n):
        for p in range(3):
            assert int(sse[i, p]) == oracle32.sse_plane(diss[i][p], refs[i][p], 8), (i, p)
            exp = oracle32.ssim_plane(diss[i][p], refs[i][p], 8)
            assert abs(rec[i, 17 + p] - exp) < 1e-9, (i, p, rec[i, 17 + p], exp)


# ---- 4. far-end localisation ------------------------------------------------------------------------------------------------
LONG = 16384
ACROSS = 48                                  # the patch (32) and 8 samples on either side
_ALONG = [0, L.STEP, LONG // 2 - L.PATCH, LONG // 2 - L.PATCH // 2, LONG - L.PATCH - 1, LONG - L.PATCH]
# first two; the patch that ends at coordinate 8192 (its filters reach across) and the one that lies across it; at the far end
# the patch one sample short of the last row / column and the one flush with it, as localized_ref.corner_places has them (one
# STEP short of it, at 48 x 16384, the f32 oracle itself is 2.0e-5 from f64: at L.REL32_MAX, no premise to build on)
LOCALIZED = {
    "wide": (LONG, ACROSS, [(x, (ACROSS - L.PATCH) // 2) for x in _ALONG]),
    "tall": (ACROSS, LONG, [((ACROSS - L.PATCH) // 2, y) for y in _ALONG]),
}
_EXPECTED = {}


def _expected(oracle64, oracle32, name):
    if name not in _EXPECTED:
        w, h, places = LOCALIZED[name]
        e = L.Expected(oracle64, oracle32, w, h, places, None, 8)      # axis None: every placement gets its own oracle runs
        for a in (e.exp64, e.exp32, e.bar, e.norm, e.rel32):
            a.setflags(write=False)
        _EXPECTED[name] = e
    return _EXPECTED[name]


@pytest.mark.parametrize("config", ["default", "fallbacks"])
@pytest.mark.parametrize("name", list(LOCALIZED))
def test_patch_at_the_far_end(oracle32, oracle64, name, config):
    from pqa2_amd.engine import FeatureEngine
    w, h, places = LOCALIZED[name]
    assert all(0 <= x <= w - L.PATCH and 0 <= y <= h - L.PATCH for x, y in places)
    e = _expected(oracle64, oracle32, name)
    _check_premises(e)      # the f32 oracle within L.REL32_MAX of f64 on every placement: the bar means what it says
    refs, diss = L.placement_clip(w, h, places, 8)
    with _switches(dict(DEFAULTS, **LOCALIZED_CONFIGS[config])):
        eng = FeatureEngine(w, h, max_batch=7)
    with eng:
        for i in range(len(refs)):
            eng.submit(i, [refs[i]], [diss[i]])
        got = eng.collect(0, len(refs))[:, :L.N_FEAT].reshape(len(places), 2, L.N_FEAT)
    _check_against_oracle(e, got, f"{w}x{h} / {config}")


# ---- 5. extension features --------------------------------------------------------------------------------------------------
EXT_SIZES = [(16384, 16), (16, 16384)]


def _ext_cases(depths):
    return [(w, h, bpc) for (w, h) in EXT_SIZES for bpc in depths]


def test_which_extension_feature_accepts_which_long_size():
    """pqa_create at 16384 x 16 and 16 x 16384, three 4:2:0 planes, 8 and 10 bit:

        float_ssim   accepted (decimation 1: a 16374 x 6 / 6 x 16374 map)
        ciede        accepted
        psnr_hvs     accepted (chroma 8192 x 8 / 8 x 8192: one block row / column)
        xpsnr        accepted (16 x 16384 is one column of 24 x 24 blocks: the filter's weight smoothing leaves WSSE 0, +inf dB)
        siti         accepted
        integrity    accepted
        cambi        accepted
        delta_itp    accepted (an entry of any context; it has no feature bit)
        float_ms_ssim  refused, PQA_EINVAL naming it: its fifth scale is 1024 x 1 and needs 11 x 11

    Each accepted feature is held against its restatement below; this test pins the list."""
    from pqa2_amd import _native as N
    from pqa2_amd.engine import FeatureEngine
    accepted = {"float_ssim": N.FEAT_FLOAT_SSIM, "ciede": N.FEAT_CIEDE, "psnr_hvs": N.FEAT_PSNR_HVS, "xpsnr": N.FEAT_XPSNR,
                "siti": N.FEAT_SITI, "integrity": N.FEAT_INTEGRITY, "cambi": N.FEAT_CAMBI, "delta_itp": N.FEAT_PSNR}
    for (w, h, bpc) in _ext_cases((8, 10)):
        for name, bit in accepted.items():
            with FeatureEngine(w, h, bit_depth=bpc, n_planes=3, features=bit, max_batch=2) as eng:
                assert eng._ctx.value, (name, w, h, bpc)
        with pytest.raises(N.PqaError) as e:
            FeatureEngine(w, h, bit_depth=bpc, n_planes=3, features=N.FEAT_MS_SSIM, max_batch=2)
        assert e.value.code == N.PQA_EINVAL and "float_ms_ssim" in str(e.value)


@pytest.mark.parametrize("w,h,bpc", _ext_cases((8, 10)))
def test_float_ssim(w, h, bpc):
    from pqa2_amd import _native as N
    from tests import ssim_family_ref as R
    from tests.test_gpu_ssim_family import TOL, _clip, _engine_ext
    refs, diss = _clip(w, h, 1, bpc, seed=w + bpc)
    _, ext = _engine_ext(w, h, bpc, refs, diss, features=N.FEAT_FLOAT_SSIM)
    want = R.ext_record(refs[0], diss[0], bpc, want_ms_ssim=False)
    d = np.abs(ext[0, :4] - want[:4])
    print(f"\n{w}x{h} {bpc}-bit: float_ssim {ext[0, 0]:.6f}, worst |d| {d.max():.2e} (bar {TOL})")
    assert np.all(np.isfinite(ext[0, :4])) and d.max() <= TOL
    assert np.isnan(ext[0, 4:]).all()


@pytest.mark.parametrize("w,h,bpc", _ext_cases((8, 10)))
def test_ciede(w, h, bpc):
    from tests import ciede_ref as R
    from tests.test_gpu_ciede import MEAN_REL, SCORE_ABS, _planes, _run
    ref, dis = _planes(w, h, bpc, 1, 1, seed=w + bpc)
    _, ext = _run(w, h, bpc, 1, 1, [ref], [dis])
    score, mean = R.frame_slots(ref, dis, bpc, 1, 1)
    print(f"\n{w}x{h} {bpc}-bit: mean dE {mean:.6f}, rel {abs(ext[0, 21] - mean) / mean:.2e}, score |d| {abs(ext[0, 20] - score):.2e}")
    assert abs(ext[0, 21] - mean) / mean <= MEAN_REL
    assert abs(ext[0, 20] - score) <= SCORE_ABS


@pytest.mark.parametrize("w,h,bpc", _ext_cases((8, 10)))
def test_psnr_hvs(w, h, bpc):
    from tests.test_gpu_psnr_hvs import _check, _frames, _run
    refs, diss = _frames(w, h, bpc, 1, 1, 1, seed=w + bpc)
    _, _, ext2 = _run(w, h, bpc, 1, 1, refs, diss)
    _check(ext2[0], refs[0], diss[0], bpc, (w, h, bpc))


@pytest.mark.parametrize("w,h,bpc", _ext_cases((8, 10)))
@pytest.mark.parametrize("hfr", [False, True])
def test_xpsnr(w, h, bpc, hfr):
    from tests import xpsnr_ref as R
    from tests.test_gpu_xpsnr import DB_ABS, _frames, _run
    refs, diss = _frames(w, h, bpc, 1, 1, 3, seed=11)       # frame 2 has both predecessors
    ext3 = _run(w, h, bpc, 1, 1, refs, diss, hfr=hfr, max_batch=2)[3]
    wsse, db = R.clip(refs, diss, bpc, hfr)
    assert np.array_equal(ext3[:, 3:6], wsse)
    # 16 x 16384 is one column of 24 x 24 blocks, and the filter's in-line weight smoothing (frames up to 640 x 480 pixels)
    # then takes every weight down to 0: WSSE 0 and +inf dB on both sides.  16384 x 16 has finite values.
    assert (wsse == 0).all() == (w == 16) and np.array_equal(np.isinf(ext3[:, :3]), np.isinf(db))
    fin = np.isfinite(db)
    assert np.abs(ext3[:, :3][fin] - np.asarray(db)[fin]).max(initial=0.0) < DB_ABS
    # what the weights are made of, which the zero weights of 16 x 16384 hide: the exact sums of every luma block (squared
    # error, spatial and temporal activity) of frame 2 through the kernel's debug entry
    from tests.test_gpu_xpsnr import _hook
    o, m1, m2, r = refs[2][0], refs[1][0], refs[0][0], diss[2][0]
    got, _ = _hook(o, m1, m2, r, bpc, hfr)
    want = np.array([[b["sse"], b["sa"], b["ta"]] for b in R.blocks(o, m1, m2, r, hfr)], np.uint64)
    assert len(want) == -(-w // 24) * -(-h // 24) and (want[:, 0] > 0).all() and want[:, 1].any() and want[:, 2].any()
    assert np.array_equal(got, want)


@pytest.mark.parametrize("w,h,bpc", _ext_cases((8, 10)))
def test_siti(w, h, bpc):
    from tests.test_gpu_siti import _close, _frames, _run, _want
    refs, diss = _frames(w, h, bpc, 1, 1, 2, seed=w + bpc)
    ext4 = _run(w, h, bpc, 1, 1, refs, diss)[4]
    _close(ext4[:, :4], _want(refs, diss, bpc))
    assert (ext4[0, [1, 3]] == 0.0).all() and (ext4[1, [1, 3]] > 0.0).all()


@pytest.mark.parametrize("w,h,bpc", _ext_cases((8, 10)))
@pytest.mark.parametrize("kind", ["noise", "extreme"])
def test_integrity(w, h, bpc, kind):
    from tests import integrity_ref as R
    from tests.test_gpu_integrity import _clip, _run, _same
    refs, diss = _clip(w, h, bpc, 1, 1, 2, seed=w + bpc, kind=kind)
    got = _run(w, h, bpc, 1, 1, refs, diss)
    _same(got, R.rows(diss, R.black_threshold(bpc)))
    if kind == "extreme":
        assert got[1, 0] == float(((1 << bpc) - 1) * w * h)


@pytest.mark.parametrize("w,h,bpc", [(16, 16384, 8), (16, 16384, 10), (16384, 16, 10)])
def test_cambi(w, h, bpc):
    """(16384 x 16 at 8 bit is test_gpu_cambi.py's test_window_wider_than_the_frame.)  The distorted side only: the numpy
    restatement of one such plane takes three to eight seconds, more than the rest of this file together."""
    from pqa2_amd import _native as N
    from tests import cambi_ref as R
    from tests.test_gpu_cambi import _close, _ramp, _run
    r = _ramp(w, h, bpc, 24, seed=w, dither=0.05)
    d = _ramp(w, h, bpc, 9, seed=w + 1, dither=0.05)
    _, ext = _run(w, h, bpc, [r], [d], features=N.FEAT_CAMBI)
    want = R.cambi(d, bpc)
    print(f"\n{w}x{h} {bpc}-bit: cambi {ext[0, 22]!r} (restatement {want!r})")
    assert want > 0 and _close(ext[0, 22], want)
    assert np.isnan(ext[0, 23])


@pytest.mark.parametrize("w,h,transfer,bpc", [(w, h, t, b) for (w, h) in EXT_SIZES for (t, b) in (("bt1886", 8), ("pq", 10))])
def test_delta_itp(w, h, transfer, bpc):
    from tests.test_gpu_ciede import _planes
    from tests.test_gpu_itp import _check_rows, _engine, _spec, _tol
    sp, ref_spec = _spec(transfer, bpc)
    ref, dis = _planes(w, h, bpc, 1, 1, seed=w + bpc)
    with _engine(w, h, bpc, 1, 1) as eng:
        rows = eng.delta_itp([ref], [dis], sp)
    _check_rows(rows, [ref], [dis], ref_spec, 1, 1, _tol(transfer, bpc), f"{w}x{h} {transfer} {bpc} bit")
