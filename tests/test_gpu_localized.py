"""Localized-content parity of the VIF, ADM and motion kernels: a parity test that a wrong halo cannot pass.

The whole-frame tests (test_gpu_parity.py) hold a feature to 5e-5 of its WHOLE value on textured frames; an error
confined to a seam -- a tile's halo column, the first lane of a 60-column ADM stripe, the row where one march segment
hands over to the next, the mirrored last column of an odd width, the ADM crop border, the second 252-wide VIF tile of
scales 2 and 3 -- is diluted 50-fold by the rest of the frame.  Here the only texture is a 32 x 32 patch on a flat
mid-grey frame (tests/localized_ref.py; premises pinned on the CPU by tests/test_localized_ref.py), the patch is swept
over the frame in steps of 16 pixels so that every seam of every scale is straddled, and the bar is

    |gpu - oracle64| <= max(REL_TOL, 8 x rel32) x max(|contribution|, 0.01 |oracle64|)

with contribution = oracle64(patch frame) - oracle64(flat frame) and rel32 the f32 oracle's own distance from f64 in
the same normalisation (tests/fuzz_parity.py's rule).  A failure names the placement, the feature and the scale: that
is the seam.

  1. flat frames: the f32 kernels give the oracles' exact values (==), every bit depth, both kernel families;
  2. placement sweeps against the oracles (wide, tall, corners of odd frames; 8 / 10 / 12 bit; kernel switches;
     integer VIF border; gain limits);
  3. translation on the GPU alone: all interior placements of a sweep agree within twice the bar;
  4. the fixed-point kernels, bit-equal to IntOracle on the same clips and on wide / tall noise, checkerboard and
     flat-patch frames -- the first fixed-point inputs with more than one tile at scales 2 and 3.
"""
import contextlib
import functools
import os

import numpy as np
import pytest

from tests import localized_ref as L

pytestmark = pytest.mark.gpu

MAX_BATCH = 7    # 256-, 130-, 64-, 36-, 34-, 32-, 16- and 6-frame clips: never a divisor, so every clip ends in a partial batch

CONFIGS = {
    "default": {},
    "no_pyramid": {"PQA_ADM_PYRAMID": "0"},
    "fallbacks": {"PQA_VIF_MFMA": "0", "PQA_ADM_MARCH": "0", "PQA_MOTION_MARCH": "0"},
}


@contextlib.contextmanager
def _switches(env):
    """The kernel switches are read at pqa_create: set them around the context's creation and restore them."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _run(w, h, refs, diss, bpc, config="default", **kw):
    from pqa2_amd.engine import FeatureEngine
    n = len(refs)
    assert n % MAX_BATCH != 0
    with _switches(CONFIGS[config]):
        eng = FeatureEngine(w, h, bit_depth=bpc, max_batch=MAX_BATCH, **kw)
    with eng:
        for i in range(n):
            eng.submit(i, [refs[i]], [diss[i]])
        return eng.collect(0, n)[:, :L.N_FEAT]


# ---- the cases: a sweep, a bit depth and which of its placements ---------------------------------------------------------
def _ends(places):
    return places[:8] + places[-8:]


def _every_fourth(places):
    return places[::4]


def _eight_interior(name):
    def pick(places):
        w, h, _, axis = L.sweep(name)
        inner = [p for p, ok in zip(places, L.interior_mask(w, h, places, axis)) if ok]
        return inner[::len(inner) // 8][:8]
    return pick


def _three_interior(name):
    def pick(places):
        w, h, _, axis = L.sweep(name)
        inner = [p for p, ok in zip(places, L.interior_mask(w, h, places, axis)) if ok]
        return [inner[0], inner[len(inner) // 2], inner[-1]]
    return pick


CASES = {
    # name: (sweep, bit depth, placement filter)
    "wide8": ("wide", 8, None), "tall8": ("tall", 8, None),
    "corners_wide8": ("corners_wide", 8, None), "corners_tall8": ("corners_tall", 8, None),
    "wide10": ("wide", 10, _every_fourth), "tall10": ("tall", 10, _every_fourth),
    "corners_wide12": ("corners_wide", 12, None), "corners_tall12": ("corners_tall", 12, None),
    "wide12": ("wide", 12, _eight_interior("wide")), "tall12": ("tall", 12, _eight_interior("tall")),
    "wide_ends8": ("wide", 8, _ends), "tall_ends8": ("tall", 8, _ends),
    "wide_three8": ("wide", 8, _three_interior("wide")), "tall_three8": ("tall", 8, _three_interior("tall")),
}
SWEEP_CASES = ["wide8", "tall8", "corners_wide8", "corners_tall8", "wide10", "tall10", "corners_wide12", "corners_tall12",
               "wide12", "tall12"]


def _case(case):
    name, bpc, pick = CASES[case]
    w, h, places, axis = L.sweep(name)
    return w, h, (pick(places) if pick else places), axis, bpc


@functools.lru_cache(maxsize=2)
def _clip(case, enhance=False):
    w, h, places, _, bpc = _case(case)
    return L.placement_clip(w, h, places, bpc, enhance)


_EXPECTED = {}   # computed once, shared by every configuration of a case, never modified


def _expected(oracle64, oracle32, case, enhance=False, **kw):
    key = (case, enhance, tuple(sorted(kw.items())))
    if key not in _EXPECTED:
        w, h, places, axis, bpc = _case(case)
        e = L.Expected(oracle64, oracle32, w, h, places, axis, bpc, enhance, **kw)
        for a in (e.exp64, e.exp32, e.bar, e.norm, e.rel32):
            a.setflags(write=False)
        _EXPECTED[key] = e
    return _EXPECTED[key]


_RECORDS = {}    # GPU records of (case, config): the translation test reads what the sweep test measured


def _records(case, config):
    if (case, config) not in _RECORDS:
        w, h, places, _, bpc = _case(case)
        refs, diss = _clip(case)
        _RECORDS[case, config] = _run(w, h, refs, diss, bpc, config).reshape(len(places), 2, L.N_FEAT)
    return _RECORDS[case, config]


def _check_premises(e):
    """From the oracle alone: the bar means what it says."""
    assert e.rel32.max() < L.REL32_MAX, ("f32 oracle too far from f64", e.places[int(e.rel32.argmax())], float(e.rel32.max()))
    assert not e.floor_used()[:, L.CHECKED][e.interior].any(), "an interior placement needs the 0.01 floor"


def _check_against_oracle(e, got, label):
    """got [n, 2, 17] against e.exp64 under e.bar; prints the worst normalised distance per feature and where."""
    assert np.all(np.isfinite(got)), label
    dist = np.where(L.CHECKED, np.abs(got - e.exp64) / e.norm, 0.0)
    over = np.where(L.CHECKED, np.abs(got - e.exp64) / e.bar, 0.0)
    print(f"\n{label}: worst |gpu - f64| / max(|contribution|, 0.01 |f64|) per feature (f32 oracle's own: {e.rel32.max():.1e})")
    for f in range(L.N_FEAT):
        k, t = np.unravel_index(int(dist[:, :, f].argmax()), dist.shape[:2])
        print(f"  {L.FEATURES[f]:11s} {dist[k, t, f]:.2e} ({over[k, t, f]:.2f} of the bar) at {e.places[k]} frame {t}")
    bad = np.argwhere(over > 1.0)
    msg = [f"{L.FEATURES[f]} at placement {e.places[k]} frame {t}: gpu {got[k, t, f]!r} f64 {e.exp64[k, t, f]!r} "
           f"distance {dist[k, t, f]:.2e} = {over[k, t, f]:.1f} x the bar" for k, t, f in bad[:8]]
    assert bad.size == 0, (label, len(bad), msg)
    assert np.all(got[0, 0, 16] == 0.0)
    return dist.max(axis=(0, 1))


# ---- 1. flat frames ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", ["default", "fallbacks"])
@pytest.mark.parametrize("bpc", [8, 10, 12])
@pytest.mark.parametrize("w,h", [L.WIDE, L.ODD_WIDE, L.TALL, (16, 16)])
def test_flat_frames_are_exact(oracle64, w, h, bpc, config):
    """ref = dis = mid grey: every sample centres to exactly zero, so VIF num = den = the pixel count of the scale, ADM
    num = den (the constant term alone; the oracles differ in its last bits, so it is held to REL_TOL) and motion 0."""
    flat = L.flat_frame(w, h, bpc)
    got = _run(w, h, [flat] * 3, [flat] * 3, bpc, config)
    want = L.flat_features(oracle64, w, h, bpc)
    assert want[:8].tolist() == L.flat_expected(w, h).tolist()
    for i in range(3):
        assert got[i, :8].tolist() == want[:8].tolist(), (i, (got[i, :8] - want[:8]).tolist())
        assert got[i, 8:12].tolist() == got[i, 12:16].tolist(), (i, (got[i, 8:12] - got[i, 12:16]).tolist())
        assert got[i, 16] == 0.0
    assert (np.abs(got[:, 8:16] - want[8:16]) / want[8:16]).max() < L.REL_TOL


# ---- 2. placement sweeps against the oracles ------------------------------------------------------------------------------
@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("case", SWEEP_CASES)
def test_placement_sweep(oracle32, oracle64, case, config):
    e = _expected(oracle64, oracle32, case)
    _check_premises(e)
    _check_against_oracle(e, _records(case, config), f"{case} / {config}")


@pytest.mark.parametrize("case", ["corners_wide8", "corners_tall8", "wide_ends8", "tall_ends8"])
def test_placement_sweep_integer_vif_border(oracle32, oracle64, case):
    """vif_border = VIF_BORDER_INTEGER (integer_vif.c's reflect-101 padding) where it matters: the patch at the frame edge."""
    from pqa2_amd import _native as N
    w, h, places, _, bpc = _case(case)
    e = _expected(oracle64, oracle32, case, vif_border101=True)
    if case.endswith("_ends8"):    # the float-border values of these placements are part of the full sweep's
        full = _expected(oracle64, oracle32, case.replace("_ends", "")).exp64
        plain = np.concatenate([full[:8], full[-8:]])
    else:
        plain = _expected(oracle64, oracle32, case).exp64
    assert np.abs(e.exp64[..., :8] - plain[..., :8]).max() > 0 and np.array_equal(e.exp64[..., 8:], plain[..., 8:])
    _check_premises(e)
    refs, diss = _clip(case)
    got = _run(w, h, refs, diss, bpc, vif_border=N.VIF_BORDER_INTEGER).reshape(len(places), 2, L.N_FEAT)
    _check_against_oracle(e, got, f"{case} / integer border")


@pytest.mark.parametrize("case", ["wide_three8", "tall_three8"])
def test_placement_sweep_gain_limits(oracle32, oracle64, case):
    """vif_enhn_gain_limit = adm_enhn_gain_limit = 1.0 (the neg models) on a sharpened patch, dis = 2 ref - dis clipped,
    so that the limit bites; first, middle and last interior placement."""
    w, h, places, _, bpc = _case(case)
    e = _expected(oracle64, oracle32, case, enhance=True, vif_gain_limit=1.0, adm_gain_limit=1.0)
    unlimited = _expected(oracle64, oracle32, case, enhance=True)
    assert (np.abs(e.contribution - unlimited.contribution) / e.norm)[..., :16].max() > 1e-2     # the option matters here
    assert e.interior.all()
    _check_premises(e)
    refs, diss = _clip(case, True)
    got = _run(w, h, refs, diss, bpc, vif_enhn_gain_limit=1.0, adm_enhn_gain_limit=1.0).reshape(len(places), 2, L.N_FEAT)
    _check_against_oracle(e, got, f"{case} / gain limits 1.0")


# ---- 3. translation on the GPU, no oracle values compared ----------------------------------------------------------------
@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("case", ["wide8", "tall8"])
def test_interior_placements_agree_on_the_gpu(oracle32, oracle64, case, config):
    """Every pair of interior placements differs by at most twice the bar (largest minus smallest record per feature).  The
    oracle only supplies the bar's scale; this is the dense check a re-tiling change can run while iterating."""
    e = _expected(oracle64, oracle32, case)
    got = _records(case, config)
    inner = np.flatnonzero(e.interior)
    assert len(inner) >= 40
    g = got[inner]
    hi, lo = g.argmax(axis=0), g.argmin(axis=0)
    spread = np.where(L.CHECKED, (g.max(axis=0) - g.min(axis=0)) / (2.0 * e.bar[e.anchor]), 0.0)
    t, f = np.unravel_index(int(spread.argmax()), spread.shape)
    print(f"\n{case} / {config}: worst spread {spread.max():.2f} of twice the bar: {L.FEATURES[f]} frame {t}, placements "
          f"{e.places[inner[hi[t, f]]]} and {e.places[inner[lo[t, f]]]}")
    bad = [(L.FEATURES[f], int(t), e.places[inner[hi[t, f]]], e.places[inner[lo[t, f]]], float(spread[t, f]))
           for t, f in np.argwhere(spread > 1.0)]
    assert not bad, bad[:8]


# ---- 4. fixed-point kernels: bit-equality with IntOracle -------------------------------------------------------------------
def _fixed_both(w, h, refs, diss, bpc):
    from oracle.int_oracle import IntOracle
    from pqa2_amd import _native as N
    want = IntOracle().clip_features_mt(refs, diss, bpc, threads=8)
    got = _run(w, h, refs, diss, bpc, fixed_point=N.FIXED_ALL)
    return got, want


@pytest.mark.parametrize("bpc", [8, 10])
@pytest.mark.parametrize("name", list(L.SWEEPS))
def test_fixed_point_placement_sweep_is_bit_exact(name, bpc):
    """Every placement of the wide, tall and corner clips, every feature double (motion across placements included)."""
    w, h, places, _ = L.sweep(name)
    refs, diss = L.placement_clip(w, h, places, bpc)
    got, want = _fixed_both(w, h, refs, diss, bpc)
    bad = np.argwhere(got.view(np.uint64) != want.view(np.uint64))
    assert bad.size == 0, [(places[i // 2], int(i % 2), L.FEATURES[f], got[i, f], want[i, f]) for i, f in bad[:6]]


@pytest.mark.parametrize("w,h,bpc", [(2064, 32, 8), (2031, 17, 8), (32, 1056, 8), (17, 1057, 8), (2064, 128, 12)])
def test_fixed_point_wide_and_tall_content_is_bit_exact(w, h, bpc):
    """Noise, checkerboard extremes and flat patches (test_fixed_point_random_geometry_sweep's kinds) at widths and heights
    with more than one tile at scales 2 and 3."""
    rng = np.random.default_rng(20250420 + w + h)
    peak = (1 << bpc) - 1
    dt = L.sample_dtype(bpc)
    refs, diss = [], []
    for kind in range(3):
        for t in range(2):
            if kind == 0:
                y = rng.integers(0, peak + 1, (h, w))
            elif kind == 1:   # flat patches: exact zeros in the high-pass bands
                y = np.repeat(np.repeat(rng.integers(0, peak + 1, (-(-h // 16), -(-w // 16))), 16, 0), 16, 1)[:h, :w] + t
            else:             # extremes: checkerboard of 0 / peak, the largest coefficients the Q formats must hold
                y = ((np.add.outer(np.arange(h), np.arange(w)) + t) % 2) * peak
            refs.append(np.clip(y, 0, peak).astype(dt))
            diss.append(np.clip(refs[-1].astype(np.int32) + rng.integers(-6, 7, (h, w)), 0, peak).astype(dt))
    got, want = _fixed_both(w, h, refs, diss, bpc)
    bad = np.argwhere(got.view(np.uint64) != want.view(np.uint64))
    assert bad.size == 0, [(("noise", "flat patches", "checkerboard")[i // 2], int(i % 2), L.FEATURES[f], got[i, f], want[i, f])
                           for i, f in bad[:6]]
