"""The premises of tests/test_gpu_localized.py, pinned on the CPU with the oracles alone (tests/localized_ref.py):

  1. a flat mid-grey frame is exact in all three oracles: VIF num = den = the pixel count of the scale, ADM num = den,
     motion 0;
  2. moving the patch by a multiple of 16 pixels inside the interior leaves all 17 features unchanged (1e-13), so the
     interior placements of a sweep can share one oracle evaluation -- and a shift of 8 would not do;
  3. the contribution normalisation sees a one-column, one-grey-level change that whole-frame normalisation cannot
     (the test of the test);
  4. the conditions under which the bar means what it says: no interior placement needs the 0.01 floor, and the f32
     oracle stays within 2e-5 of f64, contribution-normalised.
"""
import numpy as np
import pytest

from tests import localized_ref as L


@pytest.fixture(scope="module")
def int_oracle():
    from oracle.int_oracle import IntOracle
    return IntOracle()


@pytest.mark.parametrize("bpc", [8, 10])
@pytest.mark.parametrize("w,h", [L.WIDE, L.ODD_TALL])
def test_flat_frame_is_exact_in_every_oracle(oracle32, oracle64, int_oracle, w, h, bpc):
    flat = L.flat_frame(w, h, bpc)
    assert 2 * int(flat[0, 0]) == 1 << bpc           # mid grey: centres to exactly zero
    want = L.flat_expected(w, h)
    assert want[0] == w * h
    for orc in (oracle64, oracle32):
        f = L.flat_features(orc, w, h, bpc)
        assert f[:8].tolist() == want.tolist(), orc.precision
        assert f[8:12].tolist() == f[12:16].tolist() and np.all(f[8:12] > 0), orc.precision
        assert f[16] == 0.0
    assert int_oracle.vif(flat, flat, bpc).tolist() == want.tolist()
    adm = int_oracle.adm(flat, flat, bpc)
    assert adm[:4].tolist() == adm[4:].tolist() and np.all(adm[:4] > 0)
    assert int_oracle.motion_sad(int_oracle.motion_blur(flat, bpc), int_oracle.motion_blur(flat, bpc)) == 0


@pytest.mark.parametrize("name", ["wide", "tall"])
def test_shift_by_16_leaves_the_interior_unchanged(oracle64, name):
    w, h, places, axis = L.sweep(name)
    inner = [p for p, ok in zip(places, L.interior_mask(w, h, places, axis)) if ok]
    assert len(inner) >= 40
    # the first and last interior placements (nearest the crop border), the middle one and its neighbour
    picks = [inner[0], inner[len(inner) // 2], inner[len(inner) // 2 + 1], inner[-1]]
    base = L.pair_features(oracle64, w, h, *picks[1], 8)
    for p in picks:
        got = L.pair_features(oracle64, w, h, *p, 8)
        rel = np.abs(got - base) / np.maximum(np.abs(base), 1e-300)
        assert rel.max() <= 1e-13, (name, p, float(rel.max()), L.FEATURES[int(rel.max(0).argmax())])
    # one step outside the interior the crop border is felt (which is why those placements get their own oracle run) ...
    k = places.index(inner[0])
    assert not L.is_interior(places[k - 1][axis], (w, h)[axis])
    # ... and half a step is no translation at all: the coarsest scale samples every 8th pixel with a 2-sample phase
    half = list(picks[1])
    half[axis] += L.STEP // 2
    got = L.pair_features(oracle64, w, h, *half, 8)
    flat = L.flat_features(oracle64, w, h, 8)
    assert (np.abs(got - base) / L.normaliser(base, flat))[:, 11].max() > 1e-2


# The one-column change: +1 grey level on 32 distorted pixels, column 14 of the patch.  With the patch at x = 992 of
# the wide frame that is pixel 1006, inside the two-sample halo that the second 252-wide VIF tile of scale 2 (starting
# at 4 * 252 = 1008) reads from its left neighbour.
SEAM_POS, SEAM_COL = 992, 14
ADM0_LEVELS = 1   # smallest level change at which ADM num scale 0 clears twice the bar as well (at this column one level
                  # already moves it by 2.5 and 11.2 bars; at most other columns it takes 2 to 4 levels)


def _bump(dis, x, y, level):
    out = dis.copy()
    sl = (slice(y, y + L.PATCH), slice(x + SEAM_COL, x + SEAM_COL + 1))
    out[sl] = np.clip(out[sl].astype(np.int32) + level, 0, 255)
    assert np.count_nonzero(out != dis) >= L.PATCH - 2
    return out


@pytest.mark.parametrize("seed", L.SEEDS)
def test_contribution_normalisation_sees_a_one_column_change(oracle32, oracle64, seed):
    w, h = L.WIDE
    x, y = SEAM_POS, 48
    flat = L.flat_features(oracle64, w, h, 8)
    ref, dis = L.patch_frame(w, h, x, y, seed, 8)
    e64 = oracle64.clip_features([ref], [dis], 8)[0]
    e32 = oracle32.clip_features([ref], [dis], 8)[0]
    nrm = L.normaliser(e64, flat)
    assert np.all(np.abs(L.contribution(e64, flat))[:16] >= L.FLOOR * np.abs(e64[:16]))   # no floor here
    rel32 = float((np.abs(e32 - e64) / nrm)[:16].max())
    assert rel32 < L.REL32_MAX
    bar = max(L.REL_TOL, L.REL32_FACTOR * rel32)
    moved = np.abs(oracle64.clip_features([ref], [_bump(dis, x, y, 1)], 8)[0] - e64) / nrm
    print(f"\nseed {seed}: bar {bar:.2e}; one column, one level moves (x bar) " +
          " ".join(f"{L.FEATURES[k]} {moved[k] / bar:.1f}" for k in (0, 1, 2, 3, 8, 9, 10, 11)))
    for k in (0, 1, 2, 3, 9, 10, 11):     # VIF num of all four scales, ADM num of scales 1-3
        assert moved[k] >= 2.0 * bar, (L.FEATURES[k], float(moved[k]), bar)
    levels = [lv for lv in (1, 2, 3, 4)
              if abs(oracle64.clip_features([ref], [_bump(dis, x, y, lv)], 8)[0][8] - e64[8]) / nrm[8] >= 2.0 * bar]
    assert levels and levels[0] == ADM0_LEVELS, levels


def test_whole_frame_normalisation_does_not_see_it(oracle64):
    """The same change inside a 960 x 540 noise frame, divided by the whole feature value: far under REL_TOL (a quarter
    of the pixels of 1080p, so four times the 1.1e-6 measured there)."""
    w, h = 960, 540
    rng = np.random.default_rng(1)
    ref = rng.integers(0, 256, (h, w), dtype=np.uint8)
    dis = np.clip(ref.astype(np.int32) + rng.integers(-L.NOISE, L.NOISE + 1, ref.shape), 0, 255).astype(np.uint8)
    a = oracle64.clip_features([ref], [dis], 8)[0]
    b = oracle64.clip_features([ref], [_bump(dis, 480, 250, 1)], 8)[0]
    rel = np.abs(a - b)[:16] / np.abs(a[:16])
    print(f"\nwhole-frame: the one-column change moves the features by at most {rel.max():.2e} of their value")
    assert 0 < rel.max() < L.REL_TOL / 5


@pytest.mark.parametrize("name,bpc", [("wide", 8), ("tall", 8), ("wide", 10), ("tall", 12), ("corners_wide", 8),
                                      ("corners_tall", 12)])
def test_bar_conditions_hold_from_the_oracle_alone(oracle32, oracle64, name, bpc):
    """A thinned placement list (every eighth placement and both ends; the GPU module asserts the same on the full
    lists): interior placements never use the floor, rel32 < 2e-5 everywhere, and a patch outside the ADM crop
    contributes exactly 0 -- what the floor is for."""
    w, h, places, axis = L.sweep(name)
    thin = places[::8] + places[-2:] if axis is not None else places[:8]
    e = L.Expected(oracle64, oracle32, w, h, thin, axis, bpc, threads=4)
    assert e.rel32.max() < L.REL32_MAX, (name, bpc, float(e.rel32.max()), thin[int(e.rel32.argmax())])
    used = e.floor_used()[:, L.CHECKED]
    assert not used[e.interior].any()
    if axis is not None:
        assert e.interior.sum() >= 3
        assert np.all(np.abs(e.contribution[e.anchor][:, :16]) >= 0.0115 * e.flat[:16])
    else:
        assert np.any(e.contribution[0][:, 8:12] == 0.0)      # the (0, 0) corner: outside the crop of some ADM scale
        assert used.any()
