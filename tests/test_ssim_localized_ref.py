"""The premises of tests/test_gpu_ssim_localized.py, pinned on the CPU with the restatement alone
(tests/ssim_family_ref.py, tests/ssim_localized_ref.py):

  1. the f32 mode of the restatement is additive: the f64 results equal a frozen copy of the earlier code bit for bit, and
     the f32 mode stays in f32;
  2. a flat mid-grey pair gives l = c = s = 1 exactly, f64 and f32, so `deficit = value - 1` is the patch's own;
  3. the sweep sizes have the tiles their table claims (from the kernels' tile constants);
  4. moving the patch by a multiple of 16 pixels inside the interior leaves all 20 slots unchanged (1e-14), so interior
     placements can share one evaluation;
  5. the conditions under which the bar means what it says: on interior placements the f32 restatement stays within
     SSF_REL32_MAX of f64 and nothing needs the floor; placements clipped by a corner are what the floor is for;
  6. what the whole-frame test cannot see (the premise of the localized tests): the smallest change of one map column it
     would detect, against the size of the patch's deficits.
"""
import numpy as np
import pytest

from tests import ssim_family_ref as R
from tests import ssim_localized_ref as S


# ---- 1. the f64 path is the earlier code -------------------------------------------------------------------------------------
def _frozen_lcs(x, y):
    """lcs_maps(separable=True) as it stood before the dtype argument."""
    g = R.gaussian_taps()
    n = len(g)

    def flt(img):
        ow, oh = img.shape[1] - n + 1, img.shape[0] - n + 1
        hz = sum(g[k] * img[:, k:k + ow] for k in range(n))
        return sum(g[k] * hz[k:k + oh, :] for k in range(n))

    mx, my = flt(x), flt(y)
    sxx = flt(x * x) - mx * mx
    syy = flt(y * y) - my * my
    sxy = flt(x * y) - mx * my
    sxsy = np.sqrt(np.maximum(sxx, 0.0) * np.maximum(syy, 0.0))
    return ((2.0 * mx * my + R.C1) / (mx * mx + my * my + R.C1), (2.0 * sxsy + R.C2) / (sxx + syy + R.C2),
            (sxy + R.C3) / (sxsy + R.C3))


def _frozen_lpf97(img):
    h, w = img.shape
    pad = img[np.ix_(R._sym_index(h, -4, h + 4), R._sym_index(w, -4, w + 4))]
    hz = sum(R.LPF97[k] * pad[:, k:k + w] for k in range(9))
    full = sum(R.LPF97[k] * hz[k:k + h, :] for k in range(9))
    return full[::2, ::2]


def _frozen_box(img, f):
    if f == 1:
        return img
    h, w = img.shape
    a = f // 2
    pad = img[np.ix_(R._sym_index(h, -a, h - a + f), R._sym_index(w, -a, w - a + f))]
    ow, oh = -(-w // f), -(-h // f)
    acc = np.zeros((oh, ow))
    for dy in range(f):
        for dx in range(f):
            acc += pad[dy:dy + oh * f:f, dx:dx + ow * f:f]
    return acc / (f * f)


def _frozen_record(ref, dis, bpc):
    e = np.full(20, np.nan)
    h, w = ref.shape
    f = R.decimation_factor(w, h)
    to = lambda p: np.asarray(p, np.float64) / float(1 << (bpc - 8))  # noqa: E731
    l, c, s = _frozen_lcs(_frozen_box(to(ref), f), _frozen_box(to(dis), f))
    e[0:4] = [float(np.mean(l * c * s)), float(l.mean()), float(c.mean()), float(s.mean())]
    x, y = to(ref), to(dis)
    lm, cm, sm = [], [], []
    for j in range(R.MS_SCALES):
        l, c, s = _frozen_lcs(x, y)
        lm.append(float(l.mean())); cm.append(float(c.mean())); sm.append(float(s.mean()))
        if j + 1 < R.MS_SCALES:
            x, y = _frozen_lpf97(x), _frozen_lpf97(y)
    e[4] = R.ms_combine(lm, cm, sm)
    e[5:10], e[10:15], e[15:20] = lm, cm, sm
    return e


@pytest.mark.parametrize("w,h,bpc", [(161, 161, 8), (515, 521, 10), (352, 288, 12)])
def test_f64_restatement_is_unchanged_bit_for_bit(w, h, bpc):
    rng = np.random.default_rng(w + bpc)
    dt = S.sample_dtype(bpc)
    ref = rng.integers(0, 1 << bpc, (h, w)).astype(dt)
    dis = np.clip(ref.astype(np.int32) + rng.integers(-40, 41, (h, w)), 0, (1 << bpc) - 1).astype(dt)
    want = _frozen_record(ref, dis, bpc)
    for kw in ({}, {"dtype": np.float64}):
        got = R.ext_record(ref, dis, bpc, **kw)[:20]
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), kw
    x, y = R.to_float(ref, bpc), R.to_float(dis, bpc)
    for a, b in zip(R.lcs_maps(x, y, True), _frozen_lcs(x, y)):
        assert a.dtype == np.float64 and np.array_equal(a.view(np.uint64), b.view(np.uint64))
    assert np.array_equal(R.lpf97_decimate(x).view(np.uint64), _frozen_lpf97(x).view(np.uint64))
    # the f32 mode: every plane and map in f32, close to f64 but not equal to it (it is a second arithmetic, not a cast)
    x32 = R.to_float(ref, bpc, np.float32)
    assert x32.dtype == np.float32 and np.array_equal(x32.astype(np.float64), x)
    assert R.lpf97_decimate(x32, np.float32).dtype == np.float32
    assert R.box_decimate(x32, 3).dtype == np.float32
    for sep in (True, False):
        assert all(m.dtype == np.float32 for m in R.lcs_maps(x32, x32, sep, np.float32))
    e32 = R.ext_record(ref, dis, bpc, dtype=np.float32)[:20]
    assert 0 < np.abs(e32 - want).max() < 1e-5
    with pytest.raises(ValueError):
        R.lcs_maps(x, y, True, np.float16)


# ---- 2. flat frames --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bpc", [8, 10, 12])
@pytest.mark.parametrize("w,h", [S.WIDE, S.ODD_TALL, S.UNION, S.BOX_WIDE, (161, 161)])
def test_flat_pair_is_exactly_one(w, h, bpc):
    flat = S.flat_frame(w, h, bpc)
    assert 2 * int(flat[0, 0]) == 1 << bpc
    for dt in (np.float64, np.float32):
        e = S.record(flat, flat, bpc, dt)
        assert e.tolist() == [1.0] * S.N_SLOT, (dt.__name__, (e - 1.0).tolist())


def test_f32_flat_window_has_zero_moments():
    """The offset formulation: where the 11 x 11 window is flat the f32 maps are exactly 1 although a patch is in the frame
    (plain E[x^2] - mu^2 in f32 would leave rounding residue of the order of C2 there)."""
    w, h = 200, 208
    ref, dis = S.patch_frame(w, h, 64, 64, S.SEEDS[0], 8)
    x, y = R.to_float(ref, 8, np.float32), R.to_float(dis, 8, np.float32)
    for m in R.lcs_maps(x, y, True, np.float32):
        far = np.ones(m.shape, bool)
        far[64 - 10:64 + S.PATCH, 64 - 10:64 + S.PATCH] = False     # windows (top-left corner) that miss the patch
        assert np.all(m[far] == 1.0) and np.any(m[~far] != 1.0)


# ---- 3. the sweep sizes have the seams their table claims ----------------------------------------------------------------
def test_sweep_sizes_have_the_claimed_tiles():
    assert (S.MAP_TW, S.MAP_TH, S.DOWN_TW, S.DOWN_TH) == (64, 32, 64, 16)
    lv = R.ms_scale_sizes(*S.WIDE)
    assert lv[4] == (129, 11) and S.map_tiles(*lv[4]) == (2, 1)           # map 119 x 1: two map-tile columns at scale 4
    assert S.down_tiles(*lv[3]) == (3, 1)                                  # the 3 -> 4 step writes 129 columns
    assert S.map_tiles(*lv[3])[0] == 4 and S.down_tiles(*lv[2])[0] == 5   # and more than one tile at scale 3
    lv = R.ms_scale_sizes(*S.TALL)
    assert lv[4] == (11, 129) and S.map_tiles(*lv[4]) == (1, 4) and S.down_tiles(*lv[3]) == (1, 9)
    assert [S.map_tiles(*s)[1] for s in lv] == [65, 32, 16, 8, 4] and [S.down_tiles(*s)[1] for s in lv[:4]] == [65, 33, 17, 9]
    for (w, h) in (S.ODD_WIDE, S.ODD_TALL):
        assert all(a % 2 == 1 and b % 2 == 1 for a, b in R.ms_scale_sizes(w, h))          # odd at every level
        assert R.ms_ssim_fits(w, h) and max(S.map_tiles(*R.ms_scale_sizes(w, h)[4])) >= 2
    assert S.decimation_only(*S.ODD_WIDE) == (1, 1) and S.decimation_only(*S.ODD_TALL) == (1, 1)
    assert S.decimation_only(*S.UNION) == (1, 0) and S.map_tiles(*S.UNION) == (3, 7) and S.fused_tiles(*S.UNION) == (4, 7)
    for wd in range(129, 400):      # decimation-only columns: exactly the widths 64 k + 1 ... 64 k + 10
        assert (S.decimation_only(wd, 208)[0] == 1) == (1 <= wd % 64 <= 10), wd
    for hh in range(161, 400):      # decimation-only rows: the heights 32 k + 1 ... 32 k + 10 (161 and 193, not 177)
        assert (S.decimation_only(208, hh)[1] == 1) == (1 <= hh % 32 <= 10), hh
    for (w, h) in (S.BOX_TALL, S.BOX_WIDE):
        assert R.decimation_factor(w, h) == 2 and R.ms_ssim_fits(w, h)
    assert S.map_tiles(1104 // 2, 400 // 2) == (9, 6) and S.map_tiles(400 // 2, 1104 // 2) == (3, 17)    # of the decimated plane
    for name in S.SWEEPS:           # every placement list starts on the STEP grid and stays inside the frame
        w, h, places, axis = S.sweep(name)
        assert len(set(places)) == len(places) and all(0 <= x < w and 0 <= y < h for x, y in places)
        if axis is not None:
            inner = S.interior_mask(w, h, places, axis)
            assert sum(inner) >= 30 and not inner[0] and not inner[-1]


# ---- 4. translation -----------------------------------------------------------------------------------------------------------
_OWN = {}    # (sweep, placement) -> (f64, f32) records of interior placements evaluated on their own


def _own(name, p, bpc=8):
    if (name, p, bpc) not in _OWN:
        w, h, _, _ = S.sweep(name)
        _OWN[name, p, bpc] = (S.pair_records(w, h, *p, bpc), S.pair_records(w, h, *p, bpc, np.float32))
    return _OWN[name, p, bpc]


def _picks(name):
    w, h, places, axis = S.sweep(name)
    inner = [p for p, ok in zip(places, S.interior_mask(w, h, places, axis)) if ok]
    return [inner[0], inner[len(inner) // 2], inner[len(inner) // 2 + 1], inner[-1]]


@pytest.mark.parametrize("name", ["wide", "tall"])
def test_shift_by_16_leaves_the_interior_unchanged(name):
    picks = _picks(name)
    base = _own(name, picks[1])[0]
    for p in picks:
        d = np.abs(_own(name, p)[0] - base)
        assert d.max() <= 1e-14, (name, p, float(d.max()), S.SLOTS[int(d.max(0).argmax())])
    # half a step is no translation: scale 4 samples every 16th pixel
    w, h, _, axis = S.sweep(name)
    half = list(picks[1])
    half[axis] += S.STEP // 2
    moved = np.abs(S.pair_records(w, h, *half, 8) - base)
    assert moved[:, [9, 14, 19]].min() > 1e-9      # l, c, s of scale 4: five orders above what a whole step leaves


# ---- 5. the bar's conditions ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,bpc", [("wide", 8), ("tall", 10), ("box2_wide", 10), ("box2_tall", 12)])
def test_interior_placements_stay_under_the_rel32_cap_on_their_own(name, bpc):
    """First and last interior placement, each with its own f64 and f32 evaluation (Expected lets them share the
    anchor's): rel32 < SSF_REL32_MAX in every slot, and their deficit is the anchor's, so no floor."""
    picks = _picks(name)
    anchor = _own(name, picks[1], bpc)[0] - 1.0
    assert np.all(np.abs(anchor) > 1e-4)                         # every slot, l included, has a deficit worth measuring
    for p in (picks[0], picks[-1]):
        e64, e32 = _own(name, p, bpc)
        nrm = S.normaliser(e64 - 1.0, anchor)
        assert np.all(np.abs(e64 - 1.0) >= S.FLOOR * np.abs(anchor))
        rel32 = np.abs(e32 - e64) / nrm
        assert rel32.max() < S.SSF_REL32_MAX, (name, bpc, p, S.SLOTS[int(rel32.max(0).argmax())], float(rel32.max()))


@pytest.mark.parametrize("name,bpc", [("wide", 8), ("tall", 12), ("box2_wide", 8), ("corners_wide", 8), ("corners_tall", 10),
                                      ("union_x", 8)])
def test_bar_conditions_hold_from_the_restatement_alone(name, bpc):
    """A thinned placement list (the GPU module asserts the same on the full lists)."""
    w, h, places, axis = S.sweep(name)
    thin = places[::8] + places[-2:] if axis is not None else places[:1] + places[1::5]
    e = S.Expected(w, h, thin, axis, bpc, threads=4)
    assert np.all(np.isfinite(e.exp64)) and np.all(np.isfinite(e.exp32)) and np.all(e.deficit[e.anchor] < -1e-4)
    assert not e.floor_used()[e.interior].any()
    if axis is not None:
        assert e.interior.sum() >= 3
        assert e.rel32[e.interior].max() < S.SSF_REL32_MAX
        assert not e.floor_used()[e.anchor].any()
    # the bar is never looser than 8 x the f32 restatement's own distance plus one f32 ulp, never tighter than REL_TOL
    assert np.all(e.bar >= S.REL_TOL * e.norm + S.ULP32) and np.all(e.bar >= np.abs(e.exp32 - e.exp64))
    if name.startswith("corners"):
        # the clipped bottom-right corner: 56 x 56 pixels inside the 80-pixel invalid border of scale 4 -- the floor's case
        k = e.places.index((w - S.PATCH + 8, h - S.PATCH + 8)) if (w - S.PATCH + 8, h - S.PATCH + 8) in e.places else None
        assert e.floor_used().any() or k is None


# ---- 6. what the whole-frame bar sees ----------------------------------------------------------------------------------------
def test_whole_frame_bar_is_larger_than_a_seam_error_on_the_patch():
    """test_gpu_ssim_family.py::test_matches_the_restatement on its own 352 x 288 content: the smallest relative change of
    ALL windows of one map column that moves a mean by its TOL = 1e-5, and TOL against the patch's deficits."""
    from tests.test_gpu_ssim_family import TOL, _clip
    w, h, bpc = 352, 288, 8
    refs, diss = _clip(w, h, 1, bpc, seed=w + h + bpc)
    eps = S.column_detection_threshold(refs[0], diss[0], bpc, TOL)
    print("\nsmallest detectable relative change of one map column at 352 x 288: " +
          " ".join(f"{k} {v:.1e}" for k, v in eps.items()))
    assert min(eps[k] for k in ("float_ssim", "float_ssim_s", "ms_s_s0", "ms_c_s0")) > 2e-3     # 0.2 % of a whole column
    assert eps["ms_s_s0"] > 3e-3 > eps["ms_s_s4"] > 1e-4       # it grows with the map's width: 3.4e-3 * 342 / mw
    # the localized bar on the anchor placement of the wide sweep is 4 ... 67 times tighter than TOL, and TOL is 0.02 % ...
    # 1.7 % of the patch's deficits: an error of a percent of the patch's own deficit passes the whole-frame bar even on
    # a frame that holds nothing but the patch
    wd, ht, places, axis = S.sweep("wide")
    e = S.Expected(wd, ht, [_picks("wide")[1]], axis, 8, threads=2)
    ratio = TOL / e.bar[0]
    print(f"TOL / localized bar per slot: {ratio.min():.0f} ... {ratio.max():.0f}; TOL / |deficit|: "
          f"{(TOL / np.abs(e.deficit[0])).min():.1e} ... {(TOL / np.abs(e.deficit[0])).max():.1e}")
    assert ratio.min() > 3 and (TOL / np.abs(e.deficit[0])).max() < 0.05
