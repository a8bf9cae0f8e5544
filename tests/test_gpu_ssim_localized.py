"""Localized-content parity of float_ssim / float_ms_ssim (csrc/ssim_family.hip): a parity test that a wrong seam cannot
pass.

test_gpu_ssim_family.py holds whole-frame means of textured frames to an absolute 1e-5; an error on a seam -- a map
tile's halo column, the 8-row group of a thread, a decimation-only tile of the scale-0 launch (the union of the 64 x 32 map
tiling and the fused decimation's 32 x 16 tiling), a parity-split LDS column of ssf_down_kernel, the folded last column of
an odd level, the last box of a width that is no multiple of the box factor -- is diluted by the rest of the frame.  Here
the only texture is a strongly distorted 64 x 64 patch on a flat mid-grey pair (tests/ssim_localized_ref.py; premises
pinned on the CPU by tests/test_ssim_localized_ref.py), swept in steps of 16 pixels, and the bar is

    |gpu - ref64| <= max(REL_TOL, 8 x rel32) x max(|deficit|, 0.01 |anchor's deficit|) + 2^-23

with deficit = ref64 - 1 and rel32 the f32 restatement's own distance from f64 in the same normalisation.

  1. flat frames: every slot within one f32 ulp of 1;
  2. placement sweeps against the restatement (wide, tall, corners of frames odd at every level, the union tiling, box
     factor 2; 8 / 10 / 12 bit);
  3. translation on the GPU alone: interior placements agree within twice the bar;
  4. size cases: box factors 2, 3, 5, 6, 7 with folded last boxes, decimation-only tile columns and rows together, sizes
     odd at every level; u8 and u16;
  5. float_ssim alone, MS-SSIM alone and both give the same bits (the BOX and the fused-DOWN kernel variants).
"""
import numpy as np
import pytest

from tests import ssim_family_ref as R
from tests import ssim_localized_ref as S

pytestmark = pytest.mark.gpu

MAX_BATCH = 7                       # every clip ends in a partial batch (_run sees to it)
FEAT_FLOAT_SSIM, FEAT_MS_SSIM = 32, 64
BOTH = FEAT_FLOAT_SSIM | FEAT_MS_SSIM


def _run(w, h, refs, diss, bpc, features=BOTH):
    from pqa2_amd.engine import FeatureEngine
    n = len(refs)
    if n % MAX_BATCH == 0:      # a clip of whole batches gets its first frame again at the end (that record is dropped)
        refs, diss = list(refs) + [refs[0]], list(diss) + [diss[0]]
    m = len(refs)
    assert m % MAX_BATCH != 0
    with FeatureEngine(w, h, bit_depth=bpc, features=features, max_batch=MAX_BATCH) as eng:
        for i in range(m):
            eng.submit(i, [refs[i]], [diss[i]])
        return eng.collect_ext(0, m)[1][:n, :S.N_SLOT]


# ---- the cases: a sweep, a bit depth and which of its placements ---------------------------------------------------------
def _every_fourth(places):
    return places[::4]


def _eight_interior(name):
    def pick(places):
        w, h, _, axis = S.sweep(name)
        inner = [p for p, ok in zip(places, S.interior_mask(w, h, places, axis)) if ok]
        return inner[::len(inner) // 8][:8]
    return pick


CASES = {
    # name: (sweep, bit depth, placement filter)
    "wide8": ("wide", 8, None), "tall8": ("tall", 8, None),
    "corners_wide8": ("corners_wide", 8, None), "corners_tall8": ("corners_tall", 8, None),
    "union_x8": ("union_x", 8, None), "box2_tall8": ("box2_tall", 8, None), "box2_wide8": ("box2_wide", 8, None),
    "wide10": ("wide", 10, _every_fourth), "tall10": ("tall", 10, _every_fourth), "union_x10": ("union_x", 10, _every_fourth),
    "box2_tall10": ("box2_tall", 10, _every_fourth), "box2_wide10": ("box2_wide", 10, _every_fourth),
    "corners_wide12": ("corners_wide", 12, None), "corners_tall12": ("corners_tall", 12, None),
    "wide12": ("wide", 12, _eight_interior("wide")), "tall12": ("tall", 12, _eight_interior("tall")),
}


def _case(case):
    name, bpc, pick = CASES[case]
    w, h, places, axis = S.sweep(name)
    return w, h, (pick(places) if pick else places), axis, bpc


_EXPECTED = {}   # computed once per case, never modified


def _freeze(e):
    for a in (e.exp64, e.exp32, e.deficit, e.bar, e.norm, e.rel32):
        a.setflags(write=False)
    return e


def _expected(case):
    if case not in _EXPECTED:
        w, h, places, axis, bpc = _case(case)
        _EXPECTED[case] = _freeze(S.Expected(w, h, places, axis, bpc))
    return _EXPECTED[case]


_RECORDS = {}    # GPU records of a case: the translation test reads what the sweep test measured


def _records(case):
    if case not in _RECORDS:
        w, h, places, _, bpc = _case(case)
        refs, diss = S.placement_clip(w, h, places, bpc)
        _RECORDS[case] = _run(w, h, refs, diss, bpc).reshape(len(places), 2, S.N_SLOT)
    return _RECORDS[case]


def _check_premises(e):
    """From the restatement alone: the bar means what it says."""
    if e.interior.any():
        r = e.rel32[e.interior]
        assert r.max() < S.SSF_REL32_MAX, ("f32 restatement too far from f64", S.SLOTS[int(r.max((0, 1)).argmax())], float(r.max()))
    assert not e.floor_used()[e.interior].any(), "an interior placement needs the 0.01 floor"


def _check_against_restatement(e, got, label):
    """got [n, 2, 20] against e.exp64 under e.bar (slots the restatement did not evaluate are NaN and not compared);
    prints the worst distance per slot and where."""
    run = np.isfinite(e.exp64)
    assert np.all(np.isfinite(got[run])), label
    diff = np.where(run, np.abs(got - e.exp64), 0.0)
    dist = diff / np.where(run, e.norm, 1.0)
    over = diff / np.where(run, e.bar, 1.0)
    print(f"\n{label}: worst |gpu - f64| / max(|deficit|, 0.01 |anchor's|) per slot (f32 restatement's own: "
          f"{np.nanmax(e.rel32):.1e})")
    for f in range(S.N_SLOT):
        if run[..., f].any():
            k, t = np.unravel_index(int(over[:, :, f].argmax()), over.shape[:2])
            print(f"  {S.SLOTS[f]:13s} {dist[k, t, f]:.2e} ({over[k, t, f]:.2f} of the bar, |d| {diff[k, t, f]:.1e}) at "
                  f"{e.places[k]} frame {t}")
    bad = np.argwhere(over > 1.0)
    msg = [f"{S.SLOTS[f]} at placement {e.places[k]} frame {t}: gpu {got[k, t, f]!r} f64 {e.exp64[k, t, f]!r} "
           f"distance {dist[k, t, f]:.2e} = {over[k, t, f]:.1f} x the bar" for k, t, f in bad[:8]]
    assert bad.size == 0, (label, len(bad), msg)


# ---- 1. flat frames ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bpc", [8, 10, 12])
@pytest.mark.parametrize("w,h", [S.WIDE, S.TALL, S.ODD_WIDE, S.ODD_TALL, S.UNION, S.BOX_TALL, S.BOX_WIDE, (161, 161)])
def test_flat_frames_are_one(w, h, bpc):
    """ref = dis = mid grey: every window is flat, the per-thread offsets make every moment exactly zero, and each map
    value is C * rcp(C) for three constants C -- within one f32 ulp of 1, so every mean and the product are."""
    flat = S.flat_frame(w, h, bpc)
    got = _run(w, h, [flat] * 3, [flat] * 3, bpc)
    print(f"\n{w}x{h} {bpc}-bit flat: value - 1 per slot " + " ".join(f"{v:.2e}" for v in (got[0] - 1.0)))
    assert np.array_equal(got[0].view(np.uint64), got[1].view(np.uint64)) and np.array_equal(got[0].view(np.uint64), got[2].view(np.uint64))
    bad = np.argwhere(~(np.abs(got - 1.0) <= S.ULP32))
    assert bad.size == 0, [(int(i), S.SLOTS[f], got[i, f]) for i, f in bad[:8]]


# ---- 2. placement sweeps against the restatement ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_placement_sweep(case):
    e = _expected(case)
    _check_premises(e)
    _check_against_restatement(e, _records(case), case)


# ---- 3. translation on the GPU, no restatement values compared ------------------------------------------------------------
@pytest.mark.parametrize("case", ["wide8", "tall8"])
def test_interior_placements_agree_on_the_gpu(case):
    """Every pair of interior placements differs by at most twice the bar (largest minus smallest value per slot)."""
    e = _expected(case)
    got = _records(case)
    inner = np.flatnonzero(e.interior)
    assert len(inner) >= 40
    g = got[inner]
    hi, lo = g.argmax(axis=0), g.argmin(axis=0)
    spread = (g.max(axis=0) - g.min(axis=0)) / (2.0 * e.bar[e.anchor])
    t, f = np.unravel_index(int(spread.argmax()), spread.shape)
    print(f"\n{case}: worst spread {spread.max():.2f} of twice the bar: {S.SLOTS[f]} frame {t}, placements "
          f"{e.places[inner[hi[t, f]]]} and {e.places[inner[lo[t, f]]]}")
    bad = [(S.SLOTS[f], int(t), e.places[inner[hi[t, f]]], e.places[inner[lo[t, f]]], float(spread[t, f]))
           for t, f in np.argwhere(spread > 1.0)]
    assert not bad, bad[:8]


# ---- 4. size cases --------------------------------------------------------------------------------------------------------------
# w % f = h % f = 1 where f >= 3: the last box then reaches f - f // 2 - 1 samples beyond the plane (1, 2, 2, 3 for f = 3, 5,
# 6, 7; with f = 2 only the first box is folded).  What these cases hold is the box sum and its indexing over the whole
# plane; the fold itself enters only the border windows through the outermost Gaussian tap (1e-3) and stays under REL_TOL
BOX_SIZES = {(515, 521): 2, (769, 646): 3, (1281, 1291): 5, (1543, 1537): 6, (1793, 1800): 7}
UNION_SIZES = [(w, h) for w in (193, 197, 202) for h in (161, 177)]
ODD_SIZES = [(161, 161), (193, 193), (2049, 161), (161, 2049)]


def _size_case(w, h, bpc, ms):
    """The centre placement (the anchor), one clipped by the bottom-right corner (8 columns and rows outside) and one in
    the top-left corner (where every box factor folds its first box)."""
    places = [((w - S.PATCH) // 2, (h - S.PATCH) // 2), (w - S.PATCH + 8, h - S.PATCH + 8), (0, 0)]
    key = ("size", w, h, bpc, ms)
    if key not in _EXPECTED:
        _EXPECTED[key] = _freeze(S.Expected(w, h, places, None, bpc, ms=ms))
    e = _EXPECTED[key]
    refs, diss = S.placement_clip(w, h, places, bpc)
    got = _run(w, h, refs, diss, bpc).reshape(len(places), 2, S.N_SLOT)
    assert not np.isnan(got).any()
    _check_against_restatement(e, got, f"{w}x{h} {bpc}-bit")


@pytest.mark.parametrize("bpc", [8, 10])
@pytest.mark.parametrize("w,h", list(BOX_SIZES))
def test_box_factors_with_folded_last_boxes(w, h, bpc):
    """float_ssim's f x f box decimation, f = 2, 3, 5, 6, 7, on sizes that are no multiple of f in either direction: the
    last box of every row and column is folded.  The float_ssim slots against the restatement (the MS-SSIM slots of frames
    this large are the sweeps' business)."""
    f = BOX_SIZES[(w, h)]
    assert R.decimation_factor(w, h) == f and w % f == 1 and h % f == 1
    _size_case(w, h, bpc, ms=False)


@pytest.mark.parametrize("bpc", [8, 10])
@pytest.mark.parametrize("w,h", UNION_SIZES + ODD_SIZES)
def test_union_tilings_and_odd_levels(w, h, bpc):
    """Widths 193, 197, 202 (a decimation-only tile column) with heights 161 (a decimation-only tile row) and 177 (none);
    161, 193 and 2049: odd at every pyramid level."""
    if (w, h) in UNION_SIZES:
        assert S.decimation_only(w, h) == (1, 1 if h == 161 else 0)
    else:
        assert all(a % 2 == 1 and b % 2 == 1 for a, b in R.ms_scale_sizes(w, h))
    _size_case(w, h, bpc, ms=True)


# ---- 5. the kernel variants agree ------------------------------------------------------------------------------------------------
def test_each_feature_alone_gives_the_bits_of_both():
    """float_ssim alone launches only the BOX variant of the map kernel, MS-SSIM alone only the fused-DOWN and the plain
    ones: neither may depend on the other having run (box factor 2, 8 bit, every fourth placement)."""
    w, h, places, _ = S.sweep("box2_wide")
    places = places[::4]
    refs, diss = S.placement_clip(w, h, places, 8)
    both = _run(w, h, refs, diss, 8)
    fs = _run(w, h, refs, diss, 8, FEAT_FLOAT_SSIM)
    ms = _run(w, h, refs, diss, 8, FEAT_MS_SSIM)
    assert not np.isnan(both).any() and np.isnan(fs[:, 4:]).all() and np.isnan(ms[:, :4]).all()
    assert np.array_equal(fs[:, :4].view(np.uint64), both[:, :4].view(np.uint64))
    assert np.array_equal(ms[:, 4:].view(np.uint64), both[:, 4:].view(np.uint64))
