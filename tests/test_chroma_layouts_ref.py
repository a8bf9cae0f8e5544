"""The premises of tests/test_gpu_chroma_layouts.py, without a GPU: on every case of the localized ciede2000 construction
(tests/chroma_layout_ref.py) the unchanged pixels give an exact 0, no changed pixel sits at the 180-degree hue jump, the
f32 evaluation of the restatement meets the GPU test's bound with 2x room, and two wrong kernels restated in numpy (the
last luma column reading the previous chroma column; the horizontal `break` dropped) miss it by more than 20x."""
import numpy as np
import pytest

from tests import chroma_layout_ref as L


def test_layouts_geometries_and_depths():
    assert len(L.LAYOUTS) == 9 and set(L.NEVER_RUN) < set(L.LAYOUTS) and len(L.NEVER_RUN) == 6
    for hs, vs in L.LAYOUTS:
        w, h = L.seam_size(hs, vs)
        cw, ch = L.chroma_size(w, h, hs, vs)
        assert cw > 2 * 64 and ch > 2 * 4                                   # more than two workgroup tiles each way
        # the last chroma column covers one luma pixel; the last chroma row one (shift 0, 1) or three (shift 2) luma rows
        assert w - ((cw - 1) << hs) == 1 and h - ((ch - 1) << vs) == (3 if vs == 2 else 1)
        assert L.depths(hs, vs) == ((8, 10, 12) if (hs, vs) in L.NEVER_RUN else (8, 10))
        assert len(L.cases(hs, vs)) == 11 * len(L.depths(hs, vs))
    assert [s - ((L.chroma_size(s, s, 2, 2)[0] - 1) << 2) for s in (19, 18)] == [3, 2]


def test_patch_pair_differs_only_under_the_patch():
    for (hs, vs) in L.LAYOUTS:
        for (w, h, bpc, origin) in L.cases(hs, vs):
            ref, dis, changed = L.patch_pair(w, h, bpc, hs, vs, origin)
            s, top = 1 << (bpc - 8), (1 << bpc) - 1
            x0, y0 = origin
            x1, y1 = min(x0 + L.PATCH, w), min(y0 + L.PATCH, h)
            assert ref[0].shape == (h, w) and ref[1].shape == ref[2].shape == L.chroma_size(w, h, hs, vs)[::-1]
            assert ref[0].min() >= 16 * s and ref[0].max() <= 235 * s and dis[0].max() <= top
            assert min(ref[1].min(), ref[2].min()) >= 64 * s and max(ref[1].max(), ref[2].max()) <= 191 * s
            inside = np.zeros((h, w), bool)
            inside[y0:y1, x0:x1] = True
            dy = dis[0].astype(np.int64) - ref[0]
            # 235 s + 20 s does not pass full scale: every patch pixel moves by at least 20 s
            assert (dy[inside] >= 20 * s).all() and (dy[inside] <= 59 * s).all() and (dy[~inside] == 0).all()
            du, dv = dis[1].astype(np.int64) - ref[1], dis[2].astype(np.int64) - ref[2]
            under = np.zeros(du.shape, bool)
            under[y0 >> vs:((y1 - 1) >> vs) + 1, x0 >> hs:((x1 - 1) >> hs) + 1] = True
            assert (du[under] >= 10 * s).all() and (du[under] <= 39 * s).all() and (du[~under] == 0).all()
            assert (dv[under] <= -10 * s).all() and (dv[under] >= -39 * s).all() and (dv[~under] == 0).all()
            assert changed[inside].all() and inside.sum() <= changed.sum() <= (L.PATCH + 3) ** 2


@pytest.mark.parametrize("hs,vs", L.LAYOUTS)
def test_ciede_patch_premises(hs, vs):
    worst32 = worst_hue = None
    least = {"last column": np.inf, "no break": np.inf}
    for (w, h, bpc, origin) in L.cases(hs, vs):
        ref, dis, changed = L.patch_pair(w, h, bpc, hs, vs, origin)
        de64 = L.patch_de(ref, dis, bpc, hs, vs)
        de32 = L.patch_de(ref, dis, bpc, hs, vs, np.float32)
        assert (de64[~changed] == 0).all() and (de32[~changed] == 0).all()
        assert (de64[changed] > 0).all()
        n, want = int(changed.sum()), float(de64.sum())
        tol = L.bound(n, want)
        hue = L.min_hue_distance(ref, dis, changed, bpc, hs, vs)
        assert hue > 1e-3, (w, h, bpc, origin, hue)                     # zero pixels excluded: none may be
        r32 = abs(float(de32.sum()) - want) / tol
        assert r32 <= 0.5, (w, h, bpc, origin, r32)
        px = np.abs(de32 - de64) / (1.0 + de64)
        assert px.max() <= L.PAIR_TOL / 2, (w, h, bpc, origin, px.max())
        worst32 = max(worst32 or 0.0, r32)
        worst_hue = min(worst_hue or np.inf, hue)
        if L.touches_last_column(w, origin):
            moved = abs(L.mutant_last_column_sum(ref, dis, bpc, hs, vs) - want) / tol
            assert moved > 20, ("last column", w, h, bpc, origin, moved)
            least["last column"] = min(least["last column"], moved)
            if L.no_break_pad(w, hs):
                moved = abs(L.mutant_no_break_sum(ref, dis, bpc, hs, vs) - want) / tol
                assert moved > 20, ("no break", w, h, bpc, origin, moved)
                least["no break"] = min(least["no break"], moved)
    print(f"\nshift ({hs},{vs}): f32 restatement at most {worst32:.3f} of the bound, hue at least {worst_hue:.3g} degrees "
          f"from 180, mutants move the sum by at least {least['last column']:.0f}x / {least['no break']:.0f}x the bound")
    assert np.isfinite(least["last column"]) and (hs == 0) == np.isinf(least["no break"])


def test_mutants_are_the_restatement_where_they_do_not_apply():
    """The mutants differ from the restatement only through the patch: away from the last column they return its sum."""
    hs, vs = 2, 1
    w, h = L.seam_size(hs, vs)
    ref, dis, _ = L.patch_pair(w, h, 10, hs, vs, (0, 0))
    want = float(L.patch_de(ref, dis, 10, hs, vs).sum())
    assert L.mutant_last_column_sum(ref, dis, 10, hs, vs) == want
    assert L.mutant_no_break_sum(ref, dis, 10, hs, vs) == want


def test_offset_pair_shapes_and_range():
    for (hs, vs) in L.LAYOUTS:
        for (w, h, bpc) in L.PSNR_SSIM_CASES:
            refs, diss = L.offset_pair(w, h, bpc, hs, vs, seed=1)
            s = 1 << (bpc - 8)
            for p, shp in enumerate(((h, w),) + (L.chroma_size(w, h, hs, vs)[::-1],) * 2):
                r, d = refs[0][p].astype(np.int64), diss[0][p].astype(np.int64)
                assert r.shape == d.shape == shp and refs[0][p].dtype == L.dtype_of(bpc)
                assert np.abs(r - d).max() <= 9 * s and (r != d).any()
    # over the layouts the chroma sizes reach every remainder mod 4 both ways (45 x 39 and 150 x 86 alone leave out a
    # height of 1 mod 4: 45 x 41 is there for it), and shift 2 at 19 x 19 is below one window
    rem = {(cw % 4, ch % 4) for (hs, vs) in L.LAYOUTS for (w, h, _) in L.PSNR_SSIM_CASES[1:]
           for (cw, ch) in [L.chroma_size(w, h, hs, vs)]}
    assert {r[0] for r in rem} == {0, 1, 2, 3} == {r[1] for r in rem}
    assert L.chroma_size(19, 19, 2, 2) == (5, 5)
