"""The three-plane kernels on all nine chroma layouts pqa_create accepts (chroma_hshift, chroma_vshift in 0..2), on the
MI355X.  Inputs and premises: tests/chroma_layout_ref.py and tests/test_chroma_layouts_ref.py.

  * ciede2000 (csrc/ciede.hip), localized: frame pairs that differ in one 8 x 8 luma patch, so slot 21 * w * h is the
    patch's own dE00 sum, against the f64 restatement -- at tile seams, picture corners and patches clipped by the
    picture's end, where a frame mean would hide a wrong pixel.  Runs all 18 ciede_kernel<T, HS, VS> instantiations.
  * ciede2000 across submit paths, pitches and batch sizes on two shift-2 layouts.
  * FFmpeg PSNR / SSIM (csrc/psnr_ssim.hip, finalize.hip): chroma planes below one SSIM window, chroma sizes of every
    remainder mod 4, and the same bits whether the SSE comes from the SSE kernel alone or is split between the SSIM
    kernel and the two remainder strips.
xpsnr, psnr_hvs and integrity on the mixed layouts are in their own files' parametrisations."""
import numpy as np
import pytest

from tests import chroma_layout_ref as L
from tests import ciede_ref as R

pytestmark = pytest.mark.gpu
SCORE_ABS = 2e-4                      # tests/test_gpu_ciede.py: slot 20 against the restatement's score


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _ciede(w, h, bpc, hs, vs, refs, diss, **kw):
    from pqa2_amd import _native as N
    from pqa2_amd.engine import FeatureEngine
    with FeatureEngine(w, h, bit_depth=bpc, n_planes=3, chroma_shift=(hs, vs), features=N.FEAT_CIEDE, **kw) as eng:
        for i in range(len(refs)):
            eng.submit(i, refs[i], diss[i])
        return eng.collect_ext(0, len(refs))[1]


@pytest.mark.parametrize("hs,vs", L.LAYOUTS)
def test_ciede_patch_sum_matches_the_restatement(hs, vs):
    """|slot 21 * w * h - f64 patch sum| <= 2e-5 * (changed pixels + sum) on every case, slot 20 within 2e-4 of the
    restatement's score.  Worst error / bound measured on the MI355X, per layout (hs, vs): (0,0) 0.029, (0,1) 0.018,
    (0,2) 0.014, (1,0) 0.027, (1,1) 0.019, (1,2) 0.043, (2,0) 0.015, (2,1) 0.017, (2,2) 0.056 -- the size of the numpy
    f32 restatement's own distance (at most 0.050 of the bound, tests/test_chroma_layouts_ref.py); the two wrong kernels
    restated there miss the bound by 36x or more."""
    worst, where = 0.0, None
    for (w, h, origins) in L.geometries(hs, vs):
        for bpc in L.depths(hs, vs):
            pairs = [L.patch_pair(w, h, bpc, hs, vs, o) for o in origins]
            ext = _ciede(w, h, bpc, hs, vs, [p[0] for p in pairs], [p[1] for p in pairs], max_batch=3)
            for i, (ref, dis, changed) in enumerate(pairs):
                assert L.min_hue_distance(ref, dis, changed, bpc, hs, vs) > 1e-3          # no pixel is excluded
                want = float(L.patch_de(ref, dis, bpc, hs, vs).sum())
                got = ext[i, 21] * w * h
                ratio = abs(got - want) / L.bound(int(changed.sum()), want)
                if ratio > worst:
                    worst, where = ratio, (w, h, bpc, origins[i], got, want)
                assert ratio <= 1.0, (w, h, bpc, origins[i], got, want, ratio)
                assert abs(ext[i, 20] - R.score(want / (w * h))) <= SCORE_ABS, (w, h, bpc, origins[i])
                assert np.isnan(ext[i, :20]).all() and np.isnan(ext[i, 22:]).all()
    print(f"\nciede shift ({hs},{vs}): worst error / bound {worst:.3f} at {where}")


@pytest.mark.parametrize("hs,vs", [(2, 2), (0, 2)])
@pytest.mark.parametrize("bpc", [8, 10])
def test_ciede_bit_identical_across_submit_paths_and_batches(hs, vs, bpc):
    import torch
    from pqa2_amd import _native as N
    from pqa2_amd.engine import FeatureEngine
    w, h, n = 261, 35, 4
    refs, diss = L.offset_pair(w, h, bpc, hs, vs, seed=7, n=n)
    base = _ciede(w, h, bpc, hs, vs, refs, diss, max_batch=1)
    assert np.isfinite(base[:, 21]).all() and (base[:, 21] > 0).all()
    assert np.array_equal(_bits(_ciede(w, h, bpc, hs, vs, refs, diss, max_batch=3)[:, 20:22]), _bits(base[:, 20:22]))
    # device-resident planes: a row pitch of plane width + 3 samples, the base one sample into the allocation
    es, dt = (1, np.uint8) if bpc == 8 else (2, np.uint16)
    cw, ch = L.chroma_size(w, h, hs, vs)
    ptrs, keep, rps, fps = ([], []), [], [], []
    for p, (pw, ph) in enumerate(((w, h), (cw, ch), (cw, ch))):
        pitch = pw + 3
        rps.append(pitch * es)
        fps.append(ph * pitch * es)
        for side, src in enumerate((refs, diss)):
            buf = np.full(1 + n * ph * pitch, 0xA5, dt)
            for i in range(n):
                buf[1 + i * ph * pitch: 1 + (i + 1) * ph * pitch].reshape(ph, pitch)[:, :pw] = src[i][p]
            t = torch.from_numpy(buf.view(np.uint8)).cuda()
            keep.append(t)
            ptrs[side].append(t.data_ptr() + es)
    torch.cuda.synchronize()
    for mb in (1, 3):
        with FeatureEngine(w, h, bit_depth=bpc, n_planes=3, chroma_shift=(hs, vs), features=N.FEAT_CIEDE,
                           max_batch=mb) as eng:
            eng.submit_resident(0, n, ptrs[0], ptrs[1], rps, fps)
            ext = eng.collect_ext(0, n)[1]
        assert np.array_equal(_bits(ext[:, 20:22]), _bits(base[:, 20:22])), f"resident, max_batch {mb}"


# ---- FFmpeg PSNR / SSIM -----------------------------------------------------------------------------------------------
def _record(w, h, bpc, hs, vs, ref, dis, features):
    from pqa2_amd.engine import FeatureEngine
    with FeatureEngine(w, h, bit_depth=bpc, n_planes=3, chroma_shift=(hs, vs), features=features) as eng:
        eng.submit(0, ref, dis)
        return eng.collect(0, 1)


@pytest.mark.parametrize("hs,vs", L.LAYOUTS)
@pytest.mark.parametrize("w,h,bpc", L.PSNR_SSIM_CASES)
def test_psnr_ssim_on_every_layout_and_feature_mask(oracle32, w, h, bpc, hs, vs):
    from pqa2_amd import _native as N
    from pqa2_amd.engine import sse_from_records
    refs, diss = L.offset_pair(w, h, bpc, hs, vs, seed=5)
    ref, dis = refs[0], diss[0]
    psnr = _record(w, h, bpc, hs, vs, ref, dis, N.FEAT_PSNR)
    ssim = _record(w, h, bpc, hs, vs, ref, dis, N.FEAT_SSIM)
    both = _record(w, h, bpc, hs, vs, ref, dis, N.FEAT_PSNR | N.FEAT_SSIM)
    for p in range(3):
        ph, pw = ref[p].shape
        want_sse = oracle32.sse_plane(dis[p], ref[p], bpc)
        assert want_sse > 0
        assert int(sse_from_records(psnr)[0, p]) == want_sse, ("PSNR", p)
        assert int(sse_from_records(both)[0, p]) == want_sse, ("PSNR|SSIM", p)
        want_ssim = oracle32.ssim_plane(dis[p], ref[p], bpc)
        if pw < 8 or ph < 8:      # below one 8 x 8 window: no SSIM launch, the slot is 0.0 (include/pqa_vmaf.h)
            assert want_ssim == 0.0
            assert ssim[0, 17 + p] == 0.0 and both[0, 17 + p] == 0.0, p
        else:
            assert 0.0 < want_ssim < 1.0
            assert abs(ssim[0, 17 + p] - want_ssim) < 1e-9, ("SSIM", p, ssim[0, 17 + p], want_ssim)
            assert abs(both[0, 17 + p] - want_ssim) < 1e-9, ("PSNR|SSIM", p, both[0, 17 + p], want_ssim)
    assert np.array_equal(_bits(psnr[:, N.REC_SSE:N.REC_SSE + 3]), _bits(both[:, N.REC_SSE:N.REC_SSE + 3]))
    assert np.array_equal(_bits(ssim[:, 17:20]), _bits(both[:, 17:20]))
