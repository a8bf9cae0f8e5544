"""cambi on the MI355X (csrc/cambi.hip, PQA_FEAT_CAMBI / PQA_FEAT_CAMBI_FULL_REF): the full path against the restatement
(tests/cambi_ref.py) over sizes, bit depths and content, bit-identical results across every way frames reach the kernels,
NaN rows of frames without spatial features, and no effect on the other outputs."""
import numpy as np
import pytest

from tests import cambi_ref as R

pytestmark = pytest.mark.gpu
REL, ABS = 1e-9, 1e-12     # c-values are bit-exact; only the order of the double pooling sums differs


def _ramp(w, h, bpc, levels, seed, dither=0.0, step=None):
    """A dark diagonal staircase of `levels` bands, `step` codes apart (banding-prone), optionally dithered by one code."""
    rng = np.random.default_rng(seed)
    top = (1 << bpc) - 1
    step = (1 if bpc == 8 else 2) if step is None else step
    lo = (16 if bpc == 8 else 64) + int(rng.integers(0, 8))
    yy, xx = np.mgrid[0:h, 0:w]
    t = (xx + 0.37 * yy) / (w + 0.37 * h)
    v = lo + np.floor(t * levels).astype(np.int64) * step
    if dither:
        v = v + (rng.random((h, w)) < dither) * rng.choice([-1, 1], (h, w))
    return np.clip(v, 0, top).astype(np.uint8 if bpc == 8 else np.uint16)


def _natural(w, h, bpc, seed):
    """The natural synthetic clip (reference, distorted), smoothed, squeezed into a few dark codes and requantised (8-bit: one
    code, 10-bit: two codes a step): natural shapes with the wide bands of a coarse encode, so the mask keeps them."""
    from scipy import ndimage
    from pqa2_amd import synth
    refs, diss = synth.make_clip(w, h, 1, bpc, chroma=False, t0=seed)
    out = []
    for y in (refs[0][0], diss[0][0]):
        y = y.astype(np.float64) / (1 << (bpc - 8))
        for _ in range(2):
            y = ndimage.uniform_filter(y, size=max(9, min(w, h) // 12), mode="nearest")
        lo, hi = np.percentile(y, 1), np.percentile(y, 99)
        y = 16 + (y - lo) / max(hi - lo, 1e-9) * max(6, min(w, h) // 8)
        step = 1 if bpc == 8 else 2
        y = np.round(y * (1 << (bpc - 8)) / step) * step
        out.append(np.clip(y, 0, (1 << bpc) - 1).astype(np.uint8 if bpc == 8 else np.uint16))
    return out[0], out[1]


def _run(w, h, bpc, refs, diss, features=None, **kw):
    from pqa2_amd import _native as N
    from pqa2_amd.engine import FeatureEngine
    features = (N.FEAT_CAMBI | N.FEAT_CAMBI_FULL_REF) if features is None else features
    with FeatureEngine(w, h, bit_depth=bpc, n_planes=1, features=features, **kw) as eng:
        for i in range(len(refs)):
            eng.submit(i, [refs[i]], [diss[i]])
        return eng.collect_ext(0, len(refs))


def _close(got, want):
    return abs(got - want) <= max(ABS, REL * abs(want))


# every case scores above 0 on both sides (asserted): the smallest sizes have r = 1 (W + H >= 186; below that r = 0 and
# every c-value is 0)
CASES = [(128, 64, 8, "ramp"), (128, 64, 8, "natural"), (128, 64, 10, "ramp_dither"), (161, 97, 10, "natural"),
         (200, 120, 10, "natural"), (352, 288, 8, "ramp_dither"), (352, 288, 10, "ramp"), (640, 360, 8, "natural"),
         (1280, 720, 10, "ramp_dither"), (1280, 720, 10, "natural"), (1920, 1080, 8, "ramp"), (3840, 2160, 8, "ramp")]


@pytest.mark.parametrize("w,h,bpc,kind", CASES)
def test_full_path_matches_the_restatement(w, h, bpc, kind):
    if kind == "natural":
        r, d = _natural(w, h, bpc, seed=w + bpc)
    else:
        dith = 0.05 if kind == "ramp_dither" else 0.0
        r = _ramp(w, h, bpc, 24, seed=w, dither=dith)
        d = _ramp(w, h, bpc, 9, seed=w + 1, dither=dith)
    _, ext = _run(w, h, bpc, [r], [d])
    want_d, want_r = R.cambi(d, bpc), R.cambi(r, bpc)
    assert want_d > 0 and want_r > 0, "the case must exercise the path"
    print(f"\n{w}x{h} {bpc}-bit {kind}: cambi {ext[0, 22]!r} (restatement {want_d!r}), source {ext[0, 23]!r} ({want_r!r})")
    assert _close(ext[0, 22], want_d) and _close(ext[0, 23], want_r)
    assert np.isnan(ext[0, :22]).all()


def _cmap(y, bpc):
    """(per-scale c-value maps, score) of one luma plane from the kernels (pqa_debug_cambi_cmap)."""
    import ctypes as C
    from pqa2_amd import _native as N
    lib = N.load()
    h, w = y.shape
    y = np.ascontiguousarray(y, np.uint8 if bpc == 8 else np.uint16)
    sizes = R.scale_sizes(w, h)
    total = sum(a * b for a, b in sizes)
    out = np.full(total, np.nan, np.float32)
    score = C.c_double(np.nan)
    assert lib.pqa_debug_cambi_cmap(y.ctypes.data, y.strides[0], w, h, bpc, out.ctypes.data, total, C.byref(score)) == N.PQA_OK
    maps, o = [], 0
    for sw, sh in sizes:
        maps.append(out[o:o + sw * sh].reshape(sh, sw))
        o += sw * sh
    return maps, score.value


# sizes across strip (64 columns) and segment (32 .. 8r rows) boundaries, windows r = 1 .. 10
CMAP_CASES = [(200, 120, 8, "ramp_dither"), (200, 120, 10, "natural"), (352, 288, 10, "ramp_dither"),
              (1000, 300, 8, "natural"), (1000, 300, 10, "ramp"), (1280, 720, 8, "ramp_dither")]


@pytest.mark.parametrize("w,h,bpc,kind", CMAP_CASES)
def test_c_value_maps_equal_the_restatement_bit_for_bit(w, h, bpc, kind):
    """Every c-value of every scale, as bits: the integer counts, the f32 conversion and the IEEE f32 division."""
    if kind == "natural":
        y = _natural(w, h, bpc, seed=w + 3)[1]
    else:
        y = _ramp(w, h, bpc, 11, seed=w, dither=0.05 if kind == "ramp_dither" else 0.0)
    maps, score = _cmap(y, bpc)
    want_score, _, want_maps = R.cambi_detail(y, bpc)
    assert want_score > 0
    for s, (got, want) in enumerate(zip(maps, want_maps)):
        assert got.shape == want.shape
        bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, (s, bad.size, got.ravel()[bad[:4]], want.ravel()[bad[:4]])
        assert (got > 0).any() or s > 2, s   # the large scales are not trivially zero
    assert _close(score, want_score)


def test_larger_steps_score_higher_on_the_gpu():
    """The same bands one code apart and four codes apart (10 bit): the larger contrast weight wins."""
    w, h, bpc = 640, 360, 10
    fine, coarse = _ramp(w, h, bpc, 12, 1, step=1), _ramp(w, h, bpc, 12, 1, step=4)
    _, ext = _run(w, h, bpc, [fine], [coarse])
    assert ext[0, 23] > 0 and ext[0, 22] > ext[0, 23]
    assert _close(ext[0, 22], R.cambi(coarse, bpc)) and _close(ext[0, 23], R.cambi(fine, bpc))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("bpc", [8, 10])
def test_bit_identical_across_batches_submit_paths_and_alignment(bpc):
    import torch
    from pqa2_amd import _native as N
    from pqa2_amd.engine import FeatureEngine
    w, h, n = 352, 288, 7
    refs = [_ramp(w, h, bpc, 10 + i, seed=40 + i, dither=0.02 * (i % 2)) for i in range(n)]
    diss = [_ramp(w, h, bpc, 6 + i, seed=50 + i) for i in range(n)]
    feats = N.FEAT_VMAF | N.FEAT_CAMBI | N.FEAT_CAMBI_FULL_REF
    base = None
    for mb in (1, 3, 0):
        _, ext = _run(w, h, bpc, refs, diss, features=feats, max_batch=mb)
        if base is None:
            base = ext
        assert np.array_equal(_bits(ext[:, 22:24]), _bits(base[:, 22:24])), f"max_batch {mb}"
    assert not np.isnan(base[:, 22:24]).any() and (base[:, 22] > 0).all()
    # pqa_submit with three planes (luma only feeds cambi)
    cw, ch = w // 2, h // 2
    with FeatureEngine(w, h, bit_depth=bpc, n_planes=3, features=feats | N.FEAT_PSNR, max_batch=2) as eng:
        for i in range(n):
            z = np.zeros((ch, cw), refs[i].dtype)
            eng.submit(i, [refs[i], z, z], [diss[i], z, z])
        _, ext = eng.collect_ext(0, n)
    assert np.array_equal(_bits(ext[:, 22:24]), _bits(base[:, 22:24])), "three planes"
    es = 1 if bpc == 8 else 2
    dt = np.uint8 if bpc == 8 else np.uint16
    for off, pad in ((0, 0), (1, 3), (7, 13)):
        ptrs, keep = ([], []), []
        pitch = w + pad
        for side, src in enumerate((refs, diss)):
            buf = np.full(off + n * h * pitch, 0xA5, dt)
            for i in range(n):
                buf[off + i * h * pitch: off + (i + 1) * h * pitch].reshape(h, pitch)[:, :w] = src[i]
            t = torch.from_numpy(buf.view(np.uint8)).cuda()
            keep.append(t)
            ptrs[side].append(t.data_ptr() + off * es)
        torch.cuda.synchronize()
        with FeatureEngine(w, h, bit_depth=bpc, n_planes=1, features=feats, max_batch=3) as eng:
            eng.submit_resident(0, n, ptrs[0], ptrs[1], [pitch * es], [h * pitch * es])
            _, ext = eng.collect_ext(0, n)
        assert np.array_equal(_bits(ext[:, 22:24]), _bits(base[:, 22:24])), f"resident offset {off} pad {pad}"
    # decoder surfaces: NV12 (8-bit) / P010 (10-bit), samples in the high bits
    lp, cp = w + 5, w + 9
    sdt = np.uint8 if bpc == 8 else np.uint16
    shift = 0 if bpc == 8 else 16 - bpc
    L = np.zeros((2, n, h, lp), sdt)
    CH = np.zeros((2, n, h // 2, cp), sdt)
    for i in range(n):
        for side, src in enumerate((refs, diss)):
            L[side, i, :, :w] = src[i].astype(sdt) << shift
    tl, tc = torch.from_numpy(L.view(np.uint8)).cuda(), torch.from_numpy(CH.view(np.uint8)).cuda()
    torch.cuda.synchronize()
    fmt = N.SURFACE_NV12 if bpc == 8 else N.SURFACE_P01X
    lpb, cpb = lp * es, cp * es
    clip = [FeatureEngine.surface_clip(fmt, tl[s].data_ptr(), lpb, h * lpb, tc[s].data_ptr(), cpb, (h // 2) * cpb)
            for s in (0, 1)]
    with FeatureEngine(w, h, bit_depth=bpc, n_planes=1, features=feats, max_batch=2) as eng:
        eng.submit_surfaces(0, n, clip[0], clip[1])
        _, ext = eng.collect_ext(0, n)
    assert np.array_equal(_bits(ext[:, 22:24]), _bits(base[:, 22:24])), "submit_surfaces"


def test_no_effect_on_the_other_outputs():
    from pqa2_amd import _native as N
    from pqa2_amd import synth
    w, h, n, bpc = 352, 288, 5, 10
    refs, diss = synth.make_clip(w, h, n, bpc, chroma=True, t0=60)
    ext_feats = N.FEAT_FLOAT_SSIM | N.FEAT_MS_SSIM | N.FEAT_CIEDE
    from pqa2_amd.engine import FeatureEngine

    def run(features):
        with FeatureEngine(w, h, bit_depth=bpc, n_planes=3, features=features, max_batch=2) as eng:
            for i in range(n):
                eng.submit(i, refs[i], diss[i])
            return eng.collect_ext(0, n)
    plain = run(N.FEAT_ALL | ext_feats)
    both = run(N.FEAT_ALL | ext_feats | N.FEAT_CAMBI)
    only = run(N.FEAT_CAMBI)
    assert np.array_equal(_bits(plain[0]), _bits(both[0]))                     # the 24-double records
    assert np.array_equal(_bits(plain[1][:, :22]), _bits(both[1][:, :22]))     # SSIM family and ciede slots
    assert np.isnan(plain[1][:, 22:]).all()
    assert not np.isnan(both[1][:, 22]).any() and np.isnan(both[1][:, 23]).all()   # slot 23 NaN without FULL_REF
    assert np.array_equal(_bits(only[1][:, 22]), _bits(both[1][:, 22]))
    assert np.isnan(only[1][:, :22]).all()
    vmaf_only = run(N.FEAT_ALL)
    assert np.array_equal(_bits(vmaf_only[0]), _bits(both[0]))


def test_n_subsample_three():
    from pqa2_amd import _native as N
    w, h, n, bpc = 352, 288, 7, 8
    refs = [_ramp(w, h, bpc, 20, seed=80 + i) for i in range(n)]
    diss = [_ramp(w, h, bpc, 7, seed=90 + i) for i in range(n)]
    _, ext = _run(w, h, bpc, refs, diss, features=N.FEAT_VMAF | N.FEAT_CAMBI, n_subsample=3, max_batch=4)
    _, every = _run(w, h, bpc, refs, diss, features=N.FEAT_VMAF | N.FEAT_CAMBI, max_batch=4)
    for i in range(n):
        if i % 3:
            assert np.isnan(ext[i]).all(), i
        else:
            assert _close(ext[i, 22], R.cambi(diss[i], bpc)) and np.isnan(ext[i, 23]), i
            assert _bits(ext[i, 22:23]) == _bits(every[i, 22:23]), i   # the same bits as with every frame scored


def test_window_wider_than_the_frame():
    """16384 x 16: r = 88, so every window spans the frame's whole height and 177 columns."""
    w, h, bpc = 16384, 16, 8
    r_img = _ramp(w, h, bpc, 40, seed=5)
    d_img = _ramp(w, h, bpc, 11, seed=6)
    _, ext = _run(w, h, bpc, [r_img], [d_img])
    assert _close(ext[0, 22], R.cambi(d_img, bpc)) and _close(ext[0, 23], R.cambi(r_img, bpc))
