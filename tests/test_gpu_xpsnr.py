"""xpsnr on the MI355X (csrc/xpsnr.hip, PQA_FEAT_XPSNR / _HFR): the real kernels' block sums and WSSE against the
restatement (tests/xpsnr_ref.py) bit for bit, the full path over geometries, bit depths, chroma formats, contents and both
temporal orders, bit-identical ext3 rows across every way frames reach the kernels, the chain across batches, resets and
shards, and no effect on the other outputs."""
import ctypes as C

import numpy as np
import pytest

from tests import xpsnr_ref as R

pytestmark = pytest.mark.gpu
DB_ABS = 1e-12     # the dB values against the restatement (the WSSE values are equal integers)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _plane(w, h, bpc, seed, kind="textured"):
    rng = np.random.default_rng(seed)
    top = (1 << bpc) - 1
    if kind == "flat":
        return np.full((h, w), top // 3, np.int64)
    if kind == "dark":
        return rng.integers(0, 3, (h, w))
    yy, xx = np.mgrid[0:h, 0:w]
    r = (0.5 + 0.35 * np.sin(xx * 0.09 + seed) * np.cos(yy * 0.06 - seed)) * top + rng.normal(0, top * 0.05, (h, w))
    r[:, w // 2: w // 2 + 3] = top
    return np.clip(np.rint(r), 0, top).astype(np.int64)


def _frames(w, h, bpc, hs, vs, n, seed, planes=3, kind="textured"):
    """n reference frames (a moving texture) and distorted copies (noise)."""
    dt = np.uint8 if bpc == 8 else np.uint16
    top = (1 << bpc) - 1
    rng = np.random.default_rng(seed + 1)
    wc, hc = (w + (1 << hs) - 1) >> hs, (h + (1 << vs) - 1) >> vs
    base = [_plane(w, h, bpc, seed, kind), _plane(wc, hc, bpc, seed + 7, kind), _plane(wc, hc, bpc, seed + 9, kind)]
    refs, diss = [], []
    for i in range(n):
        rf = [np.roll(p, i * (k + 1), axis=1) for k, p in enumerate(base[:planes])]
        df = [np.clip(p + rng.integers(-3 * (1 << (bpc - 8)), 3 * (1 << (bpc - 8)) + 1, p.shape), 0, top) for p in rf]
        refs.append([p.astype(dt) for p in rf])
        diss.append([p.astype(dt) for p in df])
    return refs, diss


def _run(w, h, bpc, hs, vs, refs, diss, features=None, hfr=False, max_batch=0, n_subsample=1, n_planes=3):
    from pqa2_amd import _native as N
    from pqa2_amd.engine import FeatureEngine
    feats = features if features is not None else N.FEAT_XPSNR | (N.FEAT_XPSNR_HFR if hfr else 0)
    with FeatureEngine(w, h, bit_depth=bpc, n_planes=n_planes, chroma_shift=(hs, vs), features=feats,
                       max_batch=max_batch, n_subsample=n_subsample) as eng:
        for i in range(len(refs)):
            eng.submit(i, refs[i][:n_planes], diss[i][:n_planes])
        return eng.collect_ext3(0, len(refs))


def _hook(ref, m1, m2, dis, bpc, hfr):
    from pqa2_amd import _native as N
    lib = N.load()
    h, w = ref.shape
    b = R.block_size(w, h)
    nb = 1 if b < 4 else ((w + b - 1) // b) * ((h + b - 1) // b)
    out = np.zeros((nb, 3), np.uint64)
    wsse = C.c_double()
    ptr = lambda a: None if a is None else np.ascontiguousarray(a).ctypes.data   # noqa: E731
    keep = [np.ascontiguousarray(a) for a in (ref, m1, m2, dis) if a is not None]
    rc = lib.pqa_debug_xpsnr_blocks(ptr(ref), ptr(m1), ptr(m2), ptr(dis), w * ref.itemsize, w, h, bpc, int(hfr),
                                    out.ctypes.data, C.byref(wsse))
    del keep
    assert rc == 0, lib.pqa_last_error(None)
    return out, wsse.value


@pytest.mark.parametrize("w,h", [(16, 16), (44, 44), (45, 45), (352, 288), (640, 480), (642, 480), (1920, 1080),
                                 (2048, 1152), (2050, 1152), (2560, 1440), (3840, 2160)])
@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_hook_blocks_equal_the_restatement(w, h, bpc):
    refs, diss = _frames(w, h, bpc, 1, 1, 3, seed=w + bpc, planes=1)
    for hfr in (False, True):
        for (m1, m2) in ((None, None), (refs[1][0], None), (refs[1][0], refs[0][0])):
            o, r = refs[2][0], diss[2][0]
            got, wsse = _hook(o, m1, m2, r, bpc, hfr)
            want = R.blocks(o, m1, m2, r, hfr)
            assert np.array_equal(got, np.array([[b["sse"], b["sa"], b["ta"]] for b in want], np.uint64)), (hfr, m1 is None)
            ww, db, _, _ = R.frame([o], [r], m1, m2, bpc, hfr)
            assert wsse == ww[0]


@pytest.mark.parametrize("kind", ["flat", "dark"])
def test_hook_flat_and_dark_content(kind):
    for (w, h, bpc) in ((640, 480, 8), (1920, 1080, 10), (2560, 1440, 12)):
        refs, diss = _frames(w, h, bpc, 1, 1, 2, seed=3, planes=1, kind=kind)
        got, wsse = _hook(refs[1][0], refs[0][0], None, diss[1][0], bpc, False)
        want = R.blocks(refs[1][0], refs[0][0], None, diss[1][0], False)
        assert np.array_equal(got, np.array([[b["sse"], b["sa"], b["ta"]] for b in want], np.uint64))
        assert wsse == R.frame([refs[1][0]], [diss[1][0]], refs[0][0], None, bpc)[0][0]


# the mixed layouts (the two shifts differ, so the chroma blocks are not square: cbx != cby); pqa_create's block-grid
# check accepts every one of them at these sizes
MIXED = [(w, h, hs, vs, bpc, 3) for (hs, vs) in [(2, 0), (0, 2), (1, 2), (2, 1), (0, 1)] for (w, h) in [(352, 288), (45, 45)]
         for bpc in (8, 10)]


@pytest.mark.parametrize("w,h,hs,vs,bpc,planes", [(352, 288, 1, 1, 8, 3), (640, 480, 1, 0, 10, 3), (642, 480, 0, 0, 12, 3),
                                                  (1920, 1080, 1, 1, 10, 3), (2560, 1440, 1, 1, 8, 3),
                                                  (3840, 2160, 1, 1, 8, 3), (45, 45, 1, 1, 8, 3), (44, 44, 1, 1, 8, 3),
                                                  (1280, 720, 1, 1, 8, 1), (2050, 1152, 2, 2, 10, 3)] + MIXED)
@pytest.mark.parametrize("hfr", [False, True])
def test_full_path_equals_the_restatement(w, h, hs, vs, bpc, planes, hfr):
    refs, diss = _frames(w, h, bpc, hs, vs, 4, seed=11, planes=planes)
    _, _, _, ext3 = _run(w, h, bpc, hs, vs, refs, diss, hfr=hfr, n_planes=planes)
    wsse, db = R.clip(refs, diss, bpc, hfr)
    assert np.array_equal(ext3[:, 3:3 + planes], wsse)
    assert np.abs(ext3[:, :planes] - db).max() < DB_ABS
    assert np.isnan(ext3[:, 3 + planes:]).all() and np.isnan(ext3[:, planes:3]).all()


@pytest.mark.parametrize("bpc", [8, 10])
@pytest.mark.parametrize("hfr", [False, True])
def test_bit_identical_across_batches_submit_paths_and_alignment(bpc, hfr):
    import torch
    from pqa2_amd import _native as N
    from pqa2_amd.engine import FeatureEngine
    w, h, n = 352, 288, 7
    refs, diss = _frames(w, h, bpc, 1, 1, n, seed=40)
    feats = N.FEAT_VMAF | N.FEAT_XPSNR | (N.FEAT_XPSNR_HFR if hfr else 0)
    base = None
    for mb in (1, 3, 0):
        ext3 = _run(w, h, bpc, 1, 1, refs, diss, features=feats, max_batch=mb)[3]
        if base is None:
            base = ext3
        assert np.array_equal(_bits(ext3), _bits(base)), f"max_batch {mb}"
    assert np.array_equal(base[:, 3:6], R.clip(refs, diss, bpc, hfr)[0])
    ext3 = _run(w, h, bpc, 1, 1, refs, diss, features=feats, n_subsample=3)[3]
    assert np.array_equal(_bits(ext3), _bits(base)), "n_subsample 3"
    # files: fd-run submits
    import os
    import tempfile
    es = 1 if bpc == 8 else 2
    dt = np.uint8 if bpc == 8 else np.uint16
    with tempfile.TemporaryDirectory() as d:
        paths = []
        for side, src in enumerate((refs, diss)):
            pth = os.path.join(d, f"{side}.yuv")
            with open(pth, "wb") as f:
                for fr in src:
                    for p in fr:
                        f.write(np.ascontiguousarray(p).tobytes())
            paths.append(pth)
        fsz = (w * h + 2 * (w // 2) * (h // 2)) * es
        offs = [0, w * h * es, w * h * es + (w // 2) * (h // 2) * es]
        fds = [os.open(p, os.O_RDONLY) for p in paths]
        try:
            with FeatureEngine(w, h, bit_depth=bpc, n_planes=3, features=feats, max_batch=3) as eng:
                eng.submit_file_run(0, 4, fds[0], offs, fsz, fds[1], offs, fsz)
                eng.submit_file_run(4, n - 4, fds[0], [o + 4 * fsz for o in offs], fsz, fds[1],
                                    [o + 4 * fsz for o in offs], fsz)
                ext3 = eng.collect_ext3(0, n)[3]
        finally:
            for fd in fds:
                os.close(fd)
    assert np.array_equal(_bits(ext3), _bits(base)), "fd run"
    sizes = [(w, h), (w // 2, h // 2), (w // 2, h // 2)]
    for off, pad in ((0, 0), (1, 3), (7, 13)):      # device-resident planes at odd pitches and base offsets (elements)
        ptrs, keep, rps, fps = ([], []), [], [], []
        for p, (pw, ph) in enumerate(sizes):
            pitch = pw + pad + p
            rps.append(pitch * es)
            fps.append(ph * pitch * es)
            for side, src in enumerate((refs, diss)):
                buf = np.full(off + n * ph * pitch, 0xA5, dt)
                for i in range(n):
                    buf[off + i * ph * pitch: off + (i + 1) * ph * pitch].reshape(ph, pitch)[:, :pw] = src[i][p]
                t = torch.from_numpy(buf.view(np.uint8)).cuda()
                keep.append(t)
                ptrs[side].append(t.data_ptr() + off * es)
        torch.cuda.synchronize()
        with FeatureEngine(w, h, bit_depth=bpc, n_planes=3, features=feats, max_batch=3) as eng:
            eng.submit_resident(0, n, ptrs[0], ptrs[1], rps, fps)
            ext3 = eng.collect_ext3(0, n)[3]
        assert np.array_equal(_bits(ext3), _bits(base)), f"resident offset {off} pad {pad}"
        # the same run in two calls, the second with its halo (frame 2) given as prev_ref: frame 1 is kept
        with FeatureEngine(w, h, bit_depth=bpc, n_planes=3, features=feats, max_batch=2) as eng:
            eng.submit_resident(0, 3, ptrs[0], ptrs[1], rps, fps)
            eng.submit_resident(3, n - 3, [q + 3 * fps[p] for p, q in enumerate(ptrs[0])],
                                [q + 3 * fps[p] for p, q in enumerate(ptrs[1])], rps, fps,
                                ptrs[0][0] + 2 * fps[0], rps[0])
            ext3 = eng.collect_ext3(0, n)[3]
        assert np.array_equal(_bits(ext3), _bits(base)), f"resident split, offset {off}"
    lp, cp = w + 5, w + 9
    sdt = np.uint8 if bpc == 8 else np.uint16
    shift = 0 if bpc == 8 else 16 - bpc
    L = np.zeros((2, n, h, lp), sdt)
    CH = np.zeros((2, n, h // 2, cp), sdt)
    for i in range(n):
        for side, src in enumerate((refs, diss)):
            L[side, i, :, :w] = src[i][0].astype(sdt) << shift
            CH[side, i, :, 0:w:2] = src[i][1].astype(sdt) << shift
            CH[side, i, :, 1:w:2] = src[i][2].astype(sdt) << shift
    tl, tc = torch.from_numpy(L.view(np.uint8)).cuda(), torch.from_numpy(CH.view(np.uint8)).cuda()
    torch.cuda.synchronize()
    fmt = N.SURFACE_NV12 if bpc == 8 else N.SURFACE_P01X
    lpb, cpb = lp * es, cp * es
    clip = [FeatureEngine.surface_clip(fmt, tl[s].data_ptr(), lpb, h * lpb, tc[s].data_ptr(), cpb, (h // 2) * cpb)
            for s in (0, 1)]
    with FeatureEngine(w, h, bit_depth=bpc, n_planes=3, features=feats, max_batch=2) as eng:
        eng.submit_surfaces(0, n, clip[0], clip[1])
        ext3 = eng.collect_ext3(0, n)[3]
    assert np.array_equal(_bits(ext3), _bits(base)), "submit_surfaces"
    # a surface run that starts at frame 1 on a fresh context with frame 0 as prev_ref: frame -1 is then zero
    sub = [FeatureEngine.surface_clip(fmt, tl[s].data_ptr() + h * lpb, lpb, h * lpb, tc[s].data_ptr() + (h // 2) * cpb,
                                      cpb, (h // 2) * cpb) for s in (0, 1)]
    with FeatureEngine(w, h, bit_depth=bpc, n_planes=3, features=feats, max_batch=2) as eng:
        eng.submit_surfaces(1, n - 1, sub[0], sub[1], clip[0])
        ext3 = eng.collect_ext3(1, n - 1)[3]
    want = R.clip(refs[1:], diss[1:], bpc, hfr, (refs[0][0], None))[0]
    assert np.array_equal(ext3[:, 3:6], want), "surfaces with prev_ref"


@pytest.mark.parametrize("hfr", [False, True])
def test_reset_and_chain_restart_give_zero_history(hfr):
    from pqa2_amd import _native as N
    from pqa2_amd.engine import FeatureEngine
    w, h, bpc, n = 640, 480, 8, 4
    refs, diss = _frames(w, h, bpc, 1, 1, n, seed=21)
    feats = N.FEAT_XPSNR | (N.FEAT_XPSNR_HFR if hfr else 0)
    base = _run(w, h, bpc, 1, 1, refs, diss, features=feats)[3]
    with FeatureEngine(w, h, bit_depth=bpc, n_planes=3, features=feats, max_batch=2) as eng:
        for i in range(n):
            eng.submit(i, refs[i], diss[i])
        eng.collect_ext3(0, n)
        eng.reset()
        eng.submit(0, refs[2], diss[2])      # frame 2's content as a chain start
        first = eng.collect_ext3(0, 1)[3]
        eng.submit(1, refs[3], diss[3])
        eng.set_ref_history([])              # n_prev = 0: a chain start again
        eng.submit(2, refs[2], diss[2])
        again = eng.collect_ext3(1, 2)[3]
    want = R.clip([refs[2]], [diss[2]], bpc, hfr)[0]
    assert np.array_equal(first[:, 3:6], want) and np.array_equal(again[1:, 3:6], want)
    assert np.array_equal(again[0, 3:6], R.clip([refs[2], refs[3]], [diss[2], diss[3]], bpc, hfr)[0][1])
    assert not np.array_equal(first[0, 3:6], base[2, 3:6])


@pytest.mark.parametrize("hfr", [False, True])
def test_shard_equivalence(hfr):
    from pqa2_amd import _native as N
    from pqa2_amd.engine import FeatureEngine
    w, h, bpc, n, a = 1920, 1080, 10, 6, 3
    refs, diss = _frames(w, h, bpc, 1, 1, n, seed=33)
    feats = N.FEAT_VMAF | N.FEAT_XPSNR | (N.FEAT_XPSNR_HFR if hfr else 0)
    full = _run(w, h, bpc, 1, 1, refs, diss, features=feats, max_batch=2)
    with FeatureEngine(w, h, bit_depth=bpc, n_planes=3, features=feats, max_batch=2) as eng:
        eng.set_ref_history([refs[a - 1][0], refs[a - 2][0]])
        for i in range(a, n):
            eng.submit(i, refs[i], diss[i])
        tail = eng.collect_ext3(a, n - a)
    assert np.array_equal(_bits(tail[3]), _bits(full[3][a:]))
    assert np.array_equal(_bits(tail[0]), _bits(full[0][a:]))      # motion's halo armed by the same call
    with FeatureEngine(w, h, bit_depth=bpc, n_planes=3, features=feats, max_batch=2) as eng:
        eng.set_ref_history([refs[a - 1][0]])
        for i in range(a, n):
            eng.submit(i, refs[i], diss[i])
        one = eng.collect_ext3(a, n - a)[3]
    if hfr:
        assert not np.array_equal(one[0, 3:6], full[3][a, 3:6]), "second order needs frame a-2"
        assert np.array_equal(_bits(one[2:]), _bits(full[3][a + 2:]))
    else:
        assert np.array_equal(_bits(one), _bits(full[3][a:]))


def test_other_outputs_unchanged_and_nan_without_the_bit():
    from pqa2_amd import _native as N
    w, h, bpc, n = 352, 288, 8, 5
    refs, diss = _frames(w, h, bpc, 1, 1, n, seed=55)
    rest = N.FEAT_ALL | N.FEAT_FLOAT_SSIM | N.FEAT_CIEDE | N.FEAT_PSNR_HVS
    off = _run(w, h, bpc, 1, 1, refs, diss, features=rest, max_batch=2)
    on = _run(w, h, bpc, 1, 1, refs, diss, features=rest | N.FEAT_XPSNR, max_batch=2)
    for j in range(3):
        assert np.array_equal(_bits(off[j]), _bits(on[j])), j
    assert np.isnan(off[3]).all() and np.isfinite(on[3][:, :6]).all()
