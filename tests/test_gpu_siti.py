"""siti on the MI355X (csrc/siti.hip, PQA_FEAT_SITI / _REF_FULL / _DIS_FULL): the real kernel's gradient map against the
restatement (tests/siti_ref.py) bit for bit, SI / TI over geometries, bit depths, ranges, chroma formats and contents,
bit-identical ext4 rows across every way frames reach the kernels, the distorted chain across batches and shards, and no
effect on the other outputs."""
import ctypes as C
import os
import tempfile

import numpy as np
import pytest

from tests import siti_ref as R

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _plane(w, h, bpc, seed, kind="textured"):
    rng = np.random.default_rng(seed)
    top = (1 << bpc) - 1
    if kind == "flat":
        return np.full((h, w), top // 3, np.int64)
    if kind == "extreme":
        return rng.integers(0, 2, (h, w)) * top
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


def _run(w, h, bpc, hs, vs, refs, diss, features=None, max_batch=0, n_subsample=1, n_planes=3):
    from pqa2_amd import _native as N
    from pqa2_amd.engine import FeatureEngine
    feats = features if features is not None else N.FEAT_SITI
    with FeatureEngine(w, h, bit_depth=bpc, n_planes=n_planes, chroma_shift=(hs, vs), features=feats,
                       max_batch=max_batch, n_subsample=n_subsample) as eng:
        for i in range(len(refs)):
            eng.submit(i, refs[i][:n_planes], diss[i][:n_planes])
        return eng.collect_ext4(0, len(refs))


def _hook(cur, prev, bpc, full):
    from pqa2_amd import _native as N
    lib = N.load()
    h, w = cur.shape
    cur = np.ascontiguousarray(cur)
    prev = None if prev is None else np.ascontiguousarray(prev, cur.dtype)
    gmap = np.zeros((h - 2, w - 2), np.float32)
    out = np.zeros(2, np.float64)
    rc = lib.pqa_debug_siti_plane(cur.ctypes.data, None if prev is None else prev.ctypes.data, w * cur.itemsize, w, h, bpc,
                                  int(full), gmap.ctypes.data, out.ctypes.data)
    assert rc == 0, lib.pqa_last_error(None)
    return gmap, out[0], out[1]


def _want(refs, diss, bpc, ref_full=False, dis_full=False, prev=(None, None)):
    """[n, 4] expected SI / TI (f64 mode on the f32 map; exact TI) in ext4 slot order."""
    dsi, dti = R.clip([d[0] for d in diss], bpc, dis_full, prev=prev[0])
    rsi, rti = R.clip([r[0] for r in refs], bpc, ref_full, prev=prev[1])
    return np.stack([dsi, dti, rsi, rti], 1)


def _close(got, want, rel_si=1e-9, rel_ti=1e-12):
    for j, rel in ((0, rel_si), (1, rel_ti), (2, rel_si), (3, rel_ti)):
        g, w = got[:, j], want[:, j]
        assert (np.abs(g - w) <= rel * np.abs(w) + 1e-300).all(), (j, g, w)


def test_create_accepts_the_bit_and_checks_its_limits():
    from pqa2_amd import _native as N
    from pqa2_amd.engine import FeatureEngine
    with FeatureEngine(64, 48, features=N.FEAT_SITI) as eng:
        assert eng.collect_ext4(0, 0)[4].shape == (0, N.EXT4_DOUBLES)
    for feats, bpc in ((N.FEAT_SITI, 12), (N.FEAT_VMAF | N.FEAT_SITI_REF_FULL, 8), (N.FEAT_SITI_DIS_FULL, 10)):
        with pytest.raises(N.PqaError) as e:
            FeatureEngine(64, 48, bit_depth=bpc, features=feats)
        assert e.value.code == N.PQA_EINVAL and "siti" in str(e.value)


@pytest.mark.parametrize("bpc", [8, 10])
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("kind", ["textured", "flat", "extreme"])
def test_hook_gradient_map_is_bit_exact(bpc, full, kind):
    sizes = [(s, s) for s in range(3, 16)] + [(16, 16), (17, 5), (5, 17), (61, 7), (62, 9), (63, 11), (64, 48),
                                               (125, 33), (249, 130), (352, 288)]
    for (w, h) in sizes:
        cur = _plane(w, h, bpc, w * 7 + h, kind)
        prev = _plane(w, h, bpc, w * 7 + h + 1, "textured")
        dt = np.uint8 if bpc == 8 else np.uint16
        gmap, si, ti = _hook(cur.astype(dt), prev.astype(dt), bpc, full)
        yc = R.to_full(cur, bpc, full)
        want = R.gradient_map(yc)
        assert np.array_equal(gmap.view(np.uint32), want.view(np.uint32)), (w, h)
        si64 = R.std(want, "f64")
        assert abs(si - si64) <= 1e-9 * si64 + 1e-7 * float(np.abs(want).mean()), (w, h, si, si64)
        assert abs(si - R.std(want, "ffmpeg")) <= 1e-6 * max(si64, 1e-30) + 1e-6, (w, h)
        m = yc - R.to_full(prev, bpc, full)
        assert abs(ti - R.ti_exact(m)) <= 1e-12 * R.ti_exact(m), (w, h)
        _, _, ti0 = _hook(cur.astype(dt), None, bpc, full)
        assert ti0 == 0.0


@pytest.mark.parametrize("w,h", [(1920, 1080), (3840, 2160)])
@pytest.mark.parametrize("bpc", [8, 10])
def test_hook_large_planes(w, h, bpc):
    dt = np.uint8 if bpc == 8 else np.uint16
    cur, prev = _plane(w, h, bpc, 5).astype(dt), _plane(w, h, bpc, 6).astype(dt)
    gmap, si, ti = _hook(cur, prev, bpc, False)
    want = R.gradient_map(R.to_full(cur, bpc))
    assert np.array_equal(gmap.view(np.uint32), want.view(np.uint32))
    si64 = R.std(want, "f64")
    assert abs(si - si64) <= 1e-9 * si64
    assert abs(si - R.std(want, "ffmpeg")) <= 1e-6 * si64
    tw = R.ti_exact(R.to_full(cur, bpc) - R.to_full(prev, bpc))
    assert abs(ti - tw) <= 1e-12 * tw


@pytest.mark.parametrize("w,h,hs,vs,bpc,planes", [(16, 16, 1, 1, 8, 3), (17, 19, 1, 1, 8, 3), (64, 48, 1, 0, 10, 3),
                                                  (125, 61, 0, 0, 8, 3), (352, 288, 1, 1, 10, 1),
                                                  (1920, 1080, 1, 1, 8, 3), (1920, 1080, 1, 1, 10, 3),
                                                  (3840, 2160, 1, 1, 8, 3), (641, 359, 2, 2, 10, 3)])
@pytest.mark.parametrize("ranges", [(False, False), (True, False), (False, True)])
def test_full_path_equals_the_restatement(w, h, hs, vs, bpc, planes, ranges):
    from pqa2_amd import _native as N
    ref_full, dis_full = ranges
    n = 3 if w * h > 2_000_000 else 4
    refs, diss = _frames(w, h, bpc, hs, vs, n, seed=w + h + bpc, planes=planes)
    feats = N.FEAT_SITI | (N.FEAT_SITI_REF_FULL if ref_full else 0) | (N.FEAT_SITI_DIS_FULL if dis_full else 0)
    ext4 = _run(w, h, bpc, hs, vs, refs, diss, features=feats, n_planes=planes)[4]
    _close(ext4[:, :4], _want(refs, diss, bpc, ref_full, dis_full))
    assert np.isnan(ext4[:, 4:]).all()
    assert (ext4[0, [1, 3]] == 0.0).all()


def test_repeated_distorted_frames_give_zero_ti():
    from pqa2_amd import _native as N
    w, h, bpc, n = 352, 288, 8, 6
    refs, diss = _frames(w, h, bpc, 1, 1, n, seed=9)
    for i in (2, 3, 5):            # a frozen capture: the previous distorted frame again
        diss[i] = [p.copy() for p in diss[i - 1]]
    ext4 = _run(w, h, bpc, 1, 1, refs, diss, features=N.FEAT_VMAF | N.FEAT_SITI, max_batch=2)[4]
    assert (ext4[[2, 3, 5], N.EXT4_TI] == 0.0).all()
    assert (ext4[1:, N.EXT4_TI_SOURCE] > 0).all() and ext4[1, N.EXT4_TI] > 0 and ext4[4, N.EXT4_TI] > 0


@pytest.mark.parametrize("bpc", [8, 10])
def test_bit_identical_across_batches_submit_paths_and_features(bpc):
    import torch
    from pqa2_amd import _native as N
    from pqa2_amd.engine import FeatureEngine
    w, h, n = 352, 288, 7
    refs, diss = _frames(w, h, bpc, 1, 1, n, seed=40)
    feats = N.FEAT_SITI
    base = None
    for mb in (1, 7, 0):
        ext4 = _run(w, h, bpc, 1, 1, refs, diss, features=feats, max_batch=mb)[4]
        if base is None:
            base = ext4
        assert np.array_equal(_bits(ext4), _bits(base)), f"max_batch {mb}"
    _close(base[:, :4], _want(refs, diss, bpc))
    for ns in (1, 3):
        ext4 = _run(w, h, bpc, 1, 1, refs, diss, features=feats, n_subsample=ns, max_batch=3)[4]
        assert np.array_equal(_bits(ext4), _bits(base)), f"n_subsample {ns}"
    everything = (N.FEAT_ALL | N.FEAT_FLOAT_SSIM | N.FEAT_MS_SSIM | N.FEAT_CIEDE | N.FEAT_CAMBI | N.FEAT_CAMBI_FULL_REF
                  | N.FEAT_PSNR_HVS | N.FEAT_XPSNR | N.FEAT_SITI)
    ext4 = _run(w, h, bpc, 1, 1, refs, diss, features=everything, max_batch=3)[4]
    assert np.array_equal(_bits(ext4), _bits(base)), "with every other feature"
    # files: fd-run submits
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
                ext4 = eng.collect_ext4(0, n)[4]
        finally:
            for fd in fds:
                os.close(fd)
    assert np.array_equal(_bits(ext4), _bits(base)), "fd run"
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
            ext4 = eng.collect_ext4(0, n)[4]
        assert np.array_equal(_bits(ext4), _bits(base)), f"resident offset {off} pad {pad}"
        # the same run in two calls: the second continues both chains from the kept planes
        with FeatureEngine(w, h, bit_depth=bpc, n_planes=3, features=feats, max_batch=2) as eng:
            eng.submit_resident(0, 3, ptrs[0], ptrs[1], rps, fps)
            eng.submit_resident(3, n - 3, [q + 3 * fps[p] for p, q in enumerate(ptrs[0])],
                                [q + 3 * fps[p] for p, q in enumerate(ptrs[1])], rps, fps,
                                ptrs[0][0] + 2 * fps[0], rps[0])
            ext4 = eng.collect_ext4(0, n)[4]
        assert np.array_equal(_bits(ext4), _bits(base)), f"resident split, offset {off}"
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
        ext4 = eng.collect_ext4(0, n)[4]
    assert np.array_equal(_bits(ext4), _bits(base)), "submit_surfaces"
    # a surface run that starts at frame 1 with frame 0 as prev_ref and the distorted frame 0 armed: the same rows
    sub = [FeatureEngine.surface_clip(fmt, tl[s].data_ptr() + h * lpb, lpb, h * lpb, tc[s].data_ptr() + (h // 2) * cpb,
                                      cpb, (h // 2) * cpb) for s in (0, 1)]
    with FeatureEngine(w, h, bit_depth=bpc, n_planes=3, features=feats, max_batch=2) as eng:
        eng.set_dis_history(diss[0][0])
        eng.submit_surfaces(1, n - 1, sub[0], sub[1], clip[0])
        ext4 = eng.collect_ext4(1, n - 1)[4]
    assert np.array_equal(_bits(ext4), _bits(base[1:])), "surfaces with prev_ref and the distorted history"


@pytest.mark.parametrize("ranks", [2, 3])
def test_shards_equal_a_single_run(ranks):
    from pqa2_amd import _native as N
    from pqa2_amd import shard
    from pqa2_amd.engine import FeatureEngine
    w, h, bpc, n = 640, 360, 10, 7
    refs, diss = _frames(w, h, bpc, 1, 1, n, seed=33)
    feats = N.FEAT_SITI | N.FEAT_SITI_DIS_FULL
    full = _run(w, h, bpc, 1, 1, refs, diss, features=feats, max_batch=2)[4]
    rows = []
    for rank in range(ranks):
        a, b = shard.shard_bounds(n, ranks, rank)
        with FeatureEngine(w, h, bit_depth=bpc, n_planes=3, features=feats, max_batch=2) as eng:
            if a > 0:
                eng.set_motion_halo(refs[a - 1][0])
                eng.set_dis_history(diss[a - 1][0])
            for i in range(a, b):
                eng.submit(i, refs[i], diss[i])
            rows.append(eng.collect_ext4(a, b - a)[4])
    assert np.array_equal(_bits(np.concatenate(rows)), _bits(full))
    # without the distorted history the shard's first distorted TI restarts at 0; the reference side still continues
    a = shard.shard_bounds(n, ranks, 1)[0]
    with FeatureEngine(w, h, bit_depth=bpc, n_planes=3, features=feats, max_batch=2) as eng:
        eng.set_ref_history([refs[a - 1][0]])
        eng.submit(a, refs[a], diss[a])
        row = eng.collect_ext4(a, 1)[4][0]
    assert row[N.EXT4_TI] == 0.0 and row[N.EXT4_TI_SOURCE] == full[a, N.EXT4_TI_SOURCE]
    assert row[N.EXT4_SI] == full[a, N.EXT4_SI]


def test_reset_and_null_history_restart_the_chains():
    from pqa2_amd import _native as N
    from pqa2_amd.engine import FeatureEngine
    w, h, bpc, n = 64, 48, 8, 4
    refs, diss = _frames(w, h, bpc, 1, 1, n, seed=21)
    with FeatureEngine(w, h, bit_depth=bpc, n_planes=3, features=N.FEAT_SITI, max_batch=2) as eng:
        for i in range(n):
            eng.submit(i, refs[i], diss[i])
        base = eng.collect_ext4(0, n)[4]
        eng.reset()
        eng.submit(0, refs[2], diss[2])
        first = eng.collect_ext4(0, 1)[4]
        eng.submit(1, refs[3], diss[3])
        eng.set_dis_history(None)
        eng.submit(2, refs[2], diss[2])
        again = eng.collect_ext4(1, 2)[4]
    assert (first[0, [1, 3]] == 0.0).all() and first[0, 0] == base[2, 0] and first[0, 2] == base[2, 2]
    assert again[0, 1] == base[3, 1] and again[0, 3] == base[3, 3]
    assert again[1, 1] == 0.0 and again[1, 3] > 0.0
    # a jump in the frame index with no reset and nothing armed (frames 0..2, then 7..8) starts every chain -- motion, xpsnr,
    # siti and the integrity differences -- exactly as a fresh context does
    refs, diss = _frames(w, h, bpc, 1, 1, 5, seed=22)
    feats = N.FEAT_VMAF | N.FEAT_XPSNR | N.FEAT_SITI | N.FEAT_INTEGRITY
    with FeatureEngine(w, h, bit_depth=bpc, n_planes=3, features=feats, max_batch=2) as eng:
        for i in range(3):
            eng.submit(i, refs[i], diss[i])
        for i in (3, 4):
            eng.submit(i + 4, refs[i], diss[i])
        jumped = eng.collect_ext5(7, 2)
    with FeatureEngine(w, h, bit_depth=bpc, n_planes=3, features=feats, max_batch=2) as eng:
        for i in (3, 4):
            eng.submit(i - 3, refs[i], diss[i])
        fresh = eng.collect_ext5(0, 2)
    for j in (0, 3, 4, 5):
        assert np.array_equal(_bits(jumped[j]), _bits(fresh[j])), j
    assert fresh[0][0, N.REC_MOTION] == 0.0 and fresh[4][0, N.EXT4_TI] == 0.0 and np.isnan(fresh[5][0, :3]).all()


def test_other_outputs_unchanged_and_nan_without_the_bit():
    from pqa2_amd import _native as N
    w, h, bpc, n = 352, 288, 8, 5
    refs, diss = _frames(w, h, bpc, 1, 1, n, seed=55)
    rest = N.FEAT_ALL | N.FEAT_FLOAT_SSIM | N.FEAT_CIEDE | N.FEAT_PSNR_HVS | N.FEAT_XPSNR
    off = _run(w, h, bpc, 1, 1, refs, diss, features=rest, max_batch=2)
    on = _run(w, h, bpc, 1, 1, refs, diss, features=rest | N.FEAT_SITI, max_batch=2)
    for j in range(4):
        assert np.array_equal(_bits(off[j]), _bits(on[j])), j
    assert np.isnan(off[4]).all() and np.isfinite(on[4][:, :4]).all()
