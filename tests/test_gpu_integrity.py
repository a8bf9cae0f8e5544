"""Capture integrity on the MI355X (csrc/integrity.hip, PQA_FEAT_INTEGRITY): the kernel's SADs and black counts equal the
numpy restatement (tests/integrity_ref.py) as integers over bit depths, plane counts, chroma formats, sizes, pitches, base
alignments and sample extremes; rows are bit-identical across batch sizes, submit paths, feature sets and shards; the
anchored SADs; no effect on the other outputs; and a clip with a freeze, a black lead-in and a cut through the analyzer."""
import os
import tempfile

import numpy as np
import pytest

from tests import integrity_ref as R

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _clip(w, h, bpc, hs, vs, n, seed, planes=3, kind="noise"):
    """n distorted frames [Y(,U,V)] and reference frames of the same shapes."""
    dt = np.uint8 if bpc == 8 else np.uint16
    top = (1 << bpc) - 1
    rng = np.random.default_rng(seed)
    wc, hc = (w + (1 << hs) - 1) >> hs, (h + (1 << vs) - 1) >> vs
    shapes = [(h, w), (hc, wc), (hc, wc)][:planes]
    out = []
    for i in range(n):
        if kind == "extreme":       # all 0 against all 2^bpc - 1: the largest sums
            out.append([np.full(s, top if i % 2 else 0, dt) for s in shapes])
        elif kind == "dark":        # around the black threshold
            f = 1 << (bpc - 8)
            out.append([rng.integers(30 * f, 45 * f, s).astype(dt) for s in shapes])
        else:
            out.append([rng.integers(0, top + 1, s).astype(dt) for s in shapes])
    refs = [[rng.integers(0, top + 1, s).astype(dt) for s in shapes] for _ in range(n)]
    return refs, out


def _run(w, h, bpc, hs, vs, refs, diss, features=None, max_batch=0, n_planes=3, thr=None, n_subsample=1, which=5):
    from pqa2_amd import _native as N
    from pqa2_amd.engine import FeatureEngine
    feats = features if features is not None else N.FEAT_INTEGRITY
    with FeatureEngine(w, h, bit_depth=bpc, n_planes=n_planes, chroma_shift=(hs, vs), features=feats, max_batch=max_batch,
                       n_subsample=n_subsample) as eng:
        if thr is not None:
            eng.set_black_threshold(thr)
        for i in range(len(diss)):
            eng.submit(i, refs[i][:n_planes], diss[i][:n_planes])
        got = eng.collect_ext5(0, len(diss))
    return got if which is None else got[which]


def _same(got, want):
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    assert np.array_equal(np.nan_to_num(got), np.nan_to_num(want)), (got, want)


def test_create_defaults_and_threshold_rules():
    from pqa2_amd import _native as N
    from pqa2_amd.engine import FeatureEngine
    for bpc, want in ((8, 37), (10, 151), (12, 606)):
        f = 1 << (bpc - 8)
        dt = np.uint8 if bpc == 8 else np.uint16
        fr = [np.concatenate([np.full((8, 16), want, dt), np.full((8, 16), want + 1, dt)])]
        assert _run(16, 16, bpc, 1, 1, [fr], [fr], n_planes=1)[0, 3] == 128          # <= : the default threshold itself counts
        assert R.black_threshold(bpc) == want and f
    refs, diss = _clip(32, 16, 8, 1, 1, 2, 1)
    with FeatureEngine(32, 16, n_planes=3, features=N.FEAT_INTEGRITY) as eng:
        with pytest.raises(N.PqaError) as e:
            eng.set_black_threshold(256)
        assert e.value.code == N.PQA_EINVAL
        eng.set_black_threshold(255)
        eng.submit(0, refs[0], diss[0])
        eng.flush()
        with pytest.raises(N.PqaError) as e:
            eng.set_black_threshold(10)
        assert e.value.code == N.PQA_ESTATE
        assert eng.collect_ext5(0, 1)[5][0, 3] == 32 * 16
        eng.reset()
        eng.set_black_threshold(10)
    with FeatureEngine(32, 16, n_planes=3, features=N.FEAT_VMAF) as eng:     # without the bit: NaN rows, sad calls refused
        eng.submit(0, refs[0], diss[0])
        assert np.isnan(eng.collect_ext5(0, 1)[5]).all()
        eng.set_dis_history_planes(diss[0])
        with pytest.raises(N.PqaError) as e:
            eng.frame_sad(diss[0], [diss[1]])
        assert e.value.code == N.PQA_ESTATE


@pytest.mark.parametrize("bpc", [8, 10, 12])
@pytest.mark.parametrize("w,h,hs,vs,planes", [(16, 16, 1, 1, 3), (16, 16, 0, 0, 1), (17, 19, 1, 1, 3), (64, 48, 1, 0, 3),
                                              (125, 61, 0, 0, 3), (321, 241, 1, 1, 3), (321, 241, 1, 1, 1), (352, 288, 1, 0, 3),
                                              (641, 359, 2, 2, 3), (1920, 1080, 1, 1, 3), (1920, 1080, 0, 0, 3)] +
                         # the mixed layouts: the two chroma shifts differ
                         [(w, h, hs, vs, 3) for (hs, vs) in [(2, 0), (0, 2), (1, 2), (2, 1), (0, 1)]
                          for (w, h) in [(17, 19), (64, 48)]])
@pytest.mark.parametrize("kind", ["noise", "extreme", "dark"])
def test_rows_equal_the_restatement_as_integers(bpc, w, h, hs, vs, planes, kind):
    n = 3 if w * h > 1_000_000 else 4
    refs, diss = _clip(w, h, bpc, hs, vs, n, seed=w + h + bpc, planes=planes, kind=kind)
    thr = R.black_threshold(bpc)
    got = _run(w, h, bpc, hs, vs, refs, diss, n_planes=planes, max_batch=3)
    _same(got, R.rows(diss, thr))
    assert np.isnan(got[0, :3]).all() and np.isnan(got[:, 4:]).all() and np.isnan(got[1:, planes:3]).all()
    if kind == "extreme":
        assert got[1, 0] == float(((1 << bpc) - 1) * w * h)


@pytest.mark.parametrize("bpc,kind", [(8, "noise"), (10, "noise"), (12, "extreme"), (8, "extreme")])
def test_2160p_rows_equal_the_restatement(bpc, kind):
    w, h = 3840, 2160
    refs, diss = _clip(w, h, bpc, 1, 1, 3, seed=bpc, kind=kind)
    _same(_run(w, h, bpc, 1, 1, refs, diss), R.rows(diss, R.black_threshold(bpc)))


def _resident(diss_or_refs, sizes, n, es, dt, off, pad):
    import torch
    ptrs, keep, rps, fps = [], [], [], []
    for p, (pw, ph) in enumerate(sizes):
        pitch = pw + pad + p
        rps.append(pitch * es)
        fps.append(ph * pitch * es)
        buf = np.full(off + n * ph * pitch, 0xA5, dt)
        for i in range(n):
            buf[off + i * ph * pitch: off + (i + 1) * ph * pitch].reshape(ph, pitch)[:, :pw] = diss_or_refs[i][p]
        t = torch.from_numpy(buf.view(np.uint8)).cuda()
        keep.append(t)
        ptrs.append(t.data_ptr() + off * es)
    return ptrs, rps, fps, keep


@pytest.mark.parametrize("bpc", [8, 10])
def test_bit_identical_across_batches_submit_paths_and_features(bpc):
    import torch
    from pqa2_amd import _native as N
    from pqa2_amd.engine import FeatureEngine
    w, h, n = 352, 288, 7
    refs, diss = _clip(w, h, bpc, 1, 1, n, seed=40, kind="dark")
    feats = N.FEAT_INTEGRITY
    base = _run(w, h, bpc, 1, 1, refs, diss, max_batch=1)
    _same(base, R.rows(diss, R.black_threshold(bpc)))
    for mb in (3, 0):
        assert np.array_equal(_bits(_run(w, h, bpc, 1, 1, refs, diss, max_batch=mb)), _bits(base)), f"max_batch {mb}"
    assert np.array_equal(_bits(_run(w, h, bpc, 1, 1, refs, diss, max_batch=3, n_subsample=3)), _bits(base)), "n_subsample"
    everything = (N.FEAT_ALL | N.FEAT_FLOAT_SSIM | N.FEAT_MS_SSIM | N.FEAT_CIEDE | N.FEAT_CAMBI | N.FEAT_CAMBI_FULL_REF
                  | N.FEAT_PSNR_HVS | N.FEAT_XPSNR | N.FEAT_SITI | N.FEAT_INTEGRITY)
    assert np.array_equal(_bits(_run(w, h, bpc, 1, 1, refs, diss, features=everything, max_batch=3)), _bits(base)), "every feature"
    es = 1 if bpc == 8 else 2
    dt = np.uint8 if bpc == 8 else np.uint16
    with tempfile.TemporaryDirectory() as d:      # files: fd-run submits
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
                eng.submit_file_run(4, n - 4, fds[0], [o + 4 * fsz for o in offs], fsz, fds[1], [o + 4 * fsz for o in offs], fsz)
                got = eng.collect_ext5(0, n)[5]
        finally:
            for fd in fds:
                os.close(fd)
    assert np.array_equal(_bits(got), _bits(base)), "fd run"
    sizes = [(w, h), (w // 2, h // 2), (w // 2, h // 2)]
    for off, pad in ((0, 0), (1, 3), (7, 13), (16 // es, 16 // es)):   # odd pitches and unaligned bases (elements)
        rp, rps, fps, k1 = _resident(refs, sizes, n, es, dt, off, pad)
        dp, _, _, k2 = _resident(diss, sizes, n, es, dt, off, pad)
        torch.cuda.synchronize()
        with FeatureEngine(w, h, bit_depth=bpc, n_planes=3, features=feats, max_batch=3) as eng:
            eng.submit_resident(0, n, rp, dp, rps, fps)
            got = eng.collect_ext5(0, n)[5]
            # the anchored SADs of the same resident clip against its frame 2, and of host frames
            sad_dev = eng.frame_sad_resident([q + 2 * fps[p] for p, q in enumerate(dp)], rps, dp, rps, fps, n)
            sad_host = eng.frame_sad(diss[2], diss)
        assert np.array_equal(_bits(got), _bits(base)), f"resident offset {off} pad {pad}"
        assert np.array_equal(sad_dev, R.frame_sad(diss[2], diss)) and np.array_equal(sad_host, sad_dev), (off, pad)
        with FeatureEngine(w, h, bit_depth=bpc, n_planes=3, features=feats, max_batch=2) as eng:   # two calls: the kept planes
            eng.submit_resident(0, 3, rp, dp, rps, fps)
            eng.submit_resident(3, n - 3, [q + 3 * fps[p] for p, q in enumerate(rp)], [q + 3 * fps[p] for p, q in enumerate(dp)],
                                rps, fps)
            got = eng.collect_ext5(0, n)[5]
        assert np.array_equal(_bits(got), _bits(base)), f"resident split, offset {off}"
    lp, cp = w + 5, w + 9                          # decoder surfaces (4:2:0 only)
    shift = 0 if bpc == 8 else 16 - bpc
    L = np.zeros((2, n, h, lp), dt)
    CH = np.zeros((2, n, h // 2, cp), dt)
    for i in range(n):
        for side, src in enumerate((refs, diss)):
            L[side, i, :, :w] = src[i][0].astype(dt) << shift
            CH[side, i, :, 0:w:2] = src[i][1].astype(dt) << shift
            CH[side, i, :, 1:w:2] = src[i][2].astype(dt) << shift
    tl, tc = torch.from_numpy(L.view(np.uint8)).cuda(), torch.from_numpy(CH.view(np.uint8)).cuda()
    torch.cuda.synchronize()
    fmt = N.SURFACE_NV12 if bpc == 8 else N.SURFACE_P01X
    lpb, cpb = lp * es, cp * es
    clip = [FeatureEngine.surface_clip(fmt, tl[s].data_ptr(), lpb, h * lpb, tc[s].data_ptr(), cpb, (h // 2) * cpb) for s in (0, 1)]
    with FeatureEngine(w, h, bit_depth=bpc, n_planes=3, features=feats, max_batch=2) as eng:
        eng.submit_surfaces(0, n, clip[0], clip[1])
        got = eng.collect_ext5(0, n)[5]
    assert np.array_equal(_bits(got), _bits(base)), "submit_surfaces"


@pytest.mark.parametrize("ranks", [2, 3])
@pytest.mark.parametrize("bpc,hs,vs", [(8, 1, 1), (10, 1, 0), (12, 0, 0)])
def test_shards_equal_a_single_run(ranks, bpc, hs, vs):
    from pqa2_amd import _native as N
    from pqa2_amd import shard
    from pqa2_amd.engine import FeatureEngine
    w, h, n = 321, 241, 7
    refs, diss = _clip(w, h, bpc, hs, vs, n, seed=33)
    feats = N.FEAT_INTEGRITY | N.FEAT_SITI if bpc < 12 else N.FEAT_INTEGRITY
    full = _run(w, h, bpc, hs, vs, refs, diss, features=feats, max_batch=2, which=None)
    rows, siti_rows = [], []
    for rank in range(ranks):
        a, b = shard.shard_bounds(n, ranks, rank)
        with FeatureEngine(w, h, bit_depth=bpc, n_planes=3, chroma_shift=(hs, vs), features=feats, max_batch=2) as eng:
            if a > 0:
                eng.set_motion_halo(refs[a - 1][0])
                eng.set_dis_history_planes(diss[a - 1])      # arms siti's distorted luma as well
            for i in range(a, b):
                eng.submit(i, refs[i], diss[i])
            got = eng.collect_ext5(a, b - a)
            rows.append(got[5])
            siti_rows.append(got[4])
    assert np.array_equal(_bits(np.concatenate(rows)), _bits(full[5]))
    assert np.array_equal(_bits(np.concatenate(siti_rows)), _bits(full[4]))
    a = shard.shard_bounds(n, ranks, 1)[0]
    with FeatureEngine(w, h, bit_depth=bpc, n_planes=3, chroma_shift=(hs, vs), features=feats, max_batch=2) as eng:
        eng.set_dis_history_planes(diss[a - 1])
        eng.set_dis_history_planes(None)                     # NULL restarts the chain
        eng.submit(a, refs[a], diss[a])
        row = eng.collect_ext5(a, 1)[5][0]
        eng.submit(a + 1, refs[a + 1], diss[a + 1])
        eng.reset()
        eng.submit(0, refs[a + 1], diss[a + 1])
        again = eng.collect_ext5(0, 1)[5][0]
    assert np.isnan(row[:3]).all() and row[3] == full[5][a, 3] and np.isnan(again[:3]).all()


def test_frame_sad_equals_the_restatement():
    from pqa2_amd import _native as N
    from pqa2_amd.engine import FeatureEngine
    for (w, h, bpc, hs, vs, planes, n) in ((16, 16, 8, 1, 1, 3, 3), (321, 241, 10, 1, 1, 3, 19), (125, 61, 12, 0, 0, 1, 5),
                                           (1920, 1080, 8, 1, 1, 3, 11)):
        _, diss = _clip(w, h, bpc, hs, vs, n, seed=w + bpc, planes=planes)
        with FeatureEngine(w, h, bit_depth=bpc, n_planes=planes, chroma_shift=(hs, vs), features=N.FEAT_INTEGRITY, max_batch=2) as eng:
            got = eng.frame_sad(diss[1], diss)               # more frames than max_batch and than one upload chunk
            strided = eng.frame_sad([np.pad(p, ((0, 0), (0, 5)))[:, :p.shape[1]] for p in diss[1]], diss[:2])
            assert eng.frame_sad(diss[0], []).shape == (0, 3)
        assert np.array_equal(got, R.frame_sad(diss[1], diss)) and (got[1] == 0).all() and got.dtype == np.uint64
        assert np.array_equal(strided, got[:2])


def _write_pair(d, refs, diss, fps=25):
    from pqa2_amd import synth, yuvio
    info = synth.clip_info(64, 48, 8, chroma=True)
    info.fps_num, info.fps_den = fps, 1
    rp, dp = os.path.join(d, "ref.y4m"), os.path.join(d, "dis.y4m")
    yuvio.write_y4m(rp, refs, info)
    yuvio.write_y4m(dp, diss, info)
    return rp, dp


def test_drift_clip_through_score_files_alternates_the_anchor(tmp_path):
    from pqa2_amd.pipeline import score_files
    n = 12
    luma = np.full(64 * 48, 100, np.int64)
    frames = []
    for j in range(n):
        if j:
            luma = luma.copy()
            luma[(np.arange(1000) + (j - 1) * 1000) % luma.size] += 1
        frames.append([luma.reshape(48, 64).astype(np.uint8), np.full((24, 32), 128, np.uint8), np.full((24, 32), 128, np.uint8)])
    rp, dp = _write_pair(str(tmp_path), frames, frames)
    res = score_files(rp, dp, "vmaf_v0.6.1", integrity=True, integrity_options={"freeze_duration": 0.08}, psnr=False, ssim=False)
    assert list(res["freeze_anchor"]) == [0, 0, 0, 2, 2, 4, 4, 6, 6, 8, 8, 10]
    assert res["integrity"]["freezes"] == []
    assert list(res["metrics"]["freeze_mafd"]) == [0.0] + [(1000 if i % 2 else 2000) / 4608 / 256 for i in range(1, n)]


def test_other_outputs_unchanged_and_nan_without_the_bit():
    from pqa2_amd import _native as N
    w, h, bpc, n = 352, 288, 8, 5
    refs, diss = _clip(w, h, bpc, 1, 1, n, seed=55)
    rest = N.FEAT_ALL | N.FEAT_FLOAT_SSIM | N.FEAT_CIEDE | N.FEAT_PSNR_HVS | N.FEAT_XPSNR | N.FEAT_SITI
    off = _run(w, h, bpc, 1, 1, refs, diss, features=rest, max_batch=2, which=None)
    on = _run(w, h, bpc, 1, 1, refs, diss, features=rest | N.FEAT_INTEGRITY, max_batch=2, which=None)
    for j in range(5):          # the 24-double records and the four existing extension records
        assert np.array_equal(_bits(off[j]), _bits(on[j])), j
    assert np.isnan(off[5]).all() and np.isfinite(on[5][1:, :4]).all()


def test_freeze_black_and_cut_through_the_analyzer(tmp_path):
    """64 x 48 at 25 fps: 20 black frames, 30 of content, a 60-frame freeze (frames 50..109 are frame 50), 10 more of
    content, a hard cut at frame 120.  Figures: tests/integrity_ref.py fault_clip and tests/test_integrity.py."""
    from pqa2_amd import vmaf_analyzer as V
    refs, diss = R.fault_clip(20, 30, 60, 10, 10)
    rp, dp = _write_pair(str(tmp_path), refs, diss)
    a = V.VMAFAnalyzer()
    a.set_output_directory(str(tmp_path))
    a.set_test_name("cap")
    a.set_advanced_options(integrity_enabled=True, integrity_options={"black_min_duration": 0.5})
    res = a.analyze_videos(rp, dp)
    assert res is not None
    assert res["integrity"] == {
        "freezes": [{"start": 2.0, "end": 4.4, "duration": 2.4, "first_frame": 50, "last_frame": 109}],
        "blacks": [{"start": 0.0, "end": 0.8, "duration": 0.8, "first_frame": 0, "last_frame": 19}],
        "scene_changes": [{"frame": 20, "time": 0.8, "score": 29.4921875}, {"frame": 120, "time": 4.8, "score": 33.642578125}]}
    assert open(res["integrity_log"]).read().splitlines() == [
        "black_start:0 black_end:0.8 black_duration:0.8", "lavfi.scd.score: 29.492, lavfi.scd.time: 0.8", "freeze_start: 2",
        "freeze_duration: 2.4", "freeze_end: 4.4", "lavfi.scd.score: 33.643, lavfi.scd.time: 4.8"]
    frames = res["raw_results"]["frames"]
    assert len(frames) == 130 and frames[60]["metrics"]["freeze_mafd"] == 0.0 and frames[5]["metrics"]["black_ratio"] == 1.0
    assert frames[30]["metrics"]["scd_mafd"] == 1.513672
