"""Level alignment on the MI355X (csrc/level_stats.hip, pqa_level_stats / pqa_level_stats_device): the per-level transfer
table equals the numpy restatement (tests/level_ref.py) as integers -- smallest call and argument rules, row tails /
pitches / odd base addresses at 8 / 10 / 12 bit and a chroma plane, every bin, the accumulator limits on flat frames, the
contention patterns, more frames than a launch chunk, the SSE identity against the PSNR feature; the calls leave the
scoring chain alone; and range-converted Y4M pairs through score_files(level_align=) and VMAFAnalyzer give the records of
the capture mapped back by hand."""
import json

import numpy as np
import pytest

from tests import level_ref as R

pytestmark = pytest.mark.gpu


def _engine(w, h, bpc=8, **kw):
    from pqa2_amd import _native as N
    from pqa2_amd.engine import FeatureEngine
    return FeatureEngine(w, h, bit_depth=bpc, n_planes=kw.pop("n_planes", 1), features=kw.pop("features", N.FEAT_PSNR), **kw)


def _dt(bpc):
    return np.uint8 if bpc == 8 else np.uint16


def _padded(frames, pad=5, lead=1):
    """the same frames as views into one buffer: rows `pad` samples longer than a row, base `lead` samples in"""
    h, w = frames[0].shape
    buf = np.zeros((len(frames), h, w + pad), frames[0].dtype)
    buf[:, :, lead:lead + w] = np.stack(frames)
    return buf, [buf[i, :, lead:lead + w] for i in range(len(frames))]


def _resident(eng, ref_buf, dis_buf, lead, n, plane=0):
    import torch
    es = ref_buf.dtype.itemsize
    tr = torch.from_numpy(ref_buf.view(np.uint8).reshape(-1)).cuda()
    td = torch.from_numpy(dis_buf.view(np.uint8).reshape(-1)).cuda()
    torch.cuda.synchronize()
    return eng.level_stats_resident(tr.data_ptr() + lead * es, ref_buf.strides[1], ref_buf.strides[0], td.data_ptr() + lead * es,
                                    dis_buf.strides[1], dis_buf.strides[0], n, plane)


def test_smallest_call_and_argument_rules():
    from pqa2_amd import _native as N
    ref, dis = R.random_pair(1, 2, 16, 16)
    with _engine(16, 16) as eng:
        got = eng.level_stats(ref, dis)
        assert got.dtype == np.uint64 and got.shape == (2, 256, 3) and np.array_equal(got, R.level_stats(ref, dis, 8))
        assert eng.lib.pqa_level_bins(eng._ctx) == 256
        assert eng.level_stats([], []).shape == (0, 256, 3)
        assert eng.level_stats_resident(0, 16, 256, 0, 16, 256, 0).shape == (0, 256, 3)
        for call in (lambda: eng.level_stats(ref, dis, 1),      # plane 1 of a context with one plane
                     lambda: eng.level_stats(ref, dis, -1),
                     lambda: eng.level_stats(ref, dis[:1]),      # unequal list lengths
                     lambda: eng.level_stats_resident(0, 16, 256, 0, 16, 256, 1),      # null clip pointers
                     lambda: eng.level_stats_resident(0, 16, 256, 0, 16, 256, -1)):
            with pytest.raises(N.PqaError) as e:
                call()
            assert e.value.code == N.PQA_EINVAL
        assert np.array_equal(eng.level_stats(ref, dis), got)     # a refused call leaves the context usable
    with _engine(16, 16, 10) as eng:
        assert eng.lib.pqa_level_bins(eng._ctx) == 1024 and eng.level_stats([], []).shape == (0, 1024, 3)


@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_tails_pitches_and_depths(bpc):
    """50 x 18: a row is no whole number of 16-byte loads; rows padded by 5 samples, base one sample in (the per-sample
    path at 8 bit, the 2-byte one above); the host entry on contiguous frames, on views, and the resident entry agree; one
    64-byte-aligned layout with a row tail (the 16-byte loads) and one 4-byte-aligned one (the word loads)"""
    ref, dis = R.random_pair(10 + bpc, 3, 50, 18, bpc)
    want = R.level_stats(ref, dis, bpc)
    rbuf, rv = _padded(ref)
    dbuf, dv = _padded(dis)
    with _engine(50, 18, bpc) as eng:
        assert np.array_equal(eng.level_stats(ref, dis), want)
        assert np.array_equal(eng.level_stats(rv, dv), want)
        assert np.array_equal(_resident(eng, rbuf, dbuf, 1, 3), want)
        abuf, _ = _padded(ref, pad=14, lead=0)      # 64-byte rows at 8 bit, 128-byte rows at 16
        bbuf, _ = _padded(dis, pad=14, lead=0)
        assert np.array_equal(_resident(eng, abuf, bbuf, 0, 3), want)
        cbuf, _ = _padded(ref, pad=6, lead=4)       # 56-sample rows, base 4 samples in: 4-byte but not 16-byte aligned
        dbuf2, _ = _padded(dis, pad=6, lead=4)
        assert np.array_equal(_resident(eng, cbuf, dbuf2, 4, 3), want)


@pytest.mark.parametrize("bpc,lead,pad,load", [(8, 0, 7, 16), (8, 4, 7, 4), (8, 1, 6, 1), (10, 0, 7, 16), (10, 2, 7, 4), (10, 1, 6, 2)])
def test_every_load_width_with_a_row_that_ends_inside_a_load(bpc, lead, pad, load):
    """201 x 72: full loads, a row that ends one sample into a load of 16 / 8 / 4 / 2 samples, 18 rows a wave.  Rows of 208
    samples from an aligned base: the 16-byte loads; the base 4 bytes in: the word loads (at 10 bit 201 = 100 * 2 + 1, the tail
    the 50-sample rows above do not have); rows of 207 samples, base one sample in: sample by sample"""
    import torch
    w, h = 201, 72
    ref, dis = R.random_pair(90 + bpc + lead, 2, w, h, bpc)
    rbuf, _ = _padded(ref, pad=pad, lead=lead)
    dbuf, _ = _padded(dis, pad=pad, lead=lead)
    es = rbuf.dtype.itemsize
    tr = torch.from_numpy(rbuf.view(np.uint8).reshape(-1)).cuda()
    td = torch.from_numpy(dbuf.view(np.uint8).reshape(-1)).cuda()
    torch.cuda.synchronize()
    pr, pd = tr.data_ptr() + lead * es, td.data_ptr() + lead * es
    bits = pr | pd | rbuf.strides[1] | rbuf.strides[0] | dbuf.strides[1] | dbuf.strides[0]
    assert (16 if bits % 16 == 0 else 4 if bits % 4 == 0 else es) == load      # load_bytes of plane_scan.h
    with _engine(w, h, bpc) as eng:
        got = eng.level_stats_resident(pr, rbuf.strides[1], rbuf.strides[0], pd, dbuf.strides[1], dbuf.strides[0], 2)
    assert np.array_equal(got, R.level_stats(ref, dis, bpc))


def test_chroma_plane_of_a_420_context():
    """plane = 1 of a 50 x 18 4:2:0 context: 25 x 9 samples; luma-sized frames are refused for it"""
    ref, dis = R.random_pair(21, 2, 25, 9)
    luma_r, luma_d = R.random_pair(22, 2, 50, 18)
    with _engine(50, 18, n_planes=3, chroma_shift=(1, 1)) as eng:
        assert eng.plane_shape(1) == (9, 25) and eng.plane_shape(2) == (9, 25)
        assert np.array_equal(eng.level_stats(ref, dis, 1), R.level_stats(ref, dis, 8))
        assert np.array_equal(eng.level_stats(ref, dis, 2), R.level_stats(ref, dis, 8))
        assert np.array_equal(eng.level_stats(luma_r, luma_d, 0), R.level_stats(luma_r, luma_d, 8))
        rbuf, _ = _padded(ref, pad=3, lead=1)
        dbuf, _ = _padded(dis, pad=3, lead=1)
        assert np.array_equal(_resident(eng, rbuf, dbuf, 1, 2, plane=1), R.level_stats(ref, dis, 8))
        with pytest.raises(ValueError):
            eng.level_stats(luma_r, luma_d, 1)


@pytest.mark.parametrize("bpc,w,h", [(12, 128, 32), (10, 64, 16), (8, 16, 16)])
def test_every_bin(bpc, w, h):
    """the reference takes each of the L levels exactly once (a permutation), the capture is random"""
    rng = np.random.default_rng(30 + bpc)
    L = 1 << bpc
    ref = [rng.permutation(L).reshape(h, w).astype(_dt(bpc)) for _ in range(2)]
    dis = [rng.integers(0, L, (h, w)).astype(_dt(bpc)) for _ in range(2)]
    with _engine(w, h, bpc) as eng:
        got = eng.level_stats(ref, dis)
    assert np.array_equal(got, R.level_stats(ref, dis, bpc))
    assert (got[:, :, 0] == 1).all()
    for f in range(2):
        assert np.array_equal(got[f, ref[f].ravel(), 1], dis[f].ravel().astype(np.uint64))


@pytest.mark.parametrize("bpc,w,h", [(8, 512, 256), (10, 320, 64), (12, 1056, 1000)])
def test_accumulator_limits_on_flat_frames(bpc, w, h):
    """every pixel in one bin.  512 x 256 at 8 bit: 131 072 samples of 255, past the u32 limit of sum d^2 (66 052);
    1056 x 1000 at 12 bit: 1 056 000 samples of 4095, sum d = 4 324 320 000 > 2^32; reference 0 with the capture at the
    maximum; one differing pixel in a flat frame"""
    top, n = (1 << bpc) - 1, w * h
    full, zero = np.full((h, w), top, _dt(bpc)), np.zeros((h, w), _dt(bpc))
    one = full.copy()
    one[h // 2, w // 3] = 5
    with _engine(w, h, bpc) as eng:
        got = eng.level_stats([full, zero, one, full], [full, full, full, one])
    want = np.zeros((4, top + 1, 3), np.uint64)
    want[0, top] = (n, n * top, n * top * top)
    want[1, 0] = (n, n * top, n * top * top)
    want[2, top] = (n - 1, (n - 1) * top, (n - 1) * top * top)
    want[2, 5] = (1, top, top * top)
    want[3, top] = (n, (n - 1) * top + 5, (n - 1) * top * top + 25)
    assert np.array_equal(got, want)
    assert np.array_equal(want, R.level_stats([full, zero, one, full], [full, full, full, one], bpc))
    if bpc == 12:
        assert int(got[0, top, 1]) > 1 << 32


@pytest.mark.parametrize("bpc", [8, 10])
@pytest.mark.parametrize("run", [64, 2])
def test_contention_patterns(bpc, run):
    """runs of equal reference level: 64 pixels (wave-uniform for a lane per sample) and 2; 200 x 37, so the runs straddle
    row ends and load boundaries; the capture is random"""
    rng = np.random.default_rng(40 + bpc + run)
    w, h, L = 200, 37, 1 << bpc
    n_runs = -(-w * h // run)
    ref = [np.repeat(rng.integers(0, L, n_runs), run)[:w * h].reshape(h, w).astype(_dt(bpc)) for _ in range(2)]
    ref[1][:] = np.repeat(rng.integers(L - 2, L, n_runs), run)[:w * h].reshape(h, w)     # two levels only: near-flat
    dis = [rng.integers(0, L, (h, w)).astype(_dt(bpc)) for _ in range(2)]
    with _engine(w, h, bpc) as eng:
        assert np.array_equal(eng.level_stats(ref, dis), R.level_stats(ref, dis, bpc))


def test_more_frames_than_one_launch_chunk():
    ref, dis = R.random_pair(50, 9, 48, 32)
    want = R.level_stats(ref, dis, 8)
    assert len({want[f].tobytes() for f in range(9)}) == 9
    rbuf, _ = _padded(ref, pad=0, lead=0)
    dbuf, _ = _padded(dis, pad=0, lead=0)
    with _engine(48, 32) as eng:
        assert np.array_equal(eng.level_stats(ref, dis), want)
        assert np.array_equal(_resident(eng, rbuf, dbuf, 0, 9), want)


@pytest.mark.parametrize("bpc", [8, 10])
def test_sse_identity_against_the_psnr_feature(bpc):
    """sum_v (T2 - 2 v T1 + v^2 T0) of each frame is the luma SSE the same context returns through submit / collect"""
    from pqa2_amd import _native as N
    ref, dis = R.random_pair(60 + bpc, 3, 80, 48, bpc)
    with _engine(80, 48, bpc) as eng:
        T = eng.level_stats(ref, dis)
        for i in range(3):
            eng.submit(i, [ref[i]], [dis[i]])
        rec = eng.collect(0, 3)
    assert np.array_equal(T, R.level_stats(ref, dis, bpc))
    sse = [int(x) for x in rec[:, N.REC_SSE].view(np.uint64)]
    assert R.table_sse(T) == sse
    assert sse == [int(((r.astype(np.int64) - d.astype(np.int64)) ** 2).sum()) for r, d in zip(ref, dis)]


def test_independent_of_the_scoring_chain():
    from pqa2_amd import _native as N
    rng = np.random.default_rng(7)
    ref = [rng.integers(0, 256, (48, 64)).astype(np.uint8) for _ in range(6)]
    dis = [np.clip(r.astype(int) + rng.integers(-9, 10, r.shape), 0, 255).astype(np.uint8) for r in ref]

    def run(with_call):
        with _engine(64, 48, features=N.FEAT_VMAF | N.FEAT_PSNR | N.FEAT_SSIM, max_batch=4) as eng:
            tabs = []
            for i in range(6):
                eng.submit(i, [ref[i]], [dis[i]])
                if with_call and i in (0, 2, 4):    # inside a pending batch, and right after one was launched
                    tabs.append(eng.level_stats(ref, dis))
                    tabs.append(eng.level_stats(ref, dis))
            return eng.collect(0, 6), tabs
    plain, _ = run(False)
    mixed, tabs = run(True)
    assert np.array_equal(plain.view(np.uint64), mixed.view(np.uint64))
    want = R.level_stats(ref, dis, 8)
    assert len(tabs) == 6 and all(np.array_equal(t, want) for t in tabs)


# ---- end to end -----------------------------------------------------------------------------------------------------------
W, H, N_FRAMES = 96, 64, 6


def _info():
    from pqa2_amd.yuvio import VideoInfo
    return VideoInfo(width=W, height=H, fps_num=24, fps_den=1, bit_depth=8, mono=False, hshift=1, vshift=1, chroma_tag="420")


def _write_pairs(tmp_path):
    """a limited-range 4:2:0 reference (luma 16 ... 235, chroma 16 ... 240), its capture expanded to full range (case (b):
    luma 255/219 about 16, chroma 255/224 about 128, rounded), and the capture mapped back by hand with the tables"""
    from pqa2_amd import align as AL
    from pqa2_amd.yuvio import write_y4m
    ref, cap, back = [], [], []
    luts = [AL.level_lut(*AL.named_level_map("limited_to_full", 8, chroma=p > 0), 8) for p in range(3)]
    for t in range(N_FRAMES):
        planes = [R.smooth_field(70 + t, W, H, 16, 235, t)] + [R.smooth_field(80 + 7 * p + t, W // 2, H // 2, 16, 240, t)
                                                               for p in range(2)]
        moved = [R.apply_map(planes[0], *R.L2F)] + [R.apply_map(c, 255.0 / 224.0, 128.0 * (1 - 255.0 / 224.0)) for c in planes[1:]]
        ref.append(planes)
        cap.append(moved)
        back.append([R.apply_lut(m, lut) for m, lut in zip(moved, luts)])
    paths = {}
    for key, clip in (("ref", ref), ("dis", cap), ("dis_back", back)):
        paths[key] = str(tmp_path / (key + ".y4m"))
        write_y4m(paths[key], clip, _info())
    return paths


def test_end_to_end_report_and_apply(tmp_path):
    from pqa2_amd.pipeline import score_files
    p = _write_pairs(tmp_path)
    plain = score_files(p["ref"], p["dis"], "vmaf_v0.6.1")
    rep = score_files(p["ref"], p["dis"], "vmaf_v0.6.1", level_align="report")
    lv = rep["alignment"]["levels"]
    assert (lv["kind"], lv["mismatch"], lv["applied"], lv["frames"], lv["degenerate"]) == ("limited_to_full", True, False, N_FRAMES, False)
    assert set(lv["planes"]) == {"y", "u", "v"} and all(q["kind"] == "limited_to_full" and q["mismatch"] for q in lv["planes"].values())
    assert "alignment" not in plain and np.array_equal(rep["records"].view(np.uint64), plain["records"].view(np.uint64))
    done = score_files(p["ref"], p["dis"], "vmaf_v0.6.1", level_align="apply")
    assert all(q["applied"] for q in done["alignment"]["levels"]["planes"].values()) and done["alignment"]["levels"]["applied"]
    by_hand = score_files(p["ref"], p["dis_back"], "vmaf_v0.6.1")
    assert done["records"].shape == by_hand["records"].shape == (N_FRAMES, 24)
    assert np.array_equal(done["records"].view(np.uint64), by_hand["records"].view(np.uint64))
    assert not np.array_equal(done["records"].view(np.uint64), plain["records"].view(np.uint64))
    for k in done["metrics"]:
        assert np.array_equal(np.asarray(done["metrics"][k]), np.asarray(by_hand["metrics"][k])), k


def test_identity_pair_is_scored_unchanged(tmp_path):
    from pqa2_amd.pipeline import score_files
    p = _write_pairs(tmp_path)
    plain = score_files(p["ref"], p["dis_back"], "vmaf_v0.6.1")
    same = score_files(p["ref"], p["dis_back"], "vmaf_v0.6.1", level_align="apply")
    lv = same["alignment"]["levels"]
    assert (lv["kind"], lv["mismatch"], lv["applied"]) == ("identity", False, False)
    assert not any(q["applied"] for q in lv["planes"].values())
    assert np.array_equal(same["records"].view(np.uint64), plain["records"].view(np.uint64))


def test_analyzer_corrects_and_writes_the_levels_object(tmp_path):
    from pqa2_amd.pipeline import score_files
    from pqa2_amd.vmaf_analyzer import VMAFAnalyzer
    p = _write_pairs(tmp_path)
    an = VMAFAnalyzer()
    an.set_output_directory(str(tmp_path))
    an.set_test_name("levels")
    an.set_advanced_options(level_correct_enabled=True)
    lines = []
    an.status_update.connect(lines.append)
    results = an.analyze_videos(p["ref"], p["dis"])
    assert results and results["alignment"]["levels"]["kind"] == "limited_to_full"
    lv = json.load(open(results["json_path"]))["alignment"]["levels"]
    assert lv["applied"] is True and lv["mismatch"] is True and lv["frames"] == N_FRAMES and set(lv["planes"]) == {"y", "u", "v"}
    assert len(results["raw_results"]["frames"]) == N_FRAMES
    assert any("expanded from limited to full range" in s and "corrected on Y, U, V" in s for s in lines)
    by_hand = score_files(p["ref"], p["dis_back"], "vmaf_v0.6.1")
    want = [float(v) for v in by_hand["metrics"]["vmaf"]]
    got = [fr["metrics"]["vmaf"] for fr in results["raw_results"]["frames"]]
    assert got == pytest.approx(want, abs=1e-6)     # the log is written with six decimals
