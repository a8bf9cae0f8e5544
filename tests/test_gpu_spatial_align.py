"""Spatial alignment on the MI355X (csrc/shift_sse.hip, pqa_shift_sse / pqa_shift_sse_device): the shifted-window luma SSE
equals the numpy restatement (tests/spatial_align_ref.py) as integers -- smallest call, row tails / pitches / odd base
addresses at 8 / 10 / 12 bit, partial tiles in x and y at the widest search, sign and transpose, the accumulator limits at
the sample extremes; the calls leave the scoring chain alone; and displaced Y4M pairs through score_files(spatial_align=)
and VMAFAnalyzer give the records of the clips cropped by hand."""
import json

import numpy as np
import pytest

from tests import spatial_align_ref as R

pytestmark = pytest.mark.gpu


def _engine(w, h, bpc=8, **kw):
    from pqa2_amd import _native as N
    from pqa2_amd.engine import FeatureEngine
    return FeatureEngine(w, h, bit_depth=bpc, n_planes=1, features=kw.pop("features", N.FEAT_PSNR), **kw)


def _padded(frames, pad=5, lead=1):
    """the same frames as views into one buffer: rows `pad` samples longer than a row, base `lead` samples in"""
    h, w = frames[0].shape
    buf = np.zeros((len(frames), h, w + pad), frames[0].dtype)
    buf[:, :, lead:lead + w] = np.stack(frames)
    return buf, [buf[i, :, lead:lead + w] for i in range(len(frames))]


def _resident(eng, ref_buf, dis_buf, lead, n, radius):
    import torch
    es = ref_buf.dtype.itemsize
    tr = torch.from_numpy(ref_buf.view(np.uint8).reshape(-1)).cuda()
    td = torch.from_numpy(dis_buf.view(np.uint8).reshape(-1)).cuda()
    torch.cuda.synchronize()
    return eng.shift_sse_resident(tr.data_ptr() + lead * es, ref_buf.strides[1], ref_buf.strides[0], td.data_ptr() + lead * es,
                                  dis_buf.strides[1], dis_buf.strides[0], n, radius)


def test_smallest_call_and_argument_rules():
    """One summed pixel: a context is at least 16 x 16 (pqa_create), so the 3 x 3 frame at R = 1 is not reachable; the
    one-pixel window is 17 x 17 at R = 8 instead.  R = 0 on 16 x 16, n_frames = 0, and the PQA_EINVAL cases."""
    from pqa2_amd import _native as N
    with _engine(17, 17) as eng:
        r17, d17 = R.random_pair(4, 2, 17, 17)
        got = eng.shift_sse(r17, d17, 8)
        assert got.dtype == np.uint64 and got.shape == (2, 17, 17) and np.array_equal(got, R.shift_sse(r17, d17, 8))
        assert int(got[1, 3, 5]) == (int(r17[1][8, 8]) - int(d17[1][3, 5])) ** 2
    with _engine(16, 16) as eng:
        r16, d16 = R.random_pair(2, 2, 16, 16)
        got = eng.shift_sse(r16, d16, 0)
        assert got.shape == (2, 1, 1) and np.array_equal(got, R.shift_sse(r16, d16, 0))
        assert eng.shift_sse([], [], 2).shape == (0, 5, 5)
        assert np.array_equal(eng.shift_sse(r16, d16, 7), R.shift_sse(r16, d16, 7))    # a 2 x 2 window
        for bad in (17, -1, 8):    # outside 0 ... 16; 16 is not larger than 2 * 8
            with pytest.raises(N.PqaError) as e:
                eng.shift_sse(r16, d16, bad)
            assert e.value.code == N.PQA_EINVAL
    with _engine(32, 32) as eng:
        r32, d32 = R.random_pair(3, 1, 32, 32)
        with pytest.raises(N.PqaError) as e:
            eng.shift_sse(r32, d32, 16)
        assert e.value.code == N.PQA_EINVAL
        assert np.array_equal(eng.shift_sse(r32, d32, 15), R.shift_sse(r32, d32, 15))


@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_tails_pitches_and_depths(bpc):
    """50 x 18, R = 3: a row is no whole number of strips; rows padded by 5 samples, base one sample in; the host entry on
    contiguous frames, on views, and the resident entry agree; one 64-byte-aligned layout with a row tail"""
    ref, dis = R.random_pair(10 + bpc, 3, 50, 18, bpc)
    want = R.shift_sse(ref, dis, 3)
    rbuf, rv = _padded(ref)
    dbuf, dv = _padded(dis)
    with _engine(50, 18, bpc) as eng:
        assert np.array_equal(eng.shift_sse(ref, dis, 3), want)
        assert np.array_equal(eng.shift_sse(rv, dv, 3), want)
        assert np.array_equal(_resident(eng, rbuf, dbuf, 1, 3, 3), want)
        abuf, _ = _padded(ref, pad=14, lead=0)      # 64-byte rows at 8 bit, 128-byte rows at 16: the word loads, with a row tail
        bbuf, _ = _padded(dis, pad=14, lead=0)
        assert np.array_equal(_resident(eng, abuf, bbuf, 0, 3, 3), want)
        assert np.array_equal(eng.shift_sse(ref, dis, 4), R.shift_sse(ref, dis, 4))   # R a whole number of words: aligned window


@pytest.mark.parametrize("bpc,w,h", [(8, 161, 289), (10, 97, 289), (8, 200, 300)])
def test_tile_edges(bpc, w, h):
    """the widest search, R = 16.  The tile is 128 x 256 window pixels at 8 bit and 64 x 256 at 10 / 12 bit, larger than
    200 x 120, so the smallest geometry with two tiles each way and partial last tiles: 161 x 289 (window 129 x 257) at
    8 bit, 97 x 289 (window 65 x 257) at 10 bit -- last tiles one pixel wide and high; 200 x 300 for last tiles that are
    no whole number of strips; 3 frames for the per-frame output stride"""
    ref, dis = R.random_pair(20 + bpc, 3, w, h, bpc)
    want = R.shift_sse(ref, dis, 16)
    with _engine(w, h, bpc) as eng:
        got = eng.shift_sse(ref, dis, 16)
    assert got.shape == (3, 33, 33) and np.array_equal(got, want)


def test_sign_and_transpose():
    from pqa2_amd import align as AL
    ref, dis = R.shifted_pair(31, 3, 96, 64, 3, -2)
    with _engine(96, 64) as eng:
        S = eng.shift_sse(ref, dis, 4)
    assert np.array_equal(S, R.shift_sse(ref, dis, 4))
    for f in range(3):
        assert S[f, 4 - 2, 4 + 3] == 0
        rest = S[f].copy()
        rest[4 - 2, 4 + 3] = 1
        assert (rest > 0).all()
    b = AL.best_shift(S, 4, (96 - 8) * (64 - 8))
    assert (b["dx"], b["dy"], b["agreement"], b["at_edge"]) == (3, -2, 1.0, False) and b["confidence"] == float("inf")


@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_accumulator_limits_at_the_extremes(bpc):
    """512 x 288 at R = 2: 144 272 summed pixels, more than an i32 takes of centred 8-bit products (131 071) and far more
    than the 256 twelve-bit squares"""
    dt, top = (np.uint8 if bpc == 8 else np.uint16), (1 << bpc) - 1
    zero, full = np.zeros((288, 512), dt), np.full((288, 512), top, dt)
    with _engine(512, 288, bpc) as eng:
        got = eng.shift_sse([zero, zero], [full, zero], 2)
        assert got[0].tolist() == [[(512 - 4) * (288 - 4) * top * top] * 5] * 5
        assert got[1].tolist() == [[0] * 5] * 5
        assert eng.shift_sse([full], [zero], 2)[0].tolist() == [[(512 - 4) * (288 - 4) * top * top] * 5] * 5
        assert eng.shift_sse([full], [full], 2)[0].tolist() == [[0] * 5] * 5


def test_independent_of_the_scoring_chain():
    from pqa2_amd import _native as N
    rng = np.random.default_rng(7)
    ref = [rng.integers(0, 256, (48, 64)).astype(np.uint8) for _ in range(6)]
    dis = [np.clip(r.astype(int) + rng.integers(-9, 10, r.shape), 0, 255).astype(np.uint8) for r in ref]

    def run(with_call):
        with _engine(64, 48, features=N.FEAT_VMAF | N.FEAT_PSNR | N.FEAT_SSIM, max_batch=4) as eng:
            mats = []
            for i in range(6):
                eng.submit(i, [ref[i]], [dis[i]])
                if with_call and i in (0, 2, 4):    # inside a pending batch, and right after one was launched
                    mats.append(eng.shift_sse(ref, dis, 2))
                    mats.append(eng.shift_sse(ref, dis, 2))
            return eng.collect(0, 6), mats
    plain, _ = run(False)
    mixed, mats = run(True)
    assert np.array_equal(plain.view(np.uint64), mixed.view(np.uint64))
    want = R.shift_sse(ref, dis, 2)
    assert len(mats) == 6 and all(np.array_equal(m, want) for m in mats)


# ---- end to end -----------------------------------------------------------------------------------------------------------
W, H, N_FRAMES = 80, 64, 6


def _info(w, h, mono):
    from pqa2_amd.yuvio import VideoInfo
    return VideoInfo(width=w, height=h, fps_num=24, fps_den=1, bit_depth=8, mono=mono, hshift=0 if mono else 1,
                     vshift=0 if mono else 1, chroma_tag="mono" if mono else "420")


def _write_displaced(tmp_path, dx, dy, mono):
    """reference, the capture displaced by (dx, dy) in luma ((dx / 2, dy / 2) in 4:2:0 chroma) plus coding noise, and both
    cut by hand to the common window"""
    from pqa2_amd.yuvio import write_y4m
    frames = R.natural_planes(41, N_FRAMES, W, H, 0 if mono else 1, 0 if mono else 1, mono)
    rng = np.random.default_rng(42)
    cap = []
    for planes in frames:
        out = []
        for p, plane in enumerate(planes):
            sx, sy = (dx, dy) if p == 0 else (dx // 2, dy // 2)
            moved = R.shift_plane(plane, sx, sy, rng, 255)
            out.append(np.clip(moved.astype(int) + rng.integers(-3, 4, moved.shape), 0, 255).astype(np.uint8))
        cap.append(out)
    wc, hc, x0, y0 = W - abs(dx), H - abs(dy), max(0, -dx), max(0, -dy)

    def cut(planes, ox, oy):
        out = [planes[0][oy:oy + hc, ox:ox + wc]]
        for c in planes[1:]:
            out.append(c[oy >> 1:(oy >> 1) + (-(-hc >> 1)), ox >> 1:(ox >> 1) + (-(-wc >> 1))])
        return out
    paths = {}
    for key, clip, info in (("ref", frames, _info(W, H, mono)), ("dis", cap, _info(W, H, mono)),
                            ("ref_cut", [cut(f, x0, y0) for f in frames], _info(wc, hc, mono)),
                            ("dis_cut", [cut(f, x0 + dx, y0 + dy) for f in cap], _info(wc, hc, mono))):
        paths[key] = str(tmp_path / (key + ".y4m"))
        write_y4m(paths[key], clip, info)
    return paths


def test_end_to_end_luma_only(tmp_path):
    from pqa2_amd.pipeline import score_files
    p = _write_displaced(tmp_path, 3, -1, mono=True)
    res = score_files(p["ref"], p["dis"], "vmaf_v0.6.1", spatial_align=4)
    sp = res["alignment"]["spatial"]
    assert (sp["dx"], sp["dy"], sp["applied"], sp["at_edge"], sp["searched"], sp["frames"]) == (3, -1, True, False, 4, N_FRAMES)
    assert sp["agreement"] == 1.0 and sp["chroma_exact"] is True and "offset_frames" not in res["alignment"]
    by_hand = score_files(p["ref_cut"], p["dis_cut"], "vmaf_v0.6.1")
    assert res["records"].shape == by_hand["records"].shape == (N_FRAMES, 24)
    assert np.array_equal(res["records"].view(np.uint64), by_hand["records"].view(np.uint64))
    assert "alignment" not in by_hand


def test_end_to_end_420_with_psnr(tmp_path):
    from pqa2_amd.pipeline import score_files
    p = _write_displaced(tmp_path, 2, -2, mono=False)
    res = score_files(p["ref"], p["dis"], "vmaf_v0.6.1", spatial_align=4)
    sp = res["alignment"]["spatial"]
    assert (sp["dx"], sp["dy"], sp["applied"], sp["chroma_exact"]) == (2, -2, True, True)
    by_hand = score_files(p["ref_cut"], p["dis_cut"], "vmaf_v0.6.1")
    assert np.array_equal(res["records"].view(np.uint64), by_hand["records"].view(np.uint64))
    assert list(res["metrics"]) == list(by_hand["metrics"]) and "psnr_cb" in res["metrics"]
    for k in res["metrics"]:
        assert np.array_equal(np.asarray(res["metrics"][k]), np.asarray(by_hand["metrics"][k])), k


def test_negative_controls(tmp_path):
    from pqa2_amd.pipeline import score_files
    p = _write_displaced(tmp_path, 4, 0, mono=True)
    same = score_files(p["ref"], p["ref"], "vmaf_v0.6.1", spatial_align=4)
    sp = same["alignment"]["spatial"]
    assert (sp["dx"], sp["dy"], sp["applied"], sp["at_edge"]) == (0, 0, False, False) and sp["confidence"] == float("inf")
    plain = score_files(p["ref"], p["ref"], "vmaf_v0.6.1")
    assert np.array_equal(same["records"].view(np.uint64), plain["records"].view(np.uint64))
    edge = score_files(p["ref"], p["dis"], "vmaf_v0.6.1", spatial_align=4)
    sp = edge["alignment"]["spatial"]
    assert (sp["dx"], sp["dy"], sp["at_edge"], sp["applied"]) == (4, 0, True, False)
    assert sp["subpixel_dx"] is None and sp["subpixel_dy"] is None
    plain = score_files(p["ref"], p["dis"], "vmaf_v0.6.1")
    assert edge["records"].shape == (N_FRAMES, 24)
    assert np.array_equal(edge["records"].view(np.uint64), plain["records"].view(np.uint64))


def test_analyzer_writes_the_spatial_object(tmp_path):
    from pqa2_amd.vmaf_analyzer import VMAFAnalyzer
    p = _write_displaced(tmp_path, 3, -1, mono=True)
    an = VMAFAnalyzer()
    an.set_output_directory(str(tmp_path))
    an.set_test_name("spatial")
    an.set_advanced_options(spatial_align_enabled=True, spatial_align_radius=4)
    lines = []
    an.status_update.connect(lines.append)
    results = an.analyze_videos(p["ref"], p["dis"])
    assert results and results["alignment"]["spatial"]["dx"] == 3 and results["alignment"]["spatial"]["dy"] == -1
    sp = json.load(open(results["json_path"]))["alignment"]["spatial"]
    assert sp["applied"] is True and sp["searched"] == 4 and sp["frames"] == N_FRAMES
    assert len(results["raw_results"]["frames"]) == N_FRAMES
    assert any("displaced by (+3, -1) px" in s for s in lines)
