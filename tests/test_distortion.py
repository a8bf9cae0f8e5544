"""The distortion map on the host (no GPU): the numpy restatement of the tile moments (tests/tile_ref.py) against a plain loop,
pqa2_amd/distortion.py against its evaluation in fractions.Fraction and on planted defects, each rule of the defect finder in
isolation, and score_files(distortion_map=) -- result, JSON, files, a sharded gloo run, CLI and analyzer -- through the
oracle stand-in."""
import io
import json
import os
import socket
import sys
from fractions import Fraction

import numpy as np
import pytest

from tests import tile_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, T, FRAMES = 96, 64, 16, 10


def _tile_engine():
    from tests.fake_engine import OracleEngine

    class TileEngine(OracleEngine):
        """the oracle stand-in plus the restated tile moments"""

        def tile_moments(self, ref_frames, dis_frames, tile=32):
            return R.tile_moments(list(ref_frames), list(dis_frames), tile, self.bpc)
    return TileEngine


def _noisy_clip(n=FRAMES, w=W, h=H, seed=3, sigma=2.0):
    """n luma pairs: uniform noise, and the same plus Gaussian noise of `sigma` code values"""
    rng = np.random.default_rng(seed)
    ref = [rng.integers(16, 236, (h, w)).astype(np.uint8) for _ in range(n)]
    dis = [np.clip(np.rint(r + rng.normal(0.0, sigma, r.shape)), 0, 255).astype(np.uint8) for r in ref]
    return ref, dis


def _solve(ref, dis, tile=T, bpc=8, **kw):
    from pqa2_amd import distortion as DM
    h, w = ref[0].shape
    M = R.tile_moments(ref, dis, tile, bpc)
    S, counts = DM.tile_sse(M), DM.tile_counts(w, h, tile)
    hot = DM.hot_tiles(S, counts, tile=tile, bit_depth=bpc, **kw)
    return S, counts, hot, DM.find_defects(S, counts, tile=tile, bit_depth=bpc, width=w, height=h, **kw)


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def test_restatement_against_a_double_loop():
    rng = np.random.default_rng(1)
    r = rng.integers(0, 1024, (11, 19)).astype(np.uint16)
    d = rng.integers(0, 1024, (11, 19)).astype(np.uint16)
    d[2, 3] = 60000      # above 1023: read as 1023
    M = R.tile_moments([r], [d], 8, 10)
    assert M.dtype == np.uint64 and M.shape == (1, 2, 3, 6)
    want = np.zeros((2, 3, 6), object)
    for y in range(11):
        for x in range(19):
            a, b = min(int(r[y, x]), 1023), min(int(d[y, x]), 1023)
            want[y // 8, x // 8] += np.array([a, b, a * a, b * b, a * b, abs(b - a)], object)
    assert M[0].tolist() == want.tolist()
    assert R.counts(19, 11, 8) == [[64, 64, 24], [24, 24, 9]]


# ---- tile_counts, tile_metrics, frame_summary ------------------------------------------------------------------------------------
def test_tile_counts():
    from pqa2_amd import distortion as DM
    for w, h, t in ((19, 11, 8), (64, 64, 64), (65, 63, 64), (1, 1, 8), (200, 70, 32)):
        c = DM.tile_counts(w, h, t)
        assert c.dtype == np.int64 and c.tolist() == R.counts(w, h, t) and int(c.sum()) == w * h
        if c.size > 1:
            assert DM.plane_size(c, t) == (w, h)


@pytest.mark.parametrize("bpc,tile", [(8, 8), (8, 64), (10, 16), (12, 8), (12, 64)])
def test_tile_metrics_against_fractions(bpc, tile):
    """MSE, MAD and PSNR equal the Fraction evaluation; the block SSIM to 1e-12 relative: its four factors are exact integers,
    float64 rounds them, two products and one quotient"""
    from pqa2_amd import distortion as DM
    w, h, top = 150, 70, (1 << bpc) - 1
    ref, dis = R.random_pairs(40 + bpc + tile, 2, w, h, bpc)
    near = R.random_pairs(41 + bpc, 1, w, h, bpc, noise=3)
    full, zero = np.full((h, w), top, ref[0].dtype), np.zeros((h, w), ref[0].dtype)
    ref, dis = ref + near[0] + [full, full, zero], dis + near[1] + [full, zero, zero]
    M = R.tile_moments(ref, dis, tile, bpc)
    got = DM.tile_metrics(M, w, h, tile, bpc)
    n = R.counts(w, h, tile)
    mse, mad, ssim = (np.zeros(M.shape[:3]) for _ in range(3))
    worst = 0.0
    for f in range(M.shape[0]):
        for j in range(M.shape[1]):
            for i in range(M.shape[2]):
                a, b, c = R.block_metrics(M[f, j, i], n[j][i], bpc)
                mse[f, j, i], mad[f, j, i], ssim[f, j, i] = float(a), float(b), float(c)
                worst = max(worst, abs(Fraction(float(got["ssim"][f, j, i])) - c) / abs(c))
    assert all(got[k].dtype == np.float64 and got[k].shape == M.shape[:3] for k in ("mse", "mad", "psnr", "ssim"))
    assert np.array_equal(got["mse"], mse) and np.array_equal(got["mad"], mad)
    assert np.array_equal(got["psnr"], R.psnr_of(mse, bpc))
    assert worst <= 1e-12, float(worst)
    assert np.all(got["ssim"][-3] == 1.0) and np.all(got["ssim"][-1] == 1.0) and np.all(got["psnr"][-3] == 6.0 * bpc + 12.0)
    assert np.all(got["ssim"][3] > 0.9) and np.all(got["ssim"][:2] < 0.5) and np.all(got["ssim"][-2] < 1e-3)
    assert np.all(got["mse"][-2] == top * top) and np.all(got["mad"][-2] == top) and np.all(got["psnr"][-2] == 0.0)


def test_clip_summed_moments_go_through_python_ints():
    from pqa2_amd import distortion as DM
    ref, dis = R.random_pairs(9, 3, 40, 24, 12)
    M = R.tile_moments(ref, dis, 8, 12)
    total = M.sum(axis=0, dtype=np.uint64)
    got = DM.tile_metrics(total, 40, 24, 8, 12, frames=3)
    for j in range(3):
        for i in range(5):
            a, b, c = R.block_metrics(total[j, i], 64 * 3, 12)
            assert got["mse"][j, i] == float(a) and got["mad"][j, i] == float(b) and got["ssim"][j, i] == float(c)


def test_the_tiles_add_up_to_the_engines_sse():
    from pqa2_amd import _native as N
    from pqa2_amd import distortion as DM
    from pqa2_amd.engine import sse_from_records
    ref, dis = _noisy_clip(3)
    eng = _tile_engine()(W, H, features=N.FEAT_VMAF | N.FEAT_PSNR)
    for i in range(3):
        eng.submit(i, [ref[i]], [dis[i]])
    sse = sse_from_records(eng.collect(0, 3))[:, 0]
    for tile in (8, 64):
        S = DM.tile_sse(eng.tile_moments(ref, dis, tile))
        assert S.dtype == np.uint64 and [int(v) for v in S.sum(axis=(1, 2), dtype=np.uint64)] == [int(v) for v in sse]


def test_frame_summary():
    from pqa2_amd import distortion as DM
    S = np.full((3, 4, 6), 256, np.uint64)      # 24 tiles of 16 x 16: MSE 1 everywhere
    S[1, 2, 3] = 256 * 100
    S[2] = 0
    got = DM.frame_summary(S, W, H, T, 8)
    p1, p100 = float(R.psnr_of(np.array([1.0]), 8)[0]), float(R.psnr_of(np.array([100.0]), 8)[0])
    assert got["tile_psnr_min"].tolist() == [p1, p100, 60.0]
    assert got["tile_psnr_min_at"].tolist() == [[0, 0], [3, 2], [0, 0]]
    assert got["concentration"].tolist() == [2 / 24, (100 + 1) / (100 + 23), 0.0]      # ceil(24 / 16) = 2 tiles
    M = R.tile_moments(*_noisy_clip(2), T)
    again = DM.frame_summary(M, W, H, T, 8)
    assert np.array_equal(again["tile_psnr_min"], DM.frame_summary(DM.tile_sse(M), W, H, T, 8)["tile_psnr_min"])


# ---- find_defects and persistent_regions on planted damage --------------------------------------------------------------------
def test_a_clean_noisy_clip_has_no_defect():
    ref, dis = _noisy_clip()
    S, counts, hot, events = _solve(ref, dis)
    assert not hot.any() and events == []
    assert 3.0 < float(S.sum()) / (W * H * FRAMES) < 5.5      # sigma 2: an MSE near 4, the min_mse rule alone would fire


def test_an_inverted_patch_is_one_event():
    ref, dis = _noisy_clip()
    x0, y0, pw, ph = 20, 10, 40, 24
    for f in (5, 6, 7):
        dis[f][y0:y0 + ph, x0:x0 + pw] = 255 - dis[f][y0:y0 + ph, x0:x0 + pw]
    S, counts, hot, events = _solve(ref, dis)
    assert len(events) == 1
    ev = events[0]
    assert (ev["first"], ev["last"], ev["frames"]) == (5, 7, 3) and ev["peak_frame"] in (5, 6, 7)
    assert ev["box"] == [x0 // T * T, y0 // T * T, -(-(x0 + pw) // T) * T, -(-(y0 + ph) // T) * T] == [16, 0, 64, 48]
    assert ev["share"] > 0.99 and ev["peak_mse"] > 1000
    from pqa2_amd import distortion as DM
    pers = DM.persistent_regions(hot, S, counts, tile=T, width=W, height=H)
    assert pers["regions"] == [] and pers["psnr_excluding"] == pers["psnr_all"]


def test_a_burnt_in_logo_is_persistent():
    from pqa2_amd import distortion as DM
    ref, dis = _noisy_clip()
    for d in dis:
        d[16:48, 16:80] = 235      # 64 x 32, on the tile grid
    S, counts, hot, events = _solve(ref, dis)
    pers = DM.persistent_regions(hot, S, counts, tile=T, width=W, height=H)
    assert [r["box"] for r in pers["regions"]] == [[16, 16, 80, 48]] and pers["regions"][0]["tiles"] == 8 == pers["tiles"]
    assert pers["regions"][0]["frames_hot_min"] == FRAMES
    assert pers["psnr_excluding"] > pers["psnr_all"] + 10
    total, pix = sum(int(v) for v in S.ravel()), W * H * FRAMES
    inside = sum(int(v) for v in S[:, 1:3, 1:5].ravel())
    assert pers["psnr_all"] == float(R.psnr_of(np.array([total / pix]), 8)[0])
    assert pers["psnr_excluding"] == float(R.psnr_of(np.array([(total - inside) / (pix - 64 * 32 * FRAMES)]), 8)[0])
    assert len(events) == 1 and (events[0]["first"], events[0]["last"], events[0]["box"]) == (0, FRAMES - 1, [16, 16, 80, 48])
    # hot in 8 of 10 frames is not 0.9 of them; in 9 of 10 it is (9/10, not the float's binary neighbour above it)
    for gone, found in ((2, 0), (1, 1)):
        part = hot.copy()
        part[:gone] = False
        assert len(DM.persistent_regions(part, S, counts, tile=T, width=W, height=H)["regions"]) == found


# ---- one rule at a time --------------------------------------------------------------------------------------------------------
def _flat(n, ty, tx, value):
    return np.full((n, ty, tx), value, np.uint64)


def test_the_factor_rule_alone():
    from pqa2_amd import distortion as DM
    counts = DM.tile_counts(32, 32, 8)      # 16 full tiles of 64 pixels
    S = _flat(2, 4, 4, 640)                 # MSE 10 everywhere: far above min_mse
    S[0, 1, 2] = 16 * 640                   # exactly 16 times the median: not more
    S[1, 1, 2] = 16 * 640 + 1
    hot = DM.hot_tiles(S, counts, tile=8)
    assert not hot[0].any() and np.argwhere(hot[1]).tolist() == [[1, 2]]
    assert DM.hot_tiles(S, counts, tile=8, factor=8)[0, 1, 2] and not DM.hot_tiles(S, counts, tile=8, factor=17).any()
    assert DM.hot_tiles(S, counts, tile=8, factor=15.5)[0, 1, 2]
    # an edge tile is judged by its own pixel count: 24 pixels at 16 times the median MSE and one more
    counts = DM.tile_counts(19, 16, 8)
    S = _flat(1, 2, 3, 640)
    S[0, :, 2] = 16 * 10 * 24
    assert not DM.hot_tiles(S, counts, tile=8).any()
    S[0, 1, 2] += 1
    assert np.argwhere(DM.hot_tiles(S, counts, tile=8)[0]).tolist() == [[1, 2]]


@pytest.mark.parametrize("bpc,bound", [(8, 256), (10, 4120), (12, 66018)])
def test_the_min_mse_rule_alone(bpc, bound):
    """identical frames but one tile: the median is 0, the factor rule passes anything, and min_mse (4 in 8-bit code values
    squared) times (top / 255)^2 times 64 pixels decides: 256, 4120.09..., 66018.5..."""
    from pqa2_amd import distortion as DM
    top = (1 << bpc) - 1
    assert bound == 4 * top * top * 64 // (255 * 255)
    counts = DM.tile_counts(32, 32, 8)
    S = _flat(2, 4, 4, 0)
    S[0, 3, 0], S[1, 3, 0] = bound, bound + 1
    hot = DM.hot_tiles(S, counts, tile=8, bit_depth=bpc)
    assert not hot[0].any() and np.argwhere(hot[1]).tolist() == [[3, 0]]
    assert DM.hot_tiles(S, counts, tile=8, bit_depth=bpc, min_mse=0)[0, 3, 0]


def test_the_event_join():
    from pqa2_amd import distortion as DM
    counts = DM.tile_counts(32, 32, 8)
    S = _flat(7, 4, 4, 64)
    hot = np.zeros(S.shape, bool)
    hot[0, 0, 0] = hot[1, 0, 0] = hot[1, 0, 1] = hot[2, 0, 1] = True      # frames 0-2 hand on through a shared tile
    hot[4, 0, 1] = True                                                   # a frame without it in between: a new event
    hot[5, 1, 2] = True                                                   # diagonal to (0, 1): shares no tile
    hot[6, 1, 2] = hot[6, 1, 3] = True
    S[1, 0, 1] = 6400
    events = DM.find_defects(S, counts, tile=8, hot=hot)
    assert [(e["first"], e["last"], e["frames"], e["box"]) for e in events] == [
        (0, 2, 3, [0, 0, 16, 8]), (4, 4, 1, [8, 0, 16, 8]), (5, 6, 2, [16, 8, 32, 16])]
    assert events[0]["peak_frame"] == 1 and events[0]["peak_mse"] == (64 + 6400) / 128
    assert events[0]["share"] == (64 + 6400) / (15 * 64 + 6400)
    # two events that meet in a later frame are one
    hot = np.zeros(S.shape, bool)
    hot[0, 0, 0] = hot[0, 0, 2] = True
    hot[1, 0, 0] = hot[1, 0, 1] = hot[1, 0, 2] = True
    assert [(e["first"], e["last"], e["box"]) for e in DM.find_defects(S, counts, tile=8, hot=hot)] == [(0, 1, [0, 0, 24, 8])]


def test_two_disjoint_components_in_one_frame():
    from pqa2_amd import distortion as DM
    counts = DM.tile_counts(30, 32, 8)      # the last column of tiles is 6 pixels wide
    S = _flat(1, 4, 4, 0)
    S[0, 0, 0] = S[0, 1, 0] = 10000         # a component of two tiles
    S[0, 3, 3] = 5000                       # one tile in the far corner, 6 x 8 pixels
    S[0, 1, 1] = 1                          # below min_mse
    events = DM.find_defects(S, counts, tile=8)
    assert [(e["first"], e["last"], e["box"]) for e in events] == [(0, 0, [0, 0, 8, 16]), (0, 0, [24, 24, 30, 32])]
    assert events[0]["peak_mse"] == 20000 / 128 and events[1]["peak_mse"] == 5000 / 48
    assert events[0]["share"] == 20000 / 25001


def test_heatmap_pgm():
    from pqa2_amd import distortion as DM
    data = DM.heatmap_pgm(np.array([[60.0, 50.0, 35.0], [20.0, 0.0, 49.9]]))
    assert data == b"P5\n3 2\n255\n" + bytes([0, 0, 128, 255, 255, 1])
    with pytest.raises(ValueError):
        DM.heatmap_pgm(np.zeros(4))


# ---- score_files through the oracle stand-in ---------------------------------------------------------------------------------
PATCH = (24, 12, 40, 24)      # x0, y0, width, height


def _write(tmp_path, mono=False, n=FRAMES):
    from pqa2_amd.yuvio import VideoInfo, write_y4m
    info = VideoInfo(width=W, height=H, fps_num=24, fps_den=1, bit_depth=8, mono=mono, hshift=0 if mono else 1,
                     vshift=0 if mono else 1, chroma_tag="mono" if mono else "420")
    ref, dis = _noisy_clip(n)
    x0, y0, pw, ph = PATCH
    for f in (5, 6, 7)[:max(0, n - 5)]:
        dis[f][y0:y0 + ph, x0:x0 + pw] = 255 - dis[f][y0:y0 + ph, x0:x0 + pw]
    rng = np.random.default_rng(8)
    chroma = [[rng.integers(100, 156, (H // 2, W // 2)).astype(np.uint8) for _ in range(2)] for _ in range(n)]
    rp, dp = str(tmp_path / "ref.y4m"), str(tmp_path / "dis.y4m")
    write_y4m(rp, [[ref[t]] + ([] if mono else chroma[t]) for t in range(n)], info)
    write_y4m(dp, [[dis[t]] + ([] if mono else [chroma[t][0], np.minimum(chroma[t][1] + 3, 255).astype(np.uint8)]) for t in range(n)], info)
    return rp, dp


PLANE_KEYS = {"grid", "defects", "persistent", "psnr_all", "psnr_excluding", "concentration_mean", "tile_psnr_min_mean",
              "worst_frame"}


def _log_text(res, tmp_path, name):
    from pqa2_amd import report
    log = report.build_vmaf_log(res["metrics"], 0.0, res["frame_indices"],
                                {"model": res["model_name"], **report.distortion_log_keys(res.get("distortion"))})
    report.write_vmaf_json(str(tmp_path / name), log)
    return open(tmp_path / name).read()


def test_score_files_off_and_on(tmp_path):
    from pqa2_amd import report
    from pqa2_amd.pipeline import score_files
    rp, dp = _write(tmp_path)
    kw = dict(engine_factory=_tile_engine(), psnr=True)
    for bad in (4, 12, 128, -8):
        with pytest.raises(ValueError, match="distortion_map"):
            score_files(rp, dp, "vmaf_v0.6.1", distortion_map=bad, **kw)
    with pytest.raises(ValueError, match="distortion_planes"):
        score_files(rp, dp, "vmaf_v0.6.1", distortion_map=T, distortion_planes="uv", **kw)
    with pytest.raises(ValueError, match="must not be negative"):
        score_files(rp, dp, "vmaf_v0.6.1", distortion_map=T, distortion_min_mse=-1.0, **kw)
    plain = score_files(rp, dp, "vmaf_v0.6.1", **kw)
    off = score_files(rp, dp, "vmaf_v0.6.1", distortion_map=0, distortion_dir=str(tmp_path / "never"), **kw)
    assert "distortion" not in plain and "distortion" not in off and list(off["metrics"]) == list(plain["metrics"])
    assert "tile_psnr_min" not in plain["metrics"] and not os.path.exists(tmp_path / "never")
    text = _log_text(plain, tmp_path, "plain.json")
    assert text == _log_text(off, tmp_path, "off.json") and "distortion" not in text and "tile_psnr_min" not in text
    assert report.distortion_log_keys(None) == {}

    on = score_files(rp, dp, "vmaf_v0.6.1", distortion_map=T, **kw)
    assert np.array_equal(on["records"].view(np.uint64), plain["records"].view(np.uint64))
    assert all(np.array_equal(on["metrics"][k], plain["metrics"][k]) for k in plain["metrics"])
    assert set(on["metrics"]) - set(plain["metrics"]) == {"tile_psnr_min", "distortion_concentration"}
    d = on["distortion"]
    assert set(d) == {"tile", "grid", "planes", "frames"} and (d["tile"], d["grid"], d["frames"]) == (T, [6, 4], FRAMES)
    assert set(d["planes"]) == {"y"} and set(d["planes"]["y"]) == PLANE_KEYS
    y = d["planes"]["y"]
    assert len(y["defects"]) == 1 and (y["defects"][0]["first"], y["defects"][0]["last"]) == (5, 7)
    assert y["defects"][0]["box"] == [16, 0, 64, 48] and y["persistent"] == [] and y["psnr_all"] == y["psnr_excluding"]
    assert y["worst_frame"]["frame"] in (5, 6, 7) and y["worst_frame"]["tile_psnr_min"] == on["metrics"]["tile_psnr_min"].min()
    assert y["tile_psnr_min_mean"] == float(on["metrics"]["tile_psnr_min"].mean())
    assert y["concentration_mean"] == float(on["metrics"]["distortion_concentration"].mean())
    # 24 tiles, so the 2 largest: 2 / 24 of an even error; the patch touches 9 tiles and two of them hold about half of it
    assert np.all(on["metrics"]["distortion_concentration"][5:8] > 0.4) and np.all(on["metrics"]["distortion_concentration"][:5] < 0.12)
    # the clip PSNR of the solver is the one the PSNR feature's exact SSE gives
    from pqa2_amd.engine import sse_from_records
    total = sum(int(v) for v in sse_from_records(on["records"])[:, 0])
    assert y["psnr_all"] == float(R.psnr_of(np.array([total / (W * H * FRAMES)]), 8)[0])
    logged = json.loads(_log_text(on, tmp_path, "on.json"))
    assert logged["distortion"] == json.loads(json.dumps(d)) and "tile_psnr_min" in logged["frames"][0]["metrics"]
    assert "1 localised defects, 0 persistent regions" in report.distortion_summary_line(d)
    sub = score_files(rp, dp, "vmaf_v0.6.1", distortion_map=T, n_subsample=3, **kw)
    assert sub["distortion"] == d and np.array_equal(sub["metrics"]["tile_psnr_min"], on["metrics"]["tile_psnr_min"][::3])


def test_score_files_all_planes_and_files(tmp_path):
    from pqa2_amd import distortion as DM
    from pqa2_amd.pipeline import score_files
    rp, dp = _write(tmp_path)
    out = tmp_path / "maps"
    res = score_files(rp, dp, "vmaf_v0.6.1", distortion_map=8, distortion_planes="all", distortion_dir=str(out),
                      engine_factory=_tile_engine())
    d = res["distortion"]
    assert list(d["planes"]) == ["y", "cb", "cr"] and d["grid"] == d["planes"]["y"]["grid"] == [12, 8]
    assert d["planes"]["cb"]["grid"] == [6, 4] and d["planes"]["cb"]["psnr_all"] == 60.0 and d["planes"]["cr"]["psnr_all"] < 45.0
    assert sorted(os.listdir(out)) == [f"distortion_{p}.{e}" for p in ("cb", "cr", "y") for e in ("npy", "pgm")]
    from pqa2_amd.yuvio import open_video
    rr, dr = open_video(rp), open_video(dp)
    for p, name, (tx, ty) in ((0, "y", (12, 8)), (1, "cb", (6, 4)), (2, "cr", (6, 4))):
        M = R.tile_moments([rr.frame(i)[p] for i in range(FRAMES)], [dr.frame(i)[p] for i in range(FRAMES)], 8)
        total = np.load(out / f"distortion_{name}.npy")
        assert total.dtype == np.uint64 and np.array_equal(total, M.sum(axis=0, dtype=np.uint64))
        data = open(out / f"distortion_{name}.pgm", "rb").read()
        head = b"P5\n%d %d\n255\n" % (tx, ty)
        assert data.startswith(head) and len(data) == len(head) + tx * ty
        mean = DM.tile_metrics(total, W >> (p > 0), H >> (p > 0), 8, 8, frames=FRAMES)["psnr"]
        assert data == DM.heatmap_pgm(mean)
    assert max(open(out / "distortion_y.pgm", "rb").read()[-96:]) > 100 and set(open(out / "distortion_cb.pgm", "rb").read()[-24:]) == {0}


def test_all_planes_of_a_mono_clip_is_an_error(tmp_path):
    from pqa2_amd.pipeline import score_files
    rp, dp = _write(tmp_path, mono=True, n=3)
    with pytest.raises(ValueError, match="monochrome"):
        score_files(rp, dp, "vmaf_v0.6.1", distortion_map=T, distortion_planes="all", engine_factory=_tile_engine())
    assert set(score_files(rp, dp, "vmaf_v0.6.1", distortion_map=T, engine_factory=_tile_engine())["distortion"]["planes"]) == {"y"}


def _worker(rank, world, port, rp, dp, out_path):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from pqa2_amd.pipeline import score_files
    res = score_files(rp, dp, "vmaf_v0.6.1", rank=rank, world_size=world, engine_factory=_tile_engine(), distortion_map=T,
                      distortion_planes="all", distortion_dir=os.path.dirname(out_path))
    if rank == 0:
        with open(out_path, "w") as f:
            json.dump({"distortion": res["distortion"], "tile_psnr_min": res["metrics"]["tile_psnr_min"].tolist(),
                       "concentration": res["metrics"]["distortion_concentration"].tolist()}, f)
    else:
        assert res is None
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_equals_single_process(tmp_path, world):
    import torch.multiprocessing as mp
    from pqa2_amd.pipeline import score_files
    rp, dp = _write(tmp_path)
    single = score_files(rp, dp, "vmaf_v0.6.1", engine_factory=_tile_engine(), distortion_map=T, distortion_planes="all",
                         distortion_dir=str(tmp_path / "single"))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    os.makedirs(tmp_path / "sharded")
    out = str(tmp_path / "sharded" / "res.json")
    mp.spawn(_worker, args=(world, port, rp, dp, out), nprocs=world, join=True)
    got = json.load(open(out))
    assert got["distortion"] == json.loads(json.dumps(single["distortion"]))      # the event in frames 5-7 crosses a shard seam
    assert got["tile_psnr_min"] == single["metrics"]["tile_psnr_min"].tolist()
    assert got["concentration"] == single["metrics"]["distortion_concentration"].tolist()
    for name in ("distortion_y.npy", "distortion_cr.npy", "distortion_y.pgm"):
        assert open(tmp_path / "sharded" / name, "rb").read() == open(tmp_path / "single" / name, "rb").read()


# ---- CLI and analyzer --------------------------------------------------------------------------------------------------------
def test_score_cli_flags_reach_score_files(monkeypatch, tmp_path):
    from pqa2_amd import pipeline, score
    seen = []

    def fake(*a, **kw):
        seen.append(kw)
        raise RuntimeError("stop")

    monkeypatch.setattr(pipeline, "score_files", fake)
    monkeypatch.setattr(score, "_die_with_parent", lambda *a, **k: None)
    base = ["r.y4m", "d.y4m", "--json", str(tmp_path / "x.json")]
    score.main(base)
    score.main(base + ["--distortion-map", "16"])
    score.main(base + ["--distortion-map", "64", "--distortion-planes", "all", "--distortion-dir", "maps", "--distortion-factor", "8",
                       "--distortion-min-mse", "2.5"])
    score.main(base + ["--distortion-planes", "all"])      # without --distortion-map nothing is passed on
    assert not any(k.startswith("distortion") for k in seen[0]) and not any(k.startswith("distortion") for k in seen[3])
    assert {k: v for k, v in seen[0].items() if k != "progress"} == {k: v for k, v in seen[3].items() if k != "progress"}
    assert {k: v for k, v in seen[1].items() if k.startswith("distortion")} == {
        "distortion_map": 16, "distortion_planes": "y", "distortion_dir": None, "distortion_factor": 16, "distortion_min_mse": 4.0}
    assert {k: v for k, v in seen[2].items() if k.startswith("distortion")} == {
        "distortion_map": 64, "distortion_planes": "all", "distortion_dir": "maps", "distortion_factor": 8.0, "distortion_min_mse": 2.5}
    with pytest.raises(SystemExit):
        score.main(base + ["--distortion-map", "12"])


def test_analyzer_options_results_and_child_argv(tmp_path, monkeypatch):
    from pqa2_amd import vmaf_analyzer as V
    rp, dp = _write(tmp_path)
    a = V.VMAFAnalyzer()
    assert a.distortion_map_enabled is False and a.distortion_tile == 32 and a._ssim_family_kwargs() == {}
    a.set_output_directory(str(tmp_path))
    a._engine_factory = _tile_engine()
    res = a.analyze_videos(rp, dp)
    assert res is not None and "distortion" not in res
    a.set_advanced_options(distortion_map_enabled=True, distortion_tile=T)
    assert a._ssim_family_kwargs() == {"distortion_map": T}
    lines = []
    a.status_update.connect(lines.append)
    res = a.analyze_videos(rp, dp)
    assert res["distortion"]["tile"] == T and len(res["distortion"]["planes"]["y"]["defects"]) == 1
    assert res["distortion"]["planes"]["y"]["defects"][0]["box"] == [16, 0, 64, 48]
    assert any(line.startswith("Distortion map: 16 px tiles on 10 frames, 1 localised defects") for line in lines)

    class Opts:
        def __init__(self, d):
            self.d = d

        def get_setting(self, k):
            return self.d

    a.set_options_from_manager(Opts({"distortion_map_enabled": False, "distortion_tile": 64}))
    assert a.distortion_map_enabled is False and a.distortion_tile == 64

    cmds = []

    class FakePopen:
        def __init__(self, cmd, **kw):
            cmds.append(cmd)
            self.stderr = io.StringIO("")
            self.pid = os.getpid()

        def wait(self, timeout=None):
            return 1

        def poll(self):
            return 1

    monkeypatch.setattr(V.subprocess, "Popen", FakePopen)
    b = V.VMAFAnalyzer()
    b.gpus = 2
    b._run_child_job(rp, dp, "vmaf_v0.6.1", "j.json", None, None, 3)
    b.set_advanced_options(distortion_map_enabled=True, distortion_tile=8)
    b._run_child_job(rp, dp, "vmaf_v0.6.1", "j.json", None, None, 3)
    for c in cmds:
        c[c.index("--master-port") + 1] = "PORT"
    assert "--distortion-map" not in cmds[0]
    at = cmds[1].index("--distortion-map")
    assert cmds[1][at + 1] == "8" and cmds[1][:at] + cmds[1][at + 2:] == cmds[0]
