"""The distortion spectrum on the host (no GPU): the restatement of the band moments (tests/spectrum_ref.py) against plain
loops and Parseval's identity, pqa2_amd/spectrum.py on the exactness of its split, on a horizontal blur and on added noise of
known size, and score_files(spectrum=) -- result, JSON, a shared pass with the distortion map, a sharded gloo run, CLI and
analyzer -- through the oracle stand-in."""
import io
import json
import os
import socket
import sys
from fractions import Fraction

import numpy as np
import pytest

from tests import spectrum_ref as R
from tests import tile_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, L, FRAMES = 96, 64, 4, 10
BW, BH = 270, 482      # the blur and noise cases: no multiple of 2^L either way


def _band_engine(counter=None):
    from tests.fake_engine import OracleEngine

    class BandEngine(OracleEngine):
        """the oracle stand-in plus the restated band and tile moments; counts the contexts that serve them"""

        def band_moments(self, ref_frames, dis_frames, levels=4):
            if counter is not None:
                counter.setdefault("band", set()).add(id(self))
            return R.band_moments(list(ref_frames), list(dis_frames), levels, self.bpc)

        def tile_moments(self, ref_frames, dis_frames, tile=32):
            if counter is not None:
                counter.setdefault("tile", set()).add(id(self))
            return tile_ref.tile_moments(list(ref_frames), list(dis_frames), tile, self.bpc)
    return BandEngine


# ---- the restatement -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bpc,w,h,levels", [(8, 22, 20, 3), (10, 17, 9, 4), (12, 8, 8, 6), (8, 1, 1, 2)])
def test_the_restatement_equals_plain_loops(bpc, w, h, levels):
    ref, dis = R.random_pairs(bpc + w, 1, w, h, bpc)
    if bpc > 8:
        ref[0][0, 0] = 65535      # above top: read as top
    M = R.band_moments(ref, dis, levels, bpc)
    assert M.dtype == np.uint64 and M.shape == (1, levels, 4, 3)
    assert R.signed(M)[0].tolist() == R.band_moments_loops(ref[0], dis[0], levels, bpc)


@pytest.mark.parametrize("bpc,w,h,levels", [(8, 64, 32, 5), (12, 64, 64, 6), (10, 48, 16, 4)])
def test_parseval_as_integers(bpc, w, h, levels):
    """sizes that are multiples of 2^L: sum_l 4^(L-l) (E_H + E_V + E_D)_l + E_A,L == 4^L sum x^2, for the planes and their error"""
    ref, dis = R.random_pairs(3 * bpc, 1, w, h, bpc)
    S = R.signed(R.band_moments(ref, dis, levels, bpc))[0]
    r, d = ref[0].astype(object), dis[0].astype(object)
    E = S[..., 0] + S[..., 1] - 2 * S[..., 2]
    for col, want in ((S[..., 0], (r * r).sum()), (S[..., 1], (d * d).sum()), (S[..., 2], (r * d).sum()), (E, ((r - d) ** 2).sum())):
        lhs = sum(4 ** (levels - l) * int(col[l - 1, :3].sum()) for l in range(1, levels + 1)) + int(col[levels - 1, 3])
        assert lhs == 4 ** levels * int(want)


def test_band_counts_and_pool():
    from pqa2_amd import spectrum as SP
    assert SP.band_counts(270, 482, 4) == [135 * 241, 67 * 120, 33 * 60, 16 * 30]
    assert SP.band_counts(3, 1, 2) == [0, 0]
    for bad in ((0, 4, 1), (4, 4, 0), (4, 4, 7)):
        with pytest.raises(ValueError):
            SP.band_counts(*bad)
    ref, dis = R.random_pairs(4, 3, 16, 16, 12)
    M = R.band_moments(ref, dis, 2, 12)
    P = SP.pool(M)
    assert P.dtype == object and P.tolist() == (R.signed(M)[0] + R.signed(M)[1] + R.signed(M)[2]).tolist()
    big = np.full((5, 1, 4, 3), np.uint64(1 << 62), np.uint64)      # five frames at the kernel's bound: past uint64
    assert SP.pool(big)[0, 3, 0] == 5 << 62 and SP.pool(big)[0, 0, 2] == 5 << 62
    with pytest.raises(ValueError):
        SP.pool(M.astype(np.int64))


# ---- the split -------------------------------------------------------------------------------------------------------------------
def test_the_split_is_exact():
    from pqa2_amd import spectrum as SP
    ref, dis = R.random_pairs(11, 2, 40, 24, 10)
    dis[1] = R.add_noise(ref[1], 5, 30, 10)
    M = R.band_moments(ref, dis, 3, 10)
    for f in range(2):
        for row in SP.band_table(M[f], 40, 24, 10):
            for b in row["bands"].values():
                g, err, loss, noise = R.split(b["rr"], b["dd"], b["rd"])
                assert (b["gain"], b["err"], b["loss"], b["noise"]) == (g, err, loss, noise)
                assert isinstance(b["err"], Fraction) and b["err"] == b["loss"] + b["noise"] and b["noise"] >= 0 and b["loss"] >= 0
                assert b["err_mse"] == b["err"] / (16 ** row["level"] * row["count"] * 16)      # 10 bit: 4^(b - 8) = 16
    # multiples of 2^L: the band MSEs and that of A_L add up to the plane's MSE exactly, every coverage is 1
    table = SP.band_table(M[1], 40, 24, 10)
    total = sum(b["err_mse"] for _, _, b in SP._parts(table))
    diff = ref[1].astype(object) - dis[1].astype(object)
    assert total == Fraction(int((diff * diff).sum()), 40 * 24 * 16) and all(row["coverage"] == 1 for row in table)
    assert [float(r["coverage"]) for r in SP.band_table(R.band_moments(*R.random_pairs(1, 1, 9, 6), 2)[0], 9, 6, 8)] == [48 / 54, 32 / 54]


def test_identical_offset_and_empty_reference():
    from pqa2_amd import spectrum as SP
    ref = [R.noise_plane(2, 32, 32)]
    s = SP.summary(SP.band_table(R.band_moments(ref, ref, 3)[0], 32, 32, 8))
    assert (s["kind"], s["axis"], s["total_mse"], s["loss_share"]) == ("identical", None, 0.0, 0.0)
    up = [(np.minimum(ref[0], 200) + 7).astype(np.uint8)]
    base = [np.minimum(ref[0], 200)]
    table = SP.band_table(R.band_moments(base, up, 3)[0], 32, 32, 8)      # d = r + c: all of the error is in A_L
    assert all(b["err"] == 0 for row in table for k, b in row["bands"].items() if k != "a")
    assert table[-1]["bands"]["a"]["err_mse"] == 49 and SP.summary(table)["total_mse"] == 49.0
    zero = [np.zeros((32, 32), np.uint8)]
    table = SP.band_table(R.band_moments(zero, ref, 2)[0], 32, 32, 8)      # an empty reference: no gain, all noise
    assert all(b["gain"] is None and b["loss"] == 0 and b["noise"] == b["err"] for row in table for b in row["bands"].values())
    s = SP.summary(table)
    assert s["kind"] == "noise" and s["bandwidth_h"] == {"level": None, "cycles_per_pixel": None}
    small = [(ref[0] ^ (np.arange(32) % 2 == 0)[None, :]).astype(np.uint8)]      # every other column off by one: MSE 1/2
    assert SP.summary(SP.band_table(R.band_moments(ref, small, 2)[0], 32, 32, 8))["kind"] == "clean"
    assert SP.summary(SP.band_table(R.band_moments(ref, small, 2)[0], 32, 32, 8), min_mse=0.25)["kind"] != "clean"
    with pytest.raises(ValueError):
        SP.summary(table, min_mse=-1)
    with pytest.raises(ValueError):
        SP.summary(table, gain_floor=-0.5)


def _blur_case(transposed=False):
    ref = R.noise_plane(1, BH, BW) if transposed else R.noise_plane(1, BW, BH)
    dis = R.h_blur(ref.T).T if transposed else R.h_blur(ref)
    return ref, np.ascontiguousarray(dis)


def test_a_horizontal_blur_of_uniform_noise():
    """uniform 8-bit noise, 270 x 482, blurred by ([1 2 1] + 2) >> 2 along the rows: for white noise the level-1 gains are
    H 1/4 and V 3/4 (+- 0.02, the sampling spread at this size) and the level-2 H gain is 0.630"""
    from pqa2_amd import spectrum as SP
    ref, dis = _blur_case()
    table = SP.band_table(R.band_moments([ref], [dis], 4)[0], BW, BH, 8)
    g = {(row["level"], k): float(b["gain"]) for row in table for k, b in row["bands"].items()}
    print("gains", {k: round(v, 4) for k, v in g.items()})
    assert abs(g[1, "h"] - 0.25) <= 0.02 and abs(g[1, "v"] - 0.75) <= 0.02 and abs(g[2, "h"] - 0.630) <= 0.02
    s = SP.summary(table)
    assert (s["kind"], s["axis"]) == ("loss", "horizontal") and s["loss_share"] >= 0.5
    assert s["bandwidth_h"] == {"level": 2, "cycles_per_pixel": 0.25} and s["bandwidth_v"] == {"level": 1, "cycles_per_pixel": 0.5}
    assert s["loss_by_orientation"]["h"] >= 2 * s["loss_by_orientation"]["v"]
    assert abs(s["loss_share"] + s["noise_share"] - 1.0) < 1e-12
    assert SP.summary(table, gain_floor=0.2)["bandwidth_h"]["level"] == 1 and SP.summary(table, gain_floor=0.7)["bandwidth_h"]["level"] == 3
    cols = SP.frame_columns(R.band_moments([ref], [dis], 4), BW, BH, 8)
    assert cols["detail_gain_h"][0] == g[1, "h"] and cols["detail_gain_v"][0] == g[1, "v"] and cols["noise_mse"][0] == s["noise_mse"]

    tref, tdis = _blur_case(transposed=True)
    ts = SP.summary(SP.band_table(R.band_moments([tref], [tdis], 4)[0], BH, BW, 8))
    assert (ts["kind"], ts["axis"]) == ("loss", "vertical") and ts["bandwidth_v"]["level"] == 2 and ts["bandwidth_h"]["level"] == 1


def test_added_noise():
    """the same reference plus uniform +- 8 noise, clipped: every gain within 0.01 of 1, the noise per orthonormal coefficient
    flat over levels 1 ... 4, kind noise.  Flat: uniform noise on -8 ... 8 has variance 24 (a little less after clipping); level
    4 holds 3 * 480 coefficients, whose sample variance has a relative spread of sqrt((kurtosis - 1) / n) < sqrt(2 / 1440) =
    0.037; 0.15 is four of those."""
    from pqa2_amd import spectrum as SP
    ref = R.noise_plane(1, BW, BH)
    dis = R.add_noise(ref, 2, 8)
    table = SP.band_table(R.band_moments([ref], [dis], 4)[0], BW, BH, 8)
    gains = [float(b["gain"]) for _, _, b in SP._parts(table)]
    s = SP.summary(table)
    print("gains", gains, "density", s["noise_density_by_level"])
    assert all(abs(g - 1.0) <= 0.01 for g in gains)
    assert s["kind"] == "noise" and s["axis"] is None and s["noise_share"] > 0.99
    dens = s["noise_density_by_level"]
    assert len(dens) == 4 and all(abs(v / 24.0 - 1.0) <= 0.15 for v in dens) and max(dens) / min(dens) <= 1.15
    assert s["bandwidth_h"]["level"] == 1 and s["bandwidth_v"]["level"] == 1


# ---- score_files through the oracle stand-in ---------------------------------------------------------------------------------
def _write(tmp_path, mono=False, n=FRAMES, kind="blur"):
    from pqa2_amd.yuvio import VideoInfo, write_y4m
    info = VideoInfo(width=W, height=H, fps_num=24, fps_den=1, bit_depth=8, mono=mono, hshift=0 if mono else 1,
                     vshift=0 if mono else 1, chroma_tag="mono" if mono else "420")
    ref = [R.noise_plane(20 + t, W, H) for t in range(n)]
    dis = [R.h_blur(r) if kind == "blur" else R.add_noise(r, 40 + t, 8) for t, r in enumerate(ref)]
    rng = np.random.default_rng(8)
    chroma = [[rng.integers(100, 156, (H // 2, W // 2)).astype(np.uint8) for _ in range(2)] for _ in range(n)]
    rp, dp = str(tmp_path / "ref.y4m"), str(tmp_path / "dis.y4m")
    write_y4m(rp, [[ref[t]] + ([] if mono else chroma[t]) for t in range(n)], info)
    write_y4m(dp, [[dis[t]] + ([] if mono else [chroma[t][0], R.add_noise(chroma[t][1], t, 3)]) for t in range(n)], info)
    return rp, dp, ref, dis


def _log_text(res, tmp_path, name):
    from pqa2_amd import report
    log = report.build_vmaf_log(res["metrics"], 0.0, res["frame_indices"],
                                {"model": res["model_name"], **report.spectrum_log_keys(res.get("spectrum"))})
    report.write_vmaf_json(str(tmp_path / name), log)
    return open(tmp_path / name).read()


COLUMNS = {"detail_gain_h", "detail_gain_v", "noise_mse"}


def test_score_files_off_and_on(tmp_path):
    from pqa2_amd import report
    from pqa2_amd import spectrum as SP
    from pqa2_amd.pipeline import score_files
    rp, dp, ref, dis = _write(tmp_path)
    kw = dict(engine_factory=_band_engine(), psnr=True)
    for bad in (7, -1, 2.5):
        with pytest.raises(ValueError, match="spectrum"):
            score_files(rp, dp, "vmaf_v0.6.1", spectrum=bad, **kw)
    with pytest.raises(ValueError, match="spectrum_planes"):
        score_files(rp, dp, "vmaf_v0.6.1", spectrum=L, spectrum_planes="uv", **kw)
    with pytest.raises(ValueError, match="must not be negative"):
        score_files(rp, dp, "vmaf_v0.6.1", spectrum=L, spectrum_min_mse=-1.0, **kw)
    with pytest.raises(ValueError, match="must not be negative"):
        score_files(rp, dp, "vmaf_v0.6.1", spectrum=L, spectrum_gain_floor=-0.5, **kw)
    plain = score_files(rp, dp, "vmaf_v0.6.1", **kw)
    off = score_files(rp, dp, "vmaf_v0.6.1", spectrum=0, spectrum_planes="all", **kw)
    assert "spectrum" not in plain and "spectrum" not in off and list(off["metrics"]) == list(plain["metrics"])
    text = _log_text(plain, tmp_path, "plain.json")
    assert text == _log_text(off, tmp_path, "off.json") and "spectrum" not in text and "detail_gain" not in text
    assert report.spectrum_log_keys(None) == {}

    on = score_files(rp, dp, "vmaf_v0.6.1", spectrum=L, **kw)
    assert np.array_equal(on["records"].view(np.uint64), plain["records"].view(np.uint64))
    assert all(np.array_equal(on["metrics"][k], plain["metrics"][k]) for k in plain["metrics"])
    assert set(on["metrics"]) - set(plain["metrics"]) == COLUMNS and "distortion" not in on
    sp = on["spectrum"]
    assert set(sp) == {"levels", "planes", "frames"} and (sp["levels"], sp["frames"]) == (L, FRAMES) and set(sp["planes"]) == {"y"}
    M = R.band_moments(ref, dis, L)
    assert sp["planes"]["y"] == SP.analyse(M, W, H, 8)
    y = sp["planes"]["y"]
    assert set(y) == {"bands", "summary"} and len(y["bands"]) == L and set(y["bands"][0]["bands"]) == {"h", "v", "d", "a"}
    assert (y["summary"]["kind"], y["summary"]["axis"]) == ("loss", "horizontal")
    assert y["summary"]["bandwidth_h"]["level"] == 2 and y["summary"]["bandwidth_v"]["level"] == 1
    cols = SP.frame_columns(M, W, H, 8)
    assert all(np.array_equal(on["metrics"][k], cols[k]) for k in COLUMNS)
    # 96 x 64 are multiples of 2^4: the spectrum's total is the clip MSE that the PSNR feature's exact SSE gives
    from pqa2_amd.engine import sse_from_records
    total = sum(int(v) for v in sse_from_records(on["records"])[:, 0])
    assert y["summary"]["total_mse"] == float(Fraction(total, W * H * FRAMES))
    logged = json.loads(_log_text(on, tmp_path, "on.json"))
    assert logged["spectrum"] == json.loads(json.dumps(sp)) and COLUMNS <= set(logged["frames"][0]["metrics"])
    line = report.spectrum_summary_line(sp)
    assert line.startswith("Distortion spectrum: 4 octaves on 10 frames, loss (horizontal)") and "horizontal detail passes up to 1/4" in line
    sub = score_files(rp, dp, "vmaf_v0.6.1", spectrum=L, n_subsample=3, **kw)
    assert sub["spectrum"] == sp and np.array_equal(sub["metrics"]["noise_mse"], on["metrics"]["noise_mse"][::3])
    loose = score_files(rp, dp, "vmaf_v0.6.1", spectrum=L, spectrum_gain_floor=0.2, spectrum_min_mse=1e6, **kw)["spectrum"]["planes"]["y"]
    assert loose["summary"]["kind"] == "clean" and loose["summary"]["bandwidth_h"]["level"] == 1


def test_added_noise_all_planes_and_one_shared_pass(tmp_path):
    from pqa2_amd.pipeline import score_files
    rp, dp, ref, dis = _write(tmp_path, kind="noise")
    seen = {}
    res = score_files(rp, dp, "vmaf_v0.6.1", spectrum=3, spectrum_planes="all", distortion_map=16, engine_factory=_band_engine(seen))
    sp = res["spectrum"]
    assert list(sp["planes"]) == ["y", "cb", "cr"] and sp["planes"]["y"]["summary"]["kind"] == "noise"
    assert sp["planes"]["cb"]["summary"]["kind"] == "identical" and sp["planes"]["cr"]["summary"]["kind"] == "noise"
    assert len(sp["planes"]["cr"]["bands"]) == 3 and sp["planes"]["cr"]["bands"][0]["count"] == 24 * 16 * FRAMES
    # both measurements came from one pass: one small context served every tile and every band call
    assert len(seen["band"]) == 1 and seen["band"] == seen["tile"]
    alone = score_files(rp, dp, "vmaf_v0.6.1", distortion_map=16, engine_factory=_band_engine())
    assert res["distortion"] == alone["distortion"] and set(res["distortion"]["planes"]) == {"y"}
    assert COLUMNS | {"tile_psnr_min", "distortion_concentration"} <= set(res["metrics"])


def test_all_planes_of_a_mono_clip_is_an_error(tmp_path):
    from pqa2_amd.pipeline import score_files
    rp, dp, _, _ = _write(tmp_path, mono=True, n=3)
    with pytest.raises(ValueError, match="monochrome"):
        score_files(rp, dp, "vmaf_v0.6.1", spectrum=L, spectrum_planes="all", engine_factory=_band_engine())
    assert set(score_files(rp, dp, "vmaf_v0.6.1", spectrum=L, engine_factory=_band_engine())["spectrum"]["planes"]) == {"y"}


def _worker(rank, world, port, rp, dp, out_path):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from pqa2_amd.pipeline import score_files
    res = score_files(rp, dp, "vmaf_v0.6.1", rank=rank, world_size=world, engine_factory=_band_engine(), spectrum=L,
                      spectrum_planes="all", distortion_map=16)
    if rank == 0:
        with open(out_path, "w") as f:
            json.dump({"spectrum": res["spectrum"], "distortion": res["distortion"],
                       **{k: res["metrics"][k].tolist() for k in COLUMNS}}, f)
    else:
        assert res is None
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_equals_single_process(tmp_path, world):
    import torch.multiprocessing as mp
    from pqa2_amd.pipeline import score_files
    rp, dp, _, _ = _write(tmp_path)
    single = score_files(rp, dp, "vmaf_v0.6.1", engine_factory=_band_engine(), spectrum=L, spectrum_planes="all", distortion_map=16)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = str(tmp_path / "res.json")
    mp.spawn(_worker, args=(world, port, rp, dp, out), nprocs=world, join=True)
    got = json.load(open(out))
    assert got["spectrum"] == json.loads(json.dumps(single["spectrum"]))
    assert got["distortion"] == json.loads(json.dumps(single["distortion"]))
    assert all(got[k] == single["metrics"][k].tolist() for k in COLUMNS)


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
    score.main(base + ["--spectrum", "4"])
    score.main(base + ["--spectrum", "6", "--spectrum-planes", "all", "--spectrum-min-mse", "2.5", "--spectrum-gain-floor", "0.7"])
    score.main(base + ["--spectrum-planes", "all"])      # without --spectrum nothing is passed on
    assert not any(k.startswith("spectrum") for k in seen[0]) and not any(k.startswith("spectrum") for k in seen[3])
    assert {k: v for k, v in seen[0].items() if k != "progress"} == {k: v for k, v in seen[3].items() if k != "progress"}
    assert {k: v for k, v in seen[1].items() if k.startswith("spectrum")} == {
        "spectrum": 4, "spectrum_planes": "y", "spectrum_min_mse": 1.0, "spectrum_gain_floor": 0.5}
    assert {k: v for k, v in seen[2].items() if k.startswith("spectrum")} == {
        "spectrum": 6, "spectrum_planes": "all", "spectrum_min_mse": 2.5, "spectrum_gain_floor": 0.7}
    with pytest.raises(SystemExit):
        score.main(base + ["--spectrum", "7"])


def test_analyzer_options_results_and_child_argv(tmp_path, monkeypatch):
    from pqa2_amd import vmaf_analyzer as V
    rp, dp, _, _ = _write(tmp_path)
    a = V.VMAFAnalyzer()
    assert a.spectrum_enabled is False and a.spectrum_levels == 4 and a._ssim_family_kwargs() == {}
    a.set_output_directory(str(tmp_path))
    a._engine_factory = _band_engine()
    res = a.analyze_videos(rp, dp)
    assert res is not None and "spectrum" not in res
    a.set_advanced_options(spectrum_enabled=True, spectrum_levels=3)
    assert a._ssim_family_kwargs() == {"spectrum": 3}
    lines = []
    a.status_update.connect(lines.append)
    res = a.analyze_videos(rp, dp)
    assert res["spectrum"]["levels"] == 3 and res["spectrum"]["planes"]["y"]["summary"]["axis"] == "horizontal"
    assert any(line.startswith("Distortion spectrum: 3 octaves on 10 frames, loss (horizontal)") for line in lines)

    class Opts:
        def __init__(self, d):
            self.d = d

        def get_setting(self, k):
            return self.d

    a.set_options_from_manager(Opts({"spectrum_enabled": False, "spectrum_levels": 6}))
    assert a.spectrum_enabled is False and a.spectrum_levels == 6

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
    b.set_advanced_options(spectrum_enabled=True, spectrum_levels=5)
    b._run_child_job(rp, dp, "vmaf_v0.6.1", "j.json", None, None, 3)
    for c in cmds:
        c[c.index("--master-port") + 1] = "PORT"
    assert "--spectrum" not in cmds[0]
    at = cmds[1].index("--spectrum")
    assert cmds[1][at + 1] == "5" and cmds[1][:at] + cmds[1][at + 2:] == cmds[0]
