"""Temporal distortion on the host (no GPU): the restatement of the temporal moments (tests/temporal_ref.py) against plain
loops, pqa2_amd/temporal.py on clips whose fault is known -- a fixed pattern, fresh noise, frame blends, a temporal filter, a
logo, pumping gain, a jumping error pattern, repeated frames -- and score_files(temporal=) -- result, JSON, a shared pass, a
sharded gloo run, CLI and analyzer -- through the oracle stand-in.

The clips: 25 frames of 160 x 96, 8 bit, T = 32.  The reference is a smooth random field (white noise through a Gaussian of
sigma 4 px, stretched over the whole code range) panned 3 px a frame; its top 32 rows are held still."""
import io
import json
import os
import socket
import sys
from fractions import Fraction

import numpy as np
import pytest

from tests import spectrum_ref, temporal_ref as R, tile_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, T, FRAMES, PAN, STILL = 160, 96, 32, 25, 3, 32
COLUMNS = {"temporal_gain", "temporal_noise_mse", "blend_weight"}


def _field(seed: int = 5) -> np.ndarray:
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((H + 32, W + PAN * FRAMES + 32))
    k = np.exp(-0.5 * (np.arange(-16, 17) / 4.0) ** 2)
    k /= k.sum()
    x = np.apply_along_axis(lambda v: np.convolve(v, k, "valid"), 1, x)
    x = np.apply_along_axis(lambda v: np.convolve(v, k, "valid"), 0, x)
    x = (x - x.min()) / (x.max() - x.min())
    return np.rint(255.0 * x).astype(np.int64)


_CACHE = {}


def reference() -> list:
    if "ref" not in _CACHE:
        f = _field()
        out = []
        for t in range(FRAMES):
            p = f[:H, PAN * t:PAN * t + W].copy()
            p[:STILL] = f[:STILL, :W]
            out.append(p.astype(np.uint8))
        _CACHE["ref"] = out
    return _CACHE["ref"]


def _u8(x) -> np.ndarray:
    return np.clip(np.rint(x), 0, 255).astype(np.uint8)


def clip(name: str) -> list:
    """the captured clip of a case of the table"""
    if name in _CACHE:
        return _CACHE[name]
    ref = [r.astype(np.float64) for r in reference()]
    rng = np.random.default_rng(sum(name.encode()))
    if name == "identical":
        dis = [_u8(r) for r in ref]
    elif name == "fixed":       # one noise pattern of sigma 6 on every frame
        pat = 6.0 * rng.standard_normal((H, W))
        dis = [_u8(r + pat) for r in ref]
    elif name == "fresh":       # fresh noise of sigma 3 per frame
        dis = [_u8(r + 3.0 * rng.standard_normal((H, W))) for r in ref]
    elif name in ("blend2", "blend4"):
        wt = 0.5 if name == "blend2" else 0.25
        dis = [_u8(ref[0])] + [_u8(np.floor((1 - wt) * ref[k] + wt * ref[k - 1] + 0.5)) for k in range(1, FRAMES)]
    elif name == "filter":      # (1, 2, 1) / 4 over time, the ends repeated
        dis = [_u8(np.floor((ref[max(k - 1, 0)] + 2 * ref[k] + ref[min(k + 1, FRAMES - 1)]) / 4 + 0.5)) for k in range(FRAMES)]
    elif name == "logo":        # an opaque rectangle over the tiles x >= 96, y >= 64
        dis = []
        for r in ref:
            d = r.copy()
            d[64:, 96:] = 180.0
            dis.append(_u8(d))
    elif name == "pump":        # gain alternating 1.00 / 1.03
        dis = [_u8(r * (1.03 if k % 2 else 1.0)) for k, r in enumerate(ref)]
    elif name == "keyframes":   # an error pattern that changes every 12 frames
        pats = [4.0 * rng.standard_normal((H, W)) for _ in range(3)]
        dis = [_u8(r + pats[k // 12]) for k, r in enumerate(ref)]
    elif name == "repeats":     # frames 5, 10 and 15 show their predecessors
        dis = [_u8(ref[k - 1] if k in (5, 10, 15) else ref[k]) for k in range(FRAMES)]
    else:
        raise KeyError(name)
    _CACHE[name] = dis
    return dis


CASES = ("identical", "fixed", "fresh", "blend2", "blend4", "filter", "logo", "pump", "keyframes", "repeats")


def moments(name: str) -> np.ndarray:
    key = "M:" + name
    if key not in _CACHE:
        _CACHE[key] = R.temporal_moments(reference(), clip(name), T, 8)
    return _CACHE[key]


def summary(name: str, **kw) -> dict:
    from pqa2_amd import temporal as TP
    return TP.summary(moments(name), W, H, T, 8, **kw)


# ---- the restatement -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bpc,w,h,tile,n", [(8, 21, 19, 8, 3), (10, 17, 9, 16, 2), (12, 70, 5, 64, 4), (8, 1, 1, 32, 2)])
def test_the_restatement_equals_plain_loops(bpc, w, h, tile, n):
    ref, dis = tile_ref.random_pairs(bpc + w, n, w, h, bpc)
    if bpc > 8:
        ref[0][0, 0] = dis[1][h - 1, w - 1] = 65535      # above top: read as top
    M = R.temporal_moments(ref, dis, tile, bpc)
    ty, tx = -(-h // tile), -(-w // tile)
    assert M.dtype == np.uint64 and M.shape == (n - 1, ty, tx, 7)
    top = (1 << bpc) - 1
    want = [[[[0] * 7 for _ in range(tx)] for _ in range(ty)] for _ in range(n - 1)]
    for k in range(1, n):
        for y in range(h):
            for x in range(w):
                rk, rp, dk, dp = (min(int(p[y, x]), top) for p in (ref[k], ref[k - 1], dis[k], dis[k - 1]))
                a, b, e = rk - rp, dk - dp, dk - rk
                cell = want[k - 1][y // tile][x // tile]
                for m, v in enumerate((a, b, a * a, b * b, a * b, a * e, e * e)):
                    cell[m] += v
    assert R.signed(M).tolist() == want
    assert R.temporal_moments(ref[:1], dis[:1], tile, bpc).shape == (0, ty, tx, 7)
    assert R.temporal_moments([], [], tile, bpc).shape[0] == 0


# ---- the solver on clips whose fault is known --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_loss_plus_noise_is_the_temporal_error(name):
    from pqa2_amd import temporal as TP
    s = summary(name)
    ref, dis = reference(), clip(name)
    want = 0
    for k in range(1, FRAMES):
        d = (dis[k].astype(np.int64) - dis[k - 1]) - (ref[k].astype(np.int64) - ref[k - 1])
        want += int((d * d).sum())
    assert isinstance(s["err"], Fraction) and s["err"] == want and s["loss"] + s["noise"] == s["err"]
    assert s["loss"] >= 0 and s["noise"] >= 0 and s["transitions"] == FRAMES - 1
    tiles = TP.tile_table(TP.pool(moments(name)), W, H, T, 8, transitions=FRAMES - 1)
    assert sum(tiles["loss"].ravel().tolist()) == s["loss"] and sum(tiles["noise"].ravel().tolist()) == s["noise"]
    for r in TP.frame_table(moments(name), W, H, 8):
        assert r["loss"] + r["noise"] == r["err"] and r["temporal_mse"] == r["err"] / (W * H)


def test_identical():
    s = summary("identical")
    assert (s["kind"], s["temporal_mse"], s["blend_weight"], s["pops"], s["pop_period"]) == ("identical", 0.0, 0.0, [], None)
    assert s["motion_mse"] > 100.0 and s["gain"] == 1.0


def test_a_fixed_pattern_is_a_spatial_error_not_a_temporal_one():
    """sigma 6 on every frame: a spatial MSE near 36, and only what clipping at 0 and 255 leaves of it between frames"""
    s = summary("fixed")
    print("fixed", s["spatial_mse"], s["temporal_mse"])
    assert s["kind"] == "clean" and 30.0 < s["spatial_mse"] < 40.0 and 0.0 < s["temporal_mse"] < 1.0


def test_fresh_noise():
    """sigma 3 per frame: the difference of two frames' noise has variance 18; where nothing moves all of it is seen"""
    s = summary("fresh")
    print("fresh", s["still_noise_mse"], s["noise_mse"], s["still_share"])
    assert s["kind"] == "noise" and abs(s["still_noise_mse"] / s["noise_mse"] - 1.0) <= 0.10
    assert abs(s["still_share"] - STILL / H) < 1e-12 and s["pops"] == []


@pytest.mark.parametrize("name,weight", [("blend2", Fraction(1, 2)), ("blend4", Fraction(1, 4))])
def test_blends(name, weight):
    from pqa2_amd import report
    s = summary(name)
    print(name, float(s["blend"]), s["blend_residual_share"])
    assert s["kind"] == "blend" and abs(s["blend"] - weight) < Fraction(1, 100) and s["blend_residual_share"] < 0.05
    assert summary(name, blend_min=0.75)["kind"] in ("loss", "noise")      # a weight below the setting is no blend
    line = report.temporal_summary_line({"tile": T, "frames": FRAMES, "planes": {"y": {"summary": s}}})
    assert line.startswith(f"Temporal distortion: 32 px tiles on 25 frames, blend (weight {float(s['blend']):.3f}")


def test_a_temporal_filter_is_a_loss():
    s = summary("filter")
    print("filter", s["gain"], s["loss_share"], float(s["blend"]), s["blend_residual_share"])
    assert s["kind"] == "loss" and s["gain"] < 1.0 and s["loss"] >= s["noise"]
    assert s["blend_residual_share"] > 0.5      # e = (a_{k+1} - a_k) / 4 is not a multiple of a_k: no blend, whatever its weight


def test_a_logo_is_a_loss_without_noise():
    from pqa2_amd import temporal as TP
    s = summary("logo")
    assert s["kind"] == "loss" and s["noise"] == 0 and s["loss"] > 0
    tiles = TP.tile_table(TP.pool(moments("logo")), W, H, T, 8, transitions=FRAMES - 1)
    assert tiles["gain"][2, 3] == 0 and tiles["gain"][2, 4] == 0 and tiles["gain"][1, 3] == 1 and tiles["gain"][0, 0] is None
    assert tiles["loss_mse"][2, 3] > 100.0 and tiles["loss_mse"][1, 1] == 0.0
    pgm = TP.heatmap_pgm(tiles)
    assert pgm.startswith(b"P5\n5 3\n255\n") and len(pgm) == len(b"P5\n5 3\n255\n") + 15
    px = pgm[-15:]
    assert px[2 * 5 + 3] > 200 and px[2 * 5 + 4] > 200 and px[0] == 0      # the logo's tiles are bright, an untouched tile black


def test_pumping_gain_is_noise():
    s = summary("pump")
    print("pump", s["gain"], s["noise_share"], s["still_noise_mse"], s["level_step_max"])
    assert s["kind"] == "noise" and s["still_noise_mse"] > 1.0 and s["level_step_max"] > 1.0


def test_an_error_pattern_that_jumps_at_keyframes_pops():
    s = summary("keyframes")
    assert s["pops"] == [12, 24] and s["pop_period"] is None      # one gap: no period
    from pqa2_amd import temporal as TP
    assert TP.find_pops([Fraction(v) for v in (0, 9, 0, 0, 9, 0, 0, 9, 0, 1)], 1, 8) == ([2, 5, 8], 3)
    assert TP.find_pops([Fraction(v) for v in (0, 9, 0, 9, 0, 0, 9, 0, 0, 0, 9, 0)], 1, 8) == ([2, 4, 7, 11], None)      # gaps 2, 3, 4
    assert TP.find_pops([Fraction(3)] * 4, 1, 8) == ([], None) and TP.find_pops([], 1, 8) == ([], None)
    assert TP.find_pops([Fraction(0), Fraction(1)], 1, 8) == ([], None)      # not above min_mse
    with pytest.raises(ValueError):
        TP.find_pops([Fraction(1)], 1, 8, pop_factor=-1)


def test_repeated_frames_show_as_a_weight_of_one():
    from pqa2_amd import temporal as TP
    rows = TP.frame_table(moments("repeats"), W, H, 8)
    beta = [r["blend"] for r in rows]
    for t in range(FRAMES - 1):      # transition index t: frame t + 1 against frame t
        want = 1 if t in (4, 9, 14) else 0
        assert abs(beta[t] - want) <= Fraction(1, 50), (t, float(beta[t]))
    cols = TP.frame_columns(moments("repeats"), W, H, 8)
    assert set(cols) == COLUMNS and all(v.shape == (FRAMES,) for v in cols.values())
    assert cols["blend_weight"][5] == 1.0 and cols["temporal_gain"][5] == 0.0 and cols["blend_weight"][6] == 0.0
    assert (cols["temporal_gain"][0], cols["temporal_noise_mse"][0], cols["blend_weight"][0]) == (1.0, 0.0, 0.0)


def test_thresholds_units_and_errors():
    from pqa2_amd import temporal as TP
    M8 = moments("fresh")
    s8 = summary("fresh")
    # the same clip at 10 bit (every sample times 4): sums of squares times 16, and every figure of the report unchanged
    ref10 = [r.astype(np.uint16) * 4 for r in reference()]
    dis10 = [d.astype(np.uint16) * 4 for d in clip("fresh")]
    M10 = R.temporal_moments(ref10, dis10, T, 10)
    assert np.array_equal(R.signed(M10)[..., 2:], R.signed(M8)[..., 2:] * 16)
    s10 = TP.summary(M10, W, H, T, 10)
    for key in ("kind", "temporal_mse", "noise_mse", "still_noise_mse", "still_share", "pops", "level_step_max", "motion_mse"):
        assert s10[key] == s8[key], key
    assert summary("fresh", min_mse=1e6)["kind"] == "clean"
    assert summary("fresh", still_mse=0)["still_share"] == s8["still_share"]      # the still rows do not move at all
    assert summary("fresh", still_mse=1e6)["still_share"] == 1.0
    for bad in (dict(min_mse=-1), dict(blend_min=-1), dict(still_mse=-0.5), dict(pop_factor=-2)):
        with pytest.raises(ValueError):
            summary("fresh", **bad)
    with pytest.raises(ValueError):
        TP.summary(M8.astype(np.int64), W, H, T, 8)
    with pytest.raises(ValueError):
        TP.summary(M8[0], W, H, T, 8)
    with pytest.raises(ValueError):
        TP.still_noise(M8, W + 64, H, T, 8)
    empty = TP.analyse(M8[:0], W, H, T, 8)      # a clip of one frame: no transition
    assert empty["frames"] == [] and empty["summary"]["kind"] == "identical" and empty["summary"]["transitions"] == 0
    big = np.zeros((5, 1, 1, 7), np.uint64)
    big[..., 2] = big[..., 3] = np.uint64(1 << 62)      # past uint64 when five are added
    big[..., 4] = np.uint64(1 << 62)
    assert TP.pool(big)[0, 0, 2] == 5 << 62 and TP.summary(big, 64, 64, 64, 12)["kind"] == "identical"
    json.dumps(TP.analyse(M8, W, H, T, 8))


# ---- score_files through the oracle stand-in ---------------------------------------------------------------------------------
def _temporal_engine(counter=None):
    from tests.fake_engine import OracleEngine

    class TemporalEngine(OracleEngine):
        """the oracle stand-in plus the restated temporal, band and tile moments; counts the contexts that serve them"""

        def temporal_moments(self, ref_frames, dis_frames, tile=32):
            if counter is not None:
                counter.setdefault("temporal", set()).add(id(self))
                counter["frames"] = counter.get("frames", 0) + len(ref_frames)
            return R.temporal_moments(list(ref_frames), list(dis_frames), tile, self.bpc)

        def band_moments(self, ref_frames, dis_frames, levels=4):
            if counter is not None:
                counter.setdefault("band", set()).add(id(self))
            return spectrum_ref.band_moments(list(ref_frames), list(dis_frames), levels, self.bpc)

        def tile_moments(self, ref_frames, dis_frames, tile=32):
            if counter is not None:
                counter.setdefault("tile", set()).add(id(self))
            return tile_ref.tile_moments(list(ref_frames), list(dis_frames), tile, self.bpc)
    return TemporalEngine


SW, SH, SN = 96, 64, 19      # the clips of the score_files tests: three chunks of 8, 8 and 3


def _write(tmp_path, mono=False, n=SN):
    from pqa2_amd.yuvio import VideoInfo, write_y4m
    info = VideoInfo(width=SW, height=SH, fps_num=24, fps_den=1, bit_depth=8, mono=mono, hshift=0 if mono else 1,
                     vshift=0 if mono else 1, chroma_tag="mono" if mono else "420")
    ref = [np.ascontiguousarray(r[:SH, :SW]) for r in reference()[:n]]
    dis = [np.ascontiguousarray(d[:SH, :SW]) for d in clip("blend2")[:n]]
    rng = np.random.default_rng(8)
    chroma = [[rng.integers(100, 156, (SH // 2, SW // 2)).astype(np.uint8) for _ in range(2)] for _ in range(n)]
    rp, dp = str(tmp_path / "ref.y4m"), str(tmp_path / "dis.y4m")
    write_y4m(rp, [[ref[t]] + ([] if mono else chroma[t]) for t in range(n)], info)
    write_y4m(dp, [[dis[t]] + ([] if mono else [chroma[t][0], chroma[(t + 1) % n][1]]) for t in range(n)], info)
    return rp, dp, ref, dis


def _log_text(res, tmp_path, name):
    from pqa2_amd import report
    log = report.build_vmaf_log(res["metrics"], 0.0, res["frame_indices"],
                                {"model": res["model_name"], **report.temporal_log_keys(res.get("temporal"))})
    report.write_vmaf_json(str(tmp_path / name), log)
    return open(tmp_path / name).read()


def test_score_files_off_and_on(tmp_path):
    from pqa2_amd import report
    from pqa2_amd import temporal as TP
    from pqa2_amd.pipeline import score_files
    rp, dp, ref, dis = _write(tmp_path)
    kw = dict(engine_factory=_temporal_engine(), psnr=True)
    for bad in (7, -8, 2.5, True, None):
        with pytest.raises(ValueError, match="temporal"):
            score_files(rp, dp, "vmaf_v0.6.1", temporal=bad, **kw)
    with pytest.raises(ValueError, match="temporal_planes"):
        score_files(rp, dp, "vmaf_v0.6.1", temporal=T, temporal_planes="uv", **kw)
    for name in ("temporal_min_mse", "temporal_blend_min", "temporal_still_mse", "temporal_pop_factor"):
        with pytest.raises(ValueError, match="must not be negative"):
            score_files(rp, dp, "vmaf_v0.6.1", temporal=T, **{name: -1.0}, **kw)
    plain = score_files(rp, dp, "vmaf_v0.6.1", **kw)
    off = score_files(rp, dp, "vmaf_v0.6.1", temporal=0, temporal_planes="all", **kw)
    assert "temporal" not in plain and "temporal" not in off and list(off["metrics"]) == list(plain["metrics"])
    text = _log_text(plain, tmp_path, "plain.json")
    assert text == _log_text(off, tmp_path, "off.json") and "temporal" not in text and "blend_weight" not in text
    assert report.temporal_log_keys(None) == {}

    seen = {}
    on = score_files(rp, dp, "vmaf_v0.6.1", temporal=T, engine_factory=_temporal_engine(seen), psnr=True)
    assert np.array_equal(on["records"].view(np.uint64), plain["records"].view(np.uint64))
    assert all(np.array_equal(on["metrics"][k], plain["metrics"][k]) for k in plain["metrics"])
    assert set(on["metrics"]) - set(plain["metrics"]) == COLUMNS and "distortion" not in on and "spectrum" not in on
    assert seen["frames"] == SN + 2      # every frame once, and the predecessor of the second and the third chunk
    tp = on["temporal"]
    assert set(tp) == {"tile", "planes", "frames"} and (tp["tile"], tp["frames"]) == (T, SN) and set(tp["planes"]) == {"y"}
    M = R.temporal_moments(ref, dis, T)
    assert tp["planes"]["y"] == TP.analyse(M, SW, SH, T, 8)
    y = tp["planes"]["y"]
    assert set(y) == {"summary", "frames"} and len(y["frames"]) == SN - 1 and y["frames"][0]["frame"] == 1
    assert y["summary"]["kind"] == "blend" and abs(y["summary"]["blend_weight"] - 0.5) < 0.01
    cols = TP.frame_columns(M, SW, SH, 8)
    assert all(np.array_equal(on["metrics"][k], cols[k]) for k in COLUMNS)
    logged = json.loads(_log_text(on, tmp_path, "on.json"))
    assert logged["temporal"] == json.loads(json.dumps(tp)) and COLUMNS <= set(logged["frames"][0]["metrics"])
    assert logged["frames"][0]["metrics"]["temporal_gain"] == 1.0 and logged["frames"][0]["metrics"]["blend_weight"] == 0.0
    assert report.temporal_summary_line(tp).startswith("Temporal distortion: 32 px tiles on 19 frames, blend (weight 0.5")
    sub = score_files(rp, dp, "vmaf_v0.6.1", temporal=T, n_subsample=3, **kw)
    assert sub["temporal"] == tp and np.array_equal(sub["metrics"]["blend_weight"], on["metrics"]["blend_weight"][::3])
    loose = score_files(rp, dp, "vmaf_v0.6.1", temporal=T, temporal_min_mse=1e6, **kw)["temporal"]["planes"]["y"]["summary"]
    assert loose["kind"] == "clean"
    strict = score_files(rp, dp, "vmaf_v0.6.1", temporal=T, temporal_blend_min=0.75, **kw)["temporal"]["planes"]["y"]["summary"]
    assert strict["kind"] in ("loss", "noise") and strict["blend_min"] == 0.75


def test_all_planes_and_one_shared_pass(tmp_path):
    from pqa2_amd.pipeline import score_files
    rp, dp, ref, dis = _write(tmp_path)
    seen = {}
    res = score_files(rp, dp, "vmaf_v0.6.1", temporal=16, temporal_planes="all", spectrum=3, distortion_map=16,
                      engine_factory=_temporal_engine(seen))
    tp = res["temporal"]
    assert list(tp["planes"]) == ["y", "cb", "cr"] and tp["planes"]["y"]["summary"]["kind"] == "blend"
    assert tp["planes"]["cb"]["summary"]["kind"] == "identical" and tp["planes"]["cr"]["summary"]["kind"] in ("loss", "noise")
    # the three measurements came from one pass: one small context served every call
    assert len(seen["temporal"]) == 1 and seen["temporal"] == seen["band"] == seen["tile"]
    alone_t = score_files(rp, dp, "vmaf_v0.6.1", temporal=16, temporal_planes="all", engine_factory=_temporal_engine())
    alone_s = score_files(rp, dp, "vmaf_v0.6.1", spectrum=3, engine_factory=_temporal_engine())
    alone_d = score_files(rp, dp, "vmaf_v0.6.1", distortion_map=16, engine_factory=_temporal_engine())
    assert res["temporal"] == alone_t["temporal"] and res["spectrum"] == alone_s["spectrum"]
    assert res["distortion"] == alone_d["distortion"]
    assert COLUMNS | {"tile_psnr_min", "noise_mse"} <= set(res["metrics"])


def test_all_planes_of_a_mono_clip_is_an_error_and_one_frame_is_not(tmp_path):
    from pqa2_amd.pipeline import score_files
    rp, dp, _, _ = _write(tmp_path, mono=True, n=3)
    with pytest.raises(ValueError, match="monochrome"):
        score_files(rp, dp, "vmaf_v0.6.1", temporal=T, temporal_planes="all", engine_factory=_temporal_engine())
    assert set(score_files(rp, dp, "vmaf_v0.6.1", temporal=T, engine_factory=_temporal_engine())["temporal"]["planes"]) == {"y"}
    rp, dp, _, _ = _write(tmp_path, mono=True, n=1)
    one = score_files(rp, dp, "vmaf_v0.6.1", temporal=T, engine_factory=_temporal_engine())
    assert one["temporal"]["frames"] == 1 and one["temporal"]["planes"]["y"]["frames"] == []
    assert one["metrics"]["temporal_gain"].tolist() == [1.0]


def _worker(rank, world, port, rp, dp, out_path):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from pqa2_amd.pipeline import score_files
    res = score_files(rp, dp, "vmaf_v0.6.1", rank=rank, world_size=world, engine_factory=_temporal_engine(), temporal=T,
                      temporal_planes="all", spectrum=2)
    if rank == 0:
        with open(out_path, "w") as f:
            json.dump({"temporal": res["temporal"], "spectrum": res["spectrum"],
                       **{k: res["metrics"][k].tolist() for k in COLUMNS}}, f)
    else:
        assert res is None
    dist.destroy_process_group()


def test_sharded_equals_single_process(tmp_path):
    """three ranks: chunks of 7, 6 and 6 frames; the second and third read the frame in front of theirs"""
    import torch.multiprocessing as mp
    from pqa2_amd.pipeline import score_files
    rp, dp, _, _ = _write(tmp_path)
    single = score_files(rp, dp, "vmaf_v0.6.1", engine_factory=_temporal_engine(), temporal=T, temporal_planes="all", spectrum=2)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = str(tmp_path / "res.json")
    mp.spawn(_worker, args=(3, port, rp, dp, out), nprocs=3, join=True)
    got = json.load(open(out))
    assert got["temporal"] == json.loads(json.dumps(single["temporal"]))
    assert got["spectrum"] == json.loads(json.dumps(single["spectrum"]))
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
    score.main(base + ["--temporal", "32"])
    score.main(base + ["--temporal", "8", "--temporal-planes", "all", "--temporal-min-mse", "2.5", "--temporal-blend-min", "0.125",
                       "--temporal-still-mse", "0.5", "--temporal-pop-factor", "6"])
    score.main(base + ["--temporal-planes", "all"])      # without --temporal nothing is passed on
    assert not any(k.startswith("temporal") for k in seen[0]) and not any(k.startswith("temporal") for k in seen[3])
    assert {k: v for k, v in seen[0].items() if k != "progress"} == {k: v for k, v in seen[3].items() if k != "progress"}
    assert {k: v for k, v in seen[1].items() if k.startswith("temporal")} == {
        "temporal": 32, "temporal_planes": "y", "temporal_min_mse": 1.0, "temporal_blend_min": 1 / 16, "temporal_still_mse": 0.25,
        "temporal_pop_factor": 4}
    assert {k: v for k, v in seen[2].items() if k.startswith("temporal")} == {
        "temporal": 8, "temporal_planes": "all", "temporal_min_mse": 2.5, "temporal_blend_min": 0.125, "temporal_still_mse": 0.5,
        "temporal_pop_factor": 6.0}
    with pytest.raises(SystemExit):
        score.main(base + ["--temporal", "12"])


def test_analyzer_options_results_and_child_argv(tmp_path, monkeypatch):
    from pqa2_amd import vmaf_analyzer as V
    rp, dp, _, _ = _write(tmp_path)
    a = V.VMAFAnalyzer()
    assert a.temporal_enabled is False and a.temporal_tile == 32 and a._ssim_family_kwargs() == {}
    a.set_output_directory(str(tmp_path))
    a._engine_factory = _temporal_engine()
    res = a.analyze_videos(rp, dp)
    assert res is not None and "temporal" not in res
    a.set_advanced_options(temporal_enabled=True, temporal_tile=16)
    assert a._ssim_family_kwargs() == {"temporal": 16}
    lines = []
    a.status_update.connect(lines.append)
    res = a.analyze_videos(rp, dp)
    assert res["temporal"]["tile"] == 16 and res["temporal"]["planes"]["y"]["summary"]["kind"] == "blend"
    assert any(line.startswith("Temporal distortion: 16 px tiles on 19 frames, blend") for line in lines)

    class Opts:
        def __init__(self, d):
            self.d = d

        def get_setting(self, k):
            return self.d

    a.set_options_from_manager(Opts({"temporal_enabled": False, "temporal_tile": 64}))
    assert a.temporal_enabled is False and a.temporal_tile == 64

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
    b.set_advanced_options(temporal_enabled=True, temporal_tile=8)
    b._run_child_job(rp, dp, "vmaf_v0.6.1", "j.json", None, None, 3)
    for c in cmds:
        c[c.index("--master-port") + 1] = "PORT"
    assert "--temporal" not in cmds[0]
    at = cmds[1].index("--temporal")
    assert cmds[1][at + 1] == "8" and cmds[1][:at] + cmds[1][at + 2:] == cmds[0]
