"""Coding-grid detection without a GPU: the premises of the numpy restatement of the edge profiles (tests/edge_ref.py), the
solver pqa2_amd/grid.py on synthetic clips and on hand-made value lists, the plumbing through score_files, the CLI, the analyzer
and the JSON log, and the compiler's resource figures of csrc/edge_profiles.hip."""
import io
import json
import os
import socket
import sys
from fractions import Fraction

import numpy as np
import pytest

from tests import edge_ref as R, spectrum_ref, temporal_ref, tile_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, NF = 352, 288, 3
COLUMNS = {"blockiness_x", "blockiness_y"}


# ---- the restatement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bpc,w,h", [(8, 7, 5), (10, 5, 9), (12, 1, 4), (8, 6, 1)])
def test_the_restatement_equals_plain_loops(bpc, w, h):
    ref, dis = R.random_frames(2, h, w, bpc, seed=w, over=True), R.random_frames(2, h, w, bpc, seed=h + 9, over=True)
    rows, cols = R.edge_profiles(ref, dis, bpc)
    assert rows.shape == (2, h, 3) and cols.shape == (2, w, 3) and rows.dtype == cols.dtype == np.uint64
    top = (1 << bpc) - 1
    for f in range(2):
        r = [[min(int(v), top) for v in row] for row in ref[f]]
        d = [[min(int(v), top) for v in row] for row in dis[f]]
        for x in range(w):
            want = [0, 0, 0]
            for y in range(h if x else 0):
                a, b = r[y][x] - r[y][x - 1], d[y][x] - d[y][x - 1]
                want = [want[0] + a * a, want[1] + b * b, want[2] + a * b]
            assert cols[f, x].view(np.int64).tolist() == want
        for y in range(h):
            want = [0, 0, 0]
            for x in range(w if y else 0):
                a, b = r[y][x] - r[y - 1][x], d[y][x] - d[y - 1][x]
                want = [want[0] + a * a, want[1] + b * b, want[2] + a * b]
            assert rows[f, y].view(np.int64).tolist() == want


def test_one_pixel_touches_four_lines_and_line_zero_is_zero():
    for y, x in ((3, 4), (0, 0), (7, 9), (0, 5), (4, 0)):
        r, d = np.zeros((8, 10), np.uint8), np.zeros((8, 10), np.uint8)
        r[y, x], d[y, x] = 200, 90
        rows, cols = R.edge_profiles([r], [d])
        for m, q in enumerate((200 * 200, 90 * 90, 200 * 90)):
            assert {i: int(v) for i, v in enumerate(rows[0, :, m]) if v} == {i: q for i in (y, y + 1) if 1 <= i < 8}
            assert {i: int(v) for i, v in enumerate(cols[0, :, m]) if v} == {i: q for i in (x, x + 1) if 1 <= i < 10}
    rows, cols = R.edge_profiles(R.random_frames(2, 8, 10, seed=1), R.random_frames(2, 8, 10, seed=2))
    assert not rows[:, 0].any() and not cols[:, 0].any() and rows[:, 1:].all() and cols[:, 1:].all()
    empty = R.edge_profiles([], [])
    assert empty[0].shape == (0, 0, 3) and empty[1].shape == (0, 0, 3)


# ---- the solver on clips -----------------------------------------------------------------------------------------------------
_CLIP = {}


def clip():
    """synth.make_clip(352, 288, 3): the committed c352x288_8 clips; their distortion includes an 8 x 8 DC quantisation"""
    if not _CLIP:
        from pqa2_amd import synth
        _CLIP["ref"], _CLIP["dis"] = synth.make_clip(W, H, NF)
    return _CLIP["ref"], _CLIP["dis"]


def luma():
    ref, dis = clip()
    return [f[0] for f in ref], [f[0] for f in dis]


def solve(ref, dis, **kw):
    from pqa2_amd import grid as G
    h, w = ref[0].shape
    return G.summary(*R.edge_profiles(ref, dis, 8), w, h, 8, **kw)


def test_the_synthetic_clip_has_an_aligned_8_grid_in_its_luma_only():
    ref, dis = clip()
    s = solve(*luma())
    assert s["kind"] == "grid" and s["block"] == [8, 8] and s["phase"] == [0, 0] and s["aligned"] is True
    assert (s["x"]["period"], s["x"]["phase"], s["y"]["period"], s["y"]["phase"]) == (8, 0, 8, 0)
    assert s["x"]["z2"] >= 25 and s["y"]["z2"] >= 25 and s["x"]["votes"] <= s["x"]["lines"] == 43 and s["y"]["lines"] == 35
    assert 1.2 < s["x"]["contrast"] < 1.35 and 1.2 < s["y"]["contrast"] < 1.35 and s["x"]["excess_mse"] > 0
    assert s["captured_grid"] == {"x": None, "y": None} and s["reference_grid"] == {"x": None, "y": None}
    for p in (1, 2):      # the chroma planes carry noise only
        c = solve([f[p] for f in ref], [f[p] for f in dis])
        assert c["kind"] == "none" and c["x"] is None and c["y"] is None and c["block"] is None and c["aligned"] is None


def test_a_cut_moves_the_phase():
    ref, dis = luma()
    s = solve([f[5:, 3:] for f in ref], [f[5:, 3:] for f in dis])      # 3 columns and 5 rows gone: the next edge is 5 / 3 away
    assert s["kind"] == "grid" and s["block"] == [8, 8] and s["phase"] == [5, 3] and s["aligned"] is False


def _block_means(r, block=16, step=24):
    x = r.astype(np.float64)
    b = x.reshape(H // block, block, W // block, block)
    m = b.mean(axis=(1, 3), keepdims=True)
    return np.clip(np.round((b + np.round(m / step) * step - m).reshape(H, W)), 0, 255).astype(np.uint8)


def _blur(r):
    p = np.pad(r.astype(np.int64), 1, mode="edge")
    v = p[:-2] + 2 * p[1:-1] + p[2:]
    return ((v[:, :-2] + 2 * v[:, 1:-1] + v[:, 2:] + 8) // 16).astype(np.uint8)


def test_other_distortions():
    ref, dis = luma()
    s = solve(ref, [_block_means(r) for r in ref])      # a 16-grid without noise
    assert s["kind"] == "grid" and s["block"] == [16, 16] and s["phase"] == [0, 0] and s["aligned"] is True
    for seed in (1, 2, 3):
        rng = np.random.default_rng(seed)
        noisy = [np.clip(r.astype(int) + rng.integers(-6, 7, r.shape), 0, 255).astype(np.uint8) for r in ref]
        assert solve(ref, noisy)["kind"] == "none", seed
    assert solve(ref, [_blur(r) for r in ref])["kind"] == "none"
    same = solve(ref, ref)
    assert same["kind"] == "identical" and same["x"] is None and same["block"] is None
    small = solve([f[:48, :64] for f in ref], [f[:48, :64] for f in dis])      # too few lines for any period to reach 25
    assert small["kind"] == "none"


def test_frame_rows_and_analyse():
    from pqa2_amd import grid as G
    ref, dis = luma()
    rows, cols = R.edge_profiles(ref, dis, 8)
    A = G.analyse(rows, cols, W, H, 8)
    assert json.loads(json.dumps(A)) == A and set(A) == {"summary", "frames"} and len(A["frames"]) == NF
    assert [f["frame"] for f in A["frames"]] == [0, 1, 2]
    assert all(1.2 < f["blockiness_x"] < 1.35 and 1.2 < f["blockiness_y"] < 1.35 for f in A["frames"])
    colsd = G.frame_columns(A["frames"])
    assert set(colsd) == COLUMNS and colsd["blockiness_x"].shape == (NF,)
    none = G.analyse(*R.edge_profiles(ref, ref, 8), W, H, 8)
    assert all(f["blockiness_x"] == 1.0 and f["blockiness_y"] == 1.0 for f in none["frames"])
    only = G.summary(rows, cols, W, H, 8, periods=range(16, 33))      # 8 is not searched: its multiples are found
    assert only["kind"] == "grid" and only["block"] == [16, 16] and only["periods"] == [16, 32]
    assert G.summary(rows, cols, W, H, 8, z2_min=1000)["kind"] == "none"
    with pytest.raises(ValueError):
        G.summary(rows, cols, W, H, 8, periods=range(3, 9))
    with pytest.raises(ValueError):
        G.summary(rows, cols, W, H, 8, periods=range(4, 66))
    with pytest.raises(ValueError):
        G.summary(rows, cols[:2], W, H, 8)
    with pytest.raises(ValueError):
        G.summary(rows.astype(np.int64), cols, W, H, 8)
    with pytest.raises(ValueError):
        G.find_grid([1] * 100, z2_min=-1)
    with pytest.raises(ValueError):
        G.line_values(rows, "both")


# ---- the decision rules on hand-made values ----------------------------------------------------------------------------------
def _comb(n, period, phase=0, high=5, low=1):
    return [high if i % period == phase and i >= 1 else low for i in range(n)]


def test_harmonics():
    from pqa2_amd import grid as G
    g = G.find_grid(_comb(400, 8))
    assert (g["period"], g["phase"], g["lines"], g["votes"]) == (8, 0, 49, 49) and g["z2"] == 98.0 and g["contrast"] == 5.0
    # twice the period owns half the lines, all of which vote: half the z^2; half the period owns them all and as many that do not
    p16, p4 = G.find_grid(_comb(400, 8), periods=[16]), G.find_grid(_comb(400, 8), periods=[4], z2_min=0)
    assert (p16["period"], p16["phase"], p16["lines"], p16["votes"]) == (16, 8, 25, 25) and p16["z2"] == 50.0      # 8, 24 ... 392
    assert (p4["lines"], p4["votes"]) == (99, 49) and p4["z2"] == (3 * 49 - 99) ** 2 / 198 < g["z2"]
    g = G.find_grid(_comb(400, 12, phase=7))
    assert (g["period"], g["phase"]) == (12, 7)
    assert G.find_grid(_comb(400, 8), periods=range(9, 16)) is None


def test_ties_go_to_the_smaller_period_then_the_smaller_phase():
    from pqa2_amd import grid as G
    # every fourth line from 4 and every fourth line from 6 stand out alike: (4, 0) and (4, 2) tie
    v = [5 if i >= 4 and i % 2 == 0 else 1 for i in range(203)]
    g = G.find_grid(v)
    assert (g["period"], g["phase"]) == (4, 0)
    assert G.find_grid(v, periods=[6, 8])["period"] == 6      # (6, 0), (6, 2), (6, 4) and the 8s: the smaller period
    # lines 4, 8 and 10 of 12 stand out: (4, 0) owns 4 and 8, (6, 4) owns 4 and 10, two votes of two lines each
    v = [1] * 12
    v[4] = v[8] = v[10] = 5
    g4, g6 = G.find_grid(v, periods=[4], z2_min=0), G.find_grid(v, periods=[6], z2_min=0)
    assert (g4["period"], g4["phase"], g4["lines"], g4["votes"]) == (4, 0, 2, 2) and g4["z2"] == 4.0
    assert (g6["period"], g6["phase"], g6["lines"], g6["votes"]) == (6, 4, 2, 2) and g6["z2"] == 4.0
    assert G.find_grid(v, z2_min=0) == g4 == G.find_grid(v, periods=[6, 4], z2_min=0)


def test_thirteen_lines_are_the_minimum():
    from pqa2_amd import grid as G
    # 13 lines, all voting: z^2 = 26; 12 lines: 24 < 25 whatever they do
    thirteen = _comb(8 * 13 + 2, 8)      # lines 8 ... 104 inside 2 ... n - 2
    g = G.find_grid(thirteen, periods=[8])
    assert (g["lines"], g["votes"], g["z2"]) == (13, 13, 26.0)
    assert G.find_grid(_comb(8 * 12 + 2, 8), periods=[8]) is None
    assert G.find_grid(_comb(8 * 12 + 2, 8), periods=[8], z2_min=24)["z2"] == 24.0      # accepted FROM the bound
    assert G.find_grid(thirteen[:-1], periods=[8]) is None      # line 104 is now line n - 1: it has no right neighbour
    # line n - 1 has no right neighbour and line 1 no left one that is a line: neither votes
    v = [1] * 60
    v[1] = v[59] = 9
    assert G.find_grid(v, z2_min=0) is None
    assert G.find_grid([], z2_min=0) is None and G.find_grid([1, 2, 1], z2_min=0) is None


def test_an_outlier_line_cannot_fake_a_grid():
    from pqa2_amd import grid as G
    rng = np.random.default_rng(4)
    v = [int(x) for x in rng.integers(100, 200, 500)]
    base = G.find_grid(v)
    v[248] = 10 ** 12      # one vote more at most, whatever its size
    assert G.find_grid(v) == base is None
    flat = [7] * 500       # nothing is STRICTLY above its neighbours
    assert G.find_grid(flat, z2_min=0) is None


def test_a_zero_denominator_has_no_contrast():
    from pqa2_amd import grid as G
    g = G.find_grid(_comb(200, 8, low=0))
    assert g["period"] == 8 and g["contrast"] is None and g["excess_mse"] == 5.0
    g = G.find_grid(_comb(200, 8, low=0), pairs=10)
    assert g["excess_mse"] == 0.5
    lines = np.zeros((1, 200, 3), np.uint64)
    lines[0, 8::8, 1] = 9      # the capture alone has steps, the reference is flat: all of it is added
    assert G.line_values(lines) == [9 if i >= 8 and i % 8 == 0 else 0 for i in range(200)]
    assert G._frame_contrast(lines, 0, {"period": 8, "phase": 0}) == 1.0 and G._frame_contrast(lines, 0, None) == 1.0


def test_values_are_exact_and_pooling_passes_uint64():
    from pqa2_amd import grid as G
    lines = np.zeros((5, 3, 3), np.uint64)
    lines[:, 1] = (1 << 62, 1 << 62, 1 << 62)
    lines[:, 2, 0], lines[:, 2, 1] = 3, 7
    lines[:, 2, 2] = np.array([-4], np.int64).view(np.uint64)[0]      # int64 in the word
    pooled = G.pool(lines)
    assert pooled[1] == (5 << 62, 5 << 62, 5 << 62) and pooled[2] == (15, 35, -20) and pooled[0] == (0, 0, 0)
    assert G.line_values(lines, "reference") == [0, 5 << 62, 15] and G.line_values(lines, "captured") == [0, 5 << 62, 35]
    assert G.line_values(lines, "added") == [0, 0, Fraction(35 * 15 - 400, 15)]
    assert G.line_values(pooled) == G.line_values(lines) and G.pool(lines[0]) == G.pool(lines[:1])


# ---- score_files through the oracle stand-in ---------------------------------------------------------------------------------
def _grid_engine(counter=None):
    from tests.fake_engine import OracleEngine

    class GridEngine(OracleEngine):
        """the oracle stand-in plus the restated edge profiles and temporal, band and tile moments; counts the contexts that
        serve them and the frames the edge profiles read"""

        def _seen(self, what):
            if counter is not None:
                counter.setdefault(what, set()).add(id(self))

        def edge_profiles(self, ref_frames, dis_frames, shape=None):
            self._seen("edge")
            if counter is not None:
                counter["frames"] = counter.get("frames", 0) + len(ref_frames)
            return R.edge_profiles(list(ref_frames), list(dis_frames), self.bpc)

        def temporal_moments(self, ref_frames, dis_frames, tile=32):
            self._seen("temporal")
            return temporal_ref.temporal_moments(list(ref_frames), list(dis_frames), tile, self.bpc)

        def band_moments(self, ref_frames, dis_frames, levels=4):
            self._seen("band")
            return spectrum_ref.band_moments(list(ref_frames), list(dis_frames), levels, self.bpc)

        def tile_moments(self, ref_frames, dis_frames, tile=32):
            self._seen("tile")
            return tile_ref.tile_moments(list(ref_frames), list(dis_frames), tile, self.bpc)
    return GridEngine


SW, SH, SN = 136, 128, 10      # the clips of the score_files tests: 16 and 15 lines of period 8; two chunks of 8 and 2


def _write(tmp_path, mono=False, n=SN):
    from pqa2_amd import synth
    from pqa2_amd.yuvio import write_y4m
    ref, dis = synth.make_clip(SW, SH, n, chroma=not mono)
    rp, dp = str(tmp_path / "ref.y4m"), str(tmp_path / "dis.y4m")
    info = synth.clip_info(SW, SH, chroma=not mono)
    write_y4m(rp, ref, info)
    write_y4m(dp, dis, info)
    return rp, dp, ref, dis


def _log_text(res, tmp_path, name):
    from pqa2_amd import report
    log = report.build_vmaf_log(res["metrics"], 0.0, res["frame_indices"],
                                {"model": res["model_name"], **report.grid_log_keys(res.get("coding_grid"))})
    report.write_vmaf_json(str(tmp_path / name), log)
    return open(tmp_path / name).read()


def test_score_files_off_and_on(tmp_path):
    from pqa2_amd import grid as G, report
    from pqa2_amd.pipeline import score_files
    rp, dp, ref, dis = _write(tmp_path)
    kw = dict(engine_factory=_grid_engine(), psnr=True)
    with pytest.raises(ValueError, match="grid_planes"):
        score_files(rp, dp, "vmaf_v0.6.1", coding_grid=True, grid_planes="uv", **kw)
    for bad in ((3, 64), (9, 8), (4, 65), (8,), None):
        with pytest.raises(ValueError, match="grid_periods"):
            score_files(rp, dp, "vmaf_v0.6.1", coding_grid=True, grid_periods=bad, **kw)
    with pytest.raises(ValueError, match="grid_z2"):
        score_files(rp, dp, "vmaf_v0.6.1", coding_grid=True, grid_z2=-1.0, **kw)
    plain = score_files(rp, dp, "vmaf_v0.6.1", **kw)
    off = score_files(rp, dp, "vmaf_v0.6.1", coding_grid=False, grid_planes="all", grid_periods=(1, 2), grid_z2=-1, **kw)
    assert "coding_grid" not in plain and "coding_grid" not in off and list(off["metrics"]) == list(plain["metrics"])
    text = _log_text(plain, tmp_path, "plain.json")
    assert text == _log_text(off, tmp_path, "off.json") and "coding_grid" not in text and "blockiness" not in text
    assert report.grid_log_keys(None) == {}

    seen = {}
    on = score_files(rp, dp, "vmaf_v0.6.1", coding_grid=True, engine_factory=_grid_engine(seen), psnr=True)
    assert np.array_equal(on["records"].view(np.uint64), plain["records"].view(np.uint64))
    assert all(np.array_equal(on["metrics"][k], plain["metrics"][k]) for k in plain["metrics"])
    assert set(on["metrics"]) - set(plain["metrics"]) == COLUMNS and "distortion" not in on and "temporal" not in on
    assert seen["frames"] == SN      # every frame pair once
    cg = on["coding_grid"]
    assert set(cg) == {"planes"} and set(cg["planes"]) == {"y"}
    rows, cols = R.edge_profiles([f[0] for f in ref], [f[0] for f in dis], 8)
    want = G.analyse(rows, cols, SW, SH, 8)
    assert cg["planes"]["y"] == want
    s = cg["planes"]["y"]["summary"]
    assert s["kind"] == "grid" and s["block"] == [8, 8] and s["phase"] == [0, 0] and s["aligned"] is True and s["frames"] == SN
    colsd = G.frame_columns(want["frames"])
    assert all(np.array_equal(on["metrics"][k], colsd[k]) for k in COLUMNS) and (on["metrics"]["blockiness_x"] > 1.1).all()
    logged = json.loads(_log_text(on, tmp_path, "on.json"))
    assert logged["coding_grid"] == json.loads(json.dumps(cg)) and COLUMNS <= set(logged["frames"][0]["metrics"])
    assert report.grid_summary_line(cg).startswith("Coding grid: grid, blocks of 8 x 8 at phase (0, 0), z^2 3")
    sub = score_files(rp, dp, "vmaf_v0.6.1", coding_grid=True, n_subsample=3, **kw)
    assert sub["coding_grid"] == cg and np.array_equal(sub["metrics"]["blockiness_y"], on["metrics"]["blockiness_y"][::3])
    strict = score_files(rp, dp, "vmaf_v0.6.1", coding_grid=True, grid_z2=1000.0, **kw)["coding_grid"]["planes"]["y"]["summary"]
    assert strict["kind"] == "none" and strict["z2_min"] == 1000.0
    assert (score_files(rp, dp, "vmaf_v0.6.1", coding_grid=True, grid_z2=1000.0, **kw)["metrics"]["blockiness_x"] == 1.0).all()
    wide = score_files(rp, dp, "vmaf_v0.6.1", coding_grid=True, grid_periods=(16, 16), grid_z2=9.0, **kw)
    assert wide["coding_grid"]["planes"]["y"]["summary"]["block"] == [16, 16]
    assert wide["coding_grid"]["planes"]["y"]["summary"]["periods"] == [16, 16]


def test_all_planes_and_one_shared_pass(tmp_path):
    from pqa2_amd.pipeline import score_files
    rp, dp, ref, dis = _write(tmp_path)
    seen = {}
    res = score_files(rp, dp, "vmaf_v0.6.1", coding_grid=True, grid_planes="all", temporal=16, spectrum=3, distortion_map=16,
                      engine_factory=_grid_engine(seen))
    cg = res["coding_grid"]
    assert list(cg["planes"]) == ["y", "cb", "cr"] and cg["planes"]["y"]["summary"]["kind"] == "grid"
    assert cg["planes"]["cb"]["summary"]["kind"] == "none" and cg["planes"]["cr"]["summary"]["kind"] == "none"
    assert seen["frames"] == 3 * SN
    # the four measurements came from one pass: one small context served every call
    assert len(seen["edge"]) == 1 and seen["edge"] == seen["temporal"] == seen["band"] == seen["tile"]
    alone = score_files(rp, dp, "vmaf_v0.6.1", coding_grid=True, grid_planes="all", engine_factory=_grid_engine())
    others = score_files(rp, dp, "vmaf_v0.6.1", temporal=16, spectrum=3, distortion_map=16, engine_factory=_grid_engine())
    assert res["coding_grid"] == alone["coding_grid"]
    assert all(res[k] == others[k] for k in ("temporal", "spectrum", "distortion"))
    assert COLUMNS | {"tile_psnr_min", "noise_mse", "blend_weight"} <= set(res["metrics"])


def test_all_planes_of_a_mono_clip_is_an_error(tmp_path):
    from pqa2_amd.pipeline import score_files
    rp, dp, _, _ = _write(tmp_path, mono=True, n=2)
    with pytest.raises(ValueError, match="monochrome"):
        score_files(rp, dp, "vmaf_v0.6.1", coding_grid=True, grid_planes="all", engine_factory=_grid_engine())
    one = score_files(rp, dp, "vmaf_v0.6.1", coding_grid=True, engine_factory=_grid_engine())
    assert set(one["coding_grid"]["planes"]) == {"y"} and len(one["coding_grid"]["planes"]["y"]["frames"]) == 2


def _worker(rank, world, port, rp, dp, out_path):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from pqa2_amd.pipeline import score_files
    res = score_files(rp, dp, "vmaf_v0.6.1", rank=rank, world_size=world, engine_factory=_grid_engine(), coding_grid=True,
                      grid_planes="all", spectrum=2)
    if rank == 0:
        with open(out_path, "w") as f:
            json.dump({"coding_grid": res["coding_grid"], "spectrum": res["spectrum"],
                       **{k: res["metrics"][k].tolist() for k in COLUMNS}}, f)
    else:
        assert res is None
    dist.destroy_process_group()


def test_sharded_equals_single_process(tmp_path):
    """two ranks of 5 frames each"""
    import torch.multiprocessing as mp
    from pqa2_amd.pipeline import score_files
    rp, dp, _, _ = _write(tmp_path)
    single = score_files(rp, dp, "vmaf_v0.6.1", engine_factory=_grid_engine(), coding_grid=True, grid_planes="all", spectrum=2)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = str(tmp_path / "res.json")
    mp.spawn(_worker, args=(2, port, rp, dp, out), nprocs=2, join=True)
    got = json.load(open(out))
    assert got["coding_grid"] == json.loads(json.dumps(single["coding_grid"]))
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
    score.main(base + ["--coding-grid"])
    score.main(base + ["--coding-grid", "--grid-planes", "all", "--grid-min-period", "8", "--grid-max-period", "32", "--grid-z2", "16"])
    score.main(base + ["--grid-planes", "all", "--grid-z2", "9"])      # without --coding-grid nothing is passed on

    def ours(kw):
        return {k: v for k, v in kw.items() if k.startswith("grid") or k == "coding_grid"}
    assert not ours(seen[0]) and not ours(seen[3])
    assert {k: v for k, v in seen[0].items() if k != "progress"} == {k: v for k, v in seen[3].items() if k != "progress"}
    assert ours(seen[1]) == {"coding_grid": True, "grid_planes": "y", "grid_periods": (4, 64), "grid_z2": 25.0}
    assert ours(seen[2]) == {"coding_grid": True, "grid_planes": "all", "grid_periods": (8, 32), "grid_z2": 16.0}
    with pytest.raises(SystemExit):
        score.main(base + ["--coding-grid", "--grid-planes", "uv"])


def test_analyzer_options_results_and_child_argv(tmp_path, monkeypatch):
    from pqa2_amd import vmaf_analyzer as V
    rp, dp, _, _ = _write(tmp_path)
    a = V.VMAFAnalyzer()
    assert a.coding_grid_enabled is False and a._ssim_family_kwargs() == {}
    a.set_output_directory(str(tmp_path))
    a._engine_factory = _grid_engine()
    res = a.analyze_videos(rp, dp)
    assert res is not None and "coding_grid" not in res
    a.set_advanced_options(coding_grid_enabled=True)
    assert a._ssim_family_kwargs() == {"coding_grid": True}
    lines = []
    a.status_update.connect(lines.append)
    res = a.analyze_videos(rp, dp)
    assert res["coding_grid"]["planes"]["y"]["summary"]["block"] == [8, 8]
    assert any(line.startswith("Coding grid: grid, blocks of 8 x 8 at phase (0, 0)") for line in lines)

    class Opts:
        def __init__(self, d):
            self.d = d

        def get_setting(self, k):
            return self.d

    a.set_options_from_manager(Opts({"coding_grid_enabled": False}))
    assert a.coding_grid_enabled is False
    a.set_options_from_manager(Opts({"coding_grid_enabled": 1}))
    assert a.coding_grid_enabled is True

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
    b.set_advanced_options(coding_grid_enabled=True)
    b._run_child_job(rp, dp, "vmaf_v0.6.1", "j.json", None, None, 3)
    for c in cmds:
        c[c.index("--master-port") + 1] = "PORT"
    assert "--coding-grid" not in cmds[0]
    at = cmds[1].index("--coding-grid")
    assert cmds[1][:at] + cmds[1][at + 1:] == cmds[0]


def test_the_summary_line_names_a_shift_and_a_reference_grid():
    from pqa2_amd import report
    g = {"period": 8, "phase": 3, "lines": 20, "votes": 20, "z2": 40.0, "contrast": 1.5, "excess_mse": 2.0}
    cg = {"planes": {"y": {"summary": {"kind": "grid", "block": [8, None], "phase": [3, None], "aligned": False, "x": g, "y": None,
                                       "reference_grid": {"x": g, "y": None}, "captured_grid": {"x": None, "y": None}}}}}
    line = report.grid_summary_line(cg)
    assert "blocks of 8 x ? at phase (3, ?)" in line and "cropped or shifted after the encode" in line
    assert line.endswith("the reference has a grid of its own")
    assert report.grid_summary_line({"planes": {"y": {"summary": {"kind": "none"}}}}) == "Coding grid: none"
    bad = {"planes": {"y": {"summary": {"kind": "grid", "x": dict(g, contrast=float("nan"))}}}}
    assert report.grid_log_keys(bad)["coding_grid"]["planes"]["y"]["summary"]["x"]["contrast"] is None


# ---- the compiler's figures --------------------------------------------------------------------------------------------------
def test_the_kernel_needs_no_scratch(tmp_path):
    """every instance of edge_profiles_kernel (u8 / u16 samples by 16-byte, 4-byte and one-sample loads) keeps its 48 column
    accumulators, the previous row and the rows in flight in registers: the compiler's own resource figures, as test_abi.py reads
    them for the march kernels"""
    import re
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "pqa2_amd", "csrc", "edge_profiles.hip")
    out = tmp_path / "edge.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", src, "-o", str(out)],
                   check=True, capture_output=True)
    text = out.read_text()
    scratch = [int(x) for x in re.findall(r"^; ScratchSize: (\d+)", text, re.M)]
    assert len(scratch) == 6 and all(s == 0 for s in scratch), scratch
    assert "Folded Reload" not in text and "Folded Spill" not in text
