"""xpsnr without a GPU: the C ABI and its binding (PQA_FEAT_XPSNR / _HFR, the third extension record), the restatement
(tests/xpsnr_ref.py) against closed forms that do not go through it, the smoothing rule, the summary, the stats lines, and
the host layer (pipeline, sharding history, JSON, analyzer, child-job argv, CLI, compare tool) through an oracle-backed
engine."""
import io
import json
import math
import os
import re

import numpy as np
import pytest

from tests import xpsnr_ref as R
from tests.fake_engine import OracleEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pqa_vmaf.h")
CLIPS = os.path.join(ROOT, "tests", "golden", "clips")


def _enum(name):
    return int(eval(re.search(name + r"\s*=\s*([^,/\n}]+)", open(HEADER).read()).group(1).replace("u", "")))


# ---- ABI --------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree():
    from pqa2_amd import _native as N
    src = open(HEADER).read()
    assert _enum("PQA_FEAT_XPSNR") == 4096 == N.FEAT_XPSNR
    assert _enum("PQA_FEAT_XPSNR_HFR") == 8192 == N.FEAT_XPSNR_HFR
    known = re.search(r"PQA_FEAT_KNOWN\s*=([^;]+?)/\*", src, re.S).group(1)
    assert "PQA_FEAT_XPSNR" in known and "PQA_FEAT_XPSNR_HFR" in known
    assert N.FEAT_KNOWN & 4096 and N.FEAT_KNOWN & 8192
    assert not N.FEAT_KNOWN & (1 << 7) and N.FEAT_ALL == 31
    slots = ("PQA_EXT3_XPSNR_Y", "PQA_EXT3_XPSNR_U", "PQA_EXT3_XPSNR_V", "PQA_EXT3_WSSE", "PQA_EXT3_RESERVED",
             "PQA_EXT3_DOUBLES")
    assert tuple(_enum(s) for s in slots) == (0, 1, 2, 3, 6, 8)
    assert (N.EXT3_XPSNR_Y, N.EXT3_XPSNR_U, N.EXT3_XPSNR_V, N.EXT3_WSSE, N.EXT3_RESERVED, N.EXT3_DOUBLES) == (0, 1, 2, 3, 6, 8)
    # what earlier records and tables pin does not move
    assert (_enum("PQA_EXT_DOUBLES"), _enum("PQA_EXT2_DOUBLES"), _enum("PQA_PROF_KERNELS")) == (24, 8, 17)
    assert (N.EXT_DOUBLES, N.EXT2_DOUBLES, N.PROF_KERNELS) == (24, 8, 17)
    for fn in ("pqa_ext3_doubles", "pqa_collect_ext3", "pqa_set_ref_history", "pqa_debug_xpsnr_blocks"):
        assert re.search(r"PQA_API\s+int\s+" + fn + r"\s*\(", src), fn
        assert fn in N.EXPORTS, fn


def test_library_exports_and_create_checks_without_a_device():
    import ctypes as C
    from pqa2_amd import _native as N
    lib = N.load()
    assert lib.pqa_ext3_doubles() == 8
    for fn in ("pqa_collect_ext3", "pqa_set_ref_history", "pqa_debug_xpsnr_blocks"):
        assert hasattr(lib, fn)

    def create(w, h, feats):
        cfg = N.PqaConfig()
        lib.pqa_config_init(C.byref(cfg), w, h)
        cfg.features = feats
        ctx = C.c_void_p()
        rc = lib.pqa_create(C.byref(cfg), C.byref(ctx))
        return rc, lib.pqa_last_error(None).decode()

    rc, msg = create(64, 64, N.FEAT_VMAF | N.FEAT_XPSNR_HFR)
    assert rc == N.PQA_EINVAL and "xpsnr" in msg.lower()
    rc, msg = create(2049, 1152, N.FEAT_VMAF | N.FEAT_XPSNR)     # 2 x 2 activity needs even sizes
    assert rc == N.PQA_EINVAL and "xpsnr" in msg
    rc, msg = create(2050, 1151, N.FEAT_XPSNR)
    assert rc == N.PQA_EINVAL and "xpsnr" in msg
    # odd sizes at or below 2048 x 1152 are not refused for xpsnr's sake (without a device: the device error)
    rc, msg = create(2047, 1151, N.FEAT_XPSNR)
    assert "xpsnr" not in msg
    buf = np.zeros(8, np.uint64)
    assert lib.pqa_debug_xpsnr_blocks(None, None, None, None, 16, 16, 16, 8, 0, buf.ctypes.data, None) == N.PQA_EINVAL


# ---- geometry -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,b", [(3840, 2160, 128), (2560, 1440, 84), (1920, 1080, 64), (1280, 720, 44),
                                   (352, 288, 16), (640, 480, 24), (45, 45, 4), (44, 44, 0)])
def test_block_size(w, h, b):
    assert R.block_size(w, h) == b


def test_bv_threshold():
    assert R.bv_of(2048, 1152) == 1 and R.bv_of(2050, 1152) == 2 and R.bv_of(3840, 2160) == 2


# ---- closed forms -------------------------------------------------------------------------------------------------------
def _flat_clip(w, h, n, bpc, y0, c, shift=(1, 1), chroma=True):
    dt = np.uint8 if bpc == 8 else np.uint16
    wc, hc = (w + (1 << shift[0]) - 1) >> shift[0], (h + (1 << shift[1]) - 1) >> shift[1]
    ref = [np.full((h, w), y0, dt)] + ([np.full((hc, wc), y0, dt)] * 2 if chroma else [])
    dis = [np.full((h, w), y0 + c, dt)] + ([np.full((hc, wc), y0 + c, dt)] * 2 if chroma else [])
    return [ref] * n, [dis] * n


@pytest.mark.parametrize("bpc,w,h,y0,c", [(8, 64, 64, 100, 3), (10, 128, 96, 300, 5), (12, 352, 288, 1000, 7),
                                           (8, 1920, 1088, 20, 2), (8, 3840, 2176, 90, 4)])
@pytest.mark.parametrize("hfr", [False, True])
def test_flat_reference_closed_form(bpc, w, h, y0, c, hfr):
    b = R.block_size(w, h)
    assert w % b == 0 and h % b == 0, "sizes without partial edge blocks"
    refs, diss = _flat_clip(w, h, 3, bpc, y0, c)
    wsse, _ = R.clip(refs, diss, bpc, hfr)
    A = R.amplitude(w, h, bpc)
    lo = 2.0 ** (bpc - 6)
    wc, hc = w // 2, h // 2
    for i in range(3):
        first = i == 0 or (hfr and i == 1)
        m = max(2.0 * y0, lo) if first else lo
        for p, (pw, ph) in enumerate(((w, h), (wc, hc), (wc, hc))):
            want = round(c * c * pw * ph * A / m)
            assert abs(wsse[i, p] - want) <= 1, (i, p, wsse[i, p], want)
    if hfr:
        assert np.array_equal(wsse[1], wsse[0])


def test_small_frames_are_plain_psnr():
    from pqa2_amd import report
    rng = np.random.default_rng(5)
    for (w, h) in ((16, 16), (44, 44), (30, 40)):
        ref = [rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8),
               rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8)]
        dis = [np.clip(p.astype(int) + rng.integers(-5, 6, p.shape), 0, 255).astype(np.uint8) for p in ref]
        wsse, db, _, _ = R.frame(ref, dis, None, None, 8)
        sse = np.array([[int(((r.astype(int) - d) ** 2).sum()) for r, d in zip(ref, dis)]], np.float64)
        pp, _ = report.psnr_values(sse.astype(np.uint64), [(w, h), (w // 2, h // 2), (w // 2, h // 2)], 8)
        assert wsse == [int(x) for x in sse[0]]
        assert np.abs(np.array(db) - pp[0]).max() < 1e-12


def test_smoothing_rule_on_hand_made_grids():
    # 3 x 3 blocks of b = 4 over 12 x 12: raster weights
    w = [9.0, 1.0, 9.0,
         9.0, 9.0, 9.0,
         9.0, 9.0, 5.0]
    out = R.smooth(w, 12, 12, 4)
    # k=1 (x=4): p = w[1] = 1 -> w[0] = min(9, 1) = 1; k=2 (x=8 > b): p = max(w[0], w[2]) = 9 -> w[1] stays 1
    # k=3 (x=0): p = w[1] = 1 -> w[2] = 1; k=4: p = w[4] = 9, k > w_blk: max(9, w[0]) = 9 -> w[3] stays
    # k=5: p = max(w[3], w[5]) = 9, max(9, w[1]) -> w[4] stays; k=6 (x=0): p = w[4] = 9, max(9, w[2] = 1) = 9 -> w[5] stays
    # k=7: p = w[7] = 9, max(9, w[3]) -> w[6] stays; k=8: p = max(w[6], w[8]) = 9, max(9, w[4]) -> w[7] stays;
    # last block: p = max(w[7], w[5]) = 9 -> w[8] = 5 stays
    assert out == [1.0, 1.0, 1.0, 9.0, 9.0, 9.0, 9.0, 9.0, 5.0]
    w2 = [4.0, 4.0, 4.0, 4.0, 4.0, 4.0, 4.0, 2.0, 8.0]
    out2 = R.smooth(w2, 12, 12, 4)
    # k=8: p = max(w[6], w[8]) = 8, k > 3: max(8, w[4]) = 8 -> w[7] = 2 stays; last: p = max(w[7], w[5]) = 4 -> w[8] = 4
    assert out2[8] == 4.0 and out2[:8] == w2[:8]
    assert R.smooth([3.0, 2.0], 8, 4, 4) == [2.0, 2.0]


def test_summary_square_mean_root_and_fallback():
    from pqa2_amd import report
    wsse = np.array([[100.0], [400.0], [0.0]])
    db = np.array([[R.frame_db(100, 64, 64, 8)], [R.frame_db(400, 64, 64, 8)], [math.inf]])
    want = 10 * math.log10(64 * 64 * 255 ** 2 / ((10 + 20 + 0) / 3) ** 2)
    assert R.summary(wsse, db, [(64, 64)], 8)[0] == pytest.approx(want, abs=1e-12)
    got = report.xpsnr_summary(wsse, db, [(64, 64)], 8)
    assert got["y"] == R.summary(wsse, db, [(64, 64)], 8)[0] and got["min"] == got["y"]
    tiny = np.array([[0.0], [1.0], [0.0], [0.0]])       # sum sqrt = 1 < 4 frames: the mean of the dB values
    dbt = np.array([[90.0], [R.frame_db(1, 8, 8, 8)], [91.0], [92.0]])
    assert report.xpsnr_summary(tiny, dbt, [(8, 8)], 8)["y"] == pytest.approx(dbt.mean(), abs=1e-12)


def test_stats_line_format():
    from pqa2_amd import report
    lines = report.xpsnr_stats_lines(np.array([[41.23456, 43.0, math.inf], [7.0, 8.5, 9.25]]))
    assert lines[0] == "n:    1  XPSNR y: 41.2346  XPSNR u: 43.0000  XPSNR v: inf"
    assert lines[1] == "n:    2  XPSNR y: 7.0000  XPSNR u: 8.5000  XPSNR v: 9.2500"
    assert report.xpsnr_stats_lines(np.array([[50.0]])) == ["n:    1  XPSNR y: 50.0000"]


def test_hfr_switch_is_the_integer_frame_rate():
    from pqa2_amd.pipeline import xpsnr_hfr
    from pqa2_amd.yuvio import VideoInfo
    mk = lambda n, d: VideoInfo(64, 64, 8, 1, 1, False, n, d)   # noqa: E731
    assert not xpsnr_hfr(mk(30, 1)) and not xpsnr_hfr(mk(30000, 1001)) and not xpsnr_hfr(mk(63, 2))
    assert xpsnr_hfr(mk(32, 1)) and xpsnr_hfr(mk(60000, 1001)) and xpsnr_hfr(mk(64, 2))


# ---- host layer through an oracle-backed engine ----------------------------------------------------------------------
class XpsnrEngine(OracleEngine):
    """OracleEngine plus the third extension record (the restatement stands in for the kernels) and the reference
    history of pqa_set_ref_history."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.frames, self.history, self.history_calls = {}, (None, None), []

    def set_ref_history(self, planes):
        self.history_calls.append(len(planes))
        self.history = (planes[0] if planes else None, planes[1] if len(planes) > 1 else None)
        self.set_motion_halo(planes[0] if planes else None)

    def submit(self, index, ref_planes, dis_planes):
        super().submit(index, ref_planes, dis_planes)
        self.frames[index] = ([np.array(p) for p in ref_planes], [np.array(p) for p in dis_planes])

    def collect_ext3(self, first, count):
        from pqa2_amd import _native as N
        idx = sorted(self.frames)
        refs = [self.frames[i][0] for i in idx]
        diss = [self.frames[i][1] for i in idx]
        hfr = bool(self.features & N.FEAT_XPSNR_HFR)
        wsse, db = R.clip(refs, diss, self.bpc, hfr, self.history)
        ext3 = np.full((count, N.EXT3_DOUBLES), np.nan)
        for j in range(count):
            k = idx.index(first + j)
            ext3[j, :wsse.shape[1]] = db[k]
            ext3[j, 3:3 + wsse.shape[1]] = wsse[k]
        return (self.collect(first, count), np.full((count, N.EXT_DOUBLES), np.nan),
                np.full((count, N.EXT2_DOUBLES), np.nan), ext3)


KEYS = ("xpsnr_y", "xpsnr_u", "xpsnr_v")


def _clip_paths():
    return tuple(os.path.join(CLIPS, f"c352x288_8_{s}.y4m") for s in ("ref", "dist"))


def _score(tmp_path, tag, factory, paths=None, **kw):
    from pqa2_amd import report
    from pqa2_amd.pipeline import score_files
    rp, dp = paths or _clip_paths()
    res = score_files(rp, dp, "vmaf_v0.6.1", engine_factory=factory, **kw)
    log = report.build_vmaf_log(res["metrics"], 0.0, res["frame_indices"], {"model": res["model_name"]})
    path = str(tmp_path / f"{tag}.json")
    report.write_vmaf_json(path, log)
    return res, open(path).read()


def test_json_gains_xpsnr_keys_only_when_enabled(tmp_path):
    from pqa2_amd import yuvio
    _, old = _score(tmp_path, "old", OracleEngine)
    _, new_default = _score(tmp_path, "new", XpsnrEngine)
    assert new_default == old and "xpsnr" not in old
    res, text = _score(tmp_path, "on", XpsnrEngine, xpsnr=True)
    log = json.loads(text)
    rr, dr = (yuvio.open_video(p) for p in _clip_paths())
    n = len(log["frames"])
    wsse, db = R.clip([rr.frame(i) for i in range(n)], [dr.frame(i) for i in range(n)], 8)
    for i, fr in enumerate(log["frames"]):
        for p, k in enumerate(KEYS):
            assert fr["metrics"][k] == float(f"{db[i, p]:.6f}"), (i, k)
    assert res["xpsnr_lines"] == [f"n: {i + 1:4d}" + "".join(f"  XPSNR {c}: {db[i, p]:3.4f}" for p, c in enumerate("yuv"))
                                  for i in range(n)]
    summ = R.summary(wsse, db, [(352, 288), (176, 144), (176, 144)], 8)
    assert [res["xpsnr_summary"][c] for c in "yuv"] == summ and res["xpsnr_summary"]["min"] == min(summ)
    old_log = json.loads(old)
    for a, b in zip(old_log["frames"], log["frames"]):
        assert all(b["metrics"][k] == v for k, v in a["metrics"].items())


def test_monochrome_clip_gives_luma_only(tmp_path):
    from pqa2_amd import synth, yuvio
    refs, diss = synth.make_clip(64, 48, 3, 8, chroma=False)
    info = synth.clip_info(64, 48, 8, chroma=False)
    rp, dp = str(tmp_path / "r.y4m"), str(tmp_path / "d.y4m")
    yuvio.write_y4m(rp, refs, info)
    yuvio.write_y4m(dp, diss, info)
    res, _ = _score(tmp_path, "mono", XpsnrEngine, (rp, dp), xpsnr=True)
    assert "xpsnr_y" in res["metrics"] and "xpsnr_u" not in res["metrics"]
    assert res["xpsnr_lines"][0].count("XPSNR") == 1


def test_every_frame_scored_whatever_n_subsample(tmp_path):
    res, _ = _score(tmp_path, "sub", XpsnrEngine, xpsnr=True, n_subsample=2)
    assert list(res["frame_indices"]) == [0, 2] and len(res["xpsnr_lines"]) == 3


def test_shards_get_two_history_frames(tmp_path, monkeypatch):
    full, _ = _score(tmp_path, "full", XpsnrEngine, xpsnr=True, psnr=False, ssim=False)
    engines = []

    def factory(*a, **kw):
        engines.append(XpsnrEngine(*a, **kw))
        return engines[-1]

    from pqa2_amd import shard
    from pqa2_amd.pipeline import score_files
    rp, dp = _clip_paths()
    a, b = shard.shard_bounds(3, 3, 2)
    monkeypatch.setattr(shard, "gather_records", lambda local, n, *x, width=24, **k: np.zeros((n, width)))
    assert score_files(rp, dp, "vmaf_v0.6.1", engine_factory=factory, xpsnr=True, psnr=False, ssim=False,
                       rank=2, world_size=3) is None
    assert engines[-1].history_calls == [2] and a == 2
    eng = engines[-1]
    want_db = full["metrics"]["xpsnr_y"][2]
    got_db = eng.collect_ext3(2, 1)[3][0, 0]
    assert got_db == want_db


def test_analyzer_options_results_and_child_argv(tmp_path, monkeypatch):
    from pqa2_amd import vmaf_analyzer as V
    rp, dp = _clip_paths()
    a = V.VMAFAnalyzer()
    assert a.xpsnr_enabled is False
    a.set_output_directory(str(tmp_path))
    a._engine_factory = XpsnrEngine
    res = a.analyze_videos(rp, dp)
    assert res is not None and "xpsnr" not in res
    assert not [f for _, _, fs in os.walk(tmp_path) for f in fs if f.endswith("_xpsnr.txt")]
    a.set_advanced_options(xpsnr_enabled=True)
    assert a._ssim_family_kwargs() == {"xpsnr": True}
    res = a.analyze_videos(rp, dp)
    files = [os.path.join(d, f) for d, _, fs in os.walk(tmp_path) for f in fs if f.endswith("_xpsnr.txt")]
    assert len(files) == 1 and res["xpsnr_log"] == files[0]
    lines = open(files[0]).read().splitlines()
    assert len(lines) == 3 and lines[0].startswith("n:    1  XPSNR y: ")
    for k in KEYS:
        assert isinstance(res[k], float)
    assert res["xpsnr"] == min(res[k] for k in KEYS)

    class Opts:
        def __init__(self, d):
            self.d = d

        def get_setting(self, k):
            return self.d

    a.set_options_from_manager(Opts({"xpsnr_enabled": True}))
    assert a.xpsnr_enabled is True

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
    b.set_advanced_options(xpsnr_enabled=True)
    b._xpsnr_path = "x_xpsnr.txt"
    b._run_child_job(rp, dp, "vmaf_v0.6.1", "j.json", None, None, 3)
    for c in cmds:
        c[c.index("--master-port") + 1] = "PORT"
    assert "--xpsnr" not in cmds[0] and "--xpsnr" in cmds[1]
    assert cmds[1][cmds[1].index("--xpsnr-log") + 1] == "x_xpsnr.txt"
    assert [c for c in cmds[1] if c not in ("--xpsnr", "--xpsnr-log", "x_xpsnr.txt")] == cmds[0]


def test_score_cli_flag_reaches_score_files(monkeypatch, tmp_path):
    from pqa2_amd import pipeline, score
    seen = []

    def fake(*a, **kw):
        seen.append(kw)
        raise RuntimeError("stop")

    monkeypatch.setattr(pipeline, "score_files", fake)
    monkeypatch.setattr(score, "_die_with_parent", lambda *a, **k: None)
    score.main(["r.y4m", "d.y4m", "--json", str(tmp_path / "x.json")])
    score.main(["r.y4m", "d.y4m", "--json", str(tmp_path / "x.json"), "--xpsnr"])
    score.main(["r.y4m", "d.y4m", "--json", str(tmp_path / "x.json"), "--xpsnr-log", str(tmp_path / "x.txt")])
    assert "xpsnr" not in seen[0] and seen[1]["xpsnr"] is True and seen[2]["xpsnr"] is True


def test_compare_tool_knows_xpsnr(tmp_path):
    import contextlib
    import importlib.util
    from pqa2_amd import report, yuvio
    spec = importlib.util.spec_from_file_location("cmp", os.path.join(ROOT, "tools", "compare_ffmpeg_stats.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert len(mod.XPSNR_VERIFY) == 8
    rp, dp = (os.path.join(CLIPS, f"c64x48_8_{s}.y4m") for s in ("ref", "dist"))
    rr, dr = yuvio.open_video(rp), yuvio.open_video(dp)
    n = min(len(rr), len(dr))
    _, db = R.clip([rr.frame(i) for i in range(n)], [dr.frame(i) for i in range(n)], 8)
    lines = report.xpsnr_stats_lines(db)
    f = tmp_path / "x.txt"
    f.write_text("\n".join(lines) + "\n")
    with contextlib.redirect_stdout(io.StringIO()):
        assert mod.main([rp, dp, "--xpsnr", str(f)]) == 0
    f.write_text("\n".join([lines[0].replace("XPSNR y: ", "XPSNR y: 1")] + lines[1:]) + "\n")
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        assert mod.main([rp, dp, "--xpsnr", str(f)]) == 1
    assert "zero history" in out.getvalue() and "treats as the original" in out.getvalue()
