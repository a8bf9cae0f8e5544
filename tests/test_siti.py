"""siti without a GPU: the C ABI and its binding (PQA_FEAT_SITI and its range bits, the fourth extension record), the
restatement (tests/siti_ref.py) against closed forms and a hand-worked case that do not go through it, and the host layer
(pipeline, range bits, sharding history, JSON, analyzer, child-job argv, CLI) through an oracle-backed engine."""
import io
import json
import math
import os
import re

import numpy as np
import pytest

from tests import siti_ref as R
from tests.fake_engine import OracleEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pqa_vmaf.h")
CLIPS = os.path.join(ROOT, "tests", "golden", "clips")
KEYS = ("siti_si", "siti_ti", "siti_si_source", "siti_ti_source")


def _enum(name):
    return int(eval(re.search(name + r"\s*=\s*([^,/\n}]+)", open(HEADER).read()).group(1).replace("u", "")))


# ---- ABI --------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree():
    from pqa2_amd import _native as N
    src = open(HEADER).read()
    assert _enum("PQA_FEAT_SITI") == 16384 == N.FEAT_SITI
    assert _enum("PQA_FEAT_SITI_REF_FULL") == 32768 == N.FEAT_SITI_REF_FULL
    assert _enum("PQA_FEAT_SITI_DIS_FULL") == 65536 == N.FEAT_SITI_DIS_FULL
    known = re.search(r"PQA_FEAT_KNOWN\s*=([^;]+?)/\*", src, re.S).group(1)
    for b in ("PQA_FEAT_SITI", "PQA_FEAT_SITI_REF_FULL", "PQA_FEAT_SITI_DIS_FULL"):
        assert b in known
    assert N.FEAT_KNOWN & 16384 and N.FEAT_KNOWN & 32768 and N.FEAT_KNOWN & 65536 and N.FEAT_ALL == 31
    slots = ("PQA_EXT4_SI", "PQA_EXT4_TI", "PQA_EXT4_SI_SOURCE", "PQA_EXT4_TI_SOURCE", "PQA_EXT4_RESERVED", "PQA_EXT4_DOUBLES")
    assert tuple(_enum(s) for s in slots) == (0, 1, 2, 3, 4, 8)
    assert (N.EXT4_SI, N.EXT4_TI, N.EXT4_SI_SOURCE, N.EXT4_TI_SOURCE, N.EXT4_RESERVED, N.EXT4_DOUBLES) == (0, 1, 2, 3, 4, 8)
    assert (N.EXT_DOUBLES, N.EXT2_DOUBLES, N.EXT3_DOUBLES, N.PROF_KERNELS) == (24, 8, 8, 17)
    for fn in ("pqa_ext4_doubles", "pqa_collect_ext4", "pqa_set_dis_history", "pqa_debug_siti_plane"):
        assert re.search(r"PQA_API\s+int\s+" + fn + r"\s*\(", src), fn
        assert fn in N.EXPORTS, fn


def test_library_exports_and_create_checks_without_a_device():
    import ctypes as C
    from pqa2_amd import _native as N
    lib = N.load()
    assert lib.pqa_ext4_doubles() == 8

    def create(feats, bpc=8):
        cfg = N.PqaConfig()
        lib.pqa_config_init(C.byref(cfg), 64, 48)
        cfg.features = feats
        cfg.bit_depth = bpc
        ctx = C.c_void_p()
        rc = lib.pqa_create(C.byref(cfg), C.byref(ctx))
        return rc, lib.pqa_last_error(None).decode()

    for feats in (N.FEAT_VMAF | N.FEAT_SITI_REF_FULL, N.FEAT_SITI_DIS_FULL):
        rc, msg = create(feats)
        assert rc == N.PQA_EINVAL and "siti" in msg
    rc, msg = create(N.FEAT_SITI, 12)
    assert rc == N.PQA_EINVAL and "siti" in msg
    for bpc in (8, 10):   # accepted as far as siti goes (without a device: the device error)
        assert "siti" not in create(N.FEAT_SITI | N.FEAT_SITI_REF_FULL | N.FEAT_SITI_DIS_FULL, bpc)[1]
    out = np.zeros(2)
    assert lib.pqa_debug_siti_plane(None, None, 3, 3, 3, 8, 0, None, out.ctypes.data) == N.PQA_EINVAL
    plane = np.zeros((2, 2), np.uint8)
    assert lib.pqa_debug_siti_plane(plane.ctypes.data, None, 2, 2, 2, 8, 0, None, out.ctypes.data) == N.PQA_EINVAL
    plane = np.zeros((3, 3), np.uint16)
    assert lib.pqa_debug_siti_plane(plane.ctypes.data, None, 6, 3, 3, 12, 0, None, out.ctypes.data) == N.PQA_EINVAL


# ---- the restatement -----------------------------------------------------------------------------------------------------
def test_range_conversion_endpoints():
    assert list(R.to_full([16, 235, 0, 15, 236, 255], 8)) == [0, 255, 0, 0, 255, 255]
    assert list(R.to_full([64, 940, 0, 63, 941, 1023], 10)) == [0, 1023, 0, 0, 1023, 1023]
    assert list(R.to_full([17, 126], 8)) == [255 // 219, (255 * 110) // 219]        # truncating
    assert list(R.to_full([0, 255], 8, full=True)) == [0, 255]
    y = np.arange(256)
    assert (np.diff(R.to_full(y, 8)) >= 0).all()


@pytest.mark.parametrize("bpc", [8, 10])
def test_flat_plane_and_ramp_have_zero_si(bpc):
    top = (1 << bpc) - 1
    assert R.frame(np.full((9, 11), top // 2), None, bpc, True) == (0.0, 0.0)
    for slope in (1, 3, 7):
        yy, xx = np.mgrid[0:20, 0:30]
        for ramp in (slope * xx, slope * yy, slope * (xx + yy)):
            yf = R.to_full(ramp, bpc, True)
            g = R.gradient_map(yf)
            assert np.all(g == g[0, 0]) and R.std(g) == 0.0 and R.std(g, "ffmpeg") == 0.0
        assert R.gradient_map(slope * xx)[0, 0] == 8 * slope


def test_hand_worked_5x5_si():
    # a vertical edge: columns 0, 0, 10, 10, 10 on every row.  gx = s(x-1) - s(x+1) with s = 4 v: -40, -40, 0 per interior
    # row, gy = 0; the map is [40, 40, 0] three times, mean 80 / 3, SI = sqrt(((40/3)^2 * 2 + (80/3)^2) / 3) = 40 sqrt(2) / 3
    p = np.tile(np.array([0, 0, 10, 10, 10]), (5, 1))
    g = R.gradient_map(p)
    assert g.tolist() == [[40.0, 40.0, 0.0]] * 3
    si, ti = R.frame(p, None, 8, True)
    assert abs(si - 40 * math.sqrt(2) / 3) < 1e-12 and ti == 0.0
    # a single bright pixel: the 3 x 3 interior sees the full kernels around it
    q = np.zeros((5, 5), np.int64)
    q[2, 2] = 1
    gx, gy = R.sobel(q)
    assert gx.tolist() == [[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]] and gy.tolist() == [[-1, -2, -1], [0, 0, 0], [1, 2, 1]]


@pytest.mark.parametrize("bpc", [8, 10])
def test_ti_closed_forms(bpc):
    rng = np.random.default_rng(bpc)
    top = (1 << bpc) - 1
    a = rng.integers(0, top // 2, (24, 32))
    assert R.frame(a + 5, a, bpc, True)[1] == 0.0                    # a frame plus a constant
    assert R.frame(a, a, bpc, True)[1] == 0.0                        # a repeated frame, exactly 0
    assert R.frame(a, a, bpc)[1] == 0.0
    for c in (2, 9, 40):
        b = a.copy()
        b[:, :16] += c                                               # half the pixels rise by c
        assert R.frame(b, a, bpc, True)[1] == c / 2
        assert R.frame(b, a, bpc, True, "ffmpeg")[1] == c / 2
    si, ti = R.clip([a, a + 1, a + 1], bpc, True)
    assert ti.tolist() == [0.0, 0.0, 0.0] and si[0] == si[1]       # first frame 0, constant step 0, repeat 0


@pytest.mark.parametrize("bpc", [8, 10])
@pytest.mark.parametrize("full", [False, True])
def test_ffmpeg_and_f64_modes_agree(bpc, full):
    rng = np.random.default_rng(7 + bpc)
    top = (1 << bpc) - 1
    yy, xx = np.mgrid[0:90, 0:120]
    base = (0.5 + 0.4 * np.sin(xx * 0.2) * np.cos(yy * 0.13)) * top
    lumas = [np.clip(np.rint(np.roll(base, 3 * k, 1) + rng.normal(0, top * 0.03, base.shape)), 0, top).astype(np.int64)
             for k in range(3)]
    s64, t64 = R.clip(lumas, bpc, full)
    sff, tff = R.clip(lumas, bpc, full, "ffmpeg")
    assert np.allclose(sff, s64, rtol=1e-6, atol=0) and np.allclose(tff, t64, rtol=1e-6, atol=0)
    a, b = R.summary(s64, t64), R.summary(sff, tff, "ffmpeg")
    for k in ("si", "ti"):
        for s in ("avg", "max", "min"):
            assert abs(a[k][s] - b[k][s]) <= 1e-6 * max(abs(a[k][s]), 1.0)
    assert a["si"]["max"] == max(s64) and a["ti"]["min"] == 0.0


def test_const_table_and_verify_list():
    assert R.CONST["factor"] == {8: 1, 10: 4} and R.CONST["full_upper"] == 256 and R.CONST["limited_span"] == 219
    assert len(R.VERIFY) >= 5


# ---- host layer through an oracle-backed engine ----------------------------------------------------------------------
class SitiEngine(OracleEngine):
    """OracleEngine plus the fourth extension record (the restatement stands in for the kernel) and both histories."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.frames, self.ref_prev, self.dis_prev, self.dis_calls = {}, None, None, []

    def set_motion_halo(self, prev):
        super().set_motion_halo(prev)
        self.ref_prev = None if prev is None else np.array(prev)

    def set_ref_history(self, planes):
        self.set_motion_halo(planes[0] if planes else None)

    def set_dis_history(self, prev):
        self.dis_calls.append(prev is not None)
        self.dis_prev = None if prev is None else np.array(prev)

    def submit(self, index, ref_planes, dis_planes):
        super().submit(index, ref_planes, dis_planes)
        self.frames[index] = (np.array(ref_planes[0]), np.array(dis_planes[0]))

    def collect_blocks(self, first, count, blocks):
        got = self.collect_ext4(first, count)
        return got[0], {i: got[1 + i] for i in blocks}

    def collect_ext4(self, first, count):
        from pqa2_amd import _native as N
        idx = sorted(self.frames)
        rf = bool(self.features & N.FEAT_SITI_REF_FULL)
        df = bool(self.features & N.FEAT_SITI_DIS_FULL)
        dsi, dti = R.clip([self.frames[i][1] for i in idx], self.bpc, df, prev=self.dis_prev)
        rsi, rti = R.clip([self.frames[i][0] for i in idx], self.bpc, rf, prev=self.ref_prev)
        ext4 = np.full((count, N.EXT4_DOUBLES), np.nan)
        for j in range(count):
            k = idx.index(first + j)
            ext4[j, :4] = (dsi[k], dti[k], rsi[k], rti[k])
        return (self.collect(first, count), np.full((count, N.EXT_DOUBLES), np.nan),
                np.full((count, N.EXT2_DOUBLES), np.nan), np.full((count, N.EXT3_DOUBLES), np.nan), ext4)


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


def test_json_gains_siti_keys_only_when_enabled(tmp_path):
    from pqa2_amd import yuvio
    _, old = _score(tmp_path, "old", OracleEngine)
    _, new_default = _score(tmp_path, "new", SitiEngine)
    assert new_default == old and "siti" not in old
    res, text = _score(tmp_path, "on", SitiEngine, siti=True)
    log = json.loads(text)
    rr, dr = (yuvio.open_video(p) for p in _clip_paths())
    n = len(log["frames"])
    dsi, dti = R.clip([dr.frame(i)[0] for i in range(n)], 8)
    rsi, rti = R.clip([rr.frame(i)[0] for i in range(n)], 8)
    want = dict(zip(KEYS, (dsi, dti, rsi, rti)))
    for i, fr in enumerate(log["frames"]):
        for k in KEYS:
            assert fr["metrics"][k] == float(f"{want[k][i]:.6f}"), (i, k)
    for k in KEYS:
        pooled = log["pooled_metrics"][k]
        assert pooled["mean"] == float(f"{np.mean(want[k]):.6f}") and pooled["max"] == float(f"{np.max(want[k]):.6f}")
    assert log["frames"][0]["metrics"]["siti_ti"] == 0.0 and log["frames"][1]["metrics"]["siti_ti"] > 0
    old_log = json.loads(old)
    for a, b in zip(old_log["frames"], log["frames"]):
        assert all(b["metrics"][k] == v for k, v in a["metrics"].items())


def test_full_range_header_sets_that_clips_bit(tmp_path):
    from pqa2_amd import _native as N
    from pqa2_amd import synth, yuvio
    refs, diss = synth.make_clip(64, 48, 3, 8, chroma=True)
    seen = []

    def factory(*a, **kw):
        seen.append(kw["features"])
        return SitiEngine(*a, **kw)

    for ref_range, dis_range in ((None, None), ("full", None), (None, "full"), ("limited", "full"), ("full", "full")):
        paths = []
        for tag, frames, rng in (("r", refs, ref_range), ("d", diss, dis_range)):
            info = synth.clip_info(64, 48, 8, chroma=True)
            info.color_range = rng
            p = str(tmp_path / f"{tag}_{ref_range}_{dis_range}.y4m")
            yuvio.write_y4m(p, frames, info)
            paths.append(p)
        res, _ = _score(tmp_path, "fr", factory, tuple(paths), siti=True)
        f = seen[-1]
        assert f & N.FEAT_SITI
        assert bool(f & N.FEAT_SITI_REF_FULL) == (ref_range == "full")
        assert bool(f & N.FEAT_SITI_DIS_FULL) == (dis_range == "full")
        want = R.clip([d[0] for d in diss], 8, dis_range == "full")[0]
        assert np.allclose(res["metrics"]["siti_si"], want, rtol=0, atol=0)
    _score(tmp_path, "off", factory, None)
    assert not seen[-1] & (N.FEAT_SITI | N.FEAT_SITI_REF_FULL | N.FEAT_SITI_DIS_FULL)


def test_every_frame_scored_and_monochrome_clips_work(tmp_path):
    from pqa2_amd import synth, yuvio
    res, _ = _score(tmp_path, "sub", SitiEngine, siti=True, n_subsample=2)
    assert list(res["frame_indices"]) == [0, 2] and len(res["metrics"]["siti_ti"]) == 2
    refs, diss = synth.make_clip(64, 48, 3, 10, chroma=False)
    info = synth.clip_info(64, 48, 10, chroma=False)
    rp, dp = str(tmp_path / "r.y4m"), str(tmp_path / "d.y4m")
    yuvio.write_y4m(rp, refs, info)
    yuvio.write_y4m(dp, diss, info)
    res, _ = _score(tmp_path, "mono", SitiEngine, (rp, dp), siti=True, psnr=False, ssim=False)
    assert all(k in res["metrics"] for k in KEYS)


def test_shards_arm_the_distorted_history(tmp_path, monkeypatch):
    full, _ = _score(tmp_path, "full", SitiEngine, siti=True, psnr=False, ssim=False)
    engines = []

    def factory(*a, **kw):
        engines.append(SitiEngine(*a, **kw))
        return engines[-1]

    from pqa2_amd import shard
    from pqa2_amd.pipeline import score_files
    rp, dp = _clip_paths()
    a, _ = shard.shard_bounds(3, 3, 2)
    monkeypatch.setattr(shard, "gather_records", lambda local, n, *x, width=24, **k: np.zeros((n, width)))
    assert score_files(rp, dp, "vmaf_v0.6.1", engine_factory=factory, siti=True, psnr=False, ssim=False,
                       rank=2, world_size=3) is None
    eng = engines[-1]
    assert eng.dis_calls == [True] and a == 2
    row = eng.collect_ext4(2, 1)[4][0]
    for j, k in enumerate(KEYS):
        assert row[j] == full["metrics"][k][2], k
    assert score_files(rp, dp, "vmaf_v0.6.1", engine_factory=factory, psnr=False, ssim=False, rank=2,
                       world_size=3) is None
    assert engines[-1].dis_calls == []


def test_analyzer_options_results_and_child_argv(tmp_path, monkeypatch):
    from pqa2_amd import vmaf_analyzer as V
    rp, dp = _clip_paths()
    a = V.VMAFAnalyzer()
    assert a.siti_enabled is False
    a.set_output_directory(str(tmp_path))
    a._engine_factory = SitiEngine
    res = a.analyze_videos(rp, dp)
    assert res is not None and "siti_si" not in res
    a.set_advanced_options(siti_enabled=True)
    assert a._ssim_family_kwargs() == {"siti": True}
    res = a.analyze_videos(rp, dp)
    rr, dr = (__import__("pqa2_amd.yuvio", fromlist=["x"]).open_video(p) for p in (rp, dp))
    n = min(len(rr), len(dr))
    dsi, dti = R.clip([dr.frame(i)[0] for i in range(n)], 8)
    rsi, rti = R.clip([rr.frame(i)[0] for i in range(n)], 8)
    for k, v in zip(KEYS, (dsi, dti, rsi, rti)):
        assert res[k] == float(f"{np.mean(v):.6f}"), k
    assert res["siti_si_max"] == float(f"{np.max(dsi):.6f}") and res["siti_ti_max"] == float(f"{np.max(dti):.6f}")

    class Opts:
        def __init__(self, d):
            self.d = d

        def get_setting(self, k):
            return self.d

    a.set_options_from_manager(Opts({"siti_enabled": True}))
    assert a.siti_enabled is True
    a.set_options_from_manager(Opts({}))
    assert a.siti_enabled is False

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
    b.set_advanced_options(siti_enabled=True)
    b._run_child_job(rp, dp, "vmaf_v0.6.1", "j.json", None, None, 3)
    for c in cmds:
        c[c.index("--master-port") + 1] = "PORT"
    assert "--siti" not in cmds[0] and "--siti" in cmds[1]
    assert [c for c in cmds[1] if c != "--siti"] == cmds[0]


def test_score_cli_flag_reaches_score_files(monkeypatch, tmp_path):
    from pqa2_amd import pipeline, score
    seen = []

    def fake(*a, **kw):
        seen.append(kw)
        raise RuntimeError("stop")

    monkeypatch.setattr(pipeline, "score_files", fake)
    monkeypatch.setattr(score, "_die_with_parent", lambda *a, **k: None)
    score.main(["r.y4m", "d.y4m", "--json", str(tmp_path / "x.json")])
    score.main(["r.y4m", "d.y4m", "--json", str(tmp_path / "x.json"), "--siti"])
    assert "siti" not in seen[0] and seen[1]["siti"] is True
