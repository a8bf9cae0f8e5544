"""cambi without a GPU: the C ABI and its binding, pqa_create's checks, the host-built tables against the restatement
(tests/cambi_ref.py), closed forms of the restatement, and the host layer (pipeline, JSON, analyzer, child-job argv, CLI)
through an oracle-backed engine."""
import ctypes as C
import io
import json
import os
import re

import numpy as np
import pytest

from tests import cambi_ref as R
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
    assert _enum("PQA_FEAT_CAMBI") == 512 == N.FEAT_CAMBI
    assert _enum("PQA_FEAT_CAMBI_FULL_REF") == 1024 == N.FEAT_CAMBI_FULL_REF
    known = re.search(r"PQA_FEAT_KNOWN\s*=([^;]+?)/\*", src, re.S).group(1)
    assert "PQA_FEAT_CAMBI " in known + " " and "PQA_FEAT_CAMBI_FULL_REF" in known
    assert N.FEAT_KNOWN & N.FEAT_CAMBI and N.FEAT_KNOWN & N.FEAT_CAMBI_FULL_REF
    assert not N.FEAT_KNOWN & (1 << 7) and N.FEAT_ALL == 31
    assert (_enum("PQA_EXT_CAMBI"), _enum("PQA_EXT_CAMBI_SOURCE"), _enum("PQA_EXT_DOUBLES")) == (22, 23, 24)
    assert (N.EXT_CAMBI, N.EXT_CAMBI_SOURCE, N.EXT_DOUBLES) == (22, 23, 24)
    assert _enum("PQA_CAMBI_PARAM_INTS") == N.CAMBI_PARAM_INTS == R.N_PARAMS
    assert re.search(r"PQA_API\s+int\s+pqa_debug_cambi_params\s*\(", src)
    assert "pqa_debug_cambi_params" in N.EXPORTS
    lib = N.load()
    assert lib.pqa_profile_kernel_name(5) == b"reserved5" and lib.pqa_profile_kernel_name(6) == b"reserved6"


def _create(**fields):
    from pqa2_amd import _native as N
    lib = N.load()
    cfg = N.PqaConfig()
    lib.pqa_config_init(C.byref(cfg), 352, 288)
    for k, v in fields.items():
        setattr(cfg, k, v)
    ctx = C.c_void_p()
    return lib.pqa_create(C.byref(cfg), C.byref(ctx)), lib.pqa_last_error(None)


def test_create_rejects_12_bit_and_full_ref_alone_without_a_device():
    from pqa2_amd import _native as N
    rc, msg = _create(features=N.FEAT_VMAF | N.FEAT_CAMBI, bit_depth=12)
    assert rc == N.PQA_EINVAL and b"cambi" in msg
    rc, msg = _create(features=N.FEAT_VMAF | N.FEAT_CAMBI_FULL_REF)
    assert rc == N.PQA_EINVAL and b"cambi" in msg
    rc, msg = _create(features=N.FEAT_VMAF | (1 << 7))
    assert rc == N.PQA_EINVAL


@pytest.mark.parametrize("w,h", [(16, 16), (1280, 720), (1920, 1080), (3840, 2160)])
@pytest.mark.parametrize("bpc", [8, 10])
def test_debug_params_equal_the_restatement(w, h, bpc):
    from pqa2_amd import _native as N
    lib = N.load()
    out = (C.c_int32 * N.CAMBI_PARAM_INTS)()
    assert lib.pqa_debug_cambi_params(w, h, bpc, out, N.CAMBI_PARAM_INTS) == N.PQA_OK
    assert list(out) == R.params(w, h)


def test_debug_params_rejects_bad_arguments():
    from pqa2_amd import _native as N
    lib = N.load()
    out = (C.c_int32 * N.CAMBI_PARAM_INTS)()
    assert lib.pqa_debug_cambi_params(352, 288, 12, out, N.CAMBI_PARAM_INTS) == N.PQA_EINVAL
    assert lib.pqa_debug_cambi_params(352, 288, 8, out, N.CAMBI_PARAM_INTS - 1) == N.PQA_EINVAL
    assert lib.pqa_debug_cambi_params(8, 288, 8, out, N.CAMBI_PARAM_INTS) == N.PQA_EINVAL
    assert lib.pqa_debug_cambi_params(352, 288, 8, None, N.CAMBI_PARAM_INTS) == N.PQA_EINVAL


def test_cmap_hook_is_exported_and_checks_its_arguments_first():
    from pqa2_amd import _native as N
    assert re.search(r"PQA_API\s+int\s+pqa_debug_cambi_cmap\s*\(", open(HEADER).read())
    assert "pqa_debug_cambi_cmap" in N.EXPORTS
    lib = N.load()
    y = np.zeros((64, 128), np.uint8)
    total = sum(w * h for w, h in R.scale_sizes(128, 64))
    out = np.zeros(total, np.float32)
    assert lib.pqa_debug_cambi_cmap(y.ctypes.data, 128, 128, 64, 12, out.ctypes.data, total, None) == N.PQA_EINVAL
    assert lib.pqa_debug_cambi_cmap(y.ctypes.data, 128, 128, 64, 8, out.ctypes.data, total - 1, None) == N.PQA_EINVAL
    assert lib.pqa_debug_cambi_cmap(y.ctypes.data, 100, 128, 64, 8, out.ctypes.data, total, None) == N.PQA_EINVAL
    assert lib.pqa_debug_cambi_cmap(None, 128, 128, 64, 8, out.ctypes.data, total, None) == N.PQA_EINVAL


def test_window_and_tvi_tables():
    assert R.window(3840, 2160) == (65, 32, 65 * 65) and R.window(1920, 1080)[:2] == (32, 16)
    tvi = R.tvi_for_diff()
    assert all(64 <= t <= 940 - d for d, t in enumerate(tvi, 1)) and tvi == sorted(tvi)
    for d, t in enumerate(tvi, 1):   # t is the last code value that passes the contrast test
        assert R.eotf(t + d) - R.eotf(t) > 0.019 * R.eotf(t)
        assert not R.eotf(t + 1 + d) - R.eotf(t + 1) > 0.019 * R.eotf(t + 1)


# ---- closed forms of the restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("bpc", [8, 10])
def test_flat_frame_gives_zero(bpc):
    assert R.cambi(np.full((120, 200), 30 if bpc == 8 else 120, np.uint16), bpc) == 0.0


def test_iid_noise_has_an_empty_mask_and_gives_zero():
    rng = np.random.default_rng(3)
    y = rng.integers(0, 1024, (144, 256)).astype(np.uint16)
    p = R.preprocess(y, 10)
    assert not R.spatial_mask(p).any()
    assert R.cambi(y, 10) == 0.0


def test_hand_computed_c_value_and_pooling():
    """A 3 x 3 window (r = 1), all masked: eight samples at 80 (8-bit 20) and one at 84 (8-bit 21).  The centre has
    p0 = 8 and q = 1 at d = 4 only, so c = 4 * 8 * 1 / (8 + 1) in f32; the odd one out has p0 = 1, q = 8: the same."""
    p = np.full((3, 3), 80, np.int32)
    p[0, 0] = 84
    m = np.ones((3, 3), bool)
    c = R.c_values(p, m, 1, R.tvi_for_diff())
    assert c[1, 1] == np.float32(32) / np.float32(9)
    assert c[0, 0] == np.float32(np.float32(4 * 1 * 3) / np.float32(4))   # its window: itself and three 80s
    m[1, 1] = False
    assert R.c_values(p, m, 1, R.tvi_for_diff())[1, 1] == 0.0           # unmasked centres give 0
    # pooling: N = 10, k = 6, the mean of the six largest
    assert R.pool(np.arange(10, dtype=np.float32)) == (9 + 8 + 7 + 6 + 5 + 4) / 6


def _stairs(w, h, step, bands, lo=64):
    x = np.arange(w)[None, :].repeat(h, 0)
    return (lo + (x * bands // w) * step).astype(np.uint16)


def test_small_8_bit_staircase_value():
    """192 x 64 (r = 1, 9-pixel windows), 8-bit 20 | 21 halves: only the two columns at the step see both values.  The
    mask drops rows 0 and h-1 there (S = 4 * 7 - 4 = 24, not > 24).  Rows 2..h-3 have c = 4 * 6 * 3 / 9 = 8 (p0 = 6, q = 3);
    rows 1 and h-2 see masked samples in two window rows only, c = 4 * 4 * 2 / 6.  Fewer than k = 0.6 N c-values are
    non-zero, so P_0 is their sum over k."""
    w, h = 192, 64
    y = np.full((h, w), 20, np.uint8)
    y[:, w // 2:] = 21
    _, r, piw = R.window(w, h)
    assert (r, piw) == (1, 9)
    score, ps, cs = R.cambi_detail(y, 8)
    c0 = cs[0]
    edge = np.float32(32) / np.float32(6)
    want = np.zeros((h, 2), np.float32)
    want[2:-2] = 8.0
    want[[1, -2]] = edge
    assert np.array_equal(c0[:, [w // 2 - 1, w // 2]], want)
    assert (c0[:, : w // 2 - 1] == 0).all() and (c0[:, w // 2 + 1:] == 0).all()
    assert ps[0] == pytest.approx((8.0 * 2 * (h - 4) + float(edge) * 4) / int(0.6 * w * h), rel=1e-15)
    assert score == pytest.approx(sum(wt * P for wt, P in zip(R.CONST["scale_weights"], ps)) / piw, rel=1e-15)
    assert score > 0


def test_larger_steps_score_higher():
    """The same bands one code apart and three codes apart (10 bit): the larger contrast weight wins."""
    fine, coarse = _stairs(320, 180, 1, 10), _stairs(320, 180, 3, 10)
    assert 0 < R.cambi(fine, 10) < R.cambi(coarse, 10)


def test_identical_frames_give_zero_full_reference():
    y = _stairs(320, 180, 2, 12)
    c = R.cambi(y, 10)
    assert c > 0 and R.full_reference(c, R.cambi(y.copy(), 10)) == 0.0
    assert R.full_reference(1.0, 3.0) == 0.0 and R.full_reference(3.0, 1.0) == 2.0


def test_twelve_bit_is_not_defined():
    with pytest.raises(ValueError, match="cambi"):
        R.cambi(np.zeros((32, 32), np.uint16), 12)


# ---- host layer through an oracle-backed engine --------------------------------------------------------------------
class CambiEngine(OracleEngine):
    """OracleEngine plus the extension record's cambi slots (the restatement stands in for the kernels)."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.frames = {}

    def submit(self, index, ref_planes, dis_planes):
        super().submit(index, ref_planes, dis_planes)
        self.frames[index] = (np.array(ref_planes[0]), np.array(dis_planes[0]))

    def collect_blocks(self, first, count, blocks):
        got = self.collect_ext(first, count)
        return got[0], {i: got[1 + i] for i in blocks}

    def collect_ext(self, first, count):
        from pqa2_amd import _native as N
        ext = np.full((count, N.EXT_DOUBLES), np.nan)
        for i in range(count):
            if (first + i) % self.k == 0 and self.features & N.FEAT_CAMBI:
                r, d = self.frames[first + i]
                ext[i, N.EXT_CAMBI] = R.cambi(d, self.bpc)
                if self.features & N.FEAT_CAMBI_FULL_REF:
                    ext[i, N.EXT_CAMBI_SOURCE] = R.cambi(r, self.bpc)
        return self.collect(first, count), ext


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


def _banded_clip(tmp_path):
    from pqa2_amd import synth, yuvio
    w, h, n = 320, 180, 3
    info = synth.clip_info(w, h, 8, chroma=False)
    refs = [[(20 + (np.arange(w)[None, :].repeat(h, 0) * (30 + i) // w)).astype(np.uint8)] for i in range(n)]
    diss = [[(20 + (np.arange(w)[None, :].repeat(h, 0) * (8 + i) // w)).astype(np.uint8)] for i in range(n)]
    rp, dp = str(tmp_path / "r.y4m"), str(tmp_path / "d.y4m")
    yuvio.write_y4m(rp, refs, info)
    yuvio.write_y4m(dp, diss, info)
    return rp, dp, refs, diss


def test_json_gains_cambi_keys_only_when_enabled(tmp_path):
    rp, dp, refs, diss = _banded_clip(tmp_path)
    _, old = _score(tmp_path, "old", OracleEngine, (rp, dp))
    _, new_default = _score(tmp_path, "new", CambiEngine, (rp, dp))
    assert new_default == old and "cambi" not in old
    _, text = _score(tmp_path, "one", CambiEngine, (rp, dp), cambi=True)
    log = json.loads(text)
    for i, fr in enumerate(log["frames"]):
        assert fr["metrics"]["cambi"] == float(f"{R.cambi(diss[i][0], 8):.6f}")
        assert "cambi_source" not in fr["metrics"] and "cambi_full_reference" not in fr["metrics"]
    _, text = _score(tmp_path, "full", CambiEngine, (rp, dp), cambi=True, cambi_full_ref=True)
    log = json.loads(text)
    for i, fr in enumerate(log["frames"]):
        d, s = R.cambi(diss[i][0], 8), R.cambi(refs[i][0], 8)
        assert fr["metrics"]["cambi_source"] == float(f"{s:.6f}")
        assert fr["metrics"]["cambi_full_reference"] == float(f"{R.full_reference(d, s):.6f}")
    for key in ("cambi", "cambi_source", "cambi_full_reference"):
        assert set(log["pooled_metrics"][key]) == {"min", "max", "mean", "harmonic_mean"}
    old_log = json.loads(old)
    for a, b in zip(old_log["frames"], log["frames"]):
        assert all(b["metrics"][k] == v for k, v in a["metrics"].items())


def test_full_ref_without_cambi_is_an_error(tmp_path):
    with pytest.raises(ValueError, match="cambi"):
        _score(tmp_path, "bad", CambiEngine, cambi_full_ref=True)


def test_n_subsample_drops_frames_like_the_other_keys(tmp_path):
    res, _ = _score(tmp_path, "sub", CambiEngine, cambi=True, cambi_full_ref=True, n_subsample=2)
    assert list(res["frame_indices"]) == [0, 2]
    for key in ("cambi", "cambi_source", "cambi_full_reference"):
        assert len(res["metrics"][key]) == 2 and not np.isnan(res["metrics"][key]).any()


def test_analyzer_options_round_trip():
    from pqa2_amd.vmaf_analyzer import VMAFAnalyzer
    a = VMAFAnalyzer()
    assert a.cambi_enabled is False and a.cambi_full_ref_enabled is False
    a.set_advanced_options("mean", False, False, 1, True, True)
    assert a.cambi_enabled is False
    a.set_advanced_options(cambi_enabled=True)
    assert a._ssim_family_kwargs() == {"cambi": True}
    a.set_advanced_options(cambi_enabled=True, cambi_full_ref_enabled=True)
    assert a._ssim_family_kwargs() == {"cambi": True, "cambi_full_ref": True}
    a.set_advanced_options(cambi_full_ref_enabled=True)      # full reference alone asks for nothing
    assert a._ssim_family_kwargs() == {}

    class Opts:
        def __init__(self, d):
            self.d = d

        def get_setting(self, k):
            return self.d

    a.set_options_from_manager(Opts({"cambi_enabled": True, "cambi_full_ref_enabled": True}))
    assert a.cambi_enabled is True and a.cambi_full_ref_enabled is True
    a.set_options_from_manager(Opts({}))
    assert a.cambi_enabled is False and a.cambi_full_ref_enabled is False


def test_analyzer_results_and_child_argv(tmp_path, monkeypatch):
    from pqa2_amd import vmaf_analyzer as V
    rp, dp, _, _ = _banded_clip(tmp_path)
    a = V.VMAFAnalyzer()
    a.set_output_directory(str(tmp_path))
    a._engine_factory = CambiEngine
    res = a.analyze_videos(rp, dp)
    assert res is not None and "cambi" not in res
    a.set_advanced_options(cambi_enabled=True, cambi_full_ref_enabled=True)
    res = a.analyze_videos(rp, dp)
    pooled = res["raw_results"]["pooled_metrics"]
    for key in ("cambi", "cambi_source", "cambi_full_reference"):
        assert res[key] == pooled[key]["mean"]

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
    b.set_advanced_options(cambi_enabled=True)
    b._run_child_job(rp, dp, "vmaf_v0.6.1", "j.json", None, None, 3)
    b.set_advanced_options(cambi_enabled=True, cambi_full_ref_enabled=True)
    b._run_child_job(rp, dp, "vmaf_v0.6.1", "j.json", None, None, 3)
    for c in cmds:
        c[c.index("--master-port") + 1] = "PORT"
    assert "--cambi" not in cmds[0] and "--cambi" in cmds[1] and "--cambi-full-ref" not in cmds[1]
    assert [c for c in cmds[1] if c != "--cambi"] == cmds[0]
    assert [c for c in cmds[2] if c not in ("--cambi", "--cambi-full-ref")] == cmds[0] and "--cambi-full-ref" in cmds[2]


def test_score_cli_flags_reach_score_files(monkeypatch, tmp_path):
    from pqa2_amd import pipeline, score
    seen = []

    def fake(*a, **kw):
        seen.append(kw)
        raise RuntimeError("stop")

    monkeypatch.setattr(pipeline, "score_files", fake)
    monkeypatch.setattr(score, "_die_with_parent", lambda *a, **k: None)
    score.main(["r.y4m", "d.y4m", "--json", str(tmp_path / "x.json")])
    score.main(["r.y4m", "d.y4m", "--json", str(tmp_path / "x.json"), "--cambi"])
    score.main(["r.y4m", "d.y4m", "--json", str(tmp_path / "x.json"), "--cambi", "--cambi-full-ref"])
    assert "cambi" not in seen[0] and "cambi_full_ref" not in seen[0]
    assert seen[1]["cambi"] is True and "cambi_full_ref" not in seen[1]
    assert seen[2]["cambi"] is True and seen[2]["cambi_full_ref"] is True


def test_compare_tool_knows_the_cambi_keys():
    import importlib.util
    spec = importlib.util.spec_from_file_location("cmp", os.path.join(ROOT, "tools", "compare_libvmaf_log.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.CAMBI_KEYS == ("cambi", "cambi_source", "cambi_full_reference")
    assert any("VERIFY" in line for line in mod.SSIM_IMPLICATES["cambi"])


def test_compare_tool_stops_on_a_12_bit_clip(tmp_path):
    import importlib.util
    from pqa2_amd import synth, yuvio
    spec = importlib.util.spec_from_file_location("cmp", os.path.join(ROOT, "tools", "compare_libvmaf_log.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    refs, diss = synth.make_clip(64, 48, 1, 12, chroma=False)
    info = synth.clip_info(64, 48, 12, chroma=False)
    rp, dp = str(tmp_path / "r.y4m"), str(tmp_path / "d.y4m")
    yuvio.write_y4m(rp, refs, info)
    yuvio.write_y4m(dp, diss, info)
    with pytest.raises(SystemExit, match="12-bit"):
        mod.cambi_columns(rp, dp, False, 1)
