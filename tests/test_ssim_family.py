"""float_ssim / float_ms_ssim without a GPU: the restatement's closed forms, the C ABI and its binding, the host layer
(pipeline, JSON, analyzer, child-job argv) through an oracle-backed engine, and the kernels' register budget."""
import ctypes as C
import io
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests import ssim_family_ref as R
from tests.fake_engine import OracleEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pqa_vmaf.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "clips")


# ---- the restatement ---------------------------------------------------------------------------------------------
def _pair(w, h, seed=1, bpc=8):
    rng = np.random.default_rng(seed)
    top = (1 << bpc) - 1
    a = rng.integers(0, top + 1, (h, w))
    b = np.clip(a + rng.integers(-40 << (bpc - 8), 40 << (bpc - 8), a.shape), 0, top)
    dt = np.uint8 if bpc == 8 else np.uint16
    return a.astype(dt), b.astype(dt)


@pytest.mark.parametrize("w,h", [(161, 161), (200, 300), (640, 360)])
def test_identical_frames_give_exactly_one(w, h):
    a, _ = _pair(w, h)
    assert R.float_ssim(a, a)["float_ssim"] == 1.0
    assert R.ms_ssim(a, a)["float_ms_ssim"] == 1.0


@pytest.mark.parametrize("va,vb,bpc", [(16, 235, 8), (100, 101, 8), (0, 255, 8), (512, 300, 10), (4000, 12, 12)])
def test_constant_frames_closed_form(va, vb, bpc):
    w, h = 176, 200
    dt = np.uint8 if bpc == 8 else np.uint16
    a, b = np.full((h, w), va, dt), np.full((h, w), vb, dt)
    x, y = va / float(1 << (bpc - 8)), vb / float(1 << (bpc - 8))
    l = (2 * x * y + R.C1) / (x * x + y * y + R.C1)
    assert abs(R.float_ssim(a, b, bpc)["float_ssim"] - l) < 1e-12
    assert abs(R.ms_ssim(a, b, bpc)["float_ms_ssim"] - l ** 0.1333) < 1e-12


@pytest.mark.parametrize("w,h,bpc", [(161, 170, 8), (300, 257, 10), (520, 400, 12)])
def test_two_d_and_separable_windows_agree(w, h, bpc):
    a, b = _pair(w, h, seed=w, bpc=bpc)
    f2, fs = R.float_ssim(a, b, bpc), R.float_ssim(a, b, bpc, separable=True)
    m2, ms = R.ms_ssim(a, b, bpc), R.ms_ssim(a, b, bpc, separable=True)
    for k in ("float_ssim", "l", "c", "s"):
        assert abs(f2[k] - fs[k]) < 1e-12
    assert abs(m2["float_ms_ssim"] - ms["float_ms_ssim"]) < 1e-12
    for k in ("l", "c", "s"):
        assert np.abs(np.subtract(m2[k], ms[k])).max() < 1e-12


def test_negative_mean_under_fractional_exponent_is_nan():
    """Anti-correlated frames: the s means of the fine scales are negative; C pow makes float_ms_ssim NaN (defined)."""
    a, _ = _pair(176, 176, seed=3)
    d = R.ms_ssim(a, (255 - a).astype(np.uint8))
    assert min(d["s"]) < 0 and np.isnan(d["float_ms_ssim"])
    assert np.isnan(R.ms_combine([1.0, 1.0, 1.0, 1.0, -0.5], [1.0] * 5, [1.0] * 5))
    assert R.ms_combine([-0.5, 1.0, 1.0, 1.0, 1.0], [1.0] * 5, [1.0] * 5) == 1.0   # l_0..l_3 ^ 0 = 1
    assert R.ms_combine([1.0] * 5, [1.0] * 5, [0.0, 1.0, 1.0, 1.0, 1.0]) == 0.0


def test_size_rules():
    assert R.decimation_factor(1920, 1080) == 4 and R.decimation_factor(3840, 2160) == 8
    assert R.decimation_factor(352, 288) == 1 and R.decimation_factor(640, 384) == 2
    assert R.ms_ssim_fits(161, 161) and not R.ms_ssim_fits(160, 400) and not R.ms_ssim_fits(176, 144)
    assert R.float_ssim_fits(16, 16)


# ---- C ABI and binding --------------------------------------------------------------------------------------------
def _enum(name):
    src = open(HEADER).read()
    m = re.search(rf"\b{name}\s*=\s*([^,\n/}}]+)", src)
    assert m, name
    return eval(m.group(1).replace("1u", "1").replace("PQA_FEAT_", "F_"), {}, {
        "F_VMAF": 7, "F_VIF": 1, "F_ADM": 2, "F_MOTION": 4, "F_PSNR": 8, "F_SSIM": 16, "F_ALL": 31,
        "F_FLOAT_SSIM": 32, "F_MS_SSIM": 64})


def test_header_declares_the_extension_abi():
    src = open(HEADER).read()
    for sym in ("pqa_collect_ext", "pqa_ext_doubles"):
        assert re.search(rf"PQA_API\s+int\s+{sym}\s*\(", src), sym
    assert _enum("PQA_FEAT_FLOAT_SSIM") == 32 and _enum("PQA_FEAT_MS_SSIM") == 64
    assert _enum("PQA_FEAT_ALL") == 31
    assert _enum("PQA_EXT_DOUBLES") == 24
    assert [_enum(k) for k in ("PQA_EXT_FLOAT_SSIM", "PQA_EXT_MS_SSIM", "PQA_EXT_MS_SSIM_L", "PQA_EXT_MS_SSIM_C",
                               "PQA_EXT_MS_SSIM_S", "PQA_EXT_RESERVED")] == [0, 4, 5, 10, 15, 20]
    assert _enum("PQA_PROF_KERNELS") == 17


def test_binding_and_library_agree_with_the_header():
    from pqa2_amd import _native as N
    assert (N.FEAT_FLOAT_SSIM, N.FEAT_MS_SSIM, N.FEAT_ALL, N.EXT_DOUBLES, N.PROF_KERNELS) == (32, 64, 31, 24, 17)
    assert (N.EXT_FLOAT_SSIM, N.EXT_FLOAT_SSIM_LCS, N.EXT_MS_SSIM, N.EXT_MS_SSIM_L, N.EXT_MS_SSIM_C, N.EXT_MS_SSIM_S,
            N.EXT_RESERVED) == (0, 1, 4, 5, 10, 15, 20)
    assert {"pqa_collect_ext", "pqa_ext_doubles"} <= set(N.EXPORTS)
    lib = N.load()
    assert hasattr(lib, "pqa_collect_ext") and lib.pqa_ext_doubles() == 24
    assert lib.pqa_profile_kernel_name(15) == b"ms_ssim" and lib.pqa_profile_kernel_name(16) == b"float_ssim"


def test_create_rejects_unknown_bits_and_too_small_frames_without_a_device():
    """Mask and geometry are checked before any device is touched, naming the feature."""
    from pqa2_amd import _native as N
    lib = N.load()
    for w, h, feat, text in ((352, 288, 1 << 7, b"feature mask"), (176, 144, N.FEAT_MS_SSIM, b"float_ms_ssim"),
                             (160, 400, N.FEAT_VMAF | N.FEAT_MS_SSIM, b"float_ms_ssim")):
        cfg = N.PqaConfig()
        lib.pqa_config_init(C.byref(cfg), w, h)
        cfg.features = feat
        ctx = C.c_void_p()
        assert lib.pqa_create(C.byref(cfg), C.byref(ctx)) == N.PQA_EINVAL
        assert text in lib.pqa_last_error(None)


# ---- host layer through an oracle-backed engine --------------------------------------------------------------------
class SsimFamilyEngine(OracleEngine):
    """OracleEngine plus the extension record (the restatement stands in for the kernels)."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.lumas = {}

    def submit(self, index, ref_planes, dis_planes):
        super().submit(index, ref_planes, dis_planes)
        self.lumas[index] = (np.array(ref_planes[0]), np.array(dis_planes[0]))

    def collect_blocks(self, first, count, blocks):
        got = self.collect_ext(first, count)
        return got[0], {i: got[1 + i] for i in blocks}

    def collect_ext(self, first, count):
        from pqa2_amd import _native as N
        ext = np.full((count, N.EXT_DOUBLES), np.nan)
        for i in range(count):
            if (first + i) % self.k == 0:
                r, d = self.lumas[first + i]
                ext[i] = R.ext_record(r, d, self.bpc, bool(self.features & N.FEAT_FLOAT_SSIM),
                                      bool(self.features & N.FEAT_MS_SSIM))
        return self.collect(first, count), ext


def _score(tmp_path, tag, factory, **kw):
    from pqa2_amd import report
    from pqa2_amd.pipeline import score_files
    rp, dp = (os.path.join(GOLDEN, f"c352x288_8_{s}.y4m") for s in ("ref", "dist"))
    res = score_files(rp, dp, "vmaf_v0.6.1", engine_factory=factory, **kw)
    log = report.build_vmaf_log(res["metrics"], 0.0, res["frame_indices"], {"model": res["model_name"]})
    path = str(tmp_path / f"{tag}.json")
    report.write_vmaf_json(path, log)
    return res, open(path).read()


def test_json_gains_the_keys_only_when_enabled(tmp_path):
    from pqa2_amd import yuvio
    _, old = _score(tmp_path, "old", OracleEngine)
    _, new_default = _score(tmp_path, "new", SsimFamilyEngine)
    assert new_default == old                                       # default log byte-identical
    assert "ssim" in old and "float_ssim" not in old and "float_ms_ssim" not in old
    res, text = _score(tmp_path, "ext", SsimFamilyEngine, float_ssim=True, ms_ssim=True)
    log = json.loads(text)
    rr = yuvio.open_video(os.path.join(GOLDEN, "c352x288_8_ref.y4m"))
    dr = yuvio.open_video(os.path.join(GOLDEN, "c352x288_8_dist.y4m"))
    for i, fr in enumerate(log["frames"]):
        want = R.ext_record(rr.frame(i)[0], dr.frame(i)[0], 8)
        assert fr["metrics"]["float_ssim"] == float(f"{want[0]:.6f}")
        assert fr["metrics"]["float_ms_ssim"] == float(f"{want[4]:.6f}")
    for k in ("float_ssim", "float_ms_ssim"):
        assert set(log["pooled_metrics"][k]) == {"min", "max", "mean", "harmonic_mean"}
    # every key the old log had keeps its values
    old_log = json.loads(old)
    for a, b in zip(old_log["frames"], log["frames"]):
        assert all(b["metrics"][k] == v for k, v in a["metrics"].items())
    _, only_ms = _score(tmp_path, "ms", SsimFamilyEngine, ms_ssim=True)
    assert '"float_ms_ssim"' in only_ms and '"float_ssim"' not in only_ms


def test_n_subsample_drops_frames_like_the_other_keys(tmp_path):
    res, _ = _score(tmp_path, "sub", SsimFamilyEngine, float_ssim=True, n_subsample=2)
    assert list(res["frame_indices"]) == [0, 2]
    assert not np.isnan(res["metrics"]["float_ssim"]).any() and len(res["metrics"]["float_ssim"]) == 2


def test_analyzer_options_round_trip():
    from pqa2_amd.vmaf_analyzer import VMAFAnalyzer
    a = VMAFAnalyzer()
    assert (a.float_ssim_enabled, a.ms_ssim_enabled) == (False, False)
    a.set_advanced_options("mean", False, False, 1, True, True)          # the reference's positional call still works
    assert (a.float_ssim_enabled, a.ms_ssim_enabled) == (False, False)
    a.set_advanced_options(float_ssim_enabled=True, ms_ssim_enabled=True)
    assert (a.float_ssim_enabled, a.ms_ssim_enabled) == (True, True)

    class Opts:
        def __init__(self, d):
            self.d = d

        def get_setting(self, k):
            return self.d

    a.set_options_from_manager(Opts({"ms_ssim_enabled": True}))
    assert (a.float_ssim_enabled, a.ms_ssim_enabled) == (False, True)
    a.set_options_from_manager(Opts({}))
    assert (a.float_ssim_enabled, a.ms_ssim_enabled) == (False, False)
    assert a.pool_method == "mean"                                       # not tied to pool_method in either direction


def test_analyzer_results_and_child_argv(tmp_path, monkeypatch):
    from pqa2_amd import vmaf_analyzer as V
    rp, dp = (os.path.join(GOLDEN, f"c352x288_8_{s}.y4m") for s in ("ref", "dist"))
    a = V.VMAFAnalyzer()
    a.set_output_directory(str(tmp_path))
    a._engine_factory = SsimFamilyEngine
    res = a.analyze_videos(rp, dp)
    assert res is not None and "float_ssim" not in res and "float_ms_ssim" not in res
    a.set_advanced_options(float_ssim_enabled=True, ms_ssim_enabled=True)
    res = a.analyze_videos(rp, dp)
    pooled = res["raw_results"]["pooled_metrics"]
    assert res["float_ssim"] == pooled["float_ssim"]["mean"] and res["float_ms_ssim"] == pooled["float_ms_ssim"]["mean"]

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
    b.set_advanced_options(ms_ssim_enabled=True)
    b._run_child_job(rp, dp, "vmaf_v0.6.1", "j.json", None, None, 3)
    b.set_advanced_options(float_ssim_enabled=True)
    b._run_child_job(rp, dp, "vmaf_v0.6.1", "j.json", None, None, 3)
    for c in cmds:   # the rendezvous port is picked per run
        c[c.index("--master-port") + 1] = "PORT"
    plain = ["--float-ssim", "--ms-ssim"]
    assert not any(f in cmds[0] for f in plain)
    assert "--ms-ssim" in cmds[1] and "--float-ssim" not in cmds[1]
    assert "--float-ssim" in cmds[2] and "--ms-ssim" not in cmds[2]
    assert [c for c in cmds[1] if c != "--ms-ssim"] == cmds[0]          # argv otherwise unchanged


def test_score_cli_flags_reach_score_files(monkeypatch, tmp_path):
    from pqa2_amd import pipeline, score
    seen = []

    def fake(*a, **kw):
        seen.append(kw)
        raise RuntimeError("stop")

    monkeypatch.setattr(pipeline, "score_files", fake)
    monkeypatch.setattr(score, "_die_with_parent", lambda *a, **k: None)
    score.main(["r.y4m", "d.y4m", "--json", str(tmp_path / "x.json")])
    score.main(["r.y4m", "d.y4m", "--json", str(tmp_path / "x.json"), "--ms-ssim", "--float-ssim"])
    assert "ms_ssim" not in seen[0] and "float_ssim" not in seen[0]
    assert seen[1]["ms_ssim"] is True and seen[1]["float_ssim"] is True


def test_gather_records_width():
    from pqa2_amd import shard
    x = np.arange(3 * 24, dtype=np.float64).reshape(3, 24)
    assert shard.gather_records(x, 3, 1, 0).shape == (3, 24)
    assert np.array_equal(shard.gather_records(x.reshape(-1)[:60].reshape(3, 20), 3, 1, 0, width=20),
                          x.reshape(-1)[:60].reshape(3, 20))


# ---- resources -----------------------------------------------------------------------------------------------------
def test_kernels_use_no_scratch_and_no_spills(tmp_path):
    src = os.path.join(ROOT, "pqa2_amd", "csrc", "ssim_family.hip")
    out = str(tmp_path / "ssf.s")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", src,
                        "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    asm = open(out).read()
    kernels = re.findall(r"\.name:\s+(_Z\S*ssf_\S+|_Z\S*ext_nan\S+)", asm)
    assert len(kernels) >= 9
    assert re.findall(r"\.private_segment_fixed_size:\s+(\d+)", asm) and \
        all(v == "0" for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", asm))
    assert all(v == "0" for v in re.findall(r"\.(?:v|s)gpr_spill_count:\s+(\d+)", asm))
    assert "scratch_store" not in asm and "scratch_load" not in asm and "buffer_store_dword v" not in asm
