"""ciede2000 without a GPU: the f64 restatement against Sharma et al.'s published pairs and its invariants, the C ABI and
its binding, the host layer (pipeline, JSON, analyzer, child-job argv, CLI) through an oracle-backed engine, and the
kernel's register budget."""
import ctypes as C
import io
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import ciede_ref as R
from tests.fake_engine import OracleEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pqa_vmaf.h")
GOLDEN = os.path.join(ROOT, "tests", "golden")
CLIPS = os.path.join(GOLDEN, "clips")


def sharma_pairs():
    """[27, 7]: L1, a1, b1, L2, a2, b2, published dE00 (tests/golden/ciede2000_sharma.csv)."""
    return np.loadtxt(os.path.join(GOLDEN, "ciede2000_sharma.csv"), delimiter=",", comments="#")


# ---- the restatement ---------------------------------------------------------------------------------------------
def test_restatement_matches_the_sharma_pairs():
    d = sharma_pairs()
    assert d.shape == (27, 7)
    got = R.de00(*d[:, :6].T)
    assert np.abs(got - d[:, 6]).max() <= 1e-4, np.abs(got - d[:, 6])


def test_f32_restatement_near_the_sharma_pairs():
    """The f32 variant is the same definition: away from the 180-degree hue jump it stays with the published values."""
    d = sharma_pairs()
    far = R.hue_delta_from_180(*d[:, :6].T) > 1e-3
    got = R.de00(*d[:, :6].T, dtype=np.float32)
    assert np.abs(got[far] - d[far, 6]).max() <= 1e-4


def test_symmetric_and_zero_on_identical_colours():
    rng = np.random.default_rng(7)
    p = np.stack([rng.uniform(0, 100, 5000), rng.uniform(-120, 120, 5000), rng.uniform(-120, 120, 5000)])
    q = np.stack([rng.uniform(0, 100, 5000), rng.uniform(-120, 120, 5000), rng.uniform(-120, 120, 5000)])
    far = R.hue_delta_from_180(*p, *q) > 1e-6
    assert np.allclose(R.de00(*p, *q)[far], R.de00(*q, *p)[far], rtol=1e-12, atol=1e-12)
    assert (R.de00(*p, *p) == 0).all()
    assert R.de00(50, 0, 0, 50, 0, 0) == 0


def _frame(w, h, bpc, hs, vs, seed, const=None):
    rng = np.random.default_rng(seed)
    top = (1 << bpc) - 1
    dt = np.uint8 if bpc == 8 else np.uint16
    cw, ch = (w + (1 << hs) - 1) >> hs, (h + (1 << vs) - 1) >> vs
    if const is not None:
        return [np.full((h, w), const[0], dt), np.full((ch, cw), const[1], dt), np.full((ch, cw), const[2], dt)]
    return [rng.integers(0, top + 1, (h, w)).astype(dt), rng.integers(0, top + 1, (ch, cw)).astype(dt),
            rng.integers(0, top + 1, (ch, cw)).astype(dt)]


@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_constant_frames_give_the_single_pixel_value(bpc):
    s = 1 << (bpc - 8)
    a, b = (100 * s, 90 * s, 160 * s), (120 * s, 140 * s, 100 * s)
    fr, fd = _frame(33, 17, bpc, 1, 1, 0, a), _frame(33, 17, bpc, 1, 1, 0, b)
    score, mean = R.frame_slots(fr, fd, bpc)
    one = R.de00(*R.yuv_to_lab(*[np.full((1, 1), v) for v in a], bpc, 0, 0),
                 *R.yuv_to_lab(*[np.full((1, 1), v) for v in b], bpc, 0, 0))
    assert abs(mean - float(one[0, 0])) <= 1e-12 * float(one[0, 0])
    assert score == 45 - 20 * math.log10(mean)
    assert R.frame_slots(fr, fr, bpc) == (math.inf, 0.0)


@pytest.mark.parametrize("hs,vs", [(1, 1), (1, 0), (2, 2)])
def test_subsampled_chroma_equals_444_of_replicated_chroma(hs, vs):
    w, h, bpc = 37, 23, 10
    fr, fd = _frame(w, h, bpc, hs, vs, 1), _frame(w, h, bpc, hs, vs, 2)
    up = lambda f: [f[0], R.upsample(f[1], w, h, hs, vs), R.upsample(f[2], w, h, hs, vs)]
    assert np.array_equal(R.frame_de(fr, fd, bpc, hs, vs), R.frame_de(up(fr), up(fd), bpc, 0, 0))


@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_sample_extremes_are_finite(bpc):
    top = (1 << bpc) - 1
    vals = [0, top]
    combos = [(y, u, v) for y in vals for u in vals for v in vals]
    for a in combos:
        for b in combos:
            for dt in (np.float64, np.float32):
                fa, fb = _frame(16, 16, bpc, 1, 1, 0, a), _frame(16, 16, bpc, 1, 1, 0, b)
                d = R.frame_de(fa, fb, bpc, dtype=dt)
                assert np.isfinite(d).all(), (a, b, dt)
    assert all(np.isfinite(v).all() for v in R.yuv_to_lab(np.array([[0, top]]), np.array([[top]]), np.array([[0]]), bpc))


def test_f32_evaluation_distance_from_f64():
    """How far f32 evaluation of the same expressions sits from f64 on random frames (DESIGN.md section 1 quotes it)."""
    worst = 0.0
    for bpc in (8, 10, 12):
        fr, fd = _frame(96, 64, bpc, 1, 1, bpc), _frame(96, 64, bpc, 1, 1, bpc + 100)
        m64 = R.frame_slots(fr, fd, bpc)[1]
        m32 = R.frame_slots(fr, fd, bpc, dtype=np.float32)[1]
        worst = max(worst, abs(m32 - m64) / m64)
    print(f"\nf32 restatement vs f64: worst relative mean-dE distance {worst:.2e}")
    assert worst < 2e-5


# ---- C ABI and binding --------------------------------------------------------------------------------------------
def _enum(name):
    src = open(HEADER).read()
    m = re.search(rf"\b{name}\s*=\s*([^,\n/}}]+)", src)
    assert m, name
    return eval(m.group(1).replace("1u", "1"))


def test_header_binding_and_library_agree():
    from pqa2_amd import _native as N
    src = open(HEADER).read()
    assert _enum("PQA_FEAT_CIEDE") == 256 == N.FEAT_CIEDE
    assert "PQA_FEAT_CIEDE" in re.search(r"PQA_FEAT_KNOWN\s*=([^\n]+)", src).group(1)
    assert N.FEAT_KNOWN & N.FEAT_CIEDE and not N.FEAT_KNOWN & (1 << 7) and N.FEAT_ALL == 31
    assert (_enum("PQA_EXT_CIEDE2000"), _enum("PQA_EXT_CIEDE_MEAN_DE"), _enum("PQA_EXT_RESERVED")) == (20, 21, 20)
    assert (N.EXT_CIEDE2000, N.EXT_CIEDE_MEAN_DE, N.EXT_DOUBLES) == (20, 21, 24)
    assert re.search(r"PQA_API\s+int\s+pqa_debug_ciede2000\s*\(", src)
    assert "pqa_debug_ciede2000" in N.EXPORTS
    lib = N.load()
    assert hasattr(lib, "pqa_debug_ciede2000")
    assert lib.pqa_profile_kernel_name(4) == b"ciede2000"
    assert lib.pqa_profile_kernel_name(5) == b"reserved5" and lib.pqa_profile_kernel_name(6) == b"reserved6"


def test_create_rejects_ciede_without_chroma_planes_without_a_device():
    from pqa2_amd import _native as N
    lib = N.load()
    cfg = N.PqaConfig()
    lib.pqa_config_init(C.byref(cfg), 352, 288)
    cfg.features = N.FEAT_VMAF | N.FEAT_CIEDE
    cfg.n_planes = 1
    ctx = C.c_void_p()
    assert lib.pqa_create(C.byref(cfg), C.byref(ctx)) == N.PQA_EINVAL
    assert b"ciede2000" in lib.pqa_last_error(None)


# ---- host layer through an oracle-backed engine --------------------------------------------------------------------
class CiedeEngine(OracleEngine):
    """OracleEngine plus the extension record's ciede slots (the restatement stands in for the kernel)."""

    def __init__(self, *a, chroma_shift=(1, 1), **kw):
        super().__init__(*a, chroma_shift=chroma_shift, **kw)
        self.shift = chroma_shift
        self.frames = {}

    def submit(self, index, ref_planes, dis_planes):
        super().submit(index, ref_planes, dis_planes)
        self.frames[index] = ([np.array(p) for p in ref_planes], [np.array(p) for p in dis_planes])

    def collect_ext(self, first, count):
        from pqa2_amd import _native as N
        ext = np.full((count, N.EXT_DOUBLES), np.nan)
        for i in range(count):
            if (first + i) % self.k == 0 and self.features & N.FEAT_CIEDE:
                r, d = self.frames[first + i]
                assert len(r) == 3 and len(d) == 3
                ext[i, N.EXT_CIEDE2000], ext[i, N.EXT_CIEDE_MEAN_DE] = R.frame_slots(r, d, self.bpc, *self.shift)
        return self.collect(first, count), ext


def _clip_paths():
    return tuple(os.path.join(CLIPS, f"c352x288_8_{s}.y4m") for s in ("ref", "dist"))


def _score(tmp_path, tag, factory, **kw):
    from pqa2_amd import report
    from pqa2_amd.pipeline import score_files
    rp, dp = _clip_paths()
    res = score_files(rp, dp, "vmaf_v0.6.1", engine_factory=factory, **kw)
    log = report.build_vmaf_log(res["metrics"], 0.0, res["frame_indices"], {"model": res["model_name"]})
    path = str(tmp_path / f"{tag}.json")
    report.write_vmaf_json(path, log)
    return res, open(path).read()


def test_json_gains_ciede2000_only_when_enabled(tmp_path):
    from pqa2_amd import yuvio
    _, old = _score(tmp_path, "old", OracleEngine)
    _, new_default = _score(tmp_path, "new", CiedeEngine)
    assert new_default == old and "ciede2000" not in old
    res, text = _score(tmp_path, "ciede", CiedeEngine, ciede=True)
    log = json.loads(text)
    rr, dr = (yuvio.open_video(p) for p in _clip_paths())
    for i, fr in enumerate(log["frames"]):
        want = R.frame_slots(rr.frame(i), dr.frame(i), 8)[0]
        assert fr["metrics"]["ciede2000"] == float(f"{want:.6f}")
    assert set(log["pooled_metrics"]["ciede2000"]) == {"min", "max", "mean", "harmonic_mean"}
    old_log = json.loads(old)
    for a, b in zip(old_log["frames"], log["frames"]):
        assert all(b["metrics"][k] == v for k, v in a["metrics"].items())
    # without psnr / ssim the chroma planes are still read (n_planes 3)
    res, _ = _score(tmp_path, "only", CiedeEngine, ciede=True, psnr=False, ssim=False)
    assert "ciede2000" in res["metrics"] and "psnr_y" not in res["metrics"]


def test_identical_clips_give_inf_written_as_psnr_writes_it(tmp_path):
    from pqa2_amd import report
    from pqa2_amd.pipeline import score_files
    rp, _ = _clip_paths()
    res = score_files(rp, rp, "vmaf_v0.6.1", engine_factory=CiedeEngine, ciede=True)
    assert np.isinf(res["metrics"]["ciede2000"]).all()
    log = report.build_vmaf_log(res["metrics"], 0.0, res["frame_indices"], {"model": res["model_name"]})
    path = str(tmp_path / "same.json")
    report.write_vmaf_json(path, log)
    text = open(path).read()
    assert re.search(r'"ciede2000": inf\b', text) and re.search(r'"psnr_y": \S+', text)


def test_n_subsample_drops_frames_like_the_other_keys(tmp_path):
    res, _ = _score(tmp_path, "sub", CiedeEngine, ciede=True, n_subsample=2)
    assert list(res["frame_indices"]) == [0, 2]
    assert not np.isnan(res["metrics"]["ciede2000"]).any() and len(res["metrics"]["ciede2000"]) == 2


def test_mono_clip_with_ciede_is_an_error(tmp_path):
    from pqa2_amd import synth, yuvio
    from pqa2_amd.pipeline import score_files
    refs, diss = synth.make_clip(64, 48, 2, 8, chroma=False)
    info = synth.clip_info(64, 48, 8, chroma=False)
    rp, dp = str(tmp_path / "r.y4m"), str(tmp_path / "d.y4m")
    yuvio.write_y4m(rp, refs, info)
    yuvio.write_y4m(dp, diss, info)
    with pytest.raises(ValueError, match="ciede2000"):
        score_files(rp, dp, "vmaf_v0.6.1", engine_factory=CiedeEngine, ciede=True)
    score_files(rp, dp, "vmaf_v0.6.1", engine_factory=CiedeEngine)    # the same clip without ciede still scores


def test_analyzer_options_round_trip():
    from pqa2_amd.vmaf_analyzer import VMAFAnalyzer
    a = VMAFAnalyzer()
    assert a.ciede_enabled is False
    a.set_advanced_options("mean", False, False, 1, True, True)          # the reference's positional call still works
    assert a.ciede_enabled is False
    a.set_advanced_options(ciede_enabled=True)
    assert a.ciede_enabled is True and a._ssim_family_kwargs() == {"ciede": True}

    class Opts:
        def __init__(self, d):
            self.d = d

        def get_setting(self, k):
            return self.d

    a.set_options_from_manager(Opts({"ciede_enabled": True}))
    assert a.ciede_enabled is True
    a.set_options_from_manager(Opts({}))
    assert a.ciede_enabled is False and a._ssim_family_kwargs() == {}


def test_analyzer_results_and_child_argv(tmp_path, monkeypatch):
    from pqa2_amd import vmaf_analyzer as V
    rp, dp = _clip_paths()
    a = V.VMAFAnalyzer()
    a.set_output_directory(str(tmp_path))
    a._engine_factory = CiedeEngine
    res = a.analyze_videos(rp, dp)
    assert res is not None and "ciede2000" not in res
    a.set_advanced_options(ciede_enabled=True)
    res = a.analyze_videos(rp, dp)
    assert res["ciede2000"] == res["raw_results"]["pooled_metrics"]["ciede2000"]["mean"]

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
    b.set_advanced_options(ciede_enabled=True)
    b._run_child_job(rp, dp, "vmaf_v0.6.1", "j.json", None, None, 3)
    for c in cmds:   # the rendezvous port is picked per run
        c[c.index("--master-port") + 1] = "PORT"
    assert "--ciede" not in cmds[0] and "--ciede" in cmds[1]
    assert [c for c in cmds[1] if c != "--ciede"] == cmds[0]


def test_score_cli_flag_reaches_score_files(monkeypatch, tmp_path):
    from pqa2_amd import pipeline, score
    seen = []

    def fake(*a, **kw):
        seen.append(kw)
        raise RuntimeError("stop")

    monkeypatch.setattr(pipeline, "score_files", fake)
    monkeypatch.setattr(score, "_die_with_parent", lambda *a, **k: None)
    score.main(["r.y4m", "d.y4m", "--json", str(tmp_path / "x.json")])
    score.main(["r.y4m", "d.y4m", "--json", str(tmp_path / "x.json"), "--ciede"])
    assert "ciede" not in seen[0] and seen[1]["ciede"] is True


# ---- resources -----------------------------------------------------------------------------------------------------
def test_kernel_uses_no_scratch_and_no_spills(tmp_path):
    src = os.path.join(ROOT, "pqa2_amd", "csrc", "ciede.hip")
    out = str(tmp_path / "ciede.s")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", src,
                        "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    asm = open(out).read()
    kernels = re.findall(r"\.name:\s+(_Z\S*ciede_\S+)", asm)
    assert len(kernels) >= 20
    sizes = re.findall(r"\.private_segment_fixed_size:\s+(\d+)", asm)
    assert sizes and all(v == "0" for v in sizes)
    assert all(v == "0" for v in re.findall(r"\.(?:v|s)gpr_spill_count:\s+(\d+)", asm))
    assert "scratch_store" not in asm and "scratch_load" not in asm and "buffer_store_dword v" not in asm
    # the per-pixel kernels have no f64 arithmetic (the tile sum is widened once, after the wave reduction)
    for name in re.findall(r"^(_Z\S*ciede_kernel\S*):", asm, re.M):
        body = asm[asm.index(name + ":"):]
        body = body[:body.index("s_endpgm")]
        f64 = [l for l in body.split("\n") if re.search(r"\bv_(?!add_f64|cvt_f64_f32)\w+_f64\b", l)]
        assert not f64, (name, f64[:3])
