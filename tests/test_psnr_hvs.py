"""psnr_hvs without a GPU: the C ABI and its binding (PQA_FEAT_PSNR_HVS, the second extension record), pqa_create's checks,
the host-side hooks (the kernel's own DCT and tables) against the restatement (tests/psnr_hvs_ref.py), closed forms and the
f32 / f64 modes of the restatement, and the host layer (pipeline, JSON, analyzer, child-job argv, CLI, compare tool)
through an oracle-backed engine."""
import ctypes as C
import io
import json
import os
import re

import numpy as np
import pytest

from tests import psnr_hvs_ref as R
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
    assert _enum("PQA_FEAT_PSNR_HVS") == 2048 == N.FEAT_PSNR_HVS
    known = re.search(r"PQA_FEAT_KNOWN\s*=([^;]+?)/\*", src, re.S).group(1)
    assert "PQA_FEAT_PSNR_HVS" in known and N.FEAT_KNOWN & N.FEAT_PSNR_HVS
    assert not N.FEAT_KNOWN & (1 << 7) and N.FEAT_ALL == 31
    slots = ("PQA_EXT2_PSNR_HVS_Y", "PQA_EXT2_PSNR_HVS_CB", "PQA_EXT2_PSNR_HVS_CR", "PQA_EXT2_PSNR_HVS",
             "PQA_EXT2_PSNR_HVS_MSE", "PQA_EXT2_RESERVED", "PQA_EXT2_DOUBLES")
    assert tuple(_enum(s) for s in slots) == (0, 1, 2, 3, 4, 7, 8)
    assert (N.EXT2_PSNR_HVS_Y, N.EXT2_PSNR_HVS_CB, N.EXT2_PSNR_HVS_CR, N.EXT2_PSNR_HVS, N.EXT2_PSNR_HVS_MSE,
            N.EXT2_RESERVED, N.EXT2_DOUBLES) == (0, 1, 2, 3, 4, 7, 8)
    assert _enum("PQA_PSNR_HVS_TABLE_FLOATS") == N.PSNR_HVS_TABLE_FLOATS == R.TABLE_FLOATS
    # what earlier records and tables pin does not move
    assert (_enum("PQA_EXT_DOUBLES"), N.EXT_DOUBLES, _enum("PQA_PROF_KERNELS"), N.PROF_KERNELS) == (24, 24, 17, 17)
    for fn in ("pqa_ext2_doubles", "pqa_collect_ext2", "pqa_debug_psnr_hvs_dct8x8", "pqa_debug_psnr_hvs_tables",
               "pqa_debug_psnr_hvs_plane"):
        assert re.search(r"PQA_API\s+int\s+" + fn + r"\s*\(", src), fn
        assert fn in N.EXPORTS, fn
    lib = N.load()
    assert lib.pqa_ext2_doubles() == 8 and lib.pqa_ext_doubles() == 24
    for fn in N.EXPORTS:
        assert hasattr(lib, fn), fn


def _create(**fields):
    from pqa2_amd import _native as N
    lib = N.load()
    cfg = N.PqaConfig()
    lib.pqa_config_init(C.byref(cfg), 352, 288)
    for k, v in fields.items():
        setattr(cfg, k, v)
    ctx = C.c_void_p()
    return lib.pqa_create(C.byref(cfg), C.byref(ctx)), lib.pqa_last_error(None)


def test_create_rejects_monochrome_and_tiny_chroma_without_a_device():
    from pqa2_amd import _native as N
    rc, msg = _create(features=N.FEAT_VMAF | N.FEAT_PSNR_HVS, n_planes=1)
    assert rc == N.PQA_EINVAL and b"psnr_hvs" in msg
    rc, msg = _create(features=N.FEAT_PSNR_HVS, n_planes=3, width=16, height=16, chroma_hshift=2, chroma_vshift=2)
    assert rc == N.PQA_EINVAL and b"psnr_hvs" in msg
    rc, msg = _create(features=N.FEAT_VMAF | (1 << 7), n_planes=3)
    assert rc == N.PQA_EINVAL


# ---- the host-side hooks against the restatement -----------------------------------------------------------------------
def test_debug_tables_equal_const():
    from pqa2_amd import _native as N
    lib = N.load()
    out = np.zeros(R.TABLE_FLOATS, np.float32)
    assert lib.pqa_debug_psnr_hvs_tables(out.ctypes.data, R.TABLE_FLOATS) == N.PQA_OK
    assert np.array_equal(out, R.tables_f32())
    assert np.array_equal(out[:192].reshape(3, 8, 8), np.stack([R.csf(k, np.float32) for k in range(3)]))
    for k in range(3):   # every table symmetric, as Daala's are
        assert np.array_equal(R.csf(k), R.csf(k).T)
    assert lib.pqa_debug_psnr_hvs_tables(out.ctypes.data, R.TABLE_FLOATS - 1) == N.PQA_EINVAL
    assert lib.pqa_debug_psnr_hvs_tables(None, R.TABLE_FLOATS) == N.PQA_EINVAL


def _blocks(bpc, n=10_000, seed=0):
    rng = np.random.default_rng(seed + bpc)
    top = (1 << bpc) - 1
    x = rng.integers(0, top + 1, (n, 8, 8))
    x[:200] = rng.integers(0, 2, (200, 8, 8)) * top                      # sample extremes: 0 / full scale
    x[200] = top
    x[201] = 0
    x[202] = (np.indices((8, 8)).sum(0) % 2) * top                      # checkerboard: the largest (7, 7) coefficient
    x[203:400] = np.clip(x[203:400, :1, :1] + rng.integers(-3, 4, (197, 8, 8)), 0, top)   # near-flat
    return x.astype(np.int32)


def _hook_dct(x):
    from pqa2_amd import _native as N
    lib = N.load()
    out = np.zeros_like(x)
    assert lib.pqa_debug_psnr_hvs_dct8x8(x.ctypes.data, out.ctypes.data, x.shape[0]) == N.PQA_OK
    return out


@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_debug_dct_equals_the_restatement_bit_for_bit(bpc):
    x = _blocks(bpc)
    assert np.array_equal(_hook_dct(x), R.fdct8x8(x))


@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_dct_is_near_the_orthonormal_dct_and_fits_24_bit_multiplies(bpc):
    """A wrongly remembered lifting constant moves coefficients by far more than the lifting rounding does."""
    import scipy.fft
    x = _blocks(bpc)
    track = [0]
    y = R.fdct8x8(x, track)
    ref = scipy.fft.dctn(x.astype(np.float64), axes=(1, 2), norm="ortho")
    d = np.abs(y - ref).max()
    print(f"\n{bpc}-bit: max |od_bin_fdct8x8 - orthonormal DCT| = {d:.3f}, largest |u * mul + r| = {track[0]} (2^31 = {2**31})")
    assert d <= 6.0
    assert track[0] < 2 ** 30        # int32 lifting products (the kernel's v_mul_i32_i24 keeps the low 32 bits)
    assert np.abs(y).max() < 2 ** 23  # every multiplicand fits the signed 24-bit operand


def test_debug_dct_checks_its_arguments():
    from pqa2_amd import _native as N
    lib = N.load()
    x = np.zeros((1, 8, 8), np.int32)
    assert lib.pqa_debug_psnr_hvs_dct8x8(None, x.ctypes.data, 1) == N.PQA_EINVAL
    assert lib.pqa_debug_psnr_hvs_dct8x8(x.ctypes.data, x.ctypes.data, -1) == N.PQA_EINVAL
    assert lib.pqa_debug_psnr_hvs_dct8x8(x.ctypes.data, x.ctypes.data, 0) == N.PQA_OK


def test_plane_hook_checks_its_arguments_first():
    from pqa2_amd import _native as N
    lib = N.load()
    a = np.zeros((16, 16), np.uint8)
    err = np.zeros(4, np.float32)
    m = C.c_double()
    assert lib.pqa_debug_psnr_hvs_plane(a.ctypes.data, a.ctypes.data, 16, 16, 16, 8, 3, err.ctypes.data, C.byref(m)) == N.PQA_EINVAL
    assert lib.pqa_debug_psnr_hvs_plane(a.ctypes.data, a.ctypes.data, 16, 7, 16, 8, 0, err.ctypes.data, C.byref(m)) == N.PQA_EINVAL
    assert lib.pqa_debug_psnr_hvs_plane(a.ctypes.data, a.ctypes.data, 16, 16, 16, 9, 0, err.ctypes.data, C.byref(m)) == N.PQA_EINVAL
    assert lib.pqa_debug_psnr_hvs_plane(a.ctypes.data, a.ctypes.data, 15, 16, 16, 8, 0, err.ctypes.data, C.byref(m)) == N.PQA_EINVAL
    assert lib.pqa_debug_psnr_hvs_plane(None, a.ctypes.data, 16, 16, 16, 8, 0, err.ctypes.data, C.byref(m)) == N.PQA_EINVAL


# ---- closed forms of the restatement -----------------------------------------------------------------------------------
def test_block_grid():
    assert R.n_blocks(8, 8) == (1, 1)
    assert R.n_blocks(14, 15) == (1, 2)      # x = 0 only (x < 7); y = 0, 7 (y < 8)
    assert R.n_blocks(3840, 2160) == (548, 308)
    assert R.n_blocks(1920, 1080) == (274, 154)
    assert R.n_blocks(7, 100) == (0, 14)
    b = R.blocks_of(np.arange(22 * 15).reshape(15, 22))
    assert b.shape == (2, 3, 8, 8) and b[1, 2, 0, 0] == 7 * 22 + 14 and b[1, 2, 7, 7] == 14 * 22 + 21


def _frame(w, h, bpc, seed, hs=1, vs=1):
    rng = np.random.default_rng(seed)
    top = (1 << bpc) - 1
    dt = np.uint8 if bpc == 8 else np.uint16
    cw, ch = (w + (1 << hs) - 1) >> hs, (h + (1 << vs) - 1) >> vs
    out = []
    for pw, ph in ((w, h), (cw, ch), (cw, ch)):
        yy, xx = np.mgrid[0:ph, 0:pw]
        base = (0.5 + 0.3 * np.sin(xx * 0.07) * np.cos(yy * 0.05)) * top
        r = np.clip(base + rng.normal(0, top * 0.02, (ph, pw)), 0, top)
        d = np.clip(r + rng.normal(0, top * 0.01, (ph, pw)), 0, top)
        out.append((np.rint(r).astype(dt), np.rint(d).astype(dt)))
    return [o[0] for o in out], [o[1] for o in out]


@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_identical_frames_give_inf(bpc):
    r, _ = _frame(64, 48, bpc, 1)
    res = R.psnr_hvs(r, r, bpc)
    assert res["mse"] == (0.0, 0.0, 0.0)
    assert all(np.isposinf(res[k]) for k in ("psnr_hvs_y", "psnr_hvs_cb", "psnr_hvs_cr", "psnr_hvs"))


@pytest.mark.parametrize("v", [0, 1, 100, 255, 1023, 4095])
def test_flat_blocks_have_zero_ac(v):
    c = R.fdct8x8(np.full((1, 8, 8), v))[0]
    assert (c.ravel()[1:] == 0).all() and abs(c[0, 0] - 8 * v) <= 2


@pytest.mark.parametrize("bpc,a,c", [(8, 100, 3), (8, 0, 255), (10, 512, 17), (12, 4000, -1000)])
def test_flat_against_flat_plus_c_is_the_dc_error(bpc, a, c):
    """Flat frames: every AC coefficient is 0, g = 0, so both masks are 0 and only DC differs."""
    w, h = 37, 30
    dt = np.uint8 if bpc == 8 else np.uint16
    ref = [np.full((h, w), a, dt), np.full((h // 2, w // 2), a, dt), np.full((h // 2, w // 2), a, dt)]
    dis = [np.full_like(p, a + c) for p in ref]
    res = R.psnr_hvs(ref, dis, bpc)
    dc = lambda v: int(R.fdct8x8(np.full((1, 8, 8), v))[0, 0, 0])
    for k, key in enumerate(("psnr_hvs_y", "psnr_hvs_cb", "psnr_hvs_cr")):
        want = (abs(dc(a) - dc(a + c)) * R.csf(k)[0, 0]) ** 2 / 64.0
        assert res["mse"][k] == pytest.approx(want, rel=1e-12)
        assert res[key] == pytest.approx(10 * np.log10(((1 << bpc) - 1) ** 2 / want), abs=1e-9)
    comb = 0.8 * res["mse"][0] + 0.1 * (res["mse"][1] + res["mse"][2])
    assert res["psnr_hvs"] == pytest.approx(10 * np.log10(((1 << bpc) - 1) ** 2 / comb), abs=1e-9)


def test_masking_lowers_the_error_of_textured_blocks():
    """The same distortion costs less on a textured block than on a flat one (the contrast mask at work)."""
    rng = np.random.default_rng(5)
    flat = np.full((8, 8), 128)
    tex = np.clip(128 + rng.integers(-60, 61, (8, 8)), 0, 255)
    noise = rng.integers(-4, 5, (8, 8))
    e_flat = R.block_errors(flat, np.clip(flat + noise, 0, 255), 0)[0, 0]
    e_tex = R.block_errors(tex, np.clip(tex + noise, 0, 255), 0)[0, 0]
    assert 0 <= e_tex < e_flat


@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_f32_mode_agrees_with_f64_and_reports_the_drift(bpc):
    r, d = _frame(352, 288, bpc, 7)
    a, b = R.psnr_hvs(r, d, bpc), R.psnr_hvs(r, d, bpc, "f32")
    rel = [abs(x - y) / y for x, y in zip(b["mse"], a["mse"])]
    print(f"\n352x288 {bpc}-bit: libvmaf-style f32 mse drift (relative) Y {rel[0]:.2e} Cb {rel[1]:.2e} Cr {rel[2]:.2e}; "
          f"psnr_hvs |d| {abs(a['psnr_hvs'] - b['psnr_hvs']):.2e} dB")
    assert max(rel) < 1e-4
    assert abs(a["psnr_hvs"] - b["psnr_hvs"]) < 5e-4
    # per block the two modes differ by f32 rounding only (the running sum is what drifts)
    e64, e32 = R.block_errors(r[0], d[0], 0), R.block_errors(r[0], d[0], 0, "f32")
    assert np.allclose(e32, e64, rtol=1e-4, atol=1e-3)


# ---- host layer through an oracle-backed engine ----------------------------------------------------------------------
class PsnrHvsEngine(OracleEngine):
    """OracleEngine plus the second extension record's psnr_hvs slots (the restatement stands in for the kernel)."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.frames = {}

    def submit(self, index, ref_planes, dis_planes):
        super().submit(index, ref_planes, dis_planes)
        self.frames[index] = ([np.array(p) for p in ref_planes], [np.array(p) for p in dis_planes])

    def collect_blocks(self, first, count, blocks):
        got = self.collect_ext2(first, count)
        return got[0], {i: got[1 + i] for i in blocks}

    def collect_ext2(self, first, count):
        from pqa2_amd import _native as N
        ext = np.full((count, N.EXT_DOUBLES), np.nan)
        ext2 = np.full((count, N.EXT2_DOUBLES), np.nan)
        for i in range(count):
            if (first + i) % self.k == 0 and self.features & N.FEAT_PSNR_HVS:
                r, d = self.frames[first + i]
                res = R.psnr_hvs(r, d, self.bpc)
                ext2[i, :4] = [res[k] for k in ("psnr_hvs_y", "psnr_hvs_cb", "psnr_hvs_cr", "psnr_hvs")]
                ext2[i, 4:7] = res["mse"]
        return self.collect(first, count), ext, ext2


KEYS = ("psnr_hvs_y", "psnr_hvs_cb", "psnr_hvs_cr", "psnr_hvs")


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


def test_json_gains_psnr_hvs_keys_only_when_enabled(tmp_path):
    from pqa2_amd import yuvio
    _, old = _score(tmp_path, "old", OracleEngine)
    _, new_default = _score(tmp_path, "new", PsnrHvsEngine)
    assert new_default == old and "psnr_hvs" not in old
    _, text = _score(tmp_path, "on", PsnrHvsEngine, psnr_hvs=True)
    log = json.loads(text)
    rr, dr = (yuvio.open_video(p) for p in _clip_paths())
    for i, fr in enumerate(log["frames"]):
        want = R.psnr_hvs(rr.frame(i), dr.frame(i), 8)
        for k in KEYS:
            assert fr["metrics"][k] == float(f"{want[k]:.6f}"), (i, k)
    for k in KEYS:
        assert set(log["pooled_metrics"][k]) == {"min", "max", "mean", "harmonic_mean"}
    old_log = json.loads(old)
    for a, b in zip(old_log["frames"], log["frames"]):
        assert all(b["metrics"][k] == v for k, v in a["metrics"].items())


def test_monochrome_clip_is_an_error(tmp_path):
    from pqa2_amd import synth, yuvio
    refs, diss = synth.make_clip(64, 48, 2, 8, chroma=False)
    info = synth.clip_info(64, 48, 8, chroma=False)
    rp, dp = str(tmp_path / "r.y4m"), str(tmp_path / "d.y4m")
    yuvio.write_y4m(rp, refs, info)
    yuvio.write_y4m(dp, diss, info)
    with pytest.raises(ValueError, match="psnr_hvs"):
        _score(tmp_path, "mono", PsnrHvsEngine, (rp, dp), psnr_hvs=True)


def test_n_subsample_drops_frames_like_the_other_keys(tmp_path):
    res, _ = _score(tmp_path, "sub", PsnrHvsEngine, psnr_hvs=True, n_subsample=2)
    assert list(res["frame_indices"]) == [0, 2]
    for k in KEYS:
        assert len(res["metrics"][k]) == 2 and np.isfinite(res["metrics"][k]).all()


def test_psnr_hvs_without_psnr_or_ssim_still_uses_three_planes(tmp_path):
    res, _ = _score(tmp_path, "bare", PsnrHvsEngine, psnr_hvs=True, psnr=False, ssim=False)
    assert "psnr_y" not in res["metrics"] and np.isfinite(res["metrics"]["psnr_hvs_cb"]).all()


def test_analyzer_options_round_trip():
    from pqa2_amd.vmaf_analyzer import VMAFAnalyzer
    a = VMAFAnalyzer()
    assert a.psnr_hvs_enabled is False
    a.set_advanced_options("mean", False, False, 1, True, True)
    assert a.psnr_hvs_enabled is False and a._ssim_family_kwargs() == {}
    a.set_advanced_options(psnr_hvs_enabled=True)
    assert a._ssim_family_kwargs() == {"psnr_hvs": True}

    class Opts:
        def __init__(self, d):
            self.d = d

        def get_setting(self, k):
            return self.d

    a.set_options_from_manager(Opts({"psnr_hvs_enabled": True}))
    assert a.psnr_hvs_enabled is True
    a.set_options_from_manager(Opts({}))
    assert a.psnr_hvs_enabled is False


def test_analyzer_results_and_child_argv(tmp_path, monkeypatch):
    from pqa2_amd import vmaf_analyzer as V
    rp, dp = _clip_paths()
    a = V.VMAFAnalyzer()
    a.set_output_directory(str(tmp_path))
    a._engine_factory = PsnrHvsEngine
    res = a.analyze_videos(rp, dp)
    assert res is not None and "psnr_hvs" not in res
    a.set_advanced_options(psnr_hvs_enabled=True)
    res = a.analyze_videos(rp, dp)
    pooled = res["raw_results"]["pooled_metrics"]
    for k in KEYS:
        assert res[k] == pooled[k]["mean"]

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
    b.set_advanced_options(psnr_hvs_enabled=True)
    b._run_child_job(rp, dp, "vmaf_v0.6.1", "j.json", None, None, 3)
    for c in cmds:
        c[c.index("--master-port") + 1] = "PORT"
    assert "--psnr-hvs" not in cmds[0] and "--psnr-hvs" in cmds[1]
    assert [c for c in cmds[1] if c != "--psnr-hvs"] == cmds[0]


def test_score_cli_flag_reaches_score_files(monkeypatch, tmp_path):
    from pqa2_amd import pipeline, score
    seen = []

    def fake(*a, **kw):
        seen.append(kw)
        raise RuntimeError("stop")

    monkeypatch.setattr(pipeline, "score_files", fake)
    monkeypatch.setattr(score, "_die_with_parent", lambda *a, **k: None)
    score.main(["r.y4m", "d.y4m", "--json", str(tmp_path / "x.json")])
    score.main(["r.y4m", "d.y4m", "--json", str(tmp_path / "x.json"), "--psnr-hvs"])
    assert "psnr_hvs" not in seen[0] and seen[1]["psnr_hvs"] is True


def test_compare_tool_knows_the_psnr_hvs_keys():
    import importlib.util
    spec = importlib.util.spec_from_file_location("cmp", os.path.join(ROOT, "tools", "compare_libvmaf_log.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.PSNR_HVS_KEYS == KEYS
    assert len(mod.SSIM_IMPLICATES["psnr_hvs"]) == 6
    assert all("VERIFY" in line for line in mod.SSIM_IMPLICATES["psnr_hvs"])
    cols = mod.psnr_hvs_columns(*_clip_paths(), False, 2)
    (tag, c), = cols.items()
    assert "psnr_hvs_ref" in tag and all(np.isfinite(c[k]).all() and len(c[k]) == 2 for k in KEYS)
