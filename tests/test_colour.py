"""Colour-matrix alignment on the host: the named maps, the solver (align.best_colour, align.colour_correction) on the numpy
restatement of the moments (tests/colour_ref.py), the library's context-free argument rules, the command-line flags, the report
line and score_files(colour_align=) through tests/fake_engine.py.  The kernels themselves: tests/test_gpu_colour.py."""
import ctypes as C
import json
from fractions import Fraction

import numpy as np
import pytest

from tests import colour_ref as R

NAMES = [f"{x}_to_{y}" for x in ("bt601", "bt709", "bt2020") for y in ("bt601", "bt709", "bt2020") if x != y]


def _measure(ref, dis, bd, hs=1, vs=1, full=False, **kw):
    from pqa2_amd.align import best_colour
    mask = {k: kw.pop(k) for k in ("lo", "hi") if k in kw}
    h, w = ref[0][0].shape
    ch, cw = R.chroma_shape(w, h, hs, vs)
    return best_colour(R.colour_moments(ref, dis, bd, hs, vs, **mask), bd, hs, vs, full_range=full,
                       total_samples=len(ref) * ch * cw, **kw)


# ---- named maps ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("full", [False, True])
def test_named_maps_are_exact(bd, full):
    from pqa2_amd.align import COLOUR_MAPS, named_colour_map
    assert list(COLOUR_MAPS) == ["identity"] + NAMES
    ident = [[Fraction(int(i == j)) for j in range(3)] for i in range(3)]
    assert named_colour_map("identity", bd, full) == (ident, [Fraction(0)] * 3)
    f = 1 << (bd - 8)
    for name in NAMES:
        x, y = name.split("_to_")
        A, b = named_colour_map(name, bd, full)
        B, c = named_colour_map(f"{y}_to_{x}", bd, full)
        assert [[sum(A[i][k] * B[k][j] for k in range(3)) for j in range(3)] for i in range(3)] == ident     # exactly, in Fractions
        assert [b[i] + sum(A[i][j] * c[j] for j in range(3)) for i in range(3)] == [0, 0, 0]
        for luma in (0, 16 * f, 100 * f, (1 << bd) - 1):      # grey keeps its luma and stays grey
            grey = [Fraction(luma), Fraction(128 * f), Fraction(128 * f)]
            assert [sum(A[i][j] * grey[j] for j in range(3)) + b[i] for i in range(3)] == grey
    A, b = named_colour_map("bt709_to_bt601", bd, False)
    black = [16 * f, 128 * f, 128 * f]
    assert [sum(A[i][j] * black[j] for j in range(3)) + b[i] for i in range(3)] == black
    assert float(A[0][1]) == pytest.approx(0.0993117, abs=1e-6) and float(A[0][2]) == pytest.approx(0.1916995, abs=1e-6)   # the published 709 -> 601 luma row
    with pytest.raises(ValueError):
        named_colour_map("bt709_to_bt709", bd, full)


# ---- recovery --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(64, 48), (131, 77)])
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("full", [False, True])
def test_recovers_bt709_to_bt601(w, h, bd, full):
    """a seeded 4-frame 4:2:0 clip through bt709_to_bt601, clean and with sigma = 2 noise (in 8-bit units) before rounding; the
    conditions are the solver's own defaults, 2.0 and 1.25"""
    from pqa2_amd.align import named_colour_map
    ref = R.clip(7, w, h, bd, 1, 1, 4, full)
    A, b = named_colour_map("bt709_to_bt601", bd, full)
    for sigma in (None, 2.0 * (1 << (bd - 8))):
        rng = np.random.default_rng(1)
        dis = [R.convert(f, A, b, bd, 1, 1, noise=None if sigma is None else (sigma, rng)) for f in ref]
        res = _measure(ref, dis, bd, full=full)
        assert (res["kind"], res["mismatch"], res["cross_plane"], res["degenerate"], res["frames"]) == ("bt709_to_bt601", True, True, False, 4)
        chosen = res["named"]["bt709_to_bt601"]
        assert chosen <= 1.25 * res["mse_matrix"] and res["mse_identity"] > 2.0 * chosen
        assert res["mse_diagonal"] > 1.25 * res["mse_matrix"]
        for name, mse in res["named"].items():
            if name != "bt709_to_bt601":
                assert mse > 2.0 * chosen, name
        if sigma is None:      # rounding alone: every plane sits on the 1/12 floor, and every wrong name is off on every plane
            got = res["planes"]["named"]["bt709_to_bt601"]
            assert all(0.06 < v < 0.11 for v in got)
            for name, triple in res["planes"]["named"].items():
                if name != "bt709_to_bt601":
                    assert all(t > 2.0 * g for t, g in zip(triple, got)), name
        assert 0.0 <= res["samples_masked_share"] < 0.02 and res["samples"] > 0
        assert np.allclose(res["matrix"], [[float(v) for v in r] for r in A], atol=0.02)


# ---- other map shapes ------------------------------------------------------------------------------------------------------
def test_identical_pair_is_identity():
    ref = R.clip(3, 64, 48, 8, 1, 1, 2)
    res = _measure(ref, ref, 8)
    assert (res["kind"], res["mismatch"], res["cross_plane"], res["degenerate"]) == ("identity", False, False, False)
    assert res["mse_identity"] == 0.0 and res["mse_matrix"] == 0.0
    assert res["matrix"] == [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]] and res["offset"] == [0.0, 0.0, 0.0]


def test_range_change_is_not_cross_plane():
    """limited_to_full on all three planes: a mismatch, but each plane alone explains it -- level alignment's job"""
    from pqa2_amd.align import colour_correction, named_level_map
    ref = R.clip(4, 64, 48, 8, 1, 1, 3)
    maps = [named_level_map("limited_to_full", 8, chroma=p > 0) for p in range(3)]
    A = [[maps[i][0] if i == j else Fraction(0) for j in range(3)] for i in range(3)]
    dis = [R.convert(f, A, [m[1] for m in maps], 8, 1, 1) for f in ref]
    res = _measure(ref, dis, 8)
    assert res["mismatch"] is True and res["cross_plane"] is False and res["kind"] == "matrix"
    assert res["mse_diagonal"] <= 1.25 * res["mse_matrix"]
    assert colour_correction(res, 8) is not None     # the inverse exists; the pipeline leaves it to level_align all the same


def test_hand_made_matrix():
    """exact case first: dyadic matrix entries on reference samples that are multiples of 4 and constant under every chroma
    sample give integer captured samples, and the fit returns the matrix exactly.  Then a general matrix with rounding: the
    fitted entries lie within six standard deviations of uniform rounding noise, sigma^2 = 1/12, propagated through the normal
    equations of the reference data itself: cov = sigma^2 (X^T X)^-1, X = [1, Yr, Ur, Vr] per chroma sample"""
    rng = np.random.default_rng(11)
    A = [[Fraction(3, 4), Fraction(1, 4), Fraction(-1, 4)], [Fraction(1, 4), Fraction(5, 4), Fraction(0)], [Fraction(-1, 4), Fraction(1, 4), Fraction(1)]]
    b = [Fraction(20), Fraction(-30), Fraction(9)]
    ref = []
    for _ in range(2):
        yc = 4 * rng.integers(12, 40, (24, 32))
        ref.append([np.kron(yc, np.ones((2, 2), np.int64)).astype(np.uint8), (4 * rng.integers(20, 44, (24, 32))).astype(np.uint8),
                    (4 * rng.integers(20, 44, (24, 32))).astype(np.uint8)])
    dis = [R.convert(f, A, b, 8, 1, 1) for f in ref]
    res = _measure(ref, dis, 8, lo=0, hi=255)
    assert res["kind"] == "matrix" and res["mismatch"] and res["cross_plane"] and res["mse_matrix"] == 0.0
    assert res["matrix"] == [[float(v) for v in r] for r in A] and res["offset"] == [float(v) for v in b]
    assert res["map_matrix"] == res["matrix"] and res["samples_masked_share"] == 0.0

    A2 = [[0.93, 0.07, -0.05], [0.03, 1.08, 0.06], [-0.04, 0.05, 0.9]]
    b2 = [6.5, -9.25, 14.0]
    ref = R.clip(12, 64, 48, 8, 1, 1, 4)
    dis = [R.convert(f, A2, b2, 8, 1, 1) for f in ref]
    res = _measure(ref, dis, 8)
    assert res["kind"] == "matrix" and res["mismatch"] and res["cross_plane"]
    X = np.concatenate([np.stack([np.ones(f[1].size), R.block_sum(f[0], 1, 1).ravel() / 4.0, f[1].ravel().astype(float),
                                  f[2].ravel().astype(float)], axis=1) for f in ref])
    tol = 6.0 * np.sqrt(np.diag(np.linalg.inv(X.T @ X)) / 12.0)      # [offset, Y, U, V]
    for k in range(3):
        assert abs(res["offset"][k] - b2[k]) <= tol[0], k
        assert all(abs(res["matrix"][k][j] - A2[k][j]) <= tol[1 + j] for j in range(3)), k
    assert all(0.0 < v < 0.12 for v in res["planes"]["mse_matrix"])


def test_flat_clip_is_degenerate():
    from pqa2_amd.align import colour_correction
    flat = [[np.full((48, 64), 90, np.uint8), np.full((24, 32), 120, np.uint8), np.full((24, 32), 140, np.uint8)]] * 2
    res = _measure(flat, flat, 8)
    assert res["degenerate"] and (res["kind"], res["mismatch"], res["cross_plane"]) == ("identity", False, False)
    mono = R.clip(5, 64, 48, 8, 1, 1, 2)
    mono = [[f[0], np.full_like(f[1], 128), np.full_like(f[2], 128)] for f in mono]      # monochrome-looking: no chroma variation
    assert _measure(mono, mono, 8)["degenerate"]
    everything_masked = [[np.zeros_like(p) for p in f] for f in mono]
    res = _measure(mono, everything_masked, 8)
    assert res["degenerate"] and res["samples"] == 0 and res["samples_masked_share"] == 1.0
    assert colour_correction(res, 8) is not None      # the identity
    with pytest.raises(ValueError):
        from pqa2_amd.align import best_colour
        best_colour(np.zeros((1, 27), np.uint64), 8, 1, 1)


def test_mask_keeps_the_fit_on_the_true_matrix():
    """a gain of 1.9 about mid-range drives a good share of the samples into both clamps: with the default mask the fit stays
    on the matrix, with lo = 0, hi = top it visibly does not"""
    A = [[1.9, 0.1, 0.19], [0.0, 1.9, -0.11], [0.0, -0.07, 1.9]]
    centre = [126.0, 128.0, 128.0]
    b = [centre[i] - sum(A[i][j] * centre[j] for j in range(3)) for i in range(3)]
    ref = R.clip(9, 64, 48, 8, 1, 1, 4, margin=0.02, chroma_margin=0.02)
    dis = [R.convert(f, A, b, 8, 1, 1) for f in ref]
    masked, keep_all = _measure(ref, dis, 8), _measure(ref, dis, 8, lo=0, hi=255)
    assert 0.02 < masked["samples_masked_share"] < 0.9 and keep_all["samples_masked_share"] == 0.0

    def dist(res):
        return max(abs(res["matrix"][i][j] - A[i][j]) for i in range(3) for j in range(3))
    assert dist(masked) < dist(keep_all)


# ---- the correction ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bt709_to_bt601", "bt601_to_bt709", "bt2020_to_bt709"])
def test_correction_undoes_a_named_map(name):
    from pqa2_amd.align import colour_correction, named_colour_map
    ref = R.clip(21, 131, 77, 8, 1, 1, 2)
    dis = [R.convert(f, *named_colour_map(name, 8), 8, 1, 1) for f in ref]
    res = _measure(ref, dis, 8)
    assert res["kind"] == name
    m = colour_correction(res, 8)
    assert m is not None and m.dtype == np.int32 and m.shape == (12,)
    back = [R.apply(f, m, 8, 1, 1) for f in dis]
    before = np.sum([R.plane_sse(a, c) for a, c in zip(ref, dis)], axis=0)
    after = np.sum([R.plane_sse(a, c) for a, c in zip(ref, back)], axis=0)
    assert all(b0 >= 2.0 * a0 for b0, a0 in zip(before, after)), (before, after)
    ident = np.array([0, 16384, 0, 0, 0, 0, 16384, 0, 0, 0, 0, 16384], np.int32)
    assert all(np.array_equal(x, y) for x, y in zip(R.apply(ref[0], ident, 8, 1, 1), ref[0]))


def test_correction_refuses_what_the_abi_cannot_take():
    from pqa2_amd.align import colour_correction, colour_matrix_q14
    base = {"kind": "matrix", "map_offset": [0.0, 0.0, 0.0]}
    assert colour_correction(dict(base, map_matrix=[[1.0, 0.0, 0.0], [0.0, 1.0, 1.0], [0.0, 1.0, 1.0]]), 8) is None      # singular
    assert colour_correction(dict(base, map_matrix=[[0.2, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]), 8) is None      # inverse gain 5
    ok = colour_correction(dict(base, map_matrix=[[0.5, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]), 8)
    assert list(ok) == [0, 32768, 0, 0, 0, 0, 16384, 0, 0, 0, 0, 16384]
    assert colour_matrix_q14([[4, 0, 0], [0, 1, 0], [0, 0, 1]], [0, 0, 0]) is None      # a gain of 4 is the first one out
    assert colour_matrix_q14([[1, 0, 0], [0, 1, 0], [0, 0, 1]], [16384, 0, 0]) is None  # as is an offset of 2^14 code values
    assert colour_matrix_q14([[1, 0, 0], [0, 1, 0], [0, 0, 1]], [-16383, 0, 0]) is not None


# ---- library and host without a GPU ------------------------------------------------------------------------------------------
def test_library_rules_without_a_context():
    """no context can be made without a device; what remains is the null-context rule of every entry and the constant"""
    from pqa2_amd import _native as N
    lib = N.load()
    assert lib.pqa_colour_sums() == 28 == N.COLOUR_SUMS
    out = np.zeros(28, np.uint64)
    m = (C.c_int32 * 12)()
    assert lib.pqa_colour_moments(None, None, None, None, None, 0, 1, 254, out.ctypes.data) == N.PQA_EINVAL
    assert lib.pqa_colour_moments_device(None, None, None, 0, 1, 254, out.ctypes.data) == N.PQA_EINVAL
    assert lib.pqa_colour_apply(None, C.byref(m), None, None, None, None, 0) == N.PQA_EINVAL
    assert lib.pqa_colour_apply_device(None, C.byref(m), None, None, 0) == N.PQA_EINVAL
    P = C.c_void_p * 3
    planes = [np.zeros((2, 8), np.uint8), np.zeros((1, 4), np.uint8), np.zeros((1, 4), np.uint8)]
    pp = P(*[p.ctypes.data for p in planes])
    for args in ((9, 1, 1, 8, 2, C.byref(pp), C.byref(pp), 1, 254),      # bit depth
                 (8, 2, 1, 8, 2, C.byref(pp), C.byref(pp), 1, 254),      # chroma shift
                 (8, 1, 1, 0, 2, C.byref(pp), C.byref(pp), 1, 254),      # size
                 (8, 1, 1, 8, 2, None, C.byref(pp), 1, 254),             # null planes
                 (8, 1, 1, 8, 2, C.byref(pp), C.byref(pp), 9, 8),        # lo > hi
                 (8, 1, 1, 8, 2, C.byref(pp), C.byref(pp), 0, 256)):     # hi > top
        assert lib.pqa_debug_colour(*args, out.ctypes.data, None, None) == N.PQA_EINVAL
    bad = (C.c_int32 * 12)(0, 65536, 0, 0, 0, 0, 16384, 0, 0, 0, 0, 16384)
    assert lib.pqa_debug_colour(8, 1, 1, 8, 2, C.byref(pp), C.byref(pp), 1, 254, None, C.byref(bad), C.byref(pp)) == N.PQA_EINVAL


def test_cli_flags_parse(tmp_path, monkeypatch):
    from pqa2_amd import pipeline, score
    seen = []

    def fake(*a, **kw):
        seen.append(kw)
        raise RuntimeError("stop")
    monkeypatch.setattr(pipeline, "score_files", fake)
    monkeypatch.setattr(score, "_die_with_parent", lambda *a, **k: None)
    base = ["r.y4m", "d.y4m", "--json", str(tmp_path / "x.json")]
    score.main(base)
    score.main(base + ["--colour-align"])
    score.main(base + ["--colour-correct", "--colour-frames", "3"])
    assert "colour_align" not in seen[0] and "colour_frames" not in seen[0]
    assert (seen[1]["colour_align"], seen[1]["colour_frames"]) == ("report", 8)
    assert (seen[2]["colour_align"], seen[2]["colour_frames"]) == ("apply", 3)


def test_report_line_log_keys_and_analyzer_options():
    from pqa2_amd import report
    from pqa2_amd.align import named_colour_map
    from pqa2_amd.vmaf_analyzer import VMAFAnalyzer
    ref = R.clip(7, 64, 48, 8, 1, 1, 2)
    dis = [R.convert(f, *named_colour_map("bt709_to_bt601", 8), 8, 1, 1) for f in ref]
    col = dict(_measure(ref, dis, 8), applied=True)
    line = report.colour_summary_line(col)
    assert "decoded as bt709 and encoded as bt601" in line and line.endswith(", corrected")
    assert "not corrected" in report.colour_summary_line(dict(col, applied=False))
    assert "level alignment" in report.colour_summary_line(dict(col, applied=False, cross_plane=False))
    assert "nothing to correct" in report.colour_summary_line(dict(col, kind="identity", mismatch=False, applied=False))
    assert "no map measured" in report.colour_summary_line({"degenerate": True, "frames": 3})
    keys = report.alignment_log_keys({"colour": dict(col, mse_matrix=float("nan"), offset=[float("inf"), 0.0, 1.0])})
    assert keys["alignment"]["colour"]["mse_matrix"] is None and keys["alignment"]["colour"]["offset"] == [None, 0.0, 1.0]
    json.dumps(keys)
    an = VMAFAnalyzer()
    assert an.colour_align_enabled is False and an.colour_correct_enabled is False
    assert "colour_align" not in an._ssim_family_kwargs()
    an.set_advanced_options(colour_align_enabled=True)
    assert an._ssim_family_kwargs()["colour_align"] == "report"
    an.set_advanced_options(colour_correct_enabled=True)
    assert an.colour_align_enabled is False and an._ssim_family_kwargs()["colour_align"] == "apply"


# ---- score_files through the oracle stand-in ---------------------------------------------------------------------------------
def _colour_engine():
    from tests.fake_engine import OracleEngine

    class ColourEngine(OracleEngine):
        """the oracle stand-in plus the restated colour kernels"""

        def colour_moments(self, ref_frames, dis_frames, lo=None, hi=None):
            return R.colour_moments(ref_frames, dis_frames, 8, 1, 1, lo, hi)

        def colour_apply(self, frames, m):
            return [R.apply(f, m, 8, 1, 1) for f in frames]
    return ColourEngine


def _write(tmp_path, n=3, w=48, h=32, mono=False):
    from pqa2_amd import align as AL
    from pqa2_amd.yuvio import VideoInfo, write_y4m
    info = VideoInfo(width=w, height=h, fps_num=24, fps_den=1, bit_depth=8, mono=mono, hshift=1, vshift=1,
                     chroma_tag="mono" if mono else "420")
    ref = R.clip(31, w, h, 8, 1, 1, n)
    A, b = AL.named_colour_map("bt709_to_bt601", 8)
    cap = [R.convert(f, A, b, 8, 1, 1) for f in ref]
    res = AL.best_colour(R.colour_moments(ref, cap, 8, 1, 1), 8, 1, 1)
    m = AL.colour_correction(res, 8)
    back = [R.apply(f, m, 8, 1, 1) for f in cap]
    paths = {}
    for key, clip in (("ref", ref), ("dis", cap), ("dis_back", back)):
        paths[key] = str(tmp_path / (key + ".y4m"))
        write_y4m(paths[key], [f[:1] for f in clip] if mono else clip, info)
    return paths, [int(v) for v in m]


def test_score_files_report_and_apply(tmp_path):
    from pqa2_amd import report
    from pqa2_amd.pipeline import score_files
    p, m = _write(tmp_path)
    kw = dict(engine_factory=_colour_engine())
    with pytest.raises(ValueError, match="colour_align must be"):
        score_files(p["ref"], p["dis"], "vmaf_v0.6.1", colour_align="bogus", **kw)
    with pytest.raises(ValueError, match="colour_frames"):
        score_files(p["ref"], p["dis"], "vmaf_v0.6.1", colour_align="report", colour_frames=0, **kw)
    plain = score_files(p["ref"], p["dis"], "vmaf_v0.6.1", **kw)
    rep = score_files(p["ref"], p["dis"], "vmaf_v0.6.1", colour_align="report", colour_frames=2, **kw)
    col = rep["alignment"]["colour"]
    assert (col["kind"], col["mismatch"], col["cross_plane"], col["applied"], col["frames"], col["full_range"]) == \
        ("bt709_to_bt601", True, True, False, 2, False)
    assert col["correction"] == m and "alignment" not in plain and "alignment" not in report.alignment_log_keys(None)
    assert np.array_equal(rep["records"].view(np.uint64), plain["records"].view(np.uint64))
    assert "colour" in json.loads(json.dumps(report.alignment_log_keys(rep["alignment"])))["alignment"]
    done = score_files(p["ref"], p["dis"], "vmaf_v0.6.1", colour_align="apply", **kw)
    assert done["alignment"]["colour"]["applied"] is True and done["alignment"]["colour"]["frames"] == 3
    by_hand = score_files(p["ref"], p["dis_back"], "vmaf_v0.6.1", **kw)
    assert np.array_equal(done["records"].view(np.uint64), by_hand["records"].view(np.uint64))
    assert not np.array_equal(done["records"].view(np.uint64), plain["records"].view(np.uint64))
    assert done["psnr_lines"] == by_hand["psnr_lines"]
    same = score_files(p["ref"], p["ref"], "vmaf_v0.6.1", colour_align="apply", **kw)
    assert (same["alignment"]["colour"]["kind"], same["alignment"]["colour"]["applied"]) == ("identity", False)
    full = score_files(p["ref"], p["dis"], "vmaf_v0.6.1", colour_align="report", colour_full_range=True, **kw)
    assert full["alignment"]["colour"]["full_range"] is True


def test_monochrome_clip_is_refused(tmp_path):
    from pqa2_amd.pipeline import score_files
    p, _ = _write(tmp_path, mono=True)
    with pytest.raises(ValueError, match="monochrome"):
        score_files(p["ref"], p["dis"], "vmaf_v0.6.1", colour_align="report", engine_factory=_colour_engine())


def test_kernel_uses_no_scratch_and_every_instance_is_built(tmp_path):
    """the compiler's own figures for csrc/colour_moments.hip: 8 moments and 8 apply kernels (u8 / u16, four subsamplings),
    none touches scratch, and a lane's 27 non-trivial partials and their 64-bit sums fit three waves a SIMD or two"""
    import os
    import re
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "colour.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                    os.path.join(root, "pqa2_amd", "csrc", "colour_moments.hip"), "-o", str(out)], check=True, capture_output=True)
    text = out.read_text()
    scratch = [int(x) for x in re.findall(r"^; ScratchSize: (\d+)", text, re.M)]
    vgprs = [int(x) for x in re.findall(r"^; TotalNumVgprs: (\d+)", text, re.M)]
    assert len(scratch) == 16 and all(s == 0 for s in scratch), scratch
    assert all(v <= 256 for v in vgprs), vgprs
    assert "Folded Reload" not in text and "Folded Spill" not in text
