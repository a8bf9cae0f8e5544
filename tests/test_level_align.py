"""Level alignment on the host (no GPU): the numpy restatement against a direct sum, align.best_levels on five synthetic
captures with and without noise, the correction table, the degenerate flat pair, the chroma and 10-bit named maps, the
report line and options, and score_files(level_align=) through tests/fake_engine.py."""
from fractions import Fraction

import numpy as np
import pytest

from tests import level_ref as R


def test_restatement_sse_identity_and_clamped_bin():
    ref, dis = R.random_pair(3, 2, 33, 9)
    T = R.level_stats(ref, dis, 8)
    assert T.dtype == np.uint64 and T.shape == (2, 256, 3) and int(T[:, :, 0].sum()) == 2 * 33 * 9
    assert R.table_sse(T) == [int(((r.astype(np.int64) - d.astype(np.int64)) ** 2).sum()) for r, d in zip(ref, dis)]
    r10 = np.array([[5, 1023, 1024, 65535]], np.uint16)     # a 16-bit container: levels above L - 1 land in bin L - 1
    d10 = np.array([[7, 1, 2000, 65535]], np.uint16)        # ... and the captured partner enters as it is
    T = R.level_stats([r10], [d10], 10)
    assert T[0, 5].tolist() == [1, 7, 49] and int(T[0, :, 0].sum()) == 4
    assert T[0, 1023].tolist() == [3, 1 + 2000 + 65535, 1 + 2000 ** 2 + 65535 ** 2]


def _polyfit_error(name, noise):
    """the independent reference: float64 numpy.polyfit on the same pair, restricted to the unclipped pixels"""
    (_, _), a, b, _, _ = R.CASES[name]
    ref, dis = R.case_pair(name, noise)
    m = (dis > 0) & (dis < 255)
    pa, pb = np.polyfit(ref[m].astype(np.float64), dis[m].astype(np.float64), 1)
    return abs(pa - a), abs(pb - b)


@pytest.fixture(scope="module")
def tolerances():
    """{noise: (gain tolerance, offset tolerance)}: twice the worst error of the polyfit reference over the five cases"""
    out = {}
    for noise in (False, True):
        errs = [_polyfit_error(name, noise) for name in R.CASES]
        out[noise] = (2 * max(e[0] for e in errs), 2 * max(e[1] for e in errs))
    return out


@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("name", list(R.CASES))
def test_best_levels_cases(name, noise, tolerances):
    """320 x 180, 8 bit, smooth field + noise; (a) identity, (b) 16 ... 235 expanded to full, (c) full swing compressed to
    limited, (d) full swing expanded with clipping, (e) gain 0.9 offset +7; each with and without sigma = 2 noise on the
    capture.  Tolerance on gain / offset: twice the worst error of numpy.polyfit (float64, unclipped pixels only) over the
    five cases.  Measured: polyfit's worst error is 0.00017 in gain and 0.048 in offset without noise, 0.00017 and 0.028
    with it, so the tolerances are 0.00034 / 0.095 and 0.00034 / 0.056; best_levels' worst error is 0.00017 / 0.048 without
    noise and 0.00010 / 0.003 with it.  The wrong named maps are worse than the right one by a factor of 13.5 at least
    (cases a to d)."""
    from pqa2_amd.align import best_levels
    _, a, b, kind, mismatch = R.CASES[name]
    ref, dis = R.case_pair(name, noise)
    res = best_levels(R.level_stats([ref], [dis], 8), 8)
    gain_tol, off_tol = tolerances[noise]
    print(f"{name} noise={noise}: gain error {res['gain'] - a:+.5f} (tolerance {gain_tol:.5f}), offset error "
          f"{res['offset'] - b:+.4f} (tolerance {off_tol:.4f}), named {res['named']}")
    assert res["kind"] == kind and res["mismatch"] is mismatch and res["degenerate"] is False and res["frames"] == 1
    assert abs(res["gain"] - a) <= gain_tol and abs(res["offset"] - b) <= off_tol
    assert res["mse_curve"] <= res["mse_affine"] + 1e-12 and res["mse_affine"] <= res["mse_identity"] + 1e-9
    assert res["mse_identity"] == res["named"]["identity"]
    if kind != "affine":     # a named kind carries the named map's own a and b, not the fitted ones
        from pqa2_amd.align import named_level_map
        assert (res["map_gain"], res["map_offset"]) == tuple(float(x) for x in named_level_map(kind, 8))
        assert res["named"][kind] == min(res["named"].values())
    else:
        assert (res["map_gain"], res["map_offset"]) == (res["gain"], res["offset"])


def test_refit_removes_the_clipping_bias():
    """case (d): the first fit sees the clipped ends and is too flat; the refit over the unclipped levels is not"""
    from pqa2_amd import align as AL
    ref, dis = R.case_pair("d_full_expanded_clipped", False)
    T = R.level_stats([ref], [dis], 8)[0]
    T0, T1 = [int(x) for x in T[:, 0]], [int(x) for x in T[:, 1]]
    first = AL._fit([v for v in range(256) if T0[v]], T0, T1)
    res = AL.best_levels(T[None], 8)
    assert float(first[0]) < R.L2F[0] and abs(res["gain"] - R.L2F[0]) < abs(float(first[0]) - R.L2F[0])
    assert res["levels_used"] < sum(1 for c in T0 if c)


def test_lut_of_case_b_reproduces_the_reference():
    """(b) without noise: the rounding error 0.5 scaled by 219/255 is 0.43 < 0.5, so the table gives back every pixel"""
    from pqa2_amd import align as AL
    ref, dis = R.case_pair("b_limited_expanded", False)
    res = AL.best_levels(R.level_stats([ref], [dis], 8), 8)
    assert res["kind"] == "limited_to_full" and res["mse_curve"] == 0.0
    assert (res["map_gain"], res["map_offset"]) == (255 / 219, -16 * 255 / 219)
    lut = AL.correction_lut(res, 8)
    assert lut.dtype == np.uint8 and lut.shape == (256,)
    assert np.array_equal(lut, AL.level_lut(Fraction(255, 219), Fraction(-16 * 255, 219), 8))
    assert np.array_equal(R.apply_lut(dis, lut), ref)


def test_level_lut_definition():
    from pqa2_amd.align import level_lut
    assert np.array_equal(level_lut(1, 0, 8), np.arange(256))
    lut = level_lut(Fraction(1, 2), 10, 8)          # d = r / 2 + 10  ->  r = 2 (d - 10)
    assert lut[0] == 0 and lut[10] == 0 and lut[11] == 2 and lut[137] == 254 and lut[138] == 255 and lut[255] == 255
    assert level_lut(2, 0, 8)[1] == 1 and level_lut(2, 0, 8)[3] == 2      # halves round up: floor(x + 1/2)
    assert level_lut(1, 0, 10).dtype == np.uint16 and level_lut(1, 0, 10).shape == (1024,)
    with pytest.raises(ValueError):
        level_lut(0, 0, 8)


def test_degenerate_flat_pair():
    from pqa2_amd.align import best_levels
    ref, dis = np.full((20, 30), 16, np.uint8), np.full((20, 30), 0, np.uint8)
    res = best_levels(R.level_stats([ref, ref], [dis, dis], 8), 8)
    assert res["degenerate"] is True and (res["gain"], res["offset"], res["kind"], res["mismatch"]) == (1.0, 0.0, "identity", False)
    assert res["frames"] == 2 and res["mse_identity"] == 256.0 and res["mse_curve"] == 0.0
    with pytest.raises(ValueError):
        best_levels(np.zeros((1, 256, 3), np.uint64), 8)
    with pytest.raises(ValueError):
        best_levels(np.zeros((1, 256, 3), np.uint64), 10)


def test_chroma_named_maps():
    """a plane centred on 128: the chroma maps scale about the mid level, the luma maps do not fit it"""
    from pqa2_amd import align as AL
    assert AL.named_level_map("limited_to_full", 8, True) == (Fraction(255, 224), 128 * (1 - Fraction(255, 224)))
    assert AL.named_level_map("full_to_limited", 8, True) == (Fraction(224, 255), 128 * (1 - Fraction(224, 255)))
    ref = R.smooth_field(5, 160, 90, 16, 240)
    for kind, a in (("limited_to_full", 255 / 224), ("full_to_limited", 224 / 255)):
        dis = R.apply_map(ref, a, 128 * (1 - a))
        T = R.level_stats([ref], [dis], 8)
        res = AL.best_levels(T, 8, chroma=True)
        assert (res["kind"], res["mismatch"]) == (kind, True)
        assert AL.best_levels(T, 8, chroma=False)["kind"] == "affine"
        if kind == "limited_to_full":
            assert np.array_equal(R.apply_lut(dis, AL.correction_lut(res, 8, chroma=True)), ref)


def test_ten_bit_scaling_of_the_named_maps():
    from pqa2_amd import align as AL
    assert AL.named_level_map("limited_to_full", 10) == (Fraction(255, 219), Fraction(-64 * 255, 219))
    assert AL.named_level_map("full_to_limited", 10) == (Fraction(219, 255), Fraction(64))
    assert AL.named_level_map("full_to_limited", 10, True) == (Fraction(224, 255), 512 * (1 - Fraction(224, 255)))
    ref = R.smooth_field(6, 160, 90, 64, 940, bpc=10)
    dis = R.apply_map(ref, 255 / 219, -64 * 255 / 219, 10)
    res = AL.best_levels(R.level_stats([ref], [dis], 10), 10)
    assert (res["kind"], res["mismatch"], res["map_offset"]) == ("limited_to_full", True, -64 * 255 / 219)
    back = R.apply_lut(dis, AL.correction_lut(res, 10))
    assert back.dtype == np.uint16 and np.array_equal(back, ref)
    assert AL.best_levels(R.level_stats([ref], [R.apply_map(ref, 219 / 255, 64, 10)], 10), 10)["kind"] == "full_to_limited"


def test_option_values_move_the_decisions():
    from pqa2_amd.align import best_levels
    ref, dis = R.case_pair("e_gain_offset", True)
    T = R.level_stats([ref], [dis], 8)
    assert best_levels(T, 8)["kind"] == "affine"
    loose = best_levels(T, 8, snap=100.0)                     # the nearest named map is taken however poor
    assert loose["kind"] in ("identity", "limited_to_full", "full_to_limited")
    assert best_levels(T, 8, min_improvement=1000.0)["mismatch"] is False


def test_report_line_log_keys_and_analyzer_options():
    from pqa2_amd import report
    from pqa2_amd.align import best_levels
    from pqa2_amd.vmaf_analyzer import VMAFAnalyzer
    ref, dis = R.case_pair("b_limited_expanded", False)
    lv = dict(best_levels(R.level_stats([ref], [dis], 8), 8), applied=True)
    lv["planes"] = {"y": dict(lv)}
    line = report.levels_summary_line(lv)
    assert "expanded from limited to full range" in line and "corrected on Y" in line and "gain 1.16" in line
    assert "not corrected" in report.levels_summary_line(dict(lv, applied=False, planes=None))
    assert "nothing to correct" in report.levels_summary_line(dict(lv, kind="identity", mismatch=False, applied=False, planes=None))
    assert "flat reference" in report.levels_summary_line({"degenerate": True, "frames": 3})
    keys = report.alignment_log_keys({"levels": dict(lv, mse_curve=float("nan"))})
    assert keys["alignment"]["levels"]["mse_curve"] is None and keys["alignment"]["levels"]["kind"] == "limited_to_full"
    assert "confidence" not in keys["alignment"]["levels"] and keys["alignment"]["levels"]["planes"]["y"]["applied"] is True
    an = VMAFAnalyzer()
    assert an.level_align_enabled is False and an.level_correct_enabled is False
    assert "level_align" not in an._ssim_family_kwargs()
    an.set_advanced_options(level_align_enabled=True)
    assert an._ssim_family_kwargs()["level_align"] == "report"
    an.set_advanced_options(level_correct_enabled=True)
    assert an.level_align_enabled is False and an._ssim_family_kwargs()["level_align"] == "apply"


# ---- score_files through the oracle stand-in ---------------------------------------------------------------------------------
def _level_engine():
    from tests.fake_engine import OracleEngine

    class LevelEngine(OracleEngine):
        """the oracle stand-in plus the restated transfer table"""

        def level_stats(self, ref_frames, dis_frames, plane=0):
            return R.level_stats(ref_frames, dis_frames, 8)
    return LevelEngine


def _write(tmp_path, n=3, w=48, h=32):
    from pqa2_amd import align as AL
    from pqa2_amd.yuvio import VideoInfo, write_y4m
    info = VideoInfo(width=w, height=h, fps_num=24, fps_den=1, bit_depth=8, mono=False, hshift=1, vshift=1, chroma_tag="420")
    luts = [AL.level_lut(*AL.named_level_map("limited_to_full", 8, chroma=p > 0), 8) for p in range(3)]
    ref, cap, back = [], [], []
    for t in range(n):
        planes = [R.smooth_field(90 + t, w, h, 16, 235, t)] + [R.smooth_field(95 + 5 * p + t, w // 2, h // 2, 16, 240, t)
                                                               for p in range(2)]
        moved = [R.apply_map(planes[0], *R.L2F), R.apply_map(planes[1], 255 / 224, 128 * (1 - 255 / 224)), planes[2].copy()]
        ref.append(planes)
        cap.append(moved)
        back.append([R.apply_lut(moved[0], luts[0]), R.apply_lut(moved[1], luts[1]), moved[2]])
    paths = {}
    for key, clip in (("ref", ref), ("dis", cap), ("dis_back", back)):
        paths[key] = str(tmp_path / (key + ".y4m"))
        write_y4m(paths[key], clip, info)
    return paths


def test_score_files_report_and_apply(tmp_path):
    """luma and U expanded, V left alone: "report" leaves the records alone, "apply" maps exactly the planes with a
    mismatch and gives the records of the capture mapped back by hand"""
    from pqa2_amd.pipeline import score_files
    p = _write(tmp_path)
    kw = dict(engine_factory=_level_engine())
    with pytest.raises(ValueError, match="level_align must be"):
        score_files(p["ref"], p["dis"], "vmaf_v0.6.1", level_align="fix", **kw)
    with pytest.raises(ValueError, match="level_frames"):
        score_files(p["ref"], p["dis"], "vmaf_v0.6.1", level_align="report", level_frames=0, **kw)
    plain = score_files(p["ref"], p["dis"], "vmaf_v0.6.1", **kw)
    rep = score_files(p["ref"], p["dis"], "vmaf_v0.6.1", level_align="report", level_frames=2, **kw)
    lv = rep["alignment"]["levels"]
    assert (lv["kind"], lv["mismatch"], lv["applied"], lv["frames"]) == ("limited_to_full", True, False, 2)
    assert [lv["planes"][k]["kind"] for k in "yuv"] == ["limited_to_full", "limited_to_full", "identity"]
    assert lv["planes"]["y"]["gain"] == lv["gain"] and "alignment" not in plain
    assert np.array_equal(rep["records"].view(np.uint64), plain["records"].view(np.uint64))
    done = score_files(p["ref"], p["dis"], "vmaf_v0.6.1", level_align="apply", **kw)
    assert [done["alignment"]["levels"]["planes"][k]["applied"] for k in "yuv"] == [True, True, False]
    assert done["alignment"]["levels"]["frames"] == 3
    by_hand = score_files(p["ref"], p["dis_back"], "vmaf_v0.6.1", **kw)
    assert np.array_equal(done["records"].view(np.uint64), by_hand["records"].view(np.uint64))
    assert not np.array_equal(done["records"].view(np.uint64), plain["records"].view(np.uint64))
    assert done["psnr_lines"] == by_hand["psnr_lines"]
    same = score_files(p["ref"], p["dis_back"], "vmaf_v0.6.1", level_align="apply", **kw)
    assert same["alignment"]["levels"]["applied"] is False and same["alignment"]["levels"]["kind"] == "identity"
    assert np.array_equal(same["records"].view(np.uint64), by_hand["records"].view(np.uint64))
