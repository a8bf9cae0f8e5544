"""Transfer-curve alignment on the host: the isotonic regression, the monotone curve and its inverse table (align.best_curve,
align.curve_lut), and score_files(level_curve=True) through the oracle stand-in.  Inputs: tests/level_ref.py and
tests/curve_ref.py.  No GPU."""
from fractions import Fraction

import numpy as np
import pytest

from tests import curve_ref as C
from tests import level_ref as R

GAMMAS = (2.4 / 2.2, 2.2 / 2.4, 1.2, 0.8)


def _chosen_mse(lv):
    return lv["mse_affine"] if lv["kind"] == "affine" else lv["named"][lv["kind"]]


# ---- the solver ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_affine_cases_keep_their_kind(name, noise):
    """a gain and offset is no curve: with noise the monotone fit gains nothing to speak of, without it only the rounding"""
    from pqa2_amd.align import best_curve, best_levels
    ref, dis = R.case_pair(name, noise)
    T = R.level_stats([ref], [dis], 8)
    lv, cv = best_levels(T, 8), best_curve(T, 8)
    assert cv["kind"] == lv["kind"] == R.CASES[name][3] and cv["mismatch"] == lv["mismatch"]
    assert {k: cv[k] for k in lv} == lv                       # the best_levels() result stands unchanged
    assert not cv["curve_degenerate"] and cv["knots"] >= 2
    assert cv["mse_curve"] <= cv["mse_monotone"] <= _chosen_mse(lv)
    if noise:
        assert _chosen_mse(lv) <= 1.004 * cv["mse_monotone"]
    else:
        assert _chosen_mse(lv) - cv["mse_monotone"] < 0.5


def _gamma_cases():
    for g in GAMMAS:
        for sigma in (0.0, 2.0):
            yield pytest.param(8, g, sigma, id=f"8bit-g{g:.3f}-s{sigma:g}")
    for sigma in (0.0, 4.0):
        yield pytest.param(10, 2.4 / 2.2, sigma, id=f"10bit-s{sigma:g}")


@pytest.mark.parametrize("bpc, gamma, sigma", list(_gamma_cases()))
def test_gamma_captures_become_curve(bpc, gamma, sigma):
    from pqa2_amd.align import best_curve, best_levels, correction_lut, curve_lut
    ref = R.smooth_field(11, 320, 180, 0, 255) if bpc == 8 else R.smooth_field(11, 320, 180, 64, 940, bpc=10)
    dis = C.gamma_capture(ref, gamma, bpc, sigma)
    T = R.level_stats([ref], [dis], bpc)
    lv, cv = best_levels(T, bpc), best_curve(T, bpc)
    assert cv["kind"] == "curve" and cv["mismatch"] and not cv["curve_degenerate"]
    assert cv["mse_curve"] <= cv["mse_monotone"] < cv["mse_affine"]
    assert _chosen_mse(lv) > 1.1 * cv["mse_monotone"] and _chosen_mse(lv) - cv["mse_monotone"] >= 0.5 * 4 ** (bpc - 8)
    lut = curve_lut(T, bpc)
    assert lut.dtype == (np.uint8 if bpc == 8 else np.uint16) and lut.shape == (1 << bpc,) and np.all(np.diff(lut.astype(np.int64)) >= 0)
    by_curve, by_affine = C.mse(C.table_apply(dis, lut, bpc), ref), C.mse(np.take(correction_lut(lv, bpc), dis), ref)
    assert by_curve < by_affine and by_curve < C.mse(dis, ref)
    if bpc == 8:       # the estimate is reported only; a pure power law over the full range must come out near its exponent
        assert abs(cv["gamma"] - gamma) < 0.01


def test_gamma_is_normalised_to_the_range_asked_for():
    from pqa2_amd.align import best_curve
    lo, hi = 16, 235
    ref = R.smooth_field(11, 320, 180, lo, hi)
    x = (ref.astype(np.float64) - lo) / (hi - lo)
    dis = np.floor(lo + (hi - lo) * x ** 1.2 + 0.5).astype(np.uint8)
    T = R.level_stats([ref], [dis], 8)
    assert abs(best_curve(T, 8, full_range=False)["gamma"] - 1.2) < 0.01
    assert abs(best_curve(T, 8, full_range=True)["gamma"] - 1.2) > 0.02
    assert best_curve(T, 8, chroma=True)["gamma"] is None


def test_thresholds_move_the_decision():
    from pqa2_amd.align import best_curve
    ref = R.smooth_field(11, 320, 180, 0, 255)
    T = R.level_stats([ref], [C.gamma_capture(ref, 2.4 / 2.2, 8, 2.0)], 8)
    assert best_curve(T, 8)["kind"] == "curve"
    assert best_curve(T, 8, curve_snap=2.0)["kind"] == "affine"          # 5.37 against 4.04: no factor of two
    assert best_curve(T, 8, curve_min_gain=5.0)["kind"] == "affine"      # nor a gap of five
    assert best_curve(T, 8, min_count=10 ** 6)["curve_degenerate"]       # no level is a knot


# ---- isotonic regression ---------------------------------------------------------------------------------------------------
def test_isotonic_pools_violators_to_their_weighted_mean():
    from pqa2_amd.align import isotonic
    out = isotonic([1, 5, 2, 7], [1, 1, 3, 1])
    assert out == [1, Fraction(11, 4), Fraction(11, 4), 7] and all(isinstance(v, Fraction) for v in out)
    assert isotonic([3, 2, 1], [1, 1, 1]) == [2, 2, 2]                        # a chain of violators ends in one block
    assert isotonic([4, 1, 3, 2], [2, 2, 1, 1]) == [Fraction(5, 2)] * 4       # pooling back across an earlier block
    assert isotonic([1, 2, 2, 3], [1, 5, 1, 1]) == [1, 2, 2, 3]               # equal means stay apart: nothing moves
    assert isotonic([Fraction(1, 3), Fraction(1, 4)], [3, 4]) == [Fraction(2, 7)] * 2
    assert isotonic([], []) == []
    with pytest.raises(ValueError):
        isotonic([1], [0])


# ---- the inverse table -----------------------------------------------------------------------------------------------------
def test_clipped_top_plateau_maps_top_to_the_weighted_mean_of_the_run():
    from pqa2_amd.align import best_curve, curve_lut
    # dis = 2 ref up to 100, clipped at 255 from 128 on; levels 128 ... 131 hold 100, 100, 100 and 500 pixels
    rows = {v: (100, 200 * v) for v in range(20, 128)}
    rows.update({128: (100, 25500), 129: (100, 25500), 130: (100, 25500), 131: (500, 127500)})
    T = C.hand_table(8, rows)
    lut = curve_lut(T, 8)
    assert lut[255] == (128 * 100 + 129 * 100 + 130 * 100 + 131 * 500 + 400) // 800 == 130
    assert lut[40] == 20 and lut[100] == 50 and lut[101] == 50 and lut[102] == 51       # 101: a tie, the lower candidate wins
    assert lut[254] == 127 and np.all(np.diff(lut.astype(np.int64)) >= 0)
    assert best_curve(T, 8)["knots"] == 112


def test_empty_run_maps_to_its_midpoint_and_slope_one_outside_the_knots():
    from pqa2_amd.align import curve_lut
    # knots 100 ... 110 with dis = ref: below, g(v) = v down to 0; above, g(v) = v up to top -- the identity
    T = C.hand_table(8, {v: (50, 50 * v) for v in range(100, 111)})
    assert np.array_equal(curve_lut(T, 8), np.arange(256))
    # knots 10 ... 20 at dis = ref + 240: g reaches top at 15, 15 ... 20 is a populated plateau, 21 ... 255 an empty one whose g
    # is top as well -- one run 15 ... 255 whose pixels all sit in 15 ... 20; g(v) = v + 240 below 10 falls to 230 at v = 0
    T = C.hand_table(8, {v: (50, 50 * min(v + 240, 255)) for v in range(10, 21)})
    lut = curve_lut(T, 8)
    assert lut[255] == (sum(range(15, 21)) * 50 * 2 + 300) // 600 == 18 and lut[254] == 14 and lut[241] == 1
    assert np.all(lut[:231] == 0)
    # knots 200 and 201 at dis = 0 and 1: g is clamped to 0 over 0 ... 200, a run that holds level 200's pixels only; above 201,
    # g(v) = v - 200
    T = C.hand_table(8, {200: (50, 0), 201: (50, 50)})
    lut = curve_lut(T, 8)
    assert lut[0] == 200 and lut[1] == 201 and lut[55] == 255 and lut[200] == 255
    # knots 0 and 1 at dis = 250 and 251: g(v) = min(255, 250 + v), and the run 5 ... 255 holds no pixel: its midpoint 130
    T = C.hand_table(8, {0: (50, 12500), 1: (50, 12550)})
    lut = curve_lut(T, 8)
    assert lut[255] == 130 and lut[254] == 4 and lut[250] == 0 and lut[0] == 0
    T = C.hand_table(8, {0: (50, 12500), 1: (50, 12550), 3: (2, 506)})       # two pixels below min_count in the run's reach: not in it
    assert curve_lut(T, 8)[255] == 130
    T = C.hand_table(8, {0: (50, 12500), 1: (50, 12550), 200: (2, 510)})     # ... and two inside it: its weighted mean
    assert curve_lut(T, 8)[255] == 200


def test_lower_candidate_wins_a_tie():
    from pqa2_amd.align import curve_lut
    T = C.hand_table(8, {v: (20, 20 * (2 * v)) for v in range(10, 100)})     # g(v) = 2 v: every odd d lies between two levels
    lut = curve_lut(T, 8)
    assert [int(lut[d]) for d in (40, 41, 42, 43)] == [20, 20, 21, 21]
    T = C.hand_table(8, {v: (20, 20 * (3 * v)) for v in range(10, 80)})      # g(v) = 3 v: nearest, no tie
    lut = curve_lut(T, 8)
    assert [int(lut[d]) for d in (60, 61, 62, 63)] == [20, 20, 21, 21]


def test_degenerate_tables_form_no_curve():
    from pqa2_amd.align import best_curve, curve_lut
    T = C.hand_table(8, {77: (1000, 80000)})
    cv = best_curve(T, 8)
    assert cv["curve_degenerate"] and cv["degenerate"] and cv["kind"] == "identity" and cv["mse_monotone"] is None and cv["knots"] == 0
    with pytest.raises(ValueError, match="no curve"):
        curve_lut(T, 8)
    flat = C.hand_table(8, {v: (100, 12800) for v in range(50, 60)})         # a capture that is flat whatever the reference
    assert best_curve(flat, 8)["curve_degenerate"]
    with pytest.raises(ValueError, match="no curve"):
        curve_lut(flat, 8)
    # independent random pictures: where the fitted gain is not positive nothing follows the reference, no curve is formed
    seen = 0
    for seed in range(12):
        ref, dis = R.random_pair(seed, 1, 64, 64)
        T = R.level_stats(ref, dis, 8)
        cv = best_curve(T, 8)
        assert cv["kind"] != "curve"
        if cv["gain"] <= 0:
            seen += 1
            assert cv["curve_degenerate"] and cv["mse_monotone"] is None and cv["gamma"] is None
    assert seen >= 1


def test_table_sse_is_the_squared_error():
    from pqa2_amd.align import table_sse
    ref, dis = R.random_pair(4, 2, 33, 17)
    assert table_sse(R.level_stats(ref, dis, 8)) == sum(R.table_sse(R.level_stats(ref, dis, 8)))


# ---- score_files through the oracle stand-in ---------------------------------------------------------------------------------
def _curve_engine(spoil=False):
    from tests.fake_engine import OracleEngine

    class CurveEngine(OracleEngine):
        """the oracle stand-in plus the restated transfer table and table apply"""
        calls = []

        def level_stats(self, ref_frames, dis_frames, plane=0):
            return R.level_stats(ref_frames, dis_frames, 8)

        def table_apply(self, frames, table, plane=0):
            CurveEngine.calls.append((len(frames), plane))
            if spoil:     # a table that makes matters worse: the check must turn it down
                return [255 - np.asarray(f) for f in frames]
            return [C.table_apply(np.asarray(f), table, 8) for f in frames]
    return CurveEngine


def _write(tmp_path, n=4, w=64, h=48, gamma=1.3):
    from pqa2_amd import align as AL
    from pqa2_amd.yuvio import VideoInfo, write_y4m
    info = VideoInfo(width=w, height=h, fps_num=24, fps_den=1, bit_depth=8, mono=False, hshift=1, vshift=1, chroma_tag="420",
                     color_range="full")     # gamma is normalised to the range the captured clip declares
    ref = [[R.smooth_field(90 + t, w, h, 0, 255, t)] + [R.smooth_field(95 + 5 * p + t, w // 2, h // 2, 16, 240, t) for p in range(2)]
           for t in range(n)]
    cap = [[C.gamma_capture(f[0], gamma), f[1].copy(), f[2].copy()] for f in ref]
    table = AL.curve_lut(R.level_stats([f[0] for f in ref], [f[0] for f in cap], 8), 8)
    back = [[C.table_apply(f[0], table, 8), f[1], f[2]] for f in cap]
    paths = {}
    for key, clip in (("ref", ref), ("dis", cap), ("dis_back", back)):
        paths[key] = str(tmp_path / (key + ".y4m"))
        write_y4m(paths[key], clip, info)
    return paths


def test_score_files_level_curve(tmp_path):
    from pqa2_amd.pipeline import score_files
    p = _write(tmp_path)
    Eng = _curve_engine()
    kw = dict(engine_factory=Eng)
    with pytest.raises(ValueError, match="level_curve needs"):
        score_files(p["ref"], p["dis"], "vmaf_v0.6.1", level_curve=True, **kw)
    plain = score_files(p["ref"], p["dis"], "vmaf_v0.6.1", **kw)
    # off: today's results, key for key
    off = score_files(p["ref"], p["dis"], "vmaf_v0.6.1", level_align="apply", **kw)
    off2 = score_files(p["ref"], p["dis"], "vmaf_v0.6.1", level_align="apply", level_curve=False, **kw)
    assert off["alignment"] == off2["alignment"] and "mse_monotone" not in off["alignment"]["levels"]
    assert off["alignment"]["levels"]["kind"] != "curve" and not Eng.calls
    assert np.array_equal(off["records"].view(np.uint64), off2["records"].view(np.uint64))
    # report: the curve is found, the records are left alone, the table is never applied
    rep = score_files(p["ref"], p["dis"], "vmaf_v0.6.1", level_align="report", level_curve=True, **kw)
    lv = rep["alignment"]["levels"]
    assert (lv["kind"], lv["mismatch"], lv["applied"], lv["curve_applied"], lv["mse_after"]) == ("curve", True, False, False, None)
    assert abs(lv["gamma"] - 1.3) < 0.02 and lv["knots"] > 100 and lv["mse_monotone"] < lv["mse_affine"]
    assert [lv["planes"][k]["kind"] for k in "yuv"] == ["curve", "identity", "identity"]
    assert all(set(("mse_monotone", "knots", "gamma", "curve_applied", "mse_after")) <= set(lv["planes"][k]) for k in "yuv")
    assert {k: v for k, v in lv.items() if k != "planes"} == lv["planes"]["y"]
    assert np.array_equal(rep["records"].view(np.uint64), plain["records"].view(np.uint64)) and not Eng.calls
    # apply: the records of the capture mapped by hand
    done = score_files(p["ref"], p["dis"], "vmaf_v0.6.1", level_align="apply", level_curve=True, **kw)
    lv = done["alignment"]["levels"]
    assert [lv["planes"][k]["applied"] for k in "yuv"] == [True, False, False] and lv["curve_applied"]
    assert lv["mse_after"] < lv["mse_identity"] and lv["mse_after"] < off["alignment"]["levels"]["mse_affine"]
    assert Eng.calls[0] == (4, 0) and all(c[1] == 0 for c in Eng.calls)       # the check, then one call per run of the luma plane
    by_hand = score_files(p["ref"], p["dis_back"], "vmaf_v0.6.1", **kw)
    assert np.array_equal(done["records"].view(np.uint64), by_hand["records"].view(np.uint64))
    assert not np.array_equal(done["records"].view(np.uint64), plain["records"].view(np.uint64))
    assert done["psnr_lines"] == by_hand["psnr_lines"]


def test_score_files_turns_down_a_curve_that_does_not_help(tmp_path):
    from pqa2_amd.pipeline import score_files
    p = _write(tmp_path)
    kw = dict(engine_factory=_curve_engine(spoil=True))
    plain = score_files(p["ref"], p["dis"], "vmaf_v0.6.1", **kw)
    done = score_files(p["ref"], p["dis"], "vmaf_v0.6.1", level_align="apply", level_curve=True, **kw)
    lv = done["alignment"]["levels"]
    assert lv["kind"] == "curve" and lv["mismatch"] and lv["mse_after"] >= lv["mse_identity"]
    assert lv["curve_applied"] is False and lv["applied"] is False
    assert np.array_equal(done["records"].view(np.uint64), plain["records"].view(np.uint64))


# ---- the front ends --------------------------------------------------------------------------------------------------------
def test_cli_flag_analyzer_attribute_and_summary_line():
    from pqa2_amd import report, score
    from pqa2_amd.align import best_curve
    from pqa2_amd.vmaf_analyzer import VMAFAnalyzer
    import inspect
    assert "--level-curve" in inspect.getsource(score)
    ref = R.smooth_field(11, 320, 180, 0, 255)
    lv = dict(best_curve(R.level_stats([ref], [C.gamma_capture(ref, 1.2)], 8), 8), applied=True, curve_applied=True, mse_after=0.02)
    lv["planes"] = {"y": dict(lv)}
    line = report.levels_summary_line(lv)
    assert "transfer curve" in line and "gamma 1.200" in line and "corrected on Y" in line and "about the curve" in line
    assert "transfer curve" in report.levels_summary_line(dict(lv, gamma=None)) and "gamma" not in report.levels_summary_line(dict(lv, gamma=None))
    keys = report.alignment_log_keys({"levels": lv})
    assert keys["alignment"]["levels"]["kind"] == "curve" and keys["alignment"]["levels"]["planes"]["y"]["curve_applied"] is True
    an = VMAFAnalyzer()
    assert an.level_curve_enabled is False and "level_curve" not in an._ssim_family_kwargs()
    an.set_advanced_options(level_curve_enabled=True)
    assert an.level_curve_enabled and an._ssim_family_kwargs()["level_curve"] is True and an._ssim_family_kwargs()["level_align"] == "report"
    an.set_advanced_options(level_correct_enabled=True, level_curve_enabled=True)
    assert an._ssim_family_kwargs()["level_align"] == "apply" and an._ssim_family_kwargs()["level_curve"] is True
    an.set_advanced_options(level_correct_enabled=True)
    assert an.level_curve_enabled is False and "level_curve" not in an._ssim_family_kwargs()
