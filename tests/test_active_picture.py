"""Active-picture detection on the host (no GPU): the numpy restatement of the line profiles (tests/profile_ref.py) against a
plain double loop, align.active_picture and align.common_window on synthetic profiles built with it, and
score_files(active_picture=) through the oracle stand-in."""
import json
from fractions import Fraction

import numpy as np
import pytest

from tests import profile_ref as R


def _dt(bpc):
    return np.uint8 if bpc == 8 else np.uint16


def _boxed(w, h, left=0, top=0, right=0, bottom=0, bpc=8, seed=0):
    """a picture of bright noise (64 ... 200 at 8 bit) inside bars of nominal black (16 at 8 bit)"""
    s = 1 << (bpc - 8)
    f = np.full((h, w), 16 * s, _dt(bpc))
    rng = np.random.default_rng(seed)
    f[top:h - bottom, left:w - right] = rng.integers(64 * s, 200 * s, (h - top - bottom, w - left - right))
    return f


def _solve(frames, bpc=8, **kw):
    from pqa2_amd import align as AL
    rows, _ = R.line_profiles(frames, bpc)
    return AL.active_picture(rows, R.cols_of(frames, bpc), bpc, **kw)


def _bars(ap):
    return [ap[k] for k in ("left", "top", "right", "bottom")]


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def test_restatement_against_a_double_loop():
    rng = np.random.default_rng(1)
    f = rng.integers(0, 1024, (5, 7)).astype(np.uint16)
    f[2, 3] = 60000      # above 1023: read as 1023
    rows, cols = R.line_profiles([f], 10)
    assert rows.dtype == cols.dtype == np.uint64 and rows.shape == (1, 5, 2) and cols.shape == (1, 7, 2)
    want_r, want_c = [[0, 0] for _ in range(5)], [[0, 0] for _ in range(7)]
    for y in range(5):
        for x in range(7):
            v = min(int(f[y, x]), 1023)
            want_r[y][0] += v
            want_r[y][1] += v * v
            want_c[x][0] += v
            want_c[x][1] += v * v
    assert rows[0].tolist() == want_r and cols[0].tolist() == want_c
    got = R.random_frames(3, 2, 7, 5, 12)
    assert len(got) == 2 and got[0].shape == (5, 7) and got[0].dtype == np.uint16 and int(max(g.max() for g in got)) < 4096


# ---- active_picture -----------------------------------------------------------------------------------------------------------
def test_no_bars():
    ap = _solve([_boxed(40, 24, seed=s) for s in range(3)])
    assert _bars(ap) == [0, 0, 0, 0] and ap["window"] == [0, 0, 40, 24]
    assert ap["frames_used"] == 3 and ap["all_dark"] is False and ap["bar_noise"] is None


def test_bars_of_one_row_and_one_column():
    ap = _solve([_boxed(40, 24, top=1, seed=s) for s in range(2)])
    assert _bars(ap) == [0, 1, 0, 0] and ap["window"] == [0, 1, 40, 23]
    ap = _solve([_boxed(40, 24, right=1, seed=s) for s in range(2)])
    assert _bars(ap) == [0, 0, 1, 0] and ap["window"] == [0, 0, 39, 24]


@pytest.mark.parametrize("bpc", [8, 10])
def test_letterbox_and_pillarbox_together(bpc):
    ap = _solve([_boxed(40, 24, 3, 5, 2, 4, bpc, seed=s) for s in range(3)], bpc)
    assert _bars(ap) == [3, 5, 2, 4] and ap["window"] == [3, 5, 35, 15] and ap["bar_noise"] == 0


@pytest.mark.parametrize("bpc", [8, 10])
def test_the_exact_boundary_of_the_rule(bpc):
    """a row whose sum is L n is dark, one whose sum is L n + 1 is not"""
    L = 24 << (bpc - 8)
    f = _boxed(8, 6, bpc=bpc, seed=4)
    f[0, :] = L
    assert int(f[0].sum()) == L * 8 and _bars(_solve([f], bpc))[1] == 1
    f[0, 5] += 1
    assert _bars(_solve([f], bpc))[1] == 0
    g = _boxed(8, 6, bpc=bpc, seed=5)      # the same for a column, n = the active height
    g[:, 7] = L
    assert _bars(_solve([g], bpc))[2] == 1
    g[3, 7] += 1
    assert _bars(_solve([g], bpc))[2] == 0
    assert _bars(_solve([f], bpc, limit=25))[1] == 1      # the limit is an option


def test_a_black_frame_among_the_samples_is_ignored():
    frames = [_boxed(40, 24, 0, 4, 0, 4, seed=1), np.full((24, 40), 16, np.uint8), _boxed(40, 24, 0, 4, 0, 4, seed=2)]
    ap = _solve(frames)
    assert _bars(ap) == [0, 4, 0, 4] and ap["frames_used"] == 2 and ap["all_dark"] is False
    # a frame that shows picture where the others have bars is not ignored: the bars shrink to what all frames share
    frames[1] = _boxed(40, 24, 0, 2, 0, 4, seed=3)
    assert _bars(_solve(frames)) == [0, 2, 0, 4]


def test_all_frames_black():
    ap = _solve([np.full((24, 40), 16, np.uint8)] * 2)
    assert ap["all_dark"] is True and ap["window"] is None and ap["frames_used"] == 0 and ap["bar_noise"] is None


def test_a_caption_line_needs_skip():
    f = _boxed(40, 24, 0, 6, 0, 6, seed=6)
    f[0, :] = 235      # a timecode line on top of the bar
    assert _bars(_solve([f])) == [0, 0, 0, 6]
    assert _bars(_solve([f], skip=1)) == [0, 6, 0, 6]
    assert _bars(_solve([_boxed(40, 24, seed=7)], skip=1)) == [0, 0, 0, 0]      # skipped lines alone are no bar


def test_columns_are_judged_on_the_active_rows_only():
    """active height H / 4; the four left picture columns are dim: 40 on the active rows, a full-height mean of 40 / 4 + 16 * 3 / 4 =
    22 <= 24 -- the full-height profile calls them dark, the profile of the active rows does not"""
    w, h = 16, 32
    f = np.full((h, w), 16, np.uint8)
    f[12:20, :] = 200
    f[12:20, :4] = 40
    _, full = R.line_profiles([f])
    assert all(int(full[0, x, 0]) <= 24 * h for x in range(4))
    ap = _solve([f])
    assert _bars(ap) == [0, 12, 0, 12] and ap["window"] == [0, 12, 16, 8]


def test_bar_noise_as_exact_fractions():
    f = _boxed(40, 24, 0, 2, 0, 2, seed=8)
    assert _solve([f])["bar_noise"] == Fraction(0)
    f[0, :], f[1, :], f[22, :], f[23, :] = 15, 17, 17, 15      # mean 16, every sample one off
    ap = _solve([f])
    assert isinstance(ap["bar_noise"], Fraction) and ap["bar_noise"] == Fraction(1)
    f[0, 0] = 19      # one sample of 160: sum 2564, squares 41152 + 136
    n = 160
    assert _solve([f])["bar_noise"] == Fraction(16 * 16 * n + n + 19 * 19 - 15 * 15, n) - Fraction(16 * n + 4, n) ** 2
    g = _boxed(40, 24, 2, 0, 0, 0, seed=9)      # a pillar bar is pooled too: its samples over the active rows
    g[:, 0], g[:, 1] = 14, 18
    assert _solve([g])["bar_noise"] == Fraction(4)


def test_argument_rules():
    from pqa2_amd import align as AL
    rows, _ = R.line_profiles([_boxed(8, 8)])
    for kw in (dict(limit=-1), dict(limit=256), dict(skip=-1)):
        with pytest.raises(ValueError):
            AL.active_picture(rows, R.cols_of([_boxed(8, 8)]), 8, **kw)


# ---- common_window ------------------------------------------------------------------------------------------------------------
def _ap(left, top, right, bottom, dark=False):
    return {"left": left, "top": top, "right": right, "bottom": bottom, "all_dark": dark}


def test_common_window_of_equal_bars():
    from pqa2_amd import align as AL
    cw = AL.common_window(_ap(0, 10, 0, 10), _ap(0, 10, 0, 10), 64, 48, 1, 1)
    assert cw == {"crop": [0, 10, 0, 10], "same": True, "mismatch": False, "scale": [1, 1], "offset": [0, 0], "reason": None}
    assert set(cw) == {"crop", "same", "mismatch", "scale", "offset", "reason"}
    none = AL.common_window(_ap(0, 0, 0, 0), _ap(0, 0, 0, 0), 64, 48, 1, 1)
    assert none["crop"] == [0, 0, 0, 0] and none["same"] and none["reason"] == "no bars"


def test_common_window_of_bars_two_lines_apart():
    from pqa2_amd import align as AL
    cw = AL.common_window(_ap(0, 10, 0, 10), _ap(0, 12, 0, 12), 64, 48, 1, 1)
    assert cw["crop"] == [0, 12, 0, 12] and cw["same"] is False and cw["mismatch"] is False and cw["reason"] is None
    assert cw["scale"] == [1, Fraction(24, 28)] and cw["offset"] == [0, 0]
    cw = AL.common_window(_ap(4, 0, 0, 0), _ap(2, 0, 2, 0), 64, 48, 0, 0)      # the inner rectangle takes the larger bar per side
    assert cw["crop"] == [4, 0, 2, 0] and cw["offset"] == [Fraction(-2), 0] and cw["scale"] == [Fraction(60, 60), 1]


def test_common_window_of_bars_forty_lines_apart():
    from pqa2_amd import align as AL
    cw = AL.common_window(_ap(0, 0, 0, 0), _ap(0, 40, 0, 0), 400, 400, 1, 1)
    assert cw["mismatch"] is True and cw["same"] is False and cw["reason"] == "windows differ" and cw["crop"] == [0, 0, 0, 0]
    assert cw["scale"] == [Fraction(1), Fraction(9, 10)] and isinstance(cw["scale"][1], Fraction)
    assert cw["offset"] == [0, Fraction(20)]
    assert AL.common_window(_ap(0, 0, 0, 0), _ap(0, 16, 0, 0), 400, 400, 1, 1)["mismatch"] is False      # the tolerance itself is a shift
    assert AL.common_window(_ap(0, 0, 0, 0), _ap(0, 17, 0, 0), 400, 400, 1, 1)["mismatch"] is True
    assert AL.common_window(_ap(0, 0, 0, 0), _ap(0, 40, 0, 0), 400, 400, 1, 1, tolerance=40)["mismatch"] is False


def test_common_window_rounds_odd_bars_up_to_the_chroma_step():
    from pqa2_amd import align as AL
    assert AL.common_window(_ap(3, 5, 1, 7), _ap(3, 5, 1, 7), 64, 48, 1, 1)["crop"] == [4, 6, 2, 8]
    assert AL.common_window(_ap(3, 5, 1, 7), _ap(3, 5, 1, 7), 64, 48, 0, 0)["crop"] == [3, 5, 1, 7]
    assert AL.common_window(_ap(3, 5, 1, 7), _ap(3, 5, 1, 7), 64, 48, 1, 0)["crop"] == [4, 5, 2, 7]


def test_common_window_reasons():
    from pqa2_amd import align as AL
    small = AL.common_window(_ap(0, 17, 0, 16), _ap(0, 17, 0, 16), 64, 48, 0, 0)
    assert small["reason"] == "window too small" and small["crop"] == [0, 17, 0, 16]
    assert AL.common_window(_ap(0, 16, 0, 16), _ap(0, 16, 0, 16), 64, 48, 0, 0)["reason"] is None      # 16 rows remain
    dark = AL.common_window(_ap(0, 0, 0, 0, dark=True), _ap(0, 4, 0, 4), 64, 48, 1, 1)
    assert dark["reason"] == "all dark" and dark["crop"] == [0, 0, 0, 0] and dark["scale"] is None and dark["offset"] is None


# ---- score_files through the oracle stand-in ---------------------------------------------------------------------------------
def _active_engine():
    from tests.fake_engine import OracleEngine

    class ActiveEngine(OracleEngine):
        """the oracle stand-in plus the restated line profiles"""

        def line_profiles(self, frames, shape=None):
            return R.line_profiles(frames, self.bpc)
    return ActiveEngine


W, H, BAR = 48, 40, 6


def _write(tmp_path, n=3):
    """a 4:2:0 pair letterboxed by BAR rows top and bottom, and the same pair cropped by hand"""
    from pqa2_amd.yuvio import VideoInfo, write_y4m
    info = VideoInfo(width=W, height=H, fps_num=24, fps_den=1, bit_depth=8, mono=False, hshift=1, vshift=1, chroma_tag="420")
    cut = VideoInfo(width=W, height=H - 2 * BAR, fps_num=24, fps_den=1, bit_depth=8, mono=False, hshift=1, vshift=1, chroma_tag="420")
    rng = np.random.default_rng(11)
    clips = {"ref": [], "dis": [], "ref_cut": [], "dis_cut": []}
    for t in range(n):
        ref = [_boxed(W, H, 0, BAR, 0, BAR, seed=20 + t)] + [np.full((H // 2, W // 2), 128, np.uint8) for _ in range(2)]
        dis = [p.copy() for p in ref]
        noise = rng.integers(-6, 7, (H - 2 * BAR, W))
        dis[0][BAR:H - BAR] = np.clip(dis[0][BAR:H - BAR].astype(int) + noise, 0, 255)
        clips["ref"].append(ref)
        clips["dis"].append(dis)
        for key, fr in (("ref_cut", ref), ("dis_cut", dis)):
            clips[key].append([fr[0][BAR:H - BAR], fr[1][BAR // 2:(H - BAR) // 2], fr[2][BAR // 2:(H - BAR) // 2]])
    paths = {}
    for key, clip in clips.items():
        paths[key] = str(tmp_path / (key + ".y4m"))
        write_y4m(paths[key], clip, cut if key.endswith("_cut") else info)
    return paths


KEYS = {"reference", "distorted", "crop", "same", "mismatch", "scale", "offset", "applied", "reason", "frames", "limit"}


def test_score_files_reports_and_crops(tmp_path):
    from pqa2_amd import report
    from pqa2_amd.pipeline import score_files
    p = _write(tmp_path)
    kw = dict(engine_factory=_active_engine())
    with pytest.raises(ValueError, match="active_picture must be"):
        score_files(p["ref"], p["dis"], "vmaf_v0.6.1", active_picture="crop", **kw)
    with pytest.raises(ValueError, match="active_frames"):
        score_files(p["ref"], p["dis"], "vmaf_v0.6.1", active_picture="report", active_frames=0, **kw)
    for bad in (-1, 256):
        with pytest.raises(ValueError, match="active_limit"):
            score_files(p["ref"], p["dis"], "vmaf_v0.6.1", active_picture="report", active_limit=bad, **kw)
    plain = score_files(p["ref"], p["dis"], "vmaf_v0.6.1", **kw)
    assert "alignment" not in plain      # without the option nothing is measured and nothing is written
    rep = score_files(p["ref"], p["dis"], "vmaf_v0.6.1", active_picture="report", **kw)
    act = rep["alignment"]["active_picture"]
    assert set(rep["alignment"]) == {"active_picture"} and set(act) == KEYS
    assert set(act["reference"]) == {"left", "top", "right", "bottom", "window", "frames_used", "all_dark", "bar_noise"}
    assert act["crop"] == [0, BAR, 0, BAR] and act["same"] is True and act["mismatch"] is False and act["applied"] is False
    assert (act["reason"], act["frames"], act["limit"], act["scale"], act["offset"]) == (None, 3, 24, [1.0, 1.0], [0.0, 0.0])
    assert act["reference"]["window"] == act["distorted"]["window"] == [0, BAR, W, H - 2 * BAR] and act["reference"]["bar_noise"] == 0.0
    assert np.array_equal(rep["records"].view(np.uint64), plain["records"].view(np.uint64))
    json.dumps(report.alignment_log_keys(rep["alignment"]))      # the object goes into the JSON log as it is
    assert "bars (left/top/right/bottom) reference 0/6/0/6" in report.active_summary_line(act)
    done = score_files(p["ref"], p["dis"], "vmaf_v0.6.1", active_picture="apply", **kw)
    assert done["alignment"]["active_picture"]["applied"] is True
    by_hand = score_files(p["ref_cut"], p["dis_cut"], "vmaf_v0.6.1", **kw)
    assert np.array_equal(done["records"].view(np.uint64), by_hand["records"].view(np.uint64))
    assert not np.array_equal(done["records"].view(np.uint64), plain["records"].view(np.uint64))
