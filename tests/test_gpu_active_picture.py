"""Active-picture detection end to end on the MI355X: synthetic 4:2:0 clips embedded in black bars go through
score_files(active_picture=) and VMAFAnalyzer; with "apply" the records are those of the same clips cropped by hand, with
"report" and with bars that disagree they are those of the uncropped pair, and the JSON object says what was found."""
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_FRAMES = 3


def _barred(frames, left, top, right, bottom):
    """the frames with black bars drawn over their edges: luma 16, chroma 128 over the chroma samples that lie wholly inside"""
    out = []
    for planes in frames:
        y, u, v = (p.copy() for p in planes)
        h, w = y.shape
        for p, val, l, t, r, b in ((y, 16, left, top, right, bottom), (u, 128, left // 2, top // 2, right // 2, bottom // 2),
                                   (v, 128, left // 2, top // 2, right // 2, bottom // 2)):
            ph, pw = p.shape
            p[:t], p[ph - b:], p[:, :l], p[:, pw - r:] = val, val, val, val
        out.append([y, u, v])
    return out


def _cut(frames, crop):
    left, top, right, bottom = crop
    out = []
    for y, u, v in frames:
        h, w = y.shape
        out.append([y[top:h - bottom, left:w - right]] + [c[top // 2:(h - bottom) // 2, left // 2:(w - right) // 2] for c in (u, v)])
    return out


def _write(path, frames):
    from pqa2_amd import synth
    from pqa2_amd.yuvio import write_y4m
    h, w = frames[0][0].shape
    write_y4m(str(path), frames, synth.clip_info(w, h))
    return str(path)


def _pair(tmp_path, w, h, ref_bars, dis_bars, crop):
    """paths of a pair with the given bars (left, top, right, bottom) and of the same pair cut by `crop` by hand"""
    from pqa2_amd import synth
    refs, diss = synth.make_clip(w, h, N_FRAMES)
    ref, dis = _barred(refs, *ref_bars), _barred(diss, *dis_bars)
    return {"ref": _write(tmp_path / "ref.y4m", ref), "dis": _write(tmp_path / "dis.y4m", dis),
            "ref_cut": _write(tmp_path / "ref_cut.y4m", _cut(ref, crop)), "dis_cut": _write(tmp_path / "dis_cut.y4m", _cut(dis, crop))}


def _same_records(a, b):
    return a["records"].shape == b["records"].shape and np.array_equal(a["records"].view(np.uint64), b["records"].view(np.uint64))


def _bars(ap):
    return [ap[k] for k in ("left", "top", "right", "bottom")]


def test_letterboxed_pair_apply_and_report(tmp_path):
    from pqa2_amd.pipeline import score_files
    bars = [4, 6, 2, 8]
    p = _pair(tmp_path, 64, 48, bars, bars, bars)
    plain = score_files(p["ref"], p["dis"], "vmaf_v0.6.1")
    by_hand = score_files(p["ref_cut"], p["dis_cut"], "vmaf_v0.6.1")
    done = score_files(p["ref"], p["dis"], "vmaf_v0.6.1", active_picture="apply")
    act = done["alignment"]["active_picture"]
    assert set(act) == {"reference", "distorted", "crop", "same", "mismatch", "scale", "offset", "applied", "reason", "frames", "limit"}
    assert _bars(act["reference"]) == bars and _bars(act["distorted"]) == bars and act["crop"] == bars
    assert act["reference"]["window"] == [4, 6, 58, 34] and act["reference"]["bar_noise"] == 0.0 and not act["reference"]["all_dark"]
    assert (act["same"], act["mismatch"], act["applied"], act["reason"], act["frames"], act["limit"]) == (True, False, True, None, N_FRAMES, 24)
    assert done["records"].shape == (N_FRAMES, 24) and _same_records(done, by_hand) and not _same_records(done, plain)
    for k in done["metrics"]:
        assert np.array_equal(np.asarray(done["metrics"][k]), np.asarray(by_hand["metrics"][k])), k
    # report mode: the same object with applied false, and the records of the uncropped clips
    rep = score_files(p["ref"], p["dis"], "vmaf_v0.6.1", active_picture="report")
    assert rep["alignment"]["active_picture"] == dict(act, applied=False)
    assert "alignment" not in plain and _same_records(rep, plain)


def test_bars_two_rows_apart_are_cropped_to_the_inner_rectangle(tmp_path):
    from pqa2_amd.pipeline import score_files
    p = _pair(tmp_path, 64, 48, [0, 6, 0, 6], [0, 8, 0, 8], [0, 8, 0, 8])
    done = score_files(p["ref"], p["dis"], "vmaf_v0.6.1", active_picture="apply")
    act = done["alignment"]["active_picture"]
    assert _bars(act["reference"]) == [0, 6, 0, 6] and _bars(act["distorted"]) == [0, 8, 0, 8]
    assert (act["crop"], act["same"], act["mismatch"], act["applied"], act["reason"]) == ([0, 8, 0, 8], False, False, True, None)
    assert act["scale"] == [1.0, 32 / 36] and act["offset"] == [0.0, 0.0]
    assert _same_records(done, score_files(p["ref_cut"], p["dis_cut"], "vmaf_v0.6.1"))


def test_bars_forty_rows_apart_are_not_cropped(tmp_path):
    from pqa2_amd.pipeline import score_files
    p = _pair(tmp_path, 200, 120, [0, 4, 0, 4], [0, 44, 0, 4], [0, 0, 0, 0])
    done = score_files(p["ref"], p["dis"], "vmaf_v0.6.1", active_picture="apply")
    act = done["alignment"]["active_picture"]
    assert _bars(act["reference"]) == [0, 4, 0, 4] and _bars(act["distorted"]) == [0, 44, 0, 4]
    assert (act["mismatch"], act["applied"], act["reason"], act["crop"]) == (True, False, "windows differ", [0, 0, 0, 0])
    assert act["scale"] == [1.0, 72 / 112] and act["offset"] == [0.0, 20.0]
    assert _same_records(done, score_files(p["ref"], p["dis"], "vmaf_v0.6.1"))


def test_odd_bars_are_rounded_up_to_the_chroma_step(tmp_path):
    from pqa2_amd.pipeline import score_files
    p = _pair(tmp_path, 64, 48, [0, 5, 0, 5], [0, 5, 0, 5], [0, 6, 0, 6])
    done = score_files(p["ref"], p["dis"], "vmaf_v0.6.1", active_picture="apply")
    act = done["alignment"]["active_picture"]
    assert _bars(act["reference"]) == _bars(act["distorted"]) == [0, 5, 0, 5] and act["crop"] == [0, 6, 0, 6] and act["applied"]
    assert _same_records(done, score_files(p["ref_cut"], p["dis_cut"], "vmaf_v0.6.1"))


def test_analyzer_crops_and_reports_the_scored_size(tmp_path):
    from pqa2_amd.pipeline import score_files
    from pqa2_amd.vmaf_analyzer import VMAFAnalyzer
    bars = [4, 6, 2, 8]
    p = _pair(tmp_path, 64, 48, bars, bars, bars)
    an = VMAFAnalyzer()
    an.set_output_directory(str(tmp_path))
    an.set_test_name("active")
    an.set_advanced_options(active_crop_enabled=True)
    lines = []
    an.status_update.connect(lines.append)
    results = an.analyze_videos(p["ref"], p["dis"])
    assert results and results["alignment"]["active_picture"]["applied"] is True
    assert (results["width"], results["height"]) == (58, 34)
    act = json.load(open(results["json_path"]))["alignment"]["active_picture"]
    assert act["crop"] == bars and act["applied"] is True and act["frames"] == N_FRAMES
    assert any("Active picture" in s and "clips cropped by 4/6/2/8 px" in s for s in lines)
    by_hand = score_files(p["ref_cut"], p["dis_cut"], "vmaf_v0.6.1")
    want = [float(v) for v in by_hand["metrics"]["vmaf"]]
    got = [fr["metrics"]["vmaf"] for fr in results["raw_results"]["frames"]]
    assert got == pytest.approx(want, abs=1e-6)     # the log is written with six decimals
    assert results["vmaf_score"] == pytest.approx(float(np.mean(want)), abs=1e-5)
