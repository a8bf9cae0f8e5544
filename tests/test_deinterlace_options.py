"""The host side of deinterlace=: the options of score_files, the CLI and the analyzer, the `input.deinterlace` object, the
reader's length, frame rate and run-independence, and field_repair -- on the CPU, with the oracle stand-in (tests/fake_engine.py)
plus the restated deinterlacer (tests/deinterlace_ref.py) as the transform."""
import io
import os

import numpy as np
import pytest

from tests import deinterlace_ref as DR
from tests import field_ref as R
from tests.test_fields import _ListReader, _field_engine, _info, _same


def _deint_engine(counter=None):
    class DeintEngine(_field_engine()):
        """the oracle stand-in plus the restated field moments and deinterlacer; counts the source frames each call is given"""

        def deinterlace(self, frames, mode="adaptive", first=0, rate="frame", shape=None):
            if counter is not None:
                counter.setdefault("calls", []).append(len(frames))
            return DR.deinterlace([np.asarray(f) for f in frames], mode, first, rate, self.bpc)
    return DeintEngine


W, H = 96, 64


def _clip_files(tmp_path):
    """16 progressive frames at 50 fps, their interlace to 8 frames tagged It, the same untagged, and the restated field clip"""
    from pqa2_amd.yuvio import write_y4m
    prog = R.moving_clip(5, 16, W, H, wobble=0)
    woven = [[DR.interlace([f[p] for f in prog], 0)[t] for p in range(3)] for t in range(8)]
    fields = [DR.deinterlace([f[p] for f in woven], "adaptive", 0, "field") for p in range(3)]
    restated = [[fields[p][k] for p in range(3)] for k in range(16)]
    P = {}
    for name, frames, info in (("ref", prog, _info(W, H, interlace="p")), ("cap", woven, _info(W, H, interlace="t")),
                               ("untagged", woven, _info(W, H)), ("restated", restated, _info(W, H, interlace="p"))):
        info = info if name in ("cap", "untagged") else __import__("dataclasses").replace(info, fps_num=50)
        P[name] = str(tmp_path / (name + ".y4m"))
        write_y4m(P[name], frames, info)
    return P, prog, woven


def test_bad_options_are_value_errors_that_name_the_option(tmp_path):
    from pqa2_amd.pipeline import score_files
    P, _, _ = _clip_files(tmp_path)
    kw = dict(engine_factory=_deint_engine(), psnr=True)
    for bad, name in ((dict(deinterlace="bob"), "deinterlace"), (dict(deinterlace="adaptive", deinterlace_rate="double"), "deinterlace_rate"),
                      (dict(deinterlace="adaptive", deinterlace_order="top"), "deinterlace_order"),
                      (dict(deinterlace="adaptive", deinterlace_side="reference"), "deinterlace_side"),
                      (dict(deinterlace_rate="double"), "deinterlace_rate")):
        with pytest.raises(ValueError, match=name):
            score_files(P["ref"], P["cap"], "vmaf_v0.6.1", **bad, **kw)
    # a clip tagged Ip (a header without a tag reads as that) names no field order
    with pytest.raises(ValueError, match="deinterlace_order"):
        score_files(P["ref"], P["untagged"], "vmaf_v0.6.1", deinterlace="adaptive", deinterlace_rate="field", **kw)
    with pytest.raises(ValueError, match="deinterlace_order"):      # both: the progressive reference has none either
        score_files(P["ref"], P["cap"], "vmaf_v0.6.1", deinterlace="adaptive", deinterlace_side="both", **kw)
    with pytest.raises(ValueError, match="field_repair"):
        score_files(P["ref"], P["cap"], "vmaf_v0.6.1", field_repair=True, **kw)


def test_score_files_deinterlaces_the_capture_and_reports_it(tmp_path):
    from pqa2_amd.pipeline import score_files
    P, _, _ = _clip_files(tmp_path)
    kw = dict(engine_factory=_deint_engine(), psnr=True, ssim=True)
    want = score_files(P["ref"], P["restated"], "vmaf_v0.6.1", **kw)
    got = score_files(P["ref"], P["cap"], "vmaf_v0.6.1", deinterlace="adaptive", deinterlace_rate="field", **kw)
    assert len(got["records"]) == 16 and _same(got, want)
    assert got["input"]["deinterlace"] == {"side": "distorted", "mode": "adaptive", "rate": "field", "order": "tff",
                                           "declared": {"reference": "p", "distorted": "t"}, "frames": [8, 16]}
    assert got["input"]["planes_scored"] == "yuv" and "input" not in want
    # the order given outright, for the untagged file; the wrong one is a different clip
    named = score_files(P["ref"], P["untagged"], "vmaf_v0.6.1", deinterlace="adaptive", deinterlace_rate="field", deinterlace_order="tff", **kw)
    assert _same(named, want) and named["input"]["deinterlace"]["declared"]["distorted"] == "p"
    wrong = score_files(P["ref"], P["cap"], "vmaf_v0.6.1", deinterlace="adaptive", deinterlace_rate="field", deinterlace_order="bff", **kw)
    assert not _same(wrong, want) and wrong["input"]["deinterlace"]["order"] == "bff"
    # worth it: the woven frames score far below the deinterlaced fields
    intra = score_files(P["ref"], P["cap"], "vmaf_v0.6.1", deinterlace="intra", deinterlace_rate="field", **kw)
    assert got["metrics"]["psnr_y"].mean() > intra["metrics"]["psnr_y"].mean()
    # rate frame: 8 frames against the first 8 of the reference
    frame = score_files(P["ref"], P["cap"], "vmaf_v0.6.1", deinterlace="adaptive", **kw)
    assert len(frame["records"]) == 8 and frame["input"]["deinterlace"]["frames"] == [8, 8]
    # off: nothing changes and no record moves
    plain = score_files(P["ref"], P["cap"], "vmaf_v0.6.1", **kw)
    off = score_files(P["ref"], P["cap"], "vmaf_v0.6.1", deinterlace=None, deinterlace_rate="field", deinterlace_order="bff", **kw)
    assert _same(off, plain) and "input" not in off
    # both sides: two interlaced files equal the two restated clips
    both = score_files(P["cap"], P["cap"], "vmaf_v0.6.1", deinterlace="adaptive", deinterlace_rate="field", deinterlace_side="both", **kw)
    assert _same(both, score_files(P["restated"], P["restated"], "vmaf_v0.6.1", **kw)) and both["input"]["deinterlace"]["side"] == "both"


@pytest.mark.parametrize("rate", DR.RATES)
def test_the_reader_is_independent_of_its_runs(rate):
    """19 frames: whatever order and run the frames are fetched in, each equals the whole-clip call's; a run reads its source
    frames and one neighbour each side"""
    from pqa2_amd.readers import _DeinterlacedReader
    frames = R.moving_clip(9, 19, 32, 16, wobble=0)
    info = _info(32, 16, interlace="b")
    whole = [DR.deinterlace([f[p] for f in frames], "adaptive", 1, rate) for p in range(3)]
    seen = {}
    rd = _DeinterlacedReader(_ListReader(frames, info), "adaptive", 1, rate, 0, _deint_engine(seen))
    per = 2 if rate == "field" else 1
    assert len(rd) == 19 * per and rd.info.fps_num == 25 * per and rd.info.fps_den == 1 and rd.info.interlace == "p"
    assert (rd.info.width, rd.info.height) == (32, 16)
    order = list(range(len(rd) - 1, -1, -1)) + [0, 17, 3, 9, 8, 16, 15, 24 % len(rd)]
    for k in order:
        got = rd.frame(k)
        assert len(got) == 3 and all(np.array_equal(got[p], whole[p][k]) for p in range(3)), k
    assert max(seen["calls"]) <= rd.RUN // per + 2      # a run's source frames plus a neighbour each side, for each plane
    rd.close()


@pytest.mark.parametrize("rate", DR.RATES)
def test_a_clip_read_front_to_back_asks_for_every_source_frame_once(rate):
    """the wrapped reader may convert in runs of its own and keep only the last: the deinterlacer's runs reach one frame across
    their ends, so it keeps its last run's source frames and asks for each frame once, in order"""
    from pqa2_amd.readers import _DeinterlacedReader
    frames = R.moving_clip(9, 19, 32, 16, wobble=0)
    asked = []

    class Counting(_ListReader):
        def frame(self, i):
            asked.append(i)
            return super().frame(i)
    rd = _DeinterlacedReader(Counting(frames, _info(32, 16, interlace="t")), "intra", 0, rate, 0, _deint_engine())
    whole = [DR.deinterlace([f[p] for f in frames], "intra", 0, rate) for p in range(3)]
    for k in range(len(rd)):
        assert all(np.array_equal(rd.frame(k)[p], whole[p][k]) for p in range(3)), k
    assert asked == list(range(19))
    rd.close()


def test_every_plane_needs_two_rows():
    """a 4:2:0 clip of height 2 has chroma planes of one row (height 3: two, rounded up): refused by name before any context is
    made"""
    from pqa2_amd.readers import _DeinterlacedReader
    made = []

    def make(*a, **kw):
        made.append(a)
        return _deint_engine()(*a, **kw)
    with pytest.raises(ValueError, match="two rows"):
        _DeinterlacedReader(_ListReader([], _info(16, 2, interlace="t")), "adaptive", 0, "frame", 0, make)
    assert not made
    for h in (3, 4):
        _DeinterlacedReader(_ListReader([], _info(16, h, interlace="t")), "adaptive", 0, "frame", 0, make).close()
    assert len(made) == 2


def test_field_repair_interpolates_a_dropped_field(tmp_path):
    from pqa2_amd.pipeline import score_files
    from pqa2_amd.yuvio import write_y4m
    ref = R.moving_clip(5, 10, W, H)
    cap = R.top_doubled(R.with_noise(ref, 105))
    planes = [DR.deinterlace([f[p] for f in cap], "intra", 0, "frame") for p in range(3)]
    repaired = [[planes[p][t] for p in range(3)] for t in range(10)]
    P = {}
    for name, frames in (("ref", ref), ("doubled", cap), ("repaired", repaired)):
        P[name] = str(tmp_path / (name + ".y4m"))
        write_y4m(P[name], frames, _info(W, H))
    kw = dict(engine_factory=_deint_engine(), psnr=True)
    today = score_files(P["ref"], P["doubled"], "vmaf_v0.6.1", field_align="apply", **kw)
    assert today["alignment"]["fields"]["kind"] == "single_field" and not today["alignment"]["fields"]["applied"]
    assert "repair" not in today["alignment"]["fields"] and _same(today, score_files(P["ref"], P["doubled"], "vmaf_v0.6.1", **kw))
    fixed = score_files(P["ref"], P["doubled"], "vmaf_v0.6.1", field_align="apply", field_repair=True, **kw)
    f = fixed["alignment"]["fields"]
    assert f["applied"] is True and f["repair"] == "intra" and f["kind"] == "single_field"
    assert _same(fixed, score_files(P["ref"], P["repaired"], "vmaf_v0.6.1", **kw))
    assert fixed["metrics"]["psnr_y"].mean() > today["metrics"]["psnr_y"].mean()
    # a progressive capture is left alone
    clean = score_files(P["ref"], P["ref"], "vmaf_v0.6.1", field_align="apply", field_repair=True, **kw)
    assert not clean["alignment"]["fields"]["applied"] and "repair" not in clean["alignment"]["fields"]


def test_score_cli_flags_reach_score_files(monkeypatch, tmp_path):
    from pqa2_amd import pipeline, score
    seen = []

    def fake(*a, **kw):
        seen.append(kw)
        raise RuntimeError("stop")

    monkeypatch.setattr(pipeline, "score_files", fake)
    monkeypatch.setattr(score, "_die_with_parent", lambda *a, **k: None)
    base = ["r.y4m", "d.y4m", "--json", str(tmp_path / "x.json")]
    score.main(base)
    score.main(base + ["--deinterlace", "adaptive"])
    score.main(base + ["--deinterlace", "intra", "--deinterlace-rate", "field", "--field-order", "bff", "--deinterlace-side", "both"])
    score.main(base + ["--deinterlace-rate", "field", "--field-order", "bff"])      # without --deinterlace nothing is passed on
    score.main(base + ["--field-correct", "--field-repair"])

    def ours(kw):
        return {k: v for k, v in kw.items() if k.startswith("deinterlace") or k == "field_repair"}
    assert ours(seen[0]) == {} and ours(seen[3]) == {}
    assert ours(seen[1]) == {"deinterlace": "adaptive", "deinterlace_rate": "frame", "deinterlace_order": None, "deinterlace_side": "distorted"}
    assert ours(seen[2]) == {"deinterlace": "intra", "deinterlace_rate": "field", "deinterlace_order": "bff", "deinterlace_side": "both"}
    assert ours(seen[4]) == {"field_repair": True} and seen[4]["field_align"] == "apply"
    with pytest.raises(SystemExit):
        score.main(base + ["--deinterlace", "bob"])


def test_analyzer_attributes_reach_the_child_argv(monkeypatch):
    from pqa2_amd import vmaf_analyzer as V
    a = V.VMAFAnalyzer()
    assert a.deinterlace_mode is None and a.deinterlace_rate is None and a.field_order is None
    assert not any(k.startswith("deinterlace") for k in a._ssim_family_kwargs())
    a.deinterlace_mode, a.deinterlace_rate, a.field_order = "adaptive", "field", "tff"
    kw = a._ssim_family_kwargs()
    assert (kw["deinterlace"], kw["deinterlace_rate"], kw["deinterlace_order"]) == ("adaptive", "field", "tff")
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
    b._run_child_job("r.y4m", "d.y4m", "vmaf_v0.6.1", "j.json", None, None, 3)
    b.deinterlace_mode = "intra"
    b._run_child_job("r.y4m", "d.y4m", "vmaf_v0.6.1", "j.json", None, None, 3)
    b.deinterlace_rate, b.field_order = "field", "bff"
    b._run_child_job("r.y4m", "d.y4m", "vmaf_v0.6.1", "j.json", None, None, 3)
    for c in cmds:
        c[c.index("--master-port") + 1] = "PORT"
    assert not any(x.startswith("--deinterlace") or x == "--field-order" for x in cmds[0])
    assert [x for x in cmds[1] if x not in cmds[0]] == ["--deinterlace", "intra", "--deinterlace-rate", "frame"]
    assert [x for x in cmds[2] if x not in cmds[0]] == ["--deinterlace", "intra", "--deinterlace-rate", "field", "--field-order", "bff"]
