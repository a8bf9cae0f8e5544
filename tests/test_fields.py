"""Field alignment on the host (pqa2_amd/fields.py, readers._WovenReader, pipeline._align_fields): the numpy restatement of the
field moments (tests/field_ref.py) against plain loops, the solver on synthetic clips with every fault it names, the weave plan
sample for sample, and score_files / the CLI / the analyzer through a numpy-backed engine stand-in.  No GPU."""
import io
import os

import numpy as np
import pytest

from tests import field_ref as R

W, H, N_FRAMES = 64, 48, 12


# ---- premises of the restatement -----------------------------------------------------------------------------------------------
def _loops(ref, dis, bits):
    top = (1 << bits) - 1
    h, w = ref[0].shape

    def E(A, p, B, q):
        s = 0
        for i in range(h // 2):
            for x in range(w):
                d = min(int(A[2 * i + p][x]), top) - min(int(B[2 * i + q][x]), top)
                s += d * d
        return s
    out = []
    for k in range(1, len(ref)):
        row = [0] * 14
        for p in (0, 1):
            for q in (0, 1):
                row[2 * p + q] = E(dis[k], p, ref[k], q)
                row[4 + 2 * p + q] = E(dis[k], p, ref[k - 1], q)
                row[8 + 2 * p + q] = E(dis[k - 1], p, ref[k], q)
        row[12] = E(dis[k], 0, dis[k], 1)
        row[13] = E(ref[k], 0, ref[k], 1)
        out.append(row)
    return out


@pytest.mark.parametrize("w,h,bits", [(5, 4, 8), (3, 5, 8), (1, 2, 8), (4, 7, 10), (2, 3, 12)])
def test_the_restatement_equals_plain_loops(w, h, bits):
    ref, dis = R.random_pairs(w * 10 + h, 3, w, h, bits, noise=50)
    if bits > 8:
        ref[1][0, 0] = 65535      # above top: read as top
        dis[2][h - 2, w - 1] = 40000
    got = R.field_moments(ref, dis, bits)
    assert got.dtype == np.uint64 and got.shape == (2, 14) and got.tolist() == _loops(ref, dis, bits)
    assert R.field_moments(ref[:1], dis[:1], bits).shape == (0, 14) and R.field_moments([], [], bits).shape == (0, 14)


def test_identical_clips_and_an_impulse():
    ref, _ = R.random_pairs(3, 3, 9, 7)
    X = R.field_moments(ref, ref)
    assert not X[:, 0].any() and not X[:, 3].any() and X[:, 1].all() and X[:, 2].all()
    assert np.array_equal(X[:, 12], X[:, 13]) and np.array_equal(X[:, 1], X[:, 2]) and np.array_equal(X[:, 1], X[:, 13])
    # the last row of an odd height counts nowhere
    dis = [f.copy() for f in ref]
    dis[1][6, 4] ^= 0x80
    assert np.array_equal(R.field_moments(ref, dis), X)
    # flat planes, one sample of D_1 on an odd row raised by 3: the words that read D_1's parity 1
    flat = [np.full((6, 8), 100, np.uint8) for _ in range(3)]
    dis = [f.copy() for f in flat]
    dis[1][3, 5] += 3
    X = R.field_moments(flat, dis)
    assert X[0].tolist() == [0, 0, 9, 9, 0, 0, 9, 9, 0, 0, 0, 0, 9, 0]      # frame 1 as D_k
    assert X[1].tolist() == [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 9, 9, 0, 0]      # frame 1 as D_{k-1}
    # ... and one sample of R_1 on an even row
    ref = [f.copy() for f in flat]
    ref[1][2, 0] += 2
    X = R.field_moments(ref, flat)
    assert X[0].tolist() == [4, 0, 4, 0, 0, 0, 0, 0, 4, 0, 4, 0, 0, 4]      # frame 1 as R_k
    assert X[1].tolist() == [0, 0, 0, 0, 4, 0, 4, 0, 0, 0, 0, 0, 0, 0]      # frame 1 as R_{k-1}


# ---- the solver ------------------------------------------------------------------------------------------------------------------
def test_the_states():
    from pqa2_amd import fields as F
    S = F.STATES
    assert len(S) == 36 and len(set(S)) == 36 and S[0] == (0, 0, 1, 0)
    assert all(q0 in (0, 1) and q1 in (0, 1) and j0 in (-1, 0, 1) and j1 in (-1, 0, 1) for q0, j0, q1, j1 in S)
    own = [s for s in S if (s[0], s[2]) == (0, 1)]
    assert S[:9] == tuple(own) and S[1:5] == ((0, -1, 1, 0), (0, 0, 1, -1), (0, 0, 1, 1), (0, 1, 1, 0))
    for part in (S[1:9], S[9:]):
        keys = [(abs(s[1]) + abs(s[3]), s) for s in part]
        assert keys == sorted(keys)
    assert S[9] == (0, 0, 0, 0)
    assert [F.kind_of(s) for s in ((0, 0, 1, 0), (0, 0, 1, -1), (0, 1, 1, 1), (1, 0, 0, 0))] == \
        ["progressive", "field_shift", "frame_offset", "field_swap"]


def _clips(seed=1, n=N_FRAMES, **kw):
    ref = R.moving_clip(seed, n, W, H, **kw)
    return ref, R.with_noise(ref, seed + 100)


def _summary(ref, cap, **kw):
    from pqa2_amd import fields as F
    X = R.field_moments(R.lumas(ref), R.lumas(cap))
    out = F.summary(X, W, H, 8, **kw)
    print({k: out[k] for k in ("kind", "state", "top", "bottom", "comb_ratio", "static", "mse_before", "mse_after")})
    return X, out


def test_frame_costs_read_the_records():
    from pqa2_amd import fields as F
    ref, cap = _clips()
    X = R.field_moments(R.lumas(ref), R.lumas(cap))
    C = F.frame_costs(X)
    assert len(C) == N_FRAMES - 2 and all(isinstance(v, int) for v in C[0][0][0])
    for t in (1, 5, N_FRAMES - 2):
        for p in (0, 1):
            for q in (0, 1):
                for j in (-1, 0, 1):
                    a, b = cap[t][0].astype(np.int64)[p::2], ref[t + j][0].astype(np.int64)[q::2]
                    assert C[t - 1][p][q][j + 1] == int(((a - b) ** 2).sum()), (t, p, q, j)
    assert F.frame_costs(X[:1]) == [] and F.frame_costs(X[:0]) == []
    with pytest.raises(ValueError):
        F.frame_costs(np.zeros((3, 7), np.uint64))


def test_a_progressive_capture():
    ref, cap = _clips()
    X, s = _summary(ref, cap)
    assert s["kind"] == "progressive" and s["state"] == [0, 0, 1, 0] and s["flips"] == 0 and not s["static"] and s["weavable"]
    assert s["segments"] == [{"first": 1, "last": N_FRAMES - 1, "state": [0, 0, 1, 0], "kind": "progressive"}]
    assert (s["top"]["parity"], s["top"]["offset"]) == (0, 0) and (s["bottom"]["parity"], s["bottom"]["offset"]) == (1, 0)
    assert s["top"]["confidence"] > 400 and s["bottom"]["confidence"] > 400
    assert s["mse_before"] == s["mse_after"] and 1.0 < s["mse_after"] < 3.0      # noise of +-2: a variance of 2


@pytest.mark.parametrize("parity,name", [(1, "bottom"), (0, "top")])
def test_a_late_field(parity, name):
    from pqa2_amd import fields as F
    ref, cap = _clips()
    X, s = _summary(ref, R.field_late(cap, parity))
    state = [0, 0, 1, -1] if parity else [0, -1, 1, 0]
    assert s["kind"] == "field_shift" and s["state"] == state and s["flips"] == 0 and s["weavable"] and not s["static"]
    assert (s[name]["parity"], s[name]["offset"]) == (parity, -1) and s[name]["confidence"] > 400
    other = "top" if parity else "bottom"
    assert (s[other]["parity"], s[other]["offset"]) == (1 - parity, 0) and s[other]["confidence"] > 400
    assert s["mse_before"] > 100 * s["mse_after"]
    assert F.segments(X, W * H, 8) == [(1, N_FRAMES - 1, tuple(state))]


def test_swapped_fields():
    ref, cap = _clips()
    _, s = _summary(ref, R.fields_swapped(cap))
    assert s["kind"] == "field_swap" and s["state"] == [1, 0, 0, 0] and s["weavable"] and s["flips"] == 0
    assert s["top"]["confidence"] > 400 and s["bottom"]["confidence"] > 400


def test_a_picture_one_line_down():
    """captured row y shows reference row y - 1: the odd rows match the even reference rows exactly, the even rows match no
    candidate.  The identity pays the one-line error on both parities, the state found on one, so the ratio that keeps the
    segment sits near 2 by construction: here row 0 keeps its own samples, the even rows so pay on 23 row pairs of 24 and the
    ratio is about 1 + 24 / 23 (the printed mse_before / mse_after: 1444.5 / 714.5 = 2.02)."""
    ref, cap = _clips()
    _, s = _summary(ref, R.line_down(cap))
    assert s["kind"] == "vertical_shift" and not s["weavable"]
    assert s["state"][0] == s["state"][2] and (s["state"][1], s["state"][3]) == (0, 0)
    assert s["comb_ratio"] > 0.5


def test_a_line_doubled_top_field():
    ref, cap = _clips()
    _, s = _summary(ref, R.top_doubled(cap))
    assert s["kind"] == "single_field" and s["state"] == [0, 0, 0, 0] and not s["weavable"]
    assert s["comb_ratio"] < 1 / 8 and s["top"]["confidence"] > 400 and s["bottom"]["confidence"] > 400


def test_a_static_clip_is_progressive_whatever_the_noise_says():
    ref, cap = _clips(step=0, wobble=0)
    _, s = _summary(ref, cap)
    assert s["kind"] == "progressive" and s["static"] and s["flips"] == 0
    _, s = _summary(ref, R.field_late(cap, 1))      # the fault is invisible: the previous frame holds the same picture
    assert s["kind"] == "progressive" and s["static"]
    assert 0.5 < s["bottom"]["confidence"] < 2.0


def test_a_field_that_turns_late():
    from pqa2_amd import fields as F
    ref = R.moving_clip(2, 24, W, H)
    cap = R.with_noise(ref, 102)
    X, s = _summary(ref, R.field_late(cap, 1, first=10))
    assert [(g["first"], g["last"], g["state"], g["kind"]) for g in s["segments"]] == \
        [(1, 10, [0, 0, 1, 0], "progressive"), (10, 23, [0, 0, 1, -1], "field_shift")]
    assert s["flips"] == 1 and s["kind"] == "field_shift" and s["weavable"]
    # a penalty no run can pay for: one state for the whole clip
    assert len(F.segments(X, W * H, 8, penalty_mse=1e9)) == 1


def test_too_few_frames_and_the_bars():
    from pqa2_amd import fields as F
    ref, cap = _clips()
    late = R.field_late(cap, 1)
    X = R.field_moments(R.lumas(ref), R.lumas(late))
    assert F.segments(X[:1], W * H) == [] and F.summary(X[:0], W, H)["kind"] == "progressive"
    assert F.summary(X[:1], W, H)["segments"] == [] and F.summary(X[:1], W, H)["mse_before"] is None
    assert F.segments(X, W * H, 8, min_improvement=1e9) == [(1, N_FRAMES - 1, (0, 0, 1, 0))]      # nothing improves that much
    import json
    json.dumps(F.summary(X, W, H))


# ---- the weave -----------------------------------------------------------------------------------------------------------------
class _ListReader:
    def __init__(self, frames, info):
        self.frames, self.info = frames, info

    def __len__(self):
        return len(self.frames)

    def frame(self, i):
        return self.frames[i]


def _info(w=W, h=H, **kw):
    from pqa2_amd.yuvio import VideoInfo
    return VideoInfo(width=w, height=h, fps_num=25, fps_den=1, bit_depth=8, mono=False, hshift=1, vshift=1, chroma_tag="420", **kw)


def _woven(ref, faulty):
    from pqa2_amd import fields as F
    from pqa2_amd.readers import _WovenReader
    X = R.field_moments(R.lumas(ref), R.lumas(faulty))
    plan = F.weave_plan(F.segments(X, W * H, 8), len(faulty))
    rd = _WovenReader(_ListReader(faulty, _info()), plan)
    assert len(rd) == plan["u_hi"] - plan["u_lo"] == len(plan["sources"])
    return plan, rd


@pytest.mark.parametrize("fault,u_lo,u_hi", [("bottom", 0, 11), ("top", 0, 11), ("swap", 0, 12), ("none", 0, 12)])
def test_the_woven_clip_is_the_progressive_capture(fault, u_lo, u_hi):
    ref, cap = _clips()
    faulty = {"bottom": lambda: R.field_late(cap, 1), "top": lambda: R.field_late(cap, 0), "swap": lambda: R.fields_swapped(cap),
              "none": lambda: cap}[fault]()
    plan, rd = _woven(ref, faulty)
    assert (plan["u_lo"], plan["u_hi"], plan["unfilled"]) == (u_lo, u_hi, [])
    for i in range(len(rd)):
        for p in range(3):
            assert np.array_equal(rd.frame(i)[p], cap[u_lo + i][p]), (i, p)
    if fault == "none":
        assert rd.frame(3) is cap[3]      # nothing to move: the frame itself


def test_the_weave_across_a_flip():
    """the bottom field turns late at frame 10: output frame 9 has no bottom field anywhere (captured frame 10 shows that of
    frame 9 -- it does: t + j = 10 - 1), so nothing is lost here; when it turns back, a field is shown twice and one is lost"""
    from pqa2_amd import fields as F
    ref = R.moving_clip(2, 24, W, H)
    cap = R.with_noise(ref, 102)
    plan, rd = _woven(ref, R.field_late(cap, 1, first=10))
    assert (plan["u_lo"], plan["u_hi"]) == (0, 23)
    assert plan["unfilled"] == []      # frame 9's bottom field arrives twice (frames 9 and 10): the earlier wins
    assert plan["sources"][9] == ((9, 0), (9, 1)) and plan["sources"][10] == ((10, 0), (11, 1))
    for i in range(len(rd)):
        for p in range(3):
            assert np.array_equal(rd.frame(i)[p], cap[i][p]), (i, p)
    # late first, then on time: the bottom field of frame 9 is shown by nobody
    back = F.weave_plan([(1, 10, (0, 0, 1, -1)), (10, 23, (0, 0, 1, 0))], 24)
    assert back["unfilled"] == [(9, 1)] and back["sources"][9] == ((9, 0), (9, 1)) and (back["u_lo"], back["u_hi"]) == (0, 24)
    assert F.weave_plan([], 5) == {"u_lo": 0, "u_hi": 5, "sources": [((u, 0), (u, 1)) for u in range(5)], "unfilled": []}
    ahead = F.weave_plan([(1, 4, (0, 1, 1, 0))], 5)      # the top field shows the NEXT frame
    assert (ahead["u_lo"], ahead["u_hi"]) == (1, 5) and ahead["sources"][0] == ((0, 0), (1, 1))


def test_the_weave_of_an_odd_height():
    from pqa2_amd.readers import _WovenReader
    rng = np.random.default_rng(4)
    frames = [[rng.integers(0, 256, (7, 6)).astype(np.uint8)] for _ in range(3)]
    rd = _WovenReader(_ListReader(frames, _info(6, 7)), {"u_lo": 0, "u_hi": 3, "sources": [((u, 1), (u, 0)) for u in range(3)],
                                                          "unfilled": []})
    got = rd.frame(1)[0]
    assert np.array_equal(got[0:6:2], frames[1][0][1::2]) and np.array_equal(got[1::2], frames[1][0][0:6:2])
    assert np.array_equal(got[6], frames[1][0][6])      # the row without a partner stays


# ---- score_files through the oracle stand-in -----------------------------------------------------------------------------------
def _field_engine(counter=None):
    from tests.fake_engine import OracleEngine

    class FieldEngine(OracleEngine):
        """the oracle stand-in plus the restated field moments; counts the frames they are given"""

        def field_moments(self, ref_frames, dis_frames, shape=None):
            if counter is not None:
                counter.setdefault("calls", []).append(len(ref_frames))
            return R.field_moments(list(ref_frames), list(dis_frames), self.bpc)
    return FieldEngine


SW, SH, SN = 96, 64, 10


def _write(tmp_path, interlace=None):
    from pqa2_amd.yuvio import write_y4m
    info = _info(SW, SH, interlace=interlace)
    ref = R.moving_clip(5, SN, SW, SH)
    cap = R.with_noise(ref, 105)
    paths = {}
    for name, frames in (("ref", ref), ("cap", cap), ("late", R.field_late(cap, 1)), ("doubled", R.top_doubled(cap)),
                         ("cap_from", cap)):
        paths[name] = str(tmp_path / (name + ".y4m"))
        write_y4m(paths[name], frames, info)
    return paths


def _same(a, b):
    return np.array_equal(a["records"].view(np.uint64), b["records"].view(np.uint64)) and \
        list(a["metrics"]) == list(b["metrics"]) and all(np.array_equal(a["metrics"][k], b["metrics"][k]) for k in a["metrics"])


def test_score_files_off_report_and_apply(tmp_path):
    from pqa2_amd.pipeline import score_files
    P = _write(tmp_path, interlace="t")
    kw = dict(engine_factory=_field_engine(), psnr=True)
    for bad in ("on", True, 1):
        with pytest.raises(ValueError, match="field_align"):
            score_files(P["ref"], P["late"], "vmaf_v0.6.1", field_align=bad, **kw)
    with pytest.raises(ValueError, match="field_frames"):
        score_files(P["ref"], P["late"], "vmaf_v0.6.1", field_align="report", field_frames=2, **kw)
    with pytest.raises(ValueError, match="field_penalty_mse"):
        score_files(P["ref"], P["late"], "vmaf_v0.6.1", field_align="report", field_penalty_mse=-1.0, **kw)

    plain = score_files(P["ref"], P["late"], "vmaf_v0.6.1", **kw)
    assert "alignment" not in plain
    off = score_files(P["ref"], P["late"], "vmaf_v0.6.1", field_align=None, field_frames=5, **kw)
    assert _same(off, plain) and "alignment" not in off
    seen = {}
    rep = score_files(P["ref"], P["late"], "vmaf_v0.6.1", field_align="report", engine_factory=_field_engine(seen), psnr=True)
    assert _same(rep, plain) and seen["calls"] == [SN]
    f = rep["alignment"]["fields"]
    assert f["kind"] == "field_shift" and f["state"] == [0, 0, 1, -1] and f["weavable"] and not f["applied"] and f["reason"] == "report"
    assert (f["frames"], f["transitions"]) == (SN, SN - 1) and f["declared"] == {"reference": "t", "distorted": "t"}
    assert (f["bottom"]["parity"], f["bottom"]["offset"]) == (1, -1)

    good = score_files(P["ref"], P["cap"], "vmaf_v0.6.1", **kw)
    fixed = score_files(P["ref"], P["late"], "vmaf_v0.6.1", field_align="apply", **kw)
    f = fixed["alignment"]["fields"]
    assert f["applied"] and f["reason"] is None and (f["u_lo"], f["u_hi"], f["unfilled"]) == (0, SN - 1, [])
    assert len(fixed["records"]) == SN - 1
    assert np.array_equal(fixed["records"].view(np.uint64), good["records"][:SN - 1].view(np.uint64))
    # the metrics too, up to the last frame: motion2 there looks at a successor that the shorter clip does not have
    assert all(np.array_equal(fixed["metrics"][k][:SN - 2], good["metrics"][k][:SN - 2]) for k in good["metrics"])
    assert fixed["metrics"]["psnr_y"].mean() > plain["metrics"]["psnr_y"].mean() + 10

    # a measurement on the first frames only still weaves the whole clip
    part = score_files(P["ref"], P["late"], "vmaf_v0.6.1", field_align="apply", field_frames=5, **kw)
    assert part["alignment"]["fields"]["frames"] == 5 and _same(part, fixed)
    # nothing to undo, and a fault that cannot be undone: reported, the records untouched
    same = score_files(P["ref"], P["cap"], "vmaf_v0.6.1", field_align="apply", **kw)
    assert _same(same, good) and same["alignment"]["fields"]["reason"] == "progressive" and not same["alignment"]["fields"]["applied"]
    dbl = score_files(P["ref"], P["doubled"], "vmaf_v0.6.1", field_align="apply", **kw)
    assert dbl["alignment"]["fields"]["kind"] == "single_field" and dbl["alignment"]["fields"]["reason"] == "not weavable"
    assert _same(dbl, score_files(P["ref"], P["doubled"], "vmaf_v0.6.1", **kw))


def test_the_measurement_runs_in_calls_of_65_frames(monkeypatch):
    from pqa2_amd import pipeline
    ref = [[np.full((4, 4), t % 7, np.uint8)] for t in range(140)]
    info = _info(4, 4)
    seen = {}
    out, plan = pipeline._find_fields(_ListReader(ref, info), _ListReader(ref, info), None, None, True, 0, _field_engine(seen))
    assert seen["calls"] == [65, 65, 12] and out["transitions"] == 139 and out["frames"] == 140 and plan is None
    seen.clear()
    pipeline._find_fields(_ListReader(ref, info), _ListReader(ref, info), 65, None, False, 0, _field_engine(seen))
    assert seen["calls"] == [65]
    seen.clear()
    out, _ = pipeline._find_fields(_ListReader(ref[:2], info), _ListReader(ref[:2], info), None, None, True, 0, _field_engine(seen))
    assert seen["calls"] == [2] and out["reason"] == "too few frames" and not out["applied"]


# ---- CLI, analyzer, Y4M --------------------------------------------------------------------------------------------------------
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
    score.main(base + ["--field-align"])
    score.main(base + ["--field-correct", "--field-frames", "40", "--field-penalty-mse", "12.5"])
    score.main(base + ["--field-frames", "40"])      # without --field-align nothing is passed on
    assert not any(k.startswith("field") for k in seen[0]) and not any(k.startswith("field") for k in seen[3])
    assert {k: v for k, v in seen[1].items() if k.startswith("field")} == {"field_align": "report", "field_frames": None,
                                                                            "field_penalty_mse": None}
    assert {k: v for k, v in seen[2].items() if k.startswith("field")} == {"field_align": "apply", "field_frames": 40,
                                                                            "field_penalty_mse": 12.5}


def test_analyzer_attributes_reach_the_child_argv(tmp_path, monkeypatch):
    from pqa2_amd import vmaf_analyzer as V
    a = V.VMAFAnalyzer()
    assert a.field_align_enabled is False and a.field_correct_enabled is False
    assert "field_align" not in a._ssim_family_kwargs()
    a.field_align_enabled = True
    assert a._ssim_family_kwargs()["field_align"] == "report"
    a.field_correct_enabled = True
    assert a._ssim_family_kwargs()["field_align"] == "apply"

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
    b.field_align_enabled = True
    b._run_child_job("r.y4m", "d.y4m", "vmaf_v0.6.1", "j.json", None, None, 3)
    b.field_correct_enabled = True
    b._run_child_job("r.y4m", "d.y4m", "vmaf_v0.6.1", "j.json", None, None, 3)
    for c in cmds:
        c[c.index("--master-port") + 1] = "PORT"
    assert not any(x.startswith("--field") for x in cmds[0])
    assert [x for x in cmds[1] if x not in cmds[0]] == ["--field-align"] and [x for x in cmds[2] if x not in cmds[0]] == ["--field-correct"]


def test_the_y4m_interlace_tag_round_trips(tmp_path):
    from pqa2_amd.yuvio import Y4MReader, VideoInfo, write_y4m
    frames = [[np.zeros((4, 4), np.uint8), np.zeros((2, 2), np.uint8), np.zeros((2, 2), np.uint8)]]
    assert [f.name for f in __import__("dataclasses").fields(VideoInfo)][-1] == "interlace"
    heads = {}
    for tag in (None, "p", "t", "b", "m"):
        path = str(tmp_path / f"{tag}.y4m")
        write_y4m(path, frames, _info(4, 4, interlace=tag))
        heads[tag] = open(path, "rb").readline()
        assert Y4MReader(path).info.interlace == (tag or "p")
        assert f" I{tag or 'p'} ".encode() in heads[tag]
    assert heads[None] == heads["p"] == b"YUV4MPEG2 W4 H4 F25:1 Ip A1:1 C420\n"      # today's bytes
    bare = str(tmp_path / "bare.y4m")
    with open(bare, "wb") as f:
        f.write(b"YUV4MPEG2 W4 H4 F25:1 C420\nFRAME\n" + bytes(24))
    rd = Y4MReader(bare)
    assert rd.info.interlace is None and len(rd) == 1 and (rd.info.width, rd.info.height, rd.info.chroma_tag) == (4, 4, "420")
