"""Capture integrity (FFmpeg freezedetect / blackdetect / scdet, PQA_FEAT_INTEGRITY) without a device: the ABI additions,
the host state machines (pqa2_amd/integrity.py) against hand-built rows with the expected events written out, the numpy
restatement (tests/integrity_ref.py) against closed forms, and the pipeline / JSON / log plumbing through an engine
stand-in that serves rows from the restatement."""
import ctypes as C
import io
import json
import os
import re

import numpy as np
import pytest

from tests import integrity_ref as R
from tests.fake_engine import OracleEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FUNCS = ("pqa_ext5_doubles", "pqa_collect_ext5", "pqa_set_black_threshold", "pqa_set_dis_history_planes", "pqa_frame_sad",
             "pqa_frame_sad_device")
COLS = ("scd_mafd", "scd_score", "black_ratio", "freeze_mafd")


# ---- 1. header, binding, doc ----------------------------------------------------------------------------------------------
def test_header_binding_and_doc_agree():
    from pqa2_amd import _native as N
    hdr = open(os.path.join(ROOT, "include", "pqa_vmaf.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert re.search(r"PQA_FEAT_INTEGRITY\s*=\s*1u\s*<<\s*17", hdr) and N.FEAT_INTEGRITY == 1 << 17
    assert N.FEAT_KNOWN & N.FEAT_INTEGRITY and N.FEAT_ALL == 31 and not N.FEAT_KNOWN & 128
    known = hdr[hdr.index("PQA_FEAT_KNOWN ="):hdr.index("what pqa_create accepts")]
    assert "PQA_FEAT_INTEGRITY" in known
    for name, val in (("PQA_EXT5_SAD_PREV", N.EXT5_SAD_PREV), ("PQA_EXT5_BLACK_COUNT", N.EXT5_BLACK_COUNT),
                      ("PQA_EXT5_RESERVED", N.EXT5_RESERVED), ("PQA_EXT5_DOUBLES", N.EXT5_DOUBLES)):
        assert int(re.search(name + r"\s*=\s*(\d+)", hdr).group(1)) == val
    assert (N.EXT5_SAD_PREV, N.EXT5_BLACK_COUNT, N.EXT5_RESERVED, N.EXT5_DOUBLES) == (0, 3, 4, 8) == (0, 3, 4, R.EXT5_DOUBLES)
    for f in NEW_FUNCS:
        assert re.search(r"PQA_API\s+int\s+" + f + r"\s*\(", hdr), f
        assert f in N.EXPORTS, f
    for f in ("pqa_collect_ext5", "pqa_set_black_threshold", "pqa_set_dis_history_planes", "pqa_frame_sad"):
        assert f"lib.{f}.argtypes" in doc, f
    assert "131072" in doc and "integrity_enabled" in doc
    assert "integrity continuity state" in hdr[hdr.index("PQA_API int pqa_reset") - 200:hdr.index("PQA_API int pqa_reset")]
    assert re.search(r"PQA_PROF_KERNELS\s*=\s*17", hdr) and N.PROF_KERNELS == 17


def test_library_takes_the_bit_without_a_device():
    import torch
    from pqa2_amd import _native as N
    lib = N.load()
    assert lib.pqa_ext5_doubles() == 8
    for f in NEW_FUNCS:
        assert hasattr(lib, f)

    def create(features, n_planes=3):
        cfg = N.PqaConfig()
        lib.pqa_config_init(C.byref(cfg), 64, 48)
        cfg.features, cfg.n_planes = features, n_planes
        ctx = C.c_void_p()
        rc = lib.pqa_create(C.byref(cfg), C.byref(ctx))
        msg = (lib.pqa_last_error(None) or b"").decode()
        if ctx.value:
            lib.pqa_destroy(ctx)
        return rc, msg
    rc, msg = create(N.FEAT_VMAF | 128)
    assert rc == N.PQA_EINVAL and "feature mask" in msg          # bit 7 is still unknown
    rc, msg = create(N.FEAT_VMAF | (1 << 18))
    assert rc == N.PQA_EINVAL and "feature mask" in msg
    for feats, npl in ((N.FEAT_INTEGRITY, 3), (N.FEAT_INTEGRITY, 1), (N.FEAT_VMAF | N.FEAT_INTEGRITY, 3)):
        rc, msg = create(feats, npl)
        assert "feature mask" not in msg
        assert rc == (N.PQA_OK if torch.cuda.is_available() else N.PQA_EDEVICE), msg
    assert lib.pqa_set_black_threshold(None, 37) == N.PQA_EINVAL
    assert lib.pqa_set_dis_history_planes(None, None, None) == N.PQA_EINVAL
    assert lib.pqa_frame_sad(None, None, None, None, None, 0, None) == N.PQA_EINVAL
    assert lib.pqa_frame_sad_device(None, None, None, None, 0, None) == N.PQA_EINVAL


# ---- 2. the state machines against hand-built rows ----------------------------------------------------------------------------
def test_drift_moves_the_anchor_and_never_freezes():
    """64 x 48, 8 bit, 4:2:0: 4 608 samples, noise 0.001 -> still when the SAD against the anchor is <= 1 179.  Every frame
    raises 1 000 further luma samples by 1: each sad_prev is 1 000, against a frame two back it is 2 000."""
    from pqa2_amd import integrity as IG
    n = 12
    total = 64 * 48 + 2 * 32 * 24
    assert total == 4608 and int(0.001 * total * 256) == 1179
    luma = np.full(64 * 48, 100, np.int64)
    frames = []
    for j in range(n):
        if j:
            luma = luma.copy()
            luma[(np.arange(1000) + (j - 1) * 1000) % luma.size] += 1
        frames.append([luma.reshape(48, 64).astype(np.uint8), np.full((24, 32), 128, np.uint8), np.full((24, 32), 128, np.uint8)])
    rows = R.rows(frames, 37)
    assert (rows[1:, 0] == 1000).all() and (rows[1:, 1:3] == 0).all() and np.isnan(rows[0, :3]).all()
    asked = []

    def cb(anchor, i):
        asked.append((anchor, i))
        return R.frame_sad(frames[anchor], [frames[i]])[0]
    mafd, anchor, freezes = IG.freezedetect(rows[:, :3], [3072, 768, 768], 8, 25, 1, 0.001, 0.08, cb)
    assert list(anchor) == [0, 0, 0, 2, 2, 4, 4, 6, 6, 8, 8, 10]
    assert freezes == []
    assert asked == [(0, 2), (2, 4), (4, 6), (6, 8), (8, 10)]
    want = [0.0] + [(1000 if i % 2 else 2000) / 4608 / 256 for i in range(1, n)]
    assert list(mafd) == want
    # a previous-frame rule would have called every frame still and reported one long freeze
    prev_rule_still = rows[1:, :3].sum(1) / 4608 / 256 <= 0.001
    assert prev_rule_still.all()
    # the brute-force restatement agrees
    rm, ra, rf = R.freezedetect(frames, 8, 0.001, 0.08)
    assert list(ra) == list(anchor) and rf == [] and np.array_equal(rm, mafd)


def _moving_rows(n, still, moving=(80000.0, 10000.0, 10000.0)):
    rows = np.full((n, 8), np.nan)
    rows[1:, :3] = moving
    rows[:, 3] = 0.0
    for i in still:
        rows[i, :3] = 0.0
    return rows


def test_a_three_second_freeze_inside_moving_content():
    from pqa2_amd import integrity as IG
    n = 150
    rows = _moving_rows(n, range(41, 115))     # frames 41..114 repeat frame 40; frame 115 moves: 75 frames = 3 s at 25 fps
    asked = []

    def cb(anchor, i):
        asked.append((anchor, i))
        return 0.0 if i <= 114 else 100000.0
    sizes = [64 * 48, 32 * 24, 32 * 24]      # 4 608 samples: a moving frame's 100 000 is mafd 0.085, far above the noise
    mafd, anchor, freezes = IG.freezedetect(rows[:, :3], sizes, 8, 25, 1, 0.001, 2.0, cb)
    assert freezes == [{"start": 1.6, "end": 4.6, "duration": 3.0, "first_frame": 40, "last_frame": 114}]
    assert asked == [(40, i) for i in range(42, 116)]
    assert list(anchor[40:117]) == [39] + [40] * 75 + [115]
    # the duration option's boundary: the last still frame is 74 frames = 2.96 s after the anchor; >= holds exactly there
    assert len(IG.freezedetect(rows[:, :3], sizes, 8, 25, 1, 0.001, 2.96, cb)[2]) == 1
    assert IG.freezedetect(rows[:, :3], sizes, 8, 25, 1, 0.001, 2.97, cb)[2] == []
    assert IG.freezedetect(rows[:, :3], sizes, 8, 25, 1, 0.001, 3.0, cb)[2] == []
    # NTSC rate: 60 frames at 30000 / 1001 are 2.002 s
    got = IG.freezedetect(_moving_rows(100, range(11, 71))[:, :3], sizes, 8, 30000, 1001, 0.001, 2.0, lambda a, i: 0.0 if i <= 70 else 1e5)[2]
    assert got == [{"start": 10 * 1001 / 30000, "end": 71 * 1001 / 30000, "duration": 61 * 1001 / 30000, "first_frame": 10,
                    "last_frame": 70}]


def test_a_freeze_open_at_the_end_of_the_clip():
    from pqa2_amd import integrity as IG
    rows = _moving_rows(100, range(31, 100))
    freezes = IG.freezedetect(rows[:, :3], [3072, 768, 768], 8, 25, 1, 0.001, 2.0, lambda a, i: 0.0)[2]
    assert freezes == [{"start": 1.2, "end": None, "duration": None, "first_frame": 30, "last_frame": 99}]
    res = {"freezes": freezes}
    assert IG.log_lines(res) == ["freeze_start: 1.2"]


def test_a_freeze_across_shard_boundaries_gives_the_same_result():
    from pqa2_amd import integrity as IG
    from pqa2_amd import shard
    rng = np.random.default_rng(3)
    n = 30
    frames = [[rng.integers(16, 236, (16, 16)).astype(np.uint8), rng.integers(16, 240, (8, 8)).astype(np.uint8),
               rng.integers(16, 240, (8, 8)).astype(np.uint8)] for _ in range(n)]
    for i in range(9, 23):          # frames 8..22 are one picture: it spans the boundaries of 2 and of 3 shards
        frames[i] = [p.copy() for p in frames[8]]
    results = []
    for ranks in (1, 2, 3):
        parts = []
        for r in range(ranks):
            a, b = shard.shard_bounds(n, ranks, r)
            parts.append(R.rows(frames[a:b], 37, prev=frames[a - 1] if a else None))
        rows = np.concatenate(parts)
        results.append(IG.analyze(rows[:, :3], rows[:, 3], width=16, height=16, plane_sizes=[(16, 16), (8, 8), (8, 8)],
                                  bit_depth=8, fps_num=25, fps_den=1, opts={"freeze_duration": 0.4},
                                  anchored_sad=lambda a, i: R.frame_sad(frames[a], [frames[i]])[0]))
    assert results[0]["freezes"] == [{"start": 0.32, "end": 0.92, "duration": 0.6, "first_frame": 8, "last_frame": 22}]
    for res in results[1:]:
        assert res["freezes"] == results[0]["freezes"] and res["scene_changes"] == results[0]["scene_changes"]
        for k in COLS:
            assert np.array_equal(res["columns"][k], results[0]["columns"][k]), k
        assert np.array_equal(res["freeze_anchor"], results[0]["freeze_anchor"])


def test_blackdetect_runs_and_thresholds():
    from pqa2_amd import integrity as IG
    wh = 64 * 48

    def run(black_frames, n=100, **kw):
        cnt = np.zeros(n)
        cnt[list(black_frames)] = wh
        return IG.blackdetect(cnt, 64, 48, 25, 1, **kw)
    ratio, ev = run(range(10, 60))                     # 50 frames, first non-black frame 60: exactly 2.0 s
    assert ev == [{"start": 0.4, "end": 2.4, "duration": 2.0, "first_frame": 10, "last_frame": 59}]
    assert ratio[10] == 1.0 and ratio[9] == 0.0
    assert run(range(10, 59))[1] == []                 # a frame shorter: 1.96 s
    assert run(range(40, 100))[1] == [{"start": 1.6, "end": 3.96, "duration": 2.36, "first_frame": 40, "last_frame": 99}]
    assert run(range(51, 100))[1] == []                # open at the end, 1.92 s to the last frame's pts
    # picture_black_ratio_th: >= at the boundary
    cnt = np.full(60, 0.98 * 100 * 100)
    assert len(IG.blackdetect(cnt, 100, 100, 25, 1)[1]) == 1 and IG.blackdetect(cnt - 1, 100, 100, 25, 1)[1] == []
    assert (IG.black_threshold(8), IG.black_threshold(8, True), IG.black_threshold(10)) == (37, 25, 151)
    assert (R.black_threshold(8), R.black_threshold(8, True), R.black_threshold(10)) == (37, 25, 151)
    assert (IG.black_threshold(12), IG.black_threshold(10, True), IG.black_threshold(8, False, 0.0)) == (606, 102, 16)
    assert IG.log_lines({"blacks": run(range(0, 13), black_min_duration=0.5)[1]}) == ["black_start:0 black_end:0.52 black_duration:0.52"]


def test_scdet_scores():
    from pqa2_amd import integrity as IG
    wh = 64 * 48
    sad = np.zeros(10)
    sad[0] = np.nan
    sad[5] = wh * 64          # a hard cut in static content: mafd 25
    sad[6] = wh * 16          # the frame after it: mafd 6.25
    mafd, score, ev = IG.scdet(sad, 64, 48, 8, 25, 1, 10.0)
    assert list(mafd) == [0, 0, 0, 0, 0, 25.0, 6.25, 0, 0, 0]
    assert list(score) == [0, 0, 0, 0, 0, 25.0, 6.25, 0, 0, 0]      # min(25, |25 - 0|), min(6.25, |6.25 - 25|)
    assert ev == [{"frame": 5, "time": 0.2, "score": 25.0}]
    sad[0] = 12345.0         # whatever a shard's armed history puts into row 0: frame 0 has mafd 0 and score 0
    assert IG.scdet(sad, 64, 48, 8, 25, 1)[1][0] == 0.0 and IG.scdet(sad, 64, 48, 8, 25, 1)[0][0] == 0.0
    big = np.array([np.nan, wh * 384.0, 0.0])       # beyond any real sample range: the clip at 100
    mafd, score, ev = IG.scdet(big, 64, 48, 8, 25, 1)
    assert mafd[1] == 150.0 and score[1] == 100.0 and score[2] == 0.0
    assert IG.scdet(sad, 64, 48, 8, 25, 1, 25.0)[2] == ev[:0] + [{"frame": 5, "time": 0.2, "score": 25.0}]   # >= threshold
    assert IG.scdet(sad, 64, 48, 8, 25, 1, 25.01)[2] == []
    assert IG.scdet(sad, 64, 48, 10, 25, 1)[0][5] == 6.25            # the divisor is 2^bpc
    assert IG.log_lines({"scene_changes": [{"frame": 80, "time": 3.2, "score": 25.0}]}) == ["lavfi.scd.score: 25.000, lavfi.scd.time: 3.2"]


def test_options_have_ffmpegs_names_and_defaults():
    from pqa2_amd import integrity as IG
    assert IG.DEFAULTS == {"freeze_noise": 0.001, "freeze_duration": 2.0, "black_min_duration": 2.0,
                           "picture_black_ratio_th": 0.98, "pixel_black_th": 0.10, "scd_threshold": 10.0}
    assert IG.options({"scd_threshold": 5})["scd_threshold"] == 5.0 and IG.options(None) == IG.DEFAULTS
    with pytest.raises(ValueError):
        IG.options({"noise": 1})


# ---- 3. the restatement against closed forms ------------------------------------------------------------------------------------
@pytest.mark.parametrize("bpc,c", [(8, 3), (10, 17), (12, 255)])
def test_restatement_closed_forms(bpc, c):
    dt = np.uint8 if bpc == 8 else np.uint16
    w, h = 40, 22
    rng = np.random.default_rng(bpc)
    top = (1 << bpc) - 1
    a = [rng.integers(0, top - c + 1, s).astype(dt) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2))]
    b = [(p + c).astype(dt) for p in a]
    rows = R.rows([a, b, a], 37)
    assert list(rows[1, :3]) == [c * w * h, c * w * h // 4, c * w * h // 4] == list(rows[2, :3])
    assert np.isnan(rows[0, :3]).all() and np.isnan(rows[:, 4:]).all()
    assert np.array_equal(R.frame_sad(a, [a, b]), np.array([[0, 0, 0], [c * w * h, c * w * h // 4, c * w * h // 4]], np.uint64))
    f = 1 << (bpc - 8)
    black = [np.full((h, w), 16 * f, dt)]
    assert R.rows([black], R.black_threshold(bpc))[0, 3] == w * h and R.rows([black], 16 * f - 1)[0, 3] == 0
    if bpc == 8:
        assert R.rows([black], 37)[0, 3] == w * h and R.rows([black], 15)[0, 3] == 0
    lo, hi = [np.zeros((h, w), dt)], [np.full((h, w), top, dt)]
    assert R.rows([lo, hi], 0)[1, 0] == top * w * h and R.rows([lo, hi], 0, n_planes=1)[1, 3] == 0
    assert np.isnan(R.rows([lo, hi], 0)[1, 1:3]).all()


def test_fault_clip_figures():
    """The figures the pipeline tests (here and on the GPU) write out: black -> content 29.4921875, content 1.513671875,
    the hard cut 35.15625 (score 33.642578125)."""
    refs, diss = R.fault_clip(5, 10, 30, 5, 5)
    mafd, score, ev = R.scdet(diss, 8)
    assert mafd[5] == 29.4921875 and mafd[6] == 1.513671875 and mafd[50] == 35.15625 and mafd[45] == 2.9296875
    assert ev == [(5, 29.4921875), (50, 33.642578125)]
    assert R.freezedetect(diss, 8, duration=0.4)[2] == [(15, 45)]
    assert R.blackdetect(diss, 37, min_duration=0.2)[1] == [(0, 5)]


# ---- 4. pipeline plumbing -----------------------------------------------------------------------------------------------------------
class IntegrityEngine(OracleEngine):
    """OracleEngine plus the fifth extension record and the anchored SADs, served from the restatement."""
    made = []

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.dis, self.prev, self.thr, self.history_calls, self.sad_calls = {}, None, None, [], []
        IntegrityEngine.made.append(self)

    def set_black_threshold(self, thr):
        self.thr = int(thr)

    def set_dis_history_planes(self, planes):
        self.history_calls.append(planes is not None)
        self.prev = None if planes is None else [np.array(p) for p in planes]

    def submit(self, index, ref_planes, dis_planes):
        super().submit(index, ref_planes, dis_planes)
        self.dis[index] = [np.array(p) for p in dis_planes]

    def collect_blocks(self, first, count, blocks):
        got = self.collect_ext5(first, count)
        return got[0], {i: got[1 + i] for i in blocks}

    def collect_ext5(self, first, count):
        from pqa2_amd import _native as N
        assert self.features & N.FEAT_INTEGRITY and self.thr is not None
        ext5 = R.rows([self.dis[first + j] for j in range(count)], self.thr, prev=self.prev, n_planes=self.n_planes)
        nan = lambda wd: np.full((count, wd), np.nan)
        return self.collect(first, count), nan(N.EXT_DOUBLES), nan(N.EXT2_DOUBLES), nan(N.EXT3_DOUBLES), nan(N.EXT4_DOUBLES), ext5

    def frame_sad(self, anchor, frames):
        self.sad_calls.append(len(frames))
        return R.frame_sad(anchor, frames, self.n_planes)


OPTS = {"freeze_duration": 0.4, "black_min_duration": 0.2}
WANT = {"freezes": [{"start": 0.6, "end": 1.8, "duration": 1.2, "first_frame": 15, "last_frame": 44}],
        "blacks": [{"start": 0.0, "end": 0.2, "duration": 0.2, "first_frame": 0, "last_frame": 4}],
        "scene_changes": [{"frame": 5, "time": 0.2, "score": 29.4921875}, {"frame": 50, "time": 2.0, "score": 33.642578125}]}
WANT_LINES = ["black_start:0 black_end:0.2 black_duration:0.2", "lavfi.scd.score: 29.492, lavfi.scd.time: 0.2",
              "freeze_start: 0.6", "freeze_duration: 1.2", "freeze_end: 1.8", "lavfi.scd.score: 33.643, lavfi.scd.time: 2"]


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    from pqa2_amd import synth, yuvio
    d = tmp_path_factory.mktemp("integrity")
    refs, diss = R.fault_clip(5, 10, 30, 5, 5)
    info = synth.clip_info(64, 48, 8, chroma=True)
    info.fps_num, info.fps_den = 25, 1
    rp, dp = str(d / "ref.y4m"), str(d / "dis.y4m")
    yuvio.write_y4m(rp, refs, info)
    yuvio.write_y4m(dp, diss, info)
    return rp, dp, diss


def _json(tmp_path, tag, res):
    from pqa2_amd import report
    log = report.build_vmaf_log(res["metrics"], 0.0, res["frame_indices"],
                                {"model": res["model_name"], **report.integrity_log_keys(res.get("integrity"))})
    path = str(tmp_path / f"{tag}.json")
    report.write_vmaf_json(path, log)
    return open(path).read()


def test_score_files_columns_events_and_nothing_new_when_off(tmp_path, clip):
    from pqa2_amd import _native as N
    from pqa2_amd.pipeline import score_files
    rp, dp, diss = clip
    old = score_files(rp, dp, "vmaf_v0.6.1", engine_factory=OracleEngine)
    off = score_files(rp, dp, "vmaf_v0.6.1", engine_factory=IntegrityEngine)
    assert _json(tmp_path, "old", old) == _json(tmp_path, "off", off)
    assert "integrity" not in off and not any(k in off["metrics"] for k in COLS)
    assert not IntegrityEngine.made[-1].features & N.FEAT_INTEGRITY
    IntegrityEngine.made.clear()
    res = score_files(rp, dp, "vmaf_v0.6.1", engine_factory=IntegrityEngine, integrity=True, integrity_options=OPTS,
                      psnr=False, ssim=False)
    main, sad_eng = IntegrityEngine.made
    assert main.features & N.FEAT_INTEGRITY and main.n_planes == 3 and main.thr == 37 and main.history_calls == []
    assert sad_eng.features == N.FEAT_INTEGRITY and sum(sad_eng.sad_calls) >= 29 + 3
    assert res["integrity"] == WANT and res["integrity_lines"] == WANT_LINES
    rm, ra, _ = R.freezedetect(diss, 8, duration=0.4)
    assert np.array_equal(res["metrics"]["freeze_mafd"], rm) and np.array_equal(res["freeze_anchor"], ra)
    sm, ss, _ = R.scdet(diss, 8)
    assert np.array_equal(res["metrics"]["scd_mafd"], sm) and np.array_equal(res["metrics"]["scd_score"], ss)
    assert np.array_equal(res["metrics"]["black_ratio"], np.array([1.0] * 5 + [0.0] * 50))
    log = json.loads(_json(tmp_path, "on", res))
    assert log["integrity"] == WANT
    assert all(k in log["frames"][0]["metrics"] and k in log["pooled_metrics"] for k in COLS)
    old_log = json.loads(_json(tmp_path, "old2", score_files(rp, dp, "vmaf_v0.6.1", engine_factory=OracleEngine, psnr=False, ssim=False)))
    for a, b in zip(old_log["frames"], log["frames"]):
        assert all(b["metrics"][k] == v for k, v in a["metrics"].items())


def test_full_range_header_and_options_set_the_black_threshold(tmp_path):
    from pqa2_amd import synth, yuvio
    from pqa2_amd.pipeline import score_files
    refs, diss = R.fault_clip(2, 2, 2, 1, 1)
    for rng, opts, want in ((None, None, 37), ("limited", None, 37), ("full", None, 25), ("full", {"pixel_black_th": 0.2}, 51),
                            (None, {"pixel_black_th": 0.0}, 16)):
        info = synth.clip_info(64, 48, 8, chroma=True)
        info.color_range = rng
        rp, dp = str(tmp_path / "r.y4m"), str(tmp_path / "d.y4m")
        yuvio.write_y4m(rp, refs, synth.clip_info(64, 48, 8, chroma=True))
        yuvio.write_y4m(dp, diss, info)
        IntegrityEngine.made.clear()
        score_files(rp, dp, "vmaf_v0.6.1", engine_factory=IntegrityEngine, integrity=True, integrity_options=opts, psnr=False, ssim=False)
        assert IntegrityEngine.made[0].thr == want, (rng, opts)
    with pytest.raises(ValueError):
        score_files(rp, dp, "vmaf_v0.6.1", engine_factory=IntegrityEngine, integrity=True, integrity_options={"bogus": 1})


def test_shards_arm_every_plane_of_the_distorted_history(clip, monkeypatch):
    from pqa2_amd import shard
    from pqa2_amd.pipeline import score_files
    rp, dp, diss = clip
    monkeypatch.setattr(shard, "gather_records", lambda local, n, *x, width=24, **k: np.zeros((n, width)))
    IntegrityEngine.made.clear()
    assert score_files(rp, dp, "vmaf_v0.6.1", engine_factory=IntegrityEngine, integrity=True, psnr=False, ssim=False,
                       rank=1, world_size=3) is None
    eng = IntegrityEngine.made[0]
    a, b = shard.shard_bounds(len(diss), 3, 1)
    assert eng.history_calls == [True] and len(eng.prev) == 3 and all(np.array_equal(p, q) for p, q in zip(eng.prev, diss[a - 1]))
    assert np.array_equal(eng.collect_ext5(a, b - a)[5], R.rows(diss, 37)[a:b], equal_nan=True)
    IntegrityEngine.made.clear()
    score_files(rp, dp, "vmaf_v0.6.1", engine_factory=IntegrityEngine, psnr=False, ssim=False, rank=1, world_size=3)
    assert IntegrityEngine.made[0].history_calls == []


def test_analyzer_json_log_file_and_child_argv(tmp_path, clip, monkeypatch):
    from pqa2_amd import vmaf_analyzer as V
    rp, dp, _ = clip
    a = V.VMAFAnalyzer()
    assert a.integrity_enabled is False
    a.set_output_directory(str(tmp_path))
    a.set_test_name("cap")
    a._engine_factory = IntegrityEngine
    res = a.analyze_videos(rp, dp)
    assert res is not None and "integrity" not in res and "integrity" not in res["raw_results"]
    assert not [f for _, _, fs in os.walk(tmp_path) for f in fs if f.endswith("_integrity.txt")]
    a.set_advanced_options(integrity_enabled=True, integrity_options=OPTS)
    assert a._ssim_family_kwargs() == {"integrity": True, "integrity_options": OPTS}
    res = a.analyze_videos(rp, dp)
    assert res["integrity"] == WANT and res["raw_results"]["integrity"] == WANT
    assert re.fullmatch(r"cap_\d{8}_\d{6}_integrity\.txt", os.path.basename(res["integrity_log"]))
    assert open(res["integrity_log"]).read().splitlines() == WANT_LINES
    assert all(k in res["raw_results"]["pooled_metrics"] for k in COLS)

    class Opts:
        def __init__(self, d):
            self.d = d

        def get_setting(self, k):
            return self.d
    a.set_options_from_manager(Opts({"integrity_enabled": True, "integrity_options": {"scd_threshold": 5}}))
    assert a.integrity_enabled is True and a.integrity_options == {"scd_threshold": 5}
    a.set_options_from_manager(Opts({}))
    assert a.integrity_enabled is False and a.integrity_options == {}

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
    b.set_advanced_options(integrity_enabled=True, integrity_options={"freeze_duration": 0.4})
    b._integrity_path = "x_integrity.txt"
    b._run_child_job(rp, dp, "vmaf_v0.6.1", "j.json", None, None, 3)
    for c in cmds:
        c[c.index("--master-port") + 1] = "PORT"
    extra = ["--integrity", "--integrity-log", "x_integrity.txt", "--freeze-duration", "0.4"]
    assert "--integrity" not in cmds[0]
    i = cmds[1].index("--integrity")
    assert cmds[1][i:i + len(extra)] == extra and cmds[1][:i] + cmds[1][i + len(extra):] == cmds[0]


def test_score_cli_flags_reach_score_files(monkeypatch, tmp_path, clip):
    from pqa2_amd import pipeline, score
    rp, dp, _ = clip
    seen = []
    real = pipeline.score_files

    def spy(*a, **kw):
        seen.append({k: kw[k] for k in ("integrity", "integrity_options") if k in kw})
        return real(*a, engine_factory=IntegrityEngine, **kw)
    monkeypatch.setattr(pipeline, "score_files", spy)
    out = str(tmp_path / "o.json")
    assert score.main([rp, dp, "--json", out]) == 0
    assert seen[-1] == {} and "integrity" not in json.load(open(out))
    logp = str(tmp_path / "ev.txt")
    assert score.main([rp, dp, "--json", out, "--integrity", "--integrity-log", logp, "--freeze-duration", "0.4",
                       "--black-min-duration", "0.2"]) == 0
    assert seen[-1] == {"integrity": True, "integrity_options": OPTS}
    assert json.load(open(out))["integrity"] == WANT and open(logp).read().splitlines() == WANT_LINES
    assert score.main([rp, dp, "--json", out, "--scd-threshold", "30"]) == 0      # an option implies the switch
    assert seen[-1] == {"integrity": True, "integrity_options": {"scd_threshold": 30.0}}
    assert [e["frame"] for e in json.load(open(out))["integrity"]["scene_changes"]] == [50]
