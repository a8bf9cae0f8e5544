"""Capture-integrity analysis of the distorted clip: the host state machines of FFmpeg's freezedetect, blackdetect and
scdet filters (libavfilter/vf_freezedetect.c, vf_blackdetect.c, vf_scdet.c, scene_sad.c) over the per-frame integers the
GPU delivers (PQA_FEAT_INTEGRITY, the fifth extension record: the SAD of every plane against the previous frame and the
number of black luma samples).  Pure functions of those rows, the geometry, the frame rate and the options; no device.

Time: frame i has pts_i = i * fps_den / fps_num seconds.  Durations are compared as exact rationals (the options are taken
at microsecond resolution, as FFmpeg's duration options are), so a run that is exactly `duration` long qualifies.

freezedetect compares every frame with an ANCHOR frame, not with its predecessor: the anchor moves only when a frame is
not still, so slow drift adds up against it.  While the anchor is the previous frame the row's own SAD is the answer; only
inside a still run (from its second still frame on) is the `anchored_sad(anchor, frame)` callback asked for the exact SAD
against the anchor -- never on a clip without still frames.

What is unpinned against FFmpeg itself: DESIGN.md section 1."""
from __future__ import annotations

from fractions import Fraction

import numpy as np

DEFAULTS = {
    "freeze_noise": 0.001,             # freezedetect noise (n), as a ratio (not dB)
    "freeze_duration": 2.0,            # freezedetect duration (d), seconds
    "black_min_duration": 2.0,         # blackdetect black_min_duration (d), seconds
    "picture_black_ratio_th": 0.98,    # blackdetect picture_black_ratio_th (pic_th)
    "pixel_black_th": 0.10,            # blackdetect pixel_black_th (pix_th)
    "scd_threshold": 10.0,             # scdet threshold (t)
}


def options(overrides=None) -> dict:
    """DEFAULTS with `overrides` applied; an unknown name is an error."""
    out = dict(DEFAULTS)
    for k, v in (overrides or {}).items():
        if k not in DEFAULTS:
            raise ValueError(f"unknown integrity option {k!r} (known: {', '.join(DEFAULTS)})")
        if v is not None:
            out[k] = float(v)
    return out


def black_threshold(bit_depth: int, full_range: bool = False, pixel_black_th: float = 0.10) -> int:
    """blackdetect's integer sample threshold: trunc(16 f + pixel_black_th * 219 f) on a limited-range clip,
    trunc(pixel_black_th * (2^bpc - 1)) on a full-range one, f = 2^(bpc - 8).  37 / 25 at 8 bit, 151 at 10 bit limited."""
    f = 1 << (bit_depth - 8)
    if full_range:
        return int(pixel_black_th * ((1 << bit_depth) - 1))
    return int(16.0 * f + pixel_black_th * 219.0 * f)


def _seconds(frames: int, fps_num: int, fps_den: int) -> Fraction:
    return Fraction(int(frames) * int(fps_den), int(fps_num))


def _dur(seconds: float) -> Fraction:
    return Fraction(seconds).limit_denominator(1000000)


def pts(i: int, fps_num: int, fps_den: int) -> float:
    return float(_seconds(i, fps_num, fps_den))


def scdet(sad_y, width: int, height: int, bit_depth: int, fps_num: int, fps_den: int, threshold: float = 10.0):
    """(mafd [n], score [n], scene_changes): mafd_i = 100 * sad / (w h) / 2^bpc, score_i = clip(min(mafd_i, |mafd_i -
    mafd_{i-1}|), 0, 100); frame 0 (and any frame without a SAD) has mafd 0.  A scene change where score >= threshold."""
    sad = np.asarray(sad_y, np.float64)
    n = sad.shape[0]
    mafd = np.where(np.isnan(sad), 0.0, 100.0 * sad / (float(width) * float(height)) / float(1 << bit_depth))
    if n:
        mafd[0] = 0.0
    prev = np.concatenate([[0.0], mafd[:-1]]) if n else mafd
    score = np.clip(np.minimum(mafd, np.abs(mafd - prev)), 0.0, 100.0)
    if n:
        score[0] = 0.0
    events = [{"frame": int(i), "time": pts(i, fps_num, fps_den), "score": float(score[i])}
              for i in range(n) if score[i] >= threshold]
    return mafd, score, events


def blackdetect(black_count, width: int, height: int, fps_num: int, fps_den: int, picture_black_ratio_th: float = 0.98,
                black_min_duration: float = 2.0):
    """(ratio [n], blacks): frame i is black when black_count / (w h) >= picture_black_ratio_th; a run starts at the pts of
    its first frame and ends at the pts of the first non-black frame after it (the last frame's pts when the clip ends
    inside it); reported when end - start >= black_min_duration."""
    cnt = np.asarray(black_count, np.float64)
    n = cnt.shape[0]
    ratio = cnt / (float(width) * float(height))
    min_d = _dur(black_min_duration)
    events = []
    start = None

    def close(end_frame, last_frame):
        d = _seconds(end_frame - start, fps_num, fps_den)
        if d >= min_d:
            events.append({"start": pts(start, fps_num, fps_den), "end": pts(end_frame, fps_num, fps_den),
                           "duration": float(d), "first_frame": int(start), "last_frame": int(last_frame)})
    for i in range(n):
        black = ratio[i] >= picture_black_ratio_th
        if black and start is None:
            start = i
        elif not black and start is not None:
            close(i, i - 1)
            start = None
    if start is not None:       # the clip ends inside the run: it ends at the last frame's pts
        close(n - 1, n - 1)
    return ratio, events


def freezedetect(sad_prev, plane_samples, bit_depth: int, fps_num: int, fps_den: int, noise: float = 0.001,
                 duration: float = 2.0, anchored_sad=None):
    """(mafd [n], anchor [n], freezes).  sad_prev: [n, planes] SADs against the previous frame (NaN columns of planes the
    clip does not have are ignored; frame 0's row is not read); plane_samples: samples per plane.  mafd(i, A) = sum of the
    planes' SADs of frame i against the anchor A / total samples / 2^bpc; still when <= noise.  A frame that is not still
    becomes the anchor and ends an open freeze at its pts; a freeze is open once pts_i - pts_A >= duration and starts at
    pts_A.  anchored_sad(A, i) -> the SAD (a number, or per-plane numbers) of frame i against frame A, asked only when
    A != i - 1."""
    sp = np.asarray(sad_prev, np.float64)
    if sp.ndim == 1:
        sp = sp[:, None]
    n = sp.shape[0]
    n_pl = len(plane_samples)
    total = float(sum(int(s) for s in plane_samples))
    scale = float(1 << bit_depth)
    min_d = _dur(duration)
    mafd = np.zeros(n, np.float64)
    anchor = np.zeros(n, np.int64)
    events = []
    A = 0
    open_ev = None
    for i in range(1, n):
        if A == i - 1:
            sad = float(np.sum(sp[i, :n_pl]))
        else:
            if anchored_sad is None:
                raise ValueError(f"frame {i} needs its SAD against anchor frame {A}, but no anchored_sad callback was given")
            sad = float(np.sum(np.asarray(anchored_sad(A, i), np.float64)))
        mafd[i] = sad / total / scale
        anchor[i] = A
        if mafd[i] <= noise:
            if open_ev is None and _seconds(i - A, fps_num, fps_den) >= min_d:
                open_ev = {"start": pts(A, fps_num, fps_den), "end": None, "duration": None, "first_frame": int(A),
                           "last_frame": None}
        else:
            if open_ev is not None:
                open_ev["end"] = pts(i, fps_num, fps_den)
                open_ev["duration"] = float(_seconds(i - A, fps_num, fps_den))
                open_ev["last_frame"] = i - 1
                events.append(open_ev)
                open_ev = None
            A = i
    if open_ev is not None:     # open at the end of the clip: a start and no end
        open_ev["last_frame"] = n - 1
        events.append(open_ev)
    return mafd, anchor, events


def analyze(sad_prev, black_count, *, width: int, height: int, plane_sizes, bit_depth: int, fps_num: int, fps_den: int,
            opts=None, anchored_sad=None) -> dict:
    """The three filters over one clip's gathered rows.  plane_sizes: [(w, h)] of the planes the clip has.  Returns
    {"columns": {scd_mafd, scd_score, black_ratio, freeze_mafd}, "freeze_anchor", "freezes", "blacks", "scene_changes"}."""
    o = options(opts)
    sp = np.asarray(sad_prev, np.float64)
    if sp.ndim == 1:
        sp = sp[:, None]
    if not fps_num or not fps_den:
        fps_num, fps_den = 25, 1
    mafd, score, scenes = scdet(sp[:, 0], width, height, bit_depth, fps_num, fps_den, o["scd_threshold"])
    ratio, blacks = blackdetect(black_count, width, height, fps_num, fps_den, o["picture_black_ratio_th"],
                                o["black_min_duration"])
    fm, anchor, freezes = freezedetect(sp, [w * h for w, h in plane_sizes], bit_depth, fps_num, fps_den, o["freeze_noise"],
                                       o["freeze_duration"], anchored_sad)
    return {"columns": {"scd_mafd": mafd, "scd_score": score, "black_ratio": ratio, "freeze_mafd": fm},
            "freeze_anchor": anchor, "freezes": freezes, "blacks": blacks, "scene_changes": scenes}


def _t(x: float) -> str:
    return "%.6g" % x


def log_lines(result: dict) -> list:
    """One line per event in FFmpeg's log wording, ordered by the time each line states (ties: freeze, black, scene)."""
    rows = []
    for ev in result.get("freezes", []):
        rows.append((ev["start"], 0, f"freeze_start: {_t(ev['start'])}"))
        if ev["end"] is not None:
            rows.append((ev["end"], 0, f"freeze_duration: {_t(ev['duration'])}"))
            rows.append((ev["end"], 0, f"freeze_end: {_t(ev['end'])}"))
    for ev in result.get("blacks", []):
        rows.append((ev["start"], 1, f"black_start:{_t(ev['start'])} black_end:{_t(ev['end'])} black_duration:{_t(ev['duration'])}"))
    for ev in result.get("scene_changes", []):
        rows.append((ev["time"], 2, f"lavfi.scd.score: {ev['score']:.3f}, lavfi.scd.time: {_t(ev['time'])}"))
    rows.sort(key=lambda r: (r[0], r[1]))   # stable: a freeze's duration line stays in front of its end line
    return [r[2] for r in rows]


def events_json(result: dict) -> dict:
    """The three event lists as plain JSON values."""
    return {k: [dict(ev) for ev in result.get(k, [])] for k in ("freezes", "blacks", "scene_changes")}
