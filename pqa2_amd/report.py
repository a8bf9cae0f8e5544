"""On-disk artefacts the reference reads back after the three ffmpeg passes:
the libvmaf `log_fmt=json` log (app/vmaf_analyzer.py:374-375, parsed at :638-690 and by
app/ui/tabs/results_tab.py:3000-3028, app/report_generator.py:288-311) and FFmpeg's psnr/ssim
`stats_file` text logs (app/vmaf_analyzer.py:1032,1062).
"""
from __future__ import annotations

import math

import numpy as np

from .model import pool

ENGINE_VERSION = "pqa2_amd-0.2.0"


def _f6(x: float) -> str:
    x = float(x)
    if math.isnan(x):
        return "nan"
    if math.isinf(x):
        return "inf" if x > 0 else "-inf"
    return f"{x:.6f}"


def xpsnr_stats_lines(db: np.ndarray) -> list[str]:
    """FFmpeg xpsnr `stats_file` lines: `n: %4d` (1-based) then `  XPSNR %c: %3.4f` for y, u, v (as many as db's columns,
    [n, planes] per-frame dB; +inf prints as inf)."""
    lines = []
    for i, row in enumerate(np.asarray(db, dtype=np.float64).reshape(len(db), -1)):
        s = f"n: {i + 1:4d}"
        for c, v in zip("yuv", row):
            s += f"  XPSNR {c}: {_f4(v)}"
        lines.append(s)
    return lines


def _f4(x: float) -> str:
    x = float(x)
    if math.isnan(x):
        return "nan"
    if math.isinf(x):
        return "inf" if x > 0 else "-inf"
    return f"{x:3.4f}"


def xpsnr_summary(wsse: np.ndarray, db: np.ndarray, plane_sizes, bit_depth: int) -> dict:
    """FFmpeg xpsnr's clip aggregate per plane: the square-mean-root 10 log10(w h max^2 / (sum sqrt(WSSE) / N)^2) when
    sum sqrt(WSSE) >= N, else the arithmetic mean of the per-frame dB values; {"y", "u", "v" (present planes), "min"}."""
    wsse = np.asarray(wsse, dtype=np.float64).reshape(len(wsse), -1)
    db = np.asarray(db, dtype=np.float64).reshape(len(db), -1)
    n = wsse.shape[0]
    peak2 = float(((1 << bit_depth) - 1) ** 2)
    out = {}
    for p in range(wsse.shape[1]):
        w, h = plane_sizes[p]
        s = 0.0
        for x in wsse[:, p]:          # a running sum in frame order, as the filter keeps it
            s += math.sqrt(float(x))
        if n == 0:
            v = math.inf
        elif s >= n:
            avg = s / n
            v = 10.0 * math.log10(float(w * h * int(peak2)) / (avg * avg))
        else:
            t = 0.0
            for x in db[:, p]:
                t += float(x)
            v = t / n
        out["yuv"[p]] = v
    out["min"] = min(out.values()) if out else math.nan
    return out


def xpsnr_log_keys(summary: dict | None) -> dict:
    """Top-level keys of the JSON log that carry FFmpeg's xpsnr summary (xpsnr_y / _u / _v and their minimum, xpsnr); none
    without one, and none for a value that is not finite."""
    if not summary:
        return {}
    out = {f"xpsnr_{c}": float(summary[c]) for c in "yuv" if c in summary}
    out["xpsnr"] = float(summary["min"])
    return {k: v for k, v in out.items() if math.isfinite(v)}   # +inf (identical clips) has no JSON spelling: left out


def integrity_log_keys(events: dict | None) -> dict:
    """Top-level key of the JSON log that carries the capture-integrity event lists (freezes / blacks / scene_changes,
    pipeline.score_files(integrity=True)); none without them."""
    return {"integrity": events} if events is not None else {}


def alignment_log_keys(alignment: dict | None) -> dict:
    """Top-level key of the JSON log that carries the temporal alignment (pipeline.score_files(align=K)); none without it.
    An infinite confidence (an exact match) is written as null: JSON has no infinity."""
    if not alignment:
        return {}
    def finite(obj):
        conf = obj.get("confidence")
        return {**obj, "confidence": conf if conf is not None and np.isfinite(conf) else None}
    out = finite(alignment) if "confidence" in alignment else dict(alignment)
    if alignment.get("spatial"):
        out["spatial"] = finite(alignment["spatial"])
    if alignment.get("levels"):   # no confidence there; any float that is not finite becomes null, per-plane results included
        def finite_all(obj):
            return {k: finite_all(v) if isinstance(v, dict) else (None if isinstance(v, float) and not np.isfinite(v) else v)
                    for k, v in obj.items()}
        out["levels"] = finite_all(alignment["levels"])
    if alignment.get("colour"):   # lists of floats in there too; any float that is not finite becomes null
        def finite_deep(v):
            if isinstance(v, dict):
                return {k: finite_deep(x) for k, x in v.items()}
            if isinstance(v, (list, tuple)):
                return [finite_deep(x) for x in v]
            return None if isinstance(v, float) and not np.isfinite(v) else v
        out["colour"] = finite_deep(alignment["colour"])
    return {"alignment": out}


def alignment_summary_line(alignment: dict) -> str:
    """One line for a summary or a status bar: the offset found, its error and what the frame map saw."""
    k = int(alignment["offset_frames"])
    lo, hi = alignment.get("searched", [None, None])
    conf = alignment.get("confidence")
    conf_s = "exact match" if conf is None or not np.isfinite(conf) else f"confidence {conf:.1f}x"
    where = "capture late" if k > 0 else "capture early" if k < 0 else "in step"
    return (f"Alignment: offset {k:+d} frames ({alignment.get('offset_seconds', 0.0):+.3f} s, {where}), MSE "
            f"{alignment.get('mse', 0.0):.2f}, {conf_s}, {len(alignment.get('repeated', []))} repeated / "
            f"{len(alignment.get('dropped', []))} dropped frames, searched {lo} ... {hi}")


def spatial_summary_line(spatial: dict) -> str:
    """One line for a summary or a status bar: the displacement found, its error and whether the clips were cropped."""
    conf = spatial.get("confidence")
    conf_s = "exact match" if conf is None or not np.isfinite(conf) else f"confidence {conf:.1f}x"
    if spatial.get("applied"):
        what = "cropped to the common window" + ("" if spatial.get("chroma_exact", True) else ", chroma half a sample off")
    elif spatial.get("at_edge"):
        what = "minimum on the border of the search: not applied"
    else:
        what = "in place"
    return (f"Spatial alignment: capture displaced by ({int(spatial['dx']):+d}, {int(spatial['dy']):+d}) px, MSE "
            f"{spatial.get('mse', 0.0):.2f}, {conf_s}, agreement {100.0 * spatial.get('agreement', 0.0):.0f} % of "
            f"{spatial.get('frames', 0)} frames, searched +-{spatial.get('searched')} px, {what}")


def geometry_summary_line(geometry: dict) -> str:
    """One line for a summary or a status bar: the sub-pixel shift and scale found, their effect and whether they were undone."""
    if not geometry.get("converged"):
        what = "no stable estimate: nothing applied"
    elif geometry.get("applied"):
        crop = geometry.get("crop", [0, 0, 0, 0])
        what = f"capture resampled ({geometry.get('filter')}), clips cropped by {crop[0]}/{crop[1]}/{crop[2]}/{crop[3]} px"
    else:
        what = "within tolerance: nothing applied"
    return (f"Registration: capture displaced by ({geometry.get('dx', 0.0):+.3f}, {geometry.get('dy', 0.0):+.3f}) px, scaled by "
            f"({geometry.get('sx', 1.0):.5f}, {geometry.get('sy', 1.0):.5f}), {geometry.get('corner_px', 0.0):.3f} px at the "
            f"corners, MSE {geometry.get('mse_before', 0.0):.2f} -> {geometry.get('mse_after', 0.0):.2f}, "
            f"{geometry.get('iterations', 0)} iterations on {geometry.get('frames', 0)} frames, {what}")


def active_summary_line(active: dict) -> str:
    """One line for a summary or a status bar: the bars found in both clips and whether the clips were cropped."""
    def bars(ap):
        if ap.get("all_dark"):
            return "all dark"
        return "{}/{}/{}/{}".format(*(ap.get(k, 0) for k in ("left", "top", "right", "bottom")))
    crop = active.get("crop", [0, 0, 0, 0])
    if active.get("applied"):
        what = f"clips cropped by {crop[0]}/{crop[1]}/{crop[2]}/{crop[3]} px"
    elif active.get("reason"):
        what = f"{active['reason']}: nothing cropped"
    else:
        what = f"common margins {crop[0]}/{crop[1]}/{crop[2]}/{crop[3]} px, not cropped"
    return (f"Active picture: bars (left/top/right/bottom) reference {bars(active.get('reference', {}))}, capture "
            f"{bars(active.get('distorted', {}))} on {active.get('frames', 0)} frames, {what}")


def distortion_log_keys(distortion: dict | None) -> dict:
    """Top-level key of the JSON log that carries the distortion map's findings (pipeline.score_files(distortion_map=T)); none
    without them.  Any float that is not finite becomes null."""
    if not distortion:
        return {}
    def finite_deep(v):
        if isinstance(v, dict):
            return {k: finite_deep(x) for k, x in v.items()}
        if isinstance(v, (list, tuple)):
            return [finite_deep(x) for x in v]
        if isinstance(v, (np.integer, np.floating)):
            v = v.item()
        return None if isinstance(v, float) and not np.isfinite(v) else v
    return {"distortion": finite_deep(distortion)}


def spectrum_log_keys(spectrum: dict | None) -> dict:
    """Top-level key of the JSON log that carries the distortion spectrum (pipeline.score_files(spectrum=L)); none without it.
    Any float that is not finite becomes null."""
    if not spectrum:
        return {}
    return {"spectrum": distortion_log_keys(spectrum)["distortion"]}


def spectrum_summary_line(spectrum: dict) -> str:
    """One line for a summary or a status bar: what kind of difference the luma has."""
    s = spectrum.get("planes", {}).get("y", {}).get("summary", {})
    line = f"Distortion spectrum: {spectrum.get('levels', 0)} octaves on {spectrum.get('frames', 0)} frames, {s.get('kind', '?')}"
    if s.get("kind") == "loss":
        line += f" ({s.get('axis')})"
    if s.get("kind") in ("loss", "noise", "clean"):
        line += (f", MSE {s.get('total_mse', 0.0):.2f}: {100.0 * s.get('loss_share', 0.0):.0f} % detail loss, "
                 f"{100.0 * s.get('noise_share', 0.0):.0f} % added noise")
        for key, name in (("bandwidth_h", "horizontal"), ("bandwidth_v", "vertical")):
            bw = s.get(key) or {}
            if bw.get("level"):
                line += f", {name} detail passes up to 1/{1 << bw['level']} cycles per pixel"
    return line


def temporal_log_keys(temporal: dict | None) -> dict:
    """Top-level key of the JSON log that carries the temporal distortion (pipeline.score_files(temporal=T)); none without it.
    Any float that is not finite becomes null."""
    if not temporal:
        return {}
    return {"temporal": distortion_log_keys(temporal)["distortion"]}


def temporal_summary_line(temporal: dict) -> str:
    """One line for a summary or a status bar: what is wrong with the motion of the luma."""
    s = temporal.get("planes", {}).get("y", {}).get("summary", {})
    line = (f"Temporal distortion: {temporal.get('tile', 0)} px tiles on {temporal.get('frames', 0)} frames, {s.get('kind', '?')}")
    if s.get("kind") == "blend":
        line += f" (weight {s.get('blend_weight') or 0.0:.3f} of the previous frame)"
    if s.get("kind") in ("blend", "loss", "noise", "clean"):
        line += (f", temporal MSE {s.get('temporal_mse', 0.0):.2f} against a motion of {s.get('motion_mse', 0.0):.2f}: "
                 f"{100.0 * s.get('loss_share', 0.0):.0f} % loss, {100.0 * s.get('noise_share', 0.0):.0f} % noise")
        if s.get("still_noise_mse") is not None:
            line += f", {s['still_noise_mse']:.2f} where nothing moves"
        if s.get("pops"):
            line += f", {len(s['pops'])} pops"
            if s.get("pop_period"):
                line += f" every {s['pop_period']} frames"
    return line


def grid_log_keys(coding_grid: dict | None) -> dict:
    """Top-level key of the JSON log that carries the coding-grid detection (pipeline.score_files(coding_grid=True)); none
    without it.  Any float that is not finite becomes null."""
    if not coding_grid:
        return {}
    return {"coding_grid": distortion_log_keys(coding_grid)["distortion"]}


def itp_log_keys(delta_itp: dict | None) -> dict:
    """Top-level key of the JSON log that carries the BT.2124 colour difference (pipeline.score_files(delta_itp=)): the spec
    used, its coefficients included, and itp.summary; none without it.  Any float that is not finite becomes null."""
    if not delta_itp:
        return {}
    return {"delta_itp": distortion_log_keys(delta_itp)["distortion"]}


def overlay_log_keys(overlay: dict | None) -> dict:
    """Top-level key of the JSON log that carries the overlay mask (pipeline.score_files(overlay_mask=)): what was found, what
    was masked and towards what; none without it."""
    if not overlay:
        return {}
    return {"overlay": distortion_log_keys(overlay)["distortion"]}


def result_log_keys(res) -> dict:
    """The top-level keys of the JSON log that a pipeline.ScoreResult carries besides the frames: build_vmaf_log's extra_top."""
    return {"model": res["model_name"], **xpsnr_log_keys(res.get("xpsnr_summary")), **integrity_log_keys(res.get("integrity")),
            **alignment_log_keys(res.get("alignment")), **{k: res[k] for k in ("resize", "input") if res.get(k)},
            **distortion_log_keys(res.get("distortion")), **spectrum_log_keys(res.get("spectrum")),
            **temporal_log_keys(res.get("temporal")), **grid_log_keys(res.get("coding_grid")),
            **itp_log_keys(res.get("delta_itp")), **overlay_log_keys(res.get("overlay"))}


def overlay_summary_line(overlay: dict) -> str:
    """One line for a summary or a status bar: the burnt-in overlay and what was done about it."""
    boxes = overlay.get("boxes") or []
    how = "given" if not overlay.get("detected", True) else f"persistent in {overlay.get('frames_sampled', 0)} sampled frames"
    if not boxes:
        return f"Overlay mask ({overlay.get('mode', '?')}): no region {how}, nothing masked"
    fill = overlay.get("fill")
    done = (f"blended towards {'the reference' if fill == 'reference' else fill}" if overlay.get("applied") else "reported only")
    return (f"Overlay mask ({overlay.get('mode', '?')}): {len(boxes)} region{'s' if len(boxes) != 1 else ''} {how}, first "
            f"{boxes[0]}, {100.0 * overlay.get('share', 0.0):.1f} % of the picture under the mask, {done}")


def itp_summary_line(delta_itp: dict) -> str:
    """One line for a summary or a status bar: the pooled Delta E ITP and what it is made of."""
    sp, s = delta_itp.get("spec", {}), delta_itp.get("summary", {})
    line = (f"Delta E ITP ({sp.get('transfer', '?')}, {sp.get('matrix', '?')}, {sp.get('range', '?')} range): {s.get('kind', '?')}, "
            f"mean {s.get('mean', 0.0):.3f}, max {s.get('max', 0.0):.2f}, {100.0 * s.get('above_jnd', 0.0):.1f} % of the pixels "
            f"above {s.get('threshold', 1.0):g}")
    if s.get("kind") not in ("identical", None):
        line += (f", {100.0 * s.get('luminance_share', 0.0):.0f} % luminance / {100.0 * s.get('chroma_share', 0.0):.0f} % chroma, "
                 f"worst frame {s.get('worst_frame', 0)} (mean {s.get('worst_frame_mean', 0.0):.3f})")
    return line


def grid_summary_line(coding_grid: dict) -> str:
    """One line for a summary or a status bar: the block grid found in the luma."""
    s = coding_grid.get("planes", {}).get("y", {}).get("summary", {})
    line = f"Coding grid: {s.get('kind', '?')}"
    if s.get("kind") == "grid":
        px, py = s.get("block") or (None, None)
        fx, fy = s.get("phase") or (None, None)
        line += (f", blocks of {px or '?'} x {py or '?'} at phase ({'?' if fx is None else fx}, {'?' if fy is None else fy})"
                 f"{'' if s.get('aligned') else ': cropped or shifted after the encode'}")
        z = [g["z2"] for g in (s.get("x"), s.get("y")) if g]
        if z:
            line += f", z^2 {max(z):.0f}"
    if any((s.get("reference_grid") or {}).get(k) for k in ("x", "y")):
        line += "; the reference has a grid of its own"
    return line


def distortion_summary_line(distortion: dict) -> str:
    """One line for a summary or a status bar: the defects and persistent regions found in the luma."""
    y = distortion.get("planes", {}).get("y", {})
    worst = y.get("worst_frame") or {}
    line = (f"Distortion map: {distortion.get('tile', 0)} px tiles on {distortion.get('frames', 0)} frames, "
            f"{len(y.get('defects', []))} localised defects, {len(y.get('persistent', []))} persistent regions")
    if y.get("persistent") and y.get("psnr_all") is not None and y.get("psnr_excluding") is not None:
        line += f" (PSNR {y['psnr_all']:.2f} dB, {y['psnr_excluding']:.2f} dB without them)"
    if worst:
        line += f", worst tile {worst.get('tile_psnr_min', 0.0):.2f} dB in frame {worst.get('frame', 0)}"
    return line


def colour_summary_line(colour: dict) -> str:
    """One line for a summary or a status bar: the colour map found, its error and whether it was undone."""
    if colour.get("degenerate"):
        return f"Colour alignment: flat or monochrome-looking content in {colour.get('frames', 0)} frames: no map measured"
    kind = colour.get("kind", "identity")
    if kind == "identity":
        what = "colour matrix in place"
    elif kind == "matrix":
        what = "capture went through a colour matrix that is no named conversion"
    else:
        what = "capture decoded as {} and encoded as {}".format(*kind.split("_to_"))
    if colour.get("applied"):
        tail = "corrected"
    elif not colour.get("mismatch"):
        tail = "nothing to correct"
    elif not colour.get("cross_plane"):
        tail = "planes not coupled: a matter for level alignment, not corrected"
    else:
        tail = "not corrected"
    return (f"Colour alignment: {what}, MSE {colour.get('mse_identity', 0.0):.2f} as captured, {colour.get('mse_matrix', 0.0):.2f} "
            f"after the fit, {colour.get('mse_diagonal', 0.0):.2f} per plane alone, {colour.get('samples', 0)} samples of "
            f"{colour.get('frames', 0)} frames ({100.0 * (colour.get('samples_masked_share') or 0.0):.1f} % masked), {tail}")


def levels_summary_line(levels: dict) -> str:
    """One line for a summary or a status bar: the level mapping found for luma, its error and whether it was undone."""
    if levels.get("degenerate"):
        return f"Level alignment: flat reference in {levels.get('frames', 0)} frames: no mapping measured"
    kind = levels.get("kind", "identity")
    what = {"identity": "levels in place", "limited_to_full": "capture expanded from limited to full range",
            "full_to_limited": "capture compressed from full to limited range"}.get(kind, "capture levels scaled and offset")
    if kind == "curve":   # pipeline.score_files(level_curve=True) only
        gamma = levels.get("gamma")
        what = "capture levels follow a transfer curve" + (f", gamma {gamma:.3f}" if gamma is not None else "")
    planes = levels.get("planes") or {"y": levels}
    done = [k for k in planes if planes[k].get("applied")]
    if done:
        tail = "corrected on " + ", ".join(k.upper() for k in done)
    else:
        tail = "not corrected" if levels.get("mismatch") else "nothing to correct"
    fitted = f"{levels.get('mse_affine', 0.0):.2f} after the fit"
    if kind == "curve":
        fitted += f", {levels.get('mse_monotone') or 0.0:.2f} about the curve"
    return (f"Level alignment: {what} (gain {levels.get('gain', 1.0):.4f}, offset {levels.get('offset', 0.0):+.2f}), MSE "
            f"{levels.get('mse_identity', 0.0):.2f} as captured, {fitted}, "
            f"{levels.get('frames', 0)} frames, {tail}")


def build_vmaf_log(metrics: dict, fps: float, frame_indices=None, extra_top: dict | None = None) -> dict:
    """dict with libvmaf's JSON schema: version, fps, frames[{frameNum, metrics}], pooled_metrics,
    aggregate_metrics.  Values are rounded to 6 decimals like libvmaf's %.6f writer."""
    keys = list(metrics.keys())
    n = len(next(iter(metrics.values()))) if metrics else 0
    idx = list(range(n)) if frame_indices is None else list(frame_indices)
    frames = []
    for j in range(n):
        frames.append({"frameNum": int(idx[j]),
                       "metrics": {k: float(_f6(metrics[k][j])) for k in keys}})
    pooled = {k: {a: float(_f6(b)) for a, b in pool(metrics[k]).items()} for k in keys}
    log = {"version": ENGINE_VERSION, "fps": float(f"{fps:.2f}"), "frames": frames,
           "pooled_metrics": pooled, "aggregate_metrics": {}}
    if extra_top:
        log.update(extra_top)
    return log


def write_vmaf_json(path: str, log: dict) -> None:
    """Hand-rolled writer so numbers keep libvmaf's fixed 6-decimal form (json.dump would drop zeros)."""
    def num(v):
        return _f6(v) if isinstance(v, float) else str(v)
    with open(path, "w") as f:
        f.write("{\n")
        f.write(f'  "version": "{log["version"]}",\n')
        for k, v in log.items():
            if k in ("version", "fps", "frames", "pooled_metrics", "aggregate_metrics"):
                continue
            if isinstance(v, (dict, list)):      # structured extras (the integrity event lists): plain JSON
                import json
                f.write(f'  "{k}": {json.dumps(v)},\n')
                continue
            f.write(f'  "{k}": "{v}",\n' if isinstance(v, str) else f'  "{k}": {num(v)},\n')
        f.write(f'  "fps": {log["fps"]:.2f},\n')
        f.write('  "frames": [')
        for i, fr in enumerate(log["frames"]):
            f.write("\n    {\n")
            f.write(f'      "frameNum": {fr["frameNum"]},\n      "metrics": {{\n')
            items = list(fr["metrics"].items())
            for j, (k, v) in enumerate(items):
                f.write(f'        "{k}": {_f6(v)}{"," if j + 1 < len(items) else ""}\n')
            f.write("      }\n    }" + ("," if i + 1 < len(log["frames"]) else ""))
        f.write("\n  ],\n")
        f.write('  "pooled_metrics": {')
        pitems = list(log["pooled_metrics"].items())
        for i, (k, d) in enumerate(pitems):
            f.write(f'\n    "{k}": {{\n')
            ditems = list(d.items())
            for j, (a, b) in enumerate(ditems):
                f.write(f'      "{a}": {_f6(b)}{"," if j + 1 < len(ditems) else ""}\n')
            f.write("    }" + ("," if i + 1 < len(pitems) else ""))
        f.write("\n  },\n")
        f.write('  "aggregate_metrics": {\n  }\n}\n')


def _psnr(mse: float, peak: float) -> float:
    return float("inf") if mse <= 0 else 10.0 * math.log10(peak * peak / mse)


def _fmt2(x: float) -> str:
    return "inf" if math.isinf(x) else f"{x:0.2f}"


def psnr_stats_lines(sse: np.ndarray, plane_sizes, bit_depth: int, comps="yuv"):
    """FFmpeg vf_psnr.c stats_file lines from exact per-plane SSE.  sse: [n, planes] uint64."""
    peak = float((1 << bit_depth) - 1)
    sizes = np.array([w * h for (w, h) in plane_sizes], np.float64)
    weights = sizes / sizes.sum()
    lines = []
    for i in range(sse.shape[0]):
        comp_mse = [float(sse[i, p]) / sizes[p] for p in range(len(sizes))]
        mse = float(sum(comp_mse[p] * weights[p] for p in range(len(sizes))))
        parts = [f"n:{i + 1}", f"mse_avg:{mse:0.2f}"]
        parts += [f"mse_{comps[p]}:{comp_mse[p]:0.2f}" for p in range(len(sizes))]
        parts.append(f"psnr_avg:{_fmt2(_psnr(mse, peak))}")
        parts += [f"psnr_{comps[p]}:{_fmt2(_psnr(comp_mse[p], peak))}" for p in range(len(sizes))]
        lines.append(" ".join(parts) + " ")
    return lines


def psnr_values(sse: np.ndarray, plane_sizes, bit_depth: int):
    """per-frame psnr_y (dB; inf when identical) and the plane-weighted average."""
    peak = float((1 << bit_depth) - 1)
    sizes = np.array([w * h for (w, h) in plane_sizes], np.float64)
    mse_p = sse.astype(np.float64) / sizes[None, :]
    mse_avg = (mse_p * (sizes / sizes.sum())[None, :]).sum(1)
    with np.errstate(divide="ignore"):
        psnr_p = np.where(mse_p > 0, 10.0 * np.log10(peak * peak / np.where(mse_p > 0, mse_p, 1.0)), np.inf)
        psnr_avg = np.where(mse_avg > 0, 10.0 * np.log10(peak * peak / np.where(mse_avg > 0, mse_avg, 1.0)), np.inf)
    return psnr_p, psnr_avg


def ssim_all(ssim: np.ndarray, plane_sizes) -> np.ndarray:
    sizes = np.array([w * h for (w, h) in plane_sizes], np.float64)
    return (ssim * (sizes / sizes.sum())[None, :]).sum(1)


def ssim_stats_lines(ssim: np.ndarray, plane_sizes, comps="YUV"):
    """FFmpeg vf_ssim.c stats_file lines.  ssim: [n, planes]."""
    allv = ssim_all(ssim, plane_sizes)
    lines = []
    for i in range(ssim.shape[0]):
        parts = [f"n:{i + 1}"] + [f"{comps[p]}:{ssim[i, p]:f}" for p in range(ssim.shape[1])]
        db = float("inf") if allv[i] >= 1.0 else -10.0 * math.log10(1.0 - allv[i])
        parts.append(f"All:{allv[i]:f} ({'inf' if math.isinf(db) else f'{db:f}'})")
        lines.append(" ".join(parts))
    return lines
