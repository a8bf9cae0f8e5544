"""File pair -> per-frame metrics.  The part of the reference that lived inside the three ffmpeg
children (app/vmaf_analyzer.py:446, :1037, :1067): read both clips, run the extractors on every
frame pair, gather, apply the model.  Works as a single process (world_size 1) or as one rank of a
frame-sharded torch.distributed job (one process per GPU)."""
from __future__ import annotations

import dataclasses
import math
import os
import time
from collections import namedtuple
from contextlib import closing

import numpy as np

from . import _native as N
from . import model as M
from . import report, shard
from .readers import (CHROMA_SITINGS, _ColourReader, _ConvertedReader, _CroppedReader, _DeinterlacedReader, _LevelledReader, _LumaReader,  # noqa: F401
                      _MaskedReader, _RegisteredReader, _ResampledReader, _RgbReader, _ShiftedReader, _TableReader,
                      _WovenReader, _clip_context, _side_context, crop_readers, yuvio_info_444)
from .yuvio import open_video


class ScoreResult(dict):
    """keys: metrics (ordered dict name -> per-frame array), frame_indices, records, info, fps,
    psnr_lines, ssim_lines, model_name"""


def _cap(v: np.ndarray, cap: float) -> np.ndarray:
    return np.minimum(v, cap)


def score_files(reference_path: str, distorted_path: str, model: str | None = "vmaf_v0.6.1", *,
                psnr: bool = True, ssim: bool = True, n_subsample: int = 1, device: int = 0,
                rank: int = 0, world_size: int = 1, gather_device=None, max_batch: int = 0,
                progress=None, cancelled=None, engine_factory=None, raw_kwargs=None,
                fixed_point: int = 0, float_ssim: bool = False, ms_ssim: bool = False,
                ciede: bool = False, cambi: bool = False, cambi_full_ref: bool = False,
                psnr_hvs: bool = False, xpsnr: bool = False, siti: bool = False,
                integrity: bool = False, integrity_options=None, align: int = 0,
                align_frames: int | None = None, align_penalty_mse: float | None = None, spatial_align: int = 0,
                spatial_frames: int = 8, level_align: str | None = None, level_frames: int = 8, level_curve: bool = False,
                resize: str | None = None, register: str | None = None, register_frames: int = 8,
                register_min_px: float = 1.0 / 16, colour_align: str | None = None, colour_frames: int = 8,
                colour_full_range: bool | None = None, active_picture: str | None = None, active_frames: int = 8,
                active_limit: int = 24, active_skip: int = 0, distortion_map: int = 0, distortion_planes: str = "y",
                distortion_dir: str | None = None, distortion_factor=16,
                distortion_min_mse: float = 4.0, spectrum: int = 0, spectrum_planes: str = "y", spectrum_min_mse: float = 1.0,
                spectrum_gain_floor: float = 0.5, temporal: int = 0, temporal_planes: str = "y", temporal_min_mse: float = 1.0,
                temporal_blend_min: float = 1 / 16, temporal_still_mse: float = 0.25,
                temporal_pop_factor: float = 4, coding_grid: bool = False, grid_planes: str = "y", grid_periods=(4, 64),
                grid_z2: float = 25.0, chroma_mismatch: str = "error", chroma_siting: str | None = None,
                rgb_matrix: str | None = None, rgb_range: str | None = None, delta_itp: str | None = None,
                itp_matrix: str | None = None, itp_range: str | None = None, itp_peak: float | None = None,
                itp_threshold: float = 1.0, overlay_mask: str | None = None, overlay_boxes=None, overlay_frames: int = 32,
                overlay_tile: int = 16, overlay_grow: int = 1, overlay_feather: int = 16,
                overlay_share: float = 0.9, field_align: str | None = None, field_frames: int | None = None,
                field_penalty_mse: float | None = None, field_repair: bool = False, deinterlace: str | None = None,
                deinterlace_rate: str = "frame", deinterlace_order: str | None = None,
                deinterlace_side: str = "distorted") -> ScoreResult | None:
    """Returns the ScoreResult on rank 0 (None on other ranks).  `progress(frames_done, frames_total)`
    is called as frames are submitted; `cancelled()` is polled between frames (True -> PqaCancelled).
    `fixed_point`: PQA_FIXED_* mask -- extractors to run in libvmaf's fixed-point arithmetic (include/pqa_vmaf.h).
    `float_ssim` / `ms_ssim`: libvmaf's float_ssim / float_ms_ssim features as extra metric columns (extension record).
    `ciede`: libvmaf's ciede feature as the extra column ciede2000 (needs the chroma planes: a monochrome clip is an error).
    `cambi`: libvmaf's cambi banding index of the distorted luma as the extra column cambi (8- and 10-bit clips);
    `cambi_full_ref` adds cambi_source (the reference's) and cambi_full_reference = max(cambi - cambi_source, 0).
    `psnr_hvs`: libvmaf's psnr_hvs feature as the extra columns psnr_hvs_y / _cb / _cr and psnr_hvs (second extension
    record; needs the chroma planes: a monochrome clip is an error).
    `xpsnr`: FFmpeg's xpsnr filter on every frame as the extra columns xpsnr_y / _u / _v (third extension record; a
    monochrome clip gives xpsnr_y only), its stats-file lines and summary; the second-order temporal term when the clip's
    integer frame rate (fps_num // fps_den) is 32 or more.
    `siti`: FFmpeg's siti filter (ITU-T P.910 SI / TI) of the distorted and of the reference luma on every frame as the
    extra columns siti_si / siti_ti / siti_si_source / siti_ti_source (fourth extension record); a clip whose Y4M header
    says XCOLORRANGE=FULL is taken as full range, any other as limited range.
    `delta_itp` = "pq" | "hlg" | "bt1886": the ITU-R BT.2124 colour difference Delta E ITP of every pixel, for clips with that
    transfer (itp.py; csrc/delta_itp.hip) -- the colour metric that means something on an HDR clip, where `ciede` (BT.709 / sRGB
    into CIELAB) does not.  It runs after every alignment and conversion step, on the clips as scored, in a pass of its own
    over the readers on a small three-plane context, 8 pairs a call, sharded over the ranks like the records (the result does
    not depend on their number).  Adds the per-frame columns delta_e_itp (mean), delta_e_itp_max and itp_above_jnd (share of
    pixels above `itp_threshold`, default 1 = about one just-noticeable difference) and the result's `delta_itp` object: the
    spec used, coefficients included, and itp.summary.  `itp_matrix`: "bt601" | "bt709" | "bt2020" (default bt2020 for pq /
    hlg, rgb.default_matrix(height) for bt1886); `itp_range`: "full" | "limited" (default: the reference header's, else
    limited); `itp_peak`: Lw in cd/m2 for hlg (default 1000) and bt1886 (default 100).  A monochrome clip is an error.  None:
    nothing is measured and nothing is read twice.
    `integrity`: FFmpeg's freezedetect, blackdetect and scdet on the DISTORTED clip (fifth extension record; every plane of
    a colour clip): the extra columns scd_mafd / scd_score / black_ratio / freeze_mafd and, under the result's `integrity`
    key, the event lists freezes / blacks / scene_changes (integrity.py); `integrity_options`: FFmpeg's option names
    (integrity.DEFAULTS).  The black threshold follows the distorted clip's range (XCOLORRANGE=FULL: full range).
    `align` = K > 0: before scoring, the banded cross-frame SSE of the two lumas over the offsets -K ... K (pqa_cross_sse) is
    reduced to the constant frame offset k that pairs the clips (align.best_offset), and reference frame i is scored
    against captured frame i + k over the range where both exist; output frame 0 is the first scored pair.  `align_frames`
    = A limits the search to the first A reference and A + K captured frames (default: both clips whole).  The result's
    `alignment` key holds {offset_frames, offset_seconds, mse, confidence, repeated, dropped, searched} -- repeated /
    dropped from align.frame_map (`align_penalty_mse`: its step cost) are reported, not compensated.  Every rank of a
    sharded run computes the same exact integers from the same frames, so the ranks agree without a collective.
    `align` = 0: no search, the clips are paired as they are.
    `spatial_align` = R > 0 (at most 16): before scoring (after the temporal search, on the pairs it found), the shifted-window
    luma SSE of `spatial_frames` pairs spread evenly over the common range (pqa_shift_sse) is reduced to the whole-pixel
    displacement (dx, dy) of the captured picture (align.best_shift).  `alignment["spatial"]` holds {dx, dy, mse, confidence,
    agreement, at_edge, subpixel_dx, subpixel_dy, searched, frames, applied, chroma_exact}; `applied` = not at_edge and
    (dx, dy) != (0, 0).  When applied, both clips are cropped to the common window and scored at (W - |dx|) x (H - |dy|):
    the reference from (max(0, -dx), max(0, -dy)), the capture from that origin moved by (dx, dy), chroma planes from
    `origin >> shift` of each clip.  `chroma_exact` is false when dx or dy is no multiple of the chroma subsampling: chroma
    is then paired half a chroma sample off.  A scale factor inside the frame and a sub-pixel displacement are not corrected
    (a clip of another frame size: `resize`).
    `spatial_align` = 0: no search, pixel (x, y) meets pixel (x, y).
    `level_align` = "report" or "apply": before scoring (after the temporal and spatial steps, on the pairs and the window
    they produced), the per-level transfer table of `level_frames` pairs spread evenly over the common range
    (pqa_level_stats) is reduced, for every plane the clips have, to the gain and offset of the captured samples and the
    named range conversion they amount to (align.best_levels).  `alignment["levels"]` holds the luma result {gain, offset,
    kind, mismatch, mse_identity, mse_affine, mse_curve, named, map_gain, map_offset, levels_used, frames, degenerate,
    applied} and the same for every plane under `planes` ("y", "u", "v").  "report" changes nothing else: the records are
    those of a run without the option.  "apply" maps every captured plane whose `mismatch` is true through the integer table
    that undoes its chosen map (align.correction_lut, numpy.take on the host) before it is scored; `applied` says so per
    plane.  `level_align` = None: no measurement.
    `level_curve` = True, on top of `level_align`: a transfer-curve mismatch -- a gamma leg, a contrast enhancer, a black
    stretch -- is fitted as a monotone curve of the same table (align.best_curve).  `levels` and every plane under `planes`
    gain {mse_monotone, knots, gamma, curve_degenerate, curve_applied, mse_after}, and `kind` becomes "curve" where the curve
    leaves clearly less error than the map chosen above (gamma: reported only; normalised to the captured clip's range as
    `colour_full_range` is read).  Under "apply" a plane of kind "curve" with `mismatch` is first checked: the inverse table
    (align.curve_lut) is applied to the sampled captured planes on the GPU (pqa_table_apply), pqa_level_stats runs again and
    `mse_after` is the identity MSE of that second table; only if it lies below `mse_identity` does every captured plane go
    through the table before it is scored (`curve_applied` and `applied`), otherwise the plane is left as it is.  Planes of
    another kind keep the host path above.  False: every result and record is what it is without the option.
    `register` = "bilinear", "bicubic" or "lanczos": before scoring (after the temporal and spatial steps, on the pairs and the
    window they produced, and before the levels), the sub-pixel displacement and the scale factor per axis of the captured
    picture are measured on `register_frames` luma pairs spread evenly over the common range -- tile-wise gradient moments
    (pqa_flow_moments) solved coarse to fine by align.register, which resamples the capture with this filter as it goes.
    `alignment["geometry"]` holds {dx, dy, sx, sy, x0_q16, y0_q16, w_q16, h_q16, corner_px, mse_before, mse_after, iterations,
    levels, tile, converged, frames, applied, crop, filter}: the map is X_dis = n/2 + s (X_ref - n/2) + d per axis in edge
    coordinates, with the signs of `spatial` (dx > 0: displaced to the right).  `applied` = converged and corner_px >=
    `register_min_px` and mse_after < mse_before.  When applied, every captured plane is resampled onto the reference grid
    through the window of the map (pqa_resample at equal size; chroma planes with d / 2^shift and the same s -- chroma siting
    is not modelled, as under `resize`), and both clips are cropped to the reference pixels whose source centre lies inside
    the captured frame, the margins `crop` = [left, top, right, bottom] rounded up to the chroma step.  Not applied: the
    records are those of a run without the option.  After `resize` this is a second filter pass over the captured samples,
    in series with the first: the two are not folded into one.  Rotation is not modelled.  `register` = None: no
    measurement.
    `colour_align` = "report" or "apply": before scoring (after the level step, on the readers and the window it produced), the
    cross-plane moments of `colour_frames` pairs spread evenly over the common range (pqa_colour_moments, clipped samples
    masked) are reduced to the 3 x 4 map of the captured (Y, U, V) on the reference's and the named matrix conversion it
    amounts to -- bt601 / bt709 / bt2020 material decoded with one matrix and encoded with another (align.best_colour).
    `colour_full_range`: the range the named maps are formed for; None follows the captured clip's Y4M header (XCOLORRANGE=FULL:
    full range, any other: limited).  `alignment["colour"]` holds {kind, mismatch, cross_plane, degenerate, mse_identity,
    mse_matrix, mse_diagonal, named, matrix, offset, map_matrix, map_offset, planes, samples, samples_masked_share, frames,
    full_range, correction, applied}.  "report" changes nothing else: the records are those of a run without the option.
    "apply", when `mismatch` and `cross_plane` hold and the inverse of the chosen map fits the Q14 matrix of pqa_colour_apply
    (`correction`: its 12 integers, else null), maps every captured frame through that inverse on the GPU before it is scored;
    `applied` says so.  Without `cross_plane` the planes are not coupled and `level_align` is the tool.  A monochrome clip is
    an error.  `colour_align` = None: no measurement.
    `field_align` = "report" or "apply": the FIELD STRUCTURE of the capture -- a progressive programme carried over an
    interlaced link comes back with the rows of one parity from the neighbouring frame (field shift), with both fields in the
    wrong line positions (field swap) or with one field dropped and the other line-doubled (single field).  After the temporal
    search and before the active picture, the luma of the first `field_frames` frames of the common range (None: all of them)
    goes through FeatureEngine.field_moments (pqa_field_moments: the exact squared errors of every captured field against both
    reference fields of the same, the previous and the next frame) in calls of at most 65 frames that overlap by one; every
    rank does the same.  fields.summary reduces them (`field_penalty_mse`: the cost of a change of state, default that of
    `align_penalty_mse`): `alignment["fields"]` holds {kind, state, segments, flips, top, bottom, mse_before, mse_after,
    comb_ratio, static, weavable, frames, transitions, declared, applied, reason}; `declared` = {"reference", "distorted"}: the
    I tags of the Y4M headers (None where there is none), which inform and decide nothing; `reason` = null, "report",
    "progressive", "not weavable" or "too few frames".  "report" changes nothing else: the records are those of a run without
    the option.  "apply" acts only when `weavable` holds and some segment survived as non-identity: the captured clip is
    re-woven on the host from row slices of its own frames (fields.weave_plan, every plane by the same row-parity rule) and
    the reference starts at the plan's first output frame (the object gains `u_lo`, `u_hi` and `unfilled`: the output frames
    [u_lo, u_hi) and the [frame, parity] of every field lost at a flip, which stays as captured).  single_field and
    vertical_shift are reported, never applied.  `field_align` = None: no measurement.
    `active_picture` = "report" or "apply": before the spatial step (after `resize` and the temporal search, on the pairs it
    found), the black bars of both clips are measured on the luma of `active_frames` frames spread evenly over the common
    range: row and column sums (pqa_line_profiles) reduced by align.active_picture -- a line is dark in a frame when its
    mean does not exceed `active_limit` (in 8-bit code values, 0 ... 255), a bar is a run of lines from an edge that are dark
    in every frame that is not black altogether, the outermost `active_skip` lines of an edge counting as dark whatever they
    hold; columns are judged on the active rows only, from a second pass over row-sliced views.  `alignment["active_picture"]`
    holds {reference, distorted, crop, same, mismatch, scale, offset, applied, reason, frames, limit}: `reference` /
    `distorted` = {left, top, right, bottom, window, frames_used, all_dark, bar_noise} of each clip, the rest from
    align.common_window -- `crop` = [left, top, right, bottom], per side the larger bar rounded up to the chroma step;
    `mismatch` when a side differs by more than 16 lines (`scale` and `offset` of the two windows then say what `register`
    or `resize` would have to undo; nothing is cropped); `reason` = null, "no bars", "all dark", "windows differ" or "window
    too small".  "report" changes nothing else: the records are those of a run without the option.  "apply", when `reason`
    is null, cuts both clips to the common rectangle; every later step and the scoring see the cropped clips, and `applied`
    says so.  Bars that are not black, that fade or move, and a scaled picture are not modelled.  `active_picture` = None:
    no measurement.
    `spectrum` = L (1 ... 6): a distortion spectrum of the scored clips -- WHAT KIND of difference they have.  After every
    alignment step, every frame pair of this rank's shard goes through FeatureEngine.band_moments (pqa_band_moments: the second
    moments of L Haar octaves in three orientations) for the luma (`spectrum_planes` = "y") or all three planes ("all"; a
    monochrome clip is an error), in the same pass as the distortion map when both are asked for.  Rank 0 runs the solver
    (pqa2_amd/spectrum.py): `res["spectrum"]` holds {levels, planes: {y | cb | cr: {bands, summary}}, frames}; `bands` per level
    the gain, error, detail loss and added noise of H, V, D and A in 8-bit code values squared, `summary` the shares, the
    bandwidth each way, `kind` (identical, clean: total below `spectrum_min_mse`, loss, noise) and for a loss its `axis`;
    `spectrum_gain_floor` is the gain a band must keep to count as passed.  The luma adds the per-frame metric columns
    `detail_gain_h`, `detail_gain_v` and `noise_mse`.  `spectrum` = 0: nothing is measured and the result has none of it.
    `temporal` = T (8, 16, 32 or 64): the temporal distortion of the scored clips -- whether their MOTION is wrong, which no
    per-frame map or spectrum shows.  After every alignment step, in the same pass as the distortion map and the spectrum when
    those are asked for, every transition of this rank's shard goes through FeatureEngine.temporal_moments
    (pqa_temporal_moments: the exact second-order sums of the frame differences of both clips per T x T tile) for the luma
    (`temporal_planes` = "y") or all three planes ("all"; a monochrome clip is an error); a rank whose chunk starts at frame
    a > 0 also reads frame a - 1.  Rank 0 runs the solver (pqa2_amd/temporal.py): `res["temporal"]` holds {tile, planes:
    {y | cb | cr: {summary, frames}}, frames}; `summary` the temporal gain, loss and noise, the blend weight, the noise where
    the reference stands still (tile transitions that move by at most `temporal_still_mse`), the pops (transitions whose
    noise exceeds `temporal_pop_factor` times the median) with their period and `kind` (identical, clean: temporal MSE below
    `temporal_min_mse`, blend: weight at least `temporal_blend_min`, loss, noise); `frames` one row a transition.  The luma
    adds the per-frame metric columns `temporal_gain`, `temporal_noise_mse` and `blend_weight` (frame 0 has no transition:
    1, 0 and 0, as `motion` is 0 there).  `temporal` = 0: nothing is measured and the result has none of it.
    `coding_grid` = True: whether the difference between the scored clips is a BLOCK GRID, the artefact of an encoder leg.  After
    every alignment step, in the same pass as the distortion map, the spectrum and the temporal distortion when those are asked
    for, every frame pair of this rank's shard goes through FeatureEngine.edge_profiles (pqa_edge_profiles: the exact gradient
    energy of both clips and their cross term per row and column line) for the luma (`grid_planes` = "y") or all three planes
    ("all"; a monochrome clip is an error).  Rank 0 runs the solver (pqa2_amd/grid.py) over the periods `grid_periods` =
    (lo, hi), 4 <= lo <= hi <= 64, accepting from z^2 >= `grid_z2`: `res["coding_grid"]` holds {planes: {y | cb | cr:
    {summary, frames}}}; `summary` the `kind` (identical, none, grid), `block` [Px, Py], `phase` and `aligned` -- phases are in
    the coordinates of the SCORED window, after any crop or shift applied here, not of the file -- and the same search on each
    clip alone (`reference_grid`, `captured_grid`); `frames` one row a frame.  The luma adds the per-frame metric columns
    `blockiness_x` and `blockiness_y` (1 where there is no grid).  False: nothing is measured and the result has none of it.

    `distortion_map` = T (8, 16, 32 or 64): a distortion map of the scored clips -- WHERE inside the frame they differ.  After
    every alignment step, on exactly the readers the scoring loop sees, a second pass reads every frame pair of this rank's
    shard in chunks of 8 through a context of its own and takes the exact second-order sums of every T x T tile
    (pqa_tile_moments) of the luma (`distortion_planes` = "y") or of all three planes ("all"; a monochrome clip is an error).
    The pass reads and uploads both clips a SECOND time: that, and two to three and a half luma PSNR passes a plane, is its
    cost (README).
    Only the clip-summed moments and the tile SSE of every frame are kept; sharded runs gather the SSE with the records'
    transport and rank 0 runs the solver (pqa2_amd/distortion.py) on the whole clip.  `res["distortion"]` holds {tile, grid,
    planes: {y | cb | cr: {grid, defects, persistent, psnr_all, psnr_excluding, concentration_mean, tile_psnr_min_mean,
    worst_frame}}, frames}: `defects` the localised events of distortion.find_defects (a tile is hot when its MSE exceeds
    `distortion_min_mse` in 8-bit code values squared and `distortion_factor` times the frame's median tile MSE), `persistent`
    the regions hot in at least 9 of 10 frames (a burnt-in logo or clock) with the clip PSNR with (`psnr_all`) and without
    them (`psnr_excluding`).  The luma adds the per-frame metric columns `tile_psnr_min` and `distortion_concentration`.
    With `distortion_dir` rank 0 writes distortion_<plane>.pgm (distortion.heatmap_pgm of the clip-mean tile PSNR) and
    distortion_<plane>.npy (the clip-summed moments, uint64 [ty, tx, 6]) there.  `distortion_map` = 0: nothing is measured and
    every output is what it was.
    Packed capture files (.uyvy, .yuyv / .yuy2, .v210; yuvio.PackedReader) are 4:2:2 clips like any other to every step above,
    which read them through a numpy unpack; the scoring loop itself hands a clip that reaches it unwrapped (or only
    frame-shifted) to the GPU as packed bytes in runs of eight (FeatureEngine.submit_packed: unpacked in HBM, bit-identical
    records).  `chroma_mismatch`: "error" (default) refuses clips that differ in pixel format; "luma" accepts clips that differ
    ONLY in chroma subsampling (a 4:2:2 capture against a 4:2:0 master) and scores both as luma-only clips -- VMAF and luma
    PSNR / SSIM, the chroma keys absent as for a monochrome Y4M; a bit-depth difference stays an error, and chroma is not
    converted between layouts.  "convert": when the clips differ in chroma layout OR bit depth (8 / 10 / 12), the DISTORTED clip --
    the side ffmpeg would convert for libvmaf -- is converted on the GPU to the reference's layout, siting and depth, all three
    planes (FeatureEngine.format_convert: one pass, one rounding; triangle taps of this library's own, not swscale's), before
    `resize` and every alignment step, and all three planes are scored; a monochrome clip against a colour clip stays an error.
    The siting of each clip follows its header (yuvio.VideoInfo.chroma_siting); `chroma_siting` = "left" (co-sited
    horizontally, centred vertically), "center" (centred both ways) or "topleft" (co-sited both ways) overrides BOTH clips'
    on their subsampled axes.  Under "convert" a packed file is read through the numpy unpack (`packed_upload` false).  Then,
    under "luma", or when a packed file is read, the result carries `input` = {"reference": pix_fmt, "distorted": pix_fmt,
    "planes_scored": "y" | "yuv", "packed_upload": bool}; a conversion adds "conversion": {"side": "distorted", "from": pix_fmt,
    "to": pix_fmt, "bit_depth": [from, to], "siting": {"from": [h, v], "to": [h, v]}}.
    Packed RGB captures (.bgra, .argb, .rgba, .abgr, .r210; yuvio.RgbReader) have no Y'CbCr form to refuse, so whatever
    `chroma_mismatch` says an RGB clip is converted on the GPU, before any other step reads it, to the OTHER clip's layout, siting
    (`chroma_siting` overrides as above) and depth (8 or 10; a 12-bit partner is a ValueError) in one pass with one rounding
    (FeatureEngine.rgb_convert; matrix and taps of this library's own, not swscale's); two RGB clips both go to 4:4:4 at the
    reference's depth.  `rgb_matrix`: "bt601", "bt709" or "bt2020"; None: bt601 up to 576 lines, else bt709.  `rgb_range`: "full"
    or "limited" R'G'B'; None: full for the 8-bit formats, limited for r210, which is what the cards deliver.  The Y'CbCr range
    follows the partner's header (XCOLORRANGE=FULL: full, else limited).  `input` then carries "conversion": {"side", "from", "to",
    "matrix", "rgb_range", "yuv_range", "bit_depth": [from, to], "siting": {"to": [h, v]}, "coefficients": [12 Q14 integers]} (a
    list of two such objects when both clips are RGB), planes_scored "yuv", packed_upload false.

    `overlay_mask`: None, "report", "neutral" or "reference" -- a burnt-in overlay (a channel logo, a clock, a timecode, an OSD)
    taken out of the scores.  After every alignment step `overlay_frames` frame pairs spread evenly over the clips are read,
    the tile moments of their luma at `overlay_tile` (8, 16, 32 or 64) give the tiles that are hot in at least
    `overlay_share` of them (distortion.hot_tiles, persistent_tiles), and distortion.overlay_mask grows them `overlay_grow`
    tiles and feathers `overlay_feather` luma samples (a multiple of 8) around them; with `overlay_boxes` = [[x0, y0, x1, y1],
    ...] (luma pixels of the scored window, x1 and y1 exclusive) the mask is built from the boxes and nothing is detected.
    Every rank does the same.  "neutral" blends BOTH clips, every plane, towards one constant per plane inside the mask (luma:
    the rounded mean of the sampled reference frames over the masked tiles; chroma: mid-grey) -- a flat region adds nothing
    to VIF and ADM but also removes the reference's motion there, so the score reads slightly low; "reference" leaves the
    reference alone and blends the captured planes towards the reference's own samples -- the region counts as transmitted
    perfectly, so the score reads high.  The blend is FeatureEngine.mask_blend (pqa_mask_blend), and
    everything downstream -- the scores and the map, spectrum, temporal, grid and Delta E ITP passes -- sees the masked clips.
    "report" finds the mask and applies nothing.  The result carries `overlay` = {mode, detected, regions, boxes, share, fill,
    tile, grow, feather, frames_sampled, applied}: `regions` as distortion.persistent_regions gives them, `boxes` the masked
    boxes in pixels, `share` the fraction of luma samples the mask touches, `fill` the constants per plane or "reference",
    `applied` false under "report" and when no tile is persistent.  None: nothing is read or changed and the result has no such
    object.

    `deinterlace`: None, "adaptive" or "intra" -- a clip that really is interlaced (1080i: two moments in time a frame) is
    deinterlaced on the GPU in exact integers (FeatureEngine.deinterlace, pqa_deinterlace: one field of a frame kept, the other
    interpolated from the fields before and after it where the picture is still -- "adaptive" -- or from the kept field alone --
    "intra"), every plane, directly after an RGB clip became Y'CbCr and before any step that works vertically.
    `deinterlace_side`: "distorted" (a progressive master against an interlaced capture) or "both" (an interlaced clip on either
    side).  `deinterlace_rate`: "frame" -- a frame per frame, the first field kept -- or "field" -- a frame per field: twice the
    frames at twice the frame rate (a 50p master against a 25i capture).  `deinterlace_order`: "tff" or "bff", the field that comes
    first in time; None reads the clip's own Y4M I tag (t / b), and a clip without one is a ValueError.  `input` then carries
    "deinterlace": {"side", "mode", "rate", "order", "declared": {"reference", "distorted"}, "frames": [from, to]} (the frames of
    the deinterlaced clip(s) before and after).  None: nothing changes.
    `field_repair` (with field_align="apply"): when the field structure found is single_field for the whole clip -- one field was
    dropped and the other line-doubled --, the captured clip goes through deinterlace mode "intra" keeping the parity that both
    captured parities show, and `fields` carries applied true and repair "intra".  False: single_field is reported only."""
    from .engine import FeatureEngine
    make_side = engine_factory or FeatureEngine
    make = engine_factory or (lambda *aa, **kw: FeatureEngine(*aa, reuse=True, **kw))   # a parked context of this configuration
    raw_kwargs = raw_kwargs or {}
    st = _Clips(open_video(reference_path, **raw_kwargs), open_video(distorted_path, **raw_kwargs), device, make_side)
    _check_formats(chroma_mismatch, chroma_siting, rgb_matrix, rgb_range)
    _check_deinterlace(deinterlace, deinterlace_rate, deinterlace_order, deinterlace_side)
    _wrap_rgb(st, chroma_siting, rgb_matrix, rgb_range)
    _deinterlace(st, deinterlace, deinterlace_rate, deinterlace_order, deinterlace_side)   # nothing vertical may touch woven fields
    _match_chroma(st, chroma_mismatch, chroma_siting)
    _match_size(st, resize)
    _align_time(st, align, align_frames, align_penalty_mse)
    _align_fields(st, field_align, field_frames, field_penalty_mse, field_repair)
    _crop_active(st, active_picture, active_frames, active_limit, active_skip)
    _align_shift(st, spatial_align, spatial_frames)
    _register(st, register, register_frames, register_min_px)
    _align_levels(st, level_align, level_frames, level_curve)
    _align_colour(st, colour_align, colour_frames, colour_full_range)
    _mask_overlay(st, overlay_mask, overlay_boxes, overlay_frames, overlay_tile, overlay_grow, overlay_feather, overlay_share)
    passes = dict(distortion_map=distortion_map, distortion_planes=distortion_planes, distortion_factor=distortion_factor,
                  distortion_min_mse=distortion_min_mse, distortion_dir=distortion_dir, spectrum=spectrum, spectrum_planes=spectrum_planes,
                  spectrum_min_mse=spectrum_min_mse, spectrum_gain_floor=spectrum_gain_floor, temporal=temporal,
                  temporal_planes=temporal_planes, temporal_min_mse=temporal_min_mse, temporal_blend_min=temporal_blend_min,
                  temporal_still_mse=temporal_still_mse, temporal_pop_factor=temporal_pop_factor, coding_grid=coding_grid,
                  grid_planes=grid_planes, grid_periods=grid_periods, grid_z2=grid_z2)
    n, periods, itp_spec = _check_passes(st, delta_itp=delta_itp, itp_matrix=itp_matrix, itp_range=itp_range, itp_peak=itp_peak,
                                         itp_threshold=itp_threshold, **passes)
    flags = dict(float_ssim=float_ssim, ms_ssim=ms_ssim, ciede=ciede, cambi=cambi, cambi_full_ref=cambi_full_ref,
                 psnr_hvs=psnr_hvs, xpsnr=xpsnr, siti=siti)
    plan = _feature_mask(st, model, psnr=psnr, ssim=ssim, integrity=integrity, integrity_options=integrity_options, **flags)
    a, b = shard.shard_bounds(n, world_size, rank)
    t_start = time.perf_counter()
    local, local_blk = _score_shard(st, make, plan, a, b, max_batch=max_batch, n_subsample=n_subsample, fixed_point=fixed_point,
                                    xpsnr=xpsnr, siti=siti, integrity=integrity, progress=progress, cancelled=cancelled)
    to = (world_size, rank, gather_device)
    measured = _run_passes(st, a, b, n, to, cancelled, itp_spec, **passes)
    rec = shard.gather_records(local, n, *to)
    blk = {i: shard.gather_records(local_blk[i], n, *to, width=N.EXT_BLOCKS[i][1]) for i in plan.want}
    if rank != 0:
        st.close()
        return None
    ig_result = _integrity_events(st, make, blk.pop(plan.want[-1]), n, plan.n_planes, plan.ig_opts) if integrity else None   # the last block
    elapsed = time.perf_counter() - t_start
    res = _result(st, rec, blk, plan, flags, ig_result, measured, periods, itp_spec, psnr=psnr, ssim=ssim, n_subsample=n_subsample,
                  fps=n / elapsed if elapsed > 0 else 0.0, **passes)
    st.close()   # on an error their contexts go with the readers
    return res


# what _feature_mask settles: model, planes to score, PQA_FEAT_* mask, extension blocks (N.EXT_BLOCKS) to collect, integrity's two
_Plan = namedtuple("_Plan", "mdl n_planes feats want ig_opts ig_thr")


def _score_shard(st: _Clips, make, plan: _Plan, a: int, b: int, *, max_batch, n_subsample, fixed_point, xpsnr, siti, integrity,
                 progress, cancelled):
    """frames [a, b) through a scoring context: (their records, {i: the rows of extension block i}).  An error closes the
    context; a healthy one is parked for the next analysis of this geometry"""
    ri, mdl = st.ri, plan.mdl
    eng = make(ri.width, ri.height, bit_depth=ri.bit_depth, n_planes=plan.n_planes,
               chroma_shift=(ri.hshift, ri.vshift), features=plan.feats, device=st.device, max_batch=max_batch,
               result_capacity=max(b - a, 16), n_subsample=n_subsample,
               vif_enhn_gain_limit=mdl.vif_enhn_gain_limit, adm_enhn_gain_limit=mdl.adm_enhn_gain_limit,
               vif_border=mdl.vif_border, **({"fixed_point": int(fixed_point)} if fixed_point else {}))
    try:
        _arm_histories(st, eng, a, plan.n_planes, xpsnr, siti, integrity, plan.ig_thr)
        _submit_frames(st, eng, a, b, plan.n_planes, progress, cancelled)
        got = _collect(eng, a, b, plan.want)
    except BaseException:
        eng.close()
        raise
    (eng.release if hasattr(eng, "release") else eng.close)()
    return got


def _run_passes(st: _Clips, a: int, b: int, n: int, to, cancelled, itp_spec, *, distortion_map, distortion_planes, spectrum,
                spectrum_planes, temporal, temporal_planes, coding_grid, grid_planes, **_):
    """(dmap, bands, tmom, edges, itp_rows), None where not asked for: the passes of their own over the readers the scoring
    loop saw, after the scoring context is parked.  to: (world_size, rank, gather_device)"""
    dmap = bands = tmom = edges = itp_rows = None
    if distortion_map or spectrum or temporal or coding_grid:      # ONE pass for the four of them
        dmap, bands, tmom, edges = _distortion_pass(st.ref, st.dis, a, b, n, int(distortion_map), 3 if distortion_planes == "all" else 1,
                                                    st.device, st.make, *to, cancelled, levels=int(spectrum),
                                                    band_planes=3 if spectrum_planes == "all" else 1, temporal_tile=int(temporal),
                                                    temporal_planes=3 if temporal_planes == "all" else 1,
                                                    edge_planes=(3 if grid_planes == "all" else 1) if coding_grid else 0)
    if itp_spec is not None:      # every pixel of every plane, on the clips as scored
        itp_rows = _itp_pass(st.ref, st.dis, a, b, n, itp_spec, st.device, st.make, *to, cancelled)
    return dmap, bands, tmom, edges, itp_rows


def _result(st: _Clips, rec, blk, plan: _Plan, flags: dict, ig_result, measured, periods, itp_spec, *, psnr, ssim, n_subsample, fps,
            distortion_map, distortion_factor, distortion_min_mse, distortion_dir, spectrum, spectrum_min_mse, spectrum_gain_floor,
            temporal, temporal_min_mse, temporal_blend_min, temporal_still_mse, temporal_pop_factor, grid_z2, **_) -> ScoreResult:
    """rank 0: finish_records on the gathered rows, the solvers on what _run_passes measured, the objects the steps left in `st`"""
    ri = st.ri
    extra = {N.EXT_BLOCKS[i][0]: rows for i, rows in blk.items()}   # finish_records takes a block under its name in the table
    extra.update({k: True for k, v in flags.items() if v})
    if ig_result is not None:
        extra.update(integrity=ig_result)
    res = finish_records(rec, plan.mdl, ri, psnr=psnr, ssim=ssim, n_subsample=n_subsample, n_planes=plan.n_planes, fps=fps, **extra)
    dmap, bands, tmom, edges, itp_rows = measured
    if dmap is not None:
        _distortion_result(res, dmap, ri, int(distortion_map), distortion_factor, distortion_min_mse, distortion_dir)
    if bands is not None:
        _spectrum_result(res, bands, ri, int(spectrum), spectrum_min_mse, spectrum_gain_floor)
    if tmom is not None:
        _temporal_result(res, tmom, ri, int(temporal), temporal_min_mse, temporal_blend_min, temporal_still_mse, temporal_pop_factor)
    if edges is not None:
        _grid_result(res, edges, ri, periods, grid_z2)
    if itp_rows is not None:
        _itp_result(res, itp_rows, itp_spec)
    for key in ("alignment", "resize", "input", "overlay"):
        if getattr(st, key) is not None:
            res[key] = getattr(st, key)
    return res


@dataclasses.dataclass
class _Clips:
    """What the steps of score_files hand on: the two readers as the next step is to read them, the objects the result
    reports, and the wrapped readers that own a GPU context, in the order they were made."""
    ref: object
    dis: object
    device: object
    make: object                   # the maker of the small side contexts
    alignment: dict | None = None
    input: dict | None = None
    resize: dict | None = None
    overlay: dict | None = None
    owned: list = dataclasses.field(default_factory=list)

    ri = property(lambda self: self.ref.info)
    di = property(lambda self: self.dis.info)

    def own(self, reader):      # a reader with a context of its own: close() reaches it
        self.owned.append(reader)
        return reader

    def close(self):
        for rd in self.owned:
            rd.close()


def _check_formats(chroma_mismatch, chroma_siting, rgb_matrix, rgb_range) -> None:
    from . import rgb as RGB
    from .align import COLOUR_STANDARDS
    if chroma_mismatch not in ("error", "luma", "convert"):
        raise ValueError('chroma_mismatch must be "error" or "luma" or "convert"')
    if chroma_siting is not None and chroma_siting not in CHROMA_SITINGS:
        raise ValueError('chroma_siting must be None, "left", "center" or "topleft"')
    if rgb_matrix is not None and rgb_matrix not in COLOUR_STANDARDS:
        raise ValueError(f"rgb_matrix must be None or one of {sorted(COLOUR_STANDARDS)}")
    if rgb_range is not None and rgb_range not in RGB.RANGES:
        raise ValueError('rgb_range must be None, "full" or "limited"')


def _wrap_rgb(st: _Clips, siting, matrix, rgb_range) -> None:
    """a packed RGB clip becomes Y'CbCr planes in its partner's format; `input` for every packed file"""
    from . import rgb as RGB
    ri, di = st.ri, st.di
    if ri.packed in RGB.FORMATS or di.packed in RGB.FORMATS:
        both = ri.packed in RGB.FORMATS and di.packed in RGB.FORMATS
        plain = yuvio_info_444(ri) if both else None       # two RGB clips: 4:4:4 at the reference's depth
        conversions = []
        if ri.packed in RGB.FORMATS:
            st.ref = st.own(_RgbReader(st.ref, plain or di, siting, st.device, st.make, matrix, rgb_range, "reference"))
            conversions.append(st.ref.conversion)
        if di.packed in RGB.FORMATS:
            st.dis = st.own(_RgbReader(st.dis, plain or ri, siting, st.device, st.make, matrix, rgb_range, "distorted"))
            conversions.append(st.dis.conversion)
        st.input = {"reference": ri.pix_fmt, "distorted": di.pix_fmt, "planes_scored": "yuv", "packed_upload": False,
                    "conversion": conversions[0] if len(conversions) == 1 else conversions}
    elif ri.packed or di.packed:
        st.input = {"reference": ri.pix_fmt, "distorted": di.pix_fmt, "planes_scored": None, "packed_upload": False}


DEINTERLACE_ORDERS = {"tff": 0, "bff": 1}      # deinterlace_order= -> the parity of the rows that come first in time
_ORDER_TAGS = {"t": "tff", "b": "bff"}         # the Y4M I tag


def _check_deinterlace(mode, rate, order, side) -> None:
    if mode is not None and mode not in N.DEINT_MODES:
        raise ValueError(f"deinterlace must be None or one of {sorted(N.DEINT_MODES)}")
    if rate not in N.DEINT_RATES:
        raise ValueError(f"deinterlace_rate must be one of {sorted(N.DEINT_RATES)}")
    if order is not None and order not in DEINTERLACE_ORDERS:
        raise ValueError(f"deinterlace_order must be None or one of {sorted(DEINTERLACE_ORDERS)}")
    if side not in ("distorted", "both"):
        raise ValueError('deinterlace_side must be "distorted" or "both"')


def _deinterlace(st: _Clips, mode, rate, order, side) -> None:
    """deinterlace=: the distorted clip, or both, through the GPU deinterlacer; `input` reports it"""
    if mode is None:
        return
    ri, di = st.ri, st.di
    sides = ("reference", "distorted") if side == "both" else ("distorted",)
    orders = {}
    for name, info in (("reference", ri), ("distorted", di)):
        if name in sides:
            orders[name] = order or _ORDER_TAGS.get(info.interlace)
            if orders[name] is None:
                raise ValueError(f"the {name} clip's header names no field order (I tag {info.interlace!r}): deinterlace_order must say tff or bff")
    before = len(st.dis)
    if side == "both":
        st.ref = st.own(_DeinterlacedReader(st.ref, mode, DEINTERLACE_ORDERS[orders["reference"]], rate, st.device, st.make))
    st.dis = st.own(_DeinterlacedReader(st.dis, mode, DEINTERLACE_ORDERS[orders["distorted"]], rate, st.device, st.make))
    st.input = dict(st.input or {"reference": ri.pix_fmt, "distorted": di.pix_fmt, "planes_scored": None, "packed_upload": False})
    st.input["deinterlace"] = {"side": side, "mode": mode, "rate": rate, "order": orders["distorted"],
                               "declared": {"reference": ri.interlace, "distorted": di.interlace},
                               "frames": [before, len(st.dis)]}


def _match_chroma(st: _Clips, mode: str, siting) -> None:
    """chroma_mismatch: "luma" scores both clips as luma-only clips, "convert" takes the distorted clip to the reference's
    layout, siting and depth"""
    ri, di = st.ri, st.di
    kept = {k: v for k, v in (st.input or {}).items() if k == "deinterlace"}      # what the step before reported
    if (mode == "luma" and ri.bit_depth == di.bit_depth
            and (ri.hshift, ri.vshift, ri.mono) != (di.hshift, di.vshift, di.mono)):
        st.input = {"reference": ri.pix_fmt, "distorted": di.pix_fmt, "planes_scored": "y", "packed_upload": False, **kept}
        st.ref, st.dis = _LumaReader(st.ref), _LumaReader(st.dis)
    if (mode == "convert" and ri.mono == di.mono and not ri.mono
            and ri.bit_depth in N.CONVERT_BIT_DEPTHS and di.bit_depth in N.CONVERT_BIT_DEPTHS
            and (ri.hshift, ri.vshift, ri.bit_depth) != (di.hshift, di.vshift, di.bit_depth)):
        st.dis = converter = st.own(_ConvertedReader(st.dis, ri, siting, st.device, st.make))
        st.input = {"reference": ri.pix_fmt, "distorted": di.pix_fmt, "planes_scored": "yuv", "packed_upload": False,
                    "conversion": {"side": "distorted", "from": di.pix_fmt, "to": converter.info.pix_fmt,
                                   "bit_depth": [di.bit_depth, ri.bit_depth],
                                   "siting": {"from": list(converter.src_siting), "to": list(converter.dst_siting)}}, **kept}


def _match_size(st: _Clips, resize) -> None:
    """the clips must agree in size and pixel format by now; resize= takes the distorted clip to the reference's size"""
    ri, di = st.ri, st.di
    if resize is not None and resize not in N.RESAMPLE_FILTERS:
        raise ValueError(f"resize must be None or one of {sorted(N.RESAMPLE_FILTERS)}")
    if resize is None and (ri.width, ri.height) != (di.width, di.height):
        raise ValueError(f"reference is {ri.width}x{ri.height} but distorted is {di.width}x{di.height}")
    if ri.bit_depth != di.bit_depth or (ri.hshift, ri.vshift, ri.mono) != (di.hshift, di.vshift, di.mono):
        raise ValueError("reference and distorted clips differ in pixel format")
    if resize is not None:
        st.resize = {"filter": resize, "from": [di.width, di.height], "to": [ri.width, ri.height],
                     "applied": (ri.width, ri.height) != (di.width, di.height)}
        if st.resize["applied"]:
            st.dis = st.own(_ResampledReader(st.dis, ri, resize, st.device, st.make))


def _align_time(st: _Clips, align, align_frames, penalty_mse) -> None:
    if align:
        if align < 0 or align > 64:
            raise ValueError("align must be 0 ... 64 frames")
        st.alignment = _find_alignment(st.ref, st.dis, int(align), align_frames, penalty_mse, st.device, st.make)
        k = st.alignment["offset_frames"]
        st.ref, st.dis = _ShiftedReader(st.ref, max(0, -k)), _ShiftedReader(st.dis, max(0, k))


def _align_fields(st: _Clips, mode, frames, penalty_mse, repair=False) -> None:
    if repair and mode != "apply":
        raise ValueError('field_repair needs field_align="apply"')
    if mode is not None:
        if mode not in ("report", "apply"):
            raise ValueError('field_align must be None, "report" or "apply"')
        if frames is not None and frames < 3:
            raise ValueError("field_frames must be None or at least 3")
        if penalty_mse is not None and not penalty_mse >= 0:
            raise ValueError("field_penalty_mse must not be negative")
        if st.ri.height < 2:
            raise ValueError("field_align needs a frame of at least two rows")
        fields, plan = _find_fields(st.ref, st.dis, frames, penalty_mse, mode == "apply", st.device, st.make)
        st.alignment = dict(st.alignment or {}, fields=fields)
        if fields["applied"]:
            st.ref, st.dis = _ShiftedReader(st.ref, plan["u_lo"]), _WovenReader(st.dis, plan)
        elif repair and fields["segments"] and all(g["kind"] == "single_field" and g["state"][0] == fields["state"][0]
                                                      and g["state"][1] == g["state"][3] == 0 for g in fields["segments"]):
            # one field was dropped and the other line-doubled: keep the parity both captured parities show, interpolate the other
            st.dis = st.own(_DeinterlacedReader(st.dis, "intra", fields["state"][0], "frame", st.device, st.make))
            fields.update(applied=True, reason=None, repair="intra")


def _crop_window(st: _Clips, crop, dis_rd=None) -> None:
    """both clips cut by the margins [left, top, right, bottom] (dis_rd: the captured clip to cut, when a step has just made it)"""
    left, top, right, bottom = crop
    cw, ch = st.ri.width - left - right, st.ri.height - top - bottom
    st.ref, st.dis = _CroppedReader(st.ref, left, top, cw, ch), _CroppedReader(st.dis if dis_rd is None else dis_rd, left, top, cw, ch)


def _crop_active(st: _Clips, mode, frames, limit, skip) -> None:
    if mode is not None:
        if mode not in ("report", "apply"):
            raise ValueError('active_picture must be None, "report" or "apply"')
        if frames is None or frames < 1:
            raise ValueError("active_frames must be positive")
        if limit is None or not 0 <= limit <= 255:
            raise ValueError("active_limit must be 0 ... 255")
        if skip is None or skip < 0:
            raise ValueError("active_skip must not be negative")
        active = _find_active(st.ref, st.dis, int(frames), int(limit), int(skip), mode == "apply", st.device, st.make)
        st.alignment = dict(st.alignment or {}, active_picture=active)
        if active["applied"]:
            _crop_window(st, active["crop"])


def _align_shift(st: _Clips, R, frames) -> None:
    if R:
        if R < 0 or R > 16:
            raise ValueError("spatial_align must be 0 ... 16 pixels")
        if frames is None or frames < 1:
            raise ValueError("spatial_frames must be positive")
        if st.ri.width <= 2 * R or st.ri.height <= 2 * R:
            raise ValueError(f"spatial_align {R} needs a frame larger than {2 * R} pixels each way")
        spatial = _find_shift(st.ref, st.dis, int(R), int(frames), st.device, st.make)
        st.alignment = dict(st.alignment or {}, spatial=spatial)
        if spatial["applied"]:
            st.ref, st.dis = crop_readers(st.ref, st.dis, spatial["dx"], spatial["dy"])


def _register(st: _Clips, filter, frames, min_px) -> None:
    if filter is not None:
        if filter not in N.RESAMPLE_FILTERS:
            raise ValueError(f"register must be None or one of {sorted(N.RESAMPLE_FILTERS)}")
        if frames is None or frames < 1:
            raise ValueError("register_frames must be positive")
        if min_px is None or not min_px >= 0:
            raise ValueError("register_min_px must not be negative")
        geometry = _find_geometry(st.ref, st.dis, filter, int(frames), float(min_px), st.device, st.make)
        st.alignment = dict(st.alignment or {}, geometry=geometry)
        if geometry["applied"]:
            _crop_window(st, geometry["crop"], st.own(_RegisteredReader(st.dis, geometry, st.device, st.make)))


def _align_levels(st: _Clips, mode, frames, curve) -> None:
    if mode is not None:
        if mode not in ("report", "apply"):
            raise ValueError('level_align must be None, "report" or "apply"')
        if frames is None or frames < 1:
            raise ValueError("level_frames must be positive")
        levels, luts, curves = _find_levels(st.ref, st.dis, int(frames), mode == "apply", st.device, st.make,
                                            curve=bool(curve), full_range=st.di.color_range == "full")
        st.alignment = dict(st.alignment or {}, levels=levels)
        if any(lut is not None for lut in luts):
            st.dis = _LevelledReader(st.dis, luts)
        if any(t is not None for t in curves):
            st.dis = st.own(_TableReader(st.dis, curves, st.device, st.make))
    elif curve:
        raise ValueError('level_curve needs level_align="report" or "apply"')


def _align_colour(st: _Clips, mode, frames, full_range) -> None:
    if mode is not None:
        if mode not in ("report", "apply"):
            raise ValueError('colour_align must be None, "report" or "apply"')
        if frames is None or frames < 1:
            raise ValueError("colour_frames must be positive")
        if st.ri.mono:
            raise ValueError("colour alignment needs the chroma planes, but the clips are monochrome")
        full = (st.di.color_range == "full") if full_range is None else bool(full_range)
        colour = _find_colour(st.ref, st.dis, int(frames), mode == "apply", full, st.device, st.make)
        st.alignment = dict(st.alignment or {}, colour=colour)
        if colour["applied"]:
            st.dis = st.own(_ColourReader(st.dis, colour["correction"], st.device, st.make))


def _mask_overlay(st: _Clips, mode, boxes, frames, tile, grow, feather, share) -> None:
    if mode is not None or boxes is not None:
        if mode not in ("report", "neutral", "reference"):
            raise ValueError('overlay_mask must be None, "report", "neutral" or "reference"')
        if frames is None or frames < 1:
            raise ValueError("overlay_frames must be positive")
        if tile not in N.FLOW_TILES:
            raise ValueError("overlay_tile must be a tile size of 8, 16, 32 or 64")
        if grow is None or grow < 0:
            raise ValueError("overlay_grow must not be negative")
        if feather is None or feather < 0 or feather % OVERLAY_NODE:
            raise ValueError(f"overlay_feather must be a multiple of {OVERLAY_NODE}, or 0")
        if share is None or not 0 < share <= 1:
            raise ValueError("overlay_share must lie in (0, 1]")
        st.overlay, mask = _find_overlay(st.ref, st.dis, mode, boxes, int(frames), int(tile), int(grow), int(feather), share,
                                         st.device, st.make)
        if st.overlay["applied"] and mode == "neutral":
            st.ref, st.dis = [st.own(_MaskedReader(rd, mask, st.overlay["fill"], None, st.device, st.make)) for rd in (st.ref, st.dis)]
        elif st.overlay["applied"]:
            st.dis = st.own(_MaskedReader(st.dis, mask, None, st.ref, st.device, st.make))


def _check_planes(name: str, value, mono: bool) -> None:
    if value not in ("y", "all"):
        raise ValueError(f'{name} must be "y" or "all"')
    if value == "all" and mono:
        raise ValueError(f'{name}="all" needs the chroma planes, but the clips are monochrome')


def _check_passes(st: _Clips, *, distortion_map, distortion_planes, distortion_factor, distortion_min_mse, spectrum, spectrum_planes,
                  spectrum_min_mse, spectrum_gain_floor, temporal, temporal_planes, temporal_min_mse, temporal_blend_min,
                  temporal_still_mse, temporal_pop_factor, coding_grid, grid_planes, grid_periods, grid_z2, delta_itp, itp_matrix,
                  itp_range, itp_peak, itp_threshold, **_):
    """(the number of frame pairs, the grid periods to search or None, the Delta E ITP spec or None): the options of the
    passes that run after the scoring, checked on the clips as every alignment step left them"""
    ri = st.ri
    n = min(len(st.ref), len(st.dis))
    if n <= 0:
        raise ValueError("no frames to analyse")
    if distortion_map:
        if distortion_map not in N.FLOW_TILES:
            raise ValueError("distortion_map must be 0 or a tile size of 8, 16, 32 or 64")
        _check_planes("distortion_planes", distortion_planes, ri.mono)
        if distortion_factor is None or distortion_factor < 0 or distortion_min_mse is None or distortion_min_mse < 0:
            raise ValueError("distortion_factor and distortion_min_mse must not be negative")
    if spectrum is None or isinstance(spectrum, bool) or int(spectrum) != spectrum or not 0 <= spectrum <= 6:
        raise ValueError("spectrum must be 0 or a number of levels, 1 ... 6")
    if spectrum:
        _check_planes("spectrum_planes", spectrum_planes, ri.mono)
        if spectrum_min_mse is None or spectrum_min_mse < 0 or spectrum_gain_floor is None or spectrum_gain_floor < 0:
            raise ValueError("spectrum_min_mse and spectrum_gain_floor must not be negative")
    if temporal is None or isinstance(temporal, bool) or (temporal and temporal not in N.FLOW_TILES):
        raise ValueError("temporal must be 0 or a tile size of 8, 16, 32 or 64")
    if temporal:
        _check_planes("temporal_planes", temporal_planes, ri.mono)
        if any(v is None or v < 0 for v in (temporal_min_mse, temporal_blend_min, temporal_still_mse, temporal_pop_factor)):
            raise ValueError("temporal_min_mse, temporal_blend_min, temporal_still_mse and temporal_pop_factor must not be negative")
    periods = None
    if coding_grid:
        _check_planes("grid_planes", grid_planes, ri.mono)
        try:
            g_lo, g_hi = (int(v) for v in grid_periods)
        except (TypeError, ValueError):
            raise ValueError("grid_periods must be a pair (lo, hi) with 4 <= lo <= hi <= 64") from None
        if g_lo < 4 or g_hi < g_lo or g_hi > 64:
            raise ValueError("grid_periods must be a pair (lo, hi) with 4 <= lo <= hi <= 64")
        if grid_z2 is None or grid_z2 < 0:
            raise ValueError("grid_z2 must not be negative")
        periods = range(g_lo, g_hi + 1)
    itp_spec = None
    if delta_itp is not None:
        from . import itp as ITP
        if delta_itp not in ITP.TRANSFERS:
            raise ValueError('delta_itp must be None, "pq", "hlg" or "bt1886"')
        if ri.mono:
            raise ValueError("delta_itp needs the chroma planes, but the clips are monochrome")
        if itp_range not in (None, "full", "limited"):
            raise ValueError('itp_range must be None, "full" or "limited"')
        itp_full = (ri.color_range == "full") if itp_range is None else itp_range == "full"
        itp_spec = ITP.spec(delta_itp, itp_matrix, itp_full, ri.bit_depth, itp_peak, itp_threshold, height=ri.height)
    return n, periods, itp_spec


def _feature_mask(st: _Clips, model, *, psnr, ssim, integrity, integrity_options, float_ssim, ms_ssim, ciede, cambi, cambi_full_ref,
                  psnr_hvs, xpsnr, siti):
    """the _Plan of the scoring context: the checks of the feature options, the model, the planes and the feature mask"""
    from . import integrity as IG
    ri, di = st.ri, st.di
    if cambi_full_ref and not cambi:
        raise ValueError("cambi_full_ref needs cambi")
    if ciede and ri.mono:
        raise ValueError("ciede2000 needs the chroma planes, but the clips are monochrome")
    if psnr_hvs and ri.mono:
        raise ValueError("psnr_hvs needs the chroma planes, but the clips are monochrome")
    mdl = M.load_model(model)
    side = (psnr or ssim or ciede or psnr_hvs or xpsnr or integrity)
    n_planes = 1 if (ri.mono or not side) else 3
    feats = N.FEAT_VMAF | (N.FEAT_PSNR if psnr else 0) | (N.FEAT_SSIM if ssim else 0)
    want_ext = bool(float_ssim or ms_ssim or ciede or cambi)
    if want_ext:
        feats |= (N.FEAT_FLOAT_SSIM if float_ssim else 0) | (N.FEAT_MS_SSIM if ms_ssim else 0) | (N.FEAT_CIEDE if ciede else 0)
        feats |= (N.FEAT_CAMBI if cambi else 0) | (N.FEAT_CAMBI_FULL_REF if cambi_full_ref else 0)
    if psnr_hvs:
        feats |= N.FEAT_PSNR_HVS
    if xpsnr:
        feats |= N.FEAT_XPSNR | (N.FEAT_XPSNR_HFR if xpsnr_hfr(ri) else 0)
    if siti:
        feats |= N.FEAT_SITI | (N.FEAT_SITI_REF_FULL if ri.color_range == "full" else 0)
        feats |= N.FEAT_SITI_DIS_FULL if di.color_range == "full" else 0
    ig_opts = ig_thr = None
    if integrity:
        feats |= N.FEAT_INTEGRITY
        ig_opts = IG.options(integrity_options)
        ig_thr = IG.black_threshold(di.bit_depth, di.color_range == "full", ig_opts["pixel_black_th"])
    want = [i for i, on in enumerate((want_ext, psnr_hvs, xpsnr, siti, integrity)) if on]
    return _Plan(mdl, n_planes, feats, want, ig_opts, ig_thr)


def _arm_histories(st: _Clips, eng, a: int, n_planes: int, xpsnr, siti, integrity, ig_thr) -> None:
    """a rank whose chunk starts at frame a > 0 continues from the frames in front of it"""
    ref_rd, dis_rd = st.ref, st.dis
    if a > 0 and xpsnr:   # xpsnr's temporal term reads two frames back: frames a-1 and a-2 (motion's halo is a-1)
        eng.set_ref_history([ref_rd.frame(a - 1)[0]] + ([ref_rd.frame(a - 2)[0]] if a >= 2 else []))
    elif a > 0:
        eng.set_motion_halo(ref_rd.frame(a - 1)[0])   # one-frame halo in front of this rank's chunk
    if integrity:
        eng.set_black_threshold(ig_thr)
    if a > 0 and integrity:   # the differences continue from every plane of the distorted frame a-1 (siti's TI too)
        eng.set_dis_history_planes(dis_rd.frame(a - 1)[:n_planes])
    elif a > 0 and siti:    # siti's TI of the distorted clip continues from its frame a-1 (the reference's: the halo)
        eng.set_dis_history(dis_rd.frame(a - 1)[0])


def _submit_frames(st: _Clips, eng, a: int, b: int, n_planes: int, progress, cancelled) -> None:
    """frames [a, b) of both clips into the scoring context, by the cheapest route the readers offer"""
    ref_rd, dis_rd = st.ref, st.dis
    # both clips are files of packed planes (.y4m): the library reads them straight into its pinned staging (pqa_submit_fd:
    # one copy, no page faults) instead of copying frames out of the readers' mappings
    by_fd = all(hasattr(r, "fileno") and hasattr(r, "plane_offsets") for r in (ref_rd, dis_rd)) and hasattr(eng, "submit_file")
    # ... and a run of frames that lie equally spaced in both files goes down in ONE call (pqa_submit_fd_run: reading frame
    # k + 1 overlaps the upload of frame k inside the library); 8 = a staging half, and the grain of progress / cancel
    by_run = (by_fd and hasattr(eng, "submit_file_run") and all(hasattr(r, "run_stride") for r in (ref_rd, dis_rd))
              and os.environ.get("PQA_FD_RUN", "1") != "0")   # PQA_FD_RUN=0: frame by frame (A/B partner)
    # a packed capture file that reaches this loop unwrapped goes down as packed bytes, 8 frames a call (pqa_submit_packed)
    by_packed = hasattr(eng, "submit_packed") and any(hasattr(r, "packed_frame") for r in (ref_rd, dis_rd))
    if st.input is not None:
        st.input["packed_upload"] = bool(by_packed)
        st.input["planes_scored"] = "y" if n_planes == 1 else "yuv"
    i = a
    while i < b:
        if cancelled is not None and cancelled():
            eng.cancel()
            raise N.PqaCancelled(N.PQA_ECANCELLED, "cancelled")
        m = 1
        if by_packed:
            m = min(8, b - i)
            eng.submit_packed(i, *[([r.packed_frame(j) for j in range(i, i + m)], r.info.packed) if hasattr(r, "packed_frame")
                                   else ([r.frame(j)[:n_planes] for j in range(i, i + m)], None) for r in (ref_rd, dis_rd)])
        else:
            if by_run:
                m = min(8, b - i)
                rs, ds = ref_rd.run_stride(i, m), dis_rd.run_stride(i, m)
                if rs is None or ds is None:
                    m = 1
            if m > 1:
                eng.submit_file_run(i, m, ref_rd.fileno(), ref_rd.plane_offsets(i)[:n_planes], rs,
                                    dis_rd.fileno(), dis_rd.plane_offsets(i)[:n_planes], ds)
            elif by_fd:
                eng.submit_file(i, ref_rd.fileno(), ref_rd.plane_offsets(i)[:n_planes], dis_rd.fileno(), dis_rd.plane_offsets(i)[:n_planes])
            else:
                eng.submit(i, ref_rd.frame(i)[:n_planes], dis_rd.frame(i)[:n_planes])
        i += m
        if progress is not None:
            progress(i - a, b - a)


def _collect(eng, a: int, b: int, want):
    """(the records of frames [a, b), {i: the rows of extension block i for i in want})"""
    if b <= a:
        return np.zeros((0, N.RECORD_DOUBLES)), {i: np.zeros((0, N.EXT_BLOCKS[i][1])) for i in want}
    if want and hasattr(eng, "collect_blocks"):
        return eng.collect_blocks(a, b - a, want)
    if want:   # an engine_factory product from before collect_blocks: its collect_extN that reaches the last wanted block
        got = getattr(eng, f"collect_ext{want[-1] + 1 if want[-1] else ''}")(a, b - a)
        return got[0], {i: got[1 + i] for i in want}
    return eng.collect(a, b - a), {}


def _integrity_events(st: _Clips, make, ext5, n: int, n_planes: int, ig_opts) -> dict:
    # rank 0: the state machines run here on the gathered rows `ext5` of the whole clip (a freeze or a scene score that crosses a shard
    # boundary needs nothing else: every shard was armed with its frame a-1); freezedetect's anchored SADs, asked for
    # inside a still run only, come from the distorted file through a context of its own, made on first use
    from . import integrity as IG
    dis_rd, di = st.dis, st.di
    sad_eng, cache = [], {}

    def anchored_sad(anchor, i):
        if (anchor, i) not in cache:
            if not sad_eng:
                sad_eng.append(make(di.width, di.height, bit_depth=di.bit_depth, n_planes=n_planes,
                                    chroma_shift=(di.hshift, di.vshift), features=N.FEAT_INTEGRITY, device=st.device,
                                    max_batch=8, result_capacity=16))
            cache.clear()
            hi = min(n, i + 8)    # a still run asks for consecutive frames against one anchor: fetch a few at once
            got = sad_eng[0].frame_sad(dis_rd.frame(anchor)[:n_planes], [dis_rd.frame(j)[:n_planes] for j in range(i, hi)])
            for j in range(i, hi):
                cache[(anchor, j)] = got[j - i, :n_planes].astype(np.float64)
        return cache[(anchor, i)]
    try:
        return IG.analyze(ext5[:, N.EXT5_SAD_PREV:N.EXT5_SAD_PREV + n_planes], ext5[:, N.EXT5_BLACK_COUNT],
                          width=di.width, height=di.height, plane_sizes=_plane_sizes(di, n_planes), bit_depth=di.bit_depth,
                          fps_num=di.fps_num, fps_den=di.fps_den, opts=ig_opts, anchored_sad=anchored_sad)
    finally:
        for e in sad_eng:
            e.close()


def registration_crop(geometry: dict, width: int, height: int, hshift: int = 0, vshift: int = 0):
    """[left, top, right, bottom]: the margins outside the reference pixels whose source centre -- n/2 + s (x + 1/2 - n/2) + d
    - 1/2 in captured samples -- lies in 0 ... n - 1, each rounded up to the chroma step (exact, in Fractions)"""
    from fractions import Fraction
    from . import align as AL

    def axis(x0_q16, w_q16, n, step):
        d, s = AL.window_geometry(x0_q16, w_q16, n)
        half = Fraction(1, 2)
        lo = ((half - d - Fraction(n, 2)) / s + Fraction(n, 2) - half).__ceil__()        # the first x with a source centre >= 0
        hi = ((n - half - d - Fraction(n, 2)) / s + Fraction(n, 2) - half).__floor__()    # the last with one <= n - 1
        lo, hi = max(lo, 0), min(hi, n - 1)
        return -(-lo // step) * step, -(-(n - 1 - hi) // step) * step
    left, right = axis(geometry["x0_q16"], geometry["w_q16"], width, 1 << hshift)
    top, bottom = axis(geometry["y0_q16"], geometry["h_q16"], height, 1 << vshift)
    return [int(left), int(top), int(right), int(bottom)]


REGISTER_TILE = 32     # tile of the registration moments at full resolution (align.register halves it on small levels)


def _find_geometry(ref_rd, dis_rd, filter: str, n_frames: int, min_px: float, device, make) -> dict:
    """the `geometry` object of two opened, paired clips of one size: align.register on a few luma pairs, on a small context
    of its own"""
    from . import align as AL
    ri = ref_rd.info
    idx = _sample(ref_rd, dis_rd, n_frames, "no frames to align")
    with closing(_clip_context(make, device, ri)) as eng:
        geo = AL.register(eng.flow_moments, eng.resample, [ref_rd.frame(i)[0] for i in idx], [dis_rd.frame(i)[0] for i in idx],
                          filter=filter, tile=REGISTER_TILE, levels=None)
    geo["frames"] = len(idx)
    geo["filter"] = filter
    geo["applied"] = AL.geometry_applied(geo, min_px)
    hs, vs = (0, 0) if ri.mono else (ri.hshift, ri.vshift)
    geo["crop"] = registration_crop(geo, ri.width, ri.height, hs, vs) if geo["applied"] else [0, 0, 0, 0]
    return geo


def _find_levels(ref_rd, dis_rd, n_frames: int, apply: bool, device, make, curve: bool = False, full_range: bool = True):
    """(the `levels` object, [a correction table or None per plane], [a curve table or None per plane]) of two opened, paired
    clips: the per-level transfer table of a few pairs of every plane on a small context of its own.  curve: the monotone
    curve on top (align.best_curve), and under `apply` the check of its inverse on the sampled pairs"""
    from . import align as AL
    ri = ref_rd.info
    idx = _sample(ref_rd, dis_rd, n_frames, "no frames to align")
    n_planes = 1 if ri.mono else 3
    with closing(_clip_context(make, device, ri, n_planes)) as eng:
        refs, caps = [ref_rd.frame(i) for i in idx], [dis_rd.frame(i) for i in idx]
        tables = [eng.level_stats([f[p] for f in refs], [f[p] for f in caps], p) for p in range(n_planes)]
        checked = {}   # plane -> (its curve table, the squared error that is left on the sampled pairs)
        if curve:
            found = [AL.best_curve(T, ri.bit_depth, chroma=p > 0, full_range=full_range) for p, T in enumerate(tables)]
            for p, lv in enumerate(found):
                if apply and lv["kind"] == "curve" and lv["mismatch"]:
                    table = AL.curve_lut(tables[p], ri.bit_depth)
                    mapped = eng.table_apply([f[p] for f in caps], table, p)
                    checked[p] = table, AL.table_sse(eng.level_stats([f[p] for f in refs], mapped, p))
        else:
            found = [AL.best_levels(T, ri.bit_depth, chroma=p > 0) for p, T in enumerate(tables)]
    planes, luts, curves = {}, [], []
    for p, lv in enumerate(found):
        is_curve = lv["kind"] == "curve"
        if curve:
            n_pix = sum(int(x) for x in tables[p][:, :, 0].ravel())
            lv["mse_after"] = checked[p][1] / n_pix if p in checked else None   # int / int: correctly rounded
            lv["curve_applied"] = bool(p in checked and checked[p][1] < AL.table_sse(tables[p]))
        lv["applied"] = lv["curve_applied"] if is_curve else bool(apply and lv["mismatch"])
        luts.append(AL.correction_lut(lv, ri.bit_depth, chroma=p > 0) if lv["applied"] and not is_curve else None)
        curves.append(checked[p][0] if is_curve and lv["applied"] else None)
        planes["yuv"[p]] = lv
    return dict(planes["y"], planes=planes), luts, curves


OVERLAY_NODE = 8      # luma samples between the nodes of an overlay mask: 4:2:0 chroma takes the same grid at step 4


def _find_overlay(ref_rd, dis_rd, mode: str, boxes, n_frames: int, tile: int, grow: int, feather: int, share, device, make):
    """(the `overlay` object, the mask of distortion.overlay_mask or None) of two opened, paired clips of one size.  Without
    `boxes`: the luma tile moments of a few pairs on a small context of its own, the tiles hot in `share` of them, grown and
    feathered.  The neutral luma fill is the rounded mean of the sampled reference frames over the samples with alpha = 256:
    from the tiles' sums of r, which is exact, or under `boxes` from the frames themselves."""
    from . import distortion as D
    ri = ref_rd.info
    idx = _sample(ref_rd, dis_rd, n_frames, "no frames to analyse")
    shift = (0, 0) if ri.mono else (ri.hshift, ri.vshift)
    refs = [ref_rd.frame(i)[0] for i in idx]
    regions = []
    if boxes is not None:
        mask = D.overlay_mask_from_boxes(boxes, ri.width, ri.height, feather=feather, node=OVERLAY_NODE, chroma_shift=shift)
        full = D.mask_alpha(mask["nodes"], ri.width, ri.height, mask["step_log2"], mask["step_log2"]) == D.MASK_FULL
        total, count = sum(int(np.asarray(r)[full].sum(dtype=np.uint64)) for r in refs), int(full.sum()) * len(refs)
    else:
        # the one context made without chroma_shift, as it always was (a one-plane context reads no chroma)
        with closing(_side_context(make, device, ri.width, ri.height, ri.bit_depth, None)) as eng:
            Mo = eng.tile_moments(refs, [dis_rd.frame(i)[0] for i in idx], tile)
        S, counts = D.tile_sse(Mo), D.tile_counts(ri.width, ri.height, tile)
        hot = D.hot_tiles(S, counts, tile=tile, bit_depth=ri.bit_depth)
        regions = D.persistent_regions(hot, S, counts, share=share, tile=tile, bit_depth=ri.bit_depth, width=ri.width,
                                       height=ri.height)["regions"]
        tiles = D.persistent_tiles(hot, share)
        mask = D.overlay_mask(tiles, ri.width, ri.height, tile, grow=grow, feather=feather, node=OVERLAY_NODE, chroma_shift=shift)
        grown = D.grow_tiles(tiles, grow)
        total = sum(int(v) for v in Mo[..., D.SUM_R].sum(axis=0, dtype=np.uint64)[grown])      # a tile over the sample: below 2^30, exact
        count = int(counts[grown].sum()) * len(idx)
    luma = (2 * total + count) // (2 * count) if count else 1 << (ri.bit_depth - 1)
    fill = [int(luma)] + ([] if ri.mono else [1 << (ri.bit_depth - 1)] * 2)
    found = mask["bounds"] is not None
    overlay = {"mode": mode, "detected": boxes is None, "regions": regions, "boxes": mask["boxes"], "share": mask["share"],
               "fill": "reference" if mode == "reference" else fill, "tile": tile, "grow": grow, "feather": feather,
               "frames_sampled": len(idx), "applied": bool(found and mode != "report")}
    return overlay, (mask if found else None)


def _find_colour(ref_rd, dis_rd, n_frames: int, apply: bool, full_range: bool, device, make) -> dict:
    """the `colour` object of two opened, paired colour clips: the cross-plane moments of a few pairs on a small context of its
    own, reduced by align.best_colour"""
    from . import align as AL
    ri = ref_rd.info
    idx = _sample(ref_rd, dis_rd, n_frames, "no frames to align")
    with closing(_clip_context(make, device, ri, 3)) as eng:
        G = eng.colour_moments([ref_rd.frame(i)[:3] for i in idx], [dis_rd.frame(i)[:3] for i in idx])
    col = AL.best_colour(G, ri.bit_depth, ri.hshift, ri.vshift, full_range=full_range,
                         total_samples=len(idx) * ri.chroma_w * ri.chroma_h)
    col["full_range"] = bool(full_range)
    fix = AL.colour_correction(col, ri.bit_depth, full_range) if (col["mismatch"] and col["cross_plane"]) else None
    col["correction"] = None if fix is None else [int(v) for v in fix]
    col["applied"] = bool(apply and fix is not None)
    return col


def _find_active(ref_rd, dis_rd, n_frames: int, limit: int, skip: int, apply: bool, device, make) -> dict:
    """the `active_picture` object of two opened, paired clips of one size: the line profiles of a few luma planes of each on a
    small context of its own, reduced by align.active_picture and align.common_window"""
    from . import align as AL
    ri = ref_rd.info
    idx = _sample(ref_rd, dis_rd, n_frames, "no frames to align")
    with closing(_clip_context(make, device, ri)) as eng:
        found = []
        for rd in (ref_rd, dis_rd):
            lumas = [rd.frame(i)[0] for i in idx]
            rows, cols = eng.line_profiles(lumas)
            # the columns of the active rows only: a second pass over row-sliced views, made when there are bar rows
            found.append(AL.active_picture(rows, lambda t, b: cols if t == 0 and b == 0 else
                                           eng.line_profiles([y[t:ri.height - b] for y in lumas])[1],
                                           ri.bit_depth, limit=limit, skip=skip))
    hs, vs = (0, 0) if ri.mono else (ri.hshift, ri.vshift)
    out = AL.common_window(found[0], found[1], ri.width, ri.height, hs, vs)
    for key in ("scale", "offset"):
        out[key] = None if out[key] is None else [float(v) for v in out[key]]
    for key, ap in zip(("reference", "distorted"), found):
        out[key] = dict(ap, bar_noise=None if ap["bar_noise"] is None else float(ap["bar_noise"]))
    out["applied"] = bool(apply and out["reason"] is None)
    out["frames"] = len(idx)
    out["limit"] = limit
    return out


DISTORTION_PLANES = ("y", "cb", "cr")


def _plane_sizes(info, k: int):
    """[(width, height)] of the first k planes of a clip"""
    return [(info.width, info.height)] + [(info.chroma_w, info.chroma_h)] * (k - 1)


def _gather_u64(rows: np.ndarray, total: int, world_size: int, rank: int, gather_device) -> np.ndarray:
    """this rank's uint64 rows [m, ...] -> the uint64 rows [total, ...] of all ranks: they travel as the records do
    (shard.gather_records: the int64 transport carries the float64 view of a uint64 bit-exactly)"""
    cells = math.prod(rows.shape[1:])
    G = shard.gather_records(rows.reshape(rows.shape[0], cells).view(np.float64), total, world_size, rank, gather_device, width=cells)
    return np.ascontiguousarray(G).view(np.uint64).reshape((total,) + rows.shape[1:])


def _add_columns(res, columns: dict) -> None:
    """per-frame columns of every frame of the clip into res["metrics"], at the frames the result keeps"""
    keep = np.asarray(res["frame_indices"])
    for key, col in columns.items():
        res["metrics"][key] = col[keep]


def _sample(ref_rd, dis_rd, n_frames: int, error: str):
    """the frame numbers a sampled measurement reads (spatial_sample over the common range); none: ValueError(error)"""
    idx = spatial_sample(min(len(ref_rd), len(dis_rd)), n_frames)
    if not idx:
        raise ValueError(error)
    return idx


def _distortion_pass(ref_rd, dis_rd, a: int, b: int, n: int, tile: int, n_planes: int, device, make, world_size: int,
                     rank: int, gather_device, cancelled=None, levels: int = 0, band_planes: int = 1, temporal_tile: int = 0,
                     temporal_planes: int = 1, edge_planes: int = 0):
    """the measurement of score_files(distortion_map=), of score_files(spectrum=), of score_files(temporal=) and of
    score_files(coding_grid=), in one pass that reads every frame pair once, on every rank: (dmap, bands, temporal, edges).
    edges (edge_planes > 0, else None): per plane the edge profiles of every frame of the clip, uint64 (rows [n, H, 3],
    cols [n, W, 3]).  temporal (temporal_tile > 0, else None): per
    plane the temporal moments of every transition of the clip, uint64 [n - 1, ty, tx, 7]; a rank whose chunk starts at frame
    a > 0 also reads frame a - 1, so transition a is measured by the rank that owns frame a and the result does not depend
    on the number of ranks.  dmap (tile > 0, else None): per plane (tile SSE of every frame of the clip, uint64
    [n, ty, tx]; clip-summed moments, uint64 [ty, tx, 6]).  bands (levels > 0, else None): per plane the band moments of every
    frame of the clip, uint64 [n, L, 4, 3].  This rank measures its frames [a, b) in chunks of 8 pairs on a small context of
    its own; the ranks' rows travel as the records do (shard.gather_records: the int64 transport carries uint64 bit-exactly),
    their summed tile moments as one row a rank."""
    from . import distortion as DM
    ri = ref_rd.info
    if not tile:
        n_planes = 0
    if not levels:
        band_planes = 0
    if not temporal_tile:
        temporal_planes = 0
    sizes = _plane_sizes(ri, max(n_planes, band_planes, temporal_planes, edge_planes))
    edge_rows = [np.zeros((b - a, h + w, N.EDGE_SUMS), np.uint64) for w, h in sizes[:edge_planes]]   # a frame: H row lines, W column lines
    assert N.EDGE_CHUNK == N.TILE_CHUNK
    tgrids = [DM.tile_counts(w, h, temporal_tile).shape for w, h in sizes[:temporal_planes]]
    trows = [np.zeros((b - a,) + g + (N.TEMPORAL_SUMS,), np.uint64) for g in tgrids]   # row i - a: the transition INTO frame i
    assert N.TEMPORAL_CHUNK == N.TILE_CHUNK
    grids = [DM.tile_counts(w, h, tile).shape for w, h in sizes[:n_planes]]
    sse = [np.zeros((b - a,) + g, np.uint64) for g in grids]
    sums = [np.zeros(g + (N.TILE_SUMS,), np.uint64) for g in grids]
    band_rows = [np.zeros((b - a, levels, 4, N.BAND_SUMS), np.uint64) for _ in range(band_planes)]
    assert N.BAND_CHUNK == N.TILE_CHUNK
    if b > a:
        with closing(_clip_context(make, device, ri)) as eng:
            for i0 in range(a, b, N.TILE_CHUNK):
                if cancelled is not None and cancelled():
                    raise N.PqaCancelled(N.PQA_ECANCELLED, "cancelled")
                idx = range(i0, min(b, i0 + N.TILE_CHUNK))
                rf, df = [ref_rd.frame(i) for i in idx], [dis_rd.frame(i) for i in idx]
                if temporal_planes and i0 > 0:      # the predecessor of the chunk's first frame: one extra read a chunk
                    prf, pdf = [ref_rd.frame(i0 - 1)] + rf, [dis_rd.frame(i0 - 1)] + df
                    for p in range(temporal_planes):
                        trows[p][i0 - a:i0 - a + len(idx)] = eng.temporal_moments([f[p] for f in prf], [f[p] for f in pdf], temporal_tile)
                elif temporal_planes and len(idx) > 1:
                    for p in range(temporal_planes):
                        trows[p][1:len(idx)] = eng.temporal_moments([f[p] for f in rf], [f[p] for f in df], temporal_tile)
                for p in range(n_planes):
                    M = eng.tile_moments([f[p] for f in rf], [f[p] for f in df], tile)
                    sums[p] += M.sum(axis=0, dtype=np.uint64)
                    sse[p][i0 - a:i0 - a + len(idx)] = DM.tile_sse(M)
                for p in range(band_planes):
                    band_rows[p][i0 - a:i0 - a + len(idx)] = eng.band_moments([f[p] for f in rf], [f[p] for f in df], levels)
                for p in range(edge_planes):
                    er, ec = eng.edge_profiles([f[p] for f in rf], [f[p] for f in df])
                    edge_rows[p][i0 - a:i0 - a + len(idx)] = np.concatenate([er, ec], axis=1)
    to = (world_size, rank, gather_device)
    bands = [_gather_u64(rows, n, *to) for rows in band_rows]
    out = [(_gather_u64(S, n, *to), _gather_u64(T[None], world_size, *to).sum(axis=0, dtype=np.uint64)) for S, T in zip(sse, sums)]
    tmom = [_gather_u64(rows, n, *to)[1:] for rows in trows]   # frame 0 has no transition
    edges = []
    for rows, (w, h) in zip(edge_rows, sizes):
        E = _gather_u64(rows, n, *to)
        edges.append((E[:, :h], E[:, h:]))
    return (out if tile else None), (bands if levels else None), (tmom if temporal_tile else None), (edges if edge_planes else None)


def _itp_pass(ref_rd, dis_rd, a: int, b: int, n: int, spec: dict, device, make, world_size: int, rank: int, gather_device,
              cancelled=None) -> np.ndarray:
    """the measurement of score_files(delta_itp=): the rows [n, 8] of FeatureEngine.delta_itp for every frame pair of the clip,
    on every rank.  This rank measures its frames [a, b) in chunks of 8 pairs on a small three-plane context of its own; a
    frame's row depends on that frame pair alone, so the gathered rows (shard.gather_records) do not depend on the number of
    ranks."""
    from . import itp as ITP
    ri = ref_rd.info
    rows = np.zeros((b - a, N.ITP_SUMS), np.float64)
    if b > a:
        sp = ITP.native_spec(spec)
        with closing(_clip_context(make, device, ri, 3)) as eng:
            for i0 in range(a, b, N.ITP_CHUNK):
                if cancelled is not None and cancelled():
                    raise N.PqaCancelled(N.PQA_ECANCELLED, "cancelled")
                idx = range(i0, min(b, i0 + N.ITP_CHUNK))
                rows[i0 - a:i0 - a + len(idx)] = eng.delta_itp([ref_rd.frame(i)[:3] for i in idx], [dis_rd.frame(i)[:3] for i in idx], sp)
    return shard.gather_records(rows, n, world_size, rank, gather_device, width=N.ITP_SUMS)


def _itp_result(res, rows, spec: dict) -> None:
    """rank 0: adds res["delta_itp"] (the spec used, coefficients included, and itp.summary) and the three per-frame columns"""
    from . import itp as ITP
    _add_columns(res, ITP.frame_columns(rows))
    res["delta_itp"] = {"spec": dict(spec), "summary": ITP.summary(rows, spec["threshold"])}


def _grid_result(res, edges, info, periods, z2_min) -> None:
    """rank 0: the solver on the gathered edge profiles; adds res["coding_grid"] and the two luma columns"""
    from . import grid as GD
    planes = {}
    for name, (rows, cols), (w, h) in zip(DISTORTION_PLANES, edges, _plane_sizes(info, len(edges))):
        planes[name] = GD.analyse(rows, cols, w, h, info.bit_depth, periods=periods, z2_min=z2_min)
        if name == "y":
            _add_columns(res, GD.frame_columns(planes[name]["frames"]))
    res["coding_grid"] = {"planes": planes}


def _temporal_result(res, tmom, info, tile: int, min_mse, blend_min, still_mse, pop_factor) -> None:
    """rank 0: the solver on the gathered temporal moments; adds res["temporal"] and the three luma columns"""
    from . import temporal as TP
    planes = {}
    for name, M, (w, h) in zip(DISTORTION_PLANES, tmom, _plane_sizes(info, len(tmom))):
        planes[name] = TP.analyse(M, w, h, tile, info.bit_depth, min_mse=min_mse, blend_min=blend_min, still_mse=still_mse,
                                  pop_factor=pop_factor)
        if name == "y":
            _add_columns(res, TP.frame_columns(M, w, h, info.bit_depth))
    res["temporal"] = {"tile": tile, "planes": planes, "frames": int(tmom[0].shape[0]) + 1}


def _spectrum_result(res, bands, info, levels: int, min_mse, gain_floor) -> None:
    """rank 0: the solver on the gathered band moments; adds res["spectrum"] and the three luma columns"""
    from . import spectrum as SP
    planes = {}
    for name, M, (w, h) in zip(DISTORTION_PLANES, bands, _plane_sizes(info, len(bands))):
        planes[name] = SP.analyse(M, w, h, info.bit_depth, min_mse=min_mse, gain_floor=gain_floor)
        if name == "y":
            _add_columns(res, SP.frame_columns(M, w, h, info.bit_depth))
    res["spectrum"] = {"levels": levels, "planes": planes, "frames": int(bands[0].shape[0])}


def _distortion_result(res, dmap, info, tile: int, factor, min_mse, out_dir) -> None:
    """rank 0: the solver on the gathered measurement; adds res["distortion"], the two luma columns and the files"""
    from . import distortion as DM
    planes = {}
    for name, (S, M_sum), (w, h) in zip(DISTORTION_PLANES, dmap, _plane_sizes(info, len(dmap))):
        found = DM.analyse_plane(S, M_sum, w, h, tile, info.bit_depth, factor=factor, min_mse=min_mse)
        cols, mean_psnr = found.pop("columns"), found.pop("mean_psnr")
        planes[name] = found
        if name == "y":
            _add_columns(res, {"tile_psnr_min": cols["tile_psnr_min"], "distortion_concentration": cols["concentration"]})
        if out_dir is not None:
            os.makedirs(out_dir, exist_ok=True)
            with open(os.path.join(out_dir, f"distortion_{name}.pgm"), "wb") as f:
                f.write(DM.heatmap_pgm(mean_psnr))
            np.save(os.path.join(out_dir, f"distortion_{name}.npy"), M_sum)
    res["distortion"] = {"tile": tile, "grid": planes["y"]["grid"], "planes": planes, "frames": int(dmap[0][0].shape[0])}


def spatial_sample(n: int, count: int):
    """`count` frame numbers spread evenly over 0 ... n - 1 (the middles of `count` equal parts; fewer when n < count)"""
    return sorted({(2 * t + 1) * n // (2 * count) for t in range(count)}) if n > 0 else []


def _find_shift(ref_rd, dis_rd, R: int, n_frames: int, device, make) -> dict:
    """the `spatial` object of two opened (and temporally paired) clips: shifted-window SSE of a few luma pairs over
    -R ... R in both directions on a small context of its own"""
    from . import align as AL
    ri = ref_rd.info
    idx = _sample(ref_rd, dis_rd, n_frames, "no frames to align")
    with closing(_clip_context(make, device, ri)) as eng:
        S = eng.shift_sse([ref_rd.frame(i)[0] for i in idx], [dis_rd.frame(i)[0] for i in idx], R)
    sp = AL.best_shift(S, R, (ri.width - 2 * R) * (ri.height - 2 * R))
    sp["frames"] = len(idx)
    sp["applied"] = bool(not sp["at_edge"] and (sp["dx"], sp["dy"]) != (0, 0))
    sp["chroma_exact"] = bool(ri.mono or (sp["dx"] % (1 << ri.hshift) == 0 and sp["dy"] % (1 << ri.vshift) == 0))
    return sp


FIELD_CALL = 65   # frames a call of the field measurement: 64 transitions; consecutive calls share a frame


def _find_fields(ref_rd, dis_rd, n_frames, penalty_mse, apply: bool, device, make):
    """(the `fields` object, the weave plan or None) of two opened, paired clips: the field moments of the luma of the first
    n_frames frames of the common range (None: all) on a small context of its own, reduced by fields.summary"""
    from . import fields as FL
    ri = ref_rd.info
    n_all = min(len(ref_rd), len(dis_rd))
    n = n_all if n_frames is None else min(n_all, int(n_frames))
    parts = []
    with closing(_clip_context(make, device, ri)) as eng:
        for a in range(0, max(n - 1, 0), FIELD_CALL - 1):
            span = range(a, min(a + FIELD_CALL, n))
            parts.append(eng.field_moments([ref_rd.frame(i)[0] for i in span], [dis_rd.frame(i)[0] for i in span]))
    X = np.concatenate(parts) if parts else np.zeros((0, N.FIELD_SUMS), np.uint64)
    out = FL.summary(X, ri.width, ri.height, ri.bit_depth, penalty_mse)
    moved = any(g["kind"] != "progressive" for g in out["segments"])
    reason = ("too few frames" if n < 3 else "report" if not apply else "progressive" if not moved else
              None if out["weavable"] else "not weavable")
    plan = FL.weave_plan([(g["first"], g["last"], g["state"]) for g in out["segments"]], n_all) if reason is None else None
    out.update(frames=n, transitions=int(X.shape[0]), declared={"reference": ri.interlace, "distorted": dis_rd.info.interlace},
               applied=reason is None, reason=reason)
    if plan is not None:   # what the weave does: the output frames [u_lo, u_hi) and the fields left as captured
        out.update(u_lo=plan["u_lo"], u_hi=plan["u_hi"], unfilled=[list(v) for v in plan["unfilled"]])
    return out, plan


def _find_alignment(ref_rd, dis_rd, K: int, align_frames, penalty_mse, device, make) -> dict:
    """the `alignment` object of two opened clips: cross-SSE of their lumas over -K ... K on a small context of its own"""
    from . import align as AL
    ri = ref_rd.info
    n_ref, n_dis = len(ref_rd), len(dis_rd)
    if align_frames is not None:
        if align_frames < 1:
            raise ValueError("align_frames must be positive")
        n_ref, n_dis = min(n_ref, int(align_frames)), min(n_dis, int(align_frames) + K)
    if n_ref <= 0 or n_dis <= 0:
        raise ValueError("no frames to align")
    with closing(_clip_context(make, device, ri)) as eng:
        D = eng.cross_sse([ref_rd.frame(i)[0] for i in range(n_ref)], [dis_rd.frame(j)[0] for j in range(n_dis)], -K, K)
    return AL.align(D, n_ref, n_dis, ri.width * ri.height, k_lo=-K, fps=ri.fps, bit_depth=ri.bit_depth,
                    penalty_mse=penalty_mse)


def finish_records(rec: np.ndarray, mdl: M.VmafModel, info, *, psnr: bool, ssim: bool, n_subsample: int = 1,
                   n_planes: int = 1, fps: float = 0.0, ext: np.ndarray | None = None, float_ssim: bool = False,
                   ms_ssim: bool = False, ciede: bool = False, cambi: bool = False,
                   cambi_full_ref: bool = False, ext2: np.ndarray | None = None, psnr_hvs: bool = False,
                   ext3: np.ndarray | None = None, xpsnr: bool = False, ext4: np.ndarray | None = None,
                   siti: bool = False, integrity: dict | None = None) -> ScoreResult:
    """Host epilogue: records -> libvmaf-named metric columns (+ vmaf), stats-file lines.  With `float_ssim` / `ms_ssim`
    / `ciede` the extension records `ext` ([n, EXT_DOUBLES], pqa_collect_ext) add libvmaf's float_ssim / float_ms_ssim /
    ciede2000 columns, with `cambi` / `cambi_full_ref` libvmaf's cambi, cambi_source and cambi_full_reference.  With
    `psnr_hvs` the second extension records `ext2` ([n, EXT2_DOUBLES], pqa_collect_ext2) add psnr_hvs_y / _cb / _cr and
    psnr_hvs.  With `xpsnr` the third extension records `ext3` ([n, EXT3_DOUBLES], pqa_collect_ext3) add xpsnr_y / _u /
    _v, FFmpeg's stats-file lines (xpsnr_lines) and its summary (xpsnr_summary, report.xpsnr_summary) of every frame.
    With `siti` the fourth extension records `ext4` ([n, EXT4_DOUBLES], pqa_collect_ext4) add siti_si / siti_ti of the
    distorted and siti_si_source / siti_ti_source of the reference luma.  With `integrity` (the dict integrity.analyze
    returns for the clip) its four columns are added and the event lists, the anchors and FFmpeg's log lines go into the
    result (keys integrity, freeze_anchor, integrity_lines)."""
    n = rec.shape[0]
    prefix = "integer_" if mdl.is_integer else ""
    metrics = M.metrics_from_records(rec, info.width, info.height, prefix)
    plane_sizes = [(info.width, info.height)] + ([(info.chroma_w, info.chroma_h)] * 2 if n_planes == 3 else [])
    psnr_lines = ssim_lines = None
    if psnr:
        from .engine import sse_from_records
        sse = sse_from_records(rec)[:, :n_planes]
        psnr_lines = report.psnr_stats_lines(sse, plane_sizes, info.bit_depth)
        pp, _ = report.psnr_values(sse, plane_sizes, info.bit_depth)
        cap = 6.0 * info.bit_depth + 12.0          # libvmaf's psnr feature caps at 60 dB (8-bit) / 72 dB (10-bit)
        for p, name in enumerate(("psnr_y", "psnr_cb", "psnr_cr")[:n_planes]):
            metrics[name] = _cap(pp[:, p], cap)
    if ssim:
        sv = rec[:, N.REC_SSIM:N.REC_SSIM + n_planes]
        ssim_lines = report.ssim_stats_lines(sv, plane_sizes)
        metrics["ssim"] = report.ssim_all(sv, plane_sizes)

    def need(block, i, what):   # block i of N.EXT_BLOCKS, a row for every frame
        if block is None or block.shape != (n, N.EXT_BLOCKS[i][1]):
            raise ValueError(f"{what} extension records of every frame")

    if float_ssim or ms_ssim or ciede or cambi:
        need(ext, 0, "float_ssim / ms_ssim / ciede2000 / cambi need the")
        if float_ssim:
            metrics["float_ssim"] = ext[:, N.EXT_FLOAT_SSIM].copy()
        if ms_ssim:
            metrics["float_ms_ssim"] = ext[:, N.EXT_MS_SSIM].copy()
        if ciede:
            metrics["ciede2000"] = ext[:, N.EXT_CIEDE2000].copy()
        if cambi:
            metrics["cambi"] = ext[:, N.EXT_CAMBI].copy()
            if cambi_full_ref:
                src = ext[:, N.EXT_CAMBI_SOURCE].copy()
                metrics["cambi_source"] = src
                with np.errstate(invalid="ignore"):
                    metrics["cambi_full_reference"] = np.where(np.isnan(metrics["cambi"]) | np.isnan(src), np.nan,
                                                               np.maximum(metrics["cambi"] - src, 0.0))
    if psnr_hvs:
        need(ext2, 1, "psnr_hvs needs the second")
        for key, slot in (("psnr_hvs_y", N.EXT2_PSNR_HVS_Y), ("psnr_hvs_cb", N.EXT2_PSNR_HVS_CB),
                          ("psnr_hvs_cr", N.EXT2_PSNR_HVS_CR), ("psnr_hvs", N.EXT2_PSNR_HVS)):
            metrics[key] = ext2[:, slot].copy()
    xpsnr_lines = xpsnr_summary = None
    if xpsnr:
        need(ext3, 2, "xpsnr needs the third")
        for p, key in enumerate(("xpsnr_y", "xpsnr_u", "xpsnr_v")[:n_planes]):
            metrics[key] = ext3[:, N.EXT3_XPSNR_Y + p].copy()
        db = ext3[:, N.EXT3_XPSNR_Y:N.EXT3_XPSNR_Y + n_planes]
        wsse = ext3[:, N.EXT3_WSSE:N.EXT3_WSSE + n_planes]
        xpsnr_lines = report.xpsnr_stats_lines(db)
        xpsnr_summary = report.xpsnr_summary(wsse, db, plane_sizes, info.bit_depth)
    if siti:
        need(ext4, 3, "siti needs the fourth")
        for key, slot in SITI_KEYS:
            metrics[key] = ext4[:, slot].copy()
    if integrity is not None:
        from . import integrity as IG
        for key, col in integrity["columns"].items():
            if np.shape(col) != (n,):
                raise ValueError("integrity needs the columns of every frame")
            metrics[key] = np.asarray(col, np.float64).copy()
    scored = M.score_frames(mdl, metrics)
    idx = np.arange(n)
    if n_subsample > 1:
        keep = idx % n_subsample == 0
        scored = {k: np.asarray(v)[keep] for k, v in scored.items()}
        idx = idx[keep]
    return ScoreResult(metrics=scored, frame_indices=idx, records=rec, info=info, fps=fps,
                       psnr_lines=psnr_lines, ssim_lines=ssim_lines, model_name=mdl.name,
                       **({"xpsnr_lines": xpsnr_lines, "xpsnr_summary": xpsnr_summary} if xpsnr else {}),
                       **({"integrity": IG.events_json(integrity), "freeze_anchor": np.asarray(integrity["freeze_anchor"]),
                           "integrity_lines": IG.log_lines(integrity)} if integrity is not None else {}))


SITI_KEYS = (("siti_si", N.EXT4_SI), ("siti_ti", N.EXT4_TI), ("siti_si_source", N.EXT4_SI_SOURCE),
             ("siti_ti_source", N.EXT4_TI_SOURCE))


def xpsnr_hfr(info) -> bool:
    """FFmpeg's xpsnr switches to its second-order temporal term at an integer frame rate (num / den truncated) >= 32."""
    return bool(info.fps_den) and info.fps_num // info.fps_den >= 32
