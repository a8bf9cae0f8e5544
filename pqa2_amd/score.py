"""Command-line / torchrun entry of the scoring path:

    python -m pqa2_amd.score REF DIS --model vmaf_v0.6.1 --json out.json [--psnr-log p.txt --ssim-log s.txt]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 \
           -m pqa2_amd.score REF DIS --json out.json          # frame-sharded, one process per GPU

Progress goes to stderr as `frame= N` lines -- the same shape the reference parses from its ffmpeg
child (app/vmaf_analyzer.py:475-492), so VMAFAnalyzer drives a multi-GPU job exactly the way the
reference drives ffmpeg."""
from __future__ import annotations

import argparse
import os
import sys
import time


def _expected_parent() -> int:
    """The process a worker must not outlive: PQA_PARENT_PID when the launcher exported it (a launcher that starts this
    module DIRECTLY may do so to close the window between fork and this line; never set it under torchrun, whose agent --
    not the analyzer -- is the workers' parent), else the parent as it is now.  Read at the very top of main()."""
    try:
        return int(os.environ.get("PQA_PARENT_PID", "")) or os.getppid()
    except ValueError:
        return os.getppid()


def _die_with_parent(expected: int, getppid=os.getppid, kill=os.kill) -> None:
    """A worker must not outlive the job that started it (a rank blocked in the record gather holds its GPU context for
    ever): ask the kernel for SIGTERM when the parent -- torchrun's agent, or whoever started a one-rank job -- goes away.
    Linux only (prctl PR_SET_PDEATHSIG); elsewhere a no-op.

    The parent may have died BEFORE the request took effect; then this process has already been re-parented and no signal
    will ever come.  That case is recognised by comparing the parent now with `expected` (the parent at start-up) -- not by
    `getppid() == 1`: a container's entrypoint or an init-less shell IS pid 1 and perfectly alive, and under a sub-reaper
    (systemd --user, `docker run --init`, a test harness) an orphan's parent is the reaper, not 1.

    Caveat of PR_SET_PDEATHSIG: it fires when the THREAD that forked this process exits, not the parent process.  A
    launcher that spawns this module from a short-lived thread (a QThread that returns while the job runs) would end the
    job early; spawn from a thread that outlives the child.  Under torchrun the workers' parent is the agent's main thread."""
    try:
        import ctypes
        import signal
        libc = ctypes.CDLL(None, use_errno=True)
        libc.prctl(1, int(signal.SIGTERM), 0, 0, 0)   # PR_SET_PDEATHSIG = 1
        if getppid() != expected:                      # re-parented already: the parent went away before we asked
            kill(os.getpid(), signal.SIGTERM)
    except Exception:
        pass


def main(argv=None) -> int:
    parent = _expected_parent()    # before anything slow: imports, argument parsing
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC only on this pool's driver: RCCL needs it (before torch loads)
    from .integrity import DEFAULTS as IG_OPTIONS
    ap = argparse.ArgumentParser(prog="pqa2_amd.score")
    ap.add_argument("reference")
    ap.add_argument("distorted")
    ap.add_argument("--model", default="vmaf_v0.6.1")
    ap.add_argument("--json", required=True)
    ap.add_argument("--psnr-log")
    ap.add_argument("--ssim-log")
    ap.add_argument("--n-subsample", type=int, default=1)
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--fixed-point", type=int, default=0,
                    help="PQA_FIXED_* mask (1 VIF, 2 motion): extractors run in libvmaf's fixed-point arithmetic")
    ap.add_argument("--float-ssim", action="store_true", help="add libvmaf's float_ssim feature (per frame and pooled)")
    ap.add_argument("--ms-ssim", action="store_true", help="add libvmaf's float_ms_ssim feature (per frame and pooled)")
    ap.add_argument("--ciede", action="store_true", help="add libvmaf's ciede feature, key ciede2000 (per frame and pooled)")
    ap.add_argument("--cambi", action="store_true", help="add libvmaf's cambi banding index of the distorted luma")
    ap.add_argument("--cambi-full-ref", action="store_true",
                    help="with --cambi: also cambi_source and cambi_full_reference (per frame and pooled)")
    ap.add_argument("--psnr-hvs", action="store_true",
                    help="add libvmaf's psnr_hvs feature: psnr_hvs_y / _cb / _cr and psnr_hvs (per frame and pooled)")
    ap.add_argument("--xpsnr", action="store_true",
                    help="add FFmpeg's xpsnr: xpsnr_y / _u / _v per frame and FFmpeg's summary in the JSON's top level")
    ap.add_argument("--xpsnr-log", default=None, help="FFmpeg xpsnr stats_file output path (implies --xpsnr)")
    ap.add_argument("--siti", action="store_true",
                    help="add FFmpeg's siti (ITU-T P.910 SI / TI) of both clips: siti_si / _ti (distorted) and "
                         "siti_si_source / _ti_source (reference), per frame and pooled")
    ap.add_argument("--integrity", action="store_true",
                    help="add FFmpeg's freezedetect / blackdetect / scdet on the distorted clip: scd_mafd, scd_score, "
                         "black_ratio, freeze_mafd per frame and the event lists under the JSON's top-level integrity key")
    ap.add_argument("--integrity-log", default=None, help="event log in FFmpeg's wording, one line per event (implies --integrity)")
    for name in IG_OPTIONS:   # FFmpeg's option names and defaults (integrity.DEFAULTS); each implies --integrity
        ap.add_argument("--" + name.replace("_", "-"), type=float, default=None, help=f"integrity option {name}")
    ap.add_argument("--align", type=int, default=0, metavar="K",
                    help="search the frame offset that pairs the clips over -K ... K (banded cross-frame SSE) and score "
                         "the aligned range; the JSON gets a top-level alignment object")
    ap.add_argument("--align-frames", type=int, default=None, metavar="N",
                    help="with --align: search the first N reference frames only (default: the whole clips)")
    ap.add_argument("--spatial-align", type=int, default=0, metavar="R",
                    help="search the whole-pixel displacement of the captured picture over -R ... R in x and y (R <= 16, "
                         "shifted-window luma SSE) and score both clips cropped to the common window; the JSON's "
                         "alignment object gets a spatial entry")
    ap.add_argument("--spatial-frames", type=int, default=8, metavar="N",
                    help="with --spatial-align: search N frame pairs spread evenly over the clips (default 8)")
    ap.add_argument("--level-align", action="store_true",
                    help="measure the level mapping of the capture (gain, offset, limited / full range conversion) from the "
                         "per-level transfer table of a few frame pairs; the JSON's alignment object gets a levels entry")
    ap.add_argument("--level-correct", action="store_true",
                    help="--level-align, and undo a mapping found on every plane that has one before scoring")
    ap.add_argument("--level-curve", action="store_true",
                    help="--level-align, and fit a monotone transfer curve on top (a gamma mismatch, a contrast enhancer, a black "
                         "stretch); with --level-correct a plane whose curve lowers the error goes through its inverse table on the "
                         "GPU before scoring")
    ap.add_argument("--level-frames", type=int, default=8, metavar="N",
                    help="with --level-align / --level-correct: measure N frame pairs spread evenly over the clips (default 8)")
    ap.add_argument("--colour-align", action="store_true",
                    help="measure the colour matrix of the capture (bt601 / bt709 / bt2020 material decoded with one matrix and "
                         "encoded with another) from the cross-plane moments of a few frame pairs; the JSON's alignment object "
                         "gets a colour entry")
    ap.add_argument("--colour-correct", action="store_true",
                    help="--colour-align, and undo a matrix found on the GPU before scoring")
    ap.add_argument("--colour-frames", type=int, default=8, metavar="N",
                    help="with --colour-align / --colour-correct: measure N frame pairs spread evenly over the clips (default 8)")
    ap.add_argument("--active-picture", action="store_true",
                    help="measure the black bars (letterbox, pillarbox) of both clips from the row and column sums of a few "
                         "luma planes; the JSON's alignment object gets an active_picture entry")
    ap.add_argument("--active-crop", action="store_true",
                    help="--active-picture, and score both clips cropped to the common active rectangle when their bars agree")
    ap.add_argument("--active-frames", type=int, default=8, metavar="N",
                    help="with --active-picture / --active-crop: measure N frames of each clip spread evenly over it (default 8)")
    ap.add_argument("--active-limit", type=int, default=24, metavar="V",
                    help="with --active-picture / --active-crop: a line is dark when its mean does not exceed V in 8-bit code "
                         "values (default 24)")
    ap.add_argument("--active-skip", type=int, default=0, metavar="N",
                    help="with --active-picture / --active-crop: the outermost N lines of every edge count as dark whatever "
                         "they hold (a caption or timecode line; default 0)")
    ap.add_argument("--field-align", action="store_true",
                    help="measure the field structure of the capture (a field from the neighbouring frame, swapped fields, a "
                         "line-doubled field) from the exact field-against-field errors of the luma; the JSON's alignment "
                         "object gets a fields entry")
    ap.add_argument("--field-correct", action="store_true",
                    help="--field-align, and re-weave the captured clip from its own fields before scoring when the fault is "
                         "reversible (field shift, field swap)")
    ap.add_argument("--field-frames", type=int, default=None, metavar="N",
                    help="with --field-align / --field-correct: measure the first N frames of the common range (default: all)")
    ap.add_argument("--field-penalty-mse", type=float, default=None, metavar="X",
                    help="with --field-align / --field-correct: what a change of field structure costs, as an MSE of one frame "
                         "(default: that of the temporal alignment)")
    ap.add_argument("--field-repair", action="store_true",
                    help="with --field-correct: when one field of the capture was dropped and the other line-doubled (single_field "
                         "for the whole clip), interpolate the lost field from the kept one on the GPU before scoring")
    ap.add_argument("--deinterlace", default=None, metavar="MODE", choices=["adaptive", "intra"],
                    help="deinterlace the captured clip on the GPU before scoring, in exact integers: adaptive (the lost field from "
                         "the fields before and after it where the picture is still) or intra (from the kept field alone); the "
                         "JSON's input object gets a deinterlace entry")
    ap.add_argument("--deinterlace-rate", default="frame", choices=["frame", "field"],
                    help="with --deinterlace: a frame per frame, or a frame per field (twice the frames at twice the rate: a 50p "
                         "master against a 25i capture; default frame)")
    ap.add_argument("--field-order", default=None, choices=["tff", "bff"],
                    help="with --deinterlace: the field that comes first in time (default: the Y4M header's I tag)")
    ap.add_argument("--deinterlace-side", default="distorted", choices=["distorted", "both"],
                    help="with --deinterlace: the captured clip only, or both clips (default distorted)")
    ap.add_argument("--distortion-map", type=int, default=0, metavar="T", choices=[0, 8, 16, 32, 64],
                    help="measure WHERE the clips differ: the second-order sums of every T x T tile (8, 16, 32 or 64) of every "
                         "scored frame pair, in a second pass over both clips; the JSON gets a top-level distortion object "
                         "(localised defects, persistent regions such as a burnt-in logo) and two per-frame metrics")
    ap.add_argument("--distortion-planes", default="y", choices=["y", "all"],
                    help="with --distortion-map: the luma only (default) or all three planes")
    ap.add_argument("--distortion-dir", default=None, metavar="DIR",
                    help="with --distortion-map: write distortion_<plane>.pgm (the clip-mean map, one pixel a tile) and "
                         "distortion_<plane>.npy (the clip-summed tile moments) into DIR")
    ap.add_argument("--distortion-factor", type=float, default=16, metavar="F",
                    help="with --distortion-map: a tile is hot when its MSE exceeds F times the frame's median tile MSE (default 16)")
    ap.add_argument("--distortion-min-mse", type=float, default=4.0, metavar="V",
                    help="with --distortion-map: ... and V in 8-bit code values squared (default 4)")
    ap.add_argument("--spectrum", type=int, default=0, metavar="L", choices=[0, 1, 2, 3, 4, 5, 6],
                    help="measure WHAT KIND of difference the clips have: the second moments of L Haar octaves (1 ... 6) in three "
                         "orientations of every scored frame pair, in a second pass over both clips (shared with "
                         "--distortion-map); the JSON gets a top-level spectrum object (gain, detail loss and added noise per "
                         "band, the bandwidth each way, loss / noise) and three per-frame metrics")
    ap.add_argument("--spectrum-planes", default="y", choices=["y", "all"],
                    help="with --spectrum: the luma only (default) or all three planes")
    ap.add_argument("--spectrum-min-mse", type=float, default=1.0, metavar="V",
                    help="with --spectrum: below a total MSE of V in 8-bit code values squared the clips count as clean (default 1)")
    ap.add_argument("--spectrum-gain-floor", type=float, default=0.5, metavar="G",
                    help="with --spectrum: a band whose gain is at least G counts as passed by the chain (default 0.5)")
    ap.add_argument("--temporal", type=int, default=0, metavar="T", choices=[0, 8, 16, 32, 64],
                    help="measure whether the MOTION of the capture is wrong: the second-order sums of the frame differences of "
                         "both clips per T x T tile (8, 16, 32 or 64) of every transition, in a second pass over both clips "
                         "(shared with --distortion-map and --spectrum); the JSON gets a top-level temporal object (temporal "
                         "gain, loss and noise, blend weight, pops, blend / loss / noise) and three per-frame metrics")
    ap.add_argument("--temporal-planes", default="y", choices=["y", "all"],
                    help="with --temporal: the luma only (default) or all three planes")
    ap.add_argument("--temporal-min-mse", type=float, default=1.0, metavar="V",
                    help="with --temporal: below a temporal MSE of V in 8-bit code values squared the clips count as clean, and no "
                         "transition below it is a pop (default 1)")
    ap.add_argument("--temporal-blend-min", type=float, default=1 / 16, metavar="B",
                    help="with --temporal: a weight of the previous frame of at least B counts as a blend (default 1/16)")
    ap.add_argument("--temporal-still-mse", type=float, default=0.25, metavar="V",
                    help="with --temporal: a tile stands still in a transition when its reference moves by at most V in 8-bit code "
                         "values squared (default 1/4)")
    ap.add_argument("--temporal-pop-factor", type=float, default=4, metavar="F",
                    help="with --temporal: a transition pops when its noise exceeds F times the clip's median (default 4)")
    ap.add_argument("--coding-grid", action="store_true",
                    help="detect a block grid in the difference between the clips, the artefact of an encoder leg: the gradient "
                         "energy of both clips per row and column line, in a second pass over both clips (shared with "
                         "--distortion-map, --spectrum and --temporal); the JSON gets a top-level coding_grid object (period and "
                         "phase each way, in the coordinates of the scored window) and two per-frame metrics")
    ap.add_argument("--grid-planes", default="y", choices=["y", "all"],
                    help="with --coding-grid: the luma only (default) or all three planes")
    ap.add_argument("--grid-min-period", type=int, default=4, metavar="P",
                    help="with --coding-grid: the smallest block size searched, at least 4 (default 4)")
    ap.add_argument("--grid-max-period", type=int, default=64, metavar="P",
                    help="with --coding-grid: the largest block size searched, at most 64 (default 64)")
    ap.add_argument("--grid-z2", type=float, default=25.0, metavar="Z",
                    help="with --coding-grid: a period is accepted when the squared z score of its votes is at least Z (default 25)")
    ap.add_argument("--resize", default=None, metavar="FILTER", choices=["bilinear", "bicubic", "lanczos"],
                    help="resample a distorted clip whose frame size differs from the reference's to it before scoring "
                         "(exact-integer polyphase filter: bilinear, bicubic or lanczos); the JSON gets a top-level resize object")
    ap.add_argument("--register", default=None, metavar="FILTER", choices=["bilinear", "bicubic", "lanczos"],
                    help="measure the sub-pixel displacement and the scale factor of the captured picture (tile-wise gradient "
                         "moments, coarse to fine) and, where it matters, resample the capture onto the reference grid with "
                         "this filter and crop both clips; the JSON's alignment object gets a geometry entry")
    ap.add_argument("--register-frames", type=int, default=8, metavar="N",
                    help="with --register: measure N frame pairs spread evenly over the clips (default 8)")
    ap.add_argument("--chroma-siting", default=None, choices=["left", "center", "topleft"],
                    help="with --chroma-mismatch convert: where both clips' subsampled chroma sits (left: co-sited horizontally, "
                         "centred vertically, MPEG-2; center: centred both ways, JPEG; topleft: co-sited both ways) instead of "
                         "what each file's header implies")
    ap.add_argument("--rgb-matrix", default=None, choices=["bt601", "bt709", "bt2020"],
                    help="a packed RGB capture (.bgra, .argb, .rgba, .abgr, .r210) is converted on the GPU to the other clip's "
                         "Y'CbCr layout, siting, depth and range with this matrix (default: bt601 up to 576 lines, else bt709); "
                         "the JSON's input object gets a conversion entry")
    ap.add_argument("--rgb-range", default=None, choices=["full", "limited"],
                    help="the range of the R'G'B' code values of a packed RGB capture (default: full for the 8-bit formats, "
                         "limited for r210)")
    ap.add_argument("--delta-itp", default=None, metavar="TRANSFER", choices=["pq", "hlg", "bt1886"],
                    help="the ITU-R BT.2124 colour difference Delta E ITP of every pixel in ICtCp, for clips with this transfer "
                         "(pq: ST 2084; hlg: through the 1000 cd/m2 reference display; bt1886: SDR at 100 cd/m2), in a pass of its "
                         "own over both clips as scored; three per-frame metrics (delta_e_itp, delta_e_itp_max, itp_above_jnd) "
                         "and a top-level delta_itp object.  1 is about one just-noticeable difference")
    ap.add_argument("--itp-matrix", default=None, choices=["bt601", "bt709", "bt2020"],
                    help="with --delta-itp: the Y'CbCr matrix (and primaries) of the clips (default: bt2020 for pq and hlg; "
                         "bt601 up to 576 lines, else bt709 for bt1886)")
    ap.add_argument("--itp-range", default=None, choices=["full", "limited"],
                    help="with --delta-itp: the range of the code values (default: what the reference's header says, else limited)")
    ap.add_argument("--itp-peak", type=float, default=None, metavar="CD_M2",
                    help="with --delta-itp: the display's peak luminance Lw for hlg (default 1000) and bt1886 (default 100)")
    ap.add_argument("--itp-threshold", type=float, default=1.0, metavar="DE",
                    help="with --delta-itp: a pixel is counted as visibly different above this Delta E ITP (default 1)")
    ap.add_argument("--overlay-mask", default=None, metavar="MODE", choices=["report", "neutral", "reference"],
                    help="take a burnt-in overlay (a channel logo, a clock, a timecode) out of the scores: find the tiles that "
                         "differ in nearly every sampled frame and report them (report), blend both clips towards one flat value "
                         "there (neutral: reads slightly low, the region loses its motion) or blend the distorted clip towards "
                         "the reference there (reference: reads high, the region counts as perfect); the JSON gets a top-level "
                         "overlay object")
    ap.add_argument("--overlay-box", action="append", default=None, metavar="X0,Y0,X1,Y1",
                    help="with --overlay-mask: mask this box of luma pixels (X1, Y1 exclusive; repeatable) instead of detecting")
    ap.add_argument("--overlay-frames", type=int, default=32, metavar="N", help="with --overlay-mask: frame pairs sampled (default 32)")
    ap.add_argument("--overlay-tile", type=int, default=16, choices=[8, 16, 32, 64], help="with --overlay-mask: tile size (default 16)")
    ap.add_argument("--overlay-grow", type=int, default=1, metavar="TILES",
                    help="with --overlay-mask: tiles added around the detected ones (default 1)")
    ap.add_argument("--overlay-feather", type=int, default=16, metavar="PX",
                    help="with --overlay-mask: width of the mask's soft edge in luma pixels, a multiple of 8 (default 16; 0: hard)")
    ap.add_argument("--chroma-mismatch", default="error", choices=["error", "luma", "convert"],
                    help="clips that differ in chroma subsampling (a 4:2:2 capture such as .uyvy / .v210 against a 4:2:0 "
                         "master): refuse them (default), score their luma only -- VMAF and luma PSNR / SSIM --, or convert the "
                         "distorted clip on the GPU to the reference's chroma layout, siting and bit depth (8 / 10 / 12) and score "
                         "all three planes; the JSON gets a "
                         "top-level input object.  Headerless packed files (.uyvy, .yuyv, .yuy2, .v210) take their frame size "
                         "from a _WxH name hint, as raw .yuv does")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"],
                    help="collective backend of the record gather; gloo + --share-device rehearses N ranks on one GPU")
    ap.add_argument("--share-device", action="store_true", help="every rank uses device 0 (rehearsal on a one-GPU box)")
    a = ap.parse_args(argv)

    from . import report
    from .pipeline import score_files
    _die_with_parent(parent)
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    gather_device = None
    if a.share_device:
        local_rank = 0
    if world > 1:
        import torch
        import torch.distributed as dist
        torch.cuda.set_device(local_rank)
        if a.backend == "nccl":      # RCCL: the records travel GPU to GPU over xGMI
            gather_device = torch.device("cuda", local_rank)
            dist.init_process_group("nccl", device_id=gather_device)
        else:                        # gloo: host tensors (several ranks may then share one GPU)
            dist.init_process_group("gloo")
    last = [0.0]

    def progress(done, total):
        now = time.time()
        if rank == 0 and (now - last[0] > 0.25 or done == total):
            last[0] = now
            print(f"frame= {done * world} fps=0 q=0.0 size=N/A", file=sys.stderr, flush=True)

    overlay_boxes = None
    if a.overlay_box:
        try:
            overlay_boxes = [[int(v) for v in b.split(",")] for b in a.overlay_box]
        except ValueError:
            ap.error("--overlay-box takes four integers X0,Y0,X1,Y1")
        if not a.overlay_mask:
            ap.error("--overlay-box needs --overlay-mask")
    ig_opts = {k: getattr(a, k) for k in IG_OPTIONS if getattr(a, k) is not None}
    want_ig = bool(a.integrity or a.integrity_log or ig_opts)
    try:
        res = score_files(a.reference, a.distorted, a.model, psnr=bool(a.psnr_log), ssim=bool(a.ssim_log),
                          n_subsample=a.n_subsample, device=local_rank, rank=rank, world_size=world,
                          gather_device=gather_device, max_batch=a.batch, progress=progress, fixed_point=a.fixed_point,
                          **({"float_ssim": True} if a.float_ssim else {}), **({"ms_ssim": True} if a.ms_ssim else {}),
                          **({"ciede": True} if a.ciede else {}), **({"cambi": True} if a.cambi else {}),
                          **({"cambi_full_ref": True} if a.cambi_full_ref else {}),
                          **({"psnr_hvs": True} if a.psnr_hvs else {}),
                          **({"xpsnr": True} if (a.xpsnr or a.xpsnr_log) else {}),
                          **({"siti": True} if a.siti else {}),
                          **({"align": a.align, "align_frames": a.align_frames} if a.align else {}),
                          **({"spatial_align": a.spatial_align, "spatial_frames": a.spatial_frames} if a.spatial_align else {}),
                          **({"level_align": "apply" if a.level_correct else "report", "level_frames": a.level_frames}
                             if (a.level_align or a.level_correct or a.level_curve) else {}),
                          **({"level_curve": True} if a.level_curve else {}),
                          **({"colour_align": "apply" if a.colour_correct else "report", "colour_frames": a.colour_frames}
                             if (a.colour_align or a.colour_correct) else {}),
                          **({"active_picture": "apply" if a.active_crop else "report", "active_frames": a.active_frames,
                              "active_limit": a.active_limit, "active_skip": a.active_skip}
                             if (a.active_picture or a.active_crop) else {}),
                          **({"field_align": "apply" if a.field_correct else "report", "field_frames": a.field_frames,
                              "field_penalty_mse": a.field_penalty_mse} if (a.field_align or a.field_correct) else {}),
                          **({"field_repair": True} if a.field_repair else {}),
                          **({"deinterlace": a.deinterlace, "deinterlace_rate": a.deinterlace_rate, "deinterlace_order": a.field_order,
                              "deinterlace_side": a.deinterlace_side} if a.deinterlace else {}),
                          **({"distortion_map": a.distortion_map, "distortion_planes": a.distortion_planes,
                              "distortion_dir": a.distortion_dir, "distortion_factor": a.distortion_factor,
                              "distortion_min_mse": a.distortion_min_mse} if a.distortion_map else {}),
                          **({"spectrum": a.spectrum, "spectrum_planes": a.spectrum_planes,
                              "spectrum_min_mse": a.spectrum_min_mse, "spectrum_gain_floor": a.spectrum_gain_floor}
                             if a.spectrum else {}),
                          **({"temporal": a.temporal, "temporal_planes": a.temporal_planes, "temporal_min_mse": a.temporal_min_mse,
                              "temporal_blend_min": a.temporal_blend_min, "temporal_still_mse": a.temporal_still_mse,
                              "temporal_pop_factor": a.temporal_pop_factor} if a.temporal else {}),
                          **({"coding_grid": True, "grid_planes": a.grid_planes,
                              "grid_periods": (a.grid_min_period, a.grid_max_period), "grid_z2": a.grid_z2}
                             if a.coding_grid else {}),
                          **({"resize": a.resize} if a.resize else {}),
                          **({"chroma_mismatch": a.chroma_mismatch} if a.chroma_mismatch != "error" else {}),
                          **({"chroma_siting": a.chroma_siting} if a.chroma_siting else {}),
                          **({"rgb_matrix": a.rgb_matrix} if a.rgb_matrix else {}),
                          **({"rgb_range": a.rgb_range} if a.rgb_range else {}),
                          **({"delta_itp": a.delta_itp, "itp_matrix": a.itp_matrix, "itp_range": a.itp_range, "itp_peak": a.itp_peak,
                              "itp_threshold": a.itp_threshold} if a.delta_itp else {}),
                          **({"register": a.register, "register_frames": a.register_frames} if a.register else {}),
                          **({"overlay_mask": a.overlay_mask, "overlay_boxes": overlay_boxes, "overlay_frames": a.overlay_frames,
                              "overlay_tile": a.overlay_tile, "overlay_grow": a.overlay_grow, "overlay_feather": a.overlay_feather}
                             if a.overlay_mask else {}),
                          **({"integrity": True, "integrity_options": ig_opts} if want_ig else {}))
    except Exception as e:  # one line on stderr, non-zero exit: what the caller's returncode check expects
        print(f"pqa2_amd.score: error: {e}", file=sys.stderr, flush=True)
        return 1
    finally:
        if world > 1:
            import torch.distributed as dist
            if dist.is_initialized():
                dist.destroy_process_group()
    if rank == 0:
        log = report.build_vmaf_log(res["metrics"], res["fps"], res["frame_indices"], report.result_log_keys(res))
        report.write_vmaf_json(a.json, log)
        if a.integrity_log and res.get("integrity_lines") is not None:
            with open(a.integrity_log, "w") as f:
                f.write("".join(line + "\n" for line in res["integrity_lines"]))
        if a.xpsnr_log and res.get("xpsnr_lines") is not None:
            with open(a.xpsnr_log, "w") as f:
                f.write("\n".join(res["xpsnr_lines"]) + "\n")
        if a.psnr_log and res["psnr_lines"] is not None:
            with open(a.psnr_log, "w") as f:
                f.write("\n".join(res["psnr_lines"]) + "\n")
        if a.ssim_log and res["ssim_lines"] is not None:
            with open(a.ssim_log, "w") as f:
                f.write("\n".join(res["ssim_lines"]) + "\n")
        if res.get("alignment") and "offset_frames" in res["alignment"]:
            print(report.alignment_summary_line(res["alignment"]), file=sys.stderr, flush=True)
        if res.get("alignment") and res["alignment"].get("active_picture"):
            print(report.active_summary_line(res["alignment"]["active_picture"]), file=sys.stderr, flush=True)
        if res.get("alignment") and res["alignment"].get("spatial"):
            print(report.spatial_summary_line(res["alignment"]["spatial"]), file=sys.stderr, flush=True)
        if res.get("alignment") and res["alignment"].get("levels"):
            print(report.levels_summary_line(res["alignment"]["levels"]), file=sys.stderr, flush=True)
        if res.get("alignment") and res["alignment"].get("colour"):
            print(report.colour_summary_line(res["alignment"]["colour"]), file=sys.stderr, flush=True)
        if res.get("alignment") and res["alignment"].get("geometry"):
            print(report.geometry_summary_line(res["alignment"]["geometry"]), file=sys.stderr, flush=True)
        if res.get("distortion"):
            print(report.distortion_summary_line(res["distortion"]), file=sys.stderr, flush=True)
        if res.get("spectrum"):
            print(report.spectrum_summary_line(res["spectrum"]), file=sys.stderr, flush=True)
        if res.get("temporal"):
            print(report.temporal_summary_line(res["temporal"]), file=sys.stderr, flush=True)
        if res.get("coding_grid"):
            print(report.grid_summary_line(res["coding_grid"]), file=sys.stderr, flush=True)
        if res.get("delta_itp"):
            print(report.itp_summary_line(res["delta_itp"]), file=sys.stderr, flush=True)
        if res.get("overlay"):
            print(report.overlay_summary_line(res["overlay"]), file=sys.stderr, flush=True)
        print(f"VMAF score: {log['pooled_metrics']['vmaf']['mean']:.6f}", file=sys.stderr, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
