"""VMAFAnalyzer -- drop-in for the reference's app/vmaf_analyzer.py:18 `class VMAFAnalyzer(QObject)`.

Same constructor state (app/vmaf_analyzer.py:25-39), setters (:44-137), `terminate_analysis` (:139),
`get_video_metadata` (:162), `analyze_videos(reference_path, distorted_path, model, duration)` (:242)
and result dict (:919-932), same four signals (:20-23) and the same files on disk
(`<test>_<ts>_vmaf.json`, `_psnr.txt`, `_ssim.txt`, :304-311).  What changed is what happens where
the reference spawns `ffmpeg -lavfi libvmaf=...` (:446) and `psnr=`/`ssim=` (:1037,:1067): the
frame pairs go through the MI355X HIP kernels behind include/pqa_vmaf.h instead, all three metrics in
ONE pass over the decoded frames (the reference decodes both files three times).

With PyQt5 importable the class is a real QObject with pyqtSignals, so app/ui/tabs/analysis_tab.py
(:585-640) can use it unchanged; otherwise a small signal shim with the same connect/emit surface is
used (plain callables, as SURVEY.md 8(b) prescribes).
"""
from __future__ import annotations

import json
import logging
import os
import subprocess
import sys
import threading
import time
from datetime import datetime

logger = logging.getLogger(__name__)
_METADATA_CACHE = {}   # (abspath, size, mtime_ns) -> metadata dict of get_video_metadata

try:  # pragma: no cover - PyQt5 is not installed in the build container
    from PyQt5.QtCore import QObject, pyqtSignal
    _HAVE_QT = True
except Exception:
    _HAVE_QT = False

    class _BoundSignal:
        def __init__(self):
            self._slots = []
            self._lock = threading.Lock()

        def connect(self, slot):
            with self._lock:
                self._slots.append(slot)

        def disconnect(self, slot=None):
            with self._lock:
                if slot is None:
                    self._slots.clear()
                else:
                    self._slots.remove(slot)

        def emit(self, *args):
            with self._lock:
                slots = list(self._slots)
            for s in slots:
                s(*args)

    class pyqtSignal:  # noqa: N801 - mirrors the Qt name
        """Class-level declaration that hands every instance its own connect/emit object."""

        def __init__(self, *types):
            self._name = None

        def __set_name__(self, owner, name):
            self._name = "_sig_" + name

        def __get__(self, obj, objtype=None):
            if obj is None:
                return self
            sig = obj.__dict__.get(self._name)
            if sig is None:
                sig = obj.__dict__[self._name] = _BoundSignal()
            return sig

    class QObject:  # noqa: D401
        def __init__(self, *a, **k):
            pass


# Child jobs (torchrun agent + one worker per GPU) run in their own session so that a stop reaches the whole group; the
# price is that a Ctrl-C / SIGTERM aimed at THIS process no longer reaches them.  Every live child is therefore registered
# here: an atexit hook and, where nothing else has claimed them, SIGTERM / SIGINT handlers stop the groups before this
# process goes (the workers also ask the kernel for SIGTERM on parent death, pqa2_amd/score.py).
_LIVE_CHILDREN = set()
_HOOKS_INSTALLED = False


def _stop_live_children():
    for proc in list(_LIVE_CHILDREN):
        try:
            VMAFAnalyzer._stop_child(proc, grace=1.0)
        except Exception:
            pass
        _LIVE_CHILDREN.discard(proc)


def _install_child_hooks():
    global _HOOKS_INSTALLED
    if _HOOKS_INSTALLED:
        return
    _HOOKS_INSTALLED = True
    import atexit
    import signal
    import threading
    atexit.register(_stop_live_children)
    if threading.current_thread() is not threading.main_thread():
        return                                  # signal handlers can only be set from the main thread
    for sig in (signal.SIGTERM, signal.SIGINT):
        try:
            prev = signal.getsignal(sig)
            if prev not in (signal.SIG_DFL, signal.default_int_handler):
                continue                        # the application has its own handler: leave it alone (atexit still runs)

            def handler(signum, frame, _prev=prev):
                _stop_live_children()
                signal.signal(signum, _prev)    # then what would have happened anyway
                os.kill(os.getpid(), signum)
            signal.signal(sig, handler)
        except Exception:
            pass


class VMAFAnalyzer(QObject):
    """VMAF analyzer for measuring video quality with signals for UI integration."""
    analysis_progress = pyqtSignal(int)   # 0-100%
    analysis_complete = pyqtSignal(dict)  # results dict
    error_occurred = pyqtSignal(str)
    status_update = pyqtSignal(str)

    def __init__(self):
        super().__init__()
        self.output_directory = None
        self.test_name = None
        self._process_lock = threading.Lock()
        self._current_process = None
        self._terminate_requested = False
        self.threads = 4                      # kept for interface parity; the GPU path ignores it
        self.pool_method = "mean"
        self.enable_motion_score = False
        self.enable_temporal_features = False
        self.feature_subsample = 1
        self.psnr_enabled = True
        self.ssim_enabled = True
        # extensions (defaults reproduce the reference's behaviour)
        self.device = 0                       # HIP device ordinal for single-process runs
        self.gpus = 1                         # >1: frame-sharded child job, one process per GPU
        self.max_batch = 0                    # 0: the library sizes launches itself
        self.child_backend = "nccl"           # collective backend of the child job: nccl (= RCCL) | gloo
        self.child_share_device = False       # True: every rank of the child job uses device 0 (one-GPU rehearsal)
        self.fixed_point = 0                  # PQA_FIXED_* mask (1 VIF, 2 motion): libvmaf's integer arithmetic, slower
        self.float_ssim_enabled = False       # libvmaf float_ssim (feature=name=float_ssim / ssim=1) per frame and pooled
        self.ms_ssim_enabled = False          # libvmaf float_ms_ssim (feature=name=float_ms_ssim / ms_ssim=1)
        self.ciede_enabled = False            # libvmaf ciede (feature=name=ciede, key ciede2000) per frame and pooled
        self.cambi_enabled = False            # libvmaf cambi banding index (feature=name=cambi) of the distorted luma
        self.cambi_full_ref_enabled = False   # with cambi: cambi_source and cambi_full_reference (full-reference mode)
        self.psnr_hvs_enabled = False         # libvmaf psnr_hvs (feature=name=psnr_hvs): psnr_hvs_y / _cb / _cr, psnr_hvs
        self.xpsnr_enabled = False            # FFmpeg xpsnr: <test>_<ts>_xpsnr.txt stats file, xpsnr_y / _u / _v, xpsnr
        self._xpsnr_path = None               # where this analysis writes the xpsnr stats file (set per analysis)
        self.siti_enabled = False             # FFmpeg siti (ITU-T P.910 SI / TI) of both clips, per frame and pooled
        self.integrity_enabled = False        # FFmpeg freezedetect / blackdetect / scdet on the distorted clip: event lists,
        self.integrity_options = {}           # <test>_<ts>_integrity.txt; FFmpeg's option names (integrity.DEFAULTS)
        self._integrity_path = None           # where this analysis writes the event log (set per analysis)
        self.align_enabled = False            # temporal alignment before scoring: search the frame offset over
        self.align_max_offset = 8             # -align_max_offset ... align_max_offset frames (pipeline.score_files(align=))
        self.spatial_align_enabled = False    # spatial alignment before scoring: search the capture's displacement over
        self.spatial_align_radius = 8         # -radius ... radius pixels in x and y (pipeline.score_files(spatial_align=))
        self.level_align_enabled = False      # level alignment before scoring: measure the capture's gain / offset / range
        self.level_correct_enabled = False    # ... and undo it (implies the measurement; pipeline.score_files(level_align=))
        self.level_curve_enabled = False      # ... with a monotone transfer curve on top: gamma, contrast enhancer (implies the measurement; score_files(level_curve=))
        self.colour_align_enabled = False     # colour-matrix alignment before scoring: measure the capture's 3 x 4 colour map
        self.colour_correct_enabled = False   # ... and undo it (implies the measurement; pipeline.score_files(colour_align=))
        self.active_picture_enabled = False   # active-picture detection before scoring: measure the black bars of both clips
        self.active_crop_enabled = False      # ... and crop both to the common rectangle (implies the measurement; score_files(active_picture=))
        self.field_align_enabled = False      # field alignment before scoring: measure the field structure of the capture
        self.field_correct_enabled = False    # ... and re-weave a field shift or swap (implies the measurement; score_files(field_align=))
        self.deinterlace_mode = None          # deinterlace the captured clip before scoring: None, "adaptive" or "intra" (score_files(deinterlace=))
        self.deinterlace_rate = None          # ... "frame" or "field"; None: frame
        self.field_order = None               # ... "tff" or "bff"; None: the clip's own Y4M I tag
        self.distortion_map_enabled = False   # distortion map: where inside the frame the clips differ (a second pass over both
        self.distortion_tile = 32             # clips; score_files(distortion_map=)); its tile size: 8, 16, 32 or 64
        self.spectrum_enabled = False         # distortion spectrum: what kind of difference the clips have (the same second
        self.spectrum_levels = 4              # pass; score_files(spectrum=)); its number of octaves: 1 ... 6
        self.temporal_enabled = False         # temporal distortion: whether the motion of the capture is wrong (the same second
        self.temporal_tile = 32               # pass; score_files(temporal=)); its tile size: 8, 16, 32 or 64
        self.coding_grid_enabled = False      # coding-grid detection: whether the difference is a block grid (the same second
                                              # pass; score_files(coding_grid=))
        self.delta_itp = None                 # "pq" / "hlg" / "bt1886": the BT.2124 colour difference Delta E ITP of clips with this
                                              # transfer, a pass of its own over both clips (pipeline.score_files(delta_itp=))
        self.itp_matrix = None                # its Y'CbCr matrix and primaries: "bt601" / "bt709" / "bt2020"; None: by the transfer
        self.itp_peak = None                  # its display peak Lw in cd/m2 (hlg, bt1886); None: 1000 / 100
        self.overlay_mask = None              # "report" / "neutral" / "reference": find a burnt-in overlay (logo, clock, timecode)
                                              # and blend it out of the scores (pipeline.score_files(overlay_mask=))
        self.overlay_boxes = None             # [[x0, y0, x1, y1], ...] in luma pixels: mask these instead of detecting
        self.resize_filter = None             # "bilinear" / "bicubic" / "lanczos": resample a distorted clip of another frame
                                              # size to the reference's before scoring (pipeline.score_files(resize=))
        self.register_filter = None           # "bilinear" / "bicubic" / "lanczos": measure the capture's sub-pixel shift and
                                              # scale and undo them with this filter (pipeline.score_files(register=))
        self.chroma_mismatch = "error"        # "luma": clips that differ only in chroma subsampling (a 4:2:2 capture against a
                                              # 4:2:0 master) are scored on their luma (pipeline.score_files(chroma_mismatch=));
                                              # "convert": the distorted clip is converted on the GPU to the reference's chroma
                                              # layout, siting and bit depth, and all three planes are scored
        self.chroma_siting = None             # "left" / "center" / "topleft": with "convert", the siting of both clips' chroma
                                              # instead of what the files imply (pipeline.score_files(chroma_siting=))
        self.rgb_matrix = None                # "bt601" / "bt709" / "bt2020": the matrix a packed RGB capture (.bgra ... .r210) is
                                              # converted with (pipeline.score_files(rgb_matrix=)); None: by the picture height
        self.rgb_range = None                 # "full" / "limited" R'G'B' of such a capture; None: full at 8 bit, limited for r210
        self.last_fps = 0.0
        self._engine_factory = None           # tests inject a stand-in; product code leaves it None

    # ---- option plumbing (app/vmaf_analyzer.py:44-137) ------------------------------------------
    def set_options_from_manager(self, options_manager):
        if not options_manager:
            logger.warning("No options manager provided, using default settings")
            return
        try:
            s = options_manager.get_setting("vmaf")
            self.threads = s.get("threads", 4)
            self.feature_subsample = s.get("feature_subsample", 1)
            self.pool_method = s.get("pool_method", "mean")
            self.enable_motion_score = s.get("enable_motion_score", False)
            self.enable_temporal_features = s.get("enable_temporal_features", False)
            self.psnr_enabled = s.get("psnr_enabled", True)
            self.ssim_enabled = s.get("ssim_enabled", True)
            self.float_ssim_enabled = bool(s.get("float_ssim_enabled", False))
            self.ms_ssim_enabled = bool(s.get("ms_ssim_enabled", False))
            self.ciede_enabled = bool(s.get("ciede_enabled", False))
            self.cambi_enabled = bool(s.get("cambi_enabled", False))
            self.cambi_full_ref_enabled = bool(s.get("cambi_full_ref_enabled", False))
            self.psnr_hvs_enabled = bool(s.get("psnr_hvs_enabled", False))
            self.xpsnr_enabled = bool(s.get("xpsnr_enabled", False))
            self.siti_enabled = bool(s.get("siti_enabled", False))
            self.integrity_enabled = bool(s.get("integrity_enabled", False))
            self.integrity_options = dict(s.get("integrity_options", {}) or {})
            logger.info(f"VMAF options set from manager: threads={self.threads}, "
                        f"feature_subsample={self.feature_subsample}, pool={self.pool_method}")
        except Exception as e:
            logger.error(f"Error setting VMAF options from manager: {e}")
        for section in ("bookend", "analysis"):   # the alignment switches live beside the bookend settings; `analysis` overrides
            try:
                s = options_manager.get_setting(section) or {}
            except Exception:
                continue
            if "align_enabled" in s:
                self.align_enabled = bool(s["align_enabled"])
            if "align_max_offset" in s:
                self.align_max_offset = max(1, min(64, int(s["align_max_offset"])))
            if "spatial_align_enabled" in s:
                self.spatial_align_enabled = bool(s["spatial_align_enabled"])
            if "spatial_align_radius" in s:
                self.spatial_align_radius = max(1, min(16, int(s["spatial_align_radius"])))
            if "level_align_enabled" in s:
                self.level_align_enabled = bool(s["level_align_enabled"])
            if "level_correct_enabled" in s:
                self.level_correct_enabled = bool(s["level_correct_enabled"])
            if "level_curve_enabled" in s:
                self.level_curve_enabled = bool(s["level_curve_enabled"])
            if "colour_align_enabled" in s:
                self.colour_align_enabled = bool(s["colour_align_enabled"])
            if "colour_correct_enabled" in s:
                self.colour_correct_enabled = bool(s["colour_correct_enabled"])
            if "active_picture_enabled" in s:
                self.active_picture_enabled = bool(s["active_picture_enabled"])
            if "active_crop_enabled" in s:
                self.active_crop_enabled = bool(s["active_crop_enabled"])
            if "field_align_enabled" in s:
                self.field_align_enabled = bool(s["field_align_enabled"])
            if "field_correct_enabled" in s:
                self.field_correct_enabled = bool(s["field_correct_enabled"])
            for key in ("deinterlace_mode", "deinterlace_rate", "field_order"):
                if key in s:
                    setattr(self, key, s[key] or None)
            if "distortion_map_enabled" in s:
                self.distortion_map_enabled = bool(s["distortion_map_enabled"])
            if "distortion_tile" in s:
                self.distortion_tile = int(s["distortion_tile"])
            if "spectrum_enabled" in s:
                self.spectrum_enabled = bool(s["spectrum_enabled"])
            if "spectrum_levels" in s:
                self.spectrum_levels = int(s["spectrum_levels"])
            if "temporal_enabled" in s:
                self.temporal_enabled = bool(s["temporal_enabled"])
            if "temporal_tile" in s:
                self.temporal_tile = int(s["temporal_tile"])
            if "coding_grid_enabled" in s:
                self.coding_grid_enabled = bool(s["coding_grid_enabled"])

    set_options_manager = set_options_from_manager

    def set_output_directory(self, output_dir):
        self.output_directory = output_dir
        logger.info(f"Set output directory to: {self.output_directory}")

    def set_test_name(self, test_name):
        self.test_name = test_name
        logger.info(f"Set test name to: {test_name}")

    def set_advanced_options(self, pool_method="mean", enable_motion_score=False, enable_temporal_features=False,
                             feature_subsample=1, psnr_enabled=True, ssim_enabled=True, float_ssim_enabled=False,
                             ms_ssim_enabled=False, ciede_enabled=False, cambi_enabled=False,
                             cambi_full_ref_enabled=False, psnr_hvs_enabled=False, xpsnr_enabled=False,
                             siti_enabled=False, integrity_enabled=False, integrity_options=None,
                             align_enabled=False, align_max_offset=8, spatial_align_enabled=False,
                             spatial_align_radius=8, level_align_enabled=False, level_correct_enabled=False,
                             colour_align_enabled=False, colour_correct_enabled=False, active_picture_enabled=False,
                             active_crop_enabled=False, distortion_map_enabled=False, distortion_tile=32,
                             spectrum_enabled=False, spectrum_levels=4, temporal_enabled=False, temporal_tile=32,
                             coding_grid_enabled=False, level_curve_enabled=False):
        self.pool_method = pool_method
        self.enable_motion_score = enable_motion_score
        self.enable_temporal_features = enable_temporal_features
        self.feature_subsample = feature_subsample
        self.psnr_enabled = psnr_enabled
        self.ssim_enabled = ssim_enabled
        self.float_ssim_enabled = bool(float_ssim_enabled)
        self.ms_ssim_enabled = bool(ms_ssim_enabled)
        self.ciede_enabled = bool(ciede_enabled)
        self.cambi_enabled = bool(cambi_enabled)
        self.cambi_full_ref_enabled = bool(cambi_full_ref_enabled)
        self.psnr_hvs_enabled = bool(psnr_hvs_enabled)
        self.xpsnr_enabled = bool(xpsnr_enabled)
        self.siti_enabled = bool(siti_enabled)
        self.integrity_enabled = bool(integrity_enabled)
        self.integrity_options = dict(integrity_options or {})
        self.align_enabled = bool(align_enabled)
        self.align_max_offset = max(1, min(64, int(align_max_offset)))
        self.spatial_align_enabled = bool(spatial_align_enabled)
        self.spatial_align_radius = max(1, min(16, int(spatial_align_radius)))
        self.level_align_enabled = bool(level_align_enabled)
        self.level_correct_enabled = bool(level_correct_enabled)
        self.level_curve_enabled = bool(level_curve_enabled)
        self.colour_align_enabled = bool(colour_align_enabled)
        self.colour_correct_enabled = bool(colour_correct_enabled)
        self.active_picture_enabled = bool(active_picture_enabled)
        self.active_crop_enabled = bool(active_crop_enabled)
        self.distortion_map_enabled = bool(distortion_map_enabled)
        self.distortion_tile = int(distortion_tile)
        self.spectrum_enabled = bool(spectrum_enabled)
        self.spectrum_levels = int(spectrum_levels)
        self.temporal_enabled = bool(temporal_enabled)
        self.temporal_tile = int(temporal_tile)
        self.coding_grid_enabled = bool(coding_grid_enabled)

    def terminate_analysis(self):
        """Terminate a running analysis (legal from another thread, like the reference's)."""
        self._terminate_requested = True
        proc = self._current_process
        if proc is not None:
            try:
                self._stop_child(proc)
            except Exception as e:
                logger.error(f"Error terminating VMAF process: {e}")

    @staticmethod
    def _stop_child(proc, grace=3.0):
        """The child job is a torchrun agent PLUS one worker per GPU (the reference had a single ffmpeg child).  It is
        started as its own session, so SIGTERM goes to the whole process group, and after `grace` seconds SIGKILL does:
        no worker is left behind holding a GPU context or blocked in the RCCL gather."""
        import signal
        if proc.poll() is not None:
            return
        try:
            pgid = os.getpgid(proc.pid)
        except ProcessLookupError:
            return
        own_group = pgid == proc.pid      # only signal a group this analyzer created (start_new_session=True)
        try:
            os.killpg(pgid, signal.SIGTERM) if own_group else proc.terminate()
        except ProcessLookupError:
            return
        try:
            proc.wait(timeout=grace)
        except subprocess.TimeoutExpired:
            pass
        try:
            os.killpg(pgid, signal.SIGKILL) if own_group else proc.kill()   # stragglers of the group, if any
        except ProcessLookupError:
            pass

    # ---- metadata (replaces the ffprobe call, app/vmaf_analyzer.py:162-240) -------------------------
    def get_video_metadata(self, video_path, ffprobe_exe=None):
        try:
            from .yuvio import open_video
            # one analysis asks four times for the same two files (app/vmaf_analyzer.py:320-321, :919-920): the answer is
            # kept per (path, size, mtime) -- opening a clip maps it and finds its frames
            st = os.stat(video_path)
            key = (os.path.abspath(video_path), st.st_size, st.st_mtime_ns)
            hit = _METADATA_CACHE.get(key)
            if hit is not None:
                logger.info(f"Video metadata extracted: {hit['width']}x{hit['height']} @ {hit['frame_rate']}fps")
                return dict(hit, path=video_path)
            info = open_video(video_path).info
            fps = info.fps
            md = {
                "path": video_path,
                "duration": (info.n_frames / fps) if fps else 0.0,
                "frame_rate": fps,
                "width": info.width,
                "height": info.height,
                "pix_fmt": info.pix_fmt,
                "codec_name": "rawvideo",
                "bit_rate": int(info.frame_bytes * 8 * fps) if fps else 0,
                "nb_frames": info.n_frames,
            }
            logger.info(f"Video metadata extracted: {md['width']}x{md['height']} @ {md['frame_rate']}fps")
            if len(_METADATA_CACHE) > 64:
                _METADATA_CACHE.clear()
            _METADATA_CACHE[key] = dict(md)
            return md
        except Exception as e:
            logger.error(f"Error extracting video metadata: {e}")
            return None

    # ---- the entry point (app/vmaf_analyzer.py:242-616) ---------------------------------------------
    def analyze_videos(self, reference_path, distorted_path, model="vmaf_v0.6.1", duration=None):
        """Score `distorted_path` against `reference_path`.  Returns the results dict or None;
        never raises (errors go to `error_occurred`, as in the reference).  `duration` is accepted and
        unused, exactly like the reference's."""
        with self._process_lock:
            try:
                self._terminate_requested = False
                self.status_update.emit(f"Analyzing videos with model: {model}")
                logger.info(f"Starting VMAF analysis with model: {model}")
                if not os.path.exists(reference_path):
                    return self._fail(f"Reference video not found: {reference_path}")
                if not os.path.exists(distorted_path):
                    return self._fail(f"Distorted video not found: {distorted_path}")

                output_dir = self.output_directory or os.path.dirname(reference_path)
                timestamp = datetime.now().strftime("%Y%m%d_%H%M%S")
                test_name = self.test_name or "Test"
                parent_dir = os.path.dirname(reference_path)
                if test_name and test_name in parent_dir:
                    test_dir = parent_dir
                else:
                    test_dir = os.path.join(output_dir, f"{test_name}_{timestamp}")
                    os.makedirs(test_dir, exist_ok=True)
                json_path = os.path.join(test_dir, f"{test_name}_{timestamp}_vmaf.json")
                psnr_path = os.path.join(test_dir, f"{test_name}_{timestamp}_psnr.txt")
                ssim_path = os.path.join(test_dir, f"{test_name}_{timestamp}_ssim.txt")
                self._xpsnr_path = (os.path.join(test_dir, f"{test_name}_{timestamp}_xpsnr.txt")
                                    if self.xpsnr_enabled else None)
                self._integrity_path = (os.path.join(test_dir, f"{test_name}_{timestamp}_integrity.txt")
                                        if self.integrity_enabled else None)

                self.get_video_metadata(reference_path)
                dist_meta = self.get_video_metadata(distorted_path)
                total_frames = 0
                if dist_meta:
                    if dist_meta.get("nb_frames", 0) > 0:
                        total_frames = dist_meta["nb_frames"]
                    elif dist_meta.get("frame_rate", 0) > 0 and dist_meta.get("duration", 0) > 0:
                        total_frames = int(dist_meta["frame_rate"] * dist_meta["duration"])
                if model is None:
                    model = "vmaf_v0.6.1"

                self.analysis_progress.emit(0)
                self.status_update.emit("Starting VMAF analysis...")
                ok = (self._run_child_job if self.gpus > 1 else self._run_in_process)(
                    reference_path, distorted_path, model, json_path,
                    psnr_path if self.psnr_enabled else None, ssim_path if self.ssim_enabled else None,
                    total_frames)
                if not ok:
                    return None
                if self.psnr_enabled or self.ssim_enabled:
                    # one pass already produced these; the status lines keep the reference's sequence
                    self.status_update.emit("VMAF completed, running PSNR/SSIM analysis...")
                return self._parse_vmaf_results(json_path, psnr_path if self.psnr_enabled else None,
                                                ssim_path if self.ssim_enabled else None,
                                                distorted_path, reference_path)
            except Exception as e:
                import traceback
                logger.error(traceback.format_exc())
                return self._fail(f"Error in VMAF analysis: {e}")

    analyze = analyze_videos  # BASELINE.json's name for the entry point

    def _fail(self, msg):
        logger.error(msg)
        self.error_occurred.emit(msg)
        return None

    def _emit_progress(self, done, total, state):
        if total <= 0:
            return
        progress = min(95, int(done / total * 100))
        now = time.time()
        if now - state["t"] > 0.5:
            state["t"] = now
            self.analysis_progress.emit(progress)
            self.status_update.emit(f"Processing frame {done}/{total} ({progress}%)")

    def _run_in_process(self, ref, dis, model, json_path, psnr_path, ssim_path, total_frames):
        from . import _native as N
        from . import report
        from .pipeline import score_files
        state = {"t": time.time()}
        try:
            res = score_files(ref, dis, model, psnr=bool(psnr_path), ssim=bool(ssim_path),
                              n_subsample=max(1, int(self.feature_subsample or 1)), device=self.device,
                              max_batch=self.max_batch, engine_factory=self._engine_factory,
                              fixed_point=self.fixed_point, **self._ssim_family_kwargs(),
                              progress=lambda d, t: self._emit_progress(d, total_frames or t, state),
                              cancelled=lambda: self._terminate_requested)
        except N.PqaCancelled:
            self._fail("VMAF analysis was terminated by user")
            return False
        except Exception as e:
            self._fail(f"Error running VMAF analysis: {e}")
            return False
        if self._terminate_requested:
            self._fail("VMAF analysis was terminated by user")
            return False
        self.last_fps = res["fps"]
        log = report.build_vmaf_log(res["metrics"], res["fps"], res["frame_indices"], report.result_log_keys(res))
        report.write_vmaf_json(json_path, log)
        if self.integrity_enabled and self._integrity_path and res.get("integrity_lines") is not None:
            with open(self._integrity_path, "w") as f:
                f.write("".join(line + "\n" for line in res["integrity_lines"]))
        if self.xpsnr_enabled and self._xpsnr_path and res.get("xpsnr_lines") is not None:
            with open(self._xpsnr_path, "w") as f:
                f.write("\n".join(res["xpsnr_lines"]) + "\n")
        if psnr_path and res["psnr_lines"] is not None:
            self.status_update.emit("Running PSNR analysis...")
            with open(psnr_path, "w") as f:
                f.write("\n".join(res["psnr_lines"]) + "\n")
        if ssim_path and res["ssim_lines"] is not None:
            self.status_update.emit("Running SSIM analysis...")
            with open(ssim_path, "w") as f:
                f.write("\n".join(res["ssim_lines"]) + "\n")
        return True

    def _ssim_family_kwargs(self):
        """score_files keywords of the extension features (SSIM family, ciede, cambi, psnr_hvs): only the enabled ones (the
        default call is the one it always was).  cambi_full_ref counts only together with cambi."""
        return {**({"float_ssim": True} if self.float_ssim_enabled else {}),
                **({"ms_ssim": True} if self.ms_ssim_enabled else {}),
                **({"ciede": True} if self.ciede_enabled else {}),
                **({"cambi": True} if self.cambi_enabled else {}),
                **({"cambi_full_ref": True} if self.cambi_enabled and self.cambi_full_ref_enabled else {}),
                **({"psnr_hvs": True} if self.psnr_hvs_enabled else {}),
                **({"xpsnr": True} if self.xpsnr_enabled else {}),
                **({"siti": True} if self.siti_enabled else {}),
                **({"integrity": True, "integrity_options": dict(self.integrity_options)} if self.integrity_enabled else {}),
                **({"align": int(self.align_max_offset)} if self.align_enabled else {}),
                **({"spatial_align": int(self.spatial_align_radius)} if self.spatial_align_enabled else {}),
                **({"level_align": "apply" if self.level_correct_enabled else "report"}
                   if (self.level_align_enabled or self.level_correct_enabled or self.level_curve_enabled) else {}),
                **({"level_curve": True} if self.level_curve_enabled else {}),
                **({"colour_align": "apply" if self.colour_correct_enabled else "report"}
                   if (self.colour_align_enabled or self.colour_correct_enabled) else {}),
                **({"active_picture": "apply" if self.active_crop_enabled else "report"}
                   if (self.active_picture_enabled or self.active_crop_enabled) else {}),
                **({"field_align": "apply" if self.field_correct_enabled else "report"}
                   if (self.field_align_enabled or self.field_correct_enabled) else {}),
                **({"deinterlace": self.deinterlace_mode, "deinterlace_rate": self.deinterlace_rate or "frame",
                    "deinterlace_order": self.field_order} if self.deinterlace_mode else {}),
                **({"distortion_map": int(self.distortion_tile)} if self.distortion_map_enabled else {}),
                **({"spectrum": int(self.spectrum_levels)} if self.spectrum_enabled else {}),
                **({"temporal": int(self.temporal_tile)} if self.temporal_enabled else {}),
                **({"coding_grid": True} if self.coding_grid_enabled else {}),
                **({"delta_itp": self.delta_itp, "itp_matrix": self.itp_matrix, "itp_peak": self.itp_peak} if self.delta_itp else {}),
                **({"overlay_mask": self.overlay_mask, "overlay_boxes": self.overlay_boxes} if self.overlay_mask else {}),
                **({"resize": self.resize_filter} if self.resize_filter else {}),
                **({"register": self.register_filter} if self.register_filter else {}),
                **({"chroma_mismatch": self.chroma_mismatch} if self.chroma_mismatch != "error" else {}),
                **({"chroma_siting": self.chroma_siting} if self.chroma_siting else {}),
                **({"rgb_matrix": self.rgb_matrix} if self.rgb_matrix else {}),
                **({"rgb_range": self.rgb_range} if self.rgb_range else {})}

    def _run_child_job(self, ref, dis, model, json_path, psnr_path, ssim_path, total_frames):
        """Frame-sharded run: one process per GPU under torch.distributed.run, driven like the
        reference drives its ffmpeg child (stderr `frame=` lines, terminate -> kill, return code)."""
        import socket
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={self.gpus}",
               "--master-addr", "127.0.0.1", "--master-port", str(port), "-m", "pqa2_amd.score",
               ref, dis, "--model", model, "--json", json_path,
               "--n-subsample", str(max(1, int(self.feature_subsample or 1))), "--batch", str(self.max_batch)]
        if self.fixed_point:
            cmd += ["--fixed-point", str(int(self.fixed_point))]
        if self.float_ssim_enabled:
            cmd += ["--float-ssim"]
        if self.ms_ssim_enabled:
            cmd += ["--ms-ssim"]
        if self.ciede_enabled:
            cmd += ["--ciede"]
        if self.cambi_enabled:
            cmd += ["--cambi"] + (["--cambi-full-ref"] if self.cambi_full_ref_enabled else [])
        if self.psnr_hvs_enabled:
            cmd += ["--psnr-hvs"]
        if self.xpsnr_enabled:
            cmd += ["--xpsnr"] + (["--xpsnr-log", self._xpsnr_path] if self._xpsnr_path else [])
        if self.siti_enabled:
            cmd += ["--siti"]
        if self.integrity_enabled:
            cmd += ["--integrity"] + (["--integrity-log", self._integrity_path] if self._integrity_path else [])
            for k, v in self.integrity_options.items():
                cmd += ["--" + k.replace("_", "-"), str(v)]
        if self.align_enabled:
            cmd += ["--align", str(int(self.align_max_offset))]
        if self.spatial_align_enabled:
            cmd += ["--spatial-align", str(int(self.spatial_align_radius))]
        if self.level_correct_enabled:
            cmd += ["--level-correct"]
        elif self.level_align_enabled:
            cmd += ["--level-align"]
        if self.level_curve_enabled:
            cmd += ["--level-curve"]
        if self.colour_correct_enabled:
            cmd += ["--colour-correct"]
        elif self.colour_align_enabled:
            cmd += ["--colour-align"]
        if self.active_crop_enabled:
            cmd += ["--active-crop"]
        elif self.active_picture_enabled:
            cmd += ["--active-picture"]
        if self.field_correct_enabled:
            cmd += ["--field-correct"]
        elif self.field_align_enabled:
            cmd += ["--field-align"]
        if self.deinterlace_mode:
            cmd += ["--deinterlace", self.deinterlace_mode, "--deinterlace-rate", self.deinterlace_rate or "frame"]
            if self.field_order:
                cmd += ["--field-order", self.field_order]
        if self.distortion_map_enabled:
            cmd += ["--distortion-map", str(int(self.distortion_tile))]
        if self.spectrum_enabled:
            cmd += ["--spectrum", str(int(self.spectrum_levels))]
        if self.temporal_enabled:
            cmd += ["--temporal", str(int(self.temporal_tile))]
        if self.coding_grid_enabled:
            cmd += ["--coding-grid"]
        if self.delta_itp:
            cmd += ["--delta-itp", str(self.delta_itp)]
            if self.itp_matrix:
                cmd += ["--itp-matrix", str(self.itp_matrix)]
            if self.itp_peak is not None:
                cmd += ["--itp-peak", str(float(self.itp_peak))]
        if self.overlay_mask:
            cmd += ["--overlay-mask", str(self.overlay_mask)]
            for box in self.overlay_boxes or []:
                cmd += ["--overlay-box", ",".join(str(int(v)) for v in box)]
        if self.resize_filter:
            cmd += ["--resize", str(self.resize_filter)]
        if self.register_filter:
            cmd += ["--register", str(self.register_filter)]
        if self.chroma_mismatch != "error":
            cmd += ["--chroma-mismatch", str(self.chroma_mismatch)]
        if self.chroma_siting:
            cmd += ["--chroma-siting", str(self.chroma_siting)]
        if self.rgb_matrix:
            cmd += ["--rgb-matrix", str(self.rgb_matrix)]
        if self.rgb_range:
            cmd += ["--rgb-range", str(self.rgb_range)]
        if self.child_backend != "nccl":
            cmd += ["--backend", self.child_backend]
        if self.child_share_device:
            cmd += ["--share-device"]
        if psnr_path:
            cmd += ["--psnr-log", psnr_path]
        if ssim_path:
            cmd += ["--ssim-log", ssim_path]
        env = os.environ.copy()
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        env["PYTHONPATH"] = root + os.pathsep + env.get("PYTHONPATH", "")
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        state = {"t": time.time()}
        stderr_lines = []
        try:
            _install_child_hooks()
            self._current_process = subprocess.Popen(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True,
                                                     bufsize=1, env=env, start_new_session=True)
            _LIVE_CHILDREN.add(self._current_process)
            for line in iter(self._current_process.stderr.readline, ""):
                if self._terminate_requested:
                    break
                stderr_lines.append(line)
                if "frame=" in line:
                    tok = line.split("frame=")[1].split()
                    if tok and tok[0].isdigit():
                        self._emit_progress(int(tok[0]), total_frames, state)
            if self._terminate_requested:
                self.terminate_analysis()
            returncode = self._current_process.wait(timeout=60)
        except Exception as e:
            self._fail(f"Error running VMAF analysis: {e}")
            return False
        finally:
            proc, self._current_process = self._current_process, None
            if proc is not None and proc.poll() is None:
                self._stop_child(proc, grace=1.0)
            _LIVE_CHILDREN.discard(proc)
        if self._terminate_requested:
            self._fail("VMAF analysis was terminated by user")
            return False
        if returncode != 0:
            self._fail(f"VMAF analysis failed with return code {returncode}: {''.join(stderr_lines[-20:])}")
            return False
        return True

    # ---- result assembly (app/vmaf_analyzer.py:628-980) ---------------------------------------------
    def _parse_vmaf_results(self, json_path, psnr_path, ssim_path, distorted_path, reference_path):
        try:
            if not os.path.exists(json_path):
                return self._fail("VMAF analysis completed but JSON output file not found")
            with open(json_path, "r") as f:
                vmaf_data = json.load(f)
            vmaf_score = psnr_score = ssim_score = None
            if "pooled_metrics" in vmaf_data:
                pool = vmaf_data["pooled_metrics"]
                if "vmaf" in pool:
                    vmaf_score = pool["vmaf"]["mean"]
                for k in ("psnr", "psnr_y"):
                    if k in pool:
                        psnr_score = pool[k]["mean"]
                for k in ("ssim", "ssim_y"):
                    if k in pool:
                        ssim_score = pool[k]["mean"]
            elif vmaf_data.get("frames"):
                vals = [fr["metrics"]["vmaf"] for fr in vmaf_data["frames"] if "vmaf" in fr.get("metrics", {})]
                if vals:
                    vmaf_score = sum(vals) / len(vals)
            logger.info(f"VMAF Score: {vmaf_score}")
            logger.info(f"PSNR Score: {psnr_score}")
            logger.info(f"SSIM Score: {ssim_score}")

            dist_meta = self.get_video_metadata(distorted_path)
            self.get_video_metadata(reference_path)
            width = dist_meta.get("width", 0) if dist_meta else 0
            height = dist_meta.get("height", 0) if dist_meta else 0
            psnr_status = os.path.basename(psnr_path) if psnr_path and os.path.exists(psnr_path) else "Not Available"
            ssim_status = os.path.basename(ssim_path) if ssim_path and os.path.exists(ssim_path) else "Not Available"
            model_info = vmaf_data.get("model", vmaf_data.get("version", "unknown"))
            results = {
                "vmaf_score": vmaf_score,
                "psnr_score": psnr_status,     # file name or status text, as in the reference (:921)
                "ssim_score": ssim_status,
                "json_path": json_path,
                "psnr_log": psnr_path,
                "ssim_log": ssim_path,
                "reference_video": os.path.basename(reference_path) if reference_path else "",
                "distorted_video": os.path.basename(distorted_path) if distorted_path else "",
                "raw_results": vmaf_data,
                "model": model_info,
                "width": width,
                "height": height,
            }
            pooled = vmaf_data.get("pooled_metrics", {})
            for enabled, key in ((self.float_ssim_enabled, "float_ssim"), (self.ms_ssim_enabled, "float_ms_ssim"),
                                 (self.ciede_enabled, "ciede2000"), (self.cambi_enabled, "cambi"),
                                 (self.cambi_enabled and self.cambi_full_ref_enabled, "cambi_source"),
                                 (self.cambi_enabled and self.cambi_full_ref_enabled, "cambi_full_reference"),
                                 (self.psnr_hvs_enabled, "psnr_hvs_y"), (self.psnr_hvs_enabled, "psnr_hvs_cb"),
                                 (self.psnr_hvs_enabled, "psnr_hvs_cr"), (self.psnr_hvs_enabled, "psnr_hvs")):
                if enabled:
                    results[key] = pooled[key]["mean"] if key in pooled else None
            if self.xpsnr_enabled:   # FFmpeg's clip summary (square-mean-root), from the log's top level
                for key in ("xpsnr_y", "xpsnr_u", "xpsnr_v", "xpsnr"):
                    results[key] = vmaf_data.get(key)
                results["xpsnr_log"] = self._xpsnr_path
            if self.siti_enabled:   # pooled means of both clips, and the distorted clip's maxima (FFmpeg's summary)
                for key in ("siti_si", "siti_ti", "siti_si_source", "siti_ti_source"):
                    results[key] = pooled[key]["mean"] if key in pooled else None
                for key in ("siti_si", "siti_ti"):
                    results[key + "_max"] = pooled[key]["max"] if key in pooled else None
            if self.integrity_enabled:   # the event lists, from the log's top level
                results["integrity"] = vmaf_data.get("integrity")
                results["integrity_log"] = self._integrity_path
            if (self.align_enabled or self.spatial_align_enabled or self.level_align_enabled
                    or self.level_correct_enabled or self.level_curve_enabled or self.register_filter or self.colour_align_enabled
                    or self.colour_correct_enabled or self.active_picture_enabled
                    or self.active_crop_enabled or self.field_align_enabled
                    or self.field_correct_enabled):   # how the clips were paired, from the log's top level
                from . import report
                results["alignment"] = vmaf_data.get("alignment")
                if results["alignment"] and "offset_frames" in results["alignment"]:
                    self.status_update.emit(report.alignment_summary_line(results["alignment"]))
                if results["alignment"] and results["alignment"].get("active_picture"):
                    active = results["alignment"]["active_picture"]
                    self.status_update.emit(report.active_summary_line(active))
                    if active.get("applied"):   # the clips were scored without their bars: report the scored size
                        left, top, right, bottom = active["crop"]
                        results["width"], results["height"] = width - left - right, height - top - bottom
                if results["alignment"] and results["alignment"].get("spatial"):
                    self.status_update.emit(report.spatial_summary_line(results["alignment"]["spatial"]))
                if results["alignment"] and results["alignment"].get("levels"):
                    self.status_update.emit(report.levels_summary_line(results["alignment"]["levels"]))
                if results["alignment"] and results["alignment"].get("colour"):
                    self.status_update.emit(report.colour_summary_line(results["alignment"]["colour"]))
                if results["alignment"] and results["alignment"].get("geometry"):
                    self.status_update.emit(report.geometry_summary_line(results["alignment"]["geometry"]))
            if self.distortion_map_enabled:   # where the clips differ, from the log's top level
                from . import report
                results["distortion"] = vmaf_data.get("distortion")
                if results["distortion"]:
                    self.status_update.emit(report.distortion_summary_line(results["distortion"]))
            if self.spectrum_enabled:   # what kind of difference the clips have, from the log's top level
                from . import report
                results["spectrum"] = vmaf_data.get("spectrum")
                if results["spectrum"]:
                    self.status_update.emit(report.spectrum_summary_line(results["spectrum"]))
            if self.temporal_enabled:   # whether the motion is wrong, from the log's top level
                from . import report
                results["temporal"] = vmaf_data.get("temporal")
                if results["temporal"]:
                    self.status_update.emit(report.temporal_summary_line(results["temporal"]))
            if self.coding_grid_enabled:   # whether the difference is a block grid, from the log's top level
                from . import report
                results["coding_grid"] = vmaf_data.get("coding_grid")
                if results["coding_grid"]:
                    self.status_update.emit(report.grid_summary_line(results["coding_grid"]))
            if self.delta_itp:   # whether the colour error is visible, from the log's top level
                from . import report
                results["delta_itp"] = vmaf_data.get("delta_itp")
                if results["delta_itp"]:
                    self.status_update.emit(report.itp_summary_line(results["delta_itp"]))
            if self.overlay_mask:   # the burnt-in overlay and what was done about it, from the log's top level
                from . import report
                results["overlay"] = vmaf_data.get("overlay")
                if results["overlay"]:
                    self.status_update.emit(report.overlay_summary_line(results["overlay"]))
            self.analysis_progress.emit(100)
            self.status_update.emit(f"VMAF analysis complete! Score: {vmaf_score:.2f}")
            self.analysis_complete.emit(results)
            return results
        except Exception as e:
            import traceback
            logger.error(traceback.format_exc())
            return self._fail(f"Error parsing VMAF results: {e}")
