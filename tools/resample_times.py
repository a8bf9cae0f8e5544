#!/usr/bin/env python3
"""Time per plane of the exact-integer resampler (pqa_resample_device) on 8 resident planes of uniform noise: 960x540 ->
1920x1080 and 1920x1080 -> 3840x2160 (8 bit; bicubic and Lanczos-3), 3840x2160 -> 1920x1080 (8 bit, bicubic) and the 10-bit
form of the first, beside two yardsticks taken in the same run: one luma PSNR pass at the DESTINATION size (the luma-only sse
kernel of the same build, HIP events around a resident run, as tools/level_times.py takes it) and the traffic floor (source
bytes + destination bytes) / 8 TB/s.  The resample call is synchronous (one kernel launch for the 8 planes, ends in a stream
synchronise), so a host clock around the call is the time; best of --rounds after a warm-up call, which also builds and
uploads the tables.  One plane of every case is checked against the numpy restatement fed with the library's tables.
Then the end-to-end cost of score_files(resize="bicubic") on a 960x540 4:2:0 clip against a 1920x1080 reference, beside
score_files on a file holding the same clip already resampled (the resized frames come back to the host and go down again).
usage: python tools/resample_times.py [--frames 8] [--rounds 5] [--e2e-frames 24] [--out FILE]"""
import argparse, ctypes as C, os, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from pqa2_amd import _native as N
from pqa2_amd.engine import FeatureEngine
from tests import resample_ref as R

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=8)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--e2e-frames", type=int, default=24)
ap.add_argument("--out", default=None, help="also append the result lines to this file")
a = ap.parse_args()
HBM_BYTES_PER_US = 8.0e6   # 8 TB/s


def lib_dense(lib, filt, n_src, n_dst):
    first, coeff, taps = np.zeros(n_dst, np.int32), np.zeros((n_dst, 32), np.int16), C.c_int32()
    assert lib.pqa_debug_resample_table(R.FILTERS[filt], n_src, n_dst, 0, n_src * R.Q16, first.ctypes.data, coeff.ctypes.data, 32,
                                        C.byref(taps)) == 0
    return R.dense(first, coeff, n_src)


def resample(sw, sh, dw, dh, bpc, filt, n):
    dt = torch.uint8 if bpc == 8 else torch.int16
    gen = torch.Generator(device="cuda")
    gen.manual_seed(99)
    src = torch.randint(0, 1 << bpc, (n, sh, sw), generator=gen, device="cuda", dtype=torch.int32).to(dt)
    dst = torch.zeros((n, dh, dw), device="cuda", dtype=dt)
    es = src.element_size()
    torch.cuda.synchronize()
    with FeatureEngine(dw, dh, bit_depth=bpc, n_planes=1, features=N.FEAT_PSNR, max_batch=8, result_capacity=16) as eng:
        args = (src.data_ptr(), sw * es, sw * sh * es, (sh, sw), dst.data_ptr(), dw * es, dw * dh * es, (dh, dw), n, filt)
        eng.resample_resident(*args)   # warm-up: code objects, the tables of first use
        best = None
        for _ in range(a.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.resample_resident(*args)
            us = (time.perf_counter() - t0) * 1e6 / n
            best = us if best is None else min(best, us)
        np_dt = np.uint8 if bpc == 8 else np.uint16
        # the bottom right corner of the last plane (40 rows, 72 columns: two tiles each way) from the source samples it reads
        th, tv = lib_dense(eng.lib, filt, sw, dw)[dw - 72:], lib_dense(eng.lib, filt, sh, dh)[dh - 40:]
        cols, rows = np.flatnonzero(th.any(axis=0)), np.flatnonzero(tv.any(axis=0))
        want = R.apply(src[n - 1].cpu().numpy().view(np_dt)[np.ix_(rows, cols)], th[:, cols], tv[:, rows], bpc)
        assert np.array_equal(dst[n - 1].cpu().numpy().view(np_dt)[dh - 40:, dw - 72:], want)
    return best


def psnr_luma(w, h, bpc, n):
    dt = torch.uint8 if bpc == 8 else torch.int16
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    ref = torch.randint(0, 1 << bpc, (n, h, w), generator=gen, device="cuda", dtype=torch.int32).to(dt)
    dis = torch.randint(0, 1 << bpc, (n, h, w), generator=gen, device="cuda", dtype=torch.int32).to(dt)
    es = ref.element_size()
    torch.cuda.synchronize()
    with FeatureEngine(w, h, bit_depth=bpc, n_planes=1, features=N.FEAT_PSNR, result_capacity=max(16384, n)) as eng:
        eng.submit_resident(0, n, [ref.data_ptr()], [dis.data_ptr()], [w * es], [w * h * es])
        eng.sync()
        best = None
        for _ in range(a.rounds):
            eng.reset()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            eng.submit_resident(0, n, [ref.data_ptr()], [dis.data_ptr()], [w * es], [w * h * es])
            eng.sync()
            t1.record()
            torch.cuda.synchronize()
            us = t0.elapsed_time(t1) * 1e3 / n
            best = us if best is None else min(best, us)
    return best


lines = []
psnr_cache = {}
for sw, sh, dw, dh, bpc, filt in ((960, 540, 1920, 1080, 8, "bicubic"), (960, 540, 1920, 1080, 8, "lanczos"),
                                  (1920, 1080, 3840, 2160, 8, "bicubic"), (1920, 1080, 3840, 2160, 8, "lanczos"),
                                  (3840, 2160, 1920, 1080, 8, "bicubic"), (960, 540, 1920, 1080, 10, "bicubic"),
                                  (960, 540, 1920, 1080, 10, "lanczos")):
    key = (dw, dh, bpc)
    if key not in psnr_cache:
        psnr_cache[key] = psnr_luma(dw, dh, bpc, a.frames)
    psnr = psnr_cache[key]
    t = resample(sw, sh, dw, dh, bpc, filt, a.frames)
    floor = (sw * sh + dw * dh) * (1 if bpc == 8 else 2) / HBM_BYTES_PER_US
    lines.append(f"{sw}x{sh} -> {dw}x{dh} {bpc:2d}-bit {filt:8s} ({a.frames} planes): {t:8.2f} us/plane (best of {a.rounds}); luma PSNR at "
                 f"{dw}x{dh} {psnr:6.2f} us/frame, ratio {t / psnr:6.2f}; traffic floor {floor:6.2f} us, ratio {t / floor:7.2f}")
    print(lines[-1], flush=True)
    torch.cuda.empty_cache()

# ---- end to end: score_files(resize=) against a pre-scaled file ------------------------------------------------------------
from pqa2_amd import synth
from pqa2_amd.pipeline import score_files
from pqa2_amd.yuvio import VideoInfo, write_y4m

n = a.e2e_frames
refs, _ = synth.make_clip(1920, 1080, n, 8, chroma=True)
_, small = synth.make_clip(960, 540, n, 8, chroma=True)
with tempfile.TemporaryDirectory() as tmp:
    info = VideoInfo(width=1920, height=1080, fps_num=24, fps_den=1, bit_depth=8, mono=False, hshift=1, vshift=1, chroma_tag="420")
    small_info = VideoInfo(width=960, height=540, fps_num=24, fps_den=1, bit_depth=8, mono=False, hshift=1, vshift=1, chroma_tag="420")
    with FeatureEngine(1920, 1080, features=N.FEAT_PSNR, max_batch=8, result_capacity=16) as eng:
        full = [[eng.resample([p], shape, "bicubic")[0] for p, shape in zip(f, [(1080, 1920), (540, 960), (540, 960)])] for f in small]
    paths = {k: os.path.join(tmp, k + ".y4m") for k in ("ref", "small", "full")}
    write_y4m(paths["ref"], refs, info)
    write_y4m(paths["small"], small, small_info)
    write_y4m(paths["full"], full, info)
    times = {}
    for key, kw in (("full", {}), ("small", {"resize": "bicubic"})):
        res = score_files(paths["ref"], paths[key], "vmaf_v0.6.1", **kw)   # warm-up
        best = None
        for _ in range(3):
            t0 = time.perf_counter()
            res = score_files(paths["ref"], paths[key], "vmaf_v0.6.1", **kw)
            dt_ = time.perf_counter() - t0
            best = dt_ if best is None else min(best, dt_)
        times[key] = (best, res["records"])
    assert np.array_equal(times["full"][1].view(np.uint64), times["small"][1].view(np.uint64))
    t_full, t_small = times["full"][0], times["small"][0]
    lines.append(f"end to end, {n} frames 4:2:0 8-bit, 960x540 against a 1920x1080 reference: score_files(resize=bicubic) {t_small * 1e3:8.1f} ms, "
                 f"score_files on the pre-scaled 1920x1080 file {t_full * 1e3:8.1f} ms (best of 3 after a warm-up run; same records), "
                 f"{(t_small - t_full) * 1e3 / n:6.2f} ms more per frame, ratio {t_small / t_full:5.2f}")
    print(lines[-1], flush=True)
if a.out:
    with open(a.out, "a") as f:
        f.write("".join(line + "\n" for line in lines))
