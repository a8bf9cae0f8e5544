#!/usr/bin/env python3
"""Time per frame pair of the shifted-window luma SSE (pqa_shift_sse_device, R = 8: 289 shifts) at 2160p and 1080p on 8
resident 8-bit luma pairs of a natural synthetic clip (synth_torch), and once on the same pictures as 10-bit samples (the
plain-VALU path), beside its yardstick: the luma-only sse kernel (a PQA_FEAT_PSNR context with n_planes = 1, HIP events
around a resident run) times (2R + 1)^2, i.e. what one PSNR pass per shift over the same frames costs.  PQA_LIB_PATH selects
the library the yardstick is taken from (the PSNR path of a build of the parent commit is the same code).  The shift-SSE
call is synchronous, so a host clock around the call is the time (it ends in a stream synchronise and includes the copy of
the result to the host); best of --rounds after a warm-up call.  The centre entry is compared with the sse kernel's sum of
the same pair cropped to the window.
usage: python tools/shift_times.py [--frames 8] [--rounds 5] [--radius 8] [--out FILE]"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from pqa2_amd import _native as N, synth_torch
from pqa2_amd.engine import FeatureEngine

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=8)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--radius", type=int, default=8)
ap.add_argument("--out", default=None, help="also append the result lines to this file")
a = ap.parse_args()
R = a.radius


def shift(w, h, bpc, ref, dis, n, rounds):
    es = ref.element_size()
    with FeatureEngine(w, h, bit_depth=bpc, n_planes=1, features=N.FEAT_PSNR, max_batch=8, result_capacity=16) as eng:
        args = (ref.data_ptr(), w * es, w * h * es, dis.data_ptr(), w * es, w * h * es, n, R)
        S = eng.shift_sse_resident(*args)   # warm-up: code objects, the buffers of first use
        best = None
        for _ in range(rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.shift_sse_resident(*args)
            us = (time.perf_counter() - t0) * 1e6 / n
            best = us if best is None else min(best, us)
    return best, S


def psnr_luma(w, h, ref, dis, n):
    with FeatureEngine(w, h, bit_depth=8, n_planes=1, features=N.FEAT_PSNR, result_capacity=max(16384, n)) as eng:
        eng.submit_resident(0, n, [ref.data_ptr()], [dis.data_ptr()], [w], [w * h])
        eng.sync()
        best = None
        for _ in range(a.rounds):
            eng.reset()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            eng.submit_resident(0, n, [ref.data_ptr()], [dis.data_ptr()], [w], [w * h])
            eng.sync()
            t1.record()
            torch.cuda.synchronize()
            us = t0.elapsed_time(t1) * 1e3 / n
            best = us if best is None else min(best, us)
    return best


def window_sse(ref, dis):
    r, d = ref[:, R:-R, R:-R].to(torch.int64), dis[:, R:-R, R:-R].to(torch.int64)
    return ((r - d) ** 2).sum(dim=(1, 2)).cpu().numpy().astype(np.uint64)


lines = []
n_shifts = (2 * R + 1) ** 2
for w, h in ((3840, 2160), (1920, 1080)):
    clip = synth_torch.make_clip_cuda(w, h, a.frames, 8, chroma=False)
    ref, dis = clip["ref"][0].contiguous(), clip["dis"][0].contiguous()
    torch.cuda.synchronize()
    psnr = psnr_luma(w, h, ref, dis, a.frames)
    t8, S8 = shift(w, h, 8, ref, dis, a.frames, a.rounds)
    assert np.array_equal(S8[:, R, R], window_sse(ref, dis))   # the zero shift is the plain squared error of the window
    ref10, dis10 = (ref.to(torch.int16) * 4 + 1).contiguous(), (dis.to(torch.int16) * 4 + 2).contiguous()
    t10, S10 = shift(w, h, 10, ref10, dis10, a.frames, 1)
    assert np.array_equal(S10[:, R, R], window_sse(ref10, dis10))
    lines.append(f"{w}x{h} luma natural ({a.frames} pairs, R = {R}: {n_shifts} shifts): shift-SSE 8-bit {t8:8.2f} us/pair (best of "
                 f"{a.rounds}), 10-bit {t10:8.2f} us/pair (once); luma PSNR {psnr:6.2f} us/frame x {n_shifts} = "
                 f"{psnr * n_shifts:8.2f}; ratio to {n_shifts} PSNR passes: 8-bit {t8 / (psnr * n_shifts):6.3f}, 10-bit "
                 f"{t10 / (psnr * n_shifts):6.3f}")
    print(lines[-1], flush=True)
    del clip, ref, dis, ref10, dis10
    torch.cuda.empty_cache()
if a.out:
    with open(a.out, "a") as f:
        f.write("".join(line + "\n" for line in lines))
