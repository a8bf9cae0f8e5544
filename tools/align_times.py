#!/usr/bin/env python3
"""Time per reference frame of the banded cross-frame SSE (pqa_cross_sse_device, K = 8: 17 offsets) at 2160p and 1080p,
8-bit, on a resident natural synthetic clip (synth_torch), on both of its paths -- the i8 MFMA kernel and the plain-VALU
kernel (PQA_XSSE_MFMA=0, read at pqa_create: set around the context's creation, same process) -- beside its yardstick: the
luma-only sse kernel (a PQA_FEAT_PSNR context with n_planes = 1, HIP events around a resident run) times 17, i.e. what 17
separate PSNR passes over the same frames cost.  PQA_LIB_PATH selects the library the yardstick is taken from (the PSNR
path of a build of the parent commit is the same code).  The cross-SSE calls are synchronous, so a host clock around the
call is the time (it ends in a stream synchronise and includes the copy of the matrix to the host); best of --rounds after
a warm-up call.  The two paths' matrices are compared as integers.
usage: python tools/align_times.py [--frames 64] [--rounds 5] [--k 8] [--out FILE]"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from pqa2_amd import _native as N, synth_torch
from pqa2_amd.engine import FeatureEngine

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=64)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--k", type=int, default=8)
ap.add_argument("--out", default=None, help="also append the result lines to this file")
a = ap.parse_args()


def cross(w, h, ref, dis, n, mfma):
    old = os.environ.get("PQA_XSSE_MFMA")
    os.environ["PQA_XSSE_MFMA"] = "1" if mfma else "0"
    try:
        eng = FeatureEngine(w, h, bit_depth=8, n_planes=1, features=N.FEAT_PSNR, max_batch=8, result_capacity=16)
    finally:
        if old is None:
            os.environ.pop("PQA_XSSE_MFMA", None)
        else:
            os.environ["PQA_XSSE_MFMA"] = old
    with eng:
        args = (ref.data_ptr(), w, w * h, n, dis.data_ptr(), w, w * h, n, -a.k, a.k)
        D = eng.cross_sse_resident(*args)   # warm-up: code objects, the buffers of first use
        best = None
        for _ in range(a.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.cross_sse_resident(*args)
            us = (time.perf_counter() - t0) * 1e6 / n
            best = us if best is None else min(best, us)
    return best, D


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
        sse = eng.collect(0, n)[:, N.REC_SSE].copy().view(np.uint64)
    return best, sse


lines = []
span = 2 * a.k + 1
for w, h in ((3840, 2160), (1920, 1080)):
    clip = synth_torch.make_clip_cuda(w, h, a.frames, 8, chroma=False)
    ref, dis = clip["ref"][0].contiguous(), clip["dis"][0].contiguous()
    torch.cuda.synchronize()
    psnr, sse = psnr_luma(w, h, ref, dis, a.frames)
    mfma, Dm = cross(w, h, ref, dis, a.frames, True)
    valu, Dv = cross(w, h, ref, dis, a.frames, False)
    assert np.array_equal(Dm, Dv) and np.array_equal(Dm[:, a.k], sse)   # both paths, and offset 0 is the sse kernel's sum
    lines.append(f"{w}x{h} 8-bit luma natural ({a.frames}+{a.frames} frames, K = {a.k}, best of {a.rounds}): cross-SSE MFMA "
                 f"{mfma:8.2f} us/ref frame, VALU {valu:8.2f} us/ref frame; luma PSNR {psnr:6.2f} us/frame x {span} = "
                 f"{psnr * span:8.2f}; ratio to {span} PSNR passes: MFMA {mfma / (psnr * span):5.2f}, VALU {valu / (psnr * span):5.2f}")
    print(lines[-1], flush=True)
    del clip, ref, dis
    torch.cuda.empty_cache()
if a.out:
    with open(a.out, "a") as f:
        f.write("".join(line + "\n" for line in lines))
