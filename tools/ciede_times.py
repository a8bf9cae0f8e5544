#!/usr/bin/env python3
"""Kernel time of ciede2000 per frame, from the library's own event timing (pqa_profile_*): profile id 4 (the CIEDE2000
kernel and its epilogue) at 2160p 8-bit, 1080p 8-bit and 2160p 10-bit, all 4:2:0.  Only that id is timed (a subset mask:
no events between the other kernels); the clip is resident.
usage: python tools/ciede_times.py [--frames 96] [--rounds 3] [--batch 0]"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from pqa2_amd import _native as N, synth_torch
from pqa2_amd.engine import FeatureEngine

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=96)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--batch", type=int, default=0)
a = ap.parse_args()
for w, h, bits in ((3840, 2160, 8), (1920, 1080, 8), (3840, 2160, 10)):
    clip = synth_torch.make_clip_cuda(w, h, a.frames, bits, chroma=True)
    R, D = clip["ref"], clip["dis"]
    torch.cuda.synchronize()
    es = 1 if bits <= 8 else 2
    rp = [t.shape[2] * es for t in R]
    fp = [t.shape[1] * t.shape[2] * es for t in R]
    with FeatureEngine(w, h, bit_depth=bits, n_planes=3, features=N.FEAT_CIEDE, max_batch=a.batch,
                       result_capacity=max(16384, a.frames)) as eng:
        args = ([t.data_ptr() for t in R], [t.data_ptr() for t in D], rp, fp)
        eng.submit_resident(0, a.frames, *args)   # warm-up
        eng.sync()
        best = None
        for _ in range(a.rounds):
            eng.reset()
            eng.profile_enable([4])
            eng.submit_resident(0, a.frames, *args)
            eng.sync()
            prof = eng.profile_read()["ciede2000"]
            us = prof["ms"] * 1e3 / max(1, prof["frames"])
            best = us if best is None else min(best, us)
        print(f"{w}x{h} {bits}-bit 4:2:0 ({a.frames} frames, best of {a.rounds}): ciede2000 {best:8.1f} us/frame", flush=True)
    del clip, R, D
    torch.cuda.empty_cache()
