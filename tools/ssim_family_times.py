#!/usr/bin/env python3
"""Kernel time of the SSIM family per frame, from the library's own event timing (pqa_profile_*): profile id 15 (ms_ssim:
all five scales, their decimations and the extension epilogue) and 16 (float_ssim), at 2160p 8-bit, 1080p 8-bit and
2160p 10-bit.  Only those two ids are timed (a subset mask: no events between the other kernels); the clip is resident.
usage: python tools/ssim_family_times.py [--frames 96] [--rounds 3] [--batch 0]"""
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
    clip = synth_torch.make_clip_cuda(w, h, a.frames, bits)
    R, D = clip["ref"][0], clip["dis"][0]
    torch.cuda.synchronize()
    es = 1 if bits <= 8 else 2
    with FeatureEngine(w, h, bit_depth=bits, features=N.FEAT_FLOAT_SSIM | N.FEAT_MS_SSIM, max_batch=a.batch,
                       result_capacity=max(16384, a.frames)) as eng:
        eng.submit_resident(0, a.frames, [R.data_ptr()], [D.data_ptr()], [w * es], [w * h * es])   # warm-up
        eng.sync()
        best = {}
        for _ in range(a.rounds):
            eng.reset()
            eng.profile_enable([15, 16])
            eng.submit_resident(0, a.frames, [R.data_ptr()], [D.data_ptr()], [w * es], [w * h * es])
            eng.sync()
            prof = eng.profile_read()
            for k in ("ms_ssim", "float_ssim"):
                us = prof[k]["ms"] * 1e3 / max(1, prof[k]["frames"])
                best[k] = min(best.get(k, us), us)
        print(f"{w}x{h} {bits}-bit ({a.frames} frames, best of {a.rounds}): ms_ssim {best['ms_ssim']:8.1f} us/frame   "
              f"float_ssim {best['float_ssim']:7.1f} us/frame", flush=True)
    del clip, R, D
    torch.cuda.empty_cache()
