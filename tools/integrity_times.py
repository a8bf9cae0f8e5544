#!/usr/bin/env python3
"""Time per frame of the capture-integrity kernel (PQA_FEAT_INTEGRITY alone) beside its yardstick, the sse kernel
(PQA_FEAT_PSNR alone), at 2160p and 1080p, 8-bit 4:2:0, n_planes 3, on a resident natural synthetic clip (synth_torch).
Both read two frames of every plane per frame and reduce to exact integers.  No profile id is free, so HIP events
(torch.cuda.Event) bracket whole runs, automatic batch, best of --rounds, both contexts in this one process.  Prints both
times, their ratio and the GB/s the integrity time implies (two frames of all planes per frame).
usage: python tools/integrity_times.py [--frames 48] [--rounds 3] [--batch 0] [--out FILE]"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from pqa2_amd import _native as N, synth_torch
from pqa2_amd.engine import FeatureEngine

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=48)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--batch", type=int, default=0)
ap.add_argument("--out", default=None, help="also append the result lines to this file")
a = ap.parse_args()


def run(w, h, feats, clip, n, rounds):
    ptr = lambda k: [t.data_ptr() for t in clip[k]]
    rp = [t.shape[2] for t in clip["ref"]]
    fp = [t.shape[1] * t.shape[2] for t in clip["ref"]]
    with FeatureEngine(w, h, bit_depth=8, n_planes=3, chroma_shift=(1, 1), features=feats, max_batch=a.batch,
                       result_capacity=max(16384, n)) as eng:
        eng.submit_resident(0, n, ptr("ref"), ptr("dis"), rp, fp)   # warm-up
        eng.sync()
        best = None
        for _ in range(rounds):
            eng.reset()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            eng.submit_resident(0, n, ptr("ref"), ptr("dis"), rp, fp)
            eng.sync()
            t1.record()
            torch.cuda.synchronize()
            us = t0.elapsed_time(t1) * 1e3 / n
            best = us if best is None else min(best, us)
        if feats & N.FEAT_INTEGRITY:     # the rows are what they should be: exact SADs of the resident frames
            ext5 = eng.collect_blocks(0, n, [4])[1][4]
            d = clip["dis"][0]
            want = (d[1:3].to(torch.int32) - d[0:2].to(torch.int32)).abs().sum(dim=(1, 2)).cpu().numpy()
            assert np.isnan(ext5[0, 0]) and (ext5[1:3, 0] == want).all() and (ext5[1:, :3] > 0).all()
    return best


lines = []
for w, h in ((3840, 2160), (1920, 1080)):
    clip = synth_torch.make_clip_cuda(w, h, a.frames, 8, chroma=True)
    clip = {k: [t.contiguous() for t in v] for k, v in clip.items()}
    torch.cuda.synchronize()
    psnr = run(w, h, N.FEAT_PSNR, clip, a.frames, a.rounds)
    integ = run(w, h, N.FEAT_INTEGRITY, clip, a.frames, a.rounds)
    gbs = 2 * (w * h * 3 // 2) / (integ * 1e-6) / 1e9
    lines.append(f"{w}x{h} 8-bit 4:2:0 natural ({a.frames} frames, best of {a.rounds}): psnr alone {psnr:7.2f} us/frame, "
                 f"integrity alone {integ:7.2f} us/frame, ratio {integ / psnr:5.2f}, {gbs:7.0f} GB/s")
    print(lines[-1], flush=True)
    del clip
    torch.cuda.empty_cache()
if a.out:
    with open(a.out, "a") as f:
        f.write("".join(line + "\n" for line in lines))
