#!/usr/bin/env python3
"""Time of siti (SI / TI of both clips) per frame at 2160p and 1080p, 8-bit 4:2:0, on a resident natural synthetic clip
(synth_torch).  No profile id is free for it, so HIP events (torch.cuda.Event) bracket whole runs: VMAF alone and VMAF +
PQA_FEAT_SITI, best of --rounds; the difference per frame is siti's cost.  --only times PQA_FEAT_SITI alone (best of
--rounds; what a `rocprofv3 --kernel-trace --stats -- python tools/siti_times.py --only` run traces).
usage: python tools/siti_times.py [--frames 48] [--rounds 3] [--batch 0] [--only]"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from pqa2_amd import _native as N, synth_torch
from pqa2_amd.engine import FeatureEngine

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=48)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--batch", type=int, default=0)
ap.add_argument("--only", action="store_true", help="PQA_FEAT_SITI alone per size")
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
        if feats & N.FEAT_SITI:
            ext4 = eng.collect_blocks(0, n, [3])[1][3]
            assert (ext4[:, 0] > 0).all() and (ext4[1:, 1] > 0).all() and torch.isfinite(torch.from_numpy(ext4[:, :4])).all()
    return best


for w, h in ((3840, 2160), (1920, 1080)):
    clip = synth_torch.make_clip_cuda(w, h, a.frames, 8, chroma=True)
    clip = {k: [t.contiguous() for t in v] for k, v in clip.items()}
    torch.cuda.synchronize()
    if a.only:
        us = run(w, h, N.FEAT_SITI, clip, a.frames, a.rounds)
        print(f"{w}x{h} 8-bit 4:2:0 natural ({a.frames} frames, best of {a.rounds}): siti alone {us:8.1f} us/frame",
              flush=True)
    else:
        base = run(w, h, N.FEAT_VMAF, clip, a.frames, a.rounds)
        both = run(w, h, N.FEAT_VMAF | N.FEAT_SITI, clip, a.frames, a.rounds)
        print(f"{w}x{h} 8-bit 4:2:0 natural ({a.frames} frames, best of {a.rounds}): vmaf {base:8.1f} us/frame, "
              f"+siti {both - base:8.1f} us/frame", flush=True)
    del clip
    torch.cuda.empty_cache()
