#!/usr/bin/env python3
"""Time of cambi per frame at 2160p 8-bit, 1080p 8-bit and 2160p 10-bit on a resident clip.  No profile id is free for it,
so HIP events (torch.cuda.Event) bracket whole runs: VMAF alone and VMAF + PQA_FEAT_CAMBI (and + FULL_REF), best of
--rounds; the difference per frame is cambi's cost.  Two contents: a dark dithered staircase (every sample masked and
inside the histogram range: the c-value kernel's worst case) and the natural synthetic clip (synth_torch).
usage: python tools/cambi_times.py [--frames 48] [--rounds 3] [--batch 0]"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from pqa2_amd import _native as N, synth_torch
from pqa2_amd.engine import FeatureEngine

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=48)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--batch", type=int, default=0)
a = ap.parse_args()


def staircase(w, h, n, bits):
    g = torch.Generator(device="cuda").manual_seed(1)
    step = 1 if bits == 8 else 2
    lo = 16 if bits == 8 else 64
    x = torch.arange(w, device="cuda", dtype=torch.float32)[None, :]
    y = torch.arange(h, device="cuda", dtype=torch.float32)[:, None]
    out = []
    for f in range(n):
        t = (x + 0.37 * y + 7 * f) / (w + 0.37 * h)
        v = lo + torch.floor(t * 12) * step
        v = v + (torch.rand((h, w), device="cuda", generator=g) < 0.02).float()
        out.append(v)
    dt = torch.uint8 if bits == 8 else torch.int16
    return torch.stack(out).to(dt).contiguous()


def timed(w, h, bits, feats, R, D, n):
    es = 1 if bits <= 8 else 2
    with FeatureEngine(w, h, bit_depth=bits, n_planes=1, features=feats, max_batch=a.batch,
                       result_capacity=max(16384, n)) as eng:
        args = ([R.data_ptr()], [D.data_ptr()], [w * es], [w * h * es])
        eng.submit_resident(0, n, *args)   # warm-up
        eng.sync()
        best = None
        for _ in range(a.rounds):
            eng.reset()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            eng.submit_resident(0, n, *args)
            eng.sync()
            t1.record()
            torch.cuda.synchronize()
            us = t0.elapsed_time(t1) * 1e3 / n
            best = us if best is None else min(best, us)
    return best


for w, h, bits in ((3840, 2160, 8), (1920, 1080, 8), (3840, 2160, 10)):
    for content in ("staircase", "natural"):
        if content == "staircase":
            R, D = staircase(w, h, a.frames, bits), staircase(w, h, a.frames, bits).flip(2).contiguous()
        else:
            clip = synth_torch.make_clip_cuda(w, h, a.frames, bits, chroma=False)
            R, D = clip["ref"][0].contiguous(), clip["dis"][0].contiguous()
        torch.cuda.synchronize()
        base = timed(w, h, bits, N.FEAT_VMAF, R, D, a.frames)
        one = timed(w, h, bits, N.FEAT_VMAF | N.FEAT_CAMBI, R, D, a.frames)
        full = timed(w, h, bits, N.FEAT_VMAF | N.FEAT_CAMBI | N.FEAT_CAMBI_FULL_REF, R, D, a.frames)
        print(f"{w}x{h} {bits}-bit {content:9s} ({a.frames} frames, best of {a.rounds}): vmaf {base:8.1f} us/frame, "
              f"+cambi {one - base:8.1f} us/frame, +cambi full-ref {full - base:8.1f} us/frame", flush=True)
        del R, D
        torch.cuda.empty_cache()
