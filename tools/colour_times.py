#!/usr/bin/env python3
"""Time per frame (pair) of the colour-matrix kernels on 8 resident 4:2:0 frames of uniform noise at 1920x1080 and 3840x2160, 8 and
10 bit: the cross-plane moments (pqa_colour_moments_device, keep-all mask) and the matrix apply (pqa_colour_apply_device),
beside two yardsticks taken in the same run: one three-plane PSNR pass (the sse kernels of the same build, HIP events around a
resident run, as tools/flow_times.py takes its luma pass) and the traffic floor -- the bytes each kernel must move (moments:
three planes of both clips read once; apply: three planes read and written once) / 8 TB/s.  Both calls are synchronous (one
kernel launch for the 8 frames, ending in a stream synchronise), so a host clock around the call is the time; best of --rounds
after a warm-up call.  The last pair's sums and the last applied frame are checked against the numpy restatement.
usage: python tools/colour_times.py [--frames 8] [--rounds 5] [--out FILE]"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from pqa2_amd import _native as N
from pqa2_amd import align as AL
from pqa2_amd.engine import FeatureEngine
from tests import colour_ref as R

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=8)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=None, help="also append the result lines to this file")
a = ap.parse_args()
HBM_BYTES_PER_US = 8.0e6   # 8 TB/s


def clip(w, h, bpc, n, seed):
    """[Y, U, V] tensors [n, h, w] / [n, h/2, w/2] of uniform noise, their pointers and byte pitches"""
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    dt = torch.uint8 if bpc == 8 else torch.int16
    t = [torch.randint(0, 1 << bpc, (n, ph, pw), generator=gen, device="cuda", dtype=torch.int32).to(dt)
         for ph, pw in ((h, w), (h // 2, w // 2), (h // 2, w // 2))]
    es = t[0].element_size()
    return t, [p.data_ptr() for p in t], [p.shape[2] * es for p in t], [p.shape[1] * p.shape[2] * es for p in t]


def host(t, f, bpc):
    return [p[f].cpu().numpy().view(np.uint8 if bpc == 8 else np.uint16) for p in t]


def best_of(call, n):
    call()   # warm-up: code objects, the buffers of first use
    best = None
    for _ in range(a.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = call()
        us = (time.perf_counter() - t0) * 1e6 / n
        best = us if best is None else min(best, us)
    return best, got


def colour(w, h, bpc, n):
    top = (1 << bpc) - 1
    (rt, rp, row, frame), (dt, dp, _, _) = clip(w, h, bpc, n, 99), clip(w, h, bpc, n, 7)
    ot, op, _, _ = clip(w, h, bpc, n, 5)
    m = [int(v) for v in AL.colour_correction({"kind": "bt709_to_bt601"}, bpc)]
    torch.cuda.synchronize()
    with FeatureEngine(w, h, bit_depth=bpc, n_planes=3, features=N.FEAT_PSNR, max_batch=8, result_capacity=16) as eng:
        t_mom, got = best_of(lambda: eng.colour_moments_resident(rp, dp, row, frame, n, 0, top), n)
        t_app, _ = best_of(lambda: eng.colour_apply_resident(m, dp, op, row, frame, n), n)
    assert np.array_equal(got[n - 1], R.colour_moments([host(rt, n - 1, bpc)], [host(dt, n - 1, bpc)], bpc, 1, 1, 0, top)[0])
    want = R.apply(host(dt, n - 1, bpc), m, bpc, 1, 1)
    assert all(np.array_equal(x, y) for x, y in zip(host(ot, n - 1, bpc), want))
    return t_mom, t_app


def psnr_three_planes(w, h, bpc, n):
    (_, rp, row, frame), (_, dp, _, _) = clip(w, h, bpc, n, 7), clip(w, h, bpc, n, 8)
    torch.cuda.synchronize()
    with FeatureEngine(w, h, bit_depth=bpc, n_planes=3, features=N.FEAT_PSNR, result_capacity=max(16384, n)) as eng:
        eng.submit_resident(0, n, rp, dp, row, frame)
        eng.sync()
        best = None
        for _ in range(a.rounds):
            eng.reset()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            eng.submit_resident(0, n, rp, dp, row, frame)
            eng.sync()
            t1.record()
            torch.cuda.synchronize()
            us = t0.elapsed_time(t1) * 1e3 / n
            best = us if best is None else min(best, us)
    return best


lines = []
for w, h in ((1920, 1080), (3840, 2160)):
    for bpc in (8, 10):
        psnr = psnr_three_planes(w, h, bpc, a.frames)
        frame_bytes = (w * h + 2 * (w // 2) * (h // 2)) * (1 if bpc == 8 else 2)
        floor = 2 * frame_bytes / HBM_BYTES_PER_US       # moments: two clips read; apply: one read, one written
        t_mom, t_app = colour(w, h, bpc, a.frames)
        for name, t in (("moments", t_mom), ("apply  ", t_app)):
            lines.append(f"{w}x{h} {bpc:2d}-bit 4:2:0 {name} ({a.frames} frames): {t:8.2f} us/frame (best of {a.rounds}); three-plane PSNR "
                         f"{psnr:6.2f} us/frame, ratio {t / psnr:6.2f}; traffic floor {floor:6.2f} us, ratio {t / floor:7.2f}")
            print(lines[-1], flush=True)
        torch.cuda.empty_cache()
if a.out:
    with open(a.out, "a") as f:
        f.write("".join(line + "\n" for line in lines))
