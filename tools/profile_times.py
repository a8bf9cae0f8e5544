#!/usr/bin/env python3
"""Time per luma plane of the line profiles (pqa_line_profiles_device) at 2160p and 1080p, 8 and 10 bit, on 8 resident planes
of two contents: uniform noise, and the same noise inside black bars (a 2.39:1 letterbox: the bar rows add nothing to the
column table); beside its yardstick, pqa_luma_stats_device on the same planes, which reads the same bytes once and returns
three sums a frame, and beside the traffic floor of one read of the plane at 8 TB/s.  Both calls are synchronous, so a host
clock around the call is the time (each ends in a stream synchronise and includes the clearing and the copy of its result
to the host); best of --rounds after a warm-up call.  Every profile is checked: rows and columns each add up to the sums
pqa_luma_stats_device returns for the frame, and to torch's.
usage: python tools/profile_times.py [--frames 8] [--rounds 5] [--out FILE]"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from pqa2_amd import _native as N
from pqa2_amd.engine import FeatureEngine

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=8)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=None, help="also append the result lines to this file")
a = ap.parse_args()

FLOOR_BYTES_PER_US = 8e6   # 8 TB/s


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


def measure(w, h, bpc, clip, n):
    es = clip.element_size()
    with FeatureEngine(w, h, bit_depth=bpc, n_planes=1, features=N.FEAT_PSNR, max_batch=8, result_capacity=16) as eng:
        t_prof, (rows, cols) = best_of(lambda: eng.line_profiles_resident(clip.data_ptr(), w * es, w * h * es, (h, w), n), n)
        t_luma, stats = best_of(lambda: eng.luma_stats_resident(clip.data_ptr(), w * es, w * h * es, n, 0), n)
    v = clip.to(torch.int64)
    want = np.stack([v.sum(dim=(1, 2)).cpu().numpy(), (v * v).sum(dim=(1, 2)).cpu().numpy()], axis=1).astype(np.uint64)
    assert np.array_equal(rows.sum(axis=1), want) and np.array_equal(cols.sum(axis=1), want) and np.array_equal(stats[:, :2], want)
    assert np.array_equal(cols[:, :, 0], v.sum(dim=1).cpu().numpy().astype(np.uint64))
    return t_prof, t_luma


lines = []
for w, h in ((3840, 2160), (1920, 1080)):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1234)
    for bpc in (8, 10):
        dt = torch.uint8 if bpc == 8 else torch.int16
        noise = torch.randint(0, 1 << bpc, (a.frames, h, w), generator=gen, device="cuda", dtype=torch.int32).to(dt)
        boxed = noise.clone()
        bar = (h - int(round(w / 2.39))) // 2
        boxed[:, :bar], boxed[:, h - bar:] = 0, 0
        torch.cuda.synchronize()
        floor = w * h * noise.element_size() / FLOOR_BYTES_PER_US
        p_noise, l_noise = measure(w, h, bpc, noise, a.frames)
        p_boxed, l_boxed = measure(w, h, bpc, boxed, a.frames)
        lines.append(f"{w}x{h} luma {bpc:2d}-bit ({a.frames} planes): line profiles noise {p_noise:8.2f}, letterboxed {p_boxed:8.2f} "
                     f"us/plane (best of {a.rounds}); pqa_luma_stats_device {l_noise:8.2f} / {l_boxed:8.2f} us/plane; ratio "
                     f"{p_noise / l_noise:5.2f} / {p_boxed / l_boxed:5.2f}; one read at 8 TB/s {floor:6.2f} us")
        print(lines[-1], flush=True)
        del noise, boxed
    torch.cuda.empty_cache()
if a.out:
    with open(a.out, "a") as f:
        f.write("".join(line + "\n" for line in lines))
