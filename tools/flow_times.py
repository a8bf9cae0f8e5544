#!/usr/bin/env python3
"""Time per frame pair of the registration moments (pqa_flow_moments_device) on 8 resident luma pairs of uniform noise at
1920x1080 and 3840x2160, 8 and 10 bit, tiles 8 and 32, beside two yardsticks taken in the same run: one luma PSNR pass (the
luma-only sse kernel of the same build, HIP events around a resident run, as tools/resample_times.py takes it) and the traffic
floor (both planes read once) / 8 TB/s.  The call is synchronous (one kernel launch for the 8 pairs, ends in a stream
synchronise and a small copy), so a host clock around the call is the time; best of --rounds after a warm-up call.  The bottom
right corner of the last pair is checked against the numpy restatement.
usage: python tools/flow_times.py [--frames 8] [--rounds 5] [--out FILE]"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from pqa2_amd import _native as N
from pqa2_amd.engine import FeatureEngine
from tests import flow_ref as F

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=8)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=None, help="also append the result lines to this file")
a = ap.parse_args()
HBM_BYTES_PER_US = 8.0e6   # 8 TB/s


def planes(w, h, bpc, n, seed):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    return torch.randint(0, 1 << bpc, (n, h, w), generator=gen, device="cuda", dtype=torch.int32).to(torch.uint8 if bpc == 8 else torch.int16)


def flow(w, h, bpc, tile, n):
    ref, dis = planes(w, h, bpc, n, 99), planes(w, h, bpc, n, 7)
    es = ref.element_size()
    torch.cuda.synchronize()
    with FeatureEngine(w, h, bit_depth=bpc, n_planes=1, features=N.FEAT_PSNR, max_batch=8, result_capacity=16) as eng:
        args = (ref.data_ptr(), w * es, w * h * es, dis.data_ptr(), w * es, w * h * es, (h, w), n, tile)
        got = eng.flow_moments_resident(*args)   # warm-up: code objects, the buffers of first use
        best = None
        for _ in range(a.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = eng.flow_moments_resident(*args)
            us = (time.perf_counter() - t0) * 1e6 / n
            best = us if best is None else min(best, us)
    # the last two tile rows and columns of the last pair, from the samples they read (the crop starts on a tile boundary)
    np_dt = np.uint8 if bpc == 8 else np.uint16
    ty, tx = got.shape[1:3]
    y0, x0 = (ty - 2) * tile, (tx - 2) * tile
    r = ref[n - 1].cpu().numpy().view(np_dt)[y0 - 1:, x0 - 1:]
    d = dis[n - 1].cpu().numpy().view(np_dt)[y0 - 1:, x0 - 1:]
    gx, gy, dt = F._fields(r, d, bpc)      # entry (0, 0) belongs to pixel (x0, y0)
    want = np.zeros((2, 2, 6), np.int64)
    hh, ww = gx.shape
    for m, prod in enumerate((gx * gx, gx * gy, gy * gy, gx * dt, gy * dt, dt * dt)):
        for j in range(2):
            for i in range(2):
                want[j, i, m] = prod[j * tile:min((j + 1) * tile, hh), i * tile:min((i + 1) * tile, ww)].sum()
    assert np.array_equal(got[n - 1, ty - 2:, tx - 2:], want)
    return best


def psnr_luma(w, h, bpc, n):
    ref, dis = planes(w, h, bpc, n, 7), planes(w, h, bpc, n, 8)
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
for w, h in ((1920, 1080), (3840, 2160)):
    for bpc in (8, 10):
        psnr = psnr_luma(w, h, bpc, a.frames)
        floor = 2 * w * h * (1 if bpc == 8 else 2) / HBM_BYTES_PER_US
        for tile in (8, 32):
            t = flow(w, h, bpc, tile, a.frames)
            lines.append(f"{w}x{h} {bpc:2d}-bit tile {tile:2d} ({a.frames} pairs): {t:8.2f} us/pair (best of {a.rounds}); luma PSNR "
                         f"{psnr:6.2f} us/frame, ratio {t / psnr:6.2f}; traffic floor {floor:6.2f} us, ratio {t / floor:7.2f}")
            print(lines[-1], flush=True)
        torch.cuda.empty_cache()
if a.out:
    with open(a.out, "a") as f:
        f.write("".join(line + "\n" for line in lines))
