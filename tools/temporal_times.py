#!/usr/bin/env python3
"""Time per luma transition of the temporal moments (pqa_temporal_moments_device) at 1080p and 2160p, 8 and 10 bit, T = 64, on 8
resident pairs of uniform noise (7 transitions a call), in both forms of the kernel -- a workgroup per transition (the
default: four planes read a transition) and a workgroup that walks through time with the previous pair in registers
(PQA_TEMPORAL_WALK=1, read at pqa_create: set around the context's creation, same process; two planes a transition) --
beside three yardsticks on the same planes in the same process: the tile moments at T = 64 (pqa_tile_moments_device: two
planes a pair, six sums a tile), one luma PSNR pass of the engine (a FEAT_PSNR context) and the traffic floor at 8 TB/s, two
planes a transition if the previous pair is kept and four if not.  Every call ends in a stream synchronise, so a host clock
around the call is the time; minimum, median and maximum of --rounds after a warm-up call.  Every result is checked: the
tiles of the last transition add up to torch's sums of the whole plane, and the two forms return the same words.
usage: python tools/temporal_times.py [--frames 8] [--rounds 9] [--out FILE]"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from pqa2_amd import _native as N
from pqa2_amd.engine import FeatureEngine

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=8)
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--out", default=None, help="also append the result lines to this file")
a = ap.parse_args()

HBM_BYTES_PER_US = 8e6   # 8 TB/s


def planes(w, h, bpc, n, seed):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    return torch.randint(0, 1 << bpc, (n, h, w), generator=gen, device="cuda", dtype=torch.int32).to(torch.uint8 if bpc == 8 else torch.int16)


def timed(call, n):
    """(min, median, max) us per unit (n units a call) of --rounds calls after a warm-up, and the last result"""
    got = call()   # warm-up: code objects, the buffers of first use
    us = []
    for _ in range(a.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = call()
        us.append((time.perf_counter() - t0) * 1e6 / n)
    us.sort()
    return (us[0], us[len(us) // 2], us[-1]), got


def engine(w, h, bpc, walk=False):
    old = os.environ.get("PQA_TEMPORAL_WALK")
    os.environ["PQA_TEMPORAL_WALK"] = "1" if walk else "0"
    try:
        return FeatureEngine(w, h, bit_depth=bpc, n_planes=1, features=N.FEAT_PSNR, max_batch=8, result_capacity=16)
    finally:
        if old is None:
            os.environ.pop("PQA_TEMPORAL_WALK", None)
        else:
            os.environ["PQA_TEMPORAL_WALK"] = old


def temporal(ref, dis, w, h, bpc, n, walk):
    es = ref.element_size()
    with engine(w, h, bpc, walk) as eng:
        args = (ref.data_ptr(), w * es, w * h * es, dis.data_ptr(), w * es, w * h * es, (h, w), n, 64)
        t, got = timed(lambda: eng.temporal_moments_resident(*args), n - 1)
    rk, rp, dk, dp = (x.to(torch.int64) for x in (ref[n - 1], ref[n - 2], dis[n - 1], dis[n - 2]))
    x, y, e = rk - rp, dk - dp, dk - rk
    want = [int(v.sum()) for v in (x, y, x * x, y * y, x * y, x * e, e * e)]
    assert [int(v) for v in got[n - 2].view(np.int64).sum(axis=(0, 1))] == want
    return t, got


def tiles(ref, dis, w, h, bpc, n):
    es = ref.element_size()
    with engine(w, h, bpc) as eng:
        args = (ref.data_ptr(), w * es, w * h * es, dis.data_ptr(), w * es, w * h * es, (h, w), n, 64)
        return timed(lambda: eng.tile_moments_resident(*args), n)[0]


def psnr_luma(ref, dis, w, h, bpc, n):
    es = ref.element_size()
    with FeatureEngine(w, h, bit_depth=bpc, n_planes=1, features=N.FEAT_PSNR, result_capacity=max(16384, n)) as eng:
        def call():
            eng.reset()
            eng.submit_resident(0, n, [ref.data_ptr()], [dis.data_ptr()], [w * es], [w * h * es])
            eng.sync()
        t, _ = timed(call, n)
    return t


lines = []
for w, h in ((1920, 1080), (3840, 2160)):
    for bpc in (8, 10):
        ref, dis = planes(w, h, bpc, a.frames, 99), planes(w, h, bpc, a.frames, 7)
        torch.cuda.synchronize()
        psnr = psnr_luma(ref, dis, w, h, bpc, a.frames)
        tile = tiles(ref, dis, w, h, bpc, a.frames)
        plane_us = w * h * (1 if bpc == 8 else 2) / HBM_BYTES_PER_US
        words = None
        for walk in (False, True):
            t, got = temporal(ref, dis, w, h, bpc, a.frames, walk)
            assert words is None or np.array_equal(words, got)
            words = got
            floor = (2 if walk else 4) * plane_us
            lines.append(f"{w}x{h} {bpc:2d}-bit T 64 {'walking     ' if walk else 'z-transition'} ({a.frames} pairs): {t[0]:7.2f} / {t[1]:7.2f} / "
                         f"{t[2]:7.2f} us/transition (min / median / max of {a.rounds}); tile moments T 64 {tile[0]:6.2f} / {tile[1]:6.2f} / "
                         f"{tile[2]:6.2f} us/pair, ratio of minima {t[0] / tile[0]:5.2f}; luma PSNR {psnr[0]:6.2f} / {psnr[1]:6.2f} / "
                         f"{psnr[2]:6.2f} us/frame, ratio of minima {t[0] / psnr[0]:5.2f}; {4 if not walk else 2} planes once at 8 TB/s "
                         f"{floor:5.2f} us, ratio {t[0] / floor:6.2f}")
            print(lines[-1], flush=True)
        del ref, dis
        torch.cuda.empty_cache()
if a.out:
    with open(a.out, "a") as f:
        f.write("".join(line + "\n" for line in lines))
