#!/usr/bin/env python3
"""Time per luma pair of the band moments (pqa_band_moments_device) at 1080p and 2160p, 8 and 10 bit, 4 and 6 levels, on 8
resident pairs of uniform noise; beside three yardsticks on the same planes: the tile moments at T = 64
(pqa_tile_moments_device: the same two reads, six sums a tile), one luma PSNR pass of the engine (a FEAT_PSNR context: the
same two reads with one sum), and one read of both planes at 8 TB/s.  Every call ends in a stream synchronise, so a host
clock around the call is the time; minimum, median and maximum of --rounds after a warm-up call.  Every result is checked:
the band moments of the last pair against torch's own Haar transform of the planes.
usage: python tools/band_times.py [--frames 8] [--rounds 9] [--out FILE]"""
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
    """(min, median, max) us per pair of --rounds calls after a warm-up, and the last result"""
    got = call()   # warm-up: code objects, the buffers of first use
    us = []
    for _ in range(a.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = call()
        us.append((time.perf_counter() - t0) * 1e6 / n)
    us.sort()
    return (us[0], us[len(us) // 2], us[-1]), got


def haar_sums(r, d, levels):
    """[L][4][3] Python ints of one pair of int64 planes on the device"""
    out = []
    for _ in range(levels):
        co = []
        for x in (r, d):
            h2, w2 = x.shape[0] // 2, x.shape[1] // 2
            p, q, s, t = x[0:2 * h2:2, 0:2 * w2:2], x[0:2 * h2:2, 1:2 * w2:2], x[1:2 * h2:2, 0:2 * w2:2], x[1:2 * h2:2, 1:2 * w2:2]
            co.append((p - q + s - t, p + q - s - t, p - q - s + t, p + q + s + t))
        out.append([[int((co[0][o] * co[0][o]).sum()), int((co[1][o] * co[1][o]).sum()), int((co[0][o] * co[1][o]).sum())]
                    for o in range(4)])
        r, d = co[0][3], co[1][3]
    return out


def bands(ref, dis, w, h, bpc, levels, n):
    es = ref.element_size()
    with FeatureEngine(w, h, bit_depth=bpc, n_planes=1, features=N.FEAT_PSNR, max_batch=8, result_capacity=16) as eng:
        args = (ref.data_ptr(), w * es, w * h * es, dis.data_ptr(), w * es, w * h * es, (h, w), n, levels)
        t, got = timed(lambda: eng.band_moments_resident(*args), n)
    want = haar_sums(ref[n - 1].to(torch.int64), dis[n - 1].to(torch.int64), levels)
    assert got[n - 1].view(np.int64).tolist() == want
    return t


def tiles(ref, dis, w, h, bpc, n):
    es = ref.element_size()
    with FeatureEngine(w, h, bit_depth=bpc, n_planes=1, features=N.FEAT_PSNR, max_batch=8, result_capacity=16) as eng:
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
        floor = 2 * w * h * (1 if bpc == 8 else 2) / HBM_BYTES_PER_US
        for levels in (4, 6):
            t = bands(ref, dis, w, h, bpc, levels, a.frames)
            lines.append(f"{w}x{h} {bpc:2d}-bit L {levels} ({a.frames} pairs): {t[0]:7.2f} / {t[1]:7.2f} / {t[2]:7.2f} us/pair (min / "
                         f"median / max of {a.rounds}); tile moments T 64 {tile[0]:6.2f} / {tile[1]:6.2f} / {tile[2]:6.2f}, ratio of minima "
                         f"{t[0] / tile[0]:5.2f}; luma PSNR {psnr[0]:6.2f} / {psnr[1]:6.2f} / {psnr[2]:6.2f} us/frame, ratio of minima "
                         f"{t[0] / psnr[0]:5.2f}, of medians {t[1] / psnr[1]:5.2f}; both planes once at 8 TB/s {floor:5.2f} us, ratio "
                         f"{t[0] / floor:6.2f}")
            print(lines[-1], flush=True)
        del ref, dis
        torch.cuda.empty_cache()
if a.out:
    with open(a.out, "a") as f:
        f.write("".join(line + "\n" for line in lines))
