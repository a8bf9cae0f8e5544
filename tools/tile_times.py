#!/usr/bin/env python3
"""Time per luma pair of the tile moments (pqa_tile_moments_device) at 1080p and 2160p, 8 and 10 bit, tiles of 8 and 64, on 8
resident pairs of uniform noise; beside two yardsticks on the same planes: one luma PSNR pass of the engine (a FEAT_PSNR
context: the same two reads with one sum instead of six), and one read of both planes at 8 TB/s.  Both calls end in a
stream synchronise, so a host clock around the call is the time (the tile call includes the copy of its sums to the host:
ty * tx * 48 bytes a pair); minimum, median and maximum of --rounds after a warm-up call.  Every result is checked: the
tiles of the last pair add up to torch's sums of the whole plane, and its last two tile rows and columns equal numpy's.
usage: python tools/tile_times.py [--frames 8] [--rounds 9] [--out FILE]"""
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


def tiles(ref, dis, w, h, bpc, tile, n):
    es = ref.element_size()
    with FeatureEngine(w, h, bit_depth=bpc, n_planes=1, features=N.FEAT_PSNR, max_batch=8, result_capacity=16) as eng:
        args = (ref.data_ptr(), w * es, w * h * es, dis.data_ptr(), w * es, w * h * es, (h, w), n, tile)
        t, got = timed(lambda: eng.tile_moments_resident(*args), n)
    r, d = ref[n - 1].to(torch.int64), dis[n - 1].to(torch.int64)
    want = [int(v.sum()) for v in (r, d, r * r, d * d, r * d, (d - r).abs())]
    assert [int(v) for v in got[n - 1].sum(axis=(0, 1), dtype=np.uint64)] == want
    ty, tx = got.shape[1:3]
    y0, x0 = (ty - 2) * tile, (tx - 2) * tile
    rc, dc = r[y0:, x0:].cpu().numpy(), d[y0:, x0:].cpu().numpy()
    for m, v in enumerate((rc, dc, rc * rc, dc * dc, rc * dc, np.abs(dc - rc))):
        for j in range(2):
            for i in range(2):
                assert int(got[n - 1, ty - 2 + j, tx - 2 + i, m]) == int(v[j * tile:(j + 1) * tile, i * tile:(i + 1) * tile].sum())
    return t


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
        floor = 2 * w * h * (1 if bpc == 8 else 2) / HBM_BYTES_PER_US
        for tile in (8, 64):
            t = tiles(ref, dis, w, h, bpc, tile, a.frames)
            lines.append(f"{w}x{h} {bpc:2d}-bit tile {tile:2d} ({a.frames} pairs): {t[0]:7.2f} / {t[1]:7.2f} / {t[2]:7.2f} us/pair (min / "
                         f"median / max of {a.rounds}); luma PSNR {psnr[0]:6.2f} / {psnr[1]:6.2f} / {psnr[2]:6.2f} us/frame; ratio of minima "
                         f"{t[0] / psnr[0]:5.2f}, of medians {t[1] / psnr[1]:5.2f}; both planes once at 8 TB/s {floor:5.2f} us, ratio "
                         f"{t[0] / floor:6.2f}")
            print(lines[-1], flush=True)
        del ref, dis
        torch.cuda.empty_cache()
if a.out:
    with open(a.out, "a") as f:
        f.write("".join(line + "\n" for line in lines))
