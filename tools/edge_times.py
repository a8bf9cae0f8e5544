#!/usr/bin/env python3
"""Time per luma pair of the edge profiles (pqa_edge_profiles_device) at 1080p and 2160p, 8 and 10 bit, on 8 resident pairs of
uniform noise, beside four yardsticks on the same planes in the same process: the tile moments at T = 64
(pqa_tile_moments_device: the same two planes read once, six sums a tile), two line-profile calls, one per clip
(pqa_line_profiles_device: the same bytes in two launches), one luma PSNR pass of the engine (a FEAT_PSNR context) and the
traffic floor of both planes once at 8 TB/s.  Every call ends in a stream synchronise, so a host clock around the call is the
time; minimum, median and maximum of --rounds after a warm-up call; the calls alternate inside a round, so a disturbance of
the host falls on all of them.  The result is checked: the lines of the last pair add up to torch's sums of the squared
differences of the whole plane.
usage: python tools/edge_times.py [--frames 8] [--rounds 9] [--out FILE]"""
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


def timed(calls, n):
    """{name: (min, median, max) us per unit (n units a call)} of --rounds rounds, every call once a round in turn, after a
    warm-up round (code objects, the buffers of first use), and the last results"""
    got = {k: c() for k, c in calls.items()}
    us = {k: [] for k in calls}
    for _ in range(a.rounds):
        for k, c in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got[k] = c()
            us[k].append((time.perf_counter() - t0) * 1e6 / n)
    return {k: (min(v), sorted(v)[len(v) // 2], max(v)) for k, v in us.items()}, got


lines = []
for w, h in ((1920, 1080), (3840, 2160)):
    for bpc in (8, 10):
        n = a.frames
        ref, dis = planes(w, h, bpc, n, 99), planes(w, h, bpc, n, 7)
        torch.cuda.synchronize()
        es = ref.element_size()
        clip_r, clip_d = (ref.data_ptr(), w * es, w * h * es), (dis.data_ptr(), w * es, w * h * es)
        with FeatureEngine(w, h, bit_depth=bpc, n_planes=1, features=N.FEAT_PSNR, max_batch=8, result_capacity=16) as eng, \
                FeatureEngine(w, h, bit_depth=bpc, n_planes=1, features=N.FEAT_PSNR, result_capacity=max(16384, n)) as peng:
            def psnr():
                peng.reset()
                peng.submit_resident(0, n, [ref.data_ptr()], [dis.data_ptr()], [w * es], [w * h * es])
                peng.sync()

            def two_profiles():
                eng.line_profiles_resident(*clip_r, (h, w), n)
                return eng.line_profiles_resident(*clip_d, (h, w), n)
            t, got = timed({"edge": lambda: eng.edge_profiles_resident(*clip_r, *clip_d, (h, w), n),
                            "tile": lambda: eng.tile_moments_resident(*clip_r, *clip_d, (h, w), n, 64),
                            "prof": two_profiles, "psnr": psnr}, n)
        rows, cols = got["edge"]
        r, d = ref[n - 1].to(torch.int64), dis[n - 1].to(torch.int64)
        for lines_of, (x, y) in ((cols, (r[:, 1:] - r[:, :-1], d[:, 1:] - d[:, :-1])), (rows, (r[1:] - r[:-1], d[1:] - d[:-1]))):
            want = [int(v.sum()) for v in (x * x, y * y, x * y)]
            assert [int(v) for v in lines_of[n - 1].view(np.int64).sum(axis=0)] == want
        floor = 2 * w * h * es / HBM_BYTES_PER_US
        e, ti, pr, ps = t["edge"], t["tile"], t["prof"], t["psnr"]
        lines.append(f"{w}x{h} {bpc:2d}-bit edge profiles ({n} pairs): {e[0]:7.2f} / {e[1]:7.2f} / {e[2]:7.2f} us/pair (min / median / max "
                     f"of {a.rounds}); tile moments T 64 {ti[0]:6.2f} / {ti[1]:6.2f} / {ti[2]:6.2f} us/pair, ratio of minima "
                     f"{e[0] / ti[0]:5.2f}; two line-profile calls {pr[0]:6.2f} / {pr[1]:6.2f} / {pr[2]:6.2f} us/pair, ratio of minima "
                     f"{e[0] / pr[0]:5.2f}; tile + profiles {ti[0] + pr[0]:6.2f}, ratio {e[0] / (ti[0] + pr[0]):5.2f}; luma PSNR {ps[0]:6.2f} / "
                     f"{ps[1]:6.2f} / {ps[2]:6.2f} us/frame, ratio of minima {e[0] / ps[0]:5.2f}; both planes once at 8 TB/s {floor:5.2f} us, "
                     f"ratio {e[0] / floor:6.2f}")
        print(lines[-1], flush=True)
        del ref, dis
        torch.cuda.empty_cache()
if a.out:
    with open(a.out, "a") as f:
        f.write("".join(line + "\n" for line in lines))
