#!/usr/bin/env python3
"""Time per luma transition of the field moments (pqa_field_moments_device, csrc/field_moments.hip) at 1080p and 2160p, 8 and
10 bit, on 8 resident pairs of uniform noise (7 transitions a synchronous call), beside three yardsticks on the same planes in
the same process: the temporal moments at T = 64 (pqa_temporal_moments_device: the same four planes a transition, 14 dot
products a loaded row where this kernel issues 11, a tile grid written where this one writes 14 words), one luma PSNR pass of
the engine (a FEAT_PSNR context) and the traffic floor of four planes read once at 8 TB/s.  Every call ends in a stream
synchronise, so a host clock around the call is the time; minimum, median and maximum of --rounds after a warm-up call (the
spread within the run).  Every result is checked: the 14 words of the last transition equal torch's sums over the row slices.
usage: python tools/field_times.py [--frames 8] [--rounds 9] [--out FILE]"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
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


def engine(w, h, bpc):
    return FeatureEngine(w, h, bit_depth=bpc, n_planes=1, features=N.FEAT_PSNR, max_batch=8, result_capacity=16)


def fields(ref, dis, w, h, bpc, n):
    es = ref.element_size()
    with engine(w, h, bpc) as eng:
        args = (ref.data_ptr(), w * es, w * h * es, dis.data_ptr(), w * es, w * h * es, (h, w), n)
        t, got = timed(lambda: eng.field_moments_resident(*args), n - 1)
    rk, rp, dk, dp = (x.to(torch.int64) for x in (ref[n - 1], ref[n - 2], dis[n - 1], dis[n - 2]))
    h2 = h // 2

    def E(A, p, B, q):
        d = A[p:2 * h2:2] - B[q:2 * h2:2]
        return int((d * d).sum())
    want = [E(dk, p, rk, q) for p in (0, 1) for q in (0, 1)] + [E(dk, p, rp, q) for p in (0, 1) for q in (0, 1)] + \
           [E(dp, p, rk, q) for p in (0, 1) for q in (0, 1)] + [E(dk, 0, dk, 1), E(rk, 0, rk, 1)]
    assert [int(v) for v in got[n - 2]] == want
    return t


def temporal(ref, dis, w, h, bpc, n):
    es = ref.element_size()
    with engine(w, h, bpc) as eng:
        args = (ref.data_ptr(), w * es, w * h * es, dis.data_ptr(), w * es, w * h * es, (h, w), n, 64)
        return timed(lambda: eng.temporal_moments_resident(*args), n - 1)[0]


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
        tmp = temporal(ref, dis, w, h, bpc, a.frames)
        t = fields(ref, dis, w, h, bpc, a.frames)
        floor = 4 * w * h * (1 if bpc == 8 else 2) / HBM_BYTES_PER_US
        lines.append(f"{w}x{h} {bpc:2d}-bit field moments ({a.frames} pairs): {t[0]:7.2f} / {t[1]:7.2f} / {t[2]:7.2f} us/transition "
                     f"(min / median / max of {a.rounds}); temporal moments T 64 {tmp[0]:6.2f} / {tmp[1]:6.2f} / {tmp[2]:6.2f} "
                     f"us/transition, ratio of minima {t[0] / tmp[0]:5.2f}; luma PSNR {psnr[0]:6.2f} / {psnr[1]:6.2f} / {psnr[2]:6.2f} "
                     f"us/frame, ratio of minima {t[0] / psnr[0]:5.2f}; 4 planes once at 8 TB/s {floor:5.2f} us, ratio {t[0] / floor:6.2f}")
        print(lines[-1], flush=True)
        del ref, dis
        torch.cuda.empty_cache()
if a.out:
    with open(a.out, "a") as f:
        f.write("".join(line + "\n" for line in lines))
