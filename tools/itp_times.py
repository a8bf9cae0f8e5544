#!/usr/bin/env python3
"""Time per frame pair of the Delta E ITP pass (pqa_delta_itp_device, csrc/delta_itp.hip) on 8 resident 4:2:0 pairs of uniform
noise at 1920x1080 and 3840x2160: pq, hlg and bt1886 at 10 bit, bt1886 at 8 bit, beside three yardsticks taken on the same
planes in the same process: the ciede pass (PQA_FEAT_CIEDE alone, the nearest kernel: the same tile, about 40 transcendentals a
pixel pair), one three-plane PSNR pass (both: HIP events around a resident run, as tools/colour_times.py takes its PSNR pass)
and the issue-count floor -- per pixel pair the transcendentals of the transfer at 8 cycles and 80 plain vector instructions at
4, per wave of 64 pixels, over 256 CUs x 4 SIMDs at 2.4 GHz.  The call is synchronous (a kernel and its epilogue for the 8
pairs, ending in a stream synchronise), so a host clock around it is the time; best of --rounds after a warm-up call.  The last
pair's mean is checked against the numpy restatement at 1080p.
usage: python tools/itp_times.py [--frames 8] [--rounds 5] [--out FILE]"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from pqa2_amd import _native as N
from pqa2_amd import itp
from pqa2_amd.engine import FeatureEngine
from tests import itp_ref as R

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=8)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=None, help="also append the result lines to this file")
a = ap.parse_args()
SIMDS, CYCLES_PER_US = 256 * 4, 2400.0
TRANSCENDENTALS = {"pq": 61, "hlg": 41, "bt1886": 43}   # per pixel pair: 2 x (transfer + 15 for the PQ inverse) + the square root


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


def resident_pass(w, h, bpc, n, features, rp, dp, row, frame):
    """us per frame of one scoring pass with `features` over the resident planes, HIP events around it"""
    with FeatureEngine(w, h, bit_depth=bpc, n_planes=3, features=features, result_capacity=max(16384, n)) as eng:
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


def itp_pass(w, h, bpc, n, transfer, rt, dt, rp, dp, row, frame):
    sp = itp.spec(transfer, "bt2020" if transfer != "bt1886" else "bt709", False, bpc)
    ns = itp.native_spec(sp)
    with FeatureEngine(w, h, bit_depth=bpc, n_planes=3, features=N.FEAT_PSNR, max_batch=8, result_capacity=16) as eng:
        call = lambda: eng.delta_itp_resident(rp, dp, row, frame, n, ns)
        got = call()   # warm-up: code objects, the buffers of first use
        best = None
        for _ in range(a.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = call()
            us = (time.perf_counter() - t0) * 1e6 / n
            best = us if best is None else min(best, us)
    if w <= 1920:
        ref = R.make_spec(transfer, "bt2020" if transfer != "bt1886" else "bt709", False, bpc)
        want = R.frame_sums(host(rt, n - 1, bpc), host(dt, n - 1, bpc), ref, 1, 1)
        assert abs(got[n - 1, 0] - want[0]) / want[6] <= 0.3 and got[n - 1, 6] == want[6], (got[n - 1], want)
    return best


lines = []
for w, h in ((1920, 1080), (3840, 2160)):
    for bpc, transfers in ((10, ("pq", "hlg", "bt1886")), (8, ("bt1886",))):
        (rt, rp, row, frame), (dt, dp, _, _) = clip(w, h, bpc, a.frames, 7), clip(w, h, bpc, a.frames, 8)
        torch.cuda.synchronize()
        psnr = resident_pass(w, h, bpc, a.frames, N.FEAT_PSNR, rp, dp, row, frame)
        ciede = resident_pass(w, h, bpc, a.frames, N.FEAT_CIEDE, rp, dp, row, frame)
        for tr in transfers:
            t = itp_pass(w, h, bpc, a.frames, tr, rt, dt, rp, dp, row, frame)
            floor = (w * h / 64.0) * (TRANSCENDENTALS[tr] * 8 + 80 * 4) / SIMDS / CYCLES_PER_US
            lines.append(f"{w}x{h} {bpc:2d}-bit 4:2:0 delta_itp {tr:6s} ({a.frames} pairs): {t:8.2f} us/pair (best of {a.rounds}); ciede pass "
                         f"{ciede:7.2f} us, ratio {t / ciede:5.2f}; three-plane PSNR {psnr:6.2f} us, ratio {t / psnr:6.2f}; issue floor "
                         f"{floor:6.2f} us, ratio {t / floor:5.2f}")
            print(lines[-1], flush=True)
        del rt, dt
        torch.cuda.empty_cache()
if a.out:
    with open(a.out, "a") as f:
        f.write("".join(line + "\n" for line in lines))
