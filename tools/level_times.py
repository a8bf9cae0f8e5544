#!/usr/bin/env python3
"""Time per frame pair of the per-level transfer table (pqa_level_stats_device, luma plane) at 2160p and 1080p, 8 and 10 bit,
on 8 resident luma pairs of three contents: the natural synthetic clip (synth_torch), uniform noise (reference and capture
independent), and a flat frame (every pixel of the reference at one level); beside its yardstick: the luma-only sse kernel of
the same build (a PQA_FEAT_PSNR context with n_planes = 1, HIP events around a resident run of the natural clip), i.e. one
luma PSNR pass, which also reads each plane once.  The level call is synchronous, so a host clock around the call is the
time (it ends in a stream synchronise and includes the clearing of the table and the copy of the result to the host); best
of --rounds after a warm-up call.  Every table is checked: its counts sum to the pixels and its SSE identity
sum_v (T2 - 2 v T1 + v^2 T0) equals the squared error of the pair computed with torch.
usage: python tools/level_times.py [--frames 8] [--rounds 5] [--out FILE]"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from pqa2_amd import _native as N, synth_torch
from pqa2_amd.engine import FeatureEngine

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=8)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=None, help="also append the result lines to this file")
a = ap.parse_args()


def levels(w, h, bpc, ref, dis, n):
    es = ref.element_size()
    with FeatureEngine(w, h, bit_depth=bpc, n_planes=1, features=N.FEAT_PSNR, max_batch=8, result_capacity=16) as eng:
        args = (ref.data_ptr(), w * es, w * h * es, dis.data_ptr(), w * es, w * h * es, n, 0)
        T = eng.level_stats_resident(*args)   # warm-up: code objects, the table of first use
        best = None
        for _ in range(a.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.level_stats_resident(*args)
            us = (time.perf_counter() - t0) * 1e6 / n
            best = us if best is None else min(best, us)
    r, d = ref.to(torch.int64), dis.to(torch.int64)
    sse = ((r - d) ** 2).sum(dim=(1, 2)).cpu().numpy()
    v = np.arange(T.shape[1], dtype=np.int64)
    Ti = T.astype(np.int64)     # far below 2^63 at these sizes
    assert (Ti[:, :, 0].sum(axis=1) == w * h).all()
    assert np.array_equal((Ti[:, :, 2] - 2 * v * Ti[:, :, 1] + v * v * Ti[:, :, 0]).sum(axis=1), sse)
    return best


def psnr_luma(w, h, bpc, ref, dis, n):
    es = ref.element_size()
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
for w, h in ((3840, 2160), (1920, 1080)):
    clip = synth_torch.make_clip_cuda(w, h, a.frames, 8, chroma=False)
    nat_r, nat_d = clip["ref"][0].contiguous(), clip["dis"][0].contiguous()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1234)
    for bpc in (8, 10):
        if bpc == 8:
            dt, ref, dis = torch.uint8, nat_r, nat_d
        else:   # the same pictures as 10-bit samples
            dt, ref, dis = torch.int16, (nat_r.to(torch.int16) * 4 + 1).contiguous(), (nat_d.to(torch.int16) * 4 + 2).contiguous()
        top = (1 << bpc) - 1
        noise_r = torch.randint(0, top + 1, (a.frames, h, w), generator=gen, device="cuda", dtype=torch.int32).to(dt)
        noise_d = torch.randint(0, top + 1, (a.frames, h, w), generator=gen, device="cuda", dtype=torch.int32).to(dt)
        flat_r = torch.full((a.frames, h, w), 16 << (bpc - 8), device="cuda", dtype=dt)
        torch.cuda.synchronize()
        psnr = psnr_luma(w, h, bpc, ref, dis, a.frames)
        t_nat = levels(w, h, bpc, ref, dis, a.frames)
        t_noise = levels(w, h, bpc, noise_r, noise_d, a.frames)
        t_flat = levels(w, h, bpc, flat_r, noise_d, a.frames)
        lines.append(f"{w}x{h} luma {bpc:2d}-bit ({a.frames} pairs): level table natural {t_nat:8.2f}, noise {t_noise:8.2f}, flat "
                     f"{t_flat:8.2f} us/pair (best of {a.rounds}); luma PSNR {psnr:6.2f} us/frame; ratio to one PSNR pass: natural "
                     f"{t_nat / psnr:6.2f}, noise {t_noise / psnr:6.2f}, flat {t_flat / psnr:6.2f}; flat / noise {t_flat / t_noise:5.2f}")
        print(lines[-1], flush=True)
        del noise_r, noise_d, flat_r
    del clip, nat_r, nat_d, ref, dis
    torch.cuda.empty_cache()
if a.out:
    with open(a.out, "a") as f:
        f.write("".join(line + "\n" for line in lines))
