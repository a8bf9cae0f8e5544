#!/usr/bin/env python3
"""Time of the deinterlacer (pqa_deinterlace_device) per OUTPUT plane on 8 resident source planes a call at rate "frame", at 1080p
and 2160p, 8 and 10 bit, both modes, on a static clip (every plane the same noise: every wave takes the still-picture fast
path) and on a clip that moves everywhere (independent noise), with the fast path on and off (PQA_DEINT_UNIFORM, read when the
context is made).  Beside each, in the same run:
  (c) a device copy of the output bytes (hipMemcpyAsync device to device through torch),
  (t) pqa_table_apply_device on the same planes, out of place,
  (f) the traffic floor at 8 TB/s: 2.5 planes read and 1 written an output plane (intra: 0.5 read and 1 written).
Every library call is synchronous (it ends in a stream synchronise), so HIP events around it time the launch, the kernel and the
synchronise; minimum and spread (min ... max) of --rounds calls after a warm-up call, divided by the number of output planes.
One output plane of every case is compared with the numpy restatement on its first 64 rows.
usage: python tools/deinterlace_times.py [--frames 8] [--rounds 9] [--out FILE]"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from pqa2_amd import _native as N
from pqa2_amd.engine import FeatureEngine
from tests import deinterlace_ref

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=8)
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--out", default=None, help="also append the result lines to this file")
a = ap.parse_args()
HBM_BYTES_PER_US = 8.0e6   # 8 TB/s


def noise(n, h, w, bits, seed):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    return torch.randint(0, 1 << bits, (n, h, w), generator=gen, device="cuda", dtype=torch.int32).to(torch.uint8 if bits == 8 else torch.int16)


def timed(call):
    """(min, max) in microseconds of a.rounds synchronous calls, after a warm-up call"""
    call()
    ts = []
    for _ in range(a.rounds):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        call()
        t1.record()
        torch.cuda.synchronize()
        ts.append(t0.elapsed_time(t1) * 1e3)
    return min(ts), max(ts)


def engine(w, h, bits, uniform):
    if uniform:
        os.environ.pop("PQA_DEINT_UNIFORM", None)
    else:
        os.environ["PQA_DEINT_UNIFORM"] = "0"
    eng = FeatureEngine(w, h, bit_depth=bits, n_planes=1, features=N.FEAT_PSNR, max_batch=8, result_capacity=16)
    os.environ.pop("PQA_DEINT_UNIFORM", None)
    return eng


n = a.frames
lines = [f"deinterlace, {n} resident source planes a call, rate frame, per output plane; HIP events around the synchronous call, min (min ... max) "
         f"of {a.rounds} after a warm-up; one run, spread from run to run not measured"]
print(lines[0], flush=True)
for (w, h), bits in (((1920, 1080), 8), ((1920, 1080), 10), ((3840, 2160), 8), ((3840, 2160), 10)):
    dt = np.uint8 if bits == 8 else np.uint16
    moving = noise(n, h, w, bits, 1)
    static = moving[:1].expand(n, h, w).contiguous()
    dst = torch.zeros_like(moving)
    es = moving.element_size()
    rp, fp = w * es, w * h * es
    table = np.random.default_rng(bits).permutation(1 << bits).astype(dt)
    head = f"{w}x{h} {bits:2d}-bit:"
    got = {}
    for uniform in (True, False):
        with engine(w, h, bits, uniform) as eng:
            for mode in ("adaptive", "intra"):
                for name, src in (("static", static), ("moving", moving)):
                    if mode == "intra" and (name == "static" or not uniform):
                        continue      # the intra mode reads one frame and has no fast path: one case
                    got[(mode, name, uniform)] = timed(lambda: eng.deinterlace_resident((h, w), src.data_ptr(), rp, fp, dst.data_ptr(), rp, fp, n,
                                                                                      mode, 0, "frame"))
                    k = n // 2
                    rows = [src[j, :64].cpu().numpy().view(dt) for j in (k - 1, k, k + 1)]
                    want = deinterlace_ref.deinterlace(rows, mode, 0, "frame", bits)[1]
                    assert np.array_equal(dst[k, :56].cpu().numpy().view(dt), want[:56]), (mode, name, uniform)      # rows clear of the cut
            if uniform:
                kt = timed(lambda: eng.table_apply_resident(table, (h, w), moving.data_ptr(), rp, fp, dst.data_ptr(), rp, fp, n))

    def copy():
        dst.copy_(moving)
        torch.cuda.synchronize()
    kc = timed(copy)
    floor = {"adaptive": 3.5 * fp / HBM_BYTES_PER_US, "intra": 1.5 * fp / HBM_BYTES_PER_US}
    for (mode, name, uniform), (lo, hi) in got.items():
        what = f"{mode}, {name} clip, fast path {'on' if uniform else 'off'}"
        lines.append(f"{head} {what:42s}{lo / n:9.2f} us ({lo / n:.2f} ... {hi / n:.2f})   x{lo / kc[0]:.2f} copy   x{lo / kt[0]:.2f} table apply   "
                     f"x{lo / n / floor[mode]:.2f} floor")
    lines += [f"{head} {'(c) device copy of the output planes':42s}{kc[0] / n:9.2f} us ({kc[0] / n:.2f} ... {kc[1] / n:.2f})",
              f"{head} {'(t) table apply on the same planes':42s}{kt[0] / n:9.2f} us ({kt[0] / n:.2f} ... {kt[1] / n:.2f})",
              f"{head} {'(f) floor at 8 TB/s, adaptive / intra':42s}{floor['adaptive']:9.2f} / {floor['intra']:.2f} us"]
    for ln in lines[-(len(got) + 3):]:
        print(ln, flush=True)
    del moving, static, dst
    torch.cuda.empty_cache()
if a.out:
    with open(a.out, "a") as f:
        f.write("".join(line + "\n" for line in lines))
