#!/usr/bin/env python3
"""Time of the mask blend (pqa_mask_blend_device) per luma plane on resident planes of uniform noise, 8 planes a call, at 1080p
and 2160p, 8 and 10 bit, constant fill, nodes 8 samples apart:
  (a) whole plane, not in place, under a mask of one box in the middle that covers about 2 % of the frame (feather 16),
  (b) in place under the same mask: the launch covers the mask's bounds only,
  (c) in place with every node at 256: every item is filled, the source is not read,
  (d) the table apply in place on the same planes (pqa_table_apply_device, an identity table),
  (e) a device copy of the same planes (hipMemcpyAsync device to device through torch).
Every library call is synchronous (it ends in a stream synchronise), so HIP events around it time the upload of the node grid
(or the table), the launch, the kernel and the synchronise; minimum and spread (min ... max) of --rounds calls after a warm-up
call, divided by the number of planes.  One plane of (a) and of (b) is checked against a numpy blend.
The ratio to read first is (b) / (a): whether the bounding-rectangle launch works.
usage: python tools/mask_blend_times.py [--frames 8] [--rounds 9] [--out FILE]"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from pqa2_amd import _native as N
from pqa2_amd import distortion as D
from pqa2_amd.engine import FeatureEngine

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=8)
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--out", default=None, help="also append the result lines to this file")
a = ap.parse_args()


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


def blend_ref(src, nodes, fill):
    al = D.mask_alpha(nodes, src.shape[1], src.shape[0], 3, 3)
    return ((src.astype(np.int64) * (256 - al) + fill * al + 128) >> 8).astype(src.dtype)


n = a.frames
lines = [f"mask blend, {n} resident luma planes a call, per plane; HIP events around the synchronous call, min (min ... max) of {a.rounds} "
         f"after a warm-up; one run, spread from run to run not measured"]
print(lines[0], flush=True)
for (w, h), bits in (((1920, 1080), 8), ((1920, 1080), 10), ((3840, 2160), 8), ((3840, 2160), 10)):
    dt = np.uint8 if bits == 8 else np.uint16
    fill = 1 << (bits - 1)
    bw, bh = (w * 14 // 100) // 16 * 16, (h * 14 // 100) // 8 * 8      # 14 % of each side: 2 % of the frame
    x0, y0 = (w - bw) // 2 // 16 * 16, (h - bh) // 2 // 8 * 8
    mask = D.overlay_mask_from_boxes([[x0, y0, x0 + bw, y0 + bh]], w, h, feather=16, node=8)
    full = np.full_like(mask["nodes"], 256)
    table = np.arange(1 << bits).astype(dt)
    src = noise(n, h, w, bits, 1)
    dst, work = torch.zeros_like(src), src.clone()
    es = src.element_size()
    rp, fp = w * es, w * h * es
    with FeatureEngine(w, h, bit_depth=bits, n_planes=1, features=N.FEAT_PSNR, max_batch=8, result_capacity=16) as eng:
        ka = timed(lambda: eng.mask_blend_resident(mask["nodes"], (3, 3), fill, (h, w), src.data_ptr(), rp, fp, dst.data_ptr(), rp, fp, n))
        want = blend_ref(src[n - 1].cpu().numpy().view(dt), mask["nodes"], fill)
        assert np.array_equal(dst[n - 1].cpu().numpy().view(dt), want)
        kb = timed(lambda: eng.mask_blend_resident(mask["nodes"], (3, 3), fill, (h, w), work.data_ptr(), rp, fp, work.data_ptr(), rp, fp, n))
        bx0, by0, bx1, by1 = mask["bounds"]
        got = work[n - 1].cpu().numpy().view(dt)
        inside = np.zeros((h, w), bool)
        inside[y0:y0 + bh, x0:x0 + bw] = True
        assert (got[inside] == fill).all() and np.array_equal(got[:by0], want[:by0]) and np.array_equal(got[:, :bx0], want[:, :bx0])
        kc = timed(lambda: eng.mask_blend_resident(full, (3, 3), fill, (h, w), work.data_ptr(), rp, fp, work.data_ptr(), rp, fp, n))
        assert (work[n - 1] == fill).all()
        work.copy_(src)
        kd = timed(lambda: eng.table_apply_resident(table, (h, w), work.data_ptr(), rp, fp, work.data_ptr(), rp, fp, n))

    def copy():
        dst.copy_(src)
        torch.cuda.synchronize()
    ke = timed(copy)
    head = f"{w}x{h} {bits:2d}-bit:"
    lines += [f"{head} mask of one {bw}x{bh} box, bounds {bx1 - bx0}x{by1 - by0}, share of samples with alpha > 0 {mask['share']:.4f}"]
    lines += [f"{head} ({c}) {what:40s}{lo / n:9.2f} us ({lo / n:.2f} ... {hi / n:.2f})"
              for c, what, (lo, hi) in (("a", "mask blend, whole plane, not in place", ka), ("b", "mask blend in place, the 2 % mask", kb),
                                        ("c", "mask blend in place, every node 256", kc), ("d", "table apply in place", kd),
                                        ("e", "device copy of the planes", ke))]
    lines += [f"{head} ratios (b)/(a) {kb[0] / ka[0]:.3f}   (a)/(e) {ka[0] / ke[0]:.2f}   (c)/(d) {kc[0] / kd[0]:.2f}"]
    for ln in lines[-7:]:
        print(ln, flush=True)
    del src, dst, work
    torch.cuda.empty_cache()
if a.out:
    with open(a.out, "a") as f:
        f.write("".join(line + "\n" for line in lines))
