#!/usr/bin/env python3
"""Time of the table apply (pqa_table_apply_device) per luma plane on resident planes of uniform noise through a random
permutation table (the worst spread of LDS addresses), 8 planes a call, at 1080p and 2160p, 8 and 10 bit:
  (a) the kernel, out of place,
  (b) the kernel in place,
  (c) a device copy of the same planes (hipMemcpyAsync device to device through torch),
  (d) one luma PSNR pass over frames of the size,
  (e) the traffic floor: one read plus one write of the plane at 8 TB/s.
Every library call is synchronous (it ends in a stream synchronise), so HIP events around it time the table's upload, the
launch, the kernel and the synchronise; minimum and spread (min ... max) of --rounds calls after a warm-up call, divided by the
number of planes.  One plane of (a) is checked against numpy.take.
End to end: score_files(level_align="apply", level_curve=True) on a gamma'd 1080p 8-bit Y4M pair (PSNR only, no model), wall
clock, against the same run with the curve tables put through numpy.take on the host (pipeline._LevelledReader in place of
pipeline._TableReader): what the GPU path replaces.
usage: python tools/table_apply_times.py [--frames 8] [--rounds 9] [--clip-frames 16] [--out FILE]"""
import argparse, os, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from pqa2_amd import _native as N
from pqa2_amd import pipeline
from pqa2_amd.engine import FeatureEngine
from pqa2_amd.yuvio import VideoInfo, write_y4m

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=8)
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--clip-frames", type=int, default=16)
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


def psnr_case(h, w, bits, n, seed):
    ref, dis = noise(n, h, w, bits, seed), noise(n, h, w, bits, seed + 1)
    es = ref.element_size()
    with FeatureEngine(w, h, bit_depth=bits, n_planes=1, features=N.FEAT_PSNR, result_capacity=max(16384, n)) as eng:
        def call():
            eng.reset()
            eng.submit_resident(0, n, [ref.data_ptr()], [dis.data_ptr()], [w * es], [w * h * es])
            eng.sync()
        return timed(call)


n = a.frames
lines = [f"table apply, {n} resident luma planes a call, per plane; HIP events around the synchronous call, min (min ... max) of {a.rounds} "
         f"after a warm-up; one run, spread from run to run not measured"]
print(lines[0], flush=True)
for (w, h), bits in (((1920, 1080), 8), ((1920, 1080), 10), ((3840, 2160), 8), ((3840, 2160), 10)):
    dt = np.uint8 if bits == 8 else np.uint16
    table = np.random.default_rng(bits).permutation(1 << bits).astype(dt)
    src = noise(n, h, w, bits, 1)
    dst, work = torch.zeros_like(src), src.clone()
    es = src.element_size()
    rp, fp = w * es, w * h * es
    with FeatureEngine(w, h, bit_depth=bits, n_planes=1, features=N.FEAT_PSNR, max_batch=8, result_capacity=16) as eng:
        ka = timed(lambda: eng.table_apply_resident(table, (h, w), src.data_ptr(), rp, fp, dst.data_ptr(), rp, fp, n))
        assert np.array_equal(dst[n - 1].cpu().numpy().view(dt), table[src[n - 1].cpu().numpy().view(dt)])
        kb = timed(lambda: eng.table_apply_resident(table, (h, w), work.data_ptr(), rp, fp, work.data_ptr(), rp, fp, n))

    def copy():
        dst.copy_(src)
        torch.cuda.synchronize()
    kc = timed(copy)
    kd = psnr_case(h, w, bits, n, 4)
    floor = 2 * fp / HBM_BYTES_PER_US
    head = f"{w}x{h} {bits:2d}-bit:"
    lines += [f"{head} ({c}) {what:34s}{lo / n:9.2f} us ({lo / n:.2f} ... {hi / n:.2f})"
              for c, what, (lo, hi) in (("a", "table apply, out of place", ka), ("b", "table apply, in place", kb),
                                        ("c", "device copy of the planes", kc), ("d", "one luma PSNR pass", kd))]
    lines += [f"{head} (e) {'one read + one write at 8 TB/s':34s}{floor:9.2f} us",
              f"{head} ratios (a)/(c) {ka[0] / kc[0]:.2f}   (a)/(e) {ka[0] / n / floor:.2f}   (a)/(d) {ka[0] / kd[0]:.2f}"]
    for ln in lines[-6:]:
        print(ln, flush=True)
    del src, dst, work
    torch.cuda.empty_cache()

# ---- end to end ------------------------------------------------------------------------------------------------------------
w, h, nf = 1920, 1080, a.clip_frames
rng = np.random.default_rng(3)
yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
info = VideoInfo(width=w, height=h, fps_num=24, fps_den=1, bit_depth=8, mono=False, hshift=1, vshift=1, chroma_tag="420", color_range="full")
ref, cap = [], []
for t in range(nf):
    f = np.sin((xx + 3 * t) / 97.0) * np.cos((yy - 2 * t) / 71.0) + 0.6 * np.sin((xx + yy) / 173.0 + t) + rng.normal(0, 0.05, (h, w))
    y = np.round(255 * (f - f.min()) / (f.max() - f.min())).astype(np.uint8)
    c = [np.full((h // 2, w // 2), 128, np.uint8) for _ in range(2)]
    ref.append([y] + c)
    cap.append([np.clip(np.floor(255 * (y / 255.0) ** (2.4 / 2.2) + 0.5), 0, 255).astype(np.uint8)] + c)


class HostTables(pipeline._LevelledReader):
    """the same tables through numpy.take on the host"""

    def __init__(self, reader, tables, device, make):
        super().__init__(reader, tables)

    def close(self):
        pass


with tempfile.TemporaryDirectory() as tmp:
    rp_, dp_ = os.path.join(tmp, "ref.y4m"), os.path.join(tmp, "dis.y4m")
    write_y4m(rp_, ref, info)
    write_y4m(dp_, cap, info)
    kw = dict(model=None, psnr=True, ssim=False, level_align="apply", level_curve=True)
    walls, records = {}, {}
    gpu_reader = pipeline._TableReader
    for name, reader in (("gpu", gpu_reader), ("host", HostTables), ("gpu", gpu_reader), ("host", HostTables)):   # the second pair counts
        pipeline._TableReader = reader
        t0 = time.perf_counter()
        res = pipeline.score_files(rp_, dp_, **kw)
        walls[name], records[name] = time.perf_counter() - t0, res["records"]
        assert res["alignment"]["levels"]["curve_applied"]
    pipeline._TableReader = gpu_reader
    assert np.array_equal(records["gpu"].view(np.uint64), records["host"].view(np.uint64))
lines += [f"end to end, {w}x{h} 8-bit 4:2:0 Y4M pair with a 2.4 / 2.2 gamma leg on the luma, {nf} frames, PSNR only, wall clock of the "
          f"second of two runs each:",
          f"  score_files(level_align=\"apply\", level_curve=True), table on the GPU {walls['gpu'] * 1e3:9.1f} ms",
          f"  the same with the tables through numpy.take on the host             {walls['host'] * 1e3:9.1f} ms   (same records)"]
for ln in lines[-3:]:
    print(ln, flush=True)
if a.out:
    with open(a.out, "a") as f:
        f.write("".join(line + "\n" for line in lines))
