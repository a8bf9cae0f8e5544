#!/usr/bin/env python3
"""Time of the packed RGB converter (pqa_rgb_convert_device) on resident frames of uniform noise, at 1080p and 2160p:
  (a) BGRA -> 4:2:0 left, 8 bit          (b) BGRA -> 4:4:4, 8 bit
  (c) r210 -> 4:2:2 co-sited, 10 bit     (d) r210 -> 4:2:0 left, 10 bit
  (e) BGRA luma only                     (g) (a) on the general path (PQA_RGB_GENERIC)
and beside each of them
  floor  its traffic floor: 4 bytes in plus the plane bytes out per pixel, at 8 TB/s,
  copy   a device-to-device copy of the same number of bytes (half read, half written; torch's copy_),
and once per size
  empty  a call with no frames (the entry's own cost: checks and the return),
  yuv    the existing route for a Y'CbCr capture of the size: pqa_unpack_device of UYVY (8 bit) / v210 (10 bit) plus
         pqa_format_convert_device 4:2:2 -> 4:2:0 of U and V -- the comparable job in two passes, three calls.
Every call is synchronous (it ends in a stream synchronise), so HIP events around it time the launch, the kernel and the
synchronise; minimum and spread (min ... max) of --rounds calls after a warm-up call.  The last frame of (a) and (d) is checked
against the numpy restatement at 1080p.
usage: python tools/rgb_convert_times.py [--frames 8] [--rounds 9] [--out FILE]"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from pqa2_amd import _native as N
from pqa2_amd import rgb
from pqa2_amd.engine import FeatureEngine
from tests import rgb_ref as R

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=8)
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--out", default=None, help="also append the result lines to this file")
a = ap.parse_args()
HBM_BYTES_PER_US = 8.0e6   # 8 TB/s
LEFT, C422, C444 = (1, 1, 0, 1), (1, 0, 0, 0), (0, 0, 0, 0)


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


def rgb_case(eng, fmt, w, h, lay, db, n, luma_only=False, generic=False, check=False):
    """((min, max), bytes moved) of one resident call; rows 4 * w bytes apart, planes packed"""
    gen = torch.Generator(device="cuda")
    gen.manual_seed(w + db)
    src = torch.randint(0, 256, (n, h, 4 * w), generator=gen, device="cuda", dtype=torch.int32).to(torch.uint8)
    es = 1 if db == 8 else 2
    ch, cw = FeatureEngine.convert_plane_shape((h, w), lay[0], lay[1])
    shapes = [(h, w)] if luma_only else [(h, w), (ch, cw), (ch, cw)]
    dst = [torch.zeros((n, ph, pw * es), device="cuda", dtype=torch.uint8) for ph, pw in shapes]
    m = rgb.conversion_matrix("bt709", rgb.BIT_DEPTH[fmt], fmt != "r210", db, False)
    pad = [0] * (3 - len(shapes))
    t = timed(lambda: eng.rgb_convert_resident(fmt, (h, w), (*lay, db), m, src.data_ptr(), 4 * w, 4 * w * h, n, [d.data_ptr() for d in dst],
                                               [pw * es for _, pw in shapes] + pad, [ph * pw * es for ph, pw in shapes] + pad, generic=generic))
    if check:
        want = R.convert(src[n - 1].cpu().numpy(), fmt, w, h, m, (*lay, db))
        for d, wnt in zip(dst, want):
            assert np.array_equal(d[n - 1].cpu().numpy().view(wnt.dtype), wnt)
    return t, (4 * w * h + sum(ph * pw * es for ph, pw in shapes)) * n


def copy_case(nbytes):
    s = torch.zeros(nbytes // 2, device="cuda", dtype=torch.uint8)
    d = torch.empty_like(s)

    def call():
        d.copy_(s)
        torch.cuda.synchronize()
    return timed(call)


def yuv_case(eng, w, h, bits, n):
    """unpack of a packed 4:2:2 capture, then U and V 4:2:2 -> 4:2:0 at the same depth: the two-pass route that exists"""
    fmt = "uyvy422" if bits == 8 else "v210"
    es = 1 if bits == 8 else 2
    row = 4 * ((w + 1) // 2) if bits == 8 else 16 * ((w + 5) // 6)
    cw, ch = (w + 1) // 2, (h + 1) // 2
    src = torch.zeros((n, h, row), device="cuda", dtype=torch.uint8)
    y, u, v = (torch.zeros((n, h, pw * es), device="cuda", dtype=torch.uint8) for pw in (w, cw, cw))
    u2, v2 = (torch.zeros((n, ch, cw * es), device="cuda", dtype=torch.uint8) for _ in range(2))
    s422, d420 = (1, 0, 0, 0, bits), (1, 1, 0, 1, bits)

    def call():
        eng.unpack_resident(fmt, (h, w), src.data_ptr(), row, row * h, n, [y.data_ptr(), u.data_ptr(), v.data_ptr()], [w * es, cw * es, cw * es],
                            [w * h * es, cw * h * es, cw * h * es])
        for s, d in ((u, u2), (v, v2)):
            eng.format_convert_resident((h, w), s422, d420, s.data_ptr(), cw * es, cw * h * es, d.data_ptr(), cw * es, cw * ch * es, n)
    return timed(call)


n = a.frames
lines = [f"packed RGB conversion, {n} resident frames a call, HIP events around the synchronous call, per call: min (min ... max) of "
         f"{a.rounds} after a warm-up; one run, run to run not measured"]
print(lines[0], flush=True)
for w, h in ((1920, 1080), (3840, 2160)):
    with FeatureEngine(w, h, bit_depth=8, n_planes=1, features=N.FEAT_PSNR, max_batch=8, result_capacity=16) as eng:
        check = h == 1080
        cases = [("(a) bgra -> 4:2:0 left 8 bit  ", rgb_case(eng, "bgra", w, h, LEFT, 8, n, check=check)),
                 ("(b) bgra -> 4:4:4 8 bit       ", rgb_case(eng, "bgra", w, h, C444, 8, n)),
                 ("(c) r210 -> 4:2:2 10 bit      ", rgb_case(eng, "r210", w, h, C422, 10, n)),
                 ("(d) r210 -> 4:2:0 left 10 bit ", rgb_case(eng, "r210", w, h, LEFT, 10, n, check=check)),
                 ("(e) bgra luma only 8 bit      ", rgb_case(eng, "bgra", w, h, LEFT, 8, n, luma_only=True)),
                 ("(g) (a) on the general path   ", rgb_case(eng, "bgra", w, h, LEFT, 8, n, generic=True))]
        empty = timed(lambda: eng.rgb_convert_resident("bgra", (h, w), (*LEFT, 8), rgb.conversion_matrix("bt709", 8, True, 8, False), 0, 4 * w,
                                                       4 * w * h, 0, [0, 0, 0], [w, w // 2, w // 2], [w * h, w * h // 4, w * h // 4]))
        yuv8, yuv10 = yuv_case(eng, w, h, 8, n), yuv_case(eng, w, h, 10, n)
    head = f"{w}x{h}, {n} frames:"
    first = len(lines)
    for name, ((lo, hi), nbytes) in cases:
        floor = nbytes / HBM_BYTES_PER_US
        clo, chi = copy_case(nbytes)
        lines.append(f"{head} {name} {lo:9.1f} us ({lo:.1f} ... {hi:.1f}), {lo / n:7.1f} us a frame; floor {floor:8.1f} us, ratio {lo / floor:5.2f}; "
                     f"copy of the bytes {clo:8.1f} us ({clo:.1f} ... {chi:.1f}), ratio {lo / clo:5.2f}")
    t = {name[:3]: v[0][0] for name, v in cases}
    lines += [
        f"{head} empty call                     {empty[0]:9.1f} us ({empty[0]:.1f} ... {empty[1]:.1f})",
        f"{head} yuv route, uyvy 8 bit          {yuv8[0]:9.1f} us ({yuv8[0]:.1f} ... {yuv8[1]:.1f}): unpack + U, V 4:2:2 -> 4:2:0, three calls",
        f"{head} yuv route, v210 10 bit         {yuv10[0]:9.1f} us ({yuv10[0]:.1f} ... {yuv10[1]:.1f})",
        f"{head} ratios (a)/yuv8 {t['(a)'] / yuv8[0]:.2f}   (d)/yuv10 {t['(d)'] / yuv10[0]:.2f}   (g)/(a) {t['(g)'] / t['(a)']:.2f}   "
        f"(a)/(b) {t['(a)'] / t['(b)']:.2f}   (e)/(a) {t['(e)'] / t['(a)']:.2f}",
    ]
    for ln in lines[first:]:
        print(ln, flush=True)
    torch.cuda.empty_cache()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("".join(line + "\n" for line in lines))
