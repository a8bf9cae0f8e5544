#!/usr/bin/env python3
"""Time of the pixel-format converter (pqa_format_convert_device) on resident planes of uniform noise, 8 frames a call, at
1080p and 2160p, 8 and 10 bit:
  (a) U + V of 4:2:2 -> 4:2:0 (2 x frames planes in one call) on the fast path,
  (b) the same call on the general path (PQA_CONVERT_GENERIC),
  (c) the luma depth pass 10 -> 8 bit of a v210 capture against an 8-bit master (one plane a frame),
  (d) the yardstick from code that was there before: two pqa_resample_device bilinear calls that do the same 4:2:2 -> 4:2:0 job
      on U and on V (window (0, 0, w, h), destination height halved; other integers, the same work),
  (e) one three-plane PSNR pass over 4:2:0 frames of the size,
  (f) the traffic floor of (a): bytes read once plus bytes written once at 8 TB/s.
Every call is synchronous (it ends in a stream synchronise), so HIP events around it time the launch, the kernel and the
synchronise; minimum and spread (min ... max) of --rounds calls after a warm-up call.  One plane of (a) and (c) is checked
against the numpy restatement.  --frames 64 gives the same table with the per-call cost spread over more planes.
usage: python tools/format_convert_times.py [--frames 8] [--rounds 9] [--out FILE]"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from pqa2_amd import _native as N
from pqa2_amd.engine import FeatureEngine
from tests import format_convert_ref as FR

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


def np_plane(t, bits):
    return t.cpu().numpy().view(np.uint8 if bits == 8 else np.uint16)


def convert_case(eng, luma, src, dst, n_planes, generic, seed):
    sh, sw = FeatureEngine.convert_plane_shape(luma, src[0], src[1])
    dh, dw = FeatureEngine.convert_plane_shape(luma, dst[0], dst[1])
    s, d = noise(n_planes, sh, sw, src[4], seed), torch.zeros((n_planes, dh, dw), device="cuda", dtype=torch.uint8 if dst[4] == 8 else torch.int16)
    ses, des = s.element_size(), d.element_size()
    t = timed(lambda: eng.format_convert_resident(luma, src, dst, s.data_ptr(), sw * ses, sw * sh * ses, d.data_ptr(), dw * des, dw * dh * des,
                                                  n_planes, generic=generic))
    want = FR.convert(np_plane(s[n_planes - 1, -40:], src[4]), (40 << src[1], luma[1]), src, dst)   # the last rows of the last plane
    rows = want.shape[0] - 4                                                                      # but those that see the cut edge
    assert np.array_equal(np_plane(d[n_planes - 1], dst[4])[-rows:], want[-rows:])
    return t, (sw * sh * ses + dw * dh * des) * n_planes


def resample_case(eng, luma, bits, n_planes, seed):
    """(d): U, then V, of 4:2:2 -> 4:2:0 through the bilinear resampler: two calls of n_planes / 2 planes"""
    h, w = luma[0], (luma[1] + 1) // 2
    dh = (h + 1) // 2
    half = n_planes // 2
    s = [noise(half, h, w, bits, seed + k) for k in range(2)]
    d = [torch.zeros((half, dh, w), device="cuda", dtype=s[0].dtype) for _ in range(2)]
    es = s[0].element_size()

    def call():
        for k in range(2):
            eng.resample_resident(s[k].data_ptr(), w * es, w * h * es, (h, w), d[k].data_ptr(), w * es, w * dh * es, (dh, w), half, "bilinear",
                                  window=(0, 0, w, h))
    return timed(call)


def psnr_case(luma, bits, n, seed):
    h, w = luma
    ch, cw = (h + 1) // 2, (w + 1) // 2
    ref = [noise(n, *s, bits, seed + k) for k, s in enumerate(((h, w), (ch, cw), (ch, cw)))]
    dis = [noise(n, *s, bits, seed + 3 + k) for k, s in enumerate(((h, w), (ch, cw), (ch, cw)))]
    es = ref[0].element_size()
    rp, fp = [w * es, cw * es, cw * es], [w * h * es, cw * ch * es, cw * ch * es]
    with FeatureEngine(w, h, bit_depth=bits, n_planes=3, chroma_shift=(1, 1), features=N.FEAT_PSNR, result_capacity=max(16384, n)) as eng:
        def call():
            eng.reset()
            eng.submit_resident(0, n, [t.data_ptr() for t in ref], [t.data_ptr() for t in dis], rp, fp)
            eng.sync()
        return timed(call)


lines = [f"format conversion, {a.frames} resident frames a call, HIP events around the synchronous call, min (min ... max) of {a.rounds} "
         f"after a warm-up; one run, run to run not measured"]
print(lines[0], flush=True)
n = a.frames
for (w, h), bits in (((1920, 1080), 8), ((1920, 1080), 10), ((3840, 2160), 8), ((3840, 2160), 10)):
    luma = (h, w)
    s422, d420 = (1, 0, 0, 0, bits), (1, 1, 0, 1, bits)
    with FeatureEngine(w, h, bit_depth=bits, n_planes=1, features=N.FEAT_PSNR, max_batch=8, result_capacity=16) as eng:
        (fa, fa_max), traffic = convert_case(eng, luma, s422, d420, 2 * n, False, 1)
        (ga, ga_max), _t = convert_case(eng, luma, s422, d420, 2 * n, True, 1)
        (ca, ca_max), ctraffic = convert_case(eng, luma, (0, 0, 0, 0, 10), (0, 0, 0, 0, 8), n, False, 2)
        ra, ra_max = resample_case(eng, luma, bits, 2 * n, 3)
    pa, pa_max = psnr_case(luma, bits, n, 4)
    floor, cfloor = traffic / HBM_BYTES_PER_US, ctraffic / HBM_BYTES_PER_US
    head = f"{w}x{h} {bits:2d}-bit, {n} frames:"
    lines += [
        f"{head} (a) U+V 4:2:2 -> 4:2:0 fast path     {fa:9.1f} us ({fa:.1f} ... {fa_max:.1f})",
        f"{head} (b) the same, general path          {ga:9.1f} us ({ga:.1f} ... {ga_max:.1f})",
        f"{head} (c) luma 10 -> 8 bit depth pass      {ca:9.1f} us ({ca:.1f} ... {ca_max:.1f}); its traffic floor {cfloor:.1f} us, ratio {ca / cfloor:.2f}",
        f"{head} (d) two bilinear resample calls     {ra:9.1f} us ({ra:.1f} ... {ra_max:.1f})",
        f"{head} (e) one three-plane PSNR pass       {pa:9.1f} us ({pa:.1f} ... {pa_max:.1f})",
        f"{head} (f) traffic floor of (a) at 8 TB/s  {floor:9.1f} us",
        f"{head} ratios (a)/(d) {fa / ra:.3f}   (a)/(f) {fa / floor:.2f}   (b)/(a) {ga / fa:.2f}   (a)/(e) {fa / pa:.3f}",
    ]
    for ln in lines[-7:]:
        print(ln, flush=True)
    torch.cuda.empty_cache()
if a.out:
    with open(a.out, "a") as f:
        f.write("".join(line + "\n" for line in lines))
