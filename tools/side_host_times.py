#!/usr/bin/env python3
"""Time of the host-frame entries of the side analyses that work on planes of the context's size, at 1920 x 1080 and
3840 x 2160, 8 bit: pqa_luma_stats on 64 frames (the bookend detector's call size), pqa_shift_sse on 8 pairs (R = 8),
pqa_level_stats on 8 pairs, pqa_cross_sse on 64 / 64 frames (-8 ... 8), pqa_frame_sad on 8 frames of three planes, and
pqa_tile_moments on 16 pairs as the witness of the entries for planes of the call's own size.  Every call is synchronous (it
packs the caller's frames into pinned memory, uploads, launches and ends in a stream synchronise), so a host clock around the
call is the time; per case the median and min ... max of --rounds calls after a warm-up call (code objects, the buffers of
first use).  --lib loads another build of the library (an A/B partner); run the two alternately, one process a run.
usage: python tools/side_host_times.py [--lib FILE] [--rounds 5] [--out FILE]"""
import argparse, os, statistics, sys, time

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=None, help="the shared object to load (default: the one in the tree)")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=None, help="also append the result lines to this file")
a = ap.parse_args()
if a.lib:
    os.environ["PQA_LIB_PATH"] = os.path.abspath(a.lib)   # read when pqa2_amd._native is imported
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from pqa2_amd import _native as N
from pqa2_amd.engine import FeatureEngine


def frames(rng, n, h, w):
    """n different planes, cheaply: one random plane, rolled and offset (the entries' time does not depend on the samples)"""
    base = rng.integers(0, 256, (h, w), dtype=np.uint8)
    return [np.ascontiguousarray(np.roll(base, 3 * i + 1, axis=1) + np.uint8(i)) for i in range(n)]


lines = []
for w, h in ((1920, 1080), (3840, 2160)):
    rng = np.random.default_rng(w)
    ref, dis = frames(rng, 64, h, w), frames(rng, 64, h, w)
    ch, cw = h // 2, w // 2
    three = [[dis[i], c, c] for i, c in enumerate(frames(rng, 9, ch, cw))]
    with FeatureEngine(w, h, n_planes=3, chroma_shift=(1, 1), features=N.FEAT_PSNR | N.FEAT_INTEGRITY, max_batch=8,
                       result_capacity=16) as eng:
        cases = (("luma_stats 64", lambda: eng.luma_stats(dis, 120)),
                 ("shift_sse 8 R=8", lambda: eng.shift_sse(ref[:8], dis[:8], 8)),
                 ("level_stats 8", lambda: eng.level_stats(ref[:8], dis[:8])),
                 ("cross_sse 64/64 -8..8", lambda: eng.cross_sse(ref, dis, -8, 8)),
                 ("frame_sad 8x3", lambda: eng.frame_sad(three[8], three[:8])),
                 ("tile_moments 16", lambda: eng.tile_moments(ref[:16], dis[:16])))
        for name, call in cases:
            call()
            ms = []
            for _ in range(a.rounds):
                t0 = time.perf_counter()
                call()
                ms.append((time.perf_counter() - t0) * 1e3)
            lines.append(f"{w}x{h} {name}: median {statistics.median(ms):9.3f} ms (min {min(ms):9.3f} ... max {max(ms):9.3f}) of {a.rounds} calls")
            print(lines[-1], flush=True)
    del ref, dis, three
if a.out:
    with open(a.out, "a") as f:
        f.write("".join(line + "\n" for line in lines))
