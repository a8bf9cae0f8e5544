#!/usr/bin/env python3
"""Time per frame of the packed-format unpack (pqa_unpack_device, unpack.hip) on 8 resident frames of uniform noise at
1920x1080 and 3840x2160, UYVY and v210, three planes and luma only, beside two yardsticks taken in the same run: one
three-plane PSNR pass over the unpacked planes (the sse kernels of the same build, HIP events around a resident run, as
tools/flow_times.py takes it) and the traffic floor (packed bytes read + plane bytes written) / 8 TB/s.  The call is
synchronous (one launch for the 8 frames, ends in a stream synchronise), so a host clock around the call is the time: best,
median and worst of --rounds after a warm-up call.  Frame 0 is checked against the numpy unpack (tests/packed_ref.py).

Then the end-to-end leg with host clocks, on files in the page cache: score_files on a 4:2:2 Y4M pair against the same
reference with the capture as a packed file (10 bit: v210, 8 bit: UYVY) -- the packed file moves 8/3 instead of 4 bytes per
pixel over PCIe at 10 bit, and the same bytes at 8 bit.  A third leg repeats the packed run with both files held in anonymous
memory instead of a fresh file mapping (the cost of the mapping's page faults).  Best and worst of --e2e-rounds after a
warm-up run.
usage: python tools/unpack_times.py [--frames 8] [--rounds 7] [--e2e-frames 24] [--e2e-rounds 3] [--tmp DIR] [--out FILE]"""
import argparse, os, shutil, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from pqa2_amd import _native as N, pipeline, yuvio
from pqa2_amd.engine import FeatureEngine
from pqa2_amd.pipeline import score_files
from tests import packed_ref as PR

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=8)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--e2e-frames", type=int, default=24)
ap.add_argument("--e2e-rounds", type=int, default=3)
ap.add_argument("--tmp", default=None, help="directory for the end-to-end files (default: a temporary one under /dev/shm or the system's)")
ap.add_argument("--out", default=None, help="also append the result lines to this file")
a = ap.parse_args()
HBM_BYTES_PER_US = 8.0e6   # 8 TB/s
lines = []


def say(s):
    lines.append(s)
    print(s, flush=True)


def up16(v):
    return (v + 15) // 16 * 16


def unpack(fmt, w, h, n, luma_only):
    es, cw = np.dtype(PR.DTYPE[fmt]).itemsize, PR.chroma_width(w)
    pitch = up16(PR.min_row_bytes(fmt, w))
    gen = torch.Generator(device="cuda")
    gen.manual_seed(w + len(fmt))
    src = torch.randint(0, 256, (n, h, pitch), generator=gen, device="cuda", dtype=torch.int32).to(torch.uint8)
    dp = [up16(k * es) for k in (w, cw, cw)][:1 if luma_only else 3]
    dst = [torch.zeros((n, h, p), dtype=torch.uint8, device="cuda") for p in dp]
    torch.cuda.synchronize()
    with FeatureEngine(64, 64, bit_depth=PR.BIT_DEPTH[fmt]) as eng:
        args = (fmt, (h, w), src.data_ptr(), pitch, h * pitch, n, [d.data_ptr() for d in dst], dp, [h * p for p in dp])
        eng.unpack_resident(*args)   # warm-up: the code object
        us = []
        for _ in range(a.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.unpack_resident(*args)
            us.append((time.perf_counter() - t0) * 1e6 / n)
    want = PR.unpack(fmt, src[0].cpu().numpy(), w)
    for p, d in enumerate(dst):
        k = (w, cw, cw)[p]
        got = np.ascontiguousarray(d[0].cpu().numpy()[:, :k * es]).view(PR.DTYPE[fmt])
        assert np.array_equal(got, want[p]), (fmt, w, h, luma_only, p)
    traffic = h * (PR.min_row_bytes(fmt, w) + (w + (0 if luma_only else 2 * cw)) * es)
    return sorted(us), traffic / HBM_BYTES_PER_US


def psnr_three_planes(w, h, bpc, n):
    """one PSNR pass over 4:2:2 planes of the unpacked size: the project's usual yardstick"""
    es, cw = (1 if bpc == 8 else 2), (w + 1) // 2
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    mk = lambda k: torch.randint(0, 1 << bpc, (n, h, k), generator=gen, device="cuda", dtype=torch.int32).to(torch.uint8 if bpc == 8 else torch.int16)
    ref, dis = [mk(k) for k in (w, cw, cw)], [mk(k) for k in (w, cw, cw)]
    rp, fp = [w * es, cw * es, cw * es], [w * h * es, cw * h * es, cw * h * es]
    torch.cuda.synchronize()
    with FeatureEngine(w, h, bit_depth=bpc, n_planes=3, chroma_shift=(1, 0), features=N.FEAT_PSNR, result_capacity=max(16384, n)) as eng:
        run = lambda: eng.submit_resident(0, n, [t.data_ptr() for t in ref], [t.data_ptr() for t in dis], rp, fp)
        run()
        eng.sync()
        best = None
        for _ in range(a.rounds):
            eng.reset()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            run()
            eng.sync()
            t1.record()
            torch.cuda.synchronize()
            us = t0.elapsed_time(t1) * 1e3 / n
            best = us if best is None else min(best, us)
    return best


say(f"# unpack (pqa_unpack_device), {a.frames} resident frames, {a.rounds} rounds after a warm-up; host clock around the synchronous call")
for w, h in ((1920, 1080), (3840, 2160)):
    for fmt in ("uyvy422", "v210"):
        psnr = psnr_three_planes(w, h, PR.BIT_DEPTH[fmt], a.frames)
        for luma_only in (False, True):
            us, floor = unpack(fmt, w, h, a.frames, luma_only)
            say(f"{w}x{h} {fmt:8s} {'luma only   ' if luma_only else 'three planes'}: best {us[0]:7.2f} median {us[len(us) // 2]:7.2f} worst {us[-1]:7.2f} "
                f"us/frame; three-plane PSNR pass {psnr:7.2f} us/frame, ratio {us[0] / psnr:5.2f}; traffic floor {floor:6.2f} us, "
                f"ratio {us[0] / floor:6.2f}")
        torch.cuda.empty_cache()

# ---- end to end: files in the page cache, host clocks around score_files ---------------------------------------------------
tmp_root = a.tmp or tempfile.mkdtemp(prefix="pqa_unpack_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
os.makedirs(tmp_root, exist_ok=True)
say(f"# end to end: score_files (VMAF + PSNR + SSIM on three planes), {a.e2e_frames} frames, {a.e2e_rounds} rounds after a warm-up run; files in the page cache")
try:
    for w, h in ((1920, 1080), (3840, 2160)):
        for fmt, tag in (("v210", "422p10"), ("uyvy422", "422")):
            bpc = PR.BIT_DEPTH[fmt]
            rng = np.random.default_rng(w + bpc)
            # a few distinct noise frames, cycled: the clocks do not care and the files are written quickly
            base = [PR.random_planes(fmt, w, h, seed=i, extremes=False) for i in range(4)]
            noisy = [[np.clip(p.astype(np.int32) + rng.integers(-3, 4, p.shape), 0, (1 << bpc) - 1).astype(p.dtype) for p in f] for f in base]
            info = yuvio.VideoInfo(w, h, bpc, 1, 0, False, 30, 1, 0, tag)
            ref, dis = os.path.join(tmp_root, "ref.y4m"), os.path.join(tmp_root, "dis.y4m")
            cap = os.path.join(tmp_root, f"cap_{w}x{h}" + (".v210" if fmt == "v210" else ".uyvy"))
            yuvio.write_y4m(ref, (base[i % 4] for i in range(a.e2e_frames)), info)
            yuvio.write_y4m(dis, (noisy[i % 4] for i in range(a.e2e_frames)), info)
            packed = [PR.pack(fmt, *f, stride=PR.file_stride(fmt, w)).tobytes() for f in noisy]
            with open(cap, "wb") as f:
                for i in range(a.e2e_frames):
                    f.write(packed[i % 4])
            res = {}
            for name, d in (("planar Y4M", dis), ("packed file", cap), ("packed, present", cap)):
                # the third leg: the same run with both readers' file mappings replaced by arrays in anonymous memory, read
                # outside the clock -- what the page faults of a fresh mapping cost the copy into pinned memory
                present = {}

                def opener(path, _real=yuvio.open_video, **kw):
                    rd = _real(path, **kw)
                    if path not in present:
                        present[path] = np.fromfile(path, np.uint8)
                    rd._mm = present[path]
                    return rd
                pipeline.open_video = opener if name == "packed, present" else yuvio.open_video
                score_files(ref, d)   # warm-up: contexts, page cache
                ts = []
                for _ in range(a.e2e_rounds):
                    t0 = time.perf_counter()
                    r = score_files(ref, d)
                    ts.append(time.perf_counter() - t0)
                res[name] = (sorted(ts), r)
            pipeline.open_video = yuvio.open_video
            assert np.array_equal(res["planar Y4M"][1]["records"].view(np.uint64), res["packed file"][1]["records"].view(np.uint64))
            assert res["packed file"][1]["input"]["packed_upload"]
            (tp, _), (tk, _) = res["planar Y4M"], res["packed file"]
            say(f"{w}x{h} {bpc:2d}-bit 4:2:2: planar Y4M pair best {a.e2e_frames / tp[0]:7.1f} worst {a.e2e_frames / tp[-1]:7.1f} frames/s; "
                f"Y4M reference + {fmt} capture best {a.e2e_frames / tk[0]:7.1f} worst {a.e2e_frames / tk[-1]:7.1f} frames/s; "
                f"ratio of the bests {tp[0] / tk[0]:5.2f}; bytes per frame pair over PCIe {2 * info.frame_bytes} vs "
                f"{info.frame_bytes + PR.min_row_bytes(fmt, w) * h}; records bit-identical; the packed route with both files in "
                f"anonymous memory instead of a mapping: best {a.e2e_frames / res['packed, present'][0][0]:7.1f} worst "
                f"{a.e2e_frames / res['packed, present'][0][-1]:7.1f} frames/s")
            for p in (ref, dis, cap):
                os.remove(p)
finally:
    if not a.tmp:
        shutil.rmtree(tmp_root, ignore_errors=True)
if a.out:
    with open(a.out, "a") as f:
        f.write("".join(line + "\n" for line in lines))
