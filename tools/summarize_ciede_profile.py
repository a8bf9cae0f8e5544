#!/usr/bin/env python3
"""Per-frame time of the ciede2000 kernels from one rocprofv3 --kernel-trace --stats run of tools/ciede_times.py (rocpd SQLite
output): one line per kernel instance and grid.  The grid tells the geometry (ciede_kernel: one 256-thread workgroup per 64 x 4
chroma tile, frames on grid y; ciede_finalize_kernel: one workgroup per frame), the template argument the sample type.
usage: python tools/summarize_ciede_profile.py results.db"""
import collections, sqlite3, sys

con = sqlite3.connect(sys.argv[1])
rows = con.execute("select name, grid_x, grid_y, workgroup_x, duration, scratch_size from kernels where name like '%ciede%'")
agg = collections.defaultdict(lambda: [0, 0, 0])
for name, gx, gy, wg, dur, scr in rows:
    short = name.replace("void ", "").replace("pqa::(anonymous namespace)::", "")
    short = short[:short.rindex("(")]
    frames = gx // wg if "finalize" in short else gy
    a = agg[(short, gx, scr)]
    a[0] += 1
    a[1] += frames
    a[2] += dur
print(f"{'kernel':44s} {'grid_x':>9s} {'launches':>8s} {'frames':>7s} {'us/launch':>10s} {'us/frame':>9s} {'scratch':>8s}")
for (short, gx, scr), (n, fr, ns) in sorted(agg.items(), key=lambda kv: -kv[1][2]):
    print(f"{short:44s} {gx:9d} {n:8d} {fr:7d} {ns / n / 1e3:10.2f} {ns / max(1, fr) / 1e3:9.2f} {scr:8d}")
