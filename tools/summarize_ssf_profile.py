#!/usr/bin/env python3
"""Per-launch-shape summary of the SSIM-family kernels (csrc/ssim_family.hip) from a rocprofv3 run of
tools/ssim_family_times.py: kernel_trace.csv -> microseconds per frame per (kernel, grid); with a counter_collection.csv of
a separate --pmc pass, the counters per frame and per wave of the same groups.
usage: summarize_ssf_profile.py KERNEL_TRACE.csv [COUNTER_COLLECTION.csv]"""
import collections, csv, re, sys

def short(name):
    m = re.search(r"(ssf_\w+|ext_nan_kernel)(<[^>]*>)?", name)
    return (m.group(1) + (m.group(2) or "")).replace("unsigned char", "u8").replace("unsigned short", "u16") if m else None

def main(trace, counters=None):
    g = collections.OrderedDict()
    with open(trace) as f:
        for r in csv.DictReader(f):
            k = short(r["Kernel_Name"])
            if not k:
                continue
            wg = int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"])
            frames = int(r["Grid_Size_Y"]) if k.startswith(("ssf_map", "ssf_down")) else int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"])
            key = (k, wg)
            e = g.setdefault(key, [0, 0, 0, r["VGPR_Count"], r["LDS_Block_Size"]])
            e[0] += int(r["End_Timestamp"]) - int(r["Start_Timestamp"]); e[1] += frames; e[2] += 1
    print(f"{'kernel':28s} {'WG/frame':>9s} {'launches':>8s} {'frames':>7s} {'us/frame':>9s}  VGPR  LDS")
    for (k, wg), (ns, fr, n, vg, lds) in g.items():
        print(f"{k:28s} {wg:9d} {n:8d} {fr:7d} {ns / 1e3 / max(fr, 1):9.2f}  {vg:>4s}  {lds}")
    if counters:
        c = collections.defaultdict(lambda: collections.defaultdict(float))
        with open(counters) as f:
            for r in csv.DictReader(f):
                k = short(r["Kernel_Name"])
                if k:
                    c[(k, int(r["Grid_Size"]) // int(r["Workgroup_Size"]))][r["Counter_Name"]] += float(r["Counter_Value"])
        print("\ncounters (summed over launches; per wave where noted)")
        for key, d in c.items():
            waves = d.get("SQ_WAVES", 0) or 1
            print(f"{key[0]:28s} grid {key[1]:8d}: waves {waves:10.0f}  VALU/wave {d.get('SQ_INSTS_VALU', 0) / waves:7.0f}  "
                  f"LDS/wave {d.get('SQ_INSTS_LDS', 0) / waves:6.0f}  VMEM_RD/wave {d.get('SQ_INSTS_VMEM_RD', 0) / waves:5.0f}  "
                  f"wait-inst/wave-cycle {d.get('SQ_WAIT_INST_ANY', 0) / max(d.get('SQ_WAVE_CYCLES', 1), 1):5.2f}  "
                  f"busy/GUI {d.get('SQ_BUSY_CYCLES', 0) / max(d.get('GRBM_GUI_ACTIVE', 1), 1):5.2f}")

if __name__ == "__main__":
    main(*sys.argv[1:3])
