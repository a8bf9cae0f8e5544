"""vif_strip_kernel (VIF scales 1-3, vif.hip) keeps vif_stat_kernel's occupancy: the compiler's own figures.

The strip kernel carries the vertical window of the tile below in a second set of accumulators (40 VGPRs at scale 1) and the
next step's rows in flight across vif_hstat.  That only pays while three workgroups still fit a CU, which the LDS allows
(3 x 49.6 KB of 160 KB) and the registers must too: at most 168 VGPRs (512 / 3 waves per SIMD, 8-register granules), no
scratch -- a spilled accumulator is reloaded behind an s_waitcnt vmcnt(0) that also waits for the prefetch -- and not a byte of
LDS more than the tiled kernel of the same scale.  hipcc cross-compiles without a GPU; built with the flags build.sh uses."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _kernels(text):
    """mangled name -> {vgprs, scratch, lds, occupancy} from the resource comments behind each kernel"""
    out = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)^; Occupancy: (\d+)", text, re.S | re.M):
        body = m.group(2)
        out[m.group(1)] = {
            "vgprs": int(re.search(r"^; TotalNumVgprs: (\d+)", body, re.M).group(1)),
            "scratch": int(re.search(r"^; ScratchSize: (\d+)", body, re.M).group(1)),
            "lds": int(re.search(r"^; LDSByteSize: (\d+)", body, re.M).group(1)),
            "occupancy": int(m.group(3)),
        }
    return out


def test_strip_kernels_fit_three_waves_per_simd_without_scratch(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "pqa2_amd", "csrc", "vif.hip")
    out = tmp_path / "vif.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", src, "-o", str(out)],
                   check=True, capture_output=True)
    text = out.read_text()
    k = _kernels(text)
    # <N, TW, ND> of scales 1, 2, 3 as the Itanium ABI spells the template arguments
    inst = {1: "ILi9ELi248ELi5EE", 2: "ILi5ELi252ELi3EE", 3: "ILi3ELi252ELi0EE"}
    seen = 0
    for scale, targs in inst.items():
        strip = [v for n, v in k.items() if "vif_strip_kernel" + targs in n]
        tiled = [v for n, v in k.items() if "vif_stat_kernelIf" + targs[1:] in n]   # <float, N, TW, ND>
        assert len(strip) == 1 and len(tiled) == 1, (scale, sorted(k))
        s, t = strip[0], tiled[0]
        print(f"scale {scale}: strip {s}  tiled {t}")
        assert s["scratch"] == 0, (scale, s)
        assert s["vgprs"] <= 168, (scale, s)
        assert s["lds"] <= t["lds"], (scale, s, t)
        assert s["occupancy"] >= t["occupancy"] == 3, (scale, s, t)
        seen += 1
    assert seen == 3 and sum("vif_strip_kernel" in n for n in k) == 3   # every strip instance was looked at
    assert "Folded Reload" not in text and "Folded Spill" not in text
