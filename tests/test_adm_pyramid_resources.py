"""adm_pyramid_kernel (ADM scales 0 and 1 in one launch, adm_pyramid.hip) keeps three waves per SIMD: the compiler's own figures.

The kernel sits right under the 168-VGPR line (512 / 3 waves per SIMD, 8-register granules) -- its per-lane double sums live
in LDS for that reason -- and one more live value in the march costs either the third wave (two waves measured 5 % slower) or
scratch.  The dependency-cone bounds (adm_need.h) are wave-uniform and must stay in scalar registers.  Both instances (8-bit
and 16-bit samples) are checked; hipcc cross-compiles without a GPU; built with the flags build.sh uses for this file."""
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


def test_pyramid_kernels_fit_three_waves_per_simd_without_scratch(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "pqa2_amd", "csrc", "adm_pyramid.hip")
    out = tmp_path / "adm_pyramid.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-slp-vectorize", "-S", "--cuda-device-only", src,
                    "-o", str(out)], check=True, capture_output=True)
    text = out.read_text()
    k = {n: v for n, v in _kernels(text).items() if "adm_pyramid_kernel" in n}
    # <uint8_t> and <uint16_t> as the Itanium ABI spells the template argument
    for targ in ("IhE", "ItE"):
        inst = [v for n, v in k.items() if "adm_pyramid_kernel" + targ in n]
        assert len(inst) == 1, (targ, sorted(k))
        r = inst[0]
        print(f"adm_pyramid_kernel{targ}: {r}")
        assert r["scratch"] == 0, (targ, r)
        assert r["vgprs"] <= 168, (targ, r)
        assert r["occupancy"] >= 3, (targ, r)
        # three workgroups of four waves per CU must fit the 160 KB of LDS as well
        assert 3 * r["lds"] <= 160 * 1024, (targ, r)
    assert len(k) == 2   # every instance was looked at
    assert "Folded Reload" not in text and "Folded Spill" not in text
