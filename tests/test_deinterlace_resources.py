"""deinterlace_kernel (csrc/deinterlace.hip) keeps a window of 18 pieces of 16 bytes a lane (72 VGPRs) plus the five of the next
step and hides the latency of its loads behind other waves: every instance -- two sample types, three load widths, two
modes -- must run without scratch, without spills and without LDS at four waves a SIMD or more.  The compiler's own figures;
hipcc cross-compiles without a GPU; built with the flags build.sh uses for this file."""
import os
import re
import shutil
import subprocess

import pytest

from tests.test_adm_pyramid_resources import _kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_instance_runs_without_scratch_at_four_waves(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "pqa2_amd", "csrc", "deinterlace.hip")
    out = tmp_path / "deinterlace.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", src, "-o", str(out)],
                   check=True, capture_output=True)
    text = out.read_text()
    k = {n: v for n, v in _kernels(text).items() if "deinterlace_kernel" in n}
    seen = set()
    for name, r in sorted(k.items()):
        # <T, VB, MODE> as the Itanium ABI spells the template arguments: h / t, then Li<n>E twice
        m = re.search(r"deinterlace_kernelI([ht])Li(\d+)ELi(\d+)EE", name)
        assert m, name
        seen.add((m.group(1), int(m.group(2)), int(m.group(3))))
        print(f"deinterlace_kernel<{'u8' if m.group(1) == 'h' else 'u16'}, {m.group(2)}, {'intra' if m.group(3) == '0' else 'adaptive'}>: "
              f"{r['vgprs']} VGPRs, occupancy {r['occupancy']}, LDS {r['lds']}")
        assert r["scratch"] == 0, (name, r)
        assert r["occupancy"] >= 4, (name, r)
        assert r["lds"] == 0, (name, r)
    assert seen == {(t, vb, mode) for t, vbs in (("h", (16, 4, 1)), ("t", (16, 4, 2))) for vb in vbs for mode in (0, 1)}
    assert "Folded Reload" not in text and "Folded Spill" not in text
