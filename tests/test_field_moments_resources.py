"""field_moments_kernel (csrc/field_moments.hip) holds eight packed quads and 22 raw sums a lane and hides the latency of its
eight row loads behind other waves: every instance -- two sample types, three load widths -- must run without scratch and
without spills at four waves a SIMD or more.  The compiler's own figures; hipcc cross-compiles without a GPU; built with the
flags build.sh uses for this file."""
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
    src = os.path.join(ROOT, "pqa2_amd", "csrc", "field_moments.hip")
    out = tmp_path / "field_moments.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", src, "-o", str(out)],
                   check=True, capture_output=True)
    text = out.read_text()
    k = {n: v for n, v in _kernels(text).items() if "field_moments_kernel" in n}
    seen = set()
    for name, r in sorted(k.items()):
        # <T, VB> as the Itanium ABI spells the template arguments: h / t, then Li<n>E
        m = re.search(r"field_moments_kernelI([ht])Li(\d+)EE", name)
        assert m, name
        seen.add((m.group(1), int(m.group(2))))
        print(f"field_moments_kernel<{'u8' if m.group(1) == 'h' else 'u16'}, {m.group(2)}>: {r['vgprs']} VGPRs, "
              f"occupancy {r['occupancy']}, LDS {r['lds']}")
        assert r["scratch"] == 0, (name, r)
        assert r["occupancy"] >= 4, (name, r)
        assert r["lds"] <= 128, (name, r)      # the 14 words of the workgroup
    assert seen == {("h", 16), ("h", 4), ("h", 1), ("t", 16), ("t", 4), ("t", 2)}
    assert "Folded Reload" not in text and "Folded Spill" not in text
