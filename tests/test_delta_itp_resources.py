"""delta_itp_kernel (csrc/delta_itp.hip) is issue-bound: 61 transcendentals per pixel pair on the PQ path.  A spilled constant
puts a scratch load between them (the comment at the head of ciede.hip tells how that happens: unrolled shift-2 pixel loops, a
loop over chroma rows), so every instance -- two sample types, nine chroma layouts, three transfers -- must run without
scratch and without spills; LDS holds the reduction only.  The compiler's own figures; hipcc cross-compiles without a GPU;
built with the flags build.sh uses for this file."""
import os
import re
import shutil
import subprocess

import pytest

from tests.test_adm_pyramid_resources import _kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_instance_runs_without_scratch(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "pqa2_amd", "csrc", "delta_itp.hip")
    out = tmp_path / "delta_itp.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", src, "-o", str(out)],
                   check=True, capture_output=True)
    text = out.read_text()
    k = {n: v for n, v in _kernels(text).items() if "delta_itp_kernel" in n}
    seen = set()
    for name, r in sorted(k.items()):
        # <T, HS, VS, TR> as the Itanium ABI spells the template arguments: h / t, then three Li<n>E
        m = re.search(r"delta_itp_kernelI([ht])Li(\d)ELi(\d)ELi(\d)EE", name)
        assert m, name
        seen.add(m.groups())
        print(f"delta_itp_kernel<{'u8' if m.group(1) == 'h' else 'u16'}, {m.group(2)}, {m.group(3)}, transfer {m.group(4)}>: "
              f"{r['vgprs']} VGPRs, occupancy {r['occupancy']}, LDS {r['lds']}")
        assert r["scratch"] == 0, (name, r)
        assert r["lds"] <= 256, (name, r)          # 20 doubles, 4 floats and 8 ints of the tile reduction
        assert r["occupancy"] >= 4, (name, r)      # latency hiding for an issue-bound kernel; measured 8
    assert seen == {(t, str(hs), str(vs), str(tr)) for t in "ht" for hs in range(3) for vs in range(3) for tr in range(3)}
    for n, v in _kernels(text).items():
        assert v["scratch"] == 0, (n, v)           # the finalize and debug kernels too
    assert "Folded Reload" not in text and "Folded Spill" not in text
