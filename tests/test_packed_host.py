"""AddressSanitizer + UBSan over the host code of the packed capture formats (pqa2_amd/csrc/host_packed.h: row geometry, the
copy of a caller's packed or planar frames into staging, the copy of unpacked planes back out), driven on the CPU by
tests/packed_harness.cpp from heap blocks of exactly the bytes the contract lets the library touch.  A stand-alone program:
nothing is loaded into Python.  Memory safety only -- the samples themselves are tests/test_gpu_packed.py's."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "packed_harness.cpp")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_packed_host_code_is_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "packed_harness")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-pthread", "-Wall", "-Wextra",
                        "-o", exe, SRC], capture_output=True, text=True, timeout=300)
    if r.returncode != 0 and ("cannot find" in r.stderr or "unrecognized" in r.stderr):
        pytest.skip(f"g++ has no -fsanitize=address,undefined runtime here: {r.stderr[-200:]}")
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    # the sanitizer must be alive: it has to flag a staging buffer that is one byte short ...
    bad = subprocess.run([exe, "--selftest", "overflow"], capture_output=True, text=True, timeout=120, env=env)
    assert bad.returncode != 0 and "heap-buffer-overflow" in bad.stderr, (bad.returncode, bad.stderr[-500:])
    # ... and find nothing in the real code
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "packed harness ok" in r.stdout, (r.returncode, r.stdout[-300:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
