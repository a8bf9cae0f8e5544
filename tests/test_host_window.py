"""host::window_walk (pqa2_amd/csrc/host_stage.h), the staging walk of the deinterlacer's host entry, driven on the CPU by fake
callables (tests/window_harness.cpp): frame counts around the chunk, every frame packed once, every output emitted once and in
order, a failing callable stops the walk, caller rows that end at the end of their allocation.  A stand-alone program built
under AddressSanitizer + UBSan and under ThreadSanitizer and run directly.  Memory safety and bookkeeping only -- nothing here
is a parity claim."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "window_harness.cpp")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.parametrize("san", ["address,undefined", "thread"])
def test_window_walk_is_clean_under(tmp_path, san):
    exe = str(tmp_path / f"window_harness_{san.replace(',', '_')}")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", f"-fsanitize={san}", "-fno-omit-frame-pointer", "-pthread",
                        "-Wall", "-Wextra", "-o", exe, SRC], capture_output=True, text=True, timeout=300)
    if r.returncode != 0 and ("cannot find" in r.stderr or "unrecognized" in r.stderr):
        pytest.skip(f"g++ has no -fsanitize={san} runtime here: {r.stderr[-200:]}")
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1 exitcode=66", ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "window harness ok" in r.stdout, (r.returncode, r.stdout[-300:], r.stderr[-3000:])
    assert "WARNING: ThreadSanitizer" not in r.stderr and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
