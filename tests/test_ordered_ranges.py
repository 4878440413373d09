"""The range loop of the ordered splat films (bling_amd/csrc/core/ordered_ranges.h: ascending photon ranges, a
range that overflows its record buffer run again into a larger one or, past the budget, as two halves), which
the light tracer's and SPPM's ordered passes share and which includes nothing of HIP.  Builds
tests/cpp/ordered_ranges_check.cpp with g++: the full launch and accept sequences of hand-derived scripts, the
single photon past the budget (refused, with its index and the budget in the text), a capacity carried from
one sequence to the next, and the cover / order / capacity properties over seeded random scripts.  CPU only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_ordered_ranges(tmp_path):
    exe = tmp_path / "ordered_ranges_check"
    src = os.path.join(ROOT, "tests", "cpp", "ordered_ranges_check.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", str(exe), src], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ordered_ranges: 0 checks failed" in r.stdout
