"""The pass driver's integer arithmetic (bling_amd/csrc/core/pass_plan.h: wave sizing, the half-wave cut,
the greedy tile batching) and the bling_stats field table with its two folds (pass_stats.h), neither of
which includes anything of HIP.  Builds tests/cpp/pass_plan_check.cpp with g++: hand-derived cases,
properties over random tile lists, a tile larger than the chunk (refused), and both folds field by
field.  CPU only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_pass_plan_and_stats_table(tmp_path):
    exe = tmp_path / "pass_plan_check"
    src = os.path.join(ROOT, "tests", "cpp", "pass_plan_check.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", str(exe), src], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "pass_plan: 0 checks failed" in r.stdout
