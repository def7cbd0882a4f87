"""No GPU: the schedule choice (csrc/schedule_plan.hpp: plan_schedule -- the one function every entry of the library asks which schedule
factors a matrix) gives the expected plan for a table of calls and keeps its invariants over a grid of shapes, element types, block widths,
tunings and handle states.  The checker is host C++ (tests/schedule_plan_check.cpp), compiled here with g++ against the HIP headers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None or not os.path.isdir("/opt/rocm/include"), reason="needs g++ and the HIP headers")
def test_schedule_plan_table_and_invariants(tmp_path):
    exe = str(tmp_path / "schedule_plan_check")
    cmd = ["g++", "-std=c++17", "-O1", "-w", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "recursivefactorization.jl_amd", "csrc"),
           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "schedule_plan_check.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    assert " 0 violations" in r.stdout
