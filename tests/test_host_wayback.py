"""No GPU: the two pure pieces of the host entry's way back (csrc/host_wayback.hpp): the chunk plan -- pieces in order, disjoint, covering
[0, m), none larger than a bounce buffer, one block column at a time near the end -- over a grid of shapes, chunk sizes and block widths,
and the threaded column scatter -- every element exactly where it belongs, the padding untouched -- below and above the single-thread
threshold, for thread counts that do not divide the columns or exceed them.  The checker is host C++ (tests/host_wayback_check.cpp),
compiled here with g++; the header needs no HIP."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_chunk_plan_and_scatter(tmp_path):
    exe = str(tmp_path / "host_wayback_check")
    cmd = ["g++", "-std=c++17", "-O1", "-w", "-pthread", "-I" + os.path.join(ROOT, "recursivefactorization.jl_amd", "csrc"),
           os.path.join(ROOT, "tests", "host_wayback_check.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    assert " 0 violations" in r.stdout
