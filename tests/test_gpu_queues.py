"""The schedules' streams must sit on different hardware pipes whatever queues the host program created before (driver.cpp:
validate_queues).  RFLU_DUMMY_QUEUES=k reproduces the histories in which the update or the side stream would share the critical
path's pipe (k = 1, 2 in a process that starts like this one): the check has to notice it, replace the stream, and the factorization
has to run as fast as with a clean history (a shared pipe costs +65 % at n = 4096)."""
import os, re, subprocess, sys
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.gpu_exclusive]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCRIPT = r"""
import time, torch
import recursivefactorization.jl_amd as rf
n = 4096
A = torch.rand((n, n), dtype=torch.float64, device="cuda").T.contiguous().T
best = 1e9
for i in range(6):
    W = A.clone(); torch.cuda.synchronize(); t0 = time.perf_counter()
    F = rf.lu_(W, None, True, check=False); torch.cuda.synchronize()
    best = min(best, time.perf_counter() - t0)
assert F.info == 0 and rf.last_path() == "hip-lookahead"
print("BEST_MS %.3f" % (best * 1e3))
"""


def _run(k, check=True):
    env = dict(os.environ, RFLU_DUMMY_QUEUES=str(k), RFLU_QUEUE_TRACE="1", PYTHONPATH=ROOT)
    if not check:
        env["RFLU_QUEUE_CHECK"] = "0"
    p = subprocess.run([sys.executable, "-c", SCRIPT], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    ms = float(re.search(r"BEST_MS ([0-9.]+)", p.stdout).group(1))
    checks = [(m.group(1), int(m.group(2)), float(m.group(3)), float(m.group(4)))
              for m in re.finditer(r"queue check (\w+\[\d\]) attempt (\d+): ([0-9.]+) us per kernel.*\(alone ([0-9.]+)\)", p.stderr)]
    return ms, checks


def test_streams_end_up_on_different_pipes_whatever_the_queue_history():
    base_ms, base_checks = _run(0)
    assert base_checks, "the queue check did not run"
    replaced = 0
    for k in (1, 2, 3):
        ms, checks = _run(k)
        last = {}
        for name, attempt, us, alone in checks:
            last[name] = (us, alone)
            replaced += attempt > 0
        for name, (us, alone) in last.items():   # what was finally accepted drains like independent queues do (~2 us; one pipe: ~28)
            assert us <= max(2.0 * alone, alone + 5.0), (k, name, us, alone, checks)
        if ms >= 1.4 * base_ms:                  # wall-clock on a shared box: one second opinion before calling it the slow pattern
            ms = min(ms, _run(k)[0])
        assert ms < 1.4 * base_ms, (k, ms, base_ms, checks)
    assert replaced >= 1, "none of the three histories put a stream on the critical path's pipe: the test no longer tests anything"


ALTERNATE = r"""
import torch
import recursivefactorization.jl_amd as rf
n = 2048
A = torch.rand((n, n), dtype=torch.float64, device="cuda").T.contiguous().T
s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
for i in range(8):
    with torch.cuda.stream(s1 if i % 2 == 0 else s2):
        W = A.clone()
        F = rf.lu_(W, None, True, check=False)
        assert F.info == 0
torch.cuda.synchronize()
print("DONE")
"""


def test_alternating_caller_streams_are_checked_once_each():
    """The placement is cached per caller stream: a program that alternates between two streams pays for two checks (three if the
    second one forced a replacement), not for one per call."""
    env = dict(os.environ, RFLU_QUEUE_TRACE="1", PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, "-c", ALTERNATE], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0 and "DONE" in p.stdout, p.stderr[-2000:]
    rounds = len(re.findall(r"queue check ustream\[1\] attempt 0", p.stderr))
    assert 1 <= rounds <= 3, (rounds, p.stderr[-3000:])
