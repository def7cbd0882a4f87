"""Mixed-precision solve (rflu_mixed_getrf_f64_dev / rflu_mixed_getrs_f64_dev) against the Float64 path, its two streaming kernels alone,
and the crossover between residual_few and the GEMM residual.

    microbench_mixed.py [--n 4096 8192 16384 32768] [--nrhs 1 64] [--reps 5] [--sweep-n 16384] [--out profiles/mixed_sizes.txt]

Per N and nrhs, on the uniform[0,1) matrix of the benchmark (rflu_fill_uniform_f64_dev, seed 12) and uniform right-hand sides:
  mixed    lu_mixed + ldiv_mixed(fallback=False): demote + Float32 factorization + refinement to dsgesv's rule, with its step count;
  float64  lu_ + ldiv_ on a copy of the matrix (the copy is outside the timed window).  Neither entry is touched by the mixed path, so
           this is the Float64 path as it was before the mixed one existed.
The two alternate in one process; each is a host clock around calls that end in a stream synchronisation; the median over --reps after
one warm-up round is reported, with the ratio float64 / mixed (above 1: mixed wins).  The refined solution is checked against the
per-column rule with a Float64 product computed by torch before a time is printed.
Kernel times: the library's synchronous per-launch timers (rflu_profile_enable(1), events around every launch) in a run of their own:
demote_relayout is the only layout-change launch of rflu_mixed_getrf_f64_dev, residual_few the only launch of its class in
rflu_residual_f64_dev; GB/s = the algorithmic bytes (12 n^2 and 8 n^2) over that time.
Crossover: rflu_residual_f64_dev at --sweep-n for a range of right-hand-side counts, once with RFLU_MIXED_GEMV_MAX_RHS so large that
residual_few serves all of them (passes of 8) and once with 0 (the Float64 GEMM on the transposed views).
No GPU, no numbers: the script fails."""
import argparse
import ctypes
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import recursivefactorization.jl_amd as rf
from recursivefactorization.jl_amd import _ffi

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, nargs="+", default=[4096, 8192, 16384, 32768])
ap.add_argument("--nrhs", type=int, nargs="+", default=[1, 64])
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--sweep-n", type=int, default=16384)
ap.add_argument("--sweep-nrhs", type=int, nargs="+", default=[1, 4, 8, 9, 12, 16, 17, 24, 32, 48, 64])
ap.add_argument("--out", default=None, help="also write the table to this file")
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("microbench_mixed.py measures an MI355X; no GPU is visible")

EPS = float(np.finfo(np.float64).eps)
h = _ffi.default_handle(0)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def uniform_cm(n, k, seed):
    t = torch.empty((k, n), dtype=torch.float64, device="cuda:0").T   # n x k, column-major
    h.set_stream(None)
    h.call("rflu_fill_uniform_f64_dev", ptr(t), n, k, n, 0, seed, n, 0, 0, 0.0)
    return t


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def kernel_ms(name, fn):
    """time and launches of kernel class `name` inside fn() under the synchronous timers"""
    h.profile_enable(1)
    try:
        fn()
        p = h.profile()[name]
    finally:
        h.profile_enable(0)
    return p["ms"], p["launches"]


say(f"scripts/microbench_mixed.py  (uniform[0,1) matrix, seed 12; median of {args.reps} alternating runs after one warm-up; "
    f"device {torch.cuda.get_device_name(0)}; RFLU_MIXED_GEMV_MAX_RHS = {os.environ.get('RFLU_MIXED_GEMV_MAX_RHS', 'default')})")
say(f"{'N':>6s}{'nrhs':>5s} | {'mixed ms':>9s}{'(lu_mixed':>10s}{'ldiv_mixed)':>12s}{'iters':>6s} | {'float64 ms':>10s}{'(lu_':>9s}{'ldiv_)':>8s} | "
    f"{'f64/mixed':>9s} | worst ||r||/rule")
for n in args.n:
    A = uniform_cm(n, n, 12)
    W = torch.empty_like(A.T).T          # the Float64 path factors in place: its copy of A
    assert W.stride() == A.stride()
    for nrhs in args.nrhs:
        B = uniform_cm(n, nrhs, 13)
        tm, tf = [], []
        for rep in range(args.reps + 1):
            def mixed():
                t_lu, F = wall_ms(lambda: rf.lu_mixed(A))
                t_sv, X = wall_ms(lambda: rf.ldiv_mixed(F, B, fallback=False))
                return t_lu, t_sv, F, X

            def float64():
                W.copy_(A)
                t_lu, F = wall_ms(lambda: rf.lu_(W, None, True))
                X = B.clone()
                t_sv, _ = wall_ms(lambda: rf.ldiv_(F, X))
                return t_lu, t_sv, F, X

            m, f = mixed(), float64()
            if rep == 0:   # the check, once: dsgesv's rule on the refined solution, recomputed with a Float64 product
                Fm, X = m[2], m[3]
                R = B - A @ X
                rule = X.abs().amax(dim=0) * Fm.anorm * EPS * float(np.sqrt(n))
                worst = float((R.abs().amax(dim=0) / rule).max().item())
                assert Fm.iters >= 0 and worst <= 1.0, (Fm.iters, worst)
                iters = Fm.iters
                del R
                continue
            assert m[2].iters == iters
            tm.append(m[:2])
            tf.append(f[:2])
            del m, f
        tm, tf = np.median(np.array(tm), axis=0), np.median(np.array(tf), axis=0)
        say(f"{n:6d}{nrhs:5d} | {tm.sum():9.2f}{tm[0]:10.2f}{tm[1]:12.2f}{iters:6d} | {tf.sum():10.2f}{tf[0]:9.2f}{tf[1]:8.2f} | "
            f"{tf.sum() / tm.sum():9.3f} | {worst:.3f}")
        del B
    # the two streaming kernels alone (a run of their own under the per-launch timers)
    F32 = torch.empty((n, n), dtype=torch.float32, device="cuda:0")
    ipiv = torch.empty(n, dtype=torch.int64, device="cuda:0")
    info, anorm = ctypes.c_int64(0), ctypes.c_double(0.0)
    h.set_stream(None)
    ms_d, k_d = kernel_ms("transpose", lambda: h.call("rflu_mixed_getrf_f64_dev", n, ptr(A), n, ptr(F32), n, ptr(ipiv), 1, 0,
                                                      ctypes.byref(anorm), ctypes.byref(info)))
    X1, B1 = uniform_cm(n, 8, 14), uniform_cm(n, 8, 15)
    R1 = torch.empty_like(B1.T).T
    os.environ["RFLU_MIXED_GEMV_MAX_RHS"] = "1000000"
    h.reload_tuning()
    res = []
    for k in (1, 8):
        call = lambda: h.call("rflu_residual_f64_dev", n, k, ptr(A), n, ptr(X1), n, ptr(B1), n, ptr(R1), n)
        call()
        ms_r, k_r = kernel_ms("misc", call)
        res.append(f"residual_few nrhs={k}: {ms_r:.3f} ms = {8.0 * n * n / ms_r / 1e9:.2f} TB/s" + ("" if k_r == 1 else f" ({k_r} launches)"))
    os.environ.pop("RFLU_MIXED_GEMV_MAX_RHS")
    h.reload_tuning()
    say(f"{n:6d} kernels alone | demote_relayout: {ms_d:.3f} ms = {12.0 * n * n / ms_d / 1e9:.2f} TB/s (12 n^2 bytes{'' if k_d == 1 else f', {k_d} launches'}) | " + " | ".join(res) + " (8 n^2 bytes)")
    del A, W, F32, X1, B1, R1

# ---- crossover: residual_few in passes of 8 against the Float64 GEMM on the transposed views
n = args.sweep_n
A = uniform_cm(n, n, 12)
kmax = max(args.sweep_nrhs)
X1, B1 = uniform_cm(n, kmax, 14), uniform_cm(n, kmax, 15)
R1 = torch.empty_like(B1.T).T
h.set_stream(None)
say(f"crossover sweep at N = {n}: rflu_residual_f64_dev, median of {args.reps} event-timed calls, ms")
say(f"{'nrhs':>6s}{'residual_few':>14s}{'gemm':>10s}")
stream = torch.cuda.current_stream()
h.set_stream(stream.cuda_stream)
table = {}
for mode, value in (("few", "1000000"), ("gemm", "0")):
    os.environ["RFLU_MIXED_GEMV_MAX_RHS"] = value
    h.reload_tuning()
    for k in args.sweep_nrhs:
        ts = []
        for i in range(args.reps + 2):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            h.call("rflu_residual_f64_dev", n, k, ptr(A), n, ptr(X1), n, ptr(B1), n, ptr(R1), n)
            e1.record(stream)
            e1.synchronize()
            if i >= 2:
                ts.append(e0.elapsed_time(e1))
        table[(mode, k)] = float(np.median(ts))
os.environ.pop("RFLU_MIXED_GEMV_MAX_RHS")
h.reload_tuning()
h.set_stream(None)
best = 0
for k in args.sweep_nrhs:
    few, gemm = table[("few", k)], table[("gemm", k)]
    say(f"{k:6d}{few:14.3f}{gemm:10.3f}")
    if few <= gemm:
        best = k
say(f"largest measured nrhs at which residual_few is not slower than the GEMM: {best}")
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
