#!/usr/bin/env python
"""Microbenchmark of the complex mixed-precision solve.  One process; the routes of a comparison alternate call
by call; every figure is the median of REPS timed calls after one untimed call of each route.  Writes profiles/complex_mixed_sizes.txt:

  1. lu_complex_mixed + ldiv_complex_mixed against lu_complex + ldiv_complex_ (ComplexF64), n x nrhs grid;
  2. the two streaming kernels alone (the library's per-launch timers): cdemote_relayout in GB/s of 24 n^2 bytes, cresidual_few with one
     right-hand side in GB/s of 16 n^2 bytes;
  3. the narrow forward solve on the row-major factors (rflu_mixed_solve_cf32_dev) against rflu_getrs_cf32_dev (which copies the factors);
  4. the residual crossover: rflu_residual_cf64_dev through cresidual_few and through the GEMM, per number of right-hand sides.

    python scripts/microbench_complex_mixed.py [--reps 5] [--sizes 1024,4096,8192] [--out profiles/complex_mixed_sizes.txt]
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import recursivefactorization.jl_amd as rf  # noqa: E402
from recursivefactorization.jl_amd import _ffi  # noqa: E402


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def rand_cm(rows, cols, seed, dtype=torch.complex128):
    g = torch.Generator(device="cpu").manual_seed(seed)
    real = torch.float64 if dtype == torch.complex128 else torch.float32
    t = torch.complex(torch.rand((cols, rows), generator=g, dtype=real) - 0.5, torch.rand((cols, rows), generator=g, dtype=real) - 0.5)
    return t.to("cuda:0").T          # column-major


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternate(routes, reps):
    """routes: {name: callable}; one warm-up each, then reps rounds with the routes alternating; median ms per route"""
    for fn in routes.values():
        fn()
    ms = {k: [] for k in routes}
    for _ in range(reps):
        for k, fn in routes.items():
            ms[k].append(timed(fn))
    return {k: statistics.median(v) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="1024,4096,8192")
    ap.add_argument("--nrhs", default="1,8,9,64")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "complex_mixed_sizes.txt"))
    a = ap.parse_args()
    assert a.reps >= 5, "median of at least 5"
    sizes = [int(s) for s in a.sizes.split(",")]
    widths = [int(s) for s in a.nrhs.split(",")]
    h = _ffi.default_handle(0)
    h.set_stream(None)
    lines = [f"# complex mixed precision, {torch.cuda.get_device_name(0)}, librflu version {_ffi.load().rflu_version()}, median of {a.reps}, "
             "routes alternating call by call in one process", ""]

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("## 1. lu_complex_mixed + ldiv_complex_mixed against lu_complex + ldiv_complex_ (ms, factorization and solve together)")
    emit(f"{'n':>6} {'nrhs':>5} {'mixed ms':>10} {'cf64 ms':>10} {'cf64/mixed':>11} {'iters':>6}")
    for n in sizes:
        A = rand_cm(n, n, 900 + n)
        for k in widths:
            B = rand_cm(n, k, 901 + n)
            state = {}

            def mixed():
                F = rf.lu_complex_mixed(A)
                rf.ldiv_complex_mixed(F, B, fallback=False)
                state["iters"] = F.iters

            def full():
                F = rf.lu_complex(A)
                X = B.clone()
                rf.ldiv_complex_(F, X)

            ms = alternate({"mixed": mixed, "cf64": full}, a.reps)
            emit(f"{n:>6} {k:>5} {ms['mixed']:>10.3f} {ms['cf64']:>10.3f} {ms['cf64'] / ms['mixed']:>11.2f} {state['iters']:>6}")

    emit("")
    emit("## 2. the streaming kernels alone (per-launch timers of the library; GB/s of the algorithmic bytes 24 n^2 and 16 n^2)")
    emit(f"{'n':>6} {'cdemote ms':>11} {'GB/s':>8} {'cresidual_few(1) ms':>20} {'GB/s':>8}")
    for n in sizes:
        A, X, B = rand_cm(n, n, 900 + n), rand_cm(n, 1, 3), rand_cm(n, 1, 4)
        R = torch.empty_like(B)
        dem, res = [], []
        for rep in range(a.reps + 1):
            h.profile_enable(1)
            rf.lu_complex_mixed(A)
            d = h.profile()["transpose"]["ms"]
            h.profile_enable(1)
            h.call("rflu_residual_cf64_dev", n, 1, ptr(A), n, ptr(X), n, ptr(B), n, ptr(R), n)
            r = h.profile()["misc"]["ms"]
            h.profile_enable(0)
            if rep:
                dem.append(d)
                res.append(r)
        d, r = statistics.median(dem), statistics.median(res)
        emit(f"{n:>6} {d:>11.4f} {24.0 * n * n / d / 1e6:>8.1f} {r:>20.4f} {16.0 * n * n / r / 1e6:>8.1f}")

    emit("")
    emit("## 3. forward solve on the row-major ComplexF32 factors (rflu_mixed_solve_cf32_dev) against rflu_getrs_cf32_dev (ms)")
    emit(f"{'n':>6} {'nrhs':>5} {'row-major ms':>13} {'getrs ms':>10} {'getrs/row-major':>16}")
    for n in sizes:
        A = rand_cm(n, n, 900 + n)
        F = rf.lu_complex_mixed(A)
        ld = int(F.F32.stride(0))
        Fcm = F.F32.T.contiguous().T                      # the same factors column-major, for rflu_getrs_cf32_dev
        for k in widths:
            B0 = rand_cm(n, k, 5, torch.complex64)
            B1, B2 = B0.clone(), B0.clone()
            ms = alternate({
                "rm": lambda: h.call("rflu_mixed_solve_cf32_dev", n, k, ptr(F.F32), ld, ptr(F.ipiv), ptr(B1), n),
                "cm": lambda: h.call("rflu_getrs_cf32_dev", n, k, ptr(Fcm), n, ptr(F.ipiv), ptr(B2), n)}, a.reps)
            emit(f"{n:>6} {k:>5} {ms['rm']:>13.3f} {ms['cm']:>10.3f} {ms['cm'] / ms['rm']:>16.2f}")

    emit("")
    emit("## 4. residual crossover: rflu_residual_cf64_dev through cresidual_few (passes of 8) and through the ComplexF64 GEMM (ms)")
    emit(f"{'n':>6} {'nrhs':>5} {'few ms':>10} {'gemm ms':>10} {'gemm/few':>9}")
    for n in sizes:
        A = rand_cm(n, n, 900 + n)
        for k in (1, 4, 8, 9, 16, 17, 24, 32, 48, 64):
            X, B = rand_cm(n, k, 6), rand_cm(n, k, 7)
            R = torch.empty_like(B)

            def route(limit):
                def run():
                    os.environ["RFLU_MIXED_GEMV_MAX_RHS"] = limit
                    h.reload_tuning()
                    h.call("rflu_residual_cf64_dev", n, k, ptr(A), n, ptr(X), n, ptr(B), n, ptr(R), n)
                return run

            ms = alternate({"few": route("1000000"), "gemm": route("0")}, a.reps)
            emit(f"{n:>6} {k:>5} {ms['few']:>10.3f} {ms['gemm']:>10.3f} {ms['gemm'] / ms['few']:>9.2f}")
    os.environ.pop("RFLU_MIXED_GEMV_MAX_RHS", None)
    h.reload_tuning()

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
