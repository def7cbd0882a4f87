"""The complex solves against each other: ldiv!(F, B), ldiv!(transpose(F), B) and ldiv!(F', B) through their device entries.

    microbench_complex_solve.py [--n 1024 4096 8192] [--nrhs 1 8 9 64] [--reps 11] [--warmup 2] [--sweep] [--out FILE]
                                                                    (default: profiles/complex_solve_sizes.txt)

  * per precision, n and nrhs: rflu_getrs_{cf64,cf32}_dev (forward), rflu_getrs_trans_*_dev with conj = 0 ('T') and conj = 1 ('C'),
    ALTERNATING in one process on the same factors: every repetition times the three one after the other, so a drift of the machine
    falls on all of them.  Milliseconds, median of --reps after --warmup untimed rounds, host clock around call + synchronisation (the
    entries synchronise the handle's stream before they return); the spread (min .. max) is printed next to the median.  The right-hand
    sides are restored from a copy outside the window.  The factors are a diagonally dominant random matrix's own (rflu_getrf_*_dev);
  * the bytes a solve has to read, n^2 complex elements of F once, over the median: GB/s of F, the figure that bounds nrhs <= 8;
  * --sweep: the thresholds of the transposed solve, CNARROW (narrow | wide boundary) and CNB (rows per diagonal block), which only an
    experiments build of the library reads from the environment (RFLU_EXPERIMENTS=1 at build time, RFLU_LIB=.../librflu_exp.so here):
    RFLU_CNARROW in {0, 8} at nrhs <= 8 and RFLU_CNB in {64, 128, 256}.  With the default build the sweep says so and is skipped.
Neither threshold has been tuned; this script is what a tuning would start from.  No GPU, no numbers: the script fails."""
import argparse
import ctypes
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from recursivefactorization.jl_amd import _ffi
from recursivefactorization.jl_amd import build as B

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, nargs="+", default=[1024, 4096, 8192])
ap.add_argument("--nrhs", type=int, nargs="+", default=[1, 8, 9, 64])
ap.add_argument("--reps", type=int, default=11)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--sweep", action="store_true", help="CNARROW / CNB sweep (experiments build only)")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "complex_solve_sizes.txt"),
                help="the table is also written to this file")
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("microbench_complex_solve.py measures an MI355X; no GPU is visible")

lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


h = _ffi.default_handle(0)
h.set_stream(None)


def factors(n, rdt):
    """Column-major device factors and ipiv of rand + n I (well conditioned, so the solves stay finite over many repetitions)."""
    A = torch.complex(torch.rand((n, n), dtype=rdt, device="cuda:0"), torch.rand((n, n), dtype=rdt, device="cuda:0"))
    A += n * torch.eye(n, dtype=A.dtype, device="cuda:0")
    A = A.T                                   # column-major view
    ipiv = torch.empty(n, dtype=torch.int64, device="cuda:0")
    info = ctypes.c_int64(0)
    h.call(f"rflu_getrf_{'cf64' if rdt == torch.float64 else 'cf32'}_dev", n, n, ptr(A), n, ptr(ipiv), 1, ctypes.byref(info))
    assert info.value == 0
    return A, ipiv


def alternating(calls, restore):
    """calls: name -> callable.  Every round runs each once, in order; returns name -> (median, min, max) in ms over the timed rounds."""
    ts = {k: [] for k in calls}
    for i in range(args.warmup + args.reps):
        for k, call in calls.items():
            restore()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            h.synchronize()
            if i >= args.warmup:
                ts[k].append((time.perf_counter() - t0) * 1e3)
    return {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in ts.items()}


def solve_calls(cs, n, nrhs, F, ipiv, X):
    return {"fwd": lambda: h.call(f"rflu_getrs_{cs}_dev", n, nrhs, ptr(F), n, ptr(ipiv), ptr(X), n),
            "T": lambda: h.call(f"rflu_getrs_trans_{cs}_dev", n, nrhs, ptr(F), n, ptr(ipiv), ptr(X), n, 0),
            "C": lambda: h.call(f"rflu_getrs_trans_{cs}_dev", n, nrhs, ptr(F), n, ptr(ipiv), ptr(X), n, 1)}


say(f"# microbench_complex_solve.py  build {B.sources_digest()[:12]}  lib {os.path.basename(_ffi.LIB_PATH)}  reps {args.reps}  warmup {args.warmup}")
for rdt, cs, esize in ((torch.float64, "cf64", 16), (torch.float32, "cf32", 8)):
    say(f"## {cs}: forward, 'T' and 'C' device entries alternating (ms: median [min .. max]; GB/s = n^2 elements of F once over the median)")
    say("       n  nrhs          fwd_ms                    T_ms                    C_ms      fwd_GB/s   T_GB/s   C_GB/s   T/fwd")
    for n in args.n:
        F, ipiv = factors(n, rdt)
        for nrhs in args.nrhs:
            B0 = torch.complex(torch.rand((nrhs, n), dtype=rdt, device="cuda:0"), torch.rand((nrhs, n), dtype=rdt, device="cuda:0")).T
            X = B0.clone()
            r = alternating(solve_calls(cs, n, nrhs, F, ipiv, X), lambda: X.copy_(B0))
            gb = {k: n * n * esize / (v[0] * 1e-3) / 1e9 for k, v in r.items()}
            cell = {k: f"{v[0]:9.3f} [{v[1]:.3f} .. {v[2]:.3f}]" for k, v in r.items()}
            say(f"{n:8d} {nrhs:5d}   {cell['fwd']:>24s} {cell['T']:>24s} {cell['C']:>24s}   {gb['fwd']:8.1f} {gb['T']:8.1f} {gb['C']:8.1f}   {r['T'][0] / r['fwd'][0]:6.2f}")
            del B0, X
        if args.sweep:
            if "exp" not in os.path.basename(_ffi.LIB_PATH):
                say("# --sweep: the loaded library is the default build, which has CNARROW = 8 and CNB = 256 as constants; build with RFLU_EXPERIMENTS=1 and "
                    "set RFLU_LIB to librflu_exp.so")
            else:
                say(f"## {cs} n = {n}: 'T' with RFLU_CNARROW / RFLU_CNB from the environment (ms, median [min .. max])")
                for nrhs in [k for k in args.nrhs if k <= 8]:
                    B0 = torch.complex(torch.rand((nrhs, n), dtype=rdt, device="cuda:0"), torch.rand((nrhs, n), dtype=rdt, device="cuda:0")).T
                    X = B0.clone()
                    for cnarrow, cnb in ((0, 256), (8, 64), (8, 128), (8, 256)):
                        os.environ["RFLU_CNARROW"], os.environ["RFLU_CNB"] = str(cnarrow), str(cnb)   # (putenv: the library's getenv sees it)
                        v = alternating({"T": solve_calls(cs, n, nrhs, F, ipiv, X)["T"]}, lambda: X.copy_(B0))["T"]
                        say(f"    nrhs {nrhs:3d}  CNARROW {cnarrow}  CNB {cnb:4d}   {v[0]:9.3f} [{v[1]:.3f} .. {v[2]:.3f}]")
                    del B0, X
        del F, ipiv
        torch.cuda.empty_cache()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
