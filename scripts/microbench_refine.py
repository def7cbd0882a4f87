"""Iterative refinement with error bounds (rflu_gerfs_*, rflu_berr_*) against what it is measured by.

    microbench_refine.py [--n 1024 4096 16384] [--nrhs 1 8 64] [--reps 9] [--out profiles/refine_sizes.txt]

One process, routes alternating call by call, median of --reps after one warm-up each:
  * the fused pass: rflu_berr_f64_dev (absresidual_few + its combine and the per-column reduction with one host read; the pass itself
    has no entry of its own) against rflu_residual_f64_dev at the same nrhs -- the parent's kernel, which reads the same 8 n^2 bytes
    per 8 right-hand sides for half the arithmetic -- in GB/s of those bytes, and the ratio of the two times; Float32 berr too;
  * gerfs with and without ferr against getrs and getrf at the same n, Float64 and Float32, with the step counts.  X starts from the
    getrs solution every time (the n x nrhs copy that restores it is inside the timed region of the gerfs routes).
A = uniform[0, 1) + (n / 4) I from the library's generator.  No GPU, no numbers: the script fails."""
import argparse
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from recursivefactorization.jl_amd import _ffi
from recursivefactorization.jl_amd import build as B

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, nargs="+", default=[1024, 4096, 16384])
ap.add_argument("--nrhs", type=int, nargs="+", default=[1, 8, 64])
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--out", default=None, help="also write the table to this file")
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("microbench_refine.py measures an MI355X; no GPU is visible")

lines = []
h = _ffi.default_handle(0)
h.set_stream(None)


def say(s):
    print(s, flush=True)
    lines.append(s)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def alternating_ms(calls):
    ts = {k: [] for k in calls}
    for i in range(args.reps + 1):
        for k, f in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            if i >= 1:
                ts[k].append((time.perf_counter() - t0) * 1e3)
    return {k: float(np.median(v)) for k, v in ts.items()}


def cm(rows, cols, td):
    return torch.empty((cols, rows), dtype=td, device="cuda:0").T


say(f"# microbench_refine.py  {torch.cuda.get_device_name(0)}  librflu {_ffi.load().rflu_version()}  build {B.sources_digest()[:12]}  median of {args.reps}, routes alternating")
for sfx, td in (("f64", torch.float64), ("f32", torch.float32)):
    es = 8 if sfx == "f64" else 4
    for n in args.n:
        A = cm(n, n, td)
        h.call(f"rflu_fill_uniform_{sfx}_dev", ptr(A), n, n, n, 0, 12, n, 0, 0, n / 4.0)
        F = A.clone()
        ipiv = torch.zeros(n, dtype=torch.int64, device="cuda:0")
        info = ctypes.c_int64(0)

        def getrf():
            F.copy_(A)
            h.call(f"rflu_getrf_{sfx}_dev", n, n, ptr(F), n, ptr(ipiv), 1, 0, ctypes.byref(info))

        getrf()
        for nrhs in args.nrhs:
            Bm = cm(n, nrhs, td)
            h.call(f"rflu_fill_uniform_{sfx}_dev", ptr(Bm), n, nrhs, n, 0, 13, n, 0, 0, 0.0)
            X0 = Bm.clone()
            h.call(f"rflu_getrs_{sfx}_dev", n, nrhs, ptr(F), n, ptr(ipiv), ptr(X0), n)
            X, Rm = X0.clone(), cm(n, nrhs, torch.float64)
            fe, be, st = np.zeros(nrhs), np.zeros(nrhs), np.zeros(nrhs, dtype=np.intc)
            P = lambda a: ctypes.c_void_p(a.ctypes.data)   # noqa: E731

            def gerfs(with_ferr):
                X.copy_(X0)
                h.call(f"rflu_gerfs_{sfx}_dev", n, nrhs, ptr(A), n, ptr(F), n, ptr(ipiv), ptr(Bm), n, ptr(X), n,
                       P(fe) if with_ferr else ctypes.c_void_p(0), P(be), 5, P(st), ctypes.byref(info))

            def getrs():
                X.copy_(Bm)
                h.call(f"rflu_getrs_{sfx}_dev", n, nrhs, ptr(F), n, ptr(ipiv), ptr(X), n)

            calls = {"berr": lambda: h.call(f"rflu_berr_{sfx}_dev", n, nrhs, ptr(A), n, ptr(X0), n, ptr(Bm), n, P(be)),
                     "gerfs": lambda: gerfs(False), "gerfs+ferr": lambda: gerfs(True), "getrs": getrs, "getrf": getrf}
            if sfx == "f64":
                calls["residual"] = lambda: h.call("rflu_residual_f64_dev", n, nrhs, ptr(A), n, ptr(X0), n, ptr(Bm), n, ptr(Rm), n)
            ms = alternating_ms(calls)
            gerfs(True)
            passes = (nrhs + 7) // 8
            gbs = lambda t: passes * es * n * n / (t * 1e-3) / 1e9   # noqa: E731
            line = (f"{sfx} n={n:6d} nrhs={nrhs:3d}  berr {ms['berr']:8.3f} ms {gbs(ms['berr']):7.0f} GB/s")
            if sfx == "f64":
                line += f"  residual {ms['residual']:8.3f} ms {gbs(ms['residual']):7.0f} GB/s  berr/residual {ms['berr'] / ms['residual']:.2f}"
            line += (f"  gerfs {ms['gerfs']:9.3f} ms  gerfs+ferr {ms['gerfs+ferr']:9.3f} ms  getrs {ms['getrs']:8.3f} ms  getrf {ms['getrf']:8.3f} ms"
                     f"  steps {int(st.min())}..{int(st.max())}  berr/u {be.max() / (2.0 ** -53 if sfx == 'f64' else 2.0 ** -24):.2f}")
            say(line)
            getrf()   # the last timed route left fresh factors; keep them in step with ipiv

if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
