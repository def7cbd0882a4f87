"""The in-place complex inverse (rflu_getri_c*_dev) against the only way there was before it: rflu_getrs_c*_dev on an explicit identity.

    microbench_complex_inv.py [--n 1024 4096 8192] [--reps 5] [--out profiles/complex_inv_sizes.txt]

For ComplexF64 and ComplexF32, per n, the two routes ALTERNATING in one process: milliseconds (median of --reps, wall clock around the
synchronous C call after one warm-up of each; the factors are restored from a copy and the identity is rebuilt outside the window) of
getri on the factors and of getrs on a fresh n x n identity, their ratio, TFLOP/s at 8 * 4 n^3 / 3 and 8 * 2 n^3 real flops (a complex
multiply-add is eight), and the device memory each route holds: the caller's arrays plus what a fresh handle allocated for the call
(the difference of torch.cuda.mem_get_info around the first call).  Neither route is chosen by the library for the caller: the table
says which is faster where.  No GPU, no numbers: the script fails."""
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
from recursivefactorization.jl_amd import build as B

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, nargs="+", default=[1024, 4096, 8192])
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=None, help="also write the table to this file")
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("microbench_complex_inv.py measures an MI355X; no GPU is visible")

lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def held_by(call):
    """bytes the device lost over `call` (what a fresh handle allocated for it)"""
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    call()
    torch.cuda.synchronize()
    return free0 - torch.cuda.mem_get_info()[0]


def timed(call, before):
    before()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    call()                                    # the C entries are complete on return
    return (time.perf_counter() - t0) * 1e3


say(f"# microbench_complex_inv.py  build {B.sources_digest()[:12]}  reps {args.reps}")
for dt, sfx in ((torch.complex128, "cf64"), (torch.complex64, "cf32")):
    es = 16 if dt == torch.complex128 else 8
    say(f"## {sfx}: getri vs getrs on an identity, alternating (ms, median)")
    say("     n    getri_ms   ident_ms   ident/getri   getri_TF/s  ident_TF/s   getri_MiB  ident_MiB")
    for n in args.n:
        gen = torch.Generator(device="cuda:0").manual_seed(n)
        A = (torch.rand((n, n, 2), dtype=torch.float64, device="cuda:0", generator=gen) - 0.5)
        A = torch.view_as_complex(A).to(dt).T           # column-major, re and im uniform in [-1/2, 1/2)
        F = rf.lu_complex(A)
        keep, work = F.factors.clone(), F.factors
        info = ctypes.c_int64(0)
        hg, hi = _ffi.Handle(0), _ffi.Handle(0)         # fresh handles: their workspaces are what each route costs
        ident = torch.empty((n, n), dtype=dt, device="cuda:0").T

        def getri():
            hg.call(f"rflu_getri_{sfx}_dev", n, ptr(work), n, ptr(F.ipiv), ctypes.byref(info))

        def solve():
            hi.call(f"rflu_getrs_{sfx}_dev", n, n, ptr(keep), n, ptr(F.ipiv), ptr(ident), n)

        def fresh_identity():
            ident.zero_()
            ident.diagonal().fill_(1)

        fresh_identity()
        mem_g = held_by(getri) + n * n * es              # (these two calls are the warm-up)
        mem_i = held_by(solve) + 2 * n * n * es
        tg, ti = [], []
        for _ in range(args.reps):
            tg.append(timed(getri, lambda: work.copy_(keep)))
            ti.append(timed(solve, fresh_identity))
        tg, ti = float(np.median(tg)), float(np.median(ti))
        say(f"{n:6d}  {tg:10.3f} {ti:10.3f} {ti / tg:10.2f}   {8 * 4 * n ** 3 / 3 / tg / 1e9:10.2f}  {8 * 2 * n ** 3 / ti / 1e9:10.2f}  "
            f"{mem_g / 2 ** 20:10.1f} {mem_i / 2 ** 20:10.1f}")
        hg.close()
        hi.close()
        del A, F, keep, work, ident
        torch.cuda.empty_cache()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
