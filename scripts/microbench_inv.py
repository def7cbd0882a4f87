"""The in-place inverse (rflu_getri_*) against the only way there was before it: rflu_getrs_*_dev on an explicit identity.

    microbench_inv.py [--n 1024 2048 4096 8192 16384] [--bn 8 16 32 64 128] [--batch 10000] [--reps 5] [--out profiles/inv_sizes.txt]

For Float64 and Float32:
  * per n: milliseconds (median of --reps, wall clock around the synchronous C call after one warm-up; the factors are restored from a
    copy outside the window) of getri on the factors and of getrs on a fresh n x n identity, their ratio, TFLOP/s at 4 n^3 / 3 and
    2 n^3, and the device memory each route holds: the caller's arrays plus what the handle allocated for it (the difference of
    torch.cuda.mem_get_info around the first call on a fresh handle);
  * per small n at --batch matrices: batched getri (identity made in LDS) against batched getrs on an identity tensor, and the bytes
    of that tensor.
Neither route is chosen by the library for the caller: the table says which is faster where.  No GPU, no numbers: the script fails."""
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
ap.add_argument("--n", type=int, nargs="+", default=[1024, 2048, 4096, 8192, 16384])
ap.add_argument("--bn", type=int, nargs="+", default=[8, 16, 32, 64, 128])
ap.add_argument("--batch", type=int, default=10000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=None, help="also write the table to this file")
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("microbench_inv.py measures an MI355X; no GPU is visible")

lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def median_ms(call, before):
    ts = []
    for i in range(args.reps + 1):
        before()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()                                # the C entries are complete on return
        if i >= 1:
            ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def held_by(call):
    """bytes the device lost over `call` (what a fresh handle allocated for it)"""
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    call()
    torch.cuda.synchronize()
    return free0 - torch.cuda.mem_get_info()[0]


say(f"# microbench_inv.py  build {B.sources_digest()[:12]}  reps {args.reps}")
for dt, sfx in ((torch.float64, "f64"), (torch.float32, "f32")):
    es = 8 if dt == torch.float64 else 4
    say(f"## {sfx}: getri vs getrs on an identity (ms, median)")
    say("     n    getri_ms   ident_ms   ident/getri   getri_TF/s  ident_TF/s   getri_MiB  ident_MiB")
    for n in args.n:
        A = torch.rand((n, n), dtype=dt, device="cuda:0").T
        F = rf.lu(A)
        keep, work = F.factors.clone(), F.factors
        info = ctypes.c_int64(0)
        hg, hi = _ffi.Handle(0), _ffi.Handle(0)   # fresh handles: their workspaces are what each route costs
        ident = torch.empty((n, n), dtype=dt, device="cuda:0").T

        def getri():
            hg.call(f"rflu_getri_{sfx}_dev", n, ptr(work), n, ptr(F.ipiv), ctypes.byref(info))

        def solve():
            hi.call(f"rflu_getrs_{sfx}_dev", n, n, ptr(keep), n, ptr(F.ipiv), ptr(ident), n)

        def fresh_identity():
            ident.zero_()
            ident.diagonal().fill_(1)

        fresh_identity()
        mem_g = held_by(getri) + n * n * es
        mem_i = held_by(solve) + 2 * n * n * es
        tg = median_ms(getri, lambda: work.copy_(keep))
        ti = median_ms(solve, fresh_identity)
        say(f"{n:6d}  {tg:10.3f} {ti:10.3f} {ti / tg:10.2f}   {4 * n ** 3 / 3 / tg / 1e9:10.2f}  {2 * n ** 3 / ti / 1e9:10.2f}  "
            f"{mem_g / 2 ** 20:10.1f} {mem_i / 2 ** 20:10.1f}")
        hg.close()
        hi.close()
        del A, F, keep, work, ident
        torch.cuda.empty_cache()
    say(f"## {sfx}: batched getri vs batched getrs on an identity tensor, batch {args.batch} (ms, median)")
    say("     n    getri_ms   ident_ms   ident/getri   identity_MiB")
    h = _ffi.default_handle(0)
    h.set_stream(None)
    for n in args.bn:
        A = torch.rand((args.batch, n, n), dtype=dt, device="cuda:0") + 10 * torch.eye(n, dtype=dt, device="cuda:0")
        F = rf.lu_batched_(A.transpose(1, 2))
        X = torch.empty_like(A)
        info = torch.zeros(args.batch, dtype=torch.int64, device="cuda:0")
        ident = torch.empty_like(A)

        def bgetri():
            h.call(f"rflu_getri_batched_{sfx}_dev", args.batch, n, ptr(A), n, n * n, 0, ptr(F.ipiv), n, ptr(X), n, n * n, ptr(info))

        def bsolve():
            h.call(f"rflu_getrs_batched_{sfx}_dev", args.batch, n, n, ptr(A), n, n * n, 0, ptr(F.ipiv), n, ptr(ident), n, n * n, 0)

        def fresh_identity():
            ident.copy_(torch.eye(n, dtype=dt, device="cuda:0").expand(args.batch, n, n))

        tg = median_ms(bgetri, lambda: None)
        ti = median_ms(bsolve, fresh_identity)
        say(f"{n:6d}  {tg:10.3f} {ti:10.3f} {ti / tg:10.2f}   {args.batch * n * n * es / 2 ** 20:10.1f}")
        del A, F, X, ident
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
