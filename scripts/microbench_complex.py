"""The complex path against the real one of the same element precision.

    microbench_complex.py [--gemm 1024 4096] [--k 64 512] [--n 256 1024 4096] [--reps 5] [--out FILE]   (default: profiles/complex_sizes.txt)

  * the complex GEMM (rflu_gemm_rm_cf64_dev / _cf32_dev) against the real GEMM (rflu_gemm_rm_f64_dev / _f32_dev) at the same M = N
    and K: milliseconds (median of --reps, wall clock around call + synchronisation after one warm-up) and TFLOP/s, counting 2 M N K
    flops for the real product and 4 times that for the complex one;
  * rflu_getrf_cf64_dev / _cf32_dev against rflu_getrf_f64_dev / _f32_dev per n (column-major device entries, the matrix restored from a
    copy outside the window): milliseconds and TFLOP/s at 2 n^3 / 3 resp. 8 n^3 / 3.
No GPU, no numbers: the script fails."""
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
ap.add_argument("--gemm", type=int, nargs="+", default=[1024, 4096])
ap.add_argument("--k", type=int, nargs="+", default=[64, 512])
ap.add_argument("--n", type=int, nargs="+", default=[256, 1024, 4096])
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "complex_sizes.txt"),
                help="the table is also written to this file")
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("microbench_complex.py measures an MI355X; no GPU is visible")

lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


h = _ffi.default_handle(0)
h.set_stream(None)


def median_ms(call, before=lambda: None):
    ts = []
    for i in range(args.reps + 1):
        before()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        h.synchronize()
        if i >= 1:
            ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


say(f"# microbench_complex.py  build {B.sources_digest()[:12]}  reps {args.reps}")
for rdt, cdt, rs, cs in ((torch.float64, torch.complex128, "f64", "cf64"), (torch.float32, torch.complex64, "f32", "cf32")):
    say(f"## GEMM C -= A*B, M = N: {cs} against {rs} (ms, median; TFLOP/s at 8 MNK resp. 2 MNK)")
    say("     M=N      K   complex_ms    real_ms   complex_TF/s  real_TF/s   complex/real time")
    for mn in args.gemm:
        for k in args.k:
            def rnd(r, c, dt):
                t = torch.rand((r, c), dtype=rdt, device="cuda:0")
                return torch.complex(t, torch.rand((r, c), dtype=rdt, device="cuda:0")) if dt.is_complex else t

            Ar, Br, Cr = rnd(mn, k, rdt), rnd(k, mn, rdt), rnd(mn, mn, rdt)
            Ac, Bc, Cc = rnd(mn, k, cdt), rnd(k, mn, cdt), rnd(mn, mn, cdt)
            tr = median_ms(lambda: h.call(f"rflu_gemm_rm_{rs}_dev", mn, mn, k, ptr(Ar), k, ptr(Br), mn, ptr(Cr), mn))
            tc = median_ms(lambda: h.call(f"rflu_gemm_rm_{cs}_dev", mn, mn, k, ptr(Ac), k, ptr(Bc), mn, ptr(Cc), mn))
            fl = 2.0 * mn * mn * k
            say(f"{mn:8d} {k:6d}   {tc:10.3f} {tr:10.3f}   {4 * fl / tc / 1e9:10.2f} {fl / tr / 1e9:10.2f}   {tc / tr:10.2f}")
            del Ar, Br, Cr, Ac, Bc, Cc
    say(f"## getrf, n x n, pivoted, device entry: {cs} against {rs} (ms, median; TFLOP/s at 8 n^3 / 3 resp. 2 n^3 / 3)")
    say("       n   complex_ms    real_ms   complex_TF/s  real_TF/s   complex/real time")
    for n in args.n:
        Ar = torch.rand((n, n), dtype=rdt, device="cuda:0").T
        Ac = torch.complex(torch.rand((n, n), dtype=rdt, device="cuda:0"), torch.rand((n, n), dtype=rdt, device="cuda:0")).T
        keep_r, keep_c = Ar.clone(), Ac.clone()
        ipiv = torch.empty(n, dtype=torch.int64, device="cuda:0")
        info = ctypes.c_int64(0)
        tr = median_ms(lambda: h.call(f"rflu_getrf_{rs}_dev", n, n, ptr(Ar), n, ptr(ipiv), 1, 0, ctypes.byref(info)), lambda: Ar.copy_(keep_r))
        tc = median_ms(lambda: h.call(f"rflu_getrf_{cs}_dev", n, n, ptr(Ac), n, ptr(ipiv), 1, ctypes.byref(info)), lambda: Ac.copy_(keep_c))
        fl = 2.0 * n ** 3 / 3
        say(f"{n:8d}   {tc:10.3f} {tr:10.3f}   {4 * fl / tc / 1e9:10.2f} {fl / tr / 1e9:10.2f}   {tc / tr:10.2f}")
        del Ar, Ac, keep_r, keep_c
    torch.cuda.empty_cache()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
