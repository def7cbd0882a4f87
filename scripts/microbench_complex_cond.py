"""Complex operator norm and condition estimate (rflu_lange_c*, rflu_gecon_c*) against what they are measured by.

    microbench_complex_cond.py [--ln 4096 16384] [--n 1024 4096 8192] [--bn 8 32 64 128] [--batch 4096] [--reps 9] [--out profiles/complex_cond_sizes.txt]

For ComplexF64 and ComplexF32, routes alternating call by call in one process, median of --reps after one warm-up each:
  * lange: GB/s of n^2 complex elements for both norms of a column-major n x n matrix (one streaming pass: the yardstick is HBM);
  * gecon against the complex getrf at the same n: milliseconds of each, their ratio, and the number of solves the estimate took (the
    NumPy restatement of tests/complex_cond_cases.py on the downloaded factors; n <= 4096 only, it is O(n^2) per solve on the CPU);
  * gecon_batched against the only route there was: inv_complex_batched plus a norm in torch, at --batch matrices per n (sizes above the
    one-launch limit of the element type, 64 for ComplexF64, are left out).
No GPU, no numbers: the script fails."""
import argparse
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import recursivefactorization.jl_amd as rf
from recursivefactorization.jl_amd import _ffi
from recursivefactorization.jl_amd import build as B

ap = argparse.ArgumentParser()
ap.add_argument("--ln", type=int, nargs="+", default=[4096, 16384])
ap.add_argument("--n", type=int, nargs="+", default=[1024, 4096, 8192])
ap.add_argument("--bn", type=int, nargs="+", default=[8, 32, 64, 128])
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--out", default=None, help="also write the table to this file")
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("microbench_complex_cond.py measures an MI355X; no GPU is visible")

lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def alternating_ms(calls):
    """Median milliseconds of every call in `calls` (name -> function), the routes taking turns; the entries are complete on return."""
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


def crand(shape, dt):
    rt = torch.float64 if dt == torch.complex128 else torch.float32
    return torch.complex(torch.rand(shape, dtype=rt, device="cuda:0") - 0.5, torch.rand(shape, dtype=rt, device="cuda:0") - 0.5)


say(f"# microbench_complex_cond.py  {torch.cuda.get_device_name(0)}  librflu {_ffi.load().rflu_version()}  build {B.sources_digest()[:12]}  median of {args.reps}, routes alternating")
for dt, es, limit in ((torch.complex128, 16, 64), (torch.complex64, 8, 128)):
    name = "cf64" if es == 16 else "cf32"
    say(f"## {name}: lange, column-major n x n")
    say("      n    one_ms   one_GB/s    inf_ms   inf_GB/s")
    for n in args.ln:
        A = crand((n, n), dt).T
        ms = alternating_ms({"one": lambda: rf.opnorm_complex(A, 1), "inf": lambda: rf.opnorm_complex(A, math.inf)})
        gb = n * n * es / 1e9
        say(f"{n:7d} {ms['one']:9.3f} {gb / ms['one'] * 1e3:10.1f} {ms['inf']:9.3f} {gb / ms['inf'] * 1e3:10.1f}")
        del A
    say(f"## {name}: gecon (1-norm and Inf-norm) against getrf")
    say("      n   getrf_ms  gecon1_ms  geconI_ms  gecon1/getrf  solves1  solvesI")
    for n in args.n:
        A = crand((n, n), dt).T
        a1, ai = rf.opnorm_complex(A, 1), rf.opnorm_complex(A, math.inf)
        F = rf.lu_complex(A, check=False)
        work = A.clone()

        def getrf():
            work.copy_(A)
            rf.lu_complex_(work, check=False)

        def copy_only():
            work.copy_(A)

        ms = alternating_ms({"copy": copy_only, "getrf": getrf, "g1": lambda: rf.rcond_complex(F, a1, 1),
                             "gi": lambda: rf.rcond_complex(F, ai, math.inf)})
        solves = ("-", "-")
        if n <= 4096:
            import complex_cond_cases as C

            host = F.factors.cpu().numpy()
            solves = tuple(C.crcond_restatement(host, norm, an, host.dtype.type, detail=True)[2] for norm, an in ((1, a1), (2, ai)))
        say(f"{n:7d} {ms['getrf'] - ms['copy']:10.3f} {ms['g1']:10.3f} {ms['gi']:10.3f} {ms['g1'] / (ms['getrf'] - ms['copy']):13.3f} {solves[0]:>8} {solves[1]:>8}")
        del A, F, work
    say(f"## {name}: gecon_batched against inv_complex_batched + a norm in torch, batch {args.batch}")
    say("      n  gecon_ms  inv+norm_ms   ratio")
    for n in args.bn:
        if n > limit:
            continue
        A = crand((args.batch, n, n), dt)
        an = rf.opnorm_complex_batched(A, 1)
        F = rf.lu_complex_batched(A, check=False)

        def by_inverse():
            X = rf.inv_complex_batched(F, check=False)
            return 1.0 / (an * X.abs().sum(dim=1).amax(dim=1))

        ms = alternating_ms({"gecon": lambda: rf.rcond_complex_batched(F, an, 1), "inv": by_inverse})
        say(f"{n:7d} {ms['gecon']:9.3f} {ms['inv']:12.3f} {ms['inv'] / ms['gecon']:7.2f}")

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
