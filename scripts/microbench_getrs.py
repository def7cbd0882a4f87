"""ldiv!(F, B) on the device: time per solve.

    microbench_getrs.py [n]                    row-major factors from lu_ on a contiguous tensor, row-major B (1, 64, 1024 right-hand sides)
    microbench_getrs.py --trans [n ...]        column-major device entry, Float64: ldiv!(F, B) and ldiv!(F', B) ALTERNATING in one
                                               process, 1 and 64 right-hand sides (--nrhs), median of --reps timed pairs
"""
import argparse, sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch, numpy as np
import recursivefactorization.jl_amd as rf

ap = argparse.ArgumentParser()
ap.add_argument("n", nargs="*", type=int)
ap.add_argument("--trans", action="store_true", help="time the transposed next to the forward solve (column-major device entry)")
ap.add_argument("--nrhs", type=int, nargs="+", default=[1, 64])
ap.add_argument("--reps", type=int, default=11)
args = ap.parse_args()


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
    return time.perf_counter() - t0


if args.trans:
    for n in args.n or [16384, 4096]:
        A = torch.rand((n, n), dtype=torch.float64, device="cuda").T        # stride(0) == 1: a column-major matrix
        A0 = A.clone()
        F = rf.lu_(A, None, True, check=False)
        for nrhs in args.nrhs:
            B0 = torch.rand((nrhs, n), dtype=torch.float64, device="cuda").T
            X = B0.clone(); Y = B0.clone()
            assert X.stride(0) == 1 and Y.stride(0) == 1
            rf.ldiv_(F, X); rf.ldiv_(rf.Adjoint(F), Y); torch.cuda.synchronize()      # warm-up: workspaces, code objects
            res_f = ((A0 @ X - B0).norm() / B0.norm()).item()
            res_t = ((A0.T @ Y - B0).norm() / B0.norm()).item()
            tf, tt = [], []
            for _ in range(args.reps):
                X.copy_(B0); tf.append(timed(lambda: rf.ldiv_(F, X)))
                Y.copy_(B0); tt.append(timed(lambda: rf.ldiv_(rf.Adjoint(F), Y)))
            f, t = float(np.median(tf)), float(np.median(tt))
            print(f"n={n} nrhs={nrhs:3d}: forward {f*1e3:7.3f} ms (min {min(tf)*1e3:7.3f})   transposed {t*1e3:7.3f} ms (min {min(tt)*1e3:7.3f})   "
                  f"transposed/forward {t/f:5.2f}   relative residuals {res_f:.1e} / {res_t:.1e}", flush=True)
    sys.exit(0)

n = args.n[0] if args.n else 8192
A = torch.rand((n, n), dtype=torch.float64, device="cuda")          # a contiguous tensor is taken as the row-major matrix
A0 = A.clone()
F = rf.lu_(A, None, True, check=False)
for nrhs in (1, 64, 1024):
    X = torch.rand((n, nrhs), dtype=torch.float64, device="cuda")
    B0 = X.clone()
    rf.ldiv_(F, X); torch.cuda.synchronize()
    R = A0 @ X - B0
    res = (R.norm() / B0.norm()).item()
    ts = []
    for _ in range(5):
        X.copy_(B0); torch.cuda.synchronize(); t0 = time.perf_counter(); rf.ldiv_(F, X); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    t = sorted(ts)[2]
    print(f"n={n} nrhs={nrhs:5d}: {t*1e3:8.2f} ms  ({2.0*n*n*nrhs/t/1e9:9.1f} GFLOP/s)  relative residual {res:.2e}", flush=True)
