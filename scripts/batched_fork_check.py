"""Are the inputs of tests/test_gpu_batched.py safe for an exact pivot comparison?  (CPU only.)

That test demands ipiv == oracle.lu(A) exactly for every matrix of every batch.  Two correct factorizations that sum in different
orders may pick different pivots where two candidates of a column differ by a rounding error (a "fork").  For every shape, both
element types and the seeds 50000 .. 50000 + batch - 1 this script runs two independent CPU algorithms -- the recursive oracle and
LAPACK getrf -- and reports whether they agree on every pivot, the worst residual as a fraction of the reference bound
20 m eps (test/runtests.jl:19-20) and max |l_ij|.  A shape may join the test only if every line says `forks 0`.

    python scripts/batched_fork_check.py [batch]
"""
import os
import sys

import numpy as np
from scipy.linalg import lapack

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import oracle as O  # noqa: E402

SHAPES = [(1, 1), (2, 2), (7, 7), (8, 8), (10, 12), (32, 32), (50, 52), (64, 64), (65, 65), (96, 96), (128, 128), (100, 60), (60, 100)]

if __name__ == "__main__":
    batch = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
    bad = 0
    for dtype in (np.float64, np.float32):
        getrf = lapack.dgetrf if dtype == np.float64 else lapack.sgetrf
        for m, n in SHAPES:
            forks, worst, lmax = 0, 0.0, 0.0
            for b in range(batch):
                A = O.np_uniform(m, n, 50000 + b, dtype)
                F, ip, info = O.lu(A)
                _, piv, linfo = getrf(A)
                forks += int(not np.array_equal(ip, piv + 1) or info != linfo)
                worst = max(worst, O.residual(A, F, ip)[0] / (20 * m * np.finfo(dtype).eps))
                lmax = max(lmax, float(np.max(np.abs(np.tril(F[:, :min(m, n)], -1)), initial=0.0)))
            bad += forks
            print(f"{np.dtype(dtype).name} {m}x{n}: {batch} matrices, forks {forks}, worst residual {worst:.4f} of the bound, max|l| {lmax:.6f}")
    sys.exit(1 if bad else 0)
