"""CPU measurement behind the bars of tests/test_gpu_inv.py (no GPU needed): what LAPACK achieves on exactly the inputs of that test.

  * numpy.linalg.inv (getrf + getri) on rand_matrix(n, n, seed=SEEDS.get(n, 91000 + n)) and on the batch inputs (seed=93000 + b): the xGET03 ratios
    rho_R = ||A X - I||_1 / (n eps ||A||_1 ||X||_1) and rho_L (X A), both element types;
  * log|det| from oracle.lu factors (the GPU's elimination order) against numpy.linalg.slogdet of the Float64-promoted matrix, in
    units of n eps_T.

usage: python scripts/inv_cpu_bars.py"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import oracle as O  # noqa: E402
from helpers import rand_matrix  # noqa: E402

SIZES = [1, 2, 63, 64, 65, 127, 128, 129, 200, 511, 512, 513, 1025, 1100, 2112]
SEEDS = {2: 94002, 511: 97511, 512: 97512, 1025: 98025}   # as tests/test_gpu_inv.py
BATCH = [(n, 200) for n in (1, 2, 7, 8, 33, 64, 65, 100, 128)] + [(200, 3)]


def rho(A, X, dtype):
    A64, X64 = A.astype(np.float64), X.astype(np.float64)
    n = A.shape[0]
    scale = n * float(np.finfo(dtype).eps) * np.linalg.norm(A64, 1) * np.linalg.norm(X64, 1)
    return max(np.linalg.norm(A64 @ X64 - np.eye(n), 1), np.linalg.norm(X64 @ A64 - np.eye(n), 1)) / scale


def main():
    for dtype in (np.float64, np.float32):
        name = np.dtype(dtype).name
        worst_small = worst_big = worst_ld = 0.0
        for n in SIZES:
            A = rand_matrix(n, n, seed=SEEDS.get(n, 91000 + n), dtype=dtype)
            r = rho(A, np.linalg.inv(A), dtype)
            F, ipiv, info = O.lu(np.array(A, order="F"))[:3]
            d = np.diagonal(F).astype(np.float64)
            la = math.fsum(math.log(abs(float(v))) for v in d)
            sg = (-1.0) ** (int(np.sum(d < 0)) + int(np.sum(np.asarray(ipiv) != np.arange(1, n + 1))))
            s64, l64 = np.linalg.slogdet(A.astype(np.float64))
            e = abs(la - l64) / (n * float(np.finfo(dtype).eps))
            print(f"{name} n={n:5d}: LAPACK rho {r:.3e}   oracle.lu logabsdet off by {e:.3e} n eps, sign {'ok' if sg == s64 else 'DIFFERS'}")
            if n <= 2:
                worst_small = max(worst_small, r)
            else:
                worst_big = max(worst_big, r)
            worst_ld = max(worst_ld, e)
        print(f"{name}: worst LAPACK rho {worst_small:.3e} (n <= 2), {worst_big:.3e} (n >= 63); worst oracle logabsdet error {worst_ld:.3e} n eps")
        worst_b = 0.0
        for n, batch in BATCH:
            w = max(rho(A, np.linalg.inv(A), dtype) for A in (rand_matrix(n, n, seed=93000 + b, dtype=dtype) for b in range(batch)))
            print(f"{name} batch n={n:4d} x {batch}: worst LAPACK rho {w:.3e}")
            worst_b = max(worst_b, w)
        print(f"{name}: worst LAPACK rho over the batch inputs {worst_b:.3e}")


if __name__ == "__main__":
    main()
