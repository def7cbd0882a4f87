#!/usr/bin/env python
"""CPU margins of tests/test_gpu_complex_inv.py, on exactly the tests' inputs (tests/complex_inv_cases.py).  No GPU.

  1. rho_R / rho_L of numpy.linalg.inv (LAPACK zgetri / cgetri) for every size and both complex types, against the tests' bars;
  2. with --logabs, on logdet_input's column-scaled matrices: |sum log|u_ii| - slogdet(A)| / (n eps_T) for the factors of
     tests/complex_ref.py's unblocked elimination in the element type (the GPU's pivot rule), against the tests' absolute bar of
     8 n eps_T; and, where scipy is installed, the reference's own error: slogdet(A) against math.fsum over the diagonal of
     scipy.linalg.lu_factor's factors, with the largest partial sum of the logs.

    python scripts/complex_inv_cpu_bars.py [--logabs]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import complex_inv_cases as C  # noqa: E402


def main():
    for ctype in C.CDTYPES:
        name = np.dtype(ctype).name
        print(f"{name}: numpy.linalg.inv, max(rho_R, rho_L)")
        worst_large = 0.0
        for n in C.SIZES:
            for diag in ((False, True) if n in C.VARIANT_SIZES else (False,)):
                A = C.rand_matrix(n, ctype, diag)
                X = np.linalg.inv(A)
                assert X.dtype == np.dtype(ctype)
                r, l = C.rho(A, X, ctype)
                ok = "ok" if max(r, l) <= C.rho_bar(n) else "EXCEEDS THE BAR: change the seed (SEEDS in tests/complex_inv_cases.py)"
                print(f"  n={n:5d}{' +nI' if diag else '    '} rho_R={r:.4f} rho_L={l:.4f} bar={C.rho_bar(n):.0f} {ok}")
                if n >= 63:
                    worst_large = max(worst_large, r, l)
        print(f"  worst for n >= 63: {worst_large:.4f}")
    if "--logabs" in sys.argv:
        import complex_ref as R

        for ctype in C.CDTYPES:
            eps = float(np.finfo(C.real_of(ctype)).eps)
            print(f"{np.dtype(ctype).name}: unblocked elimination in the element type against slogdet in complex128, in units of n eps_T (bar 8)")
            for n in C.SIZES:
                A = C.logdet_input(n, ctype)
                F, ipiv, info = R.complex_generic_lufact(A)
                d = np.diagonal(F).astype(np.complex128)
                la = float(np.sum(np.log(np.hypot(d.real, d.imag))))
                _, want = np.linalg.slogdet(A.astype(np.complex128))
                line = f"  n={n:5d} |d| = {abs(la - want) / (n * eps):.3f} n eps"
                try:
                    import math

                    import scipy.linalg as sl

                    logs = [math.log(math.hypot(z.real, z.imag)) for z in np.diagonal(sl.lu_factor(A.astype(np.complex128))[0])]
                    line += (f"; slogdet - fsum over LAPACK's diagonal = {(want - math.fsum(logs)) / (n * np.finfo(np.float64).eps):+.3f} n eps64, "
                             f"largest partial sum {np.abs(np.cumsum(logs)).max():.1f}")
                except ImportError:
                    pass
                print(line)


if __name__ == "__main__":
    main()
