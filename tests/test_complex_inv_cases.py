"""The exact inputs of tests/test_gpu_complex_inv.py, proven on the CPU: the constructed factors are what the issue asks for, their
inverse is certified in integer arithmetic (complex_inv_cases.exact_case does that when it builds a case), and every entry and every
partial sum of ANY blocked inverse is exactly representable in Float32 -- so comparing whole buffers with `==` is a fair demand of the
GPU, whatever its blocking and summation order."""
import math

import numpy as np
import pytest

import complex_inv_cases as C


@pytest.mark.parametrize("n", C.EXACT_SIZES)
def test_the_factors_are_as_constructed(n):
    c = C.exact_case(n)
    L, U = np.tril(c.F, -1) + np.eye(n), np.triu(c.F)
    assert np.isin(np.diagonal(U), C.DIAG).all()
    off = np.concatenate([L[np.tril_indices(n, -1)], U[np.triu_indices(n, 1)]])
    assert np.isin(off, np.concatenate([[0], C.UNITS])).all()
    # bidiagonal plus a few far entries
    far = (np.count_nonzero(np.tril(L, -2)), np.count_nonzero(np.triu(U, 2)))
    assert 4 <= far[0] <= 16 and 4 <= far[1] <= 16, far
    assert np.count_nonzero(np.diagonal(L, -1)) >= n // 2 and np.count_nonzero(np.diagonal(U, 1)) >= n // 2
    # a chain crosses every 64-row boundary
    for b in range(64, n, 64):
        assert L[b, b - 1] != 0 and U[b - 1, b] != 0, b
    # ipiv moves every row
    p = C.perm_of(c.ipiv, n)
    assert (c.ipiv[:-1] > np.arange(1, n)).all() and (p != np.arange(n)).all()
    # P A = L U, and X is the inverse (float64 evaluates these small dyadic numbers exactly)
    assert np.array_equal(c.A[p, :], L @ U)
    assert np.array_equal(c.A @ c.X, np.eye(n)) and np.array_equal(c.X @ c.A, np.eye(n))
    # det A = 2^k i^q
    s, la = np.linalg.slogdet(c.A)
    assert abs(s - c.phase) <= 1e-12 and abs(la - c.log2_absdet * math.log(2.0)) <= 1e-9
    # the conjugated factors have the conjugated inverse, which is another matrix
    assert not np.array_equal(np.conj(c.X), c.X)


@pytest.mark.parametrize("n", C.EXACT_SIZES)
def test_every_partial_sum_fits_float32(n):
    c = C.exact_case(n)
    magnitude_bits, granularity_bits = C.partial_sum_bits(c)
    print(f"n={n}: any partial sum is a multiple of 2^-{granularity_bits} below 2^{magnitude_bits}: "
          f"{magnitude_bits + granularity_bits} significant bits of Float32's 24")
    assert magnitude_bits + granularity_bits <= 24
    # and the inputs and outputs themselves survive the rounding to complex64
    for M in (c.F, c.X):
        assert np.array_equal(M.astype(np.complex64).astype(np.complex128), M)
