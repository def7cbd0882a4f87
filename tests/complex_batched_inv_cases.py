"""Inputs, the CPU restatement and the bars of the complex batched inverse tests (tests/test_complex_batched_inv_cases.py,
tests/test_gpu_complex_batched_inv.py).  Pure numpy, no GPU.

Inputs: matrix b of a batch is ``complex_batched_cases.matrix(n, n, sfx, b)``; the exact inputs are ``complex_inv_cases.exact_case``.
Residual and bar: ``complex_inv_cases.rho`` (LAPACK's xGET03 ratios, evaluated in complex128; the larger of the right and the left one,
against op(A_b)) and ``complex_inv_cases.rho_bar(n)``: 1.0 for n >= 4, 4.0 for n <= 3.

``restatement`` is cgetri_batched_kernel (csrc/batched_complex.hip) in numpy: the columns of P * I, the column-oriented forward
substitution with the unit lower triangle, the column-oriented backward substitution with the upper one, ONE reciprocal per diagonal
entry by Smith's formula and multiplies from then on, everything in the element's own precision.  The order of the operations on one
element is the kernel's; whether a product and a difference are contracted into one fused operation is the compiler's choice and is
not restated (it moves single roundings, and nothing where every operation is exact)."""
import math

import numpy as np

import complex_batched_cases as CB
import complex_inv_cases as CI
import complex_ref as CR

CTYPES = CB.CTYPES
LIMIT = CB.LIMIT                                     # one launch up to here
# 32 | 33 and 64 | 65: the group of threads doubles; 7 | 8 and 63 | 64: the last pass of 8 columns is partial or full; the limits
SIZES = {"cf64": [1, 2, 3, 7, 8, 31, 32, 33, 63, 64], "cf32": [1, 2, 3, 7, 8, 31, 32, 33, 63, 64, 65, 100, 127, 128]}
BATCH = 67                                           # the last workgroup is partly empty for 4, 2 and 1 groups per workgroup
SMALL_BATCHES = (1, 7)                               # at SMALL_BATCH_SIZES only
SMALL_BATCH_SIZES = (33, 64)
EXACT_SIZES = {"cf64": [8, 33, 64], "cf32": [8, 33, 64, 65, 128]}
EXACT_COPIES = 5
FALLBACK = {"cf64": 65, "cf32": 129}                 # one past the limit: the loop over the single-matrix path
FALLBACK_BATCH = 3
NOPIVOT_SIZES = (33, 64)
NOPIVOT_BATCH = 7
LETTERS = ("N", "T", "C")


def op(A, letter):
    """op(A) by LAPACK's letter."""
    A = np.asarray(A)
    return A if letter == "N" else (A.T if letter == "T" else A.conj().T)


def worst_rho(A, X, sfx, letter="N"):
    """The larger of the right and the left residual of op(A) against X."""
    return max(CI.rho(op(A, letter), X, CTYPES[sfx]))


def reciprocal(d):
    """cdiv({1, 0}, d) of csrc/complex_dev.hpp, entry by entry, in the precision of ``d``: Smith's formula with one real reciprocal;
    both parts zero give (1 / 0, 0 / 0) = (Inf, NaN)."""
    d = np.asarray(d)
    real = CR.real_of(d.dtype)
    re, im = d.real.astype(real), d.imag.astype(real)
    one, zero = real(1), real(0)
    out = np.empty(d.shape, dtype=d.dtype)
    with np.errstate(all="ignore"):
        big_re = np.abs(re) >= np.abs(im)
        # |re| >= |im|
        rat = im / re
        scl = one / (re + im * rat)
        a_re, a_im = (one + zero * rat) * scl, (zero - one * rat) * scl
        both = (re == 0) & (im == 0)
        a_re = np.where(both, one / np.abs(re), a_re)
        a_im = np.where(both, zero / np.abs(im), a_im)
        # |re| < |im|
        rat2 = re / im
        scl2 = one / (re * rat2 + im)
        b_re, b_im = (one * rat2 + zero) * scl2, (zero * rat2 - one) * scl2
    out.real = np.where(big_re, a_re, b_re)
    out.imag = np.where(big_re, a_im, b_im)
    return out


def restatement(F, ipiv):
    """inv(A) from packed factors (and 1-based interchanges, None = NotIPIV) in the kernel's order and in the precision of ``F``."""
    F = np.asarray(F)
    n = F.shape[0]
    ctype = F.dtype.type
    perm = CR.perm_of(ipiv, n) if ipiv is not None else np.arange(n)
    X = np.zeros((n, n), dtype=F.dtype)
    X[np.arange(n), perm] = ctype(1)                 # row i of P * I is row perm[i] of I
    D = reciprocal(np.diagonal(F))
    with np.errstate(all="ignore"):
        for k in range(n):                           # L (unit) forward: x_k is final, every row below takes it out
            X[k + 1:] = X[k + 1:] - F[k + 1:, k:k + 1] * X[k:k + 1]
        for k in range(n - 1, -1, -1):               # U backward: x_k / u_kk as a product, taken out of every row above; row k is scaled last
            xk = X[k] * D[k]
            X[:k] = X[:k] - F[:k, k:k + 1] * xk[None, :]
        X = X * D[:, None]
    assert X.dtype == F.dtype
    return X


def exact_factors(n, sfx):
    """(F, ipiv, c) of complex_inv_cases.exact_case(n) with the factors cast to the element type -- exactly: every entry is a Gaussian
    dyadic rational with a handful of bits."""
    c = CI.exact_case(n)
    F = np.asfortranarray(c.F.astype(CTYPES[sfx]))
    assert np.array_equal(F.astype(np.complex128), c.F)
    return F, c.ipiv, c


def exact_inverse(c, sfx, letter):
    """X, X.T or X.conj().T of the exact case, cast to the element type (exactly)."""
    X = op(c.X, letter).astype(CTYPES[sfx])
    assert np.array_equal(X.astype(np.complex128), op(c.X, letter))
    return X


def half_bar(n):
    """What the restatement alone has to meet: half the bar for n >= 2, the bar itself at n = 1 (one reciprocal and nothing else: the
    residual is that of a single rounded complex reciprocal, which reaches 1.03 of n eps |a| |x|)."""
    return CI.rho_bar(n) if n == 1 else 0.5 * CI.rho_bar(n)


def finite(X):
    return bool(np.isfinite(np.asarray(X)).all())


assert all(max(v) == LIMIT[s] and FALLBACK[s] == LIMIT[s] + 1 for s, v in SIZES.items()) and not math.isnan(CI.rho_bar(1))
