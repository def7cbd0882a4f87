"""Shared input builders for the parity tests (mirrors of the matrices /root/reference/test/runtests.jl draws)."""
import numpy as np

import oracle as O


def rand_matrix(m, n, seed, dtype=np.float64):
    """`rand(T, m, n)` stand-in (test/runtests.jl:45) from the repo's own counter-based generator."""
    return O.np_uniform(m, n, seed, dtype)


def wilkinson(n, dtype=np.float64):
    """test/runtests.jl:130-140: unit diagonal, -1 strictly below, last column all ones (all-ties pivoting)."""
    A = np.zeros((n, n), dtype=dtype, order="F")
    A[np.arange(n), np.arange(n)] = 1
    A[:, -1] = 1
    A += np.tril(-np.ones((n, n), dtype=dtype), -1)
    return np.asfortranarray(A)


def nopivot_lu_numpy(A):
    """Textbook unpivoted right-looking LU in float64 (comparator for NoPivot info/residual)."""
    F = np.array(A, dtype=np.float64, order="F")
    m, n = F.shape
    info = 0
    for k in range(min(m, n)):
        if F[k, k] != 0:
            F[k + 1:, k] *= 1.0 / F[k, k]
        elif info == 0:
            info = k + 1
        if k + 1 < n:
            F[k + 1:, k + 1:] -= np.outer(F[k + 1:, k], F[k, k + 1:])
    return F, info


REF_SIZES = list(range(1, 11)) + [50, 130, 300]  # test/runtests.jl:39  [1:10; 50:80:200; 300]


# ---- adversarial inputs for the pivot search (tests/test_panel_edge_inputs.py proves them on the host, tests/test_gpu_panel_edges.py
# runs them through the leaf kernels and whole factorizations).  An m x n block or whole matrix, column-major, deterministic.
def _classes(m, n, seed, empty):
    """Row classes c(i) in [0, n): random, every class occurs, the classes in `empty` moved to the next one; plus the rng."""
    assert m >= n >= 2 and all(0 <= e < n - 1 for e in empty)
    rng = np.random.default_rng(seed)
    c = rng.integers(0, n, size=m)
    c[rng.choice(m, size=n, replace=False)] = np.arange(n)
    for e in sorted(empty):
        c[c == e] = e + 1
    return c, rng


def _class_matrix(c, s, n, dtype):
    m = c.size
    A = np.zeros((m, n), dtype=dtype, order="F")
    A[np.arange(m), c] = s
    A[:, n - 1] = s
    return A


def class_ties(m, n, dtype, seed, empty=()):
    """Row i has s_i = +-2^e (e in 0..2) in column c(i) and in the last column, zero elsewhere.  At step k the candidates are
    exactly the class-k rows, several of them tied at the maximum with either sign and spread over the whole height: the lowest
    CURRENT position has to win.  A row is untouched before its class column (multiplier 0) and becomes zero right of it
    afterwards (s_i - (s_i / s_p) * s_p with a power-of-two quotient), so every operation is exact: the same bits in Float32
    and Float64 and in any summation order.  `empty` classes give zero columns: info = min(empty) + 1, elimination continues."""
    c, rng = _classes(m, n, seed, empty)
    s = rng.choice([-1.0, 1.0], size=m) * 2.0 ** rng.integers(0, 3, size=m)
    return _class_matrix(c, s, n, dtype)


def near_ties(m, n, dtype, seed):
    """The structure of class_ties with s_i = +-(1 + t_i * 2^-45), t_i < 2^20 (Float64: all candidates of a column share the high
    32 bits of |a| and differ in the low word) or +-(1 + t_i * 2^-23), t_i < 64 (Float32).  The pivot sequence does not depend on
    rounding (a row is untouched until its class column); the multipliers and the last column do."""
    c, rng = _classes(m, n, seed, ())
    if np.dtype(dtype) == np.float64:
        t = rng.integers(0, 1 << 20, size=m) * 2.0 ** -45
    else:
        t = rng.integers(0, 64, size=m) * 2.0 ** -23
    s = rng.choice([-1.0, 1.0], size=m) * (1.0 + t)
    return _class_matrix(c, s, n, dtype)


def zero_columns(A, cols):
    """Copy of A with the given columns zeroed (they stay exactly zero through any elimination order)."""
    B = np.array(A, order="F", copy=True)
    B[:, list(cols)] = 0
    return B


def with_nan(A, entries):
    B = np.array(A, order="F", copy=True)
    for i, j in entries:
        B[i, j] = np.nan
    return B


def with_inf(A, entries):
    """entries: (row, column, sign)."""
    B = np.array(A, order="F", copy=True)
    for i, j, sgn in entries:
        B[i, j] = np.inf if sgn > 0 else -np.inf
    return B


def nopivot_zero_top(m, w, dtype, seed, j):
    """NoPivot block with a zero pivot at step j: top w x w block triu(rand) + 10 I with [j, j] = 0, random rows below."""
    A = rand_matrix(m, w, seed, dtype)
    A[:w] = np.triu(A[:w]) + dtype(10) * np.eye(w, dtype=dtype)
    A[j, j] = 0
    return np.asfortranarray(A.astype(dtype))

