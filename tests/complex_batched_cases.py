"""Inputs, CPU comparators and bars of the complex batched LU / solve tests (tests/test_complex_batched_cases.py,
tests/test_gpu_complex_batched.py).  Pure numpy, no GPU.

Matrix b of a batch is ``complex_ref.rand_complex(m, n, ctype, seed0=12 + 37 * b)``; its right-hand sides are built like
``complex_ref.rand_rhs`` with the seeds moved by 37 * b.  The comparator of ``ipiv`` / ``info`` / factors is
``complex_ref.complex_generic_lufact`` (the CPU restatement of the reference's rule); LAPACK's ``|re| + |im|`` is not."""
import functools

import numpy as np

import complex_ref as CR
import complex_solve_ref as CSR
import oracle as O

CTYPES = CR.CTYPES
SHAPES = {
    "cf64": [(1, 1), (7, 9), (10, 12), (32, 32), (33, 31), (50, 52), (64, 60), (64, 64)],
    "cf32": [(1, 1), (7, 9), (10, 12), (32, 32), (33, 31), (50, 52), (64, 60), (64, 64), (65, 65), (100, 60), (60, 100), (127, 128), (128, 128)],
}
FALLBACK = {"cf64": (65, 65), "cf32": (129, 129)}     # one past the one-launch limit: the loop over the single-matrix path
LIMIT = {"cf64": 64, "cf32": 128}
BATCHES = (1, 7, 67)                                  # the last workgroup is partly empty for 4, 2 and 1 groups per workgroup
NRHS = (1, 8, 9)                                      # 8 | 9: the pass boundary of the solve kernel
SQUARE = {s: [sh[0] for sh in SHAPES[s] if sh[0] == sh[1]] for s in SHAPES}
# (shape, empty classes, element types, expected info) of the exact inputs
EXACT = [((17, 9), (3,), ("cf64", "cf32"), 4), ((33, 31), (), ("cf64", "cf32"), 0), ((64, 60), (5,), ("cf64", "cf32"), 6),
         ((64, 64), (62,), ("cf64", "cf32"), 63), ((128, 100), (5, 77), ("cf32",), 6), ((128, 128), (), ("cf32",), 0)]


def eps_of(sfx):
    return CSR.eps_of(CTYPES[sfx])


def matrix(m, n, sfx, b):
    return CR.rand_complex(m, n, CTYPES[sfx], seed0=12 + 37 * b)


@functools.lru_cache(maxsize=None)
def _host_batch(m, n, sfx, batch):
    out = np.stack([matrix(m, n, sfx, b) for b in range(batch)])
    out.setflags(write=False)
    return out


def host_batch(m, n, sfx, batch):
    """(batch, m, n), read-only; a smaller batch is the head of the largest one."""
    return _host_batch(m, n, sfx, max(BATCHES))[:batch] if batch <= max(BATCHES) else _host_batch(m, n, sfx, batch)


def rhs(n, nrhs, sfx, b):
    real = CR.real_of(CTYPES[sfx])
    B = O.np_uniform(n, nrhs, 99 + n + 37 * b, real) + 1j * O.np_uniform(n, nrhs, 1099 + n + 37 * b, real)
    return B.astype(CTYPES[sfx])


@functools.lru_cache(maxsize=None)
def rhs_batch(n, nrhs, sfx, batch):
    out = np.stack([rhs(n, nrhs, sfx, b) for b in range(batch)])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def ref_factors(m, n, sfx, b, pivot=True):
    """The restatement on matrix b in the precision of the input: (factors, ipiv, info).  Computed once, never modified."""
    F, ip, info = CR.complex_generic_lufact(matrix(m, n, sfx, b), pivot)
    F.setflags(write=False)
    ip.setflags(write=False)
    return F, ip, info


def nopivot_matrix(n, sfx, b):
    """test/runtests.jl:116-128: rand + 10 I."""
    return np.asfortranarray((matrix(n, n, sfx, b) + 10 * np.eye(n)).astype(CTYPES[sfx]))


# ---- pivot forks ----------------------------------------------------------------------------------------------------------------------
def min_relative_gap(A):
    """Over the steps of the restatement on A: the smallest (largest - second largest) / largest modulus the search saw (steps with a
    single candidate do not count).  The room a rounding difference has before it changes a pivot."""
    _, _, _, mods = CR.complex_generic_lufact(A, True, moduli=True)
    worst = np.inf
    for a in mods:
        if a.size < 2:
            continue
        top = np.sort(a.astype(np.float64))[-2:]
        if top[1] > 0:
            worst = min(worst, float((top[1] - top[0]) / top[1]))
    return worst


@functools.lru_cache(maxsize=None)
def ref128_of_cf32(m, n, b):
    """The restatement in complex128 on the Float32-valued matrix b: (ipiv, moduli seen per step).  Computed once, never modified."""
    _, ip, _, mods = CR.complex_generic_lufact(matrix(m, n, "cf32", b).astype(np.complex128), True, moduli=True)
    return ip, mods


def check_ipiv_cf32(A32, ipiv_dev, ref128=None):
    """The fork rule of tests/test_gpu_complex.py, restated: ``ipiv_dev`` equals the restatement run in complex128 on the Float32-valued
    input up to the first difference; there the device's choice holds at least (1 - 8 m eps32) of the largest modulus the restatement
    saw.  ``ref128``: that restatement's (ipiv, moduli) where the caller has it already.  Returns the fork step or None."""
    m = A32.shape[0]
    if ref128 is None:
        _, ip, _, mods = CR.complex_generic_lufact(np.asarray(A32).astype(np.complex128), True, moduli=True)
    else:
        ip, mods = ref128
    diff = np.flatnonzero(ip != np.asarray(ipiv_dev))
    if diff.size == 0:
        return None
    k = int(diff[0])
    a = mods[k]
    j = int(ipiv_dev[k]) - 1 - k
    assert 0 <= j < a.size, (k, int(ipiv_dev[k]))
    assert a[j] >= (1 - 8 * m * eps_of("cf32")) * np.nanmax(a), (k, a[j], np.nanmax(a))
    return k


# ---- solves ---------------------------------------------------------------------------------------------------------------------------
TRANS = {"N": None, "T": 0, "C": 1}     # the `conj` argument of complex_solve_ref for the two transposed operators


def forward_solve(F, ipiv, B):
    """ldiv!(F, B) on packed factors in the precision of its arguments: P B, then L (unit) forward and U backward."""
    F = np.asarray(F)
    n = F.shape[0]
    X = np.array(B, copy=True).reshape(n, -1)
    assert X.dtype == F.dtype
    if ipiv is not None:
        X = X[CR.perm_of(ipiv, n)]
    with np.errstate(all="ignore"):
        for i in range(1, n):
            X[i] = X[i] - F[i, :i] @ X[:i]
        for i in range(n - 1, -1, -1):
            X[i] = (X[i] - F[i, i + 1:] @ X[i + 1:]) / F[i, i]
    return X.reshape(np.shape(B))


def ref_solve(F, ipiv, B, trans):
    return forward_solve(F, ipiv, B) if trans == "N" else CSR.trans_solve(F, ipiv, B, TRANS[trans])


def backward_error(A, X, B, trans):
    """||op(A) X - B||_inf / (||op(A)||_inf ||X||_inf) in complex128, op by LAPACK's letter."""
    if trans == "N":
        M = np.asarray(A).astype(np.complex128)
        X = np.asarray(X).astype(np.complex128).reshape(M.shape[0], -1)
        B = np.asarray(B).astype(np.complex128).reshape(M.shape[0], -1)
        return float(np.linalg.norm(M @ X - B, np.inf) / (np.linalg.norm(M, np.inf) * np.linalg.norm(X, np.inf)))
    return CSR.backward_error(A, X, B, TRANS[trans])


def bar_E(n, sfx):
    return CSR.bar_E(n, CTYPES[sfx])
