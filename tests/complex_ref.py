"""CPU comparator and inputs of the complex LU tests (tests/test_complex_glue.py, tests/test_gpu_complex.py).  Pure numpy, no GPU.

``complex_generic_lufact`` is an unblocked restatement of the reference's ``_generic_lufact!`` (/root/reference/src/lu.jl:290-338) for a
complex element type, in the precision of its argument: pivot = FIRST row of largest modulus ``abs(z)`` under a strict ``>`` that starts
from 0 (so a NaN modulus never wins and an all-zero column keeps row k), ``info`` set once (positive, 1-based) at the first pivot whose
two parts are zero, ``inv(pivot)`` formed once per column and one multiply per row, the rank-1 update carried on past a zero pivot.
It is NOT LAPACK's rule (``|re| + |im|``): ``scipy.linalg.lu_factor`` is a comparator for ``info`` and residuals only."""
import numpy as np

import helpers
import oracle as O

CTYPES = {"cf64": np.complex128, "cf32": np.complex64}
REAL_OF = {np.dtype(np.complex128): np.float64, np.dtype(np.complex64): np.float32}


def real_of(ctype):
    return REAL_OF[np.dtype(ctype)]


def complex_generic_lufact(A, pivot=True, moduli=False):
    """Returns (factors, ipiv (1-based int64), info[, moduli]).  ``moduli``: per step k the moduli of rows k.. of column k as the search
    saw them (a list of arrays), for the tests that have to judge a near-tie."""
    F = np.array(A, order="F", copy=True)
    assert F.dtype in REAL_OF, F.dtype
    one = F.dtype.type(1)
    m, n = F.shape
    mn = min(m, n)
    ipiv = np.arange(1, mn + 1, dtype=np.int64)
    info = 0
    seen = []
    with np.errstate(all="ignore"):
        for k in range(mn):
            kp = k
            if pivot:
                a = np.abs(F[k:, k])                       # hypot in the real precision of F
                if moduli:
                    seen.append(a.copy())
                cand = np.where(np.isnan(a), -1, a)        # `absi > amax` is false for a NaN
                j = int(np.argmax(cand))                   # first maximum: the lowest row wins a tie
                if cand[j] > 0:
                    kp = k + j
                ipiv[k] = kp + 1
            if F[kp, k] != 0:                              # iszero: both parts
                if kp != k:
                    F[[k, kp], :] = F[[kp, k], :]
                F[k + 1:, k] *= one / F[k, k]
            elif info == 0:
                info = k + 1
            if k + 1 < n and k + 1 < m:
                F[k + 1:, k + 1:] -= np.outer(F[k + 1:, k], F[k, k + 1:])
    return (F, ipiv, info, seen) if moduli else (F, ipiv, info)


def parts(Z):
    """A complex array as its real numbers (re, im interleaved along the last axis of a contiguous copy)."""
    Z = np.ascontiguousarray(Z)
    return Z.view(real_of(Z.dtype))


def bits(Z):
    """The words of a complex or real array, for comparisons that tell -0 from +0."""
    Z = np.ascontiguousarray(Z)
    return Z.view(np.uint64 if Z.dtype in (np.complex128, np.float64) else np.uint32)


def perm_of(ipiv, m):
    p = np.arange(m)
    for i, t in enumerate(np.asarray(ipiv)):
        j = int(t) - 1
        if j != i:
            p[i], p[j] = p[j], p[i]
    return p


def split_lu(F):
    F = np.asarray(F).astype(np.complex128)
    m, n = F.shape
    k = min(m, n)
    return np.tril(F[:, :k], -1) + np.eye(m, k), np.triu(F[:k, :])


def residual_inf(A, F, ipiv):
    """||L*U - A[p,:]||_inf evaluated in complex128 (the reference's check, test/runtests.jl:21-31)."""
    L, U = split_lu(F)
    A = np.asarray(A).astype(np.complex128)
    return float(np.linalg.norm(L @ U - A[perm_of(ipiv, A.shape[0]), :], np.inf))


def residual_fro_rel(A, F, ipiv):
    """||L*U - A[p,:]||_F / ||A||_F evaluated in complex128."""
    L, U = split_lu(F)
    A = np.asarray(A).astype(np.complex128)
    return float(np.linalg.norm(L @ U - A[perm_of(ipiv, A.shape[0]), :]) / np.linalg.norm(A))


def rand_complex(m, n, ctype, seed0=12):
    """The random input of the issue: re and im from the repo's counter generator, seeds seed0 + m + n and 1000 + seed0 + m + n."""
    real = real_of(ctype)
    A = O.np_uniform(m, n, seed0 + m + n, real) + 1j * O.np_uniform(m, n, 1000 + seed0 + m + n, real)
    return np.asfortranarray(A.astype(ctype))


def rand_rhs(n, nrhs, ctype):
    real = real_of(ctype)
    B = O.np_uniform(n, nrhs, 99 + n, real) + 1j * O.np_uniform(n, nrhs, 1099 + n, real)
    return np.asfortranarray(B.astype(ctype))


EXACT_CASES = [(70, 64, ()), (200, 130, (5, 77)), (300, 300, ()), (129, 65, (63,))]
EXACT_INFO = [0, 6, 0, 64]


def exact_complex(m, n, empty, ctype):
    """helpers.class_ties with row i turned by a unit of {1, i, -1, -i}: every modulus is a power of two, every quotient a power of two
    times a unit, every product of the elimination has a zero factor -- all operations are exact in both precisions and any order."""
    T = helpers.class_ties(m, n, np.float64, seed=7 + m, empty=empty)
    units = np.array([1, 1j, -1, -1j])[np.random.default_rng(1000 + m).integers(0, 4, size=m)]
    return np.asfortranarray((T.astype(np.complex128) * units[:, None]).astype(ctype))


# shapes of the factorization tests
REF_SHAPES = [(s, s) for s in helpers.REF_SIZES] + [(s, s + 2) for s in helpers.REF_SIZES]   # test/runtests.jl:39-45
EXTRA_SHAPES = [(63, 63), (64, 64), (65, 65), (127, 129), (128, 128), (129, 131), (302, 300),   # leaf and split boundaries
                (2100, 70), (70, 2100),                                                         # a tall leaf that streams; the fat tail
                (777, 650), (650, 777)]                                                         # three levels, interior and edge GEMM tiles
