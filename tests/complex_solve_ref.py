"""CPU comparator, inputs and bars of the complex transposed / adjoint solve tests (tests/test_complex_adjoint_glue.py,
tests/test_gpu_complex_adjoint.py).  Pure numpy, no GPU.

``trans_solve`` restates ``ldiv!(transpose(F), B)`` (conj = 0, LAPACK 'T') and ``ldiv!(F', B)`` (conj = 1, LAPACK 'C') on packed factors
in the precision of its arguments: a forward solve with U^T (lower, stored diagonal), a backward solve with L^T (upper, unit diagonal),
then the interchanges undone LAST FIRST (ipiv repeats targets, so the order matters).  The adjoint conjugates the factors."""
import functools

import numpy as np

import complex_ref as CR
import helpers


def op(A, conj):
    """transpose(A) or A' in complex128: what the solves invert."""
    A = np.asarray(A).astype(np.complex128)
    return A.conj().T if conj else A.T


def trans_solve(F, ipiv, B, conj, first_to_last=False):
    """X with op(A) X = B from the packed factors F and ipiv (1-based; None = NotIPIV).  ``first_to_last`` undoes the interchanges in the
    WRONG order, for the test that shows the order matters."""
    F = np.asarray(F)
    n = F.shape[0]
    X = np.array(B, copy=True).reshape(n, -1)
    assert X.dtype == F.dtype
    V = F.conj().T if conj else F.T          # row i of V is column i of F: lower triangle = U^T, strict upper = L^T
    with np.errstate(all="ignore"):
        for i in range(n):                   # U^T y = b
            X[i] = (X[i] - V[i, :i] @ X[:i]) / V[i, i]
        for i in range(n - 2, -1, -1):       # L^T z = y
            X[i] = X[i] - V[i, i + 1:] @ X[i + 1:]
    if ipiv is not None:
        ks = range(n) if first_to_last else range(n - 1, -1, -1)
        for k in ks:
            p = int(ipiv[k]) - 1
            if p != k:
                X[[k, p]] = X[[p, k]]
    return X.reshape(np.shape(B))


def backward_error(A, X, B, conj):
    """||op(A) X - B||_inf / (||op(A)||_inf ||X||_inf) in complex128."""
    M = op(A, conj)
    X = np.asarray(X).astype(np.complex128).reshape(M.shape[0], -1)
    B = np.asarray(B).astype(np.complex128).reshape(M.shape[0], -1)
    return float(np.linalg.norm(M @ X - B, np.inf) / (np.linalg.norm(M, np.inf) * np.linalg.norm(X, np.inf)))


def eps_of(ctype):
    return float(np.finfo(CR.real_of(ctype)).eps)


def bar_E(n, ctype):
    """The project's bar, test/runtests.jl:19: E = 20 n eps."""
    return 20 * n * eps_of(ctype)


# ---- shapes -----------------------------------------------------------------------------------------------------------------------------
# the reference's sizes, the leaf (32), split (64, 128) and CNB (256) boundaries; 650: three levels with interior and edge GEMM tiles
BE_SIZES = sorted(set(helpers.REF_SIZES) | {31, 32, 33, 63, 64, 65, 96, 130, 255, 256, 257, 300, 513, 650})


def be_nrhs(n):
    """8 | 9 is the narrow / wide boundary, 130 crosses the base kernel's 128-column workgroup."""
    return (1, 2, 8, 9, 33, 130) if n <= 130 else (1, 8, 9, 130)


NOPIV_SIZES = (8, 30, 64, 200, 300)
NOPIV_NRHS = (1, 3)


@functools.lru_cache(maxsize=None)
def rand_input(n, ctype):
    A = CR.rand_complex(n, n, ctype)
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def rand_factors(n, ctype):
    """The restatement's pivoted factors of ``rand_input``: (F, ipiv).  Computed once, never modified."""
    F, ipiv, info = CR.complex_generic_lufact(rand_input(n, ctype), True)
    assert info == 0
    F.setflags(write=False)
    ipiv.setflags(write=False)
    return F, ipiv


@functools.lru_cache(maxsize=None)
def nopivot_input(n, ctype):
    """test/runtests.jl:116-128: A + 10 I."""
    A = np.asfortranarray((CR.rand_complex(n, n, ctype) + 10 * np.eye(n)).astype(ctype))
    A.setflags(write=False)
    return A


def nopivot_rhs(n, nrhs, ctype):
    return CR.rand_rhs(n, nrhs, ctype)


# ---- the exact input: order of the interchanges and the conjugation -----------------------------------------------------------------------
EXACT_N, EXACT_SHIFT = 130, 37


def exact_input(ctype, seed=2024):
    """A[i, (i + 37) mod 130] = u_i 2^e_i with u_i in {1, i, -1, -i} and e_i in -3 .. 3, every other entry zero: a scaled permutation.
    Every operation of the factorization and of the solves is exact in both precisions and in any order."""
    n = EXACT_N
    rng = np.random.default_rng(seed)
    u = np.array([1, 1j, -1, -1j])[rng.integers(0, 4, size=n)]
    e = rng.integers(-3, 4, size=n)
    A = np.zeros((n, n), dtype=np.complex128, order="F")
    A[np.arange(n), (np.arange(n) + EXACT_SHIFT) % n] = u * np.exp2(e)
    return np.asfortranarray(A.astype(ctype))


def exact_rhs(nrhs, ctype, seed=77):
    """Parts that are small integers (-8 .. 8)."""
    rng = np.random.default_rng(seed + nrhs)
    B = rng.integers(-8, 9, size=(EXACT_N, nrhs)) + 1j * rng.integers(-8, 9, size=(EXACT_N, nrhs))
    return np.asfortranarray(B.astype(ctype))


def exact_solution(A, B, conj):
    """X[i] = B[(i + 37) mod 130] / A[i, (i + 37) mod 130], the divisor conjugated for the adjoint."""
    n = EXACT_N
    j = (np.arange(n) + EXACT_SHIFT) % n
    d = A[np.arange(n), j]
    if conj:
        d = d.conj()
    return (B[j, :] / d[:, None]).astype(A.dtype)
