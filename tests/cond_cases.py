"""Inputs and CPU references of the norm / condition-estimate tests (tests/test_cond_cases.py, tests/test_gpu_cond.py).  Pure numpy /
scipy, no GPU, no torch.

  * kernel_sum, first_argmax, sign_vector, estimate, rcond_restatement: the estimator of rflu_gecon_* restated in the kernels' own order
    -- Higham's method as LAPACK xLACN2 runs it, with the two changes include/rflu.h states (all-ones start vector with est = sum / n,
    integer alternating vector (-1)^i (n - 1 + i) with the bound 2 sum / (3 n (n - 1))), sign(v) = v >= 0 ? +1 : -1, the FIRST index of
    the maximum, and every sum of moduli in Float64 by the chunking of cond_stats_kernel (csrc/condest.hip): chunks of 1024, thread t of
    256 adds entries t, t + 256, t + 512, t + 768 in that order, the tree adds t and t + s for s = 128 .. 1, chunk sums in index order.
    The batched kernel's tree (t and t + s for s = 64 .. 1 on n <= 128 values) is this tree with its zero additions left out;
  * the random inputs: uniform(-1, 1), column-graded by 2^-k with k in [0, 10), a Hilbert-like matrix with a perturbation;
  * the exact inputs: exact_factors -- inv_cases.exact_case's constructed L and U, thinned to integer inverses, with an integer-certified
    inverse -- and vector_bits, the
    sum-of-moduli certificate that every number ANY blocked substitution forms on ANY vector the estimator can send into a solve (ones,
    +-1, e_j, the alternating vector) is exactly representable in Float32.
"""
import functools
import math

import numpy as np
import scipy.linalg as sla

from complex_inv_cases import _gran_bits
from inv_cases import exact_case

CS_CHUNK, CS_THREADS = 1024, 256          # csrc/condest.hip (asserted against the source in tests/test_cond_cases.py)
MAX_ROUNDS = 5                             # xLACN2's ITMAX
NORM_ONE, NORM_INF = 1, 2                  # enum rflu_norm

GECON_SIZES = [1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 2112]
BATCHED_SIZES = [1, 2, 3, 7, 8, 31, 32, 33, 63, 64, 65, 127, 128]
BATCHES = [67, 7, 1]
FAMILIES = ["uniform", "graded", "hilbert"]


# ---- the kernels' arithmetic -------------------------------------------------------------------------------------------------------
def kernel_sum(absvals, drop_chunk=None):
    """Float64 sum of non-negative values in the order of cond_stats_kernel / cond_final_kernel.  drop_chunk (a planted fault): that
    chunk's sum is left out."""
    a = np.asarray(absvals, dtype=np.float64)
    n = a.size
    acc = None
    for c, c0 in enumerate(range(0, n, CS_CHUNK)):
        buf = np.zeros(CS_CHUNK)
        piece = a[c0:c0 + CS_CHUNK]
        buf[:piece.size] = piece
        per = buf.reshape(CS_CHUNK // CS_THREADS, CS_THREADS)
        v = np.zeros(CS_THREADS)
        for k in range(per.shape[0]):          # four entries per thread in index order
            v = v + per[k]
        s = CS_THREADS // 2
        while s > 0:                           # the LDS tree
            v[:s] = v[:s] + v[s:2 * s]
            s //= 2
        if c == drop_chunk:
            continue
        acc = v[0] if acc is None else acc + v[0]
    return np.float64(0.0 if acc is None else acc)


def first_argmax(absvals, last=False):
    """First index of the maximum (last=True: a planted fault)."""
    a = np.asarray(absvals, dtype=np.float64)
    if last:
        return int(a.size - 1 - np.argmax(a[::-1]))
    return int(np.argmax(a))


def sign_vector(x, zero_is_negative=False):
    """sign(v) = v >= 0 ? +1 : -1 in the type of x (zero_is_negative: a planted fault)."""
    pos = (x > 0) if zero_is_negative else (x >= 0)
    return np.where(pos, 1, -1).astype(x.dtype)


def alternating(n, dtype):
    i = np.arange(n)
    return (np.where(i % 2 == 1, -1.0, 1.0) * (n - 1 + i)).astype(dtype)


def estimate(apply_m, apply_mt, n, dtype, fault=None, trace=None):
    """The estimate of ||M||_1 from x -> M x (apply_m) and x -> M^T x (apply_mt), both taking and returning arrays of `dtype`.
    Returns (est, solves); est is None when a vector came back non-finite.  trace (a list) receives every vector sent into a solve as
    (transposed, vector).  fault: None or one of "sign_of_zero", "last_argmax", "no_closing", "drop_chunk"."""
    drop = 1 if fault == "drop_chunk" else None
    solves = 0

    def run(op, x, transposed):
        nonlocal solves
        solves += 1
        if trace is not None:
            trace.append((transposed, x.copy()))
        y = np.asarray(op(x), dtype=dtype)
        return y, bool(np.isfinite(y.astype(np.float64)).all())

    x, ok = run(apply_m, np.ones(n, dtype=dtype), False)
    if not ok:
        return None, solves
    est = kernel_sum(np.abs(x.astype(np.float64)), drop) / np.float64(n)
    if n == 1:
        return est, solves
    closing = False
    j = 0
    sgn = None
    for rnd in range(MAX_ROUNDS):
        if rnd > 0:
            e = np.zeros(n, dtype=dtype)
            e[j] = 1
            x, ok = run(apply_m, e, False)
            if not ok:
                return None, solves
            est_old = est
            est = kernel_sum(np.abs(x.astype(np.float64)), drop)
            if np.array_equal(sign_vector(x, fault == "sign_of_zero"), sgn) or est <= est_old:
                closing = True
                break
        sgn = sign_vector(x, fault == "sign_of_zero")
        x, ok = run(apply_mt, sgn.copy(), True)
        if not ok:
            return None, solves
        ax = np.abs(x.astype(np.float64))
        jlast, j = j, first_argmax(ax, last=(fault == "last_argmax"))
        if (rnd > 0 and ax[jlast] == ax[j]) or rnd == MAX_ROUNDS - 1:
            closing = True
            break
    if closing and fault != "no_closing":
        x, ok = run(apply_m, alternating(n, dtype), False)
        if not ok:
            return None, solves
        alt = np.float64(2.0) * kernel_sum(np.abs(x.astype(np.float64)), drop) / (np.float64(3.0) * np.float64(n) * np.float64(n - 1))
        if alt > est:
            est = alt
    return est, solves


def triangular_solvers(F, dtype):
    """(x -> U^-1 L^-1 x, x -> L^-T U^-T x) by substitution in `dtype` on the packed factors F."""
    Fd = np.asarray(F, dtype=dtype)

    def m(x):
        with np.errstate(all="ignore"):
            y = sla.solve_triangular(Fd, x.astype(dtype), lower=True, unit_diagonal=True, check_finite=False)
            return sla.solve_triangular(Fd, y, lower=False, check_finite=False)

    def mt(x):
        with np.errstate(all="ignore"):
            y = sla.solve_triangular(Fd, x.astype(dtype), lower=False, trans=1, check_finite=False)
            return sla.solve_triangular(Fd, y, lower=True, unit_diagonal=True, trans=1, check_finite=False)

    return m, mt


def rcond_restatement(F, norm, anorm, dtype, solvers=None, fault=None, detail=False):
    """rflu_gecon_* on the packed factors F (a matrix, whatever its storage was).  solvers: (x -> M x, x -> M^T x), default: substitution
    in `dtype`.  fault "swap_inf" (planted) does not swap M and M^T for the Inf norm.  detail=True returns (rcond, est, solves)."""
    n = F.shape[0]
    out = lambda rc, est=None, solves=0: (rc, est, solves) if detail else rc   # noqa: E731
    if n == 0:
        return out(1.0)
    anorm = float(anorm)
    if anorm != anorm:
        return out(math.nan)
    if anorm == 0.0:
        return out(0.0)
    d = np.diagonal(F)
    if (d == 0).any():
        return out(0.0)
    if np.isnan(np.asarray(F, dtype=np.float64)).any():
        return out(math.nan)
    m, mt = solvers if solvers is not None else triangular_solvers(F, dtype)
    if norm == NORM_INF and fault != "swap_inf":
        m, mt = mt, m
    est, solves = estimate(m, mt, n, dtype, fault=fault)
    if est is None or est == 0.0:
        return out(0.0, est, solves)
    return out(float(np.float64(1.0) / (np.float64(anorm) * np.float64(est))), float(est), solves)


# ---- the random inputs -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _random(family, n, seed, dtype):
    rng = np.random.default_rng([20260, FAMILIES.index(family), n, seed])
    A = rng.uniform(-1.0, 1.0, size=(n, n))
    if family == "graded":
        A = A * 2.0 ** -rng.integers(0, 10, size=n)[None, :]
    elif family == "hilbert":
        i = np.arange(n)
        A = 1.0 / (1.0 + i[:, None] + i[None, :]) + 1e-3 * A + np.eye(n)
    A = np.asfortranarray(A.astype(dtype))
    A.setflags(write=False)
    return A


def random_matrix(family, n, seed, dtype):
    """uniform: uniform(-1, 1); graded: its columns scaled by 2^-k, k in [0, 10); hilbert: 1 / (1 + i + j) + I + 1e-3 uniform."""
    return _random(family, int(n), int(seed), np.dtype(dtype).type)


def true_inverse_norms(A):
    """{norm: ||A^-1||} in Float64 from the Float64 image of A (one inversion for both norms)."""
    X = np.linalg.inv(np.asarray(A, dtype=np.float64))
    return {NORM_ONE: float(np.linalg.norm(X, 1)), NORM_INF: float(np.linalg.norm(X, np.inf))}


def true_inverse_norm(A, norm):
    return true_inverse_norms(A)[norm]


def lapack_factors(A):
    """(packed L\\U, 0-based pivots) of LAPACK getrf in the element type of A."""
    lu, piv = sla.lu_factor(np.array(A, order="F"), check_finite=False)
    return lu, piv


def lapack_gecon(lu, anorm, norm):
    """LAPACK's own estimate of ||A^-1|| from its factors: 1 / (rcond * anorm)."""
    fn = sla.lapack.dgecon if lu.dtype == np.float64 else sla.lapack.sgecon
    rc, info = fn(lu, anorm, norm=b"1" if norm == NORM_ONE else b"I")
    assert info == 0
    return 1.0 / (float(rc) * float(anorm))


@functools.lru_cache(maxsize=None)
def _kept(family, n, seed, dtype):
    A = random_matrix(family, n, seed, dtype)
    lu, _ = lapack_factors(A)
    LU = (np.tril(lu.astype(np.float64), -1) + np.eye(n)) @ np.triu(lu.astype(np.float64))
    true = true_inverse_norms(LU)
    for norm in (NORM_ONE, NORM_INF):
        anorm = float(np.linalg.norm(LU, 1 if norm == NORM_ONE else np.inf))
        if lapack_gecon(lu, anorm, norm) < 0.5 * true[norm]:
            return False
    return True


def kept(family, n, seed, dtype):
    """Is this input one on which the reference -- LAPACK's gecon on LAPACK's factors -- stays at or above half of the true norm of the
    inverse of what those factors multiply to, in both norms?  Only such inputs are held to the bars of the tests."""
    return _kept(family, int(n), int(seed), np.dtype(dtype).type)


def pick_seed(family, n, dtype, start=0):
    """The first seed >= start whose input is kept."""
    for seed in range(start, start + 16):
        if kept(family, n, seed, dtype):
            return seed
    raise AssertionError((family, n, dtype, start))


def factor_product(lu):
    """L U in Float64 from packed factors: the matrix whose inverse an estimate from those factors is an estimate of."""
    F = np.asarray(lu, dtype=np.float64)
    return (np.tril(F, -1) + np.eye(F.shape[0])) @ np.triu(F)


# ---- the exact inputs --------------------------------------------------------------------------------------------------------------
class ExactFactors:
    """n; L, U; F: packed L\\U (Float64, Fortran order); Y = U^-1 L^-1, an INTEGER matrix certified in int64."""


@functools.lru_cache(maxsize=None)
def exact_factors(n, copy=0):
    """inv_cases.exact_case(n, copy) made gentler, because the estimator's alternating vector reaches 2n - 2 (12 bits at n = 2112) where
    the inverse tests send unit vectors: U's diagonal is replaced by its signs (so every entry of L, U and of their inverses is an
    integer: granularity 0), and the sub- / superdiagonal entry k with k % 3 == 2 is dropped unless k is a multiple of 64 (chains of
    two, and still one chain across EVERY 64-row boundary).  The far entries of exact_case stay.  Y = U^-1 L^-1 is formed in Float64,
    rounded, and certified: (L U) Y == I in int64."""
    c = exact_case(n, copy)
    L, U = c.L.copy(), c.U.copy()
    idx = np.arange(n)
    U[idx, idx] = np.sign(U[idx, idx])
    for k in range(1, n):
        if k % 3 == 2 and k % 64 != 0:
            L[k, k - 1] = 0.0
            U[k - 1, k] = 0.0
    eye = np.eye(n)
    Y = sla.solve_triangular(U, sla.solve_triangular(L, eye, lower=True, unit_diagonal=True), lower=False)
    Yi = np.rint(Y).astype(np.int64)
    assert np.array_equal(Yi.astype(np.float64), Y), "the inverse is not an integer matrix"
    M = np.rint(L @ U).astype(np.int64)
    assert np.array_equal(M.astype(np.float64), L @ U)
    assert np.array_equal(M @ Yi, np.eye(n, dtype=np.int64)), "the inverse is not exact"
    e = ExactFactors()
    e.n, e.L, e.U, e.Y = n, L, U, Yi.astype(np.float64)
    e.F = np.asfortranarray(np.tril(L, -1) + U)
    for a in (e.L, e.U, e.Y, e.F):
        a.setflags(write=False)
    return e


SMALL_SEEDS = list(range(8))


@functools.lru_cache(maxsize=None)
def small_exact(seed, n=3):
    """Dense integer factors of a tiny matrix: L unit lower and U upper with off-diagonal entries in {-1, 0, 1} and U's diagonal +-1, so
    the inverse is an integer matrix with entries of at most 2^(n-1).  They are here because the thinned chains of exact_factors never
    let the alternating vector's bound win: among these it does (tests/test_cond_cases.py finds the seeds)."""
    rng = np.random.default_rng([7, n, seed])
    L = np.tril(rng.integers(-1, 2, size=(n, n)), -1) + np.eye(n)
    U = np.triu(rng.integers(-1, 2, size=(n, n)), 1) + np.diag(rng.choice([-1.0, 1.0], size=n))
    Y = np.rint(np.linalg.solve(U, np.linalg.solve(L, np.eye(n))))
    assert np.array_equal((L @ U) @ Y, np.eye(n))              # small integers: exact in Float64
    e = ExactFactors()
    e.n, e.L, e.U, e.Y = n, L, U, Y
    e.F = np.asfortranarray(np.tril(L, -1) + U)
    for a in (e.L, e.U, e.Y, e.F):
        a.setflags(write=False)
    return e


def exact_cases(n):
    """The exact inputs of size n: the thinned constructed factors, and at n = 3 the dense small ones."""
    return [exact_factors(n)] + ([small_exact(s) for s in SMALL_SEEDS] if n == 3 else [])


def factor_bits(e):
    """Upper bound on the significant bits of any number any blocked substitution forms while it applies M = U^-1 L^-1 or M^T to any
    vector of the estimator, as (bits for M, bits for M^T).

    A blocked forward / backward substitution forms subset sums of the terms of entries of  T^-1 b,  T (T^-1 b)  and  D^-1 (...)  with D
    a diagonal block of T: every such partial sum is bounded, entry by entry, by  |T^-1| (I + |T| |T^-1|) |b|.  Applied to the two
    triangles in turn, everything formed on the way to M x is at most  |U^-1| (I + |U| |U^-1|) |L^-1| (I + |L| |L^-1|) |x|  and is an
    integer multiple of the product of the factors' granularities (x is an integer vector).  The estimator's vectors satisfy |x| <= ones
    (ones, +-1, e_j) or |x| = n - 1 + i (the alternating vector): the bound is taken with w_i = n - 1 + i >= 1, which covers all of them.
    A multiple of 2^-g below 2^b has at most b + g significant bits."""
    n, L, U = e.n, e.L, e.U
    eye = np.eye(n)
    a = np.abs
    Li = sla.solve_triangular(L, eye, lower=True, unit_diagonal=True)
    Ui = sla.solve_triangular(U, eye, lower=False)
    w = (n - 1 + np.arange(n)).astype(np.float64)
    w[w < 1] = 1.0
    KL = a(Li) @ (eye + a(L) @ a(Li))
    KU = a(Ui) @ (eye + a(U) @ a(Ui))
    g = 2 * _gran_bits(Li) + _gran_bits(L) + 2 * _gran_bits(Ui) + _gran_bits(U)
    b_m = (KU @ (KL @ w)).max()
    b_mt = (KL.T @ (KU.T @ w)).max()
    bits = lambda b: int(math.ceil(math.log2(2.0 * b))) + g   # noqa: E731  (the factor 2: the bound itself was formed in floating point)
    return bits(b_m), bits(b_mt)


@functools.lru_cache(maxsize=None)
def vector_bits(n, copy=0):
    return factor_bits(exact_factors(n, copy))


def case_anorm(e, norm):
    """||L U|| of an exact case (exactly representable: small integers, short sums)."""
    return float(np.linalg.norm(e.L @ e.U, 1 if norm == NORM_ONE else np.inf))


def exact_anorm(n, norm, copy=0):
    """||L U|| of the exact case (exactly representable: small half-integers, short sums)."""
    c = exact_factors(n, copy)
    return float(np.linalg.norm(c.L @ c.U, 1 if norm == NORM_ONE else np.inf))
