"""Inputs, CPU references and bars of the complex mixed-precision tests (tests/test_complex_mixed_cases.py proves them on the CPU,
tests/test_gpu_complex_mixed.py uses them on the GPU).  Pure numpy / scipy, no GPU.

  * grid_input / cpu_refine: the refinement of csrc/driver.cpp (mixed_refine) restated with scipy's ComplexF32 lu_factor and residuals
    in np.clongdouble; the rule is ||r_k||_inf <= ||x_k||_inf ||A||_inf eps64 sqrt(n) per column, every norm in MODULI.
  * exact_solve_case: CONSTRUCTED row-major factors L\\U and interchanges with a Gaussian-integer solution: every partial sum of both
    substitutions is exact in Float32 in any order, so the forward solve must return X by ==.  See its docstring.
  * cdemote_input / cdemote_restated, crefine_case: the complex inputs of the exact tests of the demoted image and of the refinement
    loop (tests/test_gpu_complex_mixed_exact.py); what makes them exact is said in tests/mixed_cases.py, parts A and B.
"""
import functools

import numpy as np

import mixed_cases as mc
from complex_inv_cases import DIAG

EPS = float(np.finfo(np.float64).eps)
GRID = [(1, 1), (8, 1), (33, 3), (65, 8), (129, 9), (257, 1), (300, 64), (513, 8), (1000, 9), (1025, 3), (2100, 33)]
# refinement steps of cpu_refine on the grid (test_complex_mixed_cases.py recomputes them); the GPU's ComplexF32 factorization rounds
# differently from LAPACK's and pivots by modulus instead of |re| + |im|, so its allowance is twice the CPU maximum
CPU_STEPS = {1: 2, 8: 2, 33: 2, 65: 2, 129: 2, 257: 2, 300: 2, 513: 3, 1000: 3, 1025: 3, 2100: 3}
GPU_STEP_ALLOWANCE = 2 * max(CPU_STEPS.values())


def uniform_complex(rows, cols, seed):
    """re and im uniform in [-1/2, 1/2), column-major complex128"""
    rng = np.random.default_rng(seed)
    return np.asfortranarray((rng.random((rows, cols)) - 0.5) + 1j * (rng.random((rows, cols)) - 0.5))


@functools.lru_cache(maxsize=None)
def grid_input(n, nrhs):
    A, B = uniform_complex(n, n, 900 + n), uniform_complex(n, nrhs, 901 + n)
    A.setflags(write=False)
    B.setflags(write=False)
    return A, B


def anorm_inf(A):
    """||A||_inf as LAPACK zlange('I') has it: the largest row sum of moduli"""
    return float(np.abs(A).sum(axis=1).max()) if A.size else 0.0


def rule_ratio(A, X, R):
    """per column ||r_k||_inf / (||x_k||_inf ||A||_inf eps sqrt(n)): the rule is met where this is <= 1"""
    n = A.shape[0]
    X, R = X.reshape(n, -1), R.reshape(n, -1)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return np.abs(R).max(axis=0) / (np.abs(X).max(axis=0) * anorm_inf(A) * EPS * np.sqrt(n))


def residual_ld(A, X, B):
    """B - A X in np.clongdouble, rounded to complex128 once"""
    ld = np.clongdouble
    return (B.astype(ld) - A.astype(ld) @ X.astype(ld)).astype(np.complex128)


def cpu_refine(A, B, max_iter=30):
    """(X, iters, first_ratio): iters as the C entry reports it; first_ratio = the worst rule_ratio of the UNREFINED ComplexF32 solve"""
    import scipy.linalg as sla

    with np.errstate(over="ignore", invalid="ignore"):
        fac = sla.lu_factor(A.astype(np.complex64), check_finite=False)
        solve32 = lambda S: sla.lu_solve(fac, S.astype(np.complex64), check_finite=False).astype(np.complex128)   # noqa: E731
        X = solve32(B)
        first = None
        step = 0
        while True:
            R = residual_ld(A, X, B)
            ratio = rule_ratio(A, X, R)
            if first is None:
                first = float(np.max(ratio)) if np.all(np.isfinite(ratio)) else float("inf")
            if np.all(ratio <= 1.0):          # (a NaN compares false: never convergence)
                return X, step, first
            if step >= max_iter:
                return X, -(step + 1), first
            X = X + solve32(R)
            step += 1


def ill_conditioned(n, log10_kappa):
    """Q1 diag(logspace(0, -log10_kappa)) Q2^H with complex unitary Q"""
    rng = np.random.default_rng(5)
    Q1, _ = np.linalg.qr(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
    Q2, _ = np.linalg.qr(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
    return np.asfortranarray(Q1 @ np.diag(np.logspace(0, -log10_kappa, n)) @ Q2.conj().T)


def float64_bars(A, B, X, Xref, nrm2):
    """bar (b): (residual, its bound, relative solution error); the project's Float64 bars of test_gpu_mixed.py"""
    n = A.shape[0]
    res = np.linalg.norm(A @ X - B)
    bound = 1000 * n * EPS * (nrm2 * np.linalg.norm(Xref) + np.linalg.norm(B))
    return float(res), float(bound), float(np.linalg.norm(X - Xref) / np.linalg.norm(Xref))


def norm2(A):
    """||A||_2; from n = 2000 on a lower bound of it (power iteration on A^H A): a smaller norm only tightens bar (b)"""
    if A.shape[0] < 2000:
        return float(np.linalg.norm(A, 2))
    w = np.ones(A.shape[0], dtype=np.complex128)
    for _ in range(20):
        w = A.conj().T @ (A @ w)
        w /= np.linalg.norm(w)
    return float(np.linalg.norm(A @ w))


# ---- the exact solve cases -----------------------------------------------------------------------------------------------------------
EXACT_N = [1, 31, 32, 33, 255, 256, 257, 513]      # the 32-row steps and the 256-row blocks of the narrow solve, the leaves of the wide one
EXACT_NRHS = [1, 8, 9]                             # one column, the widest narrow block, the first wide one
GAUSS = np.array([0, 1, -1, 1j, -1j])              # entries of L and U off the diagonal


class ExactSolveCase:
    """n, nrhs; W: packed L\\U (complex64, C order = the library's row-major layout); ipiv (1-based int64); B, X (complex64, Fortran
    order) with P B = L U X exactly; fwd_sum / bwd_sum: the largest sum over a row of the moduli of all terms of its substitution, in
    units of the grid 1/2."""


@functools.lru_cache(maxsize=None)
def exact_solve_case(n, nrhs):
    """L unit lower and U upper, dense, off-diagonal entries from {0, +-1, +-i}; diag(U) from DIAG = units, +-2, +-2i, +-1/2; ipiv[k] a
    random row in [k, n) (0-based), so targets repeat; X with re, im in {-2..2}.  Y = U X, Z = L Y and B = P^T Z are formed in INTEGER
    arithmetic on 2 U (int64 pairs), so B is known exactly; every entry of Y, Z, B is a Gaussian integer times 1/2.

    Why the GPU result must equal X by ==: the forward substitution forms, for row i, z_i - sum_{j<i} l_ij y_j, the backward one
    (y_i - sum_{j>i} u_ij x_j) / u_ii.  Every term is a Gaussian integer times 1/2.  If the sum of the moduli of ALL terms of a row is
    below 2^24 grid units, then every partial sum, in any order and grouping (the chunked sums of cgemv_sub_kernel, the shuffle tree,
    the 32-wide steps of ctrsv_block_kernel, the MFMA accumulators of the wide path), is a grid point below 2^24 units in both parts
    and therefore a Float32 number: nothing is ever rounded.  The products are exact (a factor is 0, a unit, or a power of two times a
    unit).  Smith's division by u_ii in {units, +-2, +-2i, +-1/2} forms the ratio 0 or -0, a reciprocal that is a power of two, and
    products with those: exact again.  test_complex_mixed_cases.py asserts the bound for every case."""
    rng = np.random.default_rng(31000 + 16 * n + nrhs)

    def gi(a):   # complex array with integer parts -> (re, im) int64
        return np.rint(a.real).astype(np.int64), np.rint(a.imag).astype(np.int64)

    def cmatmul(a, b):
        return a[0] @ b[0] - a[1] @ b[1], a[0] @ b[1] + a[1] @ b[0]

    L = np.tril(GAUSS[rng.integers(0, 5, (n, n))], -1) + np.eye(n)
    U = np.triu(GAUSS[rng.integers(0, 5, (n, n))], 1) + np.diag(DIAG[rng.integers(0, len(DIAG), n)])
    X = rng.integers(-2, 3, (n, nrhs)) + 1j * rng.integers(-2, 3, (n, nrhs))
    ipiv = np.array([k + 1 + rng.integers(0, n - k) for k in range(n)], dtype=np.int64)
    Y2 = cmatmul(gi(2 * U), gi(X))                 # 2 Y
    Z2 = cmatmul(gi(L), Y2)                        # 2 Z = 2 P B
    B2 = [Z2[0].copy(), Z2[1].copy()]
    for k in range(n - 1, -1, -1):                 # B = P^T Z: the interchanges undone last first
        p = ipiv[k] - 1
        if p != k:
            for part in B2:
                part[[k, p]] = part[[p, k]]
    absL, absU2 = np.abs(np.tril(L, -1)), np.abs(np.triu(2 * U, 1))
    modY2, modZ2 = np.hypot(*Y2), np.hypot(*Z2)
    c = ExactSolveCase()
    c.n, c.nrhs, c.ipiv = n, nrhs, ipiv
    c.W = np.ascontiguousarray((np.tril(L, -1) + U).astype(np.complex64))
    c.X = np.asfortranarray(X.astype(np.complex64))
    c.B = np.asfortranarray(((B2[0] + 1j * B2[1]) / 2).astype(np.complex64))
    c.L, c.U = L, U
    c.fwd_sum = float((modZ2 + absL @ modY2).max())
    c.bwd_sum = float((modY2 + absU2 @ np.abs(X)).max())
    assert np.array_equal(c.W.astype(np.complex128), np.tril(L, -1) + U)                  # the factors are Float32 numbers
    assert np.array_equal(c.B.astype(np.complex128) * 2, B2[0] + 1j * B2[1])              # so is B
    for a in (c.W, c.X, c.B, c.ipiv):
        a.setflags(write=False)
    return c


# ---- the demoted image, element by element (part A of tests/mixed_cases.py, complex) ---------------------------------------------------
CDEMOTE_SIZES = [1, 2, 63, 64, 65, 129, 193]       # both sides of the 64 x 64 tile, several tiles in the diagonal order
CDM_T = 64                                         # csrc/mixed.hip
CMUTATIONS = ["truncation", "half_away", "dropped_last_column"]


@functools.lru_cache(maxsize=None)
def cdemote_input(n, kind, fam):
    """The n x n ComplexF64 input, column-major, read-only.  kind 'upper' / 'lower' as mixed_cases.demote_input: the pivot rule is the
    largest modulus with the lowest row on ties, Smith's division of a zero numerator gives 0 and a division by 1 + 0i returns the
    numerator, so triu(F32) (upper) and tril(F32, -1) (lower) are the demoted input itself.
    fam 'random': both parts from mixed_cases.family (lower: parts in (1/4, 1/2), so every modulus is below 1/sqrt(2) < 3/4);
    fam 'axis': one part from the family, the other zero -- purely real or purely imaginary at random -- so that hypot is exact, every
    modulus is on the grid 2^-40 and ||A||_inf must come back by == (lower: the nonzero part in (1/2, 3/4))."""
    rng = np.random.default_rng([42000, n, 0 if kind == "upper" else 1, 0 if fam == "random" else 1])
    if fam == "random":
        kw = {} if kind == "upper" else {"exps": (-2,)}
        V = mc.family((n, n), rng, **kw)[0] + 1j * mc.family((n, n), rng, **kw)[0]
    else:
        kw = {} if kind == "upper" else {"exps": (-1,), "mbits": 22}
        V = mc.family((n, n), rng, **kw)[0] * np.where(rng.integers(0, 2, size=(n, n)) == 1, 1j, 1.0)
    A = np.asfortranarray(np.triu(V) if kind == "upper" else np.tril(V, -1) + np.eye(n))
    A.setflags(write=False)
    return A


def expected_cimage(A):
    """numpy's IEEE conversion of both parts"""
    with np.errstate(over="ignore"):
        return np.asarray(A).astype(np.complex64)


def exact_axis_anorm(A):
    """||A||_inf of an on-axis matrix: the modulus of an entry is |re| + |im| with one of them zero"""
    assert not np.any((A.real != 0) & (A.imag != 0))
    return mc.exact_anorm(np.abs(A.real) + np.abs(A.imag))


def cdemote_restated(A, mutation=None):
    """(F, anorm): cdemote_relayout_kernel + rowsum_max_kernel restated tile by tile: lane l owns row l of a 64 x 64 tile, wave w adds
    hypot(re, im) over the columns c = w, w + 4, .. in ascending order, the waves' sums are added as ((s0 + s1) + s2) + s3, a row's
    tiles in tile order.  The 16-byte and the element-wise forms move the same elements.  F starts as SENTINEL32 in both parts."""
    n = A.shape[0]
    conv = {"truncation": mc.truncate32, "half_away": mc.half_away32}.get(mutation, mc.expected_image)
    F = np.full((n, n), mc.SENTINEL32 * (1 + 1j), dtype=np.complex64)
    nt = (n + CDM_T - 1) // CDM_T
    part = np.zeros((nt, n))
    for bx in range(nt):
        for by in range(nt):
            tj = (by + bx) % nt
            i0, j0 = bx * CDM_T, tj * CDM_T
            P = np.zeros((CDM_T, CDM_T), dtype=np.complex128)
            blk = A[i0:i0 + CDM_T, j0:j0 + CDM_T]
            P[:blk.shape[0], :blk.shape[1]] = blk
            tile = conv(P.real) + 1j * conv(P.imag)
            rsum = np.zeros((4, CDM_T))
            for w in range(4):
                for c in range(w, CDM_T, 4):
                    rsum[w] = rsum[w] + np.hypot(P[:, c].real, P[:, c].imag)
            rows, cols = min(CDM_T, n - i0), min(CDM_T, n - j0)
            part[tj, i0:i0 + rows] = (((rsum[0] + rsum[1]) + rsum[2]) + rsum[3])[:rows]
            if mutation == "dropped_last_column" and cols < CDM_T:
                cols -= 1
            F[i0:i0 + rows, j0:j0 + cols] = tile[:rows, :cols]
    s = np.zeros(n)
    for t in range(nt):
        s = s + part[t]
    return F, float(s.max())


# ---- the refinement loop, step by step (part B of tests/mixed_cases.py, complex) -------------------------------------------------------
REFINE_N = [1, 33, 257, 513]
REFINE_NRHS = [1, 8, 9, 33, 65]      # 8 and 9: both sides of CNARROW (the column-major and the row-major image of the right-hand sides)
# c_k = 1 + 2^-S_CPLX.  The largest s that the dense cases allow.  Two conditions bind (test_complex_mixed_cases.py recomputes both):
# the largest row sum of the moduli of all terms of B - A X over the grid above is 25415 units of 1/2 (n = 513, nrhs = 8), 15 bits, so
# 15 + s <= 53 allows 38; the rule must be MISSED at step 0 by a factor no rounding of hypot or sqrt can bridge (2^10 is asked for), and
# with the dense A of n = 513 (||A||_inf about 6000, ||b|| / ||x|| about 40) a scaled column misses it by 2^(43.6 - s): s <= 33.
S_CPLX = 33


class CRefineCase(mc.RefineCase):
    """mixed_cases.RefineCase with complex A, x0, b0; F32 is complex64; every entry is a Gaussian integer times 1/2."""


@functools.lru_cache(maxsize=None)
def crefine_case(n, nrhs):
    """exact_solve_case(n, nrhs) as what rflu_mixed_getrs_cf64_dev takes: A = P^T L U formed in integer arithmetic on 2 U, dense
    ComplexF64; ||A||_inf in moduli (rounded: the rule is missed or met by orders of magnitude, mixed_cases.refine_proof)."""
    e = exact_solve_case(n, nrhs)
    L, U2 = np.rint(e.L.real).astype(np.int64) + 1j * np.rint(e.L.imag).astype(np.int64), 2 * e.U
    lr, li, ur, ui = (np.rint(p).astype(np.int64) for p in (L.real, L.imag, U2.real, U2.imag))
    A2 = [lr @ ur - li @ ui, lr @ ui + li @ ur]                       # 2 P A
    for k in range(n - 1, -1, -1):                                    # P^T: the interchanges undone last first
        p = e.ipiv[k] - 1
        if p != k:
            for part in A2:
                part[[k, p]] = part[[p, k]]
    perm = list(range(n))
    for k in range(n):
        p = int(e.ipiv[k]) - 1
        if p != k:
            perm[k], perm[p] = perm[p], perm[k]
    c = CRefineCase()
    c.n, c.nrhs, c.ipiv = n, nrhs, e.ipiv
    c.A = np.asfortranarray((A2[0] + 1j * A2[1]) / 2)
    c.x0, c.b0 = e.X.astype(np.complex128), e.B.astype(np.complex128)
    assert np.array_equal(c.A @ c.x0, c.b0)                           # small Gaussian half-integers: exact in complex128
    c.anorm = anorm_inf(c.A)
    c.F32 = e.W
    c.L, c.U, c.perm = e.L.astype(np.complex64), e.U.astype(np.complex64), np.asarray(perm)
    c.term_sum = float((np.abs(c.A) @ np.abs(c.x0) + np.abs(c.b0)).max())
    c.fwd_sum, c.bwd_sum = e.fwd_sum, e.bwd_sum
    for a in (c.A, c.x0, c.b0):
        a.setflags(write=False)
    return c
