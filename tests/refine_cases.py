"""Inputs and CPU references of the refinement tests (tests/test_refine_cases.py on the CPU, tests/test_gpu_refine.py and
tests/test_gpu_refine_exact.py on the GPU).  Pure numpy / scipy, no GPU, no torch.

  * slice_split, absresidual, refine_restated: rflu_gerfs_* restated in the kernels' own order -- the column slices of
    launch_absresidual (csrc/refine.hip; the split of launch_residual_few), inside a slice the columns in ascending order, the slices
    added in slice order, everything in Float64 for both element types; LAPACK xGERFS's loop per column; the forward error bound through
    cond_cases.estimate (the estimator of rflu_gecon_*) on M = diag(wt) A^-T.  The solves are LAPACK's getrs in the element type.
    `fault` plants one of FAULTS.
  * the random inputs: cond_cases.random_matrix rounded to the grid 2^-16, an integer solution, B = A x_true exactly;
  * the exact inputs: mixed_cases.refine_case with X_in[:, k] = c_k x0[:, k], c_k in {1, 1 + 2^-s}.
"""
import functools

import numpy as np
import scipy.linalg as sla

import cond_cases as C
import mixed_cases as MC

U = {np.float64: 2.0 ** -53, np.float32: 2.0 ** -24}          # unit roundoff: LAPACK's eps
AR_ROWS, AR_MIN_CJ, AR_TARGET_WGS, REFINE_PASS = 512, 32, 2048, 8   # csrc/refine.hip, csrc/rflu_internal.hpp
ITMAX = 5

FAMILIES = C.FAMILIES
RANDOM_N = [1, 2, 3, 63, 64, 65, 255, 257, 511, 513, 1025]
RANDOM_INPUTS = [(f, n) for f in FAMILIES for n in RANDOM_N] + [("uniform", 2112)]
RANDOM_NRHS = 3
S_EXACT = {np.float64: 30, np.float32: 10}
EXACT_NRHS = [1, 8, 9, 17]
FAULTS = ["abs_x", "no_abs_b", "update_stopped", "lstres_fixed", "neighbour_berr", "no_nuw", "swap_m", "drop_slice"]

# the largest final berr, in units of u, of the restatement and of LAPACK's gesvx over RANDOM_INPUTS (tests/test_refine_cases.py
# recomputes both and asserts that they still hold); the GPU tests allow twice as much
BERR_REF = {np.float64: 3.21, np.float32: 2.21}


def uof(dtype):
    return U[np.dtype(dtype).type]


def slice_split(n):
    """(cj, splits) of launch_absresidual: a function of n alone"""
    rb = (n + AR_ROWS - 1) // AR_ROWS
    splits = max(1, min((n + AR_MIN_CJ - 1) // AR_MIN_CJ, (AR_TARGET_WGS + rb - 1) // rb))
    cj = ((n + splits - 1) // splits + 7) // 8 * 8
    return cj, (n + cj - 1) // cj


def absresidual(A, X, B, fault=None):
    """(r, w) = (b - A x, |b| + |A| |x|) in Float64, slice by slice"""
    n = A.shape[0]
    A64, X64, B64 = (np.asarray(M, dtype=np.float64) for M in (A, X, B))
    cj, splits = slice_split(n)
    s, sw = np.zeros(X64.shape), np.zeros(X64.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        for sp in range(splits):
            if fault == "drop_slice" and sp == 1:
                continue
            acc, accw = np.zeros(X64.shape), np.zeros(X64.shape)
            for j in range(sp * cj, min(sp * cj + cj, n)):
                acc = acc + A64[:, j, None] * X64[None, j]
                accw = accw + np.abs(A64[:, j, None]) * (X64[None, j] if fault == "abs_x" else np.abs(X64[None, j]))
            s, sw = s + acc, sw + accw
        return B64 - s, (0.0 if fault == "no_abs_b" else np.abs(B64)) + sw


def berr_of(r, w):
    """per column the maximum of |r_i| / w_i that keeps a NaN; a row with w_i == 0 contributes 0"""
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(w == 0.0, 0.0, np.abs(r) / w)
    return np.where(np.isnan(q).any(axis=0), np.nan, q.max(axis=0, initial=0.0))


class Restated:
    """X, berr, ferr, steps, est (the estimates of ||A^-1 diag(wt)||_inf), wt"""


def refine_restated(A, lu, piv, B, X_in, dtype, max_iter=ITMAX, ferr=True, fault=None):
    dtype = np.dtype(dtype).type
    n, nrhs = B.shape
    u = U[dtype]
    X = np.array(X_in, dtype=dtype, order="F")
    solve = lambda v, trans=0: sla.lu_solve((lu, piv), np.asarray(v, dtype=dtype), trans=trans, check_finite=False).astype(dtype)   # noqa: E731
    out = Restated()
    out.berr, out.steps = np.zeros(nrhs), np.zeros(nrhs, dtype=np.int64)
    out.ferr, out.est, out.wt = (np.zeros(nrhs) if ferr else None), np.zeros(nrhs), np.zeros((n, nrhs), dtype=dtype)
    if max_iter <= 0:
        max_iter = ITMAX
    for k0 in range(0, nrhs, REFINE_PASS):
        cols = slice(k0, min(k0 + REFINE_PASS, nrhs))
        p = cols.stop - k0
        lstres, active, taken = np.full(p, 3.0), np.ones(p, dtype=bool), np.zeros(p, dtype=np.int64)
        while True:
            r, w = absresidual(A, X[:, cols], B[:, cols], fault)
            be = berr_of(r, w)
            seen = np.roll(be, 1) if fault == "neighbour_berr" else be
            for k in range(p):
                if not active[k]:
                    continue
                if seen[k] > u and 2.0 * seen[k] <= lstres[k] and taken[k] < max_iter:
                    if fault != "lstres_fixed":
                        lstres[k] = seen[k]
                else:
                    active[k] = False
            if not active.any():
                break
            with np.errstate(all="ignore"):
                d = solve(r.astype(dtype))                       # every column is solved, the stopped ones too
            upd = np.ones(p, dtype=bool) if fault == "update_stopped" else active
            X[:, cols][:, upd] = (X[:, cols][:, upd] + d[:, upd]).astype(dtype)
            taken[active] += 1
        out.berr[cols], out.steps[cols] = be, taken
        for k in range(p):
            wt = (np.abs(r[:, k]) + (0.0 if fault == "no_nuw" else (n + 1) * u * w[:, k])).astype(dtype)
            out.wt[:, k0 + k] = wt
            if not ferr:
                continue
            if be[k] != be[k]:
                out.ferr[k0 + k] = out.est[k0 + k] = np.nan
                continue
            m = lambda x: (wt * solve(x, 1)).astype(dtype)          # noqa: E731  M x = wt o (A^-T x)
            mt = lambda x: solve((wt * x).astype(dtype), 0)           # noqa: E731  M^T x = A^-1 (wt o x)
            if fault == "swap_m":
                m, mt = mt, m
            with np.errstate(all="ignore"):
                est, _ = C.estimate(m, mt, n, dtype)
            xmax = float(np.abs(X[:, k0 + k].astype(np.float64)).max(initial=0.0))
            out.est[k0 + k] = np.inf if est is None else est
            out.ferr[k0 + k] = np.inf if est is None else (est / xmax if xmax != 0.0 else est)
    out.X = X
    return out


# ---- the random inputs -------------------------------------------------------------------------------------------------------------
class RandomInput:
    """A, B, x_true, X_in (LAPACK's solve), lu, piv (0-based, LAPACK's factors), ipiv (1-based int64)"""


@functools.lru_cache(maxsize=None)
def random_input(family, n, dtype):
    dtype = np.dtype(dtype).type
    A = np.asfortranarray((np.rint(C.random_matrix(family, n, 0, dtype).astype(np.float64) * 2.0 ** 16) * 2.0 ** -16).astype(dtype))
    rng = np.random.default_rng([20261, FAMILIES.index(family), n])
    x = rng.integers(-4, 5, size=(n, RANDOM_NRHS))
    x[0, :] = 3
    B64 = A.astype(np.float64) @ x.astype(np.float64)            # multiples of 2^-16 below 2^37: exact in Float64
    c = RandomInput()
    c.A, c.x_true, c.B = A, x.astype(np.float64), np.asfortranarray(B64.astype(dtype))
    # B = A x_true is exact wherever the sums fit the element type; where one does not (Float32, uniform, n = 2112: 25 bits) the exact
    # solution of the ROUNDED right-hand side is x_true plus a correction of relative size 2^-24 cond(A), solved for in Float64
    c.exact_rhs = bool(np.array_equal(c.B.astype(np.float64), B64))
    c.x_ref = c.x_true if c.exact_rhs else c.x_true + np.linalg.solve(A.astype(np.float64), c.B.astype(np.float64) - B64)
    c.lu, c.piv = sla.lu_factor(A, check_finite=False)
    c.ipiv = c.piv.astype(np.int64) + 1
    c.X_in = np.asfortranarray(sla.lu_solve((c.lu, c.piv), c.B, check_finite=False).astype(dtype))
    for a in (c.A, c.B, c.x_true, c.X_in, c.lu, c.ipiv):
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def restated_random(family, n, dtype):
    """refine_restated on a random input (computed once, shared by the tests)"""
    c = random_input(family, n, dtype)
    return refine_restated(c.A, c.lu, c.piv, c.B, c.X_in, dtype)


def lapack_berr(c, dtype):
    """the final berr of LAPACK's own gerfs, run by gesvx (no equilibration) on the same input"""
    fn = sla.lapack.dgesvx if np.dtype(dtype) == np.float64 else sla.lapack.sgesvx
    res = fn(c.A, c.B)
    assert res[-1] in (0, c.A.shape[0] + 1)
    return np.asarray(res[-2], dtype=np.float64)


def true_forward_error(X, x_true):
    X64 = np.asarray(X, dtype=np.float64)
    return np.abs(X64 - x_true).max(axis=0) / np.abs(X64).max(axis=0)


def weighted_inverse_norm(A, wt):
    """||A^-1 diag(wt)||_inf with the explicit inverse in Float64"""
    Ai = np.linalg.inv(np.asarray(A, dtype=np.float64))
    return float(np.abs(Ai * np.asarray(wt, dtype=np.float64)[None, :]).sum(axis=1).max())


# ---- the exact inputs --------------------------------------------------------------------------------------------------------------
class ExactInput:
    """A, F (packed column-major factors), ipiv (1-based, or None: NotIPIV and A = L U), B = b0, X_in, x0, mask (the scaled columns)"""


def exact_input(n, nrhs, pattern, dtype, pivoted=True):
    dtype = np.dtype(dtype).type
    rc = MC.refine_case(n, nrhs)
    s = S_EXACT[dtype]
    mask = MC.scaled_columns(nrhs, pattern)
    e = ExactInput()
    e.n, e.nrhs, e.s, e.mask, e.x0 = n, nrhs, s, mask, rc.x0.astype(np.float64)
    L, Um = rc.L.astype(np.float64), rc.U.astype(np.float64)
    if pivoted:
        A, e.ipiv, b0 = np.asarray(rc.A), rc.ipiv.astype(np.int64), rc.b0.astype(np.float64)
    else:
        A, e.ipiv = L @ Um, None
        b0 = A @ e.x0
    e.A = np.asfortranarray(A.astype(dtype))
    e.F = np.asfortranarray((np.tril(L, -1) + Um).astype(dtype))
    e.b0 = b0
    e.B = np.asfortranarray(b0.astype(dtype))
    e.c = np.where(mask, 1.0 + 2.0 ** -s, 1.0)
    e.X_in = np.asfortranarray((e.x0 * e.c).astype(dtype))
    return e


def exact_proof(e, dtype):
    """The conditions under which one step returns x0 exactly; returns berr0 / u of the scaled columns (inf when there is none)."""
    dtype = np.dtype(dtype).type
    u, s = U[dtype], e.s
    A64, B64, X64 = e.A.astype(np.float64), e.B.astype(np.float64), e.X_in.astype(np.float64)
    assert np.array_equal(e.A.astype(np.float64), np.rint(A64)) and np.array_equal(B64, e.b0)          # integers, representable
    assert np.array_equal(X64, e.x0 * e.c)                                                             # c x0 is representable
    assert np.array_equal(A64 @ e.x0, e.b0)
    terms = np.abs(A64) @ np.abs(e.x0) + np.abs(e.b0)
    assert int(terms.max()).bit_length() + s + 1 <= 53                                                 # no Float64 sum of r or w rounds
    r, w = absresidual(e.A, e.X_in, e.B)
    assert np.array_equal(r, -(e.b0 * np.where(e.mask, 2.0 ** -s, 0.0)))                               # r = -2^-s b0 exactly
    assert np.array_equal(w, np.abs(B64) + np.abs(A64) @ np.abs(X64))
    assert np.array_equal(r.astype(dtype).astype(np.float64), r)                                       # (T) r is exact
    be = berr_of(r, w)
    assert np.all(be[~e.mask] == 0.0)
    if e.mask.any():
        assert be[e.mask].min() >= 2.0 ** 10 * u and be[e.mask].max() <= 1.5
        return float(be[e.mask].min() / u)
    return np.inf
