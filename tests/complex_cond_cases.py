"""Inputs and CPU references of the complex norm / condition-estimate tests (tests/test_complex_cond_cases.py,
tests/test_gpu_complex_cond.py).  Pure numpy / scipy, no GPU, no torch.  The complex counterpart of tests/cond_cases.py, whose kernel_sum,
first_argmax and alternating it reuses.

  * cmod, phase, cestimate, crcond_restatement: the estimator of rflu_gecon_c* restated in the kernels' own order -- LAPACK zlacn2 with
    the two changes include/rflu.h states (all-ones start vector with est = sum / n, integer alternating vector with the bound
    2 sum / (3 n (n - 1))), the pair of operators M and M^H, the phase vector v_i / |v_i| with |v_i| = hypot in Float64 and the two
    quotients rounded to the element type (1 + 0i for a zero), NO repeated-sign-vector test, the FIRST index of the largest modulus,
    every sum of moduli by cond_cases.kernel_sum;
  * line_sum_along / line_sum_across / lange_restatement: the norm sums of csrc/condest.hip in their order;
  * the random inputs: the three families of cond_cases with an independent imaginary part;
  * the exact inputs: the real exact factors of cond_cases embedded as complex, and axis_case -- dense small integer factors whose U has
    its columns multiplied by random powers of i, kept where every vector of the estimator's trace lies on the axes (one part of every
    entry exactly zero), so every modulus and every phase is exact in any hypot.

MEASURED on the CPU (tests/test_complex_cond_cases.py prints them): the relative gap between this restatement at the element precision
and the same restatement one precision up (complex64 -> complex128 -> clongdouble), on LAPACK's factors of the inputs with a decision
margin, the worst over the three families and both norms.  The GPU test measures the same gap on the device's own factors and uses
8 x gap + n eps as its bar; it does not take these figures.
    n        1        2        3        33       255      256      257      1025
    c128  1.6e-16  1.3e-16  2.5e-16  2.8e-16  1.8e-15  6.5e-16  6.7e-15  1.6e-15
    c64   4.2e-08  1.3e-07  5.0e-08  7.5e-08  7.3e-07  9.7e-07  1.4e-06  3.5e-06
"""
import functools
import math

import numpy as np
import scipy.linalg as sla

import cond_cases as R
from cond_cases import FAMILIES, MAX_ROUNDS, NORM_INF, NORM_ONE, alternating, first_argmax, kernel_sum

LN_CHUNK, LN_THREADS, LN_GROUP = 1024, 256, 256      # csrc/condest.hip (asserted against the source)
CGECON_SIZES = [1, 2, 3, 33, 255, 256, 257, 1025]   # single-matrix random sizes: around the 256-row block of the narrow solves, two chunks
CBATCHED_SIZES = {np.complex128: [1, 2, 3, 7, 8, 31, 32, 33, 63, 64], np.complex64: [1, 2, 3, 7, 8, 31, 32, 33, 63, 64, 65, 100, 127, 128]}
CBATCHED_LIMIT = {np.complex128: 64, np.complex64: 128}
EXACT_SIZES = [1, 2, 3, 31, 32, 33, 255, 256, 257, 1023, 1024, 1025, 2112]
BATCHES = [67, 7, 1]
AXIS_SIZES = [3, 4, 5, 6, 8]
AXIS_SEEDS = 40
MARGIN_FACTOR = 64


def real_of(dtype):
    return np.float64 if np.dtype(dtype) == np.complex128 else (np.float32 if np.dtype(dtype) == np.complex64 else np.longdouble)


def wider(dtype):
    """One precision up: complex64 -> complex128 -> clongdouble."""
    return np.complex128 if np.dtype(dtype) == np.complex64 else np.clongdouble


# ---- the kernels' arithmetic -------------------------------------------------------------------------------------------------------
def cmod(x):
    """|x_i| as the kernels form it: hypot of the parts in Float64 (wider inputs keep their precision: the reference one precision up)."""
    x = np.asarray(x)
    t = np.float64 if x.dtype in (np.complex64, np.complex128) else np.longdouble
    return np.hypot(x.real.astype(t), x.imag.astype(t))


def phase(x, zero_is_zero=False):
    """x_i / |x_i| in the type of x: two quotients formed from the Float64 modulus and rounded to the element type; 1 + 0i where both
    parts are zero (zero_is_zero: a planted fault, 0 there)."""
    x = np.asarray(x)
    a = cmod(x)
    z = (x.real == 0) & (x.imag == 0)
    safe = np.where(z, 1, a)
    rt = real_of(x.dtype)
    out = np.empty(x.shape, dtype=x.dtype)
    out.real = np.where(z, 0 if zero_is_zero else 1, (x.real.astype(a.dtype) / safe).astype(rt))
    out.imag = np.where(z, 0, (x.imag.astype(a.dtype) / safe).astype(rt))
    return out


def _gap(a, b):
    m = max(abs(float(a)), abs(float(b)))
    return math.inf if m == 0 else abs(float(a) - float(b)) / m


def cestimate(apply_m, apply_mh, n, dtype, fault=None, trace=None, info=None):
    """The estimate of ||M||_1 from x -> M x and x -> M^H x, both taking and returning arrays of `dtype`.  Returns (est, solves); est is
    None when a vector came back non-finite.  trace (a list) receives every vector sent into a solve and every vector that came back, as
    (adjoint, vector).  info (a dict) receives "margin": the smallest relative gap at any decision (the top two moduli at an argmax, est
    against est_old).  fault: None, "phase_of_zero", "last_argmax", "no_closing" or "drop_chunk"."""
    drop = 1 if fault == "drop_chunk" else None
    solves = 0
    margin = math.inf

    def run(op, x, adjoint):
        nonlocal solves
        solves += 1
        if trace is not None:
            trace.append((adjoint, x.copy()))
        y = np.asarray(op(x), dtype=dtype)
        if trace is not None:
            trace.append((adjoint, y.copy()))
        return y, bool(np.isfinite(cmod(y).astype(np.float64)).all())

    def done(est):
        if info is not None:
            info["margin"] = margin
        return est, solves

    ksum = lambda v: kernel_sum(cmod(v).astype(np.float64), drop) if np.dtype(dtype) != np.clongdouble else cmod(v).sum()   # noqa: E731
    x, ok = run(apply_m, np.ones(n, dtype=dtype), False)
    if not ok:
        return done(None)
    est = ksum(x) / type(ksum(x))(n)
    if n == 1:
        return done(est)
    closing = False
    j = 0
    for rnd in range(MAX_ROUNDS):
        if rnd > 0:
            e = np.zeros(n, dtype=dtype)
            e[j] = 1
            x, ok = run(apply_m, e, False)
            if not ok:
                return done(None)
            est_old = est
            est = ksum(x)
            margin = min(margin, _gap(est, est_old))
            if est <= est_old:
                closing = True
                break
        x, ok = run(apply_mh, phase(x, fault == "phase_of_zero"), True)
        if not ok:
            return done(None)
        ax = cmod(x)
        jlast, j = j, first_argmax(ax.astype(np.float64) if ax.dtype != np.longdouble else ax, last=(fault == "last_argmax"))
        top = np.sort(ax)[-2:]
        margin = min(margin, _gap(top[1], top[0]))
        if (rnd > 0 and ax[jlast] == ax[j]) or rnd == MAX_ROUNDS - 1:
            closing = True
            break
    if closing and fault != "no_closing":
        x, ok = run(apply_m, alternating(n, real_of(dtype)).astype(dtype), False)
        if not ok:
            return done(None)
        s = ksum(x)
        alt = type(s)(2.0) * s / (type(s)(3.0) * type(s)(n) * type(s)(n - 1))
        if alt > est:
            est = alt
    return done(est)


def _substitute(F, x, lower, unit, adjoint, transpose=False):
    """T^-1 x (or T^-H x / T^-T x) by column- / row-oriented substitution in the type of F: for the types scipy does not serve."""
    n = F.shape[0]
    T = F.conj().T if adjoint else (F.T if transpose else F)
    lower = lower != (adjoint or transpose)
    y = x.astype(F.dtype).copy()
    order = range(n) if lower else range(n - 1, -1, -1)
    for k in order:
        if not unit:
            y[k] = y[k] / T[k, k]
        if lower:
            y[k + 1:] -= T[k + 1:, k] * y[k]
        else:
            y[:k] -= T[:k, k] * y[k]
    return y


def ctriangular_solvers(F, dtype, transpose_fault=False):
    """(x -> U^-1 L^-1 x, x -> L^-H U^-H x) by substitution in `dtype` on the packed complex factors F.  transpose_fault (planted): the
    second one is x -> L^-T U^-T x."""
    Fd = np.asarray(F).astype(dtype)
    tr = 1 if transpose_fault else 2
    if np.dtype(dtype) == np.clongdouble:
        def m(x):
            with np.errstate(all="ignore"):
                return _substitute(Fd, _substitute(Fd, x, True, True, False), False, False, False)

        def mh(x):
            with np.errstate(all="ignore"):
                y = _substitute(Fd, x, False, False, not transpose_fault, transpose_fault)
                return _substitute(Fd, y, True, True, not transpose_fault, transpose_fault)

        return m, mh

    def m(x):
        with np.errstate(all="ignore"):
            y = sla.solve_triangular(Fd, x.astype(dtype), lower=True, unit_diagonal=True, check_finite=False)
            return sla.solve_triangular(Fd, y, lower=False, check_finite=False)

    def mh(x):
        with np.errstate(all="ignore"):
            y = sla.solve_triangular(Fd, x.astype(dtype), lower=False, trans=tr, check_finite=False)
            return sla.solve_triangular(Fd, y, lower=True, unit_diagonal=True, trans=tr, check_finite=False)

    return m, mh


def crcond_restatement(F, norm, anorm, dtype, solvers=None, fault=None, detail=False, info=None, trace=None):
    """rflu_gecon_c* on the packed complex factors F.  solvers: (x -> M x, x -> M^H x), default: substitution in `dtype`.  Faults (planted):
    "swap_inf" does not swap M and M^H for the Inf norm, "transpose" uses M^T where M^H belongs, the others are cestimate's.
    detail=True returns (rcond, est, solves)."""
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
    if ((d.real == 0) & (d.imag == 0)).any():
        return out(0.0)
    if np.isnan(np.asarray(F).real).any() or np.isnan(np.asarray(F).imag).any():
        return out(math.nan)
    m, mh = solvers if solvers is not None else ctriangular_solvers(F, dtype, transpose_fault=(fault == "transpose"))
    if norm == NORM_INF and fault != "swap_inf":
        m, mh = mh, m
    est, solves = cestimate(m, mh, n, dtype, fault=fault, info=info, trace=trace)
    if est is None or est == 0.0:
        return out(0.0, est, solves)
    return out(float(np.float64(1.0) / (np.float64(anorm) * np.float64(est))), float(est), solves)


# ---- the norm sums of condest.hip --------------------------------------------------------------------------------------------------
def line_sum_along(mods):
    """Sum of one line's moduli in lange_along_kernel's order."""
    a = np.asarray(mods, dtype=np.float64)
    acc = None
    for c0 in range(0, a.size, LN_CHUNK):
        buf = np.zeros(LN_CHUNK)
        piece = a[c0:c0 + LN_CHUNK]
        buf[:piece.size] = piece
        quad = buf.reshape(LN_THREADS, 4)
        v = np.zeros(LN_THREADS)
        for e in range(4):                       # a thread's four elements in index order, from 0.0
            v = v + quad[:, e]
        w = v.reshape(LN_THREADS // 64, 64).copy()
        s = 32
        while s > 0:                             # the wave tree
            w[:, :s] = w[:, :s] + w[:, s:2 * s]
            s //= 2
        cs = ((w[0, 0] + w[1, 0]) + w[2, 0]) + w[3, 0]
        acc = cs if acc is None else acc + cs
    return np.float64(0.0 if acc is None else acc)


def line_sum_across(mods):
    """Sum over the lines of one position's moduli in lange_across_kernel / lange_max_kernel's order."""
    a = np.asarray(mods, dtype=np.float64)
    acc = None
    for g0 in range(0, a.size, LN_GROUP):
        s = np.float64(0.0)
        for v in a[g0:g0 + LN_GROUP]:
            s = s + v
        acc = s if acc is None else acc + s
    return np.float64(0.0 if acc is None else acc)


def modulus64(A):
    """hypot of the Float64 parts, NaN where either part is NaN (also next to an Inf)."""
    A = np.asarray(A)
    re, im = A.real.astype(np.float64), A.imag.astype(np.float64)
    with np.errstate(all="ignore"):
        return np.where(np.isnan(re) | np.isnan(im), np.nan, np.hypot(re, im))


def lange_restatement(A, norm, row_major):
    """rflu_lange_c*_dev on the m x n complex matrix A stored column-major (row_major = 0) or row-major (1)."""
    M = modulus64(A)
    if M.size == 0:
        return 0.0
    along = (norm == NORM_ONE) != bool(row_major)
    lines = M.T if norm == NORM_ONE else M          # the sums of a 1-norm run down columns, of an Inf-norm along rows
    sums = [line_sum_along(line) if along else line_sum_across(line) for line in lines]
    return float(np.nan) if any(s != s for s in sums) else float(max(sums))


# ---- the random inputs -------------------------------------------------------------------------------------------------------------
def random_matrix(family, n, seed, dtype):
    """The family of cond_cases with an independent imaginary part (the same family, another seed)."""
    rt = real_of(dtype)
    A = R.random_matrix(family, n, seed, rt).astype(dtype) + 1j * R.random_matrix(family, n, seed + 5000, rt).astype(dtype)
    return np.asfortranarray(A.astype(dtype))


def factor_product(lu):
    F = np.asarray(lu, dtype=np.complex128)
    return (np.tril(F, -1) + np.eye(F.shape[0])) @ np.triu(F)


def true_inverse_norms(A):
    X = np.linalg.inv(np.asarray(A, dtype=np.complex128))
    return {NORM_ONE: float(np.linalg.norm(X, 1)), NORM_INF: float(np.linalg.norm(X, np.inf))}


def lapack_factors(A):
    return sla.lu_factor(np.array(A, order="F"), check_finite=False)


def lapack_gecon(lu, anorm, norm):
    """LAPACK's own estimate of ||A^-1|| from its factors (zgecon / cgecon): 1 / (rcond * anorm)."""
    fn = sla.lapack.zgecon if lu.dtype == np.complex128 else sla.lapack.cgecon
    rc, info = fn(lu, anorm, norm=b"1" if norm == NORM_ONE else b"I")
    assert info == 0
    return 1.0 / (float(rc) * float(anorm))


@functools.lru_cache(maxsize=None)
def _kept(family, n, seed, dtype):
    lu, _ = lapack_factors(random_matrix(family, n, seed, dtype))
    LU = factor_product(lu)
    true = true_inverse_norms(LU)
    for norm in (NORM_ONE, NORM_INF):
        anorm = float(np.linalg.norm(LU, 1 if norm == NORM_ONE else np.inf))
        if lapack_gecon(lu, anorm, norm) < 0.5 * true[norm]:
            return False
    return True


def kept(family, n, seed, dtype):
    """The `kept` rule of cond_cases: LAPACK's own estimate on LAPACK's factors reaches half the true norm, in both norms."""
    return _kept(family, int(n), int(seed), np.dtype(dtype).type)


@functools.lru_cache(maxsize=None)
def _margin(family, n, seed, dtype):
    lu, _ = lapack_factors(random_matrix(family, n, seed, dtype))
    worst = math.inf
    for norm in (NORM_ONE, NORM_INF):
        info = {}
        crcond_restatement(lu, norm, 1.0, dtype, info=info)
        worst = min(worst, info.get("margin", math.inf))
    return worst


def margin_bar(n, dtype):
    return MARGIN_FACTOR * n * float(np.finfo(real_of(dtype)).eps)


def has_margin(family, n, seed, dtype):
    """Does every decision of the restatement (on LAPACK's factors of this input) have a relative gap above 64 n eps?"""
    return _margin(family, int(n), int(seed), np.dtype(dtype).type) > margin_bar(n, dtype)


def pick_seed(family, n, dtype, start=0, margin=False):
    """The first seed >= start whose input is kept (and, with margin=True, has a decision margin)."""
    for seed in range(start, start + 32):
        if kept(family, n, seed, dtype) and (not margin or has_margin(family, n, seed, dtype)):
            return seed
    raise AssertionError((family, n, dtype, start, margin))


def decision_margin(lu, norm, dtype):
    """The smallest relative decision gap of the restatement on these factors."""
    info = {}
    crcond_restatement(lu, norm, 1.0, dtype, info=info)
    return info.get("margin", math.inf)


# ---- the exact inputs --------------------------------------------------------------------------------------------------------------
def embedded_exact(n):
    """cond_cases.exact_factors(n) with zero imaginary parts: (packed complex128 factors, the real case)."""
    e = R.exact_factors(n)
    return np.asfortranarray(e.F.astype(np.complex128)), e


class AxisCase:
    """n, seed; F: packed complex128 factors L \\ (U D), D = diag(i^p); dinv = 1 / diag(D); Y = U^-1 L^-1 (integer); so M = D^-1 Y."""


UNITS = np.array([1, 1j, -1, -1j])


@functools.lru_cache(maxsize=None)
def axis_candidate(seed, n):
    e = R.small_exact(seed, n)
    p = np.random.default_rng([11, n, seed]).integers(0, 4, size=n)
    c = AxisCase()
    c.n, c.seed = n, seed
    c.d = UNITS[p]
    c.dinv = UNITS[(4 - p) % 4]
    c.Y = e.Y
    c.L, c.U = e.L, e.U * c.d[None, :]
    c.F = np.asfortranarray(np.tril(e.L, -1).astype(np.complex128) + c.U)
    assert np.array_equal(c.d * c.dinv, np.ones(n))
    return c


def axis_solvers(c, dtype, transpose_fault=False):
    """Exact M x = D^-1 (Y x) and M^H x = Y^T (conj(D^-1) x) on Gaussian integers (transpose_fault: M^T x = Y^T (D^-1 x))."""
    Yc = c.Y.astype(np.complex128)

    def m(x):
        return (c.dinv * (Yc @ x.astype(np.complex128))).astype(dtype)

    def mh(x):
        return (Yc.T @ ((c.dinv if transpose_fault else c.dinv.conj()) * x.astype(np.complex128))).astype(dtype)

    return m, mh


def axis_anorm(c, norm):
    """||L U D||: a sum of moduli of Gaussian integers, rounded -- but only an input of the estimate, the same double on both sides."""
    return float(np.abs(c.L @ c.U).sum(axis=0 if norm == NORM_ONE else 1).max())


def on_axes(v):
    return bool(((v.real == 0) | (v.imag == 0)).all())


def axis_rcond(c, norm, dtype, fault=None, trace=None):
    return crcond_restatement(c.F, norm, 1.0, dtype, solvers=axis_solvers(c, dtype, fault == "transpose"),
                              fault=None if fault == "transpose" else fault, trace=trace)


@functools.lru_cache(maxsize=None)
def axis_search():
    """(qualifying (case, norm) pairs, those among them on which M^T for M^H changes the estimate).  A pair qualifies when every vector
    of the trace -- everything sent into a solve and everything that came back -- has one part of every entry exactly zero.  (In the
    1-norm the first solve is M ones = D^-1 (Y ones), on the axes by construction; in the Inf norm it is M^H ones = Y^T conj(D^-1) ones,
    which mixes the axes unless the powers of i happen to allow it: most Inf-norm candidates do not qualify.)"""
    good, notice = [], []
    for n in AXIS_SIZES:
        for seed in range(AXIS_SEEDS):
            c = axis_candidate(seed, n)
            for norm in (NORM_ONE, NORM_INF):
                trace = []
                want = axis_rcond(c, norm, np.complex128, trace=trace)
                if not all(on_axes(v) for _, v in trace):
                    continue
                good.append((c, norm))
                if axis_rcond(c, norm, np.complex128, fault="transpose") != want:
                    notice.append((c, norm))
    return tuple(good), tuple(notice)


def axis_cases(norm, limit=16):
    """The axis-scaled cases the GPU tests use in this norm: those that notice M^T for M^H first, then others, `limit` in all."""
    good, notice = axis_search()
    first = [c for c, nm in notice if nm == norm]
    rest = [c for c, nm in good if nm == norm and (c, nm) not in notice]
    return (first + rest)[:limit]
