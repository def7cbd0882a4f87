"""Inputs, CPU references and their proofs for the EXACT tests of the mixed-precision solves (tests/test_mixed_cases.py proves them on
the CPU; tests/test_gpu_mixed_exact.py and tests/test_gpu_complex_mixed_exact.py use them on the GPU; the complex counterparts of
parts A and B live in tests/complex_mixed_cases.py and reuse what is here).  Pure numpy / scipy: no torch, no GPU.

A. The demoted image.  rflu_mixed_getrf_* factors the Float32 image of A in place at once, so it can only be read through inputs whose
   factorization does no arithmetic on it:
     * `upper`: A upper triangular with a normal nonzero diagonal.  Every multiplier is (+-0) / u_kk or (+-0) * (1 / u_kk) = +-0, every
       update a - (+-0) u = a, every inv(L11) product 1 * a + 0 * ...: triu(F32) == float32(triu(A)), ipiv the identity, info 0.
     * `lower`: A unit lower triangular with |a_ij| <= 3/4 below the diagonal.  The pivot stays on the diagonal (1 > 3/4, the rule is a
       strict '>'), the multipliers are a_ik / 1 or a_ik * 1, U stays the identity: tril(F32, -1) == float32(tril(A, -1)).
   Two calls show every element of the image.  Only VALUES are compared: -0 - (-0) may flip the sign of a zero.
   The nonzero entries (`family`) are v = +-(2^23 + m + off) 2^(e - 23): a normal Float32 f = +-(2^23 + m) 2^(e - 23), 1 <= m, plus
   `off` units of ulp32(f) from OFFSETS = {0, +-1/4, +-1/2 (the exact tie), +-(1/2 +- 2^-16)}; m is random, so both parities of f's
   last bit meet every offset and entries differ from position to position (a moved element is seen).  With e in {-1, 0}: |v| < 2 on the
   grid 2^-40, so every sum of at most 2^12 moduli is below 2^13 on that grid, 53 bits: every partial row sum of |a| is exact in
   Float64 IN ANY ORDER for n <= 2^12, and ||A||_inf must come back by ==.  The expected image is numpy's IEEE conversion
   (round to nearest, ties to even).
   `demote_restated` restates demote_relayout_kernel's index arithmetic (csrc/mixed.hip) tile by tile, with the mutations a test
   should see: truncation, round-half-away, a dropped last column of a partial tile, exchanged ra / rb rows, a missing last odd row.

B. The refinement loop.  `refine_case(n, nrhs)` is tests/solve_cases.py's SolveCase as what rflu_mixed_getrs_f64_dev takes: the packed
   factors as a row-major Float32 image, ipiv, A = P^T L U as a dense Float64 array of small integers, ||A||_inf exactly, the integer
   solution x0 and b0 = A x0.  With B[:, k] = c_k b0[:, k] and c_k in {1, 1 + 2^-s}: demote(B) = b0 (s >= 25: the perturbation is below
   half an ulp32), step 0 returns x0 (SolveCase's proof), R = B - A x0 = 2^-s b0 in the scaled columns and 0 in the others, exactly;
   the rule fails; demote(R), its solve (a power-of-two scaling of the exact case) and X += d are exact; the next residual is exactly
   0: iters == 1 and X[:, k] == c_k x0[:, k] by ==.  `refine_proof` checks the conditions per case, `refine_restated` is the loop of
   csrc/driver.cpp (mixed_getrs) in numpy with scipy's Float32 triangular solves, and with the mutations a test should see.

C. The residual alone.  `residual_case(n)`: integer A, X, B with |entries| <= 4 and B - A X in int64.
"""
import functools
import math
from fractions import Fraction

import numpy as np

from solve_cases import solve_case

EPS = float(np.finfo(np.float64).eps)

# ---- A. the demoted image ------------------------------------------------------------------------------------------------------------
DEMOTE_SIZES = [1, 2, 63, 64, 65, 127, 128, 129, 130, 193, 257, 577]   # both sides of the 128-row and the 64-column tile, an odd last
#                                                                       # row, several tiles in the diagonal order (5 x 10 at 577)
OFFSETS = np.array([0.0, 0.25, -0.25, 0.5, -0.5, 0.5 + 2.0 ** -16, -(0.5 + 2.0 ** -16), 0.5 - 2.0 ** -16, -(0.5 - 2.0 ** -16)])
GRID_BITS = 40                       # every family value with e >= -1 is a multiple of 2^-40
DM_TI, DM_TJ = 128, 64               # csrc/mixed.hip
MUTATIONS = ["truncation", "half_away", "dropped_last_column", "exchanged_rows", "missing_last_odd_row"]


def family(shape, rng, exps=(-1, 0), mbits=23):
    """(v, m, off): v = +-(2^23 + m + off) 2^(e - 23) in Float64, 1 <= m < 2^mbits - 1 (mbits = 22: |f| < 3/4 2^(e + 1)), e from
    exps; m and off (the index into OFFSETS) are returned for the proofs."""
    m = rng.integers(1, 2 ** mbits - 1, size=shape)
    k = rng.integers(0, len(OFFSETS), size=shape)
    e = rng.choice(np.asarray(exps, dtype=np.int64), size=shape)
    sign = rng.choice(np.array([-1.0, 1.0]), size=shape)
    v = sign * (float(2 ** 23) + m + OFFSETS[k]) * np.exp2((e - 23).astype(np.float64))
    return v, m, k


@functools.lru_cache(maxsize=None)
def demote_input(n, kind):
    """The n x n Float64 input of part A, column-major, read-only.  kind: 'upper' or 'lower'."""
    rng = np.random.default_rng([41000, n, 0 if kind == "upper" else 1])
    if kind == "upper":
        A = np.triu(family((n, n), rng)[0])
    else:
        A = np.tril(family((n, n), rng, exps=(-1,), mbits=22)[0], -1) + np.eye(n)
    A = np.asfortranarray(A)
    A.setflags(write=False)
    return A


def visible(kind):
    """the part of the factored image that is the demoted input itself: mask(n) -> boolean n x n"""
    return (lambda n: np.triu(np.ones((n, n), dtype=bool))) if kind == "upper" else (lambda n: np.tril(np.ones((n, n), dtype=bool), -1))


def expected_image(A):
    """numpy's IEEE conversion: round to nearest, ties to even, gradual underflow, overflow to Inf"""
    with np.errstate(over="ignore"):
        return np.asarray(A).astype(np.float32)


def exact_anorm(A):
    """||A||_inf of a real matrix on the grid 2^-40, in integer arithmetic (the row sums are below 2^53 grid units, see the module
    docstring, so the result is a Float64 number)"""
    K = np.rint(np.abs(A) * 2.0 ** GRID_BITS)
    assert np.array_equal(K * 2.0 ** -GRID_BITS, np.abs(A)), "an entry is off the grid 2^-40"
    top = max(int(s) for s in K.astype(np.int64).sum(axis=1)) if A.size else 0
    assert top < 2 ** 53
    return float(top) * 2.0 ** -GRID_BITS


def truncate32(v):
    """Float64 -> Float32 toward zero"""
    f = expected_image(v)
    over = np.abs(f.astype(np.float64)) > np.abs(v)
    return np.where(over, np.nextafter(f, np.float32(0)), f).astype(np.float32)


def half_away32(v):
    """Float64 -> Float32 to nearest, ties AWAY from zero"""
    lo = truncate32(v)
    hi = np.nextafter(lo, np.where(np.signbit(v), -np.inf, np.inf).astype(np.float32)).astype(np.float32)
    tie = (np.abs(v) - np.abs(lo.astype(np.float64))) == (np.abs(hi.astype(np.float64)) - np.abs(v))
    return np.where(tie & (lo != v), hi, expected_image(v)).astype(np.float32)


SENTINEL32 = np.float32(-7.25)


def demote_restated(A, vin, vout, mutation=None):
    """(F, anorm): demote_relayout_kernel<VIN, VOUT> + rowsum_max_kernel (csrc/mixed.hip) restated tile by tile: lane l of a tile owns
    rows ra, rb = (2l, 2l + 1) [VIN] or (l, l + 64); wave w adds |a| over the columns c = w, w + 4, .. in ascending order, the four
    waves' sums are added as ((s0 + s1) + s2) + s3, a row's tiles in tile order.  F starts as SENTINEL32 everywhere."""
    n = A.shape[0]
    conv = {"truncation": truncate32, "half_away": half_away32}.get(mutation, expected_image)
    F = np.full((n, n), SENTINEL32, dtype=np.float32)
    nti, ntj = (n + DM_TI - 1) // DM_TI, (n + DM_TJ - 1) // DM_TJ
    part = np.zeros((ntj, n))
    lane = np.arange(64)
    ra, rb = (2 * lane, 2 * lane + 1) if vin else (lane, lane + 64)
    for bx in range(nti):
        for by in range(ntj):
            tj = (by + bx) % ntj                                   # the diagonal tile order
            i0, j0 = bx * DM_TI, tj * DM_TJ
            P = np.zeros((DM_TI, DM_TJ))
            blk = A[i0:i0 + DM_TI, j0:j0 + DM_TJ]
            P[:blk.shape[0], :blk.shape[1]] = blk
            oka, okb = i0 + ra < n, i0 + rb < n
            va, vb = P[ra] * oka[:, None], P[rb] * okb[:, None]
            if vin and mutation == "missing_last_odd_row":         # no scalar fallback where the pair is cut by the edge
                va = va * okb[:, None]
            tile = np.zeros((DM_TI, DM_TJ), dtype=np.float32)
            if mutation == "exchanged_rows":
                tile[ra], tile[rb] = conv(vb), conv(va)
            else:
                tile[ra], tile[rb] = conv(va), conv(vb)
            rsum = np.zeros((4, DM_TI))
            for w in range(4):
                sa, sb = np.zeros(64), np.zeros(64)
                for c in range(w, DM_TJ, 4):
                    sa, sb = sa + np.abs(va[:, c]), sb + np.abs(vb[:, c])
                rsum[w, ra], rsum[w, rb] = sa, sb
            rows = min(DM_TI, n - i0)
            part[tj, i0:i0 + rows] = (((rsum[0] + rsum[1]) + rsum[2]) + rsum[3])[:rows]
            cols = min(DM_TJ, n - j0)
            if mutation == "dropped_last_column" and cols < DM_TJ:
                cols -= 1
            # VOUT stores 16 float4 per row and the columns of a cut float4 one by one, the other form one element per lane: the
            # same elements are written either way
            F[i0:i0 + rows, j0:j0 + cols] = tile[:rows, :cols]
    s = np.zeros(n)
    for t in range(ntj):
        s = s + part[t]
    return F, float(s.max())


# ---- B. the refinement loop ----------------------------------------------------------------------------------------------------------
S_REAL = 30
REFINE_N = [1, 63, 64, 65, 129, 513]
REFINE_NRHS = [1, 8, 9, 33, 65]       # 9: two residual passes, 8 + 1; 65: a second tile of convert_transpose
PATTERNS = ["none", "all", "mixed_a", "mixed_b"]
LOOP_MUTATIONS = ["wrong_column", "rule_first_column_only", "rule_last_column_only", "double_update", "iters_off_by_one"]


def scaled_columns(nrhs, pattern):
    """Which columns get c_k = 1 + 2^-s.  mixed_a: the first, the last and every third one between; mixed_b: its complement (the first
    and the last column keep c = 1, so a rule that reads one of them alone stops too early).  With one column both are 'all'; with
    two, mixed_a is the first and mixed_b the last."""
    k = np.arange(nrhs)
    if pattern == "none":
        return np.zeros(nrhs, dtype=bool)
    if pattern == "all" or nrhs == 1:
        return np.ones(nrhs, dtype=bool)
    a = (k % 3 == 0) | (k == nrhs - 1) if nrhs > 2 else (k == 0)
    return a if pattern == "mixed_a" else ~a


class RefineCase:
    """n, nrhs; F32 (n x n float32, C order: the row-major packed L\\U); ipiv (1-based int64); A (float64, Fortran order, integers);
    anorm (exact); x0, b0 = A x0 (int64); L, U (dense float32, for the restatement)."""

    def rhs(self, pattern, s):
        """(B, Xwant, mask): B[:, k] = c_k b0[:, k] and the solution c_k x0[:, k], Float64, Fortran order"""
        mask = scaled_columns(self.nrhs, pattern)
        c = np.where(mask, 1.0 + 2.0 ** -s, 1.0)
        return np.asfortranarray(self.b0 * c), np.asfortranarray(self.x0 * c), mask


@functools.lru_cache(maxsize=None)
def refine_case(n, nrhs):
    """SolveCase(n, nrhs, seed) with the smallest seed whose first and last columns of x0 are not zero (n = 1 draws one number per
    column from [-4, 4]): a zero column meets the rule whatever c_k is."""
    for seed in range(64):
        sc = solve_case(n, nrhs, seed)
        if np.any(sc.x_true[:, 0]) and np.any(sc.x_true[:, -1]):
            break
    else:
        raise AssertionError("no seed gives nonzero first and last columns")
    c = RefineCase()
    c.n, c.nrhs, c.seed, c.ipiv = n, nrhs, seed, sc.ipiv
    L, U = sc.L().toarray(), sc.U().toarray()
    A = sc.apply_pt(L @ U)                                            # int64, exact
    c.x0 = sc.x_true
    c.b0 = sc.b_forward()
    assert np.array_equal(A @ c.x0, c.b0)
    c.A = np.asfortranarray(A.astype(np.float64))
    c.anorm = float(np.abs(A).sum(axis=1).max())
    c.F32 = np.ascontiguousarray(sc.dense_factors(np.float32))
    c.L, c.U, c.perm = L.astype(np.float32), U.astype(np.float32), sc.perm()
    c.term_sum = int((np.abs(A) @ np.abs(c.x0) + np.abs(c.b0)).max())  # the largest row sum of the moduli of ALL terms of B - A X
    for a in (c.A, c.F32, c.x0, c.b0):
        a.setflags(write=False)
    return c


def rule_holds_exactly(rn, xn, anorm, n):
    """||r|| <= ||x|| anorm eps sqrt(n) in exact arithmetic: both sides are >= 0, so the squares are compared as fractions"""
    lhs, rhs = Fraction(float(rn)), Fraction(float(xn)) * Fraction(float(anorm)) * Fraction(EPS)
    return lhs * lhs <= rhs * rhs * int(n)


def refine_proof(c, pattern, s, grid=1.0, modulus=np.abs):
    """The conditions of part B for one case and pattern; returns (bits of the largest term sum, the smallest factor by which a column
    misses the rule at step 0).  `grid`: the unit all entries are multiples of (1 for the real cases, 1/2 for the complex ones)."""
    B, Xw, mask = c.rhs(pattern, s)
    assert s >= 25
    bits = int(c.term_sum / grid).bit_length()
    assert bits + s <= 53, (bits, s)                                  # no Float64 sum of B - A X rounds, in any order
    scaled = np.where(mask, 2.0 ** -s, 0.0)
    assert np.array_equal(B, c.b0 + c.b0 * scaled) and np.array_equal(Xw, c.x0 + c.x0 * scaled)   # c_k b0 and c_k x0 are Float64 numbers
    assert np.array_equal(B.astype(_narrow(B)), c.b0.astype(_narrow(B)))                         # demote(B) == b0
    R0 = c.b0 * scaled                                                # the residual after step 0, exact
    assert np.array_equal(R0.astype(_narrow(B)).astype(B.dtype), R0)                             # demote(R) is exact
    rn, xn = modulus(R0).max(axis=0), modulus(c.x0).max(axis=0)
    missed = [k for k in range(c.nrhs) if not rule_holds_exactly(rn[k], xn[k], c.anorm, c.n)]
    assert (len(missed) > 0) == bool(mask.any())                      # the rule fails at step 0 iff a column is scaled ...
    assert set(missed) <= set(np.flatnonzero(mask))
    margin = min((rn[k] / (xn[k] * c.anorm * EPS * math.sqrt(c.n)) for k in missed), default=math.inf)
    assert margin >= 2.0 ** 10                                        # ... by far more than any rounding of the norms or of sqrt
    # and holds at step 1 and for c = 1: the residual is exactly 0 there, and 0 <= anything that is no NaN
    x1 = modulus(Xw).max(axis=0)
    assert np.all(np.isfinite(x1)) and all(rule_holds_exactly(0.0, x1[k], c.anorm, c.n) for k in range(c.nrhs))
    return bits, margin


def _narrow(M):
    return np.complex64 if np.iscomplexobj(M) else np.float32


def refine_restated(c, B, anorm, max_iter=30, mutation=None):
    """mixed_getrs of csrc/driver.cpp in numpy: Float32 solves on the dense factors (scipy's triangular solves: one more summation
    order), Float64 residuals, the per-column rule.  Returns (X, iters)."""
    import scipy.linalg as sla

    n, nrhs = B.shape
    narrow = _narrow(B)

    def solve32(S):
        y = S.astype(narrow)[c.perm]
        y = sla.solve_triangular(c.L, y, lower=True, unit_diagonal=True, check_finite=False)
        return sla.solve_triangular(c.U, y, lower=False, check_finite=False).astype(narrow).astype(B.dtype)

    scale = anorm * EPS * math.sqrt(n)
    X = solve32(B)
    step = 0
    while True:
        with np.errstate(invalid="ignore"):
            R = B - c.A @ X
            rn, xn = np.abs(R).max(axis=0), np.abs(X).max(axis=0)
        cols = {"rule_first_column_only": [0], "rule_last_column_only": [nrhs - 1]}.get(mutation, range(nrhs))
        if all(rn[k] <= xn[k] * scale for k in cols):
            return X, step + (1 if mutation == "iters_off_by_one" else 0)
        if step >= max_iter:
            return X, -(step + 1)
        d = solve32(R)
        if mutation == "wrong_column":
            d = np.roll(d, 1, axis=1)
        X = X + d + (d if mutation == "double_update" else 0)
        step += 1


# ---- C. the residual alone -----------------------------------------------------------------------------------------------------------
RESIDUAL_N = [1, 511, 512, 513, 1025]       # the 512-row workgroup of residual_few (256 rows for complex) and several column slices
RESIDUAL_NRHS = list(range(1, 10))          # every width of a pass, and 9 = 8 + 1


@functools.lru_cache(maxsize=None)
def residual_case(n, cplx=False):
    """(A, X, B, R): integers (Gaussian integers if cplx) with parts in [-4, 4], 9 columns, R = B - A X in int64 arithmetic; returned as
    Float64 / ComplexF64 arrays (every sum is below 2^53 by far)."""
    rng = np.random.default_rng([43000, n, int(cplx)])
    k = max(RESIDUAL_NRHS)

    def draw(rows, cols):
        return rng.integers(-4, 5, size=(rows, cols)), (rng.integers(-4, 5, size=(rows, cols)) if cplx else np.zeros((rows, cols), dtype=np.int64))

    (ar, ai), (xr, xi), (br, bi) = draw(n, n), draw(n, k), draw(n, k)
    if n == 1:
        ar[0, 0] = 3                                                  # (a zero matrix would leave R = B)
    rr, ri = br - (ar @ xr - ai @ xi), bi - (ar @ xi + ai @ xr)
    pack = (lambda re, im: np.asfortranarray(re + 1j * im)) if cplx else (lambda re, im: np.asfortranarray(re.astype(np.float64)))
    out = tuple(pack(re, im) for re, im in ((ar, ai), (xr, xi), (br, bi), (rr, ri)))
    for a in out:
        a.setflags(write=False)
    return out
