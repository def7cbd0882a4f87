"""Inputs and CPU references of the real inv / det / logabsdet tests (tests/test_inv_cases.py, tests/test_gpu_inv.py,
tests/test_gpu_inv_exact.py).  Pure numpy (and the CPU oracle for the factors of the random inputs), no GPU, no torch.

  * matrix / host_batch: the random inputs of tests/test_gpu_inv.py (one definition for the GPU test and for the CPU measurement);
  * rho: LAPACK's xGET03 ratios ||A X - I||_1 / (n eps_T ||A||_1 ||X||_1) and the same with X A, evaluated in Float64;
  * exact_case: CONSTRUCTED real factors (nothing is computed by an elimination) whose inverse is known exactly -- see its docstring;
    complex_inv_cases.partial_sum_bits (with |M| = |re|) bounds the bits of every partial sum of any blocked inverse of them;
  * getri_transcription (imported from complex_inv_cases: getri_view<E> of csrc/inverse.hip is one host path for real and complex
    elements, and the transcription does not care about the element type): the two sweeps in numpy with the index arithmetic of the drivers;
  * batched_restatement: getri_batched_kernel of csrc/batched.hip in numpy, in the kernel's own order and in the element's precision;
    compose_interchanges and bsubstitute (column- and row-reading) also serve the restatement of the batched SOLVE in
    tests/batched_solve_cases.py."""
import functools
import math
import os
import re
from fractions import Fraction

import numpy as np

import oracle as O
from complex_inv_cases import (_blk64_mode0, _trmm_rect_rec, _trtri_sweep, getri_transcription, partial_sum_bits,  # noqa: F401
                               perm_of)
from helpers import rand_matrix

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "recursivefactorization.jl_amd", "csrc")


def header_constants():
    """NB, GETRI_W, BATCHED_MAX_DIM (csrc/rflu_internal.hpp) and BNR (csrc/batched_kernels.hpp, used by csrc/batched.hip) as the sources
    state them: a change of one of them fails tests/test_inv_cases.py instead of moving a boundary away from the sizes below."""
    internal = open(os.path.join(CSRC, "rflu_internal.hpp")).read()
    kernels = open(os.path.join(CSRC, "batched_kernels.hpp")).read()
    return {
        "NB": int(re.search(r"constexpr int NB = (\d+);", internal).group(1)),
        "GETRI_W": int(re.search(r"constexpr int64_t GETRI_W = (\d+);", internal).group(1)),
        "BATCHED_MAX_DIM": int(re.search(r"constexpr int64_t BATCHED_MAX_DIM = (\d+);", internal).group(1)),
        "BNR": int(re.search(r"constexpr int BNR = (\d+);", kernels).group(1)),
    }


NB, GETRI_W, BNR, BATCHED_MAX_DIM = 64, 512, 8, 128       # asserted against header_constants() in tests/test_inv_cases.py
DTYPES = [np.float64, np.float32]

# ---- the random inputs of tests/test_gpu_inv.py -------------------------------------------------------------------------------------
SIZES = [1, 2, 63, 64, 65, 127, 128, 129, 200, 511, 512, 513, 1025, 1100, 2112]   # every 64-row boundary up to 128, W-1, W, W+1, 2W+1
VARIANT_SIZES = [65, 200, 513]
BATCH_CASES = [(n, 200) for n in (1, 2, 7, 8, 33, 64, 65, 100, 128)] + [(64, 1), (64, 257)]
# seed of the n x n input: 91000 + n, except where that matrix is too ill-conditioned for the ABSOLUTE logabsdet bar 8 n eps_T of
# tests/test_gpu_inv.py to mean anything -- there the CPU oracle's own factors miss it (n = 2: cond 551, off by 10 n eps in both element
# types; 511, 512, 1025: 13 .. 15 n eps64); the next seed in steps of 3000 at which oracle.lu stays within 2 n eps_T is taken
# (scripts/inv_cpu_bars.py)
SEEDS = {2: 94002, 511: 97511, 512: 97512, 1025: 98025}


@functools.lru_cache(maxsize=None)
def _matrix(n, dtype, diag):
    A = np.array(rand_matrix(n, n, seed=SEEDS.get(n, 91000 + n), dtype=dtype), order="F")
    if diag:
        A += dtype(10) * np.eye(n, dtype=dtype)
    A.setflags(write=False)
    return A


def matrix(n, dtype, diag=False):
    """rand_matrix(n, n, seed=SEEDS.get(n, 91000 + n), dtype), + 10 I for NoPivot."""
    return _matrix(n, np.dtype(dtype).type, bool(diag))


@functools.lru_cache(maxsize=None)
def _batch(n, batch, dtype):
    out = np.stack([rand_matrix(n, n, seed=93000 + b, dtype=dtype) for b in range(batch)])
    out.setflags(write=False)
    return out


def host_batch(n, batch, dtype):
    """Matrix b of a batch is rand_matrix(n, n, seed=93000 + b, dtype)."""
    return _batch(n, batch, np.dtype(dtype).type)


def rho(A, X, dtype, exact=False):
    """(rho_R, rho_L) in Float64, as tests/test_gpu_inv.py evaluates them; a non-finite X gives inf.  exact=True evaluates the two
    ratios in rational arithmetic (for the smallest sizes only: the cost grows fast).  Why it exists: for Float64 data the Float64
    evaluation of A X - I rounds at the size of the residual itself.  That does not matter where the ratio is far from its bar, and it
    decides at n = 1: there the inverse is ONE correctly rounded reciprocal x = (1 / a)(1 + d), |d| <= u / (1 + u) with u = eps / 2, so
    |a x - 1| = |d| and |a| |x| >= 1 / (1 + u) give rho <= 1/2 exactly -- attained, and the rounded evaluation reports 0.5000000000000001."""
    A64, X64 = np.asarray(A, dtype=np.float64), np.asarray(X, dtype=np.float64)
    n = A64.shape[0]
    if not np.isfinite(X64).all():
        return math.inf, math.inf
    if exact:
        fa = [[Fraction(float(v)) for v in row] for row in A64]
        fx = [[Fraction(float(v)) for v in row] for row in X64]
        one_norm = lambda M: max(sum(abs(M[i][j]) for i in range(n)) for j in range(n))   # noqa: E731
        mul = lambda P, Q: [[sum(P[i][k] * Q[k][j] for k in range(n)) - (1 if i == j else 0) for j in range(n)] for i in range(n)]   # noqa: E731
        scale = n * Fraction(float(np.finfo(dtype).eps)) * one_norm(fa) * one_norm(fx)
        return float(one_norm(mul(fa, fx)) / scale), float(one_norm(mul(fx, fa)) / scale)
    scale = n * float(np.finfo(dtype).eps) * np.linalg.norm(A64, 1) * np.linalg.norm(X64, 1)
    eye = np.eye(n)
    return float(np.linalg.norm(A64 @ X64 - eye, 1) / scale), float(np.linalg.norm(X64 @ A64 - eye, 1) / scale)


RHO_BAR = 1.0            # the bar of tests/test_gpu_inv.py, every size


def half_bar(n):
    """What a CPU restatement alone has to meet on the random inputs: half the GPU bar."""
    return 0.5 * RHO_BAR


def cpu_factors(A):
    """(F, ipiv) of the CPU oracle (the GPU's elimination order) in the element type of A; the input must not be singular."""
    F, ipiv, info = O.lu(np.array(A, order="F"))
    assert info == 0, info
    return F, ipiv


# ---- constructed factors with an exactly known inverse ---------------------------------------------------------------------------
EXACT_SIZES = [65, 130, 513, 577, 1025]
BATCHED_EXACT_SIZES = [1, 2, 3, 7, 8, 33, 64, 65, 100, 128]
EXACT_COPIES = 5         # differently seeded exact cases per size in the batched test
EXACT_BATCH = 67         # the last workgroup is partly empty for 4, 2 and 1 groups per workgroup
UNITS = np.array([1.0, -1.0, 1.0, -1.0])                  # four draws, as the complex construction has them: the same draw order
DIAG = np.array([1.0, -1.0, 2.0, -2.0, 0.5, -0.5])
SCALE_BITS = 24          # the exact inverse is held as integers times 2^-SCALE_BITS
# seed of exact_case(n, copy): 97000 + n + 3000 * copy.  partial_sum_bits stays <= 24 at every (size, copy) used (tests/test_inv_cases.py
# asserts it and prints the counts).  One seed is replaced: at n = 1025 the default 98025 (23 bits) leaves three all-zero 64 x 64
# off-diagonal blocks in X -- (2, 9), (2, 14), (6, 15) -- behind which a dropped block would hide; in steps of 3000 the seeds
# 101025 and 107025 need 26 and 25 bits, 104025, 110025 and 113025 leave zero blocks again, 116025 is the first with neither fault
# (22 bits, no zero block)
EXACT_SEEDS = {(1025, 0): 116025}


class ExactCase:
    """n; F: packed L\\U (float64, Fortran order); ipiv (1-based int64); A = P^T L U; X = A^-1, every entry a dyadic rational, certified in
    integer arithmetic; Y = U^-1 L^-1 (the NotIPIV result); sign, log2_absdet: det A = sign * 2^log2_absdet; L, U."""


def _int_of(Z, bits):
    """int64 array of Z * 2^bits, which must be integral."""
    S = np.asarray(Z, dtype=np.float64) * float(2 ** bits)
    R = np.rint(S)
    assert np.array_equal(R, S), "not a dyadic rational at this scale"
    assert np.abs(R).max(initial=0) < 2.0 ** 40
    return R.astype(np.int64)


@functools.lru_cache(maxsize=None)
def exact_case(n, copy=0):
    """L unit lower and U upper, each bidiagonal plus a few far entries, off-diagonal entries in {0, +-1}, U's diagonal in
    {+-1, +-2, +-1/2}; ipiv moves every row (ipiv[k] > k + 1 for k < n - 1; the last row is moved by the earlier ones).  The bidiagonals are
    cut after every third entry so that the chains of the inverses stay short (three long, six where a cut would fall on a multiple of 64
    and is left out, so that a chain straddles EVERY 64-row boundary) and every magnitude small; the far entries reach across the 64-row
    blocks and, from n = 513 on, across the block columns of width 512.  This is complex_inv_cases.exact_case with real units and a real
    diagonal, drawn in the same order.

    The inverse: Y = U^-1 L^-1 is first formed in float64, then CERTIFIED in integer arithmetic -- with every number an integer times a
    power of two, (2 L U) (2^24 Y) == 2^25 I holds exactly in int64 -- and a nonsingular matrix has one inverse.  A^-1 = Y P, i.e.
    column p[i] of X is column i of Y."""
    rng = np.random.default_rng(EXACT_SEEDS.get((n, copy), 97000 + n + 3000 * copy))
    L = np.eye(n)
    U = np.zeros((n, n))
    U[np.arange(n), np.arange(n)] = DIAG[rng.integers(0, len(DIAG), size=n)]
    for k in range(1, n):
        if k % 3 != 0 or k % NB == 0:
            L[k, k - 1] = UNITS[rng.integers(0, 4)]
            U[k - 1, k] = UNITS[rng.integers(0, 4)]
    far = [(n - 1, 0), (n - 2, 4), (n // 2 + 1, 3), (n - 1, n // 2)]
    far += [(70 + 64 * q, 2 + 64 * q) for q in range((n - 71) // 64 + 1) if 70 + 64 * q < n]
    for (i, j) in far:
        if 0 <= j < i - 1 < n:
            L[i, j] = UNITS[rng.integers(0, 4)]
            U[j, i] = UNITS[rng.integers(0, 4)]
    ipiv = np.array([int(rng.integers(k + 2, n + 1)) for k in range(n - 1)] + [n], dtype=np.int64)
    M = L @ U                                              # exact: small half-integers, short sums
    Y = np.linalg.solve(U, np.linalg.solve(L, np.eye(n)))
    M2, Yi = _int_of(M, 1), _int_of(Y, SCALE_BITS)
    rows, cols = np.nonzero(M2)                            # a handful of entries per row: the int64 product row by nonzero entry
    P = np.zeros((n, n), dtype=np.int64)
    np.add.at(P, rows, M2[rows, cols][:, None] * Yi[cols])  # int64: exact (|2 m| <= 8, |2^24 y| < 2^40, at most n terms)
    assert np.array_equal(P, (2 ** (SCALE_BITS + 1)) * np.eye(n, dtype=np.int64)), "the inverse is not exact"
    p = perm_of(ipiv, n)
    A = np.zeros((n, n))
    A[p, :] = M                                            # P A = L U
    X = np.zeros((n, n))
    X[:, p] = Y
    c = ExactCase()
    c.n, c.ipiv, c.A, c.X, c.Y = n, ipiv, np.asfortranarray(A), np.asfortranarray(X), np.asfortranarray(Y)
    c.F = np.asfortranarray(np.tril(L, -1) + U)
    d = np.diagonal(U)
    c.log2_absdet = int(np.sum(np.abs(d) == 2)) - int(np.sum(np.abs(d) == 0.5))
    c.sign = -1.0 if (int(np.sum(d < 0)) + int(np.sum(ipiv != np.arange(1, n + 1)))) % 2 else 1.0   # each interchange a factor -1
    c.L, c.U = L, U
    for a in (c.A, c.X, c.Y, c.F, c.ipiv):
        a.setflags(write=False)
    return c


def exact_bits(n, copy=0):
    """Significant bits any partial sum of any blocked inverse of exact_case(n, copy) needs: magnitude plus granularity."""
    magnitude, granularity = partial_sum_bits(exact_case(n, copy))
    return magnitude + granularity


# ---- getri_batched_kernel, restated ------------------------------------------------------------------------------------------------
def compose_interchanges(ipiv, n, ignore_p1=False):
    """sperm of csrc/batched.hip: the interchanges k <-> ipiv[k] - 1, k = 0 .. n - 1, composed on the identity held as two entries per
    lane (p0: rows 0 .. 63, p1: rows 64 .. 127); an entry with p <= k or p >= n is skipped (nothing to exchange, or not an interchange
    getrf could have written).  Row i of P * I is row sperm[i] of I.  ignore_p1 (a mutation): what is written to the p1 half is lost."""
    half = [np.arange(64), np.arange(64, 128)]
    if ipiv is not None:
        for k in range(n):
            p = int(ipiv[k]) - 1
            if p <= k or p >= n:
                continue
            vk, vp = half[k >> 6][k & 63], half[p >> 6][p & 63]
            if not (ignore_p1 and k >= 64):
                half[k >> 6][k & 63] = vp
            if not (ignore_p1 and p >= 64):
                half[p >> 6][p & 63] = vk
    return np.concatenate(half)[:n]


def bsubstitute(F, x, trans=False, mutation=None):
    """bsubstitute<T, false> of csrc/batched.hip on the columns of x, in place: L (unit) forward, column-oriented -- after step k every
    row below takes f * x_k out of itself; U backward -- every row above takes f * (x_k / u_kk) out of itself, a DIVISION per use, the
    stored x_k staying undivided; then every row is divided by its own diagonal entry.  The precision is that of F; whether a product and
    a difference are contracted into one fused operation is the compiler's choice and is not restated (it moves single roundings, and
    nothing where every operation is exact).
    trans=True is bsubstitute<T, true>: the same image read by rows, bf(i, k) = F[k, i] -- U^T, a NON-unit lower triangle, forward with
    the division per use and the stored x_k undivided, then every row divided by its diagonal entry, then L^T (unit) backward.
    mutation (tests/test_batched_solve_cases.py): "backward_skips_last_column" starts the backward sweep at column n - 2,
    "no_final_division" leaves every row undivided."""
    n = F.shape[0]
    T = F.T if trans else F                               # T[i, k] = bf<T, TRANS>(s, ld, i, k)
    diag = np.diagonal(F)
    top = n - 2 if mutation == "backward_skips_last_column" else n - 1
    with np.errstate(all="ignore"):
        for k in range(n):
            xk = x[k:k + 1] / diag[k] if trans else x[k:k + 1]
            x[k + 1:] -= T[k + 1:, k:k + 1] * xk
        if trans and mutation != "no_final_division":
            x /= diag[:, None]
        for k in range(top, -1, -1):
            xk = x[k:k + 1] if trans else x[k:k + 1] / diag[k]
            x[:k] -= T[:k, k:k + 1] * xk
        if not trans and mutation != "no_final_division":
            x /= diag[:, None]


def batched_restatement(F, ipiv, row_major=False, passes=True, inverse_perm=False, swap_store=False, ignore_p1=False):
    """The memory image rflu_getri_batched_*_dev leaves for ONE matrix, as an (n, n) C-ordered array `out` with out[a, b] the element at
    offset a * n + b: the column-major call stores X[i, j] at j * n + i, the row-major one at i * n + j.  F: the packed factors as a
    matrix (whatever their storage was: the kernel loads either orientation into the same LDS image), in the element type.
    passes=True makes the BNR = 8 columns of P * I of each pass and substitutes pass by pass, as the kernel does; passes=False
    substitutes all n columns at once -- the same operations on every element (columns never meet), far fewer numpy calls.
    The other keywords are the mutations of tests/test_inv_cases.py: the inverse permutation in place of sperm, the two store branches
    exchanged, the p1 half of the composition ignored."""
    F = np.asarray(F)
    n = F.shape[0]
    T = F.dtype.type
    sperm = compose_interchanges(ipiv, n, ignore_p1=ignore_p1)
    if inverse_perm:
        inv = np.empty(n, dtype=np.int64)
        inv[sperm] = np.arange(n)
        sperm = inv
    out = np.zeros((n, n), dtype=F.dtype)
    to_rows = bool(row_major) != bool(swap_store)
    step = BNR if passes else max(n, 1)
    for j0 in range(0, n, step):
        nr = min(step, n - j0)
        one = sperm - j0
        x = np.where(one[:, None] == np.arange(nr)[None, :], T(1), T(0)).astype(F.dtype)   # row r: 1 in column sperm[r] - j0
        bsubstitute(F, x)
        if to_rows:
            out[:, j0:j0 + nr] = x                         # X[i * ldi + j0 + j]
        else:
            out[j0:j0 + nr, :] = x.T                       # X[i + (j0 + j) * ldi]
    return out


def batched_inverse(F, ipiv, **kw):
    """The inverse as a matrix from batched_restatement's column-major image."""
    return batched_restatement(F, ipiv, row_major=False, **kw).T
