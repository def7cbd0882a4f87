"""Inputs, references and the CPU restatement for the tests that hold the BATCHED solves -- rflu_getrs_batched_{f64,f32}_dev
(getrs_batched_kernel, csrc/batched.hip) and rflu_getrs_batched_{cf64,cf32}_dev (cgetrs_batched_kernel, csrc/batched_complex.hip) -- to
exact and rounding-level references (tests/test_batched_solve_cases.py proves them on the CPU, tests/test_gpu_batched_solve_exact.py
uses them on the GPU).  Pure numpy / scipy (and the CPU oracle for the factors of the random inputs), no GPU, no torch.

  * member(n, kind, copy): CONSTRUCTED dense factors, interchanges and a small-integer solution for one member of a batch, with the
    right-hand sides of every operator formed in int64 and the certificate (the largest sum of the moduli of all terms of any row's
    substitution) that makes `==` a fair demand in any order of summation.  See its docstring.
  * INTERCHANGES: the special sequences -- the identity, ipiv[k] = n for every k, every k < 64 exchanged with a row >= 64.
  * restatement: both kernels' solve in numpy in the element type: the interchanges composed in two halves
    (inv_cases.compose_interchanges), passes of BNR right-hand sides, the gather in front (N) or the scatter behind (T, C) through sperm,
    both orientations of F and B, member b at b * strideF / b * strideB / b * stride_ipiv, the real kernel's division of x_k by every
    reader (inv_cases.bsubstitute, column- and row-reading) and the complex kernel's one reciprocal per column by Smith's formula
    followed by multiplications (cbsubstitute here).  `mutation` plants one of MUTATIONS.
  * general inputs: the uniform matrices and right-hand sides of tests/test_gpu_batched.py and tests/complex_batched_cases.py, factored
    with pivoting and no diagonal shift, and omega_batch: the componentwise backward error of tests/test_gpu_solve_exact.py and
    tests/complex_solve_cases.py for every member of a batch, in numpy.longdouble / clongdouble on the rounded factors.

What the exact cases do NOT exercise: rounding (every operation on them is exact); the rounding cases cover that side."""
import functools
import os
import re

import numpy as np

import complex_batched_cases as CB
import complex_batched_inv_cases as CBI
import complex_ref as CR
import inv_cases as IC
from complex_inv_cases import DIAG as CDIAG
from complex_solve_cases import _cmul
from helpers import rand_matrix

CSRC = IC.CSRC
BNR, BT, BATCHED_MAX_DIM, CBATCHED_MAX_DIM_CF32, CBATCHED_MAX_DIM_CF64 = 8, 256, 128, 128, 64   # asserted against header_constants()
SFX = ("f64", "f32", "cf64", "cf32")
DTYPE = {"f64": np.float64, "f32": np.float32, "cf64": np.complex128, "cf32": np.complex64}
KIND = {"f64": "real", "f32": "real", "cf64": "complex", "cf32": "complex"}
LIMIT = {"f64": BATCHED_MAX_DIM, "f32": BATCHED_MAX_DIM, "cf64": CBATCHED_MAX_DIM_CF64, "cf32": CBATCHED_MAX_DIM_CF32}
OPS = {"real": ("N", "T"), "complex": ("N", "T", "C")}
TRANS_CODE = {"N": 0, "T": 1, "C": 2}
FLOAT32_LIMIT = float(2 ** 24)

# 1: one row, nothing to substitute; 2: one term; 7 | 8 | 9: the row-major load's eight lanes per row, one pass of rows more; 31 | 32 |
# 33 and 63 | 64 | 65: the group of threads doubles (4 / 2 / 1 matrices per workgroup), 64 | 65 also the p0 / p1 halves of the composed
# interchanges; 100: no power of two; 127 | 128: the limit
GRID_N = [1, 2, 7, 8, 9, 31, 32, 33, 63, 64, 65, 100, 127, 128]
GRID_NRHS = [1, 7, 8, 9, 16, 17]       # a partial pass, a full one, one column into the second, two full ones, one into the third
FULL_NRHS_N = (8, 9, 33, 64, 65, 128)  # these sizes meet every nrhs, the others 1 and 9
BATCHES = [1, 3, 5, 67]                # 67: the last workgroup is partly empty for 4, 2 and 1 matrices per workgroup
NRHS_MAX = max(GRID_NRHS)
ABOVE = {"f64": 129, "f32": 129, "cf64": 65, "cf32": 129}   # one past the limit: the loop over the single-matrix path
ABOVE_BATCH = 3
STORAGE_N, STORAGE_NRHS = (9, 65, 128), (1, 9)
ROUNDING_N, ROUNDING_NRHS, ROUNDING_BATCH = (8, 33, 64, 100, 128), (1, 9), 67
SPECIAL_N = (65, 128)
INTERCHANGES = ("identity", "last", "cross")
CPU_MEMBERS = 6                        # members of a batch whose omega tests/test_batched_solve_cases.py computes from the restatement
M_RATIO, FLOOR = 16.0, 1.0 / 8.0       # omega <= M_RATIO max(omega_ref, FLOOR eps): tests/test_gpu_solve_exact.py


def header_constants():
    """BNR, BT (csrc/batched_kernels.hpp), BATCHED_MAX_DIM and the two complex one-launch limits (csrc/rflu_internal.hpp) as the
    sources state them: a change of one of them fails tests/test_batched_solve_cases.py instead of moving a boundary away from the grids."""
    internal = open(os.path.join(CSRC, "rflu_internal.hpp")).read()
    kernels = open(os.path.join(CSRC, "batched_kernels.hpp")).read()
    return {
        "BNR": int(re.search(r"constexpr int BNR = (\d+);", kernels).group(1)),
        "BT": int(re.search(r"constexpr int BT = (\d+);", kernels).group(1)),
        "BATCHED_MAX_DIM": int(re.search(r"constexpr int64_t BATCHED_MAX_DIM = (\d+);", internal).group(1)),
        "CBATCHED_MAX_DIM_CF32": int(re.search(r"constexpr int64_t CBATCHED_MAX_DIM_CF32 = (\d+);", internal).group(1)),
        "CBATCHED_MAX_DIM_CF64": int(re.search(r"constexpr int64_t CBATCHED_MAX_DIM_CF64 = (\d+);", internal).group(1)),
    }


def eps_of(sfx):
    return float(np.finfo(DTYPE[sfx]).eps)


def sizes(sfx):
    """GRID_N cut at the one-launch limit of the element type"""
    return [n for n in GRID_N if n <= LIMIT[sfx]]


def nrhs_of(n):
    return GRID_NRHS if n in FULL_NRHS_N else [1, 9]


def exact_grid(sfx):
    """(n, nrhs, batch, ipiv given) of part (a) of the GPU test: every n with its nrhs; the batch and whether ipiv is given or NULL
    cycle through their eight combinations along the list, and every case runs every operator in both orientations -- so every value of
    every axis meets every operator and both orientations."""
    combos = [(b, g) for g in (True, False) for b in BATCHES]
    combos = combos[:4] + combos[5:] + combos[4:5]          # (1, NULL) last: the cycle of 8 does not lock onto the nrhs cycle of 6
    out = []
    for n in sizes(sfx):
        for nrhs in nrhs_of(n):
            batch, given = combos[len(out) % len(combos)]
            out.append((n, nrhs, batch, given))
    return out


# ---- constructed members ------------------------------------------------------------------------------------------------------------------
RDIAG = np.array([1.0, -1.0, 2.0, -2.0, 0.5, -0.5])
GAUSS = np.array([0, 1, -1, 1j, -1j])


def interchanges(n, which, rng=None):
    """1-based ipiv.  "random": ipiv[k] a random row in [k, n) (0-based), so targets repeat; "identity"; "last": ipiv[k] = n for every
    k, the deepest composition (row n - 1 travels through every position); "cross": every k < 64 exchanges with a row >= 64 (every
    exchange crosses the p0 / p1 halves; at n = 65 that row is always 64, at n = 128 it is 64 + (37 k + 11) mod 64, every row of the
    upper half once), rows from 64 stay."""
    k = np.arange(n, dtype=np.int64)
    if which == "random":
        return np.array([i + 1 + rng.integers(0, n - i) for i in range(n)], dtype=np.int64)
    if which == "identity":
        return k + 1
    if which == "last":
        return np.full(n, n, dtype=np.int64)
    assert which == "cross" and n > 64
    return np.where(k < 64, 64 + (37 * k + 11) % (n - 64), k) + 1


def _gi(a):
    return np.rint(a.real).astype(np.int64), np.rint(a.imag).astype(np.int64)


def _cmatmul(a, b):
    return a[0] @ b[0] - a[1] @ b[1], a[0] @ b[1] + a[1] @ b[0]


def _hyp(p):
    return np.hypot(p[0].astype(np.float64), p[1].astype(np.float64))


class Member:
    """n, kind; F: packed L\\U (float64 / complex128, Fortran order; every entry a Float32 number); ipiv (1-based int64); X: n x NRHS_MAX,
    the solution of every operator; B[op]: n x NRHS_MAX with op(P^T L U) X = B[op] exactly; sums[op]: the largest sum over a row of
    the moduli of all terms of its substitution, either sweep, in units of the grid 1/2."""


@functools.lru_cache(maxsize=None)
def member(n, kind, copy=0, which="random"):
    """One member of a batch, seeded by (n, kind, copy): every copy has its own factors, interchanges and solution.

    real: L unit lower with entries from {-1, 0, 1}, U strictly upper from {-2 .. 2}, diag(U) from {+-1, +-2, +-1/2}, X integers in
    [-4, 4].  DENSE, unlike tests/solve_cases.py, whose triangles are bidiagonal inside a 64-row block (the single-matrix solve inverts
    its diagonal blocks, which only such triangles survive exactly): at n <= 64 those would not notice a substitution that drops every
    term but the neighbouring one.  complex: the recipe of complex_mixed_cases.exact_solve_case -- off-diagonal entries from
    {0, +-1, +-i}, diag(U) from complex_inv_cases.DIAG (units, +-2, +-2i, +-1/2), X with re, im in {-2 .. 2}.
    `which`: the interchanges (interchanges()); L, U and X do not depend on it.

    B['N'] = P^T L U X, B['T'] = U^T L^T P X and B['C'] (factors conjugated) are formed in int64 pairs on 2 U, so that the half-integer
    grid is integers.  Why a correct solve returns X by ==: every term of either substitution -- l_ij y_j, u_ij x_j, and for T / C
    u_ji y_j, l_ji z_j -- is a (Gaussian) integer times 1/2 known from X itself.  If the moduli of ALL terms of a row sum to less than
    2^24 grid units, every partial sum in any order is a grid point below 2^24 units and therefore a Float32 number: nothing is ever
    rounded.  The products are exact (a factor is 0, a unit, or a small integer times a power of two against a small integer), the
    real kernel's x_k / u_kk divides by a power of two, and the complex kernel's reciprocal of a unit, +-2, +-2i or +-1/2 by Smith's
    formula is a power of two times a unit.  tests/test_batched_solve_cases.py asserts the bound for every member used."""
    rng = np.random.default_rng([41000, n, 0 if kind == "real" else 1, copy])
    if kind == "real":
        L = np.tril(rng.integers(-1, 2, (n, n)), -1) + np.eye(n)
        U = np.triu(rng.integers(-2, 3, (n, n)), 1) + np.diag(RDIAG[rng.integers(0, len(RDIAG), n)])
        X = rng.integers(-4, 5, (n, NRHS_MAX)).astype(np.float64)
        L, U, X = L.astype(np.complex128), U.astype(np.complex128), X.astype(np.complex128)
    else:
        L = np.tril(GAUSS[rng.integers(0, 5, (n, n))], -1) + np.eye(n)
        U = np.triu(GAUSS[rng.integers(0, 5, (n, n))], 1) + np.diag(CDIAG[rng.integers(0, len(CDIAG), n)])
        X = rng.integers(-2, 3, (n, NRHS_MAX)) + 1j * rng.integers(-2, 3, (n, NRHS_MAX))
    ipiv = interchanges(n, which, rng)
    perm = CR.perm_of(ipiv, n)
    absL, absU2 = np.abs(np.tril(L, -1)), np.abs(np.triu(2 * U, 1))
    B2, sums = {}, {}
    # N: Y = U X, Z = L Y, B = P^T Z
    Y2 = _cmatmul(_gi(2 * U), _gi(X))
    Z2 = _cmatmul(_gi(L), Y2)
    B2["N"] = tuple(np.empty_like(p) for p in Z2)
    for dst, src in zip(B2["N"], Z2):
        dst[perm] = src                                    # (P B)[i] = B[perm[i]] = Z[i]
    sums["N"] = float(max((_hyp(Z2) + absL @ _hyp(Y2)).max(), (_hyp(Y2) + absU2 @ np.abs(X)).max()))
    # T, C: Y = L^T (P X), B = U^T Y
    for op in OPS[kind][1:]:
        Lo, U2o = (L.conj(), (2 * U).conj()) if op == "C" else (L, 2 * U)
        PX = _gi(X[perm])
        Y = _cmatmul(_gi(Lo.T), PX)
        B2[op] = _cmatmul(_gi(U2o.T), Y)
        first = (_hyp(B2[op]) + absU2.T @ _hyp(Y)).max()                  # 2 b_i and (2 u_ji) y_j
        second = (2 * _hyp(Y) + 2 * (absL.T @ _hyp(PX))).max()            # 2 y_i and 2 l_ji z_j
        sums[op] = float(max(first, second))
    c = Member()
    c.n, c.kind, c.ipiv, c.sums = n, kind, ipiv, sums
    F = np.tril(L, -1) + U
    c.B = {op: (p[0] + 1j * p[1]) / 2 for op, p in B2.items()}
    if kind == "real":
        F, X = F.real.copy(), X.real.copy()
        c.B = {op: b.real.copy() for op, b in c.B.items()}
    c.F, c.X = np.asfortranarray(F), np.asfortranarray(X)
    low = np.float32 if kind == "real" else np.complex64
    for a in (c.F, c.X, *c.B.values()):
        assert np.array_equal(a.astype(low).astype(a.dtype), a)           # Float32 numbers, all of them
        a.setflags(write=False)
    c.ipiv.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def above_member(sfx, copy):
    """The constructed member at ABOVE[sfx], where the batched entry loops over the single-matrix path.  complex: member().  real:
    tests/solve_cases.py's case (n, NRHS_MAX, seed = copy) -- the single-matrix real solve inverts its 64-row diagonal blocks, and the
    inverse of a DENSE unit triangle with entries +-1 has entries far beyond 2^24, so products with it are rounded in Float32 however
    exact the solution is; solve_cases' triangles, bidiagonal inside a block, are the ones proven exact for that path
    (tests/test_solve_cases.py), and what the loop adds -- member b at b * stride -- they notice as well as a dense member."""
    n = ABOVE[sfx]
    if KIND[sfx] == "complex":
        return member(n, "complex", copy)
    from solve_cases import solve_case

    s = solve_case(n, NRHS_MAX, seed=copy)
    c = Member()
    c.n, c.kind, c.ipiv = n, "real", s.ipiv
    c.F, c.X = s.dense_factors(np.float64), np.asfortranarray(s.x_true.astype(np.float64))
    c.B = {"N": s.b_forward().astype(np.float64), "T": s.b_transposed().astype(np.float64)}
    return c


# ---- the general inputs ---------------------------------------------------------------------------------------------------------------------
def general_matrix(n, sfx, b):
    """Matrix b of a batch: rand_matrix(n, n, seed=50000 + b) (tests/test_gpu_batched.py) / complex_batched_cases.matrix"""
    if KIND[sfx] == "real":
        return rand_matrix(n, n, seed=50000 + b, dtype=DTYPE[sfx])
    return CB.matrix(n, n, sfx, b)


def general_rhs(n, nrhs, sfx, b):
    """rand_matrix(n, nrhs, seed=70000 + b) (tests/test_gpu_batched.py) / complex_batched_cases.rhs"""
    if KIND[sfx] == "real":
        return rand_matrix(n, nrhs, seed=70000 + b, dtype=DTYPE[sfx])
    return CB.rhs(n, nrhs, sfx, b)


@functools.lru_cache(maxsize=None)
def general_batch(n, sfx, batch):
    out = np.stack([general_matrix(n, sfx, b) for b in range(batch)])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def general_rhs_batch(n, nrhs, sfx, batch):
    out = np.stack([general_rhs(n, nrhs, sfx, b) for b in range(batch)])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def cpu_factors(n, sfx, b):
    """(F, ipiv) of the CPU comparator of the batched factorization on matrix b, partial pivoting, no diagonal shift: the CPU oracle
    (real) / complex_ref.complex_generic_lufact (complex).  The GPU test takes rflu_getrf_batched_*'s own factors instead."""
    if KIND[sfx] == "real":
        F, ipiv = IC.cpu_factors(general_matrix(n, sfx, b))
    else:
        F, ipiv, info = CB.ref_factors(n, n, sfx, b)
        assert info == 0
    return np.asarray(F), np.asarray(ipiv, dtype=np.int64)


def perms_of(ipiv, n):
    """(batch, n): perm of every member, (P x)[i] = x[perm[i]]; ipiv None: the identity"""
    return np.stack([CR.perm_of(ip, n) for ip in ipiv])


LD = {"real": np.longdouble, "complex": np.clongdouble}


def omega_batch(F, perm, B, X, op):
    """Componentwise backward error of every member of a batch, (batch,) float64:
        'N':  max |P b - L (U x)| / (|L| (|U| |x|) + |P b|)        'T': max |b - U^T (L^T z)| / (|U^T| (|L^T| |z|) + |b|),  z = P x
    ('C': the factors conjugated), every | | a modulus, in numpy.longdouble / clongdouble on the ROUNDED factors F (batch, n, n);
    perm (batch, n); B, X (batch, n, nrhs).  A non-finite X gives inf."""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "numpy.longdouble is no wider than Float64 here: the reference needs an extended type"
    F = np.asarray(F)
    batch, n = F.shape[0], F.shape[1]
    ld = LD["complex" if np.iscomplexobj(F) else "real"]
    Fl = F.astype(ld)
    L = np.tril(Fl, -1) + np.eye(n, dtype=ld)
    U = np.triu(Fl)
    if op == "C":
        L, U = L.conj(), U.conj()
    b, x = np.asarray(B).astype(ld).reshape(batch, n, -1), np.asarray(X).astype(ld).reshape(batch, n, -1)
    rows = np.arange(batch)[:, None]
    with np.errstate(all="ignore"):
        if op == "N":
            pb = b[rows, perm]
            num = np.abs(pb - L @ (U @ x))
            den = np.abs(L) @ (np.abs(U) @ np.abs(x)) + np.abs(pb)
        else:
            Lt, Ut = np.swapaxes(L, 1, 2), np.swapaxes(U, 1, 2)
            z = x[rows, perm]
            num = np.abs(b - Ut @ (Lt @ z))
            den = np.abs(Ut) @ (np.abs(Lt) @ np.abs(z)) + np.abs(b)
        w = (num / den).reshape(batch, -1).max(axis=1).astype(np.float64)
    fin = np.isfinite(x).reshape(batch, -1).all(axis=1)
    assert (den[fin] > 0).all()
    return np.where(fin & np.isfinite(w), w, np.inf)


def lapack_solve(F, ipiv, B, op):
    """scipy.linalg.lu_solve (xGETRS) on the same factors, interchanges (1-based, None = none) and right-hand sides, in their type"""
    import scipy.linalg as sla

    n = F.shape[0]
    piv = (np.arange(n) if ipiv is None else np.asarray(ipiv) - 1).astype(np.int32)
    X = sla.lu_solve((np.asfortranarray(F), piv), np.asfortranarray(B), trans=TRANS_CODE[op], check_finite=False)
    assert X.dtype == F.dtype
    return X


def complex_c(sfx, n):
    """The derived bound: omega <= n eps (real: gamma_n per triangle, tests/test_gpu_solve_exact.py) and 4 n eps (complex:
    complex_solve_cases.complex_c has the derivation)"""
    return (1.0 if KIND[sfx] == "real" else 4.0) * n


# ---- both kernels' solve, restated ---------------------------------------------------------------------------------------------------------
MUTATIONS = (
    "backward_skips_last_column",   # the backward sweep starts at column n - 2
    "no_final_division",            # the rows are never divided by (multiplied with the reciprocal of) their diagonal entry
    "inverse_perm",                 # the inverse of sperm
    "gather_for_scatter",           # T / C: the solution is gathered through sperm where the kernel scatters
    "ignore_p1",                    # what the composition writes to the p1 half (rows from 64) is lost
    "ignore_j0",                    # the load of the second and later passes forgets j0: column 8 reads column 0
    "neighbour_ipiv",               # member b composes the ipiv of member b + 1 (the last one: b - 1)
    "strideB_for_strideF",          # member b's factors are looked for at b * strideB
    "t_for_c",                      # complex: 'C' runs the unconjugated substitution AND reciprocal, i.e. all of 'T'
    "c_for_t",                      # complex: 'T' conjugates
    "recip_unconjugated",           # complex 'C': the reciprocal diagonal is left unconjugated, the triangle is conjugated
    "rm_load_as_cm",                # the row-major right-hand-side load addresses B as column-major
)


def cbsubstitute(F, x, mode, D, mutation=None):
    """cbsubstitute<R, MODE> of csrc/batched_complex.hip on the columns of x, in place, by parts as cmul / csub of csrc/complex_dev.hpp
    have them (products and sums rounded separately where the compiler may fuse them).  mode 0: the image by columns, L (unit)
    forward and U backward; 1: by rows; 2: by rows, conjugated as it is read.  D[k]: the reciprocal of op(F)(k, k); x_k is scaled by
    it for every reader while the non-unit triangle runs, the stored x_k staying unscaled, then every row is scaled."""
    n = F.shape[0]
    T = F if mode == 0 else (F.T if mode == 1 else F.T.conj())
    unit_lower = mode == 0
    top = n - 2 if mutation == "backward_skips_last_column" else n - 1

    def take(rows, k, scaled):
        xk = _cmul(x[k:k + 1], D[k]) if scaled else x[k:k + 1]
        p = _cmul(T[rows, k:k + 1], xk)
        x[rows] = x[rows] - p                                  # csub: part by part, which is what complex subtraction is

    with np.errstate(all="ignore"):
        for k in range(n):
            take(slice(k + 1, n), k, not unit_lower)
        if not unit_lower and mutation != "no_final_division":
            x[...] = _cmul(x, D[:, None])
        for k in range(top, -1, -1):
            take(slice(0, k), k, unit_lower)
        if unit_lower and mutation != "no_final_division":
            x[...] = _cmul(x, D[:, None])


def restatement(F, lda, strideF, ipiv, stride_ipiv, B, ldb, strideB, batch, n, nrhs, row_major, op, mutation=None):
    """The memory image rflu_getrs_batched_*_dev leaves in B.  F, B: FLAT arrays in the element type holding the caller's buffers
    (element (i, j) of member b's factors at b * strideF + i + j * lda, row-major: + i * lda + j; B likewise with ldb / strideB);
    ipiv: flat int64 (member b at b * stride_ipiv) or None.  Returns the new flat B; elements the kernel does not store keep their value.
    Column-major, in the kernel's words: `x[r + j * ld] = B[src + (j0 + j) * ldb]`; row-major: `x[i + rr * ld] = B[src * ldb + j0 + rr]`
    with rr = t & 7 the column of the pass."""
    F, out = np.asarray(F), np.array(B, copy=True)
    dtype = F.dtype
    real = not np.iscomplexobj(F)
    assert out.dtype == dtype and (op in OPS["real" if real else "complex"])
    trans = op != "N"
    if not real:
        if mutation == "t_for_c" and op == "C":
            op = "T"
        elif mutation == "c_for_t" and op == "T":
            op = "C"
    rows = np.arange(n)
    for b in range(batch):
        offF = b * (strideB if mutation == "strideB_for_strideF" else strideF)
        offB = b * strideB
        idx = offF + ((rows[:, None] * lda + rows[None, :]) if row_major else (rows[:, None] + rows[None, :] * lda))
        S = F[idx % F.size]                                        # (the mutation may point outside: wrapped, whatever is there)
        if ipiv is None:
            ip = None
        else:
            bi = b if mutation != "neighbour_ipiv" else (b + 1 if b + 1 < batch else max(b - 1, 0))
            ip = ipiv[bi * stride_ipiv: bi * stride_ipiv + n]
        sperm = IC.compose_interchanges(ip, n, ignore_p1=mutation == "ignore_p1")
        if mutation == "inverse_perm":
            inv = np.empty(n, dtype=np.int64)
            inv[sperm] = rows
            sperm = inv
        if not real:
            d = np.diagonal(S)
            D = CBI.reciprocal(d.conj() if (op == "C" and mutation != "recip_unconjugated") else d)
        for j0 in range(0, nrhs, BNR):
            nr = min(BNR, nrhs - j0)
            cols = np.arange(nr)
            src = rows if trans else sperm
            jl = 0 if (mutation == "ignore_j0" and j0 > 0) else j0
            if not row_major or mutation == "rm_load_as_cm":
                at = offB + src[:, None] + (jl + cols[None, :]) * ldb
            else:
                at = offB + src[:, None] * ldb + jl + cols[None, :]
            x = out[at % out.size].copy()
            if real:
                IC.bsubstitute(S, x, trans=trans, mutation=mutation)
            else:
                cbsubstitute(S, x, TRANS_CODE[op], D, mutation=mutation)
            dst = sperm if trans else rows
            if trans and mutation == "gather_for_scatter":
                x, dst = x[sperm], rows
            if not row_major:
                out[offB + dst[:, None] + (j0 + cols[None, :]) * ldb] = x
            else:
                out[offB + dst[:, None] * ldb + j0 + cols[None, :]] = x
    return out


def pack(M, row_major):
    """(batch, r, c) matrices -> the flat packed buffer of either orientation (ld = the contiguous dimension, stride = r * c)"""
    M = np.asarray(M)
    return np.ascontiguousarray(M if row_major else np.transpose(M, (0, 2, 1))).reshape(-1)


def unpack(flat, batch, r, c, row_major):
    flat = np.asarray(flat)
    return flat.reshape(batch, r, c) if row_major else np.transpose(flat.reshape(batch, c, r), (0, 2, 1))


def solve_packed(F, ipiv, B, op, row_major=False, mutation=None):
    """restatement on packed buffers: F (batch, n, n), ipiv (batch, n) or None, B (batch, n, nrhs) -> X (batch, n, nrhs)"""
    F, B = np.asarray(F), np.asarray(B)
    batch, n, nrhs = B.shape
    ip = None if ipiv is None else np.ascontiguousarray(ipiv, dtype=np.int64).reshape(-1)
    out = restatement(pack(F, row_major), n, n * n, ip, n, pack(B, row_major), nrhs if row_major else n, n * nrhs, batch, n, nrhs,
                      row_major, op, mutation)
    return unpack(out, batch, n, nrhs, row_major)


# ---- a batch of constructed members between general ones -------------------------------------------------------------------------------------
def exact_positions(batch):
    """Where the constructed members sit: five spread over the 67, every other member of a small batch"""
    if batch == 67:
        return [5 + 13 * k for k in range(5)]
    return list(range(0, batch, 2))


def mixed_batch(n, sfx, batch, factors, given=True, which="random"):
    """(F, ipiv, B, exact): F (batch, n, n) and ipiv (batch, n) in the element type, B: op -> (batch, n, NRHS_MAX), exact: position ->
    Member.  `factors(b)` -> (F, ipiv) of general matrix b (the CPU comparator's, or the GPU's own); the general members' right-hand
    sides are general_rhs for every operator.  given=False is the ipiv = NULL call: the constructed members have the identity for
    interchanges, the general ones keep their L and U (a solve with L U itself) and ipiv comes back None."""
    kind, dtype = KIND[sfx], DTYPE[sfx]
    F = np.empty((batch, n, n), dtype=dtype)
    ipiv = np.empty((batch, n), dtype=np.int64)
    rhs = general_rhs_batch(n, NRHS_MAX, sfx, batch)
    B = {op: np.array(rhs) for op in OPS[kind]}
    exact = {}
    pos = exact_positions(batch)
    for b in range(batch):
        if b in pos:
            if kind == "real" and n > LIMIT[sfx]:              # the loop over the single-matrix path: see above_member
                assert n == ABOVE[sfx] and given and which == "random"
                c = above_member(sfx, pos.index(b))
            else:
                c = member(n, kind, pos.index(b), which if given else "identity")
            F[b], ipiv[b] = c.F.astype(dtype), c.ipiv
            for op in OPS[kind]:
                B[op][b] = c.B[op].astype(dtype)
            exact[b] = c
        else:
            F[b], ipiv[b] = factors(b)
    if not given:
        ipiv = None
    return F, ipiv, B, exact
