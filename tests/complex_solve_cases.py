"""Inputs, references and CPU restatements for the tests that hold the complex solves -- ldiv!(F, B) ('N'), ldiv!(transpose(F), B) ('T')
and ldiv!(F', B) ('C') in ComplexF64 and ComplexF32 -- to exact and rounding-level references (tests/test_complex_solve_cases.py proves
them on the CPU, tests/test_gpu_complex_solve_exact.py uses them on the GPU).  Pure numpy / scipy, no GPU, no torch.

  * exact cases: complex_mixed_cases.exact_solve_case(n, 130), generated once per n, columns sliced.  `rhs` adds the right-hand sides of
    the transposed and the adjoint solve, formed like the forward one in int64 pairs on the half-integer grid; `row_sums` the two
    quantities that make a case independent of the order of summation (exact_solve_case's docstring has the argument: if the moduli of
    ALL terms of a row's substitution sum to less than 2^24 grid units, every partial sum in any order is a Float32 number).
  * general factors: LAPACK's cgetrf / zgetrf of complex_solve_ref.rand_input, and `omega`, the componentwise backward error
        'N':  max |P b - L (U x)| / (|L| (|U| |x|) + |P b|)        'T': max |b - U^T (L^T z)| / (|U^T| (|L^T| |z|) + |b|),  z = P x
    ('C': the factors conjugated), every | | a modulus, evaluated in numpy.clongdouble on the ROUNDED factors.
  * narrow_restatement / wide_restatement: the two device paths of csrc/complex_solve.hip and csrc/complex.hip in the element type with
    the kernels' own blocking and order of summation (products and sums are rounded separately here where the device fuses them: NumPy
    has no fused multiply-add).  `mutation` plants one of MUTATIONS; tests/test_complex_solve_cases.py shows which test notices it.
"""
import functools
import os
import re

import numpy as np

import complex_mixed_cases as CM
import complex_ref as CR
import complex_solve_ref as SR

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "recursivefactorization.jl_amd", "csrc")
CNB, CNARROW, CLEAF = 256, 8, 32      # asserted against header_constants() in tests/test_complex_solve_cases.py
CGEMV_WAVES, CG_BK = 4, 16
CTYPES = [np.complex128, np.complex64]
TRANS = ("N", "T", "C")
LD = np.clongdouble

# the 32-row steps and the partial last step of ctrsv_block_kernel; the CNB boundary; odd and even bands right of a block (the EPL = 2
# tail, both parities of the 16-byte test); 1 .. 4 leaves of the recursion with the uneven split at 97; partial K slabs of the GEMM;
# 1100: bands of 768 and 1024 elements, a second round of chunks per wave in both element types
GRID_N = [1, 2, 31, 32, 33, 64, 65, 97, 255, 256, 257, 513, 1100]
# the narrow / wide switch 8 | 9, the r / r + 4 pairing, the 32-wide transpose tile, the 64-wide GEMM tile with interior and edge tiles,
# the 128-thread workgroup of ctri_base_kernel
GRID_NRHS = [1, 2, 7, 8, 9, 31, 32, 33, 64, 65, 128, 129, 130]
NRHS_MAX = max(GRID_NRHS)
ROUNDING_N = [65, 129, 300, 700]
ROUNDING_NRHS = [1, 8, 9, 33, 64, 65, 130]
FLOAT32_LIMIT = float(2 ** 24)


def header_constants():
    """CNB, CNARROW, CLEAF (csrc/complex.hpp), CGEMV_WAVES (csrc/complex_solve.hip) and CG_BK (csrc/complex_gemm.hip) as the sources state
    them: a change of one of them fails tests/test_complex_solve_cases.py instead of moving a boundary away from GRID_N / GRID_NRHS."""
    hpp = open(os.path.join(CSRC, "complex.hpp")).read()
    solve = open(os.path.join(CSRC, "complex_solve.hip")).read()
    gemm = open(os.path.join(CSRC, "complex_gemm.hip")).read()
    return {
        "CNB": int(re.search(r"constexpr int CNB = (\d+);", hpp).group(1)),
        "CNARROW": int(re.search(r"constexpr int CNARROW = (\d+);", hpp).group(1)),
        "CLEAF": int(re.search(r"constexpr int CLEAF = (\d+);", hpp).group(1)),
        "CGEMV_WAVES": int(re.search(r"constexpr int CGEMV_WAVES = (\d+);", solve).group(1)),
        "CG_BK": int(re.search(r"CG_BK = (\d+)", gemm).group(1)),
    }


def eps_of(ctype):
    return SR.eps_of(ctype)


def path_of(nrhs, column_major_forward=False):
    """'narrow' (B's own columns) or 'wide' (row-major image, recursion, GEMM); rflu_getrs_cf*_dev always takes the wide one."""
    return "wide" if (column_major_forward or nrhs > CNARROW) else "narrow"


# ---- exact cases ---------------------------------------------------------------------------------------------------------------------------
def case(n):
    """exact_solve_case(n, NRHS_MAX): one generator, one case per n; narrower blocks are its first columns."""
    return CM.exact_solve_case(n, NRHS_MAX)


def perm_of(ipiv, n):
    """perm with (P X)[i] = X[perm[i]]: the interchanges applied first to last (the targets repeat, so the order matters)."""
    p = np.arange(n)
    for k in range(len(ipiv)):
        t = int(ipiv[k]) - 1
        if t != k:
            p[k], p[t] = p[t], p[k]
    return p


def _gi(a):
    return np.rint(a.real).astype(np.int64), np.rint(a.imag).astype(np.int64)


def _cmatmul(a, b):
    return a[0] @ b[0] - a[1] @ b[1], a[0] @ b[1] + a[1] @ b[0]


@functools.lru_cache(maxsize=None)
def _transposed(n, trans):
    """(2 B as int64 pairs, Y = L^T P X as int64 pairs, P X as int64 pairs) of the 'T' / 'C' solve of case(n)"""
    c = case(n)
    L, U2 = c.L, 2 * c.U
    if trans == "C":
        L, U2 = L.conj(), U2.conj()
    PX = _gi(c.X.astype(np.complex128)[perm_of(c.ipiv, n)])
    Y = _cmatmul(_gi(L.T), PX)                    # L^T (P X): integers
    B2 = _cmatmul(_gi(U2.T), Y)                   # 2 U^T Y = 2 B
    return B2, Y, PX


@functools.lru_cache(maxsize=None)
def rhs_pairs(n, trans):
    """2 B as (re, im) int64 arrays, B the right-hand sides with op(A) X = B exactly"""
    if trans == "N":
        c = case(n)
        B = c.B.astype(np.complex128) * 2         # (exact_solve_case asserts that this equals its own integer pairs)
        return _gi(B)
    return _transposed(n, trans)[0]


@functools.lru_cache(maxsize=None)
def _rhs(n, trans):
    B2 = rhs_pairs(n, trans)
    B = np.asfortranarray(((B2[0] + 1j * B2[1]) / 2).astype(np.complex64))
    assert np.array_equal(B.astype(np.complex128) * 2, B2[0] + 1j * B2[1])
    B.setflags(write=False)
    return B


def rhs(c, trans):
    """B (complex64, Fortran order, read-only) with op(A) X = B exactly: 'N' is the case's own B = P^T L U X, 'T' is U^T (L^T (P X)),
    'C' the same with both factors conjugated."""
    return _rhs(c.n, trans)


def row_sums(c, trans):
    """(first sweep, second sweep): max_i (|b_i| + sum_j |t_ij| |y_j|) over the rows of each substitution, j over the off-diagonal entries
    of its triangle (the terms that are summed), in grid units of 1/2.  'N': L then U.  'T' / 'C': the lower triangle of U^T (with its
    diagonal, which divides), then the strict upper one of L^T."""
    if trans == "N":
        return c.fwd_sum, c.bwd_sum
    B2, Y, PX = _transposed(c.n, trans)
    absU2 = np.abs(np.triu(2 * c.U, 1))
    absL = np.abs(np.tril(c.L, -1))
    modY, modPX = np.hypot(*Y), np.hypot(*PX)
    first = float((np.hypot(*B2) + absU2.T @ modY).max())               # 2 b_i and (2 u_ji) y_j
    second = float((2 * modY + 2 * (absL.T @ modPX)).max())             # 2 y_i and 2 l_ji z_j
    return first, second


@functools.lru_cache(maxsize=None)
def _factors_cm(n, ctype):
    c = case(n)
    F = np.asfortranarray(c.W.astype(ctype))
    assert np.array_equal(F.astype(np.complex128), c.W.astype(np.complex128))
    F.setflags(write=False)
    return F


def factors_cm(c, ctype):
    """the packed L\\U column-major (Fortran order) in `ctype`: complex64 as the case has it, complex128 exactly"""
    return _factors_cm(c.n, np.dtype(ctype).type)


def apply_p(c, X):
    return X[perm_of(c.ipiv, c.n)]


# ---- general factors and the componentwise backward error -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def general_factors(n, ctype):
    """LAPACK cgetrf / zgetrf of complex_solve_ref.rand_input(n, ctype): (packed factors in Fortran order, 0-based pivots, perm)"""
    import scipy.linalg as sla

    A = SR.rand_input(n, ctype)
    lu, piv = sla.lu_factor(A, check_finite=False)
    assert lu.dtype == np.dtype(ctype)
    lu = np.asfortranarray(lu)
    perm = perm_of(piv.astype(np.int64) + 1, n)
    for a in (lu, piv, perm):
        a.setflags(write=False)
    return lu, piv, perm


_TRIANGLES = {}   # (id of the factors, trans) -> (the factors, their triangles in clongdouble); a handful of entries


def _triangles_ld(lu, trans):
    key = (id(lu), trans)
    if key not in _TRIANGLES or _TRIANGLES[key][0] is not lu:
        if len(_TRIANGLES) >= 6:
            _TRIANGLES.clear()
        n = lu.shape[0]
        L = np.tril(lu, -1).astype(LD) + np.eye(n, dtype=LD)
        U = np.triu(lu).astype(LD)
        if trans == "C":
            L, U = L.conj(), U.conj()
        if trans != "N":
            L, U = np.ascontiguousarray(L.T), np.ascontiguousarray(U.T)
        _TRIANGLES[key] = (lu, (L, U, np.abs(L), np.abs(U)))
    return _TRIANGLES[key][1]


def omega(lu, perm, B, X, trans, per_column=False):
    """Componentwise backward error of X as a solution of op(P^T L U) X = B with the ROUNDED factors `lu`, in numpy.clongdouble, moduli
    throughout.  `per_column` returns the maximum over the rows of every column instead of one number."""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "numpy.longdouble is no wider than Float64 here: the reference needs an extended type"
    L, U, aL, aU = _triangles_ld(lu, trans)           # 'T' / 'C': already transposed (and conjugated)
    n = lu.shape[0]
    b, x = np.asarray(B).reshape(n, -1).astype(LD), np.asarray(X).reshape(n, -1).astype(LD)
    if trans == "N":
        pb = b[perm]
        num = np.abs(pb - L @ (U @ x))
        den = aL @ (aU @ np.abs(x)) + np.abs(pb)
    else:
        z = x[perm]
        num = np.abs(b - U @ (L @ z))                 # U^T (L^T z)
        den = aU @ (aL @ np.abs(z)) + np.abs(b)
    assert (den > 0).all()
    w = (num / den).max(axis=0)
    return w.astype(np.float64) if per_column else float(w.max())


# assertion (e) 3 of the GPU test: omega <= M_RATIO * max(omega_ref, eps / 8).  On the CPU the narrow restatement is at most 2.30 times
# LAPACK's omega and the wide one 3.40 times over the rounding cases (tests/test_complex_solve_cases.py recomputes both and this
# constant); four times that for the GPU's different summation order, rounded up to a power of two
M_RATIO = 16.0


def complex_c(n):
    """The constant of assertion (e) 2: omega <= c n eps with c = 4.  In the standard model a real operation has relative error
    <= u = eps / 2, and a complex product computed with four multiplications and two additions has relative error <= sqrt(2) gamma_2
    (Higham, Accuracy and Stability of Numerical Algorithms, Lemma 3.5), gamma_k = k u / (1 - k u); a complex addition has u.  A
    substitution with a triangle of n rows computed in any order therefore satisfies (T + dT) x = b with |dT| <= gamma'_n |T|, where every
    factor (1 + delta) of the real analysis (Theorem 8.5: gamma_n) is replaced by one with |delta| <= sqrt(2) gamma_2 ~ 2 sqrt(2) u; the
    division by the diagonal (Smith's formula) is within the same 2 sqrt(2) u to first order.  So gamma'_n <= 2 sqrt(2) n u to first
    order per triangle, and for the two triangles of L U (Theorem 9.4, |dL| |dU| second order) the componentwise backward error is
    bounded by 2 * 2 sqrt(2) n u = 2 sqrt(2) n eps = 2.83 n eps, rounded up to 4 n eps for the second-order terms.  The real file
    (tests/test_gpu_solve_exact.py) uses n eps where the same reasoning gives 2 n u = n eps."""
    return 4.0 * n


# ---- complex arithmetic in the element type, spelled out by parts like csrc/complex_dev.hpp --------------------------------------------------
def _join(re_, im_):
    out = np.empty(np.broadcast(re_, im_).shape, dtype=np.result_type(re_.dtype, np.complex64))
    out.real = re_
    out.imag = im_
    return out


def _cfma(v, x, acc):
    """cfma of complex_dev.hpp: fma(-v.im, x.im, fma(v.re, x.re, acc.re)), fma(v.im, x.re, fma(v.re, x.im, acc.im))"""
    return _join((acc.real + v.real * x.real) - v.imag * x.imag, (acc.imag + v.real * x.imag) + v.imag * x.real)


def _cmul(a, b):
    return _join(a.real * b.real - a.imag * b.imag, a.real * b.imag + a.imag * b.real)


def _cdiv(a, b):
    """a / b by Smith's formula as cdiv of complex_dev.hpp has it; b one element"""
    R = a.real.dtype.type
    br, bi = R(b.real), R(b.imag)
    with np.errstate(all="ignore"):
        if abs(br) >= abs(bi):
            if br == 0 and bi == 0:
                return _join(a.real / abs(br), a.imag / abs(bi))
            rat = bi / br
            scl = R(1) / (br + bi * rat)
            return _join((a.real + a.imag * rat) * scl, (a.imag - a.real * rat) * scl)
        rat = br / bi
        scl = R(1) / (br * rat + bi)
        return _join((a.real * rat + a.imag) * scl, (a.imag * rat - a.real) * scl)


# ---- the mutations ------------------------------------------------------------------------------------------------------------------------------
MUTATIONS = (
    "odd_tail",              # 1. cgemv_sub_kernel drops the last band element when the band length is odd and EPL = 2
    "skip_round2",           # 2. cgemv_sub_kernel skips the second round of chunks of every wave
    "no_conj_elementwise",   # 3. cgemv_sub_kernel does not conjugate in its element-by-element load branch
    "no_conj_out",           # 4. the wide path does not conjugate B on the way out
    "drop_r4",               # 5. phase 3 of ctrsv_block_kernel drops the r + 4 partner
    "wrong_split",           # 6. the two sub-solves of ctrsm_rec / ctriu_rec split at n / 2 rounded down to 32, the GEMM between them
                             #    at the right n1 (a wrong split used by all three alike is another correct solve: see the CPU test)
    "one_term",              # 7. a LOCAL fault: cgemv_sub_kernel drops one term, the last band element, from one row (row 5) of the band
)                            #    right of the first block (the second sweep); 1 .. 6 touch every row of a launch
ONE_TERM_ROW = 5


def split(n):
    return ((n + CLEAF - 1) // CLEAF + 1) // 2 * CLEAF


def wrong_split(n):
    return max(n // 2 // CLEAF * CLEAF, CLEAF)


# ---- the narrow path: csolve_narrow / csolve_fwd_narrow ---------------------------------------------------------------------------------------
def _gemv_sub(V, ld, i0, i1, k0, k1, X, conj, mutation):
    """cgemv_sub_kernel for the rows [i0, i1): X[i] -= sum over k in [k0, k1) of V[i, k] X[k].  Chunks of 64 * EPL elements dealt to four
    waves, lane l of a chunk the EPL elements from l * EPL on; a lane sums in ascending k, then the 64-lane tree (offsets 32 .. 1), then
    the four waves in order."""
    if i1 <= i0 or k1 <= k0:
        return
    ctype = X.dtype.type
    epl = 16 // np.dtype(ctype).itemsize
    chunk = 64 * epl
    band = k1 - k0
    rounds = -(-band // (CGEMV_WAVES * chunk))
    padded = rounds * CGEMV_WAVES * chunk
    rows = np.arange(i0, i1)
    Vb = np.zeros((i1 - i0, padded), dtype=ctype)             # (a zero element adds an exact zero: the padding changes nothing)
    Vb[:, :band] = V[i0:i1, k0:k1]
    if conj:
        plain = np.zeros(Vb.shape, dtype=bool)
        if mutation == "no_conj_elementwise":
            vec = ((rows * ld + k0) * np.dtype(ctype).itemsize) % 16 == 0          # (F itself on a 16-byte boundary)
            lane_start = np.arange(padded) // epl * epl
            plain = (~vec[:, None]) | ((band - lane_start) < epl)[None, :]
        Vb = np.where(plain, Vb, Vb.conj())
    if mutation == "odd_tail" and epl == 2 and band % 2 == 1:
        Vb[:, band - 1] = 0
    if mutation == "one_term" and i0 == 0 and k0 > 0:
        Vb[ONE_TERM_ROW, band - 1] = 0
    Xb = np.zeros((padded, X.shape[1]), dtype=ctype)
    Xb[:band] = X[k0:k1]
    Vb = Vb.reshape(i1 - i0, rounds, CGEMV_WAVES, 64, epl)
    Xb = Xb.reshape(rounds, CGEMV_WAVES, 64, epl, X.shape[1])
    acc = np.zeros((i1 - i0, CGEMV_WAVES, 64, X.shape[1]), dtype=ctype)
    for q in range(rounds):
        if mutation == "skip_round2" and q == 1:
            continue
        for e in range(epl):
            acc = _cfma(Vb[:, q, :, :, e, None], Xb[None, q, :, :, e, :], acc)
    off = 32
    while off > 0:                                            # lane 0 of the shuffle tree
        acc = _join(acc[:, :, :off].real + acc[:, :, off:2 * off].real, acc[:, :, :off].imag + acc[:, :, off:2 * off].imag)
        off >>= 1
    s = acc[:, 0, 0]
    for w in range(1, CGEMV_WAVES):
        s = _join(s.real + acc[:, w, 0].real, s.imag + acc[:, w, 0].imag)
    X[i0:i1] = _join(X[i0:i1].real - s.real, X[i0:i1].imag - s.imag)


def _trsv_block(T, Y, upper, unit, mutation):
    """ctrsv_block_kernel: Y <- T^-1 Y for one diagonal block (T: nb x nb, already conjugated where the kernel would) in 32-row steps:
    the step's triangle column by column, then the block's waiting rows take Y[i] -= sum_j T[i, j] x[j], j ascending from a zero sum."""
    nb, nrhs = Y.shape
    ctype = Y.dtype.type
    nsteps = (nb + 31) // 32
    for q in range(nsteps):
        s = 32 * (nsteps - 1 - q if upper else q)
        jn = min(32, nb - s)
        y = Y[s:s + jn].copy()
        Tp = T[s:s + jn, s:s + jn]
        for jj in range(jn):
            j = jn - 1 - jj if upper else jj
            if not unit:
                y[j] = _cdiv(y[j], Tp[j, j])
            sel = slice(0, j) if upper else slice(j + 1, jn)
            y[sel] = _cfma(-Tp[sel, j, None], y[None, j], y[sel])
        Y[s:s + jn] = y
        u0, u1 = (0, s) if upper else (s + 32, nb)
        if u1 > u0:
            acc = np.zeros((u1 - u0, nrhs), dtype=ctype)
            for j in range(jn):
                acc = _cfma(T[u0:u1, s + j, None], y[None, j], acc)
            if mutation == "drop_r4":
                acc[:, 4:] = 0
            Y[u0:u1] = _join(Y[u0:u1].real - acc.real, Y[u0:u1].imag - acc.imag)


def _swap_rows(X, ipiv, descending):
    if ipiv is None:
        return
    n = X.shape[0]
    for k in (range(n - 1, -1, -1) if descending else range(n)):
        p = int(ipiv[k]) - 1
        if p != k and 0 <= p < n:
            X[[k, p]] = X[[p, k]]


def narrow_restatement(F, ipiv, B, trans, mutation=None, ld=None):
    """csolve_fwd_narrow ('N': F read as the row-major packed factors, interchanges first and ascending, L unit lower, U upper) and
    csolve_narrow ('T' / 'C': V = F^T, the lower triangle with the diagonal, then the unit upper one, V conjugated as it is loaded for
    'C', interchanges last and descending).  Diagonal blocks of CNB rows; nrhs <= CNARROW.  `ld`: the leading dimension the 16-byte
    test of cgemv_sub_kernel sees (default n, F itself taken to be aligned)."""
    F = np.asarray(F)
    n = F.shape[0]
    X = np.array(B, dtype=F.dtype, copy=True).reshape(n, -1)
    assert X.shape[1] <= CNARROW + 1 and n <= 1100, "the restatement is for the narrow path's sizes"
    ld = n if ld is None else ld
    conj = trans == "C"
    V = F if trans == "N" else F.T
    lower_unit = trans == "N"
    if trans == "N":
        _swap_rows(X, ipiv, descending=False)

    def diag_block(j0, nb):
        T = V[j0:j0 + nb, j0:j0 + nb]
        return T.conj() if conj else T

    with np.errstate(all="ignore"):
        for j0 in range(0, n, CNB):
            nb = min(CNB, n - j0)
            _gemv_sub(V, ld, j0, j0 + nb, 0, j0, X, conj, mutation)
            _trsv_block(diag_block(j0, nb), X[j0:j0 + nb], False, lower_unit, mutation)
        for j0 in range((n - 1) // CNB * CNB, -1, -CNB):
            nb = min(CNB, n - j0)
            _gemv_sub(V, ld, j0, j0 + nb, j0 + nb, n, X, conj, mutation)
            _trsv_block(diag_block(j0, nb), X[j0:j0 + nb], True, not lower_unit, mutation)
    if trans != "N":
        _swap_rows(X, ipiv, descending=True)
    return X.reshape(np.shape(B))


# ---- the wide path: ctrsm_rec / ctriu_rec on a row-major image with the complex GEMM in between ------------------------------------------------
def _base(T, X, upper, unit):
    """ctri_base_kernel: one leaf-sized triangle, row by row, acc <- acc - t x in ascending t, then the division"""
    n = T.shape[0]
    for s in range(n):
        i = n - 1 - s if upper else s
        acc = X[i].copy()
        for t in (range(i + 1, n) if upper else range(i)):
            p = _cmul(T[i, t, None], X[t])
            acc = _join(acc.real - p.real, acc.imag - p.imag)
        if not unit:
            acc = _cdiv(acc, T[i, i])
        X[i] = acc


def _gemm_sub(A, Bm, C):
    """cgemm_sub_kernel: C <- C - A B, the accumulators start as C and take the products in ascending k, in K steps of 4 per part:
    Cr -= Ar Br (4 k), Cr += Ai Bi (4 k); Ci -= Ar Bi, Ci -= Ai Br"""
    K = A.shape[1]
    cr, ci = C.real.copy(), C.imag.copy()
    for k4 in range(0, K, 4):
        ks = range(k4, min(k4 + 4, K))
        for k in ks:
            cr = cr - A[:, k, None].real * Bm[None, k].real
        for k in ks:
            cr = cr + A[:, k, None].imag * Bm[None, k].imag
        for k in ks:
            ci = ci - A[:, k, None].real * Bm[None, k].imag
        for k in ks:
            ci = ci - A[:, k, None].imag * Bm[None, k].real
    C[...] = _join(cr, ci)


def _rec(T, X, upper, unit, sub_split, gemm_split):
    """ctrsm_rec (lower) / ctriu_rec (upper); `sub_split` is what the two sub-solves take for n1, `gemm_split` what the GEMM takes"""
    n = T.shape[0]
    if n <= CLEAF:
        _base(T, X, upper, unit)
        return
    ns, n1 = sub_split(n), gemm_split(n)
    if not upper:
        _rec(T[:ns, :ns], X[:ns], upper, unit, sub_split, gemm_split)
        _gemm_sub(T[n1:, :n1], X[:n1], X[n1:])
        _rec(T[ns:, ns:], X[ns:], upper, unit, sub_split, gemm_split)
    else:
        _rec(T[ns:, ns:], X[ns:], upper, unit, sub_split, gemm_split)
        _gemm_sub(T[:n1, n1:], X[n1:], X[:n1])
        _rec(T[:ns, :ns], X[:ns], upper, unit, sub_split, gemm_split)


def wide_restatement(F, ipiv, B, trans, mutation=None, consistent_wrong_split=False):
    """cgetrs_cm_dev / csolve_fwd_image ('N': interchanges first, ctrsm_rec with the unit lower triangle, ctriu_rec with the upper one)
    and csolve_wide ('T' / 'C': V = F^T unconjugated, B conjugated on the way in and out for 'C': A^H x = b <=> A^T conj(x) = conj(b);
    interchanges last and descending).  `consistent_wrong_split`: the sub-solves AND the GEMM split at wrong_split(n)."""
    F = np.asarray(F)
    n = F.shape[0]
    X = np.array(B, dtype=F.dtype, copy=True).reshape(n, -1)
    conj = trans == "C"
    V = F if trans == "N" else F.T
    sub = wrong_split if (mutation == "wrong_split" or consistent_wrong_split) else split
    gem = wrong_split if consistent_wrong_split else split
    with np.errstate(all="ignore"):
        if trans == "N":
            _swap_rows(X, ipiv, descending=False)
            _rec(V, X, False, True, sub, gem)
            _rec(V, X, True, False, sub, gem)
        else:
            if conj:
                X = X.conj()
            _rec(V, X, False, False, sub, gem)
            _rec(V, X, True, True, sub, gem)
            _swap_rows(X, ipiv, descending=True)
            if conj and mutation != "no_conj_out":
                X = X.conj()
    return X.reshape(np.shape(B))


def plain_substitution(F, ipiv, B, trans):
    """op(P^T L U) X = B by plain row-by-row substitution with NumPy's own complex arithmetic in the element type: 'N' here, 'T' / 'C'
    complex_solve_ref.trans_solve."""
    F = np.asarray(F)
    if trans != "N":
        return SR.trans_solve(F, ipiv, B, trans == "C")
    n = F.shape[0]
    X = np.array(B, dtype=F.dtype, copy=True).reshape(n, -1)
    _swap_rows(X, ipiv, descending=False)
    with np.errstate(all="ignore"):
        for i in range(1, n):
            X[i] = X[i] - F[i, :i] @ X[:i]
        for i in range(n - 1, -1, -1):
            X[i] = (X[i] - F[i, i + 1:] @ X[i + 1:]) / F[i, i]
    return X.reshape(np.shape(B))


def old_bar_ratio(n, ctype, X, B, trans):
    """the normwise backward error of X on complex_solve_ref.rand_input(n, ctype) in units of the old bar E = 20 n eps"""
    A = SR.rand_input(n, ctype).astype(np.complex128)
    M = A if trans == "N" else (A.conj().T if trans == "C" else A.T)
    X = np.asarray(X).astype(np.complex128).reshape(n, -1)
    Bw = np.asarray(B).astype(np.complex128).reshape(n, -1)
    with np.errstate(all="ignore"):
        be = np.linalg.norm(M @ X - Bw, np.inf) / (np.linalg.norm(M, np.inf) * np.linalg.norm(X, np.inf))
    return float(be / SR.bar_E(n, ctype))


def rand_rhs(n, nrhs, ctype):
    """complex_ref.rand_rhs; its counter runs down the columns, so rand_rhs(n, k) is the first k columns of rand_rhs(n, NRHS_MAX)"""
    return CR.rand_rhs(n, nrhs, ctype)
