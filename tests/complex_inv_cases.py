"""Inputs and CPU references of the complex inv / det / logabsdet tests (tests/test_complex_inv_glue.py, tests/test_complex_inv_cases.py,
tests/test_gpu_complex_inv.py, scripts/complex_inv_cpu_bars.py).  Pure numpy, no GPU.

  * rand_matrix: re and im uniform in [-1/2, 1/2) from seeded generators, in the element type's own precision;
  * rho: LAPACK's xGET03 ratios ||A X - I||_1 / (n eps_T ||A||_1 ||X||_1) and the same with X A, evaluated in complex128;
  * exact_case: CONSTRUCTED factors (nothing is computed by an elimination) whose inverse is known exactly -- see its docstring;
  * kernel_order_logabsdet: the complex reduction of csrc/inverse.hip restated on the host, in its own order;
  * getri_transcription: the two sweeps of csrc/inverse.hip in numpy with the index arithmetic of the drivers."""
import functools
import math

import numpy as np

NB = 64                 # rflu_internal.hpp
GETRI_W = 512
LD_CHUNK, LD_THREADS = 1024, 256
SIZES = [1, 2, 3, 63, 64, 65, 127, 128, 129, 200, 511, 512, 513, 1025, 1100, 2112]   # every 64-row boundary, W-1, W, W+1, 2W+1
VARIANT_SIZES = [65, 200, 513]
EXACT_SIZES = [65, 130, 513]
CDTYPES = [np.complex128, np.complex64]
# seed of the n x n input: 95000 + n, except for seven sizes.  Those were chosen, before logdet_input below existed, to leave room under the
# absolute logabsdet bar 8 n eps_T of the GPU test in complex128: the next seed in steps of 3000 at which (a) numpy.linalg.slogdet is within
# 2.1 n eps64 of the exactly rounded sum (math.fsum) of the logs of LAPACK's own factors, (b) LAPACK's zgetrf and tests/complex_ref.py's
# unblocked elimination both stay within 4.1 n eps64 of it, and, where several qualify (n = 1100), (c) log det is least sensitive:
# sqrt(sum |inv(A)^T .* A|^2), the first-order response to entrywise relative perturbations, is 33 at seed 114100 against 91 at 99100.
# (a) turned out not to travel from one machine to the next (see logdet_input, which removes the need for it); (b) and (c) still say
# something about the matrix, and the residual tests and their CPU table (scripts/complex_inv_cpu_bars.py) were run on these inputs, so
# the seeds stay.
SEEDS = {127: 98127, 128: 101128, 512: 98512, 513: 104513, 1025: 111025, 1100: 114100, 2112: 115112}


def real_of(ctype):
    return np.float64 if np.dtype(ctype) == np.complex128 else np.float32


def csfx(ctype):
    return "cf64" if np.dtype(ctype) == np.complex128 else "cf32"


@functools.lru_cache(maxsize=None)
def _rand_matrix(n, ctype, diag):
    rng_re, rng_im = np.random.default_rng(SEEDS.get(n, 95000 + n)), np.random.default_rng(96000 + SEEDS.get(n, 95000 + n))
    real = real_of(ctype)
    A = (rng_re.random((n, n)) - 0.5).astype(real) + 1j * (rng_im.random((n, n)) - 0.5).astype(real)
    A = np.asfortranarray(A.astype(ctype))
    if diag:
        A += ctype(n) * np.eye(n, dtype=ctype)   # diagonally dominant: |a_ii| >= n - 1/sqrt(2) > the sum of the others' moduli
    A.setflags(write=False)
    return A


def rand_matrix(n, ctype, diag=False):
    return _rand_matrix(n, np.dtype(ctype).type, bool(diag))


def logdet_scale(n):
    """Column scales 2^-e_j, e_j = floor((j + 1) m) - floor(j m) with m = max(0, log2(n) / 2 - 2): on rand_matrix's inputs
    log2|det A| / n is log2(n) / 2 - 2.0 within 0.03 from n = 129 on (numpy.linalg.slogdet on the CPU), so the scaled matrix has
    log|det| near 0 and so has every leading part of the sum of log|u_jj|."""
    m = max(0.0, 0.5 * math.log2(n) - 2.0)
    j = np.arange(n + 1)
    return np.ldexp(1.0, -(np.floor(j[1:] * m) - np.floor(j[:-1] * m)).astype(np.int64))


def logdet_input(n, ctype):
    """The input of the GPU test that compares logabsdet with numpy.linalg.slogdet: rand_matrix(n, ctype) with column j multiplied by
    logdet_scale(n)[j].  Powers of two: every entry is scaled exactly in both precisions, the pivot search compares within a column, so
    the elimination chooses the same rows and produces the same L and the same U with its columns scaled exactly -- the factorization
    under test is the same, only log|u_jj| moves by an exact multiple of log 2.  Why: the test's bar is ABSOLUTE, 8 n eps_T.  Unscaled,
    log|det A| is 5135 at n = 2112 and the bar four ulps of it, while numpy.linalg.slogdet adds its 2112 logs one after the other, each
    addition rounding at the ulp of a partial sum in the thousands: against the exact sum (math.fsum) over LAPACK's own diagonal it was
    found 0.0 n eps64 off on one machine and 21.3 on another ON THE SAME MATRIX (the last bits of the diagonal depend on the LAPACK
    build and its threads), up to 31 over 48 seeds.  The reference cannot carry that bar there, on any seed.  Scaled, no partial sum
    exceeds 381 at n = 2112 (193 at 1100; |u_jj| drifts along the diagonal, the scale does not follow that), its ulp is 5.7e-14 at
    most, and 2112 roundings of at most half of that each add up to about 0.29 sqrt(2112) 4e-14 = 5e-13, one n eps64, against the bar's
    eight wherever the test runs (measured where this was written: 1.4 n eps64 at n = 2112, less at every other size).  What the comparison still sees in full is what the factors contribute: a relative error
    in u_jj moves its log by the same absolute amount whatever the scale."""
    A = np.array(rand_matrix(n, ctype) * logdet_scale(n)[None, :].astype(real_of(ctype)), order="F")
    A.setflags(write=False)
    return A


def rho(A, X, ctype):
    """(rho_R, rho_L) in complex128; a non-finite X gives inf."""
    A, X = np.asarray(A, dtype=np.complex128), np.asarray(X, dtype=np.complex128)
    n = A.shape[0]
    if not np.isfinite(X).all():
        return math.inf, math.inf
    scale = n * float(np.finfo(real_of(ctype)).eps) * np.linalg.norm(A, 1) * np.linalg.norm(X, 1)
    eye = np.eye(n)
    return float(np.linalg.norm(A @ X - eye, 1) / scale), float(np.linalg.norm(X @ A - eye, 1) / scale)


def rho_bar(n):
    """n >= 4: the bar tests/test_gpu_inv.py holds the real types to; n <= 3: one complex reciprocal and one complex product are about
    eight unit roundoffs = 4 eps (LAPACK itself reaches 1.00 at n = 1)."""
    return 1.0 if n >= 4 else 4.0


def perm_of(ipiv, n):
    p = np.arange(n)
    for i, t in enumerate(np.asarray(ipiv)):
        j = int(t) - 1
        if j != i:
            p[i], p[j] = p[j], p[i]
    return p


# ---- constructed factors with an exactly known inverse ---------------------------------------------------------------------------
UNITS = np.array([1, -1, 1j, -1j])
DIAG = np.array([1, -1, 1j, -1j, 2, -2, 2j, -2j, 0.5, -0.5])
SCALE_BITS = 24        # the exact inverse is held as Gaussian integers times 2^-SCALE_BITS


class ExactCase:
    """n; F: packed L\\U (complex128, Fortran order); ipiv (1-based int64); A = P^T L U; X = A^-1, every entry a Gaussian dyadic rational,
    certified in integer arithmetic; log2_absdet, phase: det A = 2^log2_absdet * phase with phase in {1, i, -1, -i};
    bound / gran: see partial_sum_bits."""


def _gauss_int(Z, bits):
    """(re, im) int64 arrays of Z * 2^bits, which must be integral."""
    S = np.asarray(Z, dtype=np.complex128) * float(2 ** bits)
    re, im = np.rint(S.real), np.rint(S.imag)
    assert np.array_equal(re, S.real) and np.array_equal(im, S.imag), "not a dyadic rational at this scale"
    assert max(np.abs(re).max(initial=0), np.abs(im).max(initial=0)) < 2.0 ** 40
    return re.astype(np.int64), im.astype(np.int64)


def _gauss_matmul(a, b):
    (ar, ai), (br, bi) = a, b
    return ar @ br - ai @ bi, ar @ bi + ai @ br      # int64: exact (the callers bound the magnitudes)


@functools.lru_cache(maxsize=None)
def exact_case(n):
    """L unit lower and U upper, each bidiagonal plus a few far entries, off-diagonal entries in {0, +-1, +-i}, U's diagonal in
    {+-1, +-i, +-2, +-2i, +-1/2}; ipiv moves every row (ipiv[k] > k + 1 for k < n - 1; the last row is moved by the earlier ones).  The
    bidiagonals are cut after every third entry so that the chains of the inverses stay short (three long, six where a cut would fall on
    a multiple of 64 and is left out, so that a chain straddles EVERY 64-row boundary) and every magnitude small; the far entries reach
    across the 64-row blocks and, at n = 513, across the block column of width 512.

    The inverse: Y = U^-1 L^-1 is first formed in complex128, then CERTIFIED in integer arithmetic -- with every number a Gaussian integer
    times a power of two, (2 L U) (2^24 Y) == 2^25 I holds exactly in int64 -- and a nonsingular matrix has one inverse.
    A^-1 = Y P, i.e. column p[i] of X is column i of Y."""
    rng = np.random.default_rng(97000 + n)
    L = np.eye(n, dtype=np.complex128)
    U = np.zeros((n, n), dtype=np.complex128)
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
    M = L @ U                                              # exact: small Gaussian half-integers, short sums
    Y = np.linalg.solve(U, np.linalg.solve(L, np.eye(n)))
    Yi = _gauss_int(Y, SCALE_BITS)
    Pr, Pi = _gauss_matmul(_gauss_int(M, 1), Yi)
    assert np.array_equal(Pr, (2 ** (SCALE_BITS + 1)) * np.eye(n, dtype=np.int64)) and not Pi.any(), "the inverse is not exact"
    p = perm_of(ipiv, n)
    A = np.zeros((n, n), dtype=np.complex128)
    A[p, :] = M                                            # P A = L U
    X = np.zeros((n, n), dtype=np.complex128)
    X[:, p] = Y
    c = ExactCase()
    c.n, c.ipiv, c.A, c.X = n, ipiv, np.asfortranarray(A), np.asfortranarray(X)
    c.F = np.asfortranarray(np.tril(L, -1) + U)
    d = np.diagonal(U)
    c.log2_absdet = int(np.sum(np.abs(d) == 2)) - int(np.sum(np.abs(d) == 0.5))
    quarter = int(np.sum(np.rint(np.angle(d) / (math.pi / 2)).astype(np.int64))) + 2 * (n - 1)   # n - 1 interchanges, each a factor -1
    c.phase = [1, 1j, -1, -1j][quarter % 4]
    c.L, c.U = L, U
    for a in (c.A, c.X, c.F, c.ipiv):
        a.setflags(write=False)
    return c


def _gran_bits(Z):
    """Smallest e >= 0 with Z * 2^e a Gaussian integer."""
    for e in range(0, 60):
        S = np.asarray(Z, dtype=np.complex128) * float(2 ** e)
        if np.array_equal(np.rint(S.real), S.real) and np.array_equal(np.rint(S.imag), S.imag):
            return e
    raise AssertionError("not dyadic")


def partial_sum_bits(c):
    """An upper bound on the bits any partial sum of any blocked inverse needs, whatever its blocking and summation order.

    Write G = U^T, H = L^T.  Every number a blocked getri forms is a sum of (a subset of the terms of) an entry of one of
        G^-1,  G G^-1,  G^-1 G G^-1,  H^-1,  H H^-1,  H^-1 G^-1,  H (H^-1 G^-1),  H^-1 H H^-1 G^-1
    (a block of an inverse, a panel times an inverted block, an inverted block times that, a strip of Z, H times rows of Z already
    done, an inverted block of H times what remains), each term a product of real or imaginary parts.  With |M| = |re| + |im| taken
    entry by entry -- an upper bound on every real product that the complex product splits into -- any such subset sum is at most
        B = max entry of  |H^-1| (I + |H| |H^-1|) |G^-1| (I + |G| |G^-1|)
    in magnitude, and it is an integer multiple of the product of the factors' granularities 2^-g.  A multiple of 2^-g below 2^b has at
    most b + g significant bits.  Returns (ceil(log2 B), g)."""
    a = lambda M: np.abs(M.real) + np.abs(M.imag)
    n = c.n
    G, H = c.U.T, c.L.T
    Gi = np.linalg.solve(G, np.eye(n))
    Hi = np.linalg.solve(H, np.eye(n))
    eye = np.eye(n)
    B = a(Hi) @ (eye + a(H) @ a(Hi)) @ a(Gi) @ (eye + a(G) @ a(Gi))
    g = 2 * _gran_bits(Hi) + _gran_bits(H) + 2 * _gran_bits(Gi) + _gran_bits(G)
    return int(math.ceil(math.log2(2.0 * B.max()))), g     # the factor 2: the bound itself was formed in floating point


# ---- logabsdet in the kernel's own order -----------------------------------------------------------------------------------------
def _cmul(a, b):
    return complex(a.real * b.real - a.imag * b.imag, a.real * b.imag + a.imag * b.real)


def kernel_order_logabsdet(diag, ipiv):
    """(logabs, phase, sum of |log|) over a downloaded diagonal as ld_chunk / ld_combine / ld_finish of csrc/inverse.hip order
    it for complex elements: chunks of 1024, thread t of 256 takes entries t, t + 256, t + 512, t + 768 of its chunk in that order, the tree adds
    t and t + s for s = 128 .. 1, the chunks are combined in index order; Float64 throughout; parity and one renormalisation last."""
    d = np.asarray(diag, dtype=np.complex128)
    n = len(d)
    mod = np.hypot(d.real, d.imag)
    with np.errstate(divide="ignore", invalid="ignore"):
        logs = np.log(mod)
        unit = d / mod
    tot_s, tot_p, mass = None, None, 0.0
    for c0 in range(0, n, LD_CHUNK):
        s = np.zeros(LD_THREADS)
        p = [complex(1.0, 0.0)] * LD_THREADS
        for k in range(LD_CHUNK // LD_THREADS):
            for t in range(LD_THREADS):
                i = c0 + k * LD_THREADS + t
                if i < n:
                    s[t] += logs[i]
                    p[t] = _cmul(p[t], complex(unit[i]))
        w = LD_THREADS // 2
        while w:
            for t in range(w):
                s[t] += s[t + w]
                p[t] = _cmul(p[t], p[t + w])
            w //= 2
        tot_s = s[0] if tot_s is None else tot_s + s[0]
        tot_p = p[0] if tot_p is None else _cmul(tot_p, p[0])
    mass = float(np.sum(np.abs(logs)))
    swaps = 0 if ipiv is None else int(np.sum(np.asarray(ipiv)[:n] != np.arange(1, n + 1)))
    if swaps % 2:
        tot_p = -tot_p
    return float(tot_s), tot_p / abs(tot_p), mass


# ---- the two sweeps, transcribed ------------------------------------------------------------------------------------------------
def _blk64_mode0(C, M, B):
    """C_b -= tril(M_b) B_b for every 64-row block b; M_b the diagonal blocks of M."""
    m = C.shape[0]
    for r0 in range(0, m, NB):
        r1 = min(r0 + NB, m)
        C[r0:r1] -= np.tril(M[r0:r1, r0:r1]) @ B[r0:r1]


def _trmm_rect_rec(m, L, B, C):
    if m <= NB:
        return
    leaves = (m + NB - 1) // NB
    n1 = ((leaves + 1) // 2) * NB
    C[n1:m] -= L[n1:m, 0:n1] @ B[0:n1]
    _trmm_rect_rec(n1, L, B, C)
    _trmm_rect_rec(m - n1, L[n1:, n1:], B[n1:], C[n1:])


def _trtri_sweep(V, n, W, wide=GETRI_W, recurse=True):
    nblk = (n + W - 1) // W
    for jb in range(nblk - 1, -1, -1):
        j0 = jb * W
        w = min(W, n - j0)
        m = n - j0 - w
        Vjj = V[j0:j0 + w, j0:j0 + w]
        if recurse and W > NB and w > NB:
            _trtri_sweep(Vjj, w, NB)
        if m <= 0:
            continue
        D = -np.tril(Vjj)
        P = V[j0 + w:n, j0:j0 + w]
        Q = np.zeros((m, w), dtype=V.dtype)
        Q -= P @ D
        P[:] = 0
        G22 = V[j0 + w:n, j0 + w:n]
        _blk64_mode0(P, G22, Q)
        _trmm_rect_rec(m, G22, Q, P)


def getri_transcription(F, ipiv, W=GETRI_W, recurse=True, reverse=True, conj_h=False):
    """A^-1 from packed column-major factors F by the steps of getri_view<E> (csrc/inverse.hip).  The keyword arguments are the three mutations of
    the issue: recurse=False skips the width-64 sweep inside a wide diagonal block, reverse=False applies the interchanges forwards,
    conj_h=True conjugates H as it is saved."""
    n = F.shape[0]
    V = np.array(np.asarray(F).T, order="C")               # the transposed view: F's memory read row-major
    nb = (n + NB - 1) // NB
    W = min(W, nb * NB)
    Hinv = []
    for b in range(nb):
        r0, r1 = b * NB, min(b * NB + NB, n)
        blk = V[r0:r1, r0:r1]
        V[r0:r1, r0:r1] = np.triu(blk, 1) + np.tril(np.linalg.inv(np.tril(blk)))
        Hinv.append(np.linalg.inv(np.triu(blk, 1) + np.eye(r1 - r0)))
    _trtri_sweep(V, n, W, recurse=recurse)
    for ib in range((n + W - 1) // W - 1, -1, -1):
        i0 = ib * W
        w = min(W, n - i0)
        Hs = np.zeros((w, n), dtype=V.dtype)
        for r in range(w):
            Hs[r, i0 + r + 1:] = V[i0 + r, i0 + r + 1:]
            V[i0 + r, i0 + r + 1:] = 0
        if conj_h:
            Hs = Hs.conj()
        Zi = V[i0:i0 + w]
        if n - i0 - w > 0:
            Zi -= Hs[:, i0 + w:] @ V[i0 + w:]
        subs = (w + NB - 1) // NB
        for sb in range(subs - 1, -1, -1):
            s = sb * NB
            rows = min(NB, w - s)
            ks = s + NB
            if ks < w:
                Zi[s:s + rows] -= Hs[s:s + rows, i0 + ks:i0 + w] @ V[i0 + ks:i0 + w]
            Zi[s:s + rows] = (np.conj(Hinv[(i0 + s) // NB]) if conj_h else Hinv[(i0 + s) // NB]) @ Zi[s:s + rows]
    if ipiv is not None:
        order = range(n - 1, -1, -1) if reverse else range(n)
        for k in order:
            p = int(ipiv[k]) - 1
            if p != k:
                V[[k, p]] = V[[p, k]]
    return V.T
