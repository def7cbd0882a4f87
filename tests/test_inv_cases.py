"""What tests/test_gpu_inv_exact.py and tests/test_gpu_inv.py rely on, proven on the CPU (tests/inv_cases.py):

  * the constructed real factors are what their docstring says, their inverse is certified in integer arithmetic (exact_case does that
    when it builds a case), and every entry and every partial sum of ANY blocked inverse is exactly representable in Float32 -- so
    comparing whole buffers with `==` is a fair demand of the GPU, whatever its blocking and summation order;
  * the transcription of getri_view<E> (csrc/inverse.hip) and the restatement of getri_batched_kernel (csrc/batched.hip) return that
    inverse by `==` in both precisions, and each mutation of them is caught at every size where it can differ -- and is shown NOT to
    differ below, so the size lists are seen to cover the switch;
  * on the random inputs of tests/test_gpu_inv.py the two restatements alone stay at or below half the GPU residual bar: the bar
    hides no failure of the algorithm and leaves a kernel room for nothing but its own mistakes.  The worst ratios are printed."""
import math

import numpy as np
import pytest

import inv_cases as C

ALL_EXACT = sorted(set(C.EXACT_SIZES + C.BATCHED_EXACT_SIZES))


def test_constants_are_the_sources():
    h = C.header_constants()
    assert (h["NB"], h["GETRI_W"], h["BNR"], h["BATCHED_MAX_DIM"]) == (C.NB, C.GETRI_W, C.BNR, C.BATCHED_MAX_DIM)


def test_sizes_cover_the_switches():
    """Both sides of BNR, NB, BATCHED_MAX_DIM and GETRI_W as csrc/rflu_internal.hpp and csrc/batched_kernels.hpp state them, a size with
    three block columns, a last block column of one row and one of NB + 1 rows."""
    h = C.header_constants()
    nb, w, bnr, lim = h["NB"], h["GETRI_W"], h["BNR"], h["BATCHED_MAX_DIM"]
    b, e, s = set(C.BATCHED_EXACT_SIZES), set(C.EXACT_SIZES), set(C.SIZES)
    assert {bnr - 1, bnr} <= b and {nb, nb + 1} <= b and max(b) == lim          # 7 | 8, the p0 | p1 halves and tpm, the limit
    assert {1, 2, 3} <= b                                                       # the smallest sizes at which each mutation can show
    assert min(e) == nb + 1 and 2 * nb + 2 in e                                 # one and two 64-row boundaries, W < 512
    assert w + 1 in e and w + nb + 1 in e                                       # a last block column of 1 row and of NB + 1 rows
    assert any(n > 2 * w for n in e) and max(e) <= 2112                         # three block columns
    assert all(n > lim or n in b for n in e if n <= lim)
    assert {nb - 1, nb, nb + 1, 2 * nb - 1, 2 * nb, 2 * nb + 1, w - 1, w, w + 1, 2 * w + 1} <= s
    assert {lim} <= {n for n, _ in C.BATCH_CASES} and all(n <= lim for n, _ in C.BATCH_CASES)
    assert set(C.VARIANT_SIZES) <= s
    for groups in (4, 2):
        assert C.EXACT_BATCH % groups                                           # the last workgroup is partly empty


@pytest.mark.parametrize("n", ALL_EXACT)
def test_the_factors_are_as_constructed(n):
    copies = range(C.EXACT_COPIES) if n in C.BATCHED_EXACT_SIZES else (0,)
    for k in copies:
        c = C.exact_case(n, k)
        L, U = np.tril(c.F, -1) + np.eye(n), np.triu(c.F)
        assert np.array_equal(L, c.L) and np.array_equal(U, c.U)
        assert np.isin(np.diagonal(U), C.DIAG).all()
        off = np.concatenate([L[np.tril_indices(n, -1)], U[np.triu_indices(n, 1)]])
        assert np.isin(off, [0.0, 1.0, -1.0]).all()
        if n >= 65:
            far = (np.count_nonzero(np.tril(L, -2)), np.count_nonzero(np.triu(U, 2)))
            assert 4 <= far[0] <= 24 and 4 <= far[1] <= 24, far
            assert np.count_nonzero(np.diagonal(L, -1)) >= n // 2 and np.count_nonzero(np.diagonal(U, 1)) >= n // 2
        for b in range(C.NB, n, C.NB):                                          # a chain crosses every 64-row boundary
            assert L[b, b - 1] != 0 and U[b - 1, b] != 0, b
        p = C.perm_of(c.ipiv, n)                                                # ipiv moves every row
        assert (c.ipiv[:-1] > np.arange(1, n)).all() and (n == 1 or (p != np.arange(n)).all())
        # P A = L U, X is the inverse and Y the one without interchanges (float64 evaluates these small dyadic numbers exactly)
        assert np.array_equal(c.A[p, :], L @ U)
        assert np.array_equal(c.A @ c.X, np.eye(n)) and np.array_equal(c.X @ c.A, np.eye(n))
        assert np.array_equal(c.X[:, p], c.Y)
        assert np.array_equal((L @ U) @ c.Y, np.eye(n))
        # det A = sign * 2^k
        s, la = np.linalg.slogdet(c.A)
        assert s == c.sign and abs(la - c.log2_absdet * math.log(2.0)) <= 1e-9
        # a transposed store, a forgotten permutation or a dropped block must be visible
        if n >= 2:
            assert not np.array_equal(c.X, c.X.T) and not np.array_equal(c.X, c.Y)
        if n >= 130:
            full = n // C.NB                                                    # every full 64 x 64 off-diagonal block
            for i in range(full):
                for j in range(full):
                    if i != j:
                        assert c.X[i * C.NB:(i + 1) * C.NB, j * C.NB:(j + 1) * C.NB].any(), (n, i, j)
            if n % C.NB:                                                        # and the partial last block row and block column
                assert c.X[full * C.NB:, :full * C.NB].any() and c.X[:full * C.NB, full * C.NB:].any()


@pytest.mark.parametrize("n", ALL_EXACT)
def test_every_partial_sum_fits_float32(n):
    copies = range(C.EXACT_COPIES) if n in C.BATCHED_EXACT_SIZES else (0,)
    for k in copies:
        c = C.exact_case(n, k)
        magnitude_bits, granularity_bits = C.partial_sum_bits(c)
        print(f"n={n} copy {k}: any partial sum is a multiple of 2^-{granularity_bits} below 2^{magnitude_bits}: "
              f"{magnitude_bits + granularity_bits} significant bits of Float32's 24")
        assert magnitude_bits + granularity_bits <= 24
        for M in (c.F, c.X, c.Y, c.A):                                          # inputs and outputs survive the rounding to Float32
            assert np.array_equal(M.astype(np.float32).astype(np.float64), M)


# ---- the single-matrix path: the transcription and its mutations ---------------------------------------------------------------------
@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("n", C.EXACT_SIZES)
def test_the_transcription_returns_the_exact_inverse(n, dtype):
    c = C.exact_case(n)
    X = C.getri_transcription(c.F.astype(dtype), c.ipiv)
    assert X.dtype == dtype and np.array_equal(X, c.X)
    Y = C.getri_transcription(c.F.astype(dtype), None)                          # NotIPIV: U^-1 L^-1
    assert Y.dtype == dtype and np.array_equal(Y, c.Y)


@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("n", [1, 2, 3, 7, 64] + C.EXACT_SIZES)
def test_mutations_of_the_transcription_are_caught(n, dtype):
    """recurse=False (the width-64 sweep inside a wide diagonal block skipped): differs from n = 65 on and cannot differ up to 64, where
    there is one 64-row block; reverse=False (the interchanges applied forwards): differs from n = 3 on -- at n = 2 there is one
    interchange, and one is its own reverse."""
    c = C.exact_case(n)
    F = c.F.astype(dtype)
    assert np.array_equal(C.getri_transcription(F, c.ipiv), c.X)
    assert np.array_equal(C.getri_transcription(F, c.ipiv, recurse=False), c.X) == (n <= C.NB)
    assert np.array_equal(C.getri_transcription(F, c.ipiv, reverse=False), c.X) == (n <= 2)


# ---- the batched kernel: the restatement and its mutations ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("n", C.BATCHED_EXACT_SIZES)
def test_the_batched_restatement_returns_the_exact_inverse(n, dtype):
    for k in range(C.EXACT_COPIES):
        c = C.exact_case(n, k)
        F = c.F.astype(dtype)
        want = c.X.astype(dtype)
        cm, rm = C.batched_restatement(F, c.ipiv, row_major=False), C.batched_restatement(F, c.ipiv, row_major=True)
        assert cm.dtype == rm.dtype == dtype
        assert np.array_equal(rm, want) and np.array_equal(cm, want.T)          # the memory images of the two orientations
        assert np.array_equal(C.batched_restatement(F, None, row_major=True), c.Y)   # NotIPIV
        assert np.array_equal(C.batched_restatement(F, c.ipiv, row_major=True, passes=False), rm)


@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("n", C.BATCHED_EXACT_SIZES)
def test_mutations_of_the_batched_restatement_are_caught(n, dtype):
    """The inverse permutation in place of sperm: the composed interchanges are one cycle through all n rows (every ipiv[k] > k + 1), its
    own inverse only for n <= 2.  The store branches exchanged: the transposed matrix, another one from n = 2 on.  The p1 half of the
    composition ignored: differs as soon as a row >= 64 takes part, from n = 65 on, and cannot differ below."""
    for k in range(C.EXACT_COPIES):
        c = C.exact_case(n, k)
        F = c.F.astype(dtype)
        for row_major in (False, True):
            good = C.batched_restatement(F, c.ipiv, row_major=row_major)
            mutant = lambda **kw: C.batched_restatement(F, c.ipiv, row_major=row_major, **kw)   # noqa: E731
            assert np.array_equal(mutant(inverse_perm=True), good) == (n <= 2), (n, k)
            assert np.array_equal(mutant(swap_store=True), good) == (n <= 1), (n, k)
            assert np.array_equal(mutant(ignore_p1=True), good) == (n <= 64), (n, k)


def test_the_composition_skips_what_getrf_could_not_have_written():
    """p <= k or p >= n: skipped, as the kernel skips it."""
    assert C.compose_interchanges(np.array([3, 1, 9, 4]), 4).tolist() == [2, 1, 0, 3]
    assert C.compose_interchanges(None, 5).tolist() == [0, 1, 2, 3, 4]
    ip = C.exact_case(100).ipiv
    assert np.array_equal(C.compose_interchanges(ip, 100), C.perm_of(ip, 100))


# ---- how much room the restatements leave under the GPU bar ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", C.DTYPES)
def test_the_batched_restatement_stays_inside_half_the_bar(dtype):
    """Every matrix of every case of BATCH_CASES (the batches of 1 and 257 at n = 64 are the head and an extension of the 200); the
    larger of rho_R and rho_L, printed per size.  n <= 2 is evaluated in rational arithmetic (inv_cases.rho says why): at n = 1 the
    inverse is one correctly rounded reciprocal, whose ratio is at most 1/2 and reaches it.  Where this was written: Float64 0.46 / 0.33 /
    0.12 / 0.10 at n = 1 / 2 / 7 / 8 and at most 0.018 from n = 33 on; Float32 0.45 / 0.29 / 0.11 / 0.08 and at most 0.017."""
    table = []
    for n in sorted({n for n, _ in C.BATCH_CASES}):
        batch = max(b for m, b in C.BATCH_CASES if m == n)
        A = C.host_batch(n, batch, dtype)
        worst = 0.0
        for b in range(batch):
            F, ipiv = C.cpu_factors(A[b])
            X = C.batched_inverse(F, ipiv, passes=False)
            assert X.dtype == dtype
            worst = max(worst, *C.rho(A[b], X, dtype, exact=n <= 2))
        table.append((n, batch, worst))
        assert worst <= C.half_bar(n), (n, worst)
    print(f"{np.dtype(dtype).name}: worst rho of the batched restatement (half bar {C.half_bar(2)}): "
          + ", ".join(f"n={n} x {b}: {w:.4f}" for n, b, w in table))


@pytest.mark.parametrize("dtype", C.DTYPES)
def test_the_transcription_stays_inside_half_the_bar(dtype):
    """getri_transcription in the element type on the factors of the CPU oracle, every size of SIZES and the NoPivot inputs of
    VARIANT_SIZES (marked +).  Where this was written: at most 0.11 (n = 2) and 0.021 for n >= 63 in Float64, 0.071 and 0.014 in Float32."""
    table = []
    for n, diag in [(n, False) for n in C.SIZES] + [(n, True) for n in C.VARIANT_SIZES]:
        A = C.matrix(n, dtype, diag)
        if diag:
            F, _, info = C.O.lu(np.array(A, order="F"), pivot=False)
            assert info == 0
            ipiv = None
        else:
            F, ipiv = C.cpu_factors(A)
        X = C.getri_transcription(F, ipiv)
        assert X.dtype == dtype
        w = max(C.rho(A, X, dtype, exact=n <= 2))
        table.append((f"{n}{'+' if diag else ''}", w))
        assert w <= C.half_bar(n), (n, diag, w)
    print(f"{np.dtype(dtype).name}: worst rho of the transcription (half bar {C.half_bar(2)}): " + ", ".join(f"n={n}: {w:.4f}" for n, w in table))
