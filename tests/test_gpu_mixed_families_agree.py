"""-m gpu: the real and the complex mixed-precision kernels agree with EACH OTHER, bit for bit (rflu_mixed_getrf_{f64,cf64}_dev and
rflu_residual_{f64,cf64}_dev; one kernel source, csrc/mixed.hip, whose demote and residual bodies stay two per family).

For a real matrix A the complex matrix A + 0i has the moduli hypot(a, 0) = |a| exactly and the products (a + 0i)(x + 0i) = ax + 0i
exactly, and both families add them in the same order:
  demote    both use 64-column tiles and four waves that take the columns w, w + 4, ... of a tile in ascending order; the waves' sums are
            added in wave order and the tiles' sums in tile order.  So ||A||_inf is the same Float64 word, the real parts of the
            ComplexF32 image are the Float32 image and its imaginary parts are +0.
  residual  cfma with zero imaginary parts is the real fma chain (its real part adds -0, its imaginary part stays +0), and the column
            split (splits, cj) is the same while ceil(n / 32) <= ceil(2048 / ceil(n / 256)), far beyond every n here.  So the real parts
            of R are the real R and the imaginary parts are +0.
No tolerance anywhere.  Every call goes through the raw C ABI.

Sizes.  Demote: n = 1; 65 (one tile plus a row and a column); 129 (past the real tile's 128 rows); 257 (past the 256-row block of the
second stage of the norm).  Residual: n in {1, 257, 513} (one, two and three of the complex kernel's 256-row workgroups, one and two of
the real kernel's 512-row ones) with 1, 8 and 9 right-hand sides (9 = two passes); random Float64 data, not integers, so that the order
of the sums shows."""
import numpy as np
import pytest

import mixed_cases as mc
from gpu_util import Store, handle
from test_gpu_mixed_exact import mixed_getrf, residual_path  # noqa: F401

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)


def words(store):
    """the matrix of a Store as its real words, outer x inner x (1 | 2): what get() returns, without arithmetic on signed zeros"""
    return store.raw()[store.off:].reshape(store.outer, store.ld, store.w)[:, :store.inner]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


@pytest.mark.parametrize("n", [1, 65, 129, 257])
def test_complex_demote_of_an_embedded_real_matrix_is_the_real_demote(n):
    """mixed_cases' upper-triangular input: the factorization does no arithmetic on the upper triangle, so there the images are compared
    on bits; below it both hold the zeros the elimination leaves, compared by value (a division or an update may flip a zero's sign).
    With 16-byte accesses and, one word off with odd leading dimensions, with the element-wise ones."""
    h = handle()
    A = mc.demote_input(n, "upper")
    vis = mc.visible("upper")(n)
    for aligned in (True, False):
        off = 0 if aligned else 1
        lda, ldf = (n + 2 - n % 2, (n + 3) // 4 * 4 + 4) if aligned else (n + 1 + n % 2, n + 3)
        sAr, sFr = Store(A, lda, off=off), Store(np.full((n, n), -7.25), ldf, np.float32, off=off, row_major=True)
        sAc, sFc = Store(A + 0j, lda, off=off), Store(np.full((n, n), -7.25 * (1 + 1j)), ldf, np.float32, off=off, row_major=True)
        what = f"n={n} aligned={aligned}"
        ipiv_r, anorm_r, info_r = mixed_getrf(h, n, sAr, sFr)
        ipiv_c, anorm_c, info_c = mixed_getrf(h, n, sAc, sFc, "rflu_mixed_getrf_cf64_dev")
        assert info_r == 0 and info_c == 0 and np.array_equal(ipiv_r, ipiv_c), what
        # a guard, so that the equality is not between two wrong words
        assert anorm_r == mc.exact_anorm(A), what
        assert bits(np.float64(anorm_c)) == bits(np.float64(anorm_r)), f"{what}: ||A||_inf {anorm_c!r} complex, {anorm_r!r} real"
        fr, fc = words(sFr), words(sFc)
        assert np.array_equal(fr[..., 0], mc.expected_image(A)), what
        assert np.array_equal(bits(fc[..., 0])[vis], bits(fr[..., 0])[vis]), f"{what}: real parts of the image"
        assert not bits(fc[..., 1])[vis].any(), f"{what}: an imaginary part of the image is not +0"
        assert np.array_equal(fc[..., 0], fr[..., 0]) and not fc[..., 1].any(), f"{what}: below the diagonal"
        assert sFr.padding_intact() and sFc.padding_intact(), what


@pytest.mark.parametrize("residual_path", ["residual_few"], indirect=True)
@pytest.mark.parametrize("nrhs", [1, 8, 9])
@pytest.mark.parametrize("n", [1, 257, 513])
def test_complex_residual_of_embedded_real_data_is_the_real_residual(n, nrhs, residual_path):
    h = handle()
    rng = np.random.default_rng([52000, n, nrhs])
    A, X, B = rng.standard_normal((n, n)), rng.standard_normal((n, nrhs)), rng.standard_normal((n, nrhs))
    # the guard, so that the equality is not between two wrong words: a Float64 sum of n products and one subtraction, in any order, is
    # within (n + 2) eps (|B| + |A| |X|) of the exact one; the kernel's and numpy's are two such sums
    ref, bar = B - A @ X, 2 * (n + 2) * EPS * (np.abs(B) + np.abs(A) @ np.abs(X))
    for aligned in (True, False):
        off = 0 if aligned else 1
        ld = (lambda pad: n + 2 - n % 2) if aligned else (lambda pad: n + pad + n % 2)      # even on a boundary / odd, one word off
        got = []
        for name, z, blank in (("rflu_residual_f64_dev", 0.0, -7.25), ("rflu_residual_cf64_dev", 0j, -7.25 * (1 + 1j))):
            sA, sX, sB = Store(A + z, ld(1), off=off), Store(X + z, ld(3), off=off), Store(B + z, ld(5), off=off)
            sR = Store(np.full((n, nrhs), blank), ld(7), off=off)
            h.call(name, n, nrhs, sA.ptr, sA.ld, sX.ptr, sX.ld, sB.ptr, sB.ld, sR.ptr, sR.ld)
            assert sR.padding_intact()
            got.append(words(sR))
        rr, rc = got
        what = f"n={n} nrhs={nrhs} aligned={aligned}"
        assert (np.abs(rr[..., 0].T - ref) <= bar).all(), what
        bad = np.argwhere(bits(rc[..., 0]) != bits(rr[..., 0]))
        assert bad.size == 0, f"{what}: {len(bad)} real parts differ, the first at (column, row) {bad[0]}"
        assert not bits(rc[..., 1]).any(), f"{what}: an imaginary part is not +0"
