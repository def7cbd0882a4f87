"""-m gpu: the complex mixed-precision solve -- ComplexF32 factors of a ComplexF64 matrix, ComplexF64 iterative refinement (LAPACK
zcgesv's scheme) -- through rflu_mixed_getrf_cf64_dev / rflu_mixed_getrs_cf64_dev / rflu_residual_cf64_dev /
rflu_mixed_solve_cf32_dev and lu_complex_mixed / ldiv_complex_mixed.  Inputs, references and bars: tests/complex_mixed_cases.py, proved
on the CPU by tests/test_complex_mixed_cases.py.

Bars.  (a) the rule itself, per column, recomputed in NumPy with moduli: ||b - A x||_inf <= ||x||_inf ||A||_inf eps sqrt(n).  The
unrefined ComplexF32 solve misses it by 4e7 .. 3e8 on the CPU, so this is the assertion that fails without refinement.  (b) the
project's Float64 bars (test_gpu_mixed.py): ||A X - B||_F < 1000 n eps (||A||_2 ||Xref|| + ||B||), relative error below 1e-6.
(c) the forward solve on constructed factors: == (complex_mixed_cases.exact_solve_case says why).  (d) the residual kernel alone
against np.clongdouble: |R - exact| <= 2 (n + 2) eps (|A| |X| + |B|) componentwise in moduli: each part is a chain of 2n fused
multiply-adds bounded by n eps sum |a| |x|, the modulus of the error is sqrt(2) of that, and 2 covers the subtraction.
(e) ||A||_inf: |anorm - max row sum of |a_ij|| <= (n + 2) eps anorm: one hypot is within an ulp, n additions add n eps / 2.
"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import complex_mixed_cases as cm
import recursivefactorization.jl_amd as rf
from gpu_util import handle, ptr, to_dev_cm
from test_julia_glue import ROOT

pytestmark = pytest.mark.gpu

EPS = cm.EPS
PASS = 8   # right-hand sides per launch of cresidual_few (csrc/rflu_internal.hpp: RESIDUAL_PASS)


def _crossover_default():
    src = open(os.path.join(ROOT, "recursivefactorization.jl_amd", "csrc", "rflu_internal.hpp")).read()
    assert int(re.search(r"constexpr int RESIDUAL_PASS = (\d+);", src).group(1)) == PASS
    return int(re.search(r"int64_t mixed_gemv_max_rhs = (\d+);", src).group(1))


@functools.lru_cache(maxsize=None)
def grid_case(n, nrhs):
    """(A, B, Xref, ||A||_2): computed once, shared by the tests, never written."""
    A, B = cm.grid_input(n, nrhs)
    return A, B, np.linalg.solve(A, B), cm.norm2(A)


def check_float64_quality(A, B, X, Xref, nrm2, what):
    """Bars (a) and (b) on a solution X of A X = B."""
    A, B, X, Xref = (np.asarray(M).reshape(M.shape[0], -1) for M in (A, B, X, Xref))
    ratio = cm.rule_ratio(A, X, B - A @ X)
    res, bound, err = cm.float64_bars(A, B, X, Xref, nrm2)
    print(f"{what}: worst ||r||/bound {np.max(ratio):.3e}, residual {res:.3e} (bound {bound:.3e}, ratio {res / bound:.3e}), solution error {err:.3e}")
    assert np.all(np.isfinite(X))
    assert np.all(ratio <= 1.0), ratio.max()
    assert res < bound
    assert err < 1e-6


def check_anorm(anorm, A):
    n = A.shape[0]
    row_sums = cm.anorm_inf(A)
    print(f"anorm: |anorm - row sums| / ((n + 2) eps anorm) = {abs(anorm - row_sums) / ((n + 2) * EPS * anorm):.3e}")
    assert abs(anorm - row_sums) <= (n + 2) * EPS * anorm


@pytest.mark.parametrize("n,nrhs", cm.GRID)
def test_refinement_reaches_float64_quality(n, nrhs):
    A, B, Xref, nrm2 = grid_case(n, nrhs)
    dA, dB = _dev(A), _dev(B)
    F = rf.lu_complex_mixed(dA)
    assert F.info == 0 and F.A is dA and F.F32.dtype == torch.complex64 and F.F32.stride(1) == 1
    X = rf.ldiv_complex_mixed(F, dB, fallback=False)
    print(f"n={n} nrhs={nrhs}: {F.iters} refinement steps (CPU restatement: {cm.CPU_STEPS[n]})")
    assert 0 <= F.iters <= cm.GPU_STEP_ALLOWANCE and not F.fell_back
    if n >= 8:
        assert F.iters >= 1
    assert X.shape == dB.shape and X.dtype == torch.complex128 and X.data_ptr() != dB.data_ptr()
    check_float64_quality(A, B, X.cpu().numpy(), Xref, nrm2, f"n={n} nrhs={nrhs}")
    assert np.array_equal(dA.cpu().numpy(), A) and np.array_equal(dB.cpu().numpy(), B)   # only read
    check_anorm(F.anorm, A)


def _dev(M):
    """column-major device copy of a (possibly read-only) host array"""
    return to_dev_cm(np.array(M, order="F"))


class Padded:
    """A complex matrix held with leading dimension ld (complex elements) in a REAL device buffer: NaN in the padding, the first element
    ONE REAL WORD after a 16-byte boundary (8 bytes for Float64 parts, 4 for Float32: aligned to the real type only).  Column-major
    unless row_major.  `ptr` is what the C entries take; `get()` reads the matrix back, `raw()` the whole buffer."""

    def __init__(self, M, ld, real=np.float64, row_major=False):
        S = np.asarray(M) if row_major else np.asarray(M).T            # outer x inner, inner contiguous
        self.outer, self.inner = S.shape
        self.ld, self.row_major = ld, row_major
        host = np.full(2 * self.outer * ld + 1, np.nan, dtype=real)
        v = host[1:].reshape(self.outer, ld, 2)
        v[:, :self.inner, 0], v[:, :self.inner, 1] = S.real, S.imag
        self.buf = torch.from_numpy(host).to("cuda:0")
        assert self.buf.data_ptr() % 16 == 0
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + host.itemsize)

    def raw(self):
        return self.buf.cpu().numpy()

    def get(self):
        v = self.raw()[1:].reshape(self.outer, self.ld, 2)[:, :self.inner]
        S = v[..., 0] + 1j * v[..., 1]
        return S if self.row_major else S.T

    def padding_is_nan(self):
        r = self.raw()
        return bool(np.isnan(r[0]) and np.isnan(r[1:].reshape(self.outer, self.ld, 2)[:, self.inner:]).all())


def same_bits(a, b):
    return a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("nrhs", cm.EXACT_NRHS)
@pytest.mark.parametrize("n", cm.EXACT_N)
def test_forward_solve_on_constructed_factors_is_exact(n, nrhs):
    c = cm.exact_solve_case(n, nrhs)
    h = handle()
    ipiv = torch.from_numpy(c.ipiv.copy()).to("cuda:0")
    # dense and aligned
    dW = torch.from_numpy(c.W.copy()).to("cuda:0")
    dB = _dev(c.B)
    h.call("rflu_mixed_solve_cf32_dev", n, nrhs, ptr(dW), n, ptr(ipiv), ptr(dB), n)
    got = dB.cpu().numpy()
    assert np.array_equal(got, c.X), f"{np.count_nonzero(got != c.X)} of {got.size} entries differ"
    assert np.array_equal(dW.cpu().numpy(), c.W)                                          # the factors are only read
    # odd ldf / ldb, both pointers 4 bytes past a 16-byte boundary, NaN in the padding
    ldf, ldb = n + (2 if n % 2 else 1), n + (4 if n % 2 else 3)
    assert ldf % 2 == 1 and ldb % 2 == 1
    pW = Padded(c.W, ldf, np.float32, row_major=True)
    pB = Padded(c.B, ldb, np.float32)
    assert pW.ptr.value % 16 == 4 and pB.ptr.value % 16 == 4
    W0 = pW.raw()
    h.call("rflu_mixed_solve_cf32_dev", n, nrhs, pW.ptr, ldf, ptr(ipiv), pB.ptr, ldb)
    assert np.array_equal(pB.get(), c.X)
    assert same_bits(pW.raw(), W0)
    assert pB.padding_is_nan()                                                            # the padding of B was not written
    # two calls are equal
    again = _dev(c.B)
    h.call("rflu_mixed_solve_cf32_dev", n, nrhs, ptr(dW), n, ptr(ipiv), ptr(again), n)
    assert np.array_equal(again.cpu().numpy(), got)


@pytest.mark.parametrize("nrhs", [3, 9])
def test_forward_solve_notipiv(nrhs):
    """ipiv = NULL: no interchange; B' = P B of the constructed case is the right-hand side of L U X = B'."""
    n = 257
    c = cm.exact_solve_case(n, nrhs if nrhs == 9 else 8)
    k = nrhs
    Z = c.B[:, :k].copy()
    for i in range(n):
        p = c.ipiv[i] - 1
        if p != i:
            Z[[i, p]] = Z[[p, i]]
    dW, dB = torch.from_numpy(c.W.copy()).to("cuda:0"), to_dev_cm(Z)
    handle().call("rflu_mixed_solve_cf32_dev", n, k, ptr(dW), n, ctypes.c_void_p(0), ptr(dB), n)
    assert np.array_equal(dB.cpu().numpy(), c.X[:, :k])


CROSS = _crossover_default()
RES_NRHS = sorted({1, 3, PASS, PASS + 1, CROSS, CROSS + 1})


@functools.lru_cache(maxsize=None)
def residual_case(n):
    """Inputs for the widest count, B - A X in np.clongdouble and the componentwise bound: once per n, shared by both paths."""
    k = max(RES_NRHS)
    A, X, B = cm.uniform_complex(n, n, 1200 + n), cm.uniform_complex(n, k, 1201 + n), cm.uniform_complex(n, k, 1202 + n)
    ld = np.clongdouble
    exact = B.astype(ld) - A.astype(ld) @ X.astype(ld)
    bound = 2 * (n + 2) * EPS * (np.abs(A) @ np.abs(X) + np.abs(B))
    return A, X, B, exact, bound


@pytest.mark.parametrize("path", ["cresidual_few", "gemm"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000, 2049])
def test_residual_kernel_alone(n, path, monkeypatch):
    monkeypatch.setenv("RFLU_MIXED_GEMV_MAX_RHS", "1000000" if path == "cresidual_few" else "0")
    h = handle()
    h.reload_tuning()
    A, X, B, exact, bound = residual_case(n)
    pA = Padded(A, n + 3)
    for nrhs in RES_NRHS:
        pX, pB = Padded(X[:, :nrhs], n + 1), Padded(B[:, :nrhs], n + 5)
        pR = Padded(np.full((n, nrhs), np.nan + 0j), n + 7)
        h.call("rflu_residual_cf64_dev", n, nrhs, pA.ptr, n + 3, pX.ptr, n + 1, pB.ptr, n + 5, pR.ptr, n + 7)
        R = pR.get()
        err = np.abs(R.astype(np.clongdouble) - exact[:, :nrhs]).astype(np.float64)
        print(f"{path} n={n} nrhs={nrhs}: worst |R - exact| / bound = {np.max(err / bound[:, :nrhs]):.3e}")
        assert np.all(np.isfinite(R))
        assert np.all(err <= bound[:, :nrhs])
        assert pR.padding_is_nan()                                                         # the padding of R was not written
        first = pR.raw()
        h.call("rflu_residual_cf64_dev", n, nrhs, pA.ptr, n + 3, pX.ptr, n + 1, pB.ptr, n + 5, pR.ptr, n + 7)
        assert same_bits(pR.raw(), first)                                                  # bit-identical from run to run
    monkeypatch.undo()
    h.reload_tuning()


def test_odd_leading_dimensions_and_unaligned_pointers():
    n, nrhs, lda, ldb, ldx, ldf = 130, 5, 137, 133, 131, 131
    A, B = cm.uniform_complex(n, n, 900 + n), cm.uniform_complex(n, nrhs, 901 + n)
    pA, pB = Padded(A, lda), Padded(B, ldb)
    pX = Padded(np.full((n, nrhs), np.nan + 0j), ldx)
    pF = Padded(np.full((n, n), np.nan + 0j), ldf, np.float32, row_major=True)
    assert pA.ptr.value % 16 == 8 and pF.ptr.value % 16 == 4
    ipiv = torch.zeros(n, dtype=torch.int64, device="cuda:0")
    A0, B0 = pA.raw(), pB.raw()
    h = handle()
    info, anorm, iters = ctypes.c_int64(-1), ctypes.c_double(-1.0), ctypes.c_int(-99)
    h.call("rflu_mixed_getrf_cf64_dev", n, pA.ptr, lda, pF.ptr, ldf, ptr(ipiv), 1, ctypes.byref(anorm), ctypes.byref(info))
    assert info.value == 0
    check_anorm(anorm.value, A)
    h.call("rflu_mixed_getrs_cf64_dev", n, nrhs, pA.ptr, lda, pF.ptr, ldf, ptr(ipiv), anorm.value, pB.ptr, ldb, pX.ptr, ldx, 30,
           ctypes.byref(iters))
    print(f"n={n} odd leading dimensions: {iters.value} refinement steps")
    assert 1 <= iters.value <= cm.GPU_STEP_ALLOWANCE
    check_float64_quality(A, B, pX.get(), np.linalg.solve(A, B), np.linalg.norm(A, 2), "odd leading dimensions")
    # inputs bit-identical, padding included; the padding of X and F32 was not written
    assert same_bits(pA.raw(), A0) and same_bits(pB.raw(), B0)
    assert pX.padding_is_nan() and pF.padding_is_nan()
    # the same matrix from an aligned, densely packed buffer: the 16-byte and the element-wise forms add the same numbers in the same
    # order, and factor the same ComplexF32 image
    G = rf.lu_complex_mixed(to_dev_cm(A))
    assert G.anorm == anorm.value
    assert np.array_equal(G.F32.cpu().numpy(), pF.get()) and np.array_equal(G.ipiv.cpu().numpy(), ipiv.cpu().numpy())
    X2 = rf.ldiv_complex_mixed(G, to_dev_cm(B), fallback=False)
    assert G.iters == iters.value and np.array_equal(X2.cpu().numpy(), pX.get())


def test_nopivot_on_a_diagonally_dominant_matrix():
    n = 300
    A = np.asfortranarray(cm.uniform_complex(n, n, 600 + n) + 10.0 * np.eye(n))
    B = cm.uniform_complex(n, 3, 700 + n)
    F = rf.lu_complex_mixed(to_dev_cm(A), rf.NoPivot())
    assert isinstance(F.ipiv, rf.NotIPIV) and F.info == 0
    X = rf.ldiv_complex_mixed(F, to_dev_cm(B), fallback=False)
    print(f"NoPivot n={n}: {F.iters} refinement steps")
    assert 1 <= F.iters <= cm.GPU_STEP_ALLOWANCE
    check_float64_quality(A, B, X.cpu().numpy(), np.linalg.solve(A, B), np.linalg.norm(A, 2), "NoPivot")


def _raw_refine(A, B, max_iter=30):
    n, nrhs = B.shape
    dA, dB = to_dev_cm(A), to_dev_cm(B)
    dX = torch.empty((nrhs, n), dtype=torch.complex128, device="cuda:0").T
    dF = torch.empty((n, n), dtype=torch.complex64, device="cuda:0")
    ipiv = torch.zeros(n, dtype=torch.int64, device="cuda:0")
    info, anorm, iters = ctypes.c_int64(-1), ctypes.c_double(-1.0), ctypes.c_int(0)
    h = handle()
    h.call("rflu_mixed_getrf_cf64_dev", n, ptr(dA), n, ptr(dF), n, ptr(ipiv), 1, ctypes.byref(anorm), ctypes.byref(info))
    # h.call raises unless the status is RFLU_OK: non-convergence is no error of the call
    h.call("rflu_mixed_getrs_cf64_dev", n, nrhs, ptr(dA), n, ptr(dF), n, ptr(ipiv), anorm.value, ptr(dB), n, ptr(dX), n, max_iter, ctypes.byref(iters))
    return iters.value


def test_non_convergence_is_reported_never_dressed_up_as_success():
    n = 300
    B = cm.uniform_complex(n, 2, 77)
    A = cm.ill_conditioned(n, 10)                    # kappa = 1e10 >> 1 / eps32: the CPU restatement stalls at 6e6 times the bar
    iters = _raw_refine(A, B)
    print(f"kappa 1e10: iters = {iters}")
    assert iters == -31                              # 30 steps taken, not converged
    assert _raw_refine(A, B, max_iter=4) == -5
    dA, dB = to_dev_cm(A), to_dev_cm(B)
    F = rf.lu_complex_mixed(dA)
    X = rf.ldiv_complex_mixed(F, dB)
    assert F.iters < 0 and F.fell_back
    X = X.cpu().numpy()
    res, bound, _ = cm.float64_bars(A, B, X, np.linalg.solve(A, B), np.linalg.norm(A, 2))
    print(f"kappa 1e10, ComplexF64 fallback: residual {res:.3e} (bound {bound:.3e})")
    assert res < bound
    assert np.array_equal(dA.cpu().numpy(), A) and np.array_equal(dB.cpu().numpy(), B)
    with pytest.raises(rf.NotConvergedError):
        rf.ldiv_complex_mixed(F, dB, fallback=False)
    iters = _raw_refine(cm.ill_conditioned(n, 12), B)
    print(f"kappa 1e12: iters = {iters}")
    assert iters < 0
    # An entry that is finite in Float64 and overflows Float32 becomes Inf in the ComplexF32 image; nothing special-cases it.  In the LAST
    # column it cannot stay harmless: its row is taken as a pivot row at some column k < n - 1 (unless it is the very last row left, which
    # a matrix with 299 other candidates per column does not do), so u[k, n-1] = Inf meets the nonzero multipliers of the rows below in
    # the rank-1 update, Inf - Inf follows, u[n-1, n-1] is NaN or Inf and the back substitution multiplies it by 0: NaN in X, and a NaN is
    # never convergence.
    A39 = np.array(cm.grid_input(n, 64)[0], order="F")
    A39[0, n - 1] = 1e39
    iters = _raw_refine(A39, B)
    print(f"an entry of 1e39 in the last column: iters = {iters}")
    assert iters < 0
    # Elsewhere the Inf may be taken as a pivot itself: its multipliers are 0 and no NaN arises.  What holds then is the other half of the
    # contract: iters >= 0 is never reported unless the rule, which scales with ||A||_inf >= 1e39, is really met.
    A39 = np.array(cm.grid_input(n, 64)[0], order="F")
    A39[7, 11] = 1e39
    dA, dB = to_dev_cm(A39), to_dev_cm(B)
    F = rf.lu_complex_mixed(dA)
    X = rf.ldiv_complex_mixed(F, dB).cpu().numpy()
    print(f"an entry of 1e39 at (7, 11): iters = {F.iters}, fell back: {F.fell_back}")
    assert F.fell_back == (F.iters < 0) and np.all(np.isfinite(X))
    assert np.all(cm.rule_ratio(A39, X, cm.residual_ld(A39, X, B)) <= 1.0)


def test_complexf32_singular_input_falls_back_to_complexf64():
    n = 64
    A = np.eye(n, dtype=np.complex128, order="F")
    A[0:2, 0:2] = np.array([[1.0, 1.0], [1.0, 1.0 + 1e-12]]) * (1 + 1j)   # exactly singular once demoted
    B = cm.uniform_complex(n, 2, 64)
    F = rf.lu_complex_mixed(to_dev_cm(A))
    assert F.info == 2 and not F.issuccess()
    with pytest.raises(rf.SingularException):
        rf.ldiv_complex_mixed(F, to_dev_cm(B), fallback=False)
    X = rf.ldiv_complex_mixed(F, to_dev_cm(B)).cpu().numpy()
    assert F.fell_back
    res, bound, err = cm.float64_bars(A, B, X, np.linalg.solve(A, B), np.linalg.norm(A, 2))
    print(f"ComplexF32-singular: residual {res:.3e} (bound {bound:.3e}), solution error {err:.3e}")
    assert res < bound and err < 1e-6


def test_two_calls_are_bit_identical():
    n, nrhs = 1000, 9
    A, B, _, _ = grid_case(n, nrhs)
    out = []
    for _ in range(2):
        F = rf.lu_complex_mixed(_dev(A))
        X = rf.ldiv_complex_mixed(F, _dev(B), fallback=False)
        out.append((X.cpu().numpy(), F.anorm, F.iters))
    assert np.array_equal(out[0][0], out[1][0]) and out[0][1] == out[1][1] and out[0][2] == out[1][2]


def test_argument_checks_of_the_abi():
    h = handle()
    n = 16
    dA, dB = to_dev_cm(cm.uniform_complex(n, n, 1)), to_dev_cm(cm.uniform_complex(n, 2, 2))
    dX = torch.empty((2, n), dtype=torch.complex128, device="cuda:0").T
    dF = torch.empty((n, n), dtype=torch.complex64, device="cuda:0")
    dB32 = torch.zeros((2, n), dtype=torch.complex64, device="cuda:0").T
    ipiv = torch.zeros(n, dtype=torch.int64, device="cuda:0")
    info, anorm, iters = ctypes.c_int64(0), ctypes.c_double(0.0), ctypes.c_int(7)
    null = ctypes.c_void_p(0)
    rf_, rs_, res_, sol_ = "rflu_mixed_getrf_cf64_dev", "rflu_mixed_getrs_cf64_dev", "rflu_residual_cf64_dev", "rflu_mixed_solve_cf32_dev"
    bad = [
        (rf_, (-1, ptr(dA), n, ptr(dF), n, ptr(ipiv), 1, ctypes.byref(anorm), ctypes.byref(info))),
        (rf_, (n, ptr(dA), n - 1, ptr(dF), n, ptr(ipiv), 1, ctypes.byref(anorm), ctypes.byref(info))),
        (rf_, (n, ptr(dA), n, ptr(dF), n - 1, ptr(ipiv), 1, ctypes.byref(anorm), ctypes.byref(info))),
        (rf_, (n, null, n, ptr(dF), n, ptr(ipiv), 1, ctypes.byref(anorm), ctypes.byref(info))),
        (rf_, (n, ptr(dA), n, ptr(dF), n, null, 1, ctypes.byref(anorm), ctypes.byref(info))),   # pivoting needs ipiv
        (rf_, (n, ptr(dA), n, ptr(dF), n, ptr(ipiv), 1, null, ctypes.byref(info))),
        (rs_, (n, -2, ptr(dA), n, ptr(dF), n, ptr(ipiv), 1.0, ptr(dB), n, ptr(dX), n, 30, ctypes.byref(iters))),
        (rs_, (n, 2, ptr(dA), n, ptr(dF), n, ptr(ipiv), 1.0, ptr(dB), n - 1, ptr(dX), n, 30, ctypes.byref(iters))),
        (rs_, (n, 2, ptr(dA), n, ptr(dF), n, ptr(ipiv), 1.0, ptr(dB), n, null, n, 30, ctypes.byref(iters))),
        (rs_, (n, 2, ptr(dA), n, ptr(dF), n, ptr(ipiv), 1.0, ptr(dB), n, ptr(dX), n, 30, null)),
        (res_, (n, 2, ptr(dA), n, ptr(dX), n, ptr(dB), n, null, n)),
        (res_, (n, 2, ptr(dA), n, ptr(dX), n - 1, ptr(dB), n, ptr(dX), n)),
        (sol_, (-1, 2, ptr(dF), n, ptr(ipiv), ptr(dB32), n)),
        (sol_, (n, 2, ptr(dF), n - 1, ptr(ipiv), ptr(dB32), n)),
        (sol_, (n, 2, ptr(dF), n, ptr(ipiv), ptr(dB32), n - 1)),
        (sol_, (n, 2, null, n, ptr(ipiv), ptr(dB32), n)),
        (sol_, (n, 2, ptr(dF), n, ptr(ipiv), null, n)),
    ]
    for name, args in bad:
        with pytest.raises(rf.RfluError, match="status 1"):
            h.call(name, *args)
    # empty problems: success, *iters = 0, nothing launched
    h.call(rs_, n, 0, ptr(dA), n, ptr(dF), n, ptr(ipiv), 1.0, null, n, null, n, 30, ctypes.byref(iters))
    assert iters.value == 0
    iters.value = 7
    h.call(rs_, 0, 2, null, 1, null, 1, null, 0.0, null, 1, null, 1, 30, ctypes.byref(iters))
    assert iters.value == 0
    h.call(rf_, 0, null, 1, null, 1, null, 1, ctypes.byref(anorm), ctypes.byref(info))
    assert info.value == 0 and anorm.value == 0.0
    h.call(res_, 0, 2, null, 1, null, 1, null, 1, null, 1)
    h.call(res_, n, 0, null, n, null, n, null, n, null, n)
    h.call(sol_, 0, 2, null, 1, null, null, 1)
    h.call(sol_, n, 0, null, n, null, null, n)
