"""-m gpu: the mixed-precision solve -- Float32 factors of a Float64 matrix, Float64 iterative refinement (LAPACK dsgesv's scheme) --
through rflu_mixed_getrf_f64_dev / rflu_mixed_getrs_f64_dev / rflu_residual_f64_dev, lu_mixed / ldiv_mixed and
linsolve.RF32MixedLUFactorization.

Bounds.  (a) dsgesv's own rule, per column, recomputed in NumPy: ||b - A x||_inf <= ||x||_inf ||A||_inf eps sqrt(n).  A plain Float32
solve of these inputs misses it by seven to eight orders of magnitude (first-iterate ratios 1.4e-8 .. 6.3e-7 with scipy's Float32
lu_factor on the CPU), so this is the assertion that fails without refinement.  (b) the project's bounds for a Float64 solve
(test_gpu_ldiv_adjoint.py): ||A X - B||_F < 1000 n eps (||A||_2 ||Xref|| + ||B||) and a relative solution error below 1e-6; on the CPU
the refined solutions of the grid below sit at most at 0.006 of the first and 7e-12 of the second.  From n = 2000 on ||A||_2 enters
through a LOWER bound (power iteration, as test_adjoint_solve_n16384 does): the SVD of such a matrix takes many seconds, and a
smaller norm only tightens the bound.  Step counts: the same inputs converge on the CPU in 2 steps for n <= 1001, 3 at 2100 and 5 at
4100; the GPU's Float32 factorization rounds differently from LAPACK's, so the allowance is twice the CPU maximum.
(c) the residual kernel alone, componentwise against B - A X in np.longdouble: |R_gpu - R_exact| <= (n + 2) eps (|A| |X| + |B|), the
standard bound of a dot product of length n followed by one subtraction.
"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import recursivefactorization.jl_amd as rf
from gpu_util import handle, ptr, to_dev_cm
from helpers import rand_matrix
from recursivefactorization.jl_amd import linsolve as LS
from test_julia_glue import ROOT

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
GRID = [(1, 1), (8, 1), (65, 3), (129, 8), (300, 64), (513, 1), (1000, 9), (1001, 3), (2100, 33), (4100, 20)]
PASS = 8   # right-hand sides per launch of residual_few (csrc/rflu_internal.hpp: RESIDUAL_PASS)


def _crossover_default():
    src = open(os.path.join(ROOT, "recursivefactorization.jl_amd", "csrc", "rflu_internal.hpp")).read()
    assert int(re.search(r"constexpr int RESIDUAL_PASS = (\d+);", src).group(1)) == PASS
    return int(re.search(r"int64_t mixed_gemv_max_rhs = (\d+);", src).group(1))


def norm2(A):
    """||A||_2; from n = 2000 on a lower bound of it (twenty steps of the power iteration on A'A)."""
    if A.shape[0] < 2000:
        return np.linalg.norm(A, 2)
    w = np.ones(A.shape[0])
    for _ in range(20):
        w = A.T @ (A @ w)
        w /= np.linalg.norm(w)
    return np.linalg.norm(A @ w)


@functools.lru_cache(maxsize=None)
def grid_case(n, nrhs):
    """(A, B, Xref, ||A||_2): computed once, shared by the tests, never written."""
    A = rand_matrix(n, n, seed=900 + n)
    B = rand_matrix(n, nrhs, seed=901 + n).copy(order="F")
    return A, B, np.linalg.solve(A, B), norm2(A)


def check_float64_quality(A, B, X, Xref, nrm2, what):
    """The assertions (a) and (b) of the module docstring on a solution X of A X = B."""
    A, B, X, Xref = (np.asarray(M).reshape(M.shape[0], -1) for M in (A, B, X, Xref))
    n = A.shape[0]
    R = B - A @ X
    anorm = np.abs(A).sum(axis=1).max()
    rn, xn = np.abs(R).max(axis=0), np.abs(X).max(axis=0)
    bound = xn * anorm * EPS * np.sqrt(n)
    res = np.linalg.norm(A @ X - B)
    scale = nrm2 * np.linalg.norm(Xref) + np.linalg.norm(B)
    err = np.linalg.norm(X - Xref) / np.linalg.norm(Xref)
    print(f"{what}: worst ||r||/bound {np.max(rn / bound):.3e}, residual {res:.3e} (bound {1000 * n * EPS * scale:.3e}), solution error {err:.3e}")
    assert np.all(np.isfinite(X))
    assert np.all(rn <= bound), (rn / bound).max()
    assert res < 1000 * n * EPS * scale
    assert err < 1e-6


@pytest.mark.parametrize("n,nrhs", GRID)
def test_refinement_reaches_float64_quality(n, nrhs):
    A, B, Xref, nrm2 = grid_case(n, nrhs)
    dA, dB = to_dev_cm(A), to_dev_cm(B)
    F = rf.lu_mixed(dA)
    assert F.info == 0 and F.A is dA and F.F32.dtype == torch.float32
    X = rf.ldiv_mixed(F, dB, fallback=False)
    print(f"n={n} nrhs={nrhs}: {F.iters} refinement steps")
    assert F.iters >= 0 and not F.fell_back
    assert F.iters <= 10
    if n >= 8:
        assert F.iters >= 1
    assert X.shape == dB.shape and X.data_ptr() != dB.data_ptr()
    check_float64_quality(A, B, X.cpu().numpy(), Xref, nrm2, f"n={n} nrhs={nrhs}")
    assert np.array_equal(dA.cpu().numpy(), A) and np.array_equal(dB.cpu().numpy(), B)   # only read
    row_sums = np.abs(A).sum(axis=1).max()
    assert abs(F.anorm - row_sums) <= n * EPS * row_sums


def _padded_cm(M, ld, dtype=torch.float64):
    """Column-major copy of M with leading dimension ld, NaN in the padding, starting ONE ELEMENT after a 16-byte boundary."""
    rows, cols = M.shape
    buf = torch.full((cols * ld + 1,), float("nan"), dtype=dtype, device="cuda:0")
    assert buf.data_ptr() % 16 == 0
    view = buf[1:].view(cols, ld).T[:rows]          # shape (rows, cols), strides (1, ld)
    view.copy_(torch.from_numpy(np.ascontiguousarray(M)).to("cuda:0"))
    assert view.data_ptr() % 16 == buf.element_size() and view.stride() == (1, ld)
    return buf, view


def test_odd_leading_dimensions_and_unaligned_pointers():
    n, nrhs, lda, ldb, ldx, ldf = 130, 5, 137, 133, 131, 131
    A = rand_matrix(n, n, seed=900 + n)
    B = rand_matrix(n, nrhs, seed=901 + n).copy(order="F")
    Abuf, dA = _padded_cm(A, lda)
    Bbuf, dB = _padded_cm(B, ldb)
    Xbuf, dX = _padded_cm(np.full((n, nrhs), np.nan), ldx)
    Fbuf = torch.full((n * ldf + 1,), float("nan"), dtype=torch.float32, device="cuda:0")
    dF = Fbuf[1:].view(n, ldf)                      # row-major, 4 bytes after a 16-byte boundary
    ipiv = torch.zeros(n, dtype=torch.int64, device="cuda:0")
    A0, B0 = Abuf.clone(), Bbuf.clone()
    h = handle()
    info, anorm, iters = ctypes.c_int64(-1), ctypes.c_double(-1.0), ctypes.c_int(-99)
    h.call("rflu_mixed_getrf_f64_dev", n, ptr(dA), lda, ptr(dF), ldf, ptr(ipiv), 1, 0, ctypes.byref(anorm), ctypes.byref(info))
    assert info.value == 0
    row_sums = np.abs(A).sum(axis=1).max()
    assert abs(anorm.value - row_sums) <= n * EPS * row_sums
    h.call("rflu_mixed_getrs_f64_dev", n, nrhs, ptr(dA), lda, ptr(dF), ldf, ptr(ipiv), anorm.value, ptr(dB), ldb, ptr(dX), ldx, 30,
           ctypes.byref(iters))
    print(f"n={n} odd leading dimensions: {iters.value} refinement steps")
    assert 1 <= iters.value <= 10
    check_float64_quality(A, B, dX.cpu().numpy(), np.linalg.solve(A, B), np.linalg.norm(A, 2), "odd leading dimensions")
    # inputs bit-identical, padding included; the padding of X and F32 was not written
    assert torch.equal(Abuf.view(torch.int64), A0.view(torch.int64)) and torch.equal(Bbuf.view(torch.int64), B0.view(torch.int64))
    assert bool(torch.isnan(Xbuf[1:].view(nrhs, ldx)[:, n:]).all()) and bool(torch.isnan(Xbuf[:1]).all())
    assert bool(torch.isnan(dF[:, n:]).all()) and bool(torch.isnan(Fbuf[:1]).all())
    # the same matrix from an aligned, densely packed buffer: the 16-byte and the element-wise loads add the row sums in the same order
    assert rf.lu_mixed(to_dev_cm(A)).anorm == anorm.value


def test_nopivot_on_a_diagonally_dominant_matrix():
    n = 300
    A = np.asfortranarray(rand_matrix(n, n, seed=600 + n) + 10.0 * np.eye(n))
    B = rand_matrix(n, 3, seed=700 + n).copy(order="F")
    F = rf.lu_mixed(to_dev_cm(A), rf.NoPivot())
    assert isinstance(F.ipiv, rf.NotIPIV) and F.info == 0
    X = rf.ldiv_mixed(F, to_dev_cm(B), fallback=False)
    print(f"NoPivot n={n}: {F.iters} refinement steps")
    assert 1 <= F.iters <= 10
    check_float64_quality(A, B, X.cpu().numpy(), np.linalg.solve(A, B), np.linalg.norm(A, 2), "NoPivot")


def _ill_conditioned(n, log10_kappa):
    rng = np.random.default_rng(5)
    Q1, _ = np.linalg.qr(rng.standard_normal((n, n)))
    Q2, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return np.asfortranarray(Q1 @ np.diag(np.logspace(0, -log10_kappa, n)) @ Q2.T)


def _raw_refine(A, B, max_iter=30):
    n, nrhs = B.shape
    dA, dB = to_dev_cm(A), to_dev_cm(B)
    dX = torch.empty((nrhs, n), dtype=torch.float64, device="cuda:0").T
    dF = torch.empty((n, n), dtype=torch.float32, device="cuda:0")
    ipiv = torch.zeros(n, dtype=torch.int64, device="cuda:0")
    info, anorm, iters = ctypes.c_int64(-1), ctypes.c_double(-1.0), ctypes.c_int(0)
    h = handle()
    h.call("rflu_mixed_getrf_f64_dev", n, ptr(dA), n, ptr(dF), n, ptr(ipiv), 1, 0, ctypes.byref(anorm), ctypes.byref(info))
    # h.call raises unless the status is RFLU_OK: non-convergence is no error of the call
    h.call("rflu_mixed_getrs_f64_dev", n, nrhs, ptr(dA), n, ptr(dF), n, ptr(ipiv), anorm.value, ptr(dB), n, ptr(dX), n, max_iter, ctypes.byref(iters))
    return iters.value


def test_non_convergence_is_reported_never_dressed_up_as_success():
    n = 300
    B = rand_matrix(n, 2, seed=77).copy(order="F")
    A = _ill_conditioned(n, 10)                      # kappa = 1e10 >> 1 / eps32: the refinement stalls (about 2e-8 on the CPU)
    iters = _raw_refine(A, B)
    print(f"kappa 1e10: iters = {iters}")
    assert iters == -31                              # 30 steps taken, not converged
    assert _raw_refine(A, B, max_iter=4) == -5
    dA, dB = to_dev_cm(A), to_dev_cm(B)
    F = rf.lu_mixed(dA)
    X = rf.ldiv_mixed(F, dB)
    assert F.iters < 0 and F.fell_back
    X = X.cpu().numpy()
    Xref = np.linalg.solve(A, B)
    res = np.linalg.norm(A @ X - B)
    bound = 1000 * n * EPS * (np.linalg.norm(A, 2) * np.linalg.norm(Xref) + np.linalg.norm(B))
    print(f"kappa 1e10, Float64 fallback: residual {res:.3e} (bound {bound:.3e})")
    assert res < bound
    assert np.array_equal(dA.cpu().numpy(), A) and np.array_equal(dB.cpu().numpy(), B)
    with pytest.raises(rf.NotConvergedError):
        rf.ldiv_mixed(F, dB, fallback=False)
    # kappa = 1e12: the iterate overflows to Inf on the CPU within 30 steps; the call must come back and say "not converged"
    iters = _raw_refine(_ill_conditioned(n, 12), B)
    print(f"kappa 1e12: iters = {iters}")
    assert iters < 0


def test_float32_singular_input_falls_back_to_float64():
    n = 64
    A = np.eye(n, order="F")
    A[0:2, 0:2] = [[1.0, 1.0], [1.0, 1.0 + 1e-12]]   # exactly singular once demoted
    B = rand_matrix(n, 2, seed=64).copy(order="F")
    F = rf.lu_mixed(to_dev_cm(A))
    assert F.info == 2 and not F.issuccess()
    with pytest.raises(rf.SingularException):
        rf.ldiv_mixed(F, to_dev_cm(B), fallback=False)
    X = rf.ldiv_mixed(F, to_dev_cm(B)).cpu().numpy()
    assert F.fell_back
    Xref = np.linalg.solve(A, B)
    res = np.linalg.norm(A @ X - B)
    bound = 1000 * n * EPS * (np.linalg.norm(A, 2) * np.linalg.norm(Xref) + np.linalg.norm(B))
    print(f"Float32-singular: residual {res:.3e} (bound {bound:.3e})")
    assert res < bound


CROSS = _crossover_default()
RES_NRHS = sorted({1, 3, PASS, PASS + 1, CROSS, CROSS + 1})


@functools.lru_cache(maxsize=None)
def residual_case(n):
    """Inputs for the widest count and B - A X in np.longdouble with its componentwise bound: once per n, shared by both paths."""
    k = max(RES_NRHS)
    A, X, B = rand_matrix(n, n, seed=1200 + n), rand_matrix(n, k, seed=1201 + n), rand_matrix(n, k, seed=1202 + n)
    exact = B.astype(np.longdouble) - A.astype(np.longdouble) @ X.astype(np.longdouble)
    bound = (n + 2) * EPS * (np.abs(A) @ np.abs(X) + np.abs(B))
    return A, X, B, exact, bound


@pytest.mark.parametrize("path", ["residual_few", "gemm"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000, 2049])
def test_residual_kernel_alone(n, path, monkeypatch):
    monkeypatch.setenv("RFLU_MIXED_GEMV_MAX_RHS", "1000000" if path == "residual_few" else "0")
    h = handle()
    h.reload_tuning()
    A, X, B, exact, bound = residual_case(n)
    _, dA = _padded_cm(A, n + 3)
    for nrhs in RES_NRHS:
        _, dX = _padded_cm(X[:, :nrhs], n + 1)
        _, dB = _padded_cm(B[:, :nrhs], n + 5)
        Rbuf, dR = _padded_cm(np.full((n, nrhs), np.nan), n + 7)
        h.call("rflu_residual_f64_dev", n, nrhs, ptr(dA), n + 3, ptr(dX), n + 1, ptr(dB), n + 5, ptr(dR), n + 7)
        R = dR.cpu().numpy()
        err = np.abs(R.astype(np.longdouble) - exact[:, :nrhs]).astype(np.float64)
        print(f"{path} n={n} nrhs={nrhs}: worst |R - exact| / bound = {np.max(err / bound[:, :nrhs]):.3e}")
        assert np.all(np.isfinite(R))
        assert np.all(err <= bound[:, :nrhs])
        assert bool(torch.isnan(Rbuf[1:].view(nrhs, n + 7)[:, n:]).all())       # the padding of R was not written
        h.call("rflu_residual_f64_dev", n, nrhs, ptr(dA), n + 3, ptr(dX), n + 1, ptr(dB), n + 5, ptr(dR), n + 7)
        assert np.array_equal(dR.cpu().numpy(), R)                               # bit-identical from run to run


def test_two_calls_are_bit_identical():
    n, nrhs = 1000, 9
    A, B, _, _ = grid_case(n, nrhs)
    out = []
    for _ in range(2):
        F = rf.lu_mixed(to_dev_cm(A))
        X = rf.ldiv_mixed(F, to_dev_cm(B), fallback=False)
        out.append((X.cpu().numpy(), F.anorm, F.iters))
    assert np.array_equal(out[0][0], out[1][0]) and out[0][1] == out[1][1] and out[0][2] == out[1][2]


def test_argument_checks_of_the_abi():
    h = handle()
    n = 16
    dA, dB = to_dev_cm(rand_matrix(n, n, seed=1)), to_dev_cm(rand_matrix(n, 2, seed=2))
    dX = torch.empty((2, n), dtype=torch.float64, device="cuda:0").T
    dF = torch.empty((n, n), dtype=torch.float32, device="cuda:0")
    ipiv = torch.zeros(n, dtype=torch.int64, device="cuda:0")
    info, anorm, iters = ctypes.c_int64(0), ctypes.c_double(0.0), ctypes.c_int(7)
    null = ctypes.c_void_p(0)
    bad = [
        ("rflu_mixed_getrf_f64_dev", (-1, ptr(dA), n, ptr(dF), n, ptr(ipiv), 1, 0, ctypes.byref(anorm), ctypes.byref(info))),
        ("rflu_mixed_getrf_f64_dev", (n, ptr(dA), n - 1, ptr(dF), n, ptr(ipiv), 1, 0, ctypes.byref(anorm), ctypes.byref(info))),
        ("rflu_mixed_getrf_f64_dev", (n, ptr(dA), n, ptr(dF), n - 1, ptr(ipiv), 1, 0, ctypes.byref(anorm), ctypes.byref(info))),
        ("rflu_mixed_getrf_f64_dev", (n, null, n, ptr(dF), n, ptr(ipiv), 1, 0, ctypes.byref(anorm), ctypes.byref(info))),
        ("rflu_mixed_getrf_f64_dev", (n, ptr(dA), n, ptr(dF), n, null, 1, 0, ctypes.byref(anorm), ctypes.byref(info))),   # pivoting needs ipiv
        ("rflu_mixed_getrf_f64_dev", (n, ptr(dA), n, ptr(dF), n, ptr(ipiv), 1, 0, null, ctypes.byref(info))),
        ("rflu_mixed_getrs_f64_dev", (n, -2, ptr(dA), n, ptr(dF), n, ptr(ipiv), 1.0, ptr(dB), n, ptr(dX), n, 30, ctypes.byref(iters))),
        ("rflu_mixed_getrs_f64_dev", (n, 2, ptr(dA), n, ptr(dF), n, ptr(ipiv), 1.0, ptr(dB), n - 1, ptr(dX), n, 30, ctypes.byref(iters))),
        ("rflu_mixed_getrs_f64_dev", (n, 2, ptr(dA), n, ptr(dF), n, ptr(ipiv), 1.0, ptr(dB), n, null, n, 30, ctypes.byref(iters))),
        ("rflu_mixed_getrs_f64_dev", (n, 2, ptr(dA), n, ptr(dF), n, ptr(ipiv), 1.0, ptr(dB), n, ptr(dX), n, 30, null)),
        ("rflu_residual_f64_dev", (n, 2, ptr(dA), n, ptr(dX), n, ptr(dB), n, null, n)),
        ("rflu_residual_f64_dev", (n, 2, ptr(dA), n, ptr(dX), n - 1, ptr(dB), n, ptr(dX), n)),
    ]
    for name, args in bad:
        with pytest.raises(rf.RfluError, match="status 1"):
            h.call(name, *args)
    # empty problems: success, *iters = 0, nothing launched
    h.call("rflu_mixed_getrs_f64_dev", n, 0, ptr(dA), n, ptr(dF), n, ptr(ipiv), 1.0, null, n, null, n, 30, ctypes.byref(iters))
    assert iters.value == 0
    iters.value = 7
    h.call("rflu_mixed_getrs_f64_dev", 0, 2, null, 1, null, 1, null, 0.0, null, 1, null, 1, 30, ctypes.byref(iters))
    assert iters.value == 0
    h.call("rflu_mixed_getrf_f64_dev", 0, null, 1, null, 1, null, 1, 0, ctypes.byref(anorm), ctypes.byref(info))
    assert info.value == 0 and anorm.value == 0.0


def test_linear_solve_protocol_on_the_device():
    n = 1000
    A, B, Xref, nrm2 = grid_case(n, 9)
    dA = to_dev_cm(A)
    b1, b2 = B[:, 0].copy(), B[:, 1].copy()
    cache = LS.init(dA, torch.from_numpy(b1).to("cuda:0"), LS.RF32MixedLUFactorization())
    assert cache.isfresh and cache.nfactor == 0
    sol = LS.solve_(cache)
    assert sol.retcode is LS.ReturnCode.Success and cache.nfactor == 1 and not cache.isfresh
    assert isinstance(cache.cacheval, rf.MixedLU) and cache.cacheval.iters >= 1 and not cache.cacheval.fell_back
    check_float64_quality(A, b1, sol.u.cpu().numpy(), Xref[:, 0], nrm2, "LinearSolve, first b")
    cache.b = torch.from_numpy(b2).to("cuda:0")
    sol = LS.solve_(cache)
    assert sol.retcode is LS.ReturnCode.Success and cache.nfactor == 1                 # the factors were reused
    check_float64_quality(A, b2, sol.u.cpu().numpy(), Xref[:, 1], nrm2, "LinearSolve, second b")
    assert cache.A is dA and np.array_equal(dA.cpu().numpy(), A)                       # cache.A is NOT overwritten
    A2 = np.asfortranarray(A + np.eye(n))
    dA2 = to_dev_cm(A2)
    cache.A = dA2
    assert cache.isfresh
    sol = LS.solve_(cache)
    assert sol.retcode is LS.ReturnCode.Success and cache.nfactor == 2
    check_float64_quality(A2, b2, sol.u.cpu().numpy(), np.linalg.solve(A2, b2), np.linalg.norm(A2, 2), "LinearSolve, new A")
    assert np.array_equal(dA2.cpu().numpy(), A2)
