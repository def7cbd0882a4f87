"""-m gpu: ldiv!(F', B) / ldiv!(transpose(F), B) -- the solve with the adjoint factorization (LAPACK getrs, trans = 'T') through the
public lu / lu_ / ldiv_ with rf.Adjoint, on the host entry, the column-major and the row-major device entries.

Bounds.  Residual and solution against NumPy: the project's own bounds for the forward solve (test_gpu_lu.py:
test_ldiv_cooperative_and_recursive_paths) -- A' has the norm and the condition number of A.  The same matrices were run through
scipy.linalg.lapack.dgetrs(..., trans=1) on the CPU: LAPACK's solution passes both bounds for every case with the seeds below
(worst residual 3.2e-6 of its bound, worst solution error 5.3e-11 against 1e-6).  rand + 10 I: the reference's bound, test/runtests.jl:126-128.
"""
import ctypes

import numpy as np
import pytest
import torch

import recursivefactorization.jl_amd as rf
from gpu_util import fill_uniform_cm, handle, ptr, to_dev_cm, to_dev_rm
from helpers import rand_matrix

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
# the (n, nrhs) grid of test_ldiv_cooperative_and_recursive_paths plus odd leading dimensions
GRID = [(129, 8), (1000, 9), (1001, 3), (3000, 1), (3000, 20), (4100, 64), (2000, 70), (1000, 33), (2100, 130), (300, 64), (4100, 400)]


def grid_case(n, nrhs):
    A = rand_matrix(n, n, seed=900 + n)
    B = rand_matrix(n, nrhs, seed=901 + n).copy(order="F")
    return A, B


@pytest.mark.parametrize("n,nrhs", GRID)
def test_adjoint_solve_against_numpy(n, nrhs):
    A, B = grid_case(n, nrhs)
    dF = rf.lu_(to_dev_cm(A), None, True)
    dB = to_dev_cm(B)
    out = rf.ldiv_(rf.Adjoint(dF), dB)
    assert out is dB
    X = dB.cpu().numpy()
    Xref = np.linalg.solve(A.T, B)
    scale = np.linalg.norm(A, 2) * np.linalg.norm(Xref) + np.linalg.norm(B)
    res = np.linalg.norm(A.T @ X - B)
    err = np.linalg.norm(X - Xref) / np.linalg.norm(Xref)
    print(f"n={n} nrhs={nrhs}: residual {res:.3e} (bound {1000 * n * EPS * scale:.3e}), solution error {err:.3e}")
    assert res < 1000 * n * EPS * scale
    assert err < 1e-6


@pytest.mark.parametrize("n,nrhs", GRID)
def test_adjoint_solve_agrees_with_factoring_the_transpose(n, nrhs):
    # a wrong direction of the interchanges survives a residual test on a diagonally dominant matrix; it does not survive this
    A, B = grid_case(n, nrhs)
    X = to_dev_cm(B)
    rf.ldiv_(rf.Adjoint(rf.lu(to_dev_cm(A))), X)
    Y = to_dev_cm(B)
    rf.ldiv_(rf.lu(to_dev_cm(np.asfortranarray(A.T))), Y)
    x, y = X.cpu().numpy(), Y.cpu().numpy()
    rel = np.linalg.norm(x - y) / np.linalg.norm(y)
    print(f"n={n} nrhs={nrhs}: |x - y| / |y| = {rel:.3e}")
    assert rel < 1e-6


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", [1, 8, 64, 65, 200, 300, 1000])
def test_adjoint_solve_step(dtype, n):
    eps = np.finfo(dtype).eps
    D = (rand_matrix(n, n, seed=600 + n, dtype=dtype) + dtype(10) * np.eye(n, dtype=dtype)).astype(dtype, order="F")
    Dt = D.astype(np.float64).T
    v = rand_matrix(n, 1, seed=700 + n, dtype=dtype)[:, 0].copy()
    B3 = rand_matrix(n, 3, seed=800 + n, dtype=dtype).copy(order="F")
    bound = 1000 * n * eps
    for pivot in (rf.NoPivot(), rf.RowMaximum()):
        nopiv = isinstance(pivot, rf.NoPivot)
        # host
        G = rf.lu(D, pivot)
        assert isinstance(G.ipiv, rf.NotIPIV) == nopiv
        x = rf.ldiv_(rf.Adjoint(G), v.copy())
        assert x.dtype == dtype and x.shape == (n,) and np.linalg.norm(Dt @ x - v) < bound
        X = rf.ldiv_(rf.Adjoint(G), B3.copy(order="F"))
        assert X.dtype == dtype and np.linalg.norm(Dt @ X - B3) < bound
        # device-resident, column-major
        dF = rf.lu_(to_dev_cm(D), None, pivot)
        assert isinstance(dF.ipiv, rf.NotIPIV) == nopiv
        dv = torch.from_numpy(v.copy()).to("cuda:0")
        rf.ldiv_(rf.Adjoint(dF), dv)
        assert np.linalg.norm(Dt @ dv.cpu().numpy() - v) < bound
        dB = to_dev_cm(B3)
        rf.ldiv_(rf.Adjoint(dF), dB)
        assert np.linalg.norm(Dt @ dB.cpu().numpy() - B3) < bound
        # device-resident, row-major factors and row-major right-hand sides
        rF = rf.lu_(to_dev_rm(D), None, pivot)
        rv = torch.from_numpy(v.copy()).to("cuda:0")
        rf.ldiv_(rf.Adjoint(rF), rv)
        assert np.linalg.norm(Dt @ rv.cpu().numpy() - v) < bound
        rB = to_dev_rm(B3)
        rf.ldiv_(rf.Adjoint(rF), rB)
        assert np.linalg.norm(Dt @ rB.cpu().numpy() - B3) < bound


def test_adjoint_solve_with_a_permutation_that_matters():
    n = 500
    D = rand_matrix(n, n, seed=4242) + 10.0 * np.eye(n)
    rows = np.random.default_rng(4243).permutation(n)
    A = np.asfortranarray(D[rows, :])
    B = rand_matrix(n, 3, seed=4244).copy(order="F")
    for F, X in ((rf.lu(A), B.copy(order="F")), (rf.lu_(to_dev_cm(A), None, True), to_dev_cm(B)), (rf.lu_(to_dev_rm(A), None, True), to_dev_rm(B))):
        ip = np.asarray(F.ipiv.cpu().numpy() if hasattr(F.ipiv, "cpu") else F.ipiv)
        assert np.count_nonzero(ip != np.arange(1, n + 1)) > n // 2
        rf.ldiv_(rf.Adjoint(F), X)
        x = X.cpu().numpy() if hasattr(X, "cpu") else X
        assert np.linalg.norm(A.T @ x - B) < 1000 * n * EPS


def test_strided_lda_through_the_raw_abi():
    """rflu_getrs_trans_f64_dev with lda = n + 3, ldb = n + 5 against lda = ldb = n: BIT FOR BIT.  The factors are read in place in
    both cases (no padded copy); a leading dimension that is not a multiple of 16 bytes only turns the 16-byte loads of a block into
    element loads of the same values, and every sum runs in the same order."""
    n, nrhs = 777, 5
    A = rand_matrix(n, n, seed=7771)
    B = rand_matrix(n, nrhs, seed=7772).copy(order="F")
    dF = rf.lu_(to_dev_cm(A), None, True)
    h = handle()
    X0 = to_dev_cm(B)
    h.call("rflu_getrs_trans_f64_dev", n, nrhs, ptr(dF.factors), n, ptr(dF.ipiv), ptr(X0), n)
    lda, ldb = n + 3, n + 5
    Fp = torch.full((n, lda), float("nan"), dtype=torch.float64, device="cuda:0")   # column j of F = row j of Fp
    Fp[:, :n] = dF.factors.T
    Bp = torch.full((nrhs, ldb), float("nan"), dtype=torch.float64, device="cuda:0")
    Bp[:, :n] = to_dev_cm(B).T
    h.call("rflu_getrs_trans_f64_dev", n, nrhs, ptr(Fp), lda, ptr(dF.ipiv), ptr(Bp), ldb)
    x0, x1 = X0.cpu().numpy(), Bp[:, :n].T.cpu().numpy()
    assert np.array_equal(x0, x1)
    assert bool(torch.isnan(Bp[:, n:]).all()) and bool(torch.isnan(Fp[:, n:]).all())   # the padding was neither read into the result nor written
    assert np.linalg.norm(x0 - np.linalg.solve(A.T, B)) / np.linalg.norm(x0) < 1e-6
    # an 8-byte aligned pointer that is not 16-byte aligned: the same matrix one element further on
    Fo = torch.empty(n * n + 1, dtype=torch.float64, device="cuda:0")
    Fo[1:] = dF.factors.T.reshape(-1)
    X2 = to_dev_cm(B)
    h.call("rflu_getrs_trans_f64_dev", n, nrhs, ctypes.c_void_p(Fo.data_ptr() + 8), n, ptr(dF.ipiv), ptr(X2), n)
    assert np.array_equal(x0, X2.cpu().numpy())


def test_errors_alias_and_the_forward_solve_afterwards():
    n = 700
    A = rand_matrix(n, n, seed=311)
    b = rand_matrix(n, 1, seed=312)[:, 0].copy()
    S = A.copy(order="F"); S[:, n // 2] = 0
    with pytest.raises(rf.SingularException):
        rf.ldiv_(rf.Adjoint(rf.lu(S, True, check=False)), b.copy())
    with pytest.raises(rf.SingularException):
        rf.ldiv_(rf.Adjoint(rf.lu_(to_dev_cm(S), None, True, check=False)), torch.from_numpy(b.copy()).to("cuda:0"))
    assert rf.Transpose is rf.Adjoint
    dF = rf.lu_(to_dev_cm(A), None, True)
    xa = torch.from_numpy(b.copy()).to("cuda:0"); rf.ldiv_(rf.Adjoint(dF), xa)
    xt = torch.from_numpy(b.copy()).to("cuda:0"); rf.ldiv_(rf.Transpose(dF), xt)
    assert torch.equal(xa, xt)
    # lu of a wrapped matrix hands back the wrapper ldiv_ takes (src/lu.jl:85-87): lu(A') \ b solves A' x = b
    W = rf.lu(rf.Adjoint(to_dev_cm(A)))
    assert isinstance(W, rf.Adjoint)
    xw = torch.from_numpy(b.copy()).to("cuda:0"); rf.ldiv_(W, xw)
    assert torch.equal(xa, xw)
    ref_t = np.linalg.solve(A.T, b)
    assert np.linalg.norm(xa.cpu().numpy() - ref_t) / np.linalg.norm(ref_t) < 1e-6
    # the exchange area and the tag counter are shared with the forward solve: narrow and wide passes of both, interleaved
    ref = np.linalg.solve(A, b)
    for _ in range(2):
        xf = torch.from_numpy(b.copy()).to("cuda:0"); rf.ldiv_(dF, xf)
        assert np.linalg.norm(xf.cpu().numpy() - ref) / np.linalg.norm(ref) < 1e-6
        B64 = rand_matrix(n, 64, seed=313).copy(order="F")
        Xt = to_dev_cm(B64); rf.ldiv_(rf.Adjoint(dF), Xt)
        Xf = to_dev_cm(B64); rf.ldiv_(dF, Xf)
        rt, rfw = np.linalg.solve(A.T, B64), np.linalg.solve(A, B64)
        assert np.linalg.norm(Xt.cpu().numpy() - rt) / np.linalg.norm(rt) < 1e-6
        assert np.linalg.norm(Xf.cpu().numpy() - rfw) / np.linalg.norm(rfw) < 1e-6
        xa2 = torch.from_numpy(b.copy()).to("cuda:0"); rf.ldiv_(rf.Adjoint(dF), xa2)
        assert torch.equal(xa, xa2)


@pytest.mark.parametrize("nrhs", [1, 64])
def test_adjoint_solve_n16384(nrhs):
    """The size the solve was tuned for; the factorization is served by the engine.  Residual bound of the first case, with
    Xref = numpy.linalg.solve(A', B) on the CPU.  ||A||_2 enters through a LOWER bound (twenty steps of the power iteration on A'A,
    ||A w|| / ||w||): the SVD of a 16384 x 16384 matrix takes minutes, and a smaller norm only tightens the bound."""
    n = 16384
    dA = fill_uniform_cm(n, np.float64, seed=12)
    A = dA.cpu().numpy()
    B = rand_matrix(n, nrhs, seed=16385).copy(order="F")
    dF = rf.lu_(dA, None, True)
    assert rf.last_path() == "hip-engine"
    dB = to_dev_cm(B)
    rf.ldiv_(rf.Adjoint(dF), dB)
    X = dB.cpu().numpy()
    Xref = np.linalg.solve(A.T, B)
    w = np.ones(n)
    for _ in range(20):
        w = A.T @ (A @ w)
        w /= np.linalg.norm(w)
    norm2_lower = np.linalg.norm(A @ w)
    scale = norm2_lower * np.linalg.norm(Xref) + np.linalg.norm(B)
    res = np.linalg.norm(A.T @ X - B)
    print(f"n={n} nrhs={nrhs}: residual {res:.3e} (bound {1000 * n * EPS * scale:.3e}), ||A||_2 >= {norm2_lower:.1f}")
    assert res < 1000 * n * EPS * scale
