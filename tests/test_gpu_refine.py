"""-m gpu: rflu_gerfs_* / rflu_berr_* (csrc/refine.hip, gerfs_dev of csrc/driver.cpp) on random inputs, and the Python functions above them.

  * berr: final berr[k] <= 2 BERR_REF u (tests/refine_cases.py: the reference's own worst, LAPACK's gesvx included; the margin 2
    because one step more or less moves a stagnating berr by a factor of that order); berr recomputed from the downloaded X in
    longdouble differs by at most 2 (n + 2) 2^-53 (1 + berr): the Float64 accumulation's own bound (n + 1 roundings of relative size
    2^-53 in each of r and w, one more for the quotient; derived, not measured);
  * ferr: the true forward error is at most ferr[k]; with wt recomputed from the downloaded X in longdouble and the explicit inverse in
    Float64, the device's ||x|| ferr over the true ||A^-1 diag(wt)||_inf lies in [1/3, 1 + 2 gap + 4 n eps] (Float32; gap: the
    restatement's own) and in [1/6, twice that] (Float64, whose |r| is itself rounding noise of at most (n + 1) u w: every weight is
    only fixed within a factor 2); ferr = NULL changes no bit of the rest;
  * structure, bit for bit: a column alone against the same column in passes of 9 and 17, padded leading dimensions, a pointer off the
    16-byte boundary, two runs, and a solve, an inverse, a condition estimate and a mixed solve after gerfs against a fresh handle;
  * special values and every argument error; the Python functions.
Measured figures are printed (pytest -s)."""
import ctypes

import numpy as np
import pytest
import scipy.linalg as sla
import torch

import cond_cases as C
import refine_cases as R
import recursivefactorization.jl_amd as rf
from gpu_util import handle, ptr, sfx, to_dev_cm
from recursivefactorization.jl_amd import _ffi
from refine_gpu import berr, gerfs, same, same_result

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
IDS = ["f64", "f32"]


def longdouble_rw(A, X, B):
    Al, Xl, Bl = (np.asarray(M, dtype=np.longdouble) for M in (A, X, B))
    return Bl - Al @ Xl, np.abs(Bl) + np.abs(Al) @ np.abs(Xl)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_random_inputs_berr_and_ferr(dtype):
    u, eps = R.uof(dtype), 2.0 * R.uof(dtype)
    worst_berr = worst_dev = worst_fe = 0.0
    lo, hi = np.inf, 0.0
    for family, n in R.RANDOM_INPUTS:
        c = R.random_input(family, n, dtype)
        ref = R.restated_random(family, n, dtype)
        g = gerfs(c.A, c.lu, c.ipiv, c.B, c.X_in, dtype)
        what = (family, n)
        assert g.info == 0 and g.intact, what
        print(f"{np.dtype(dtype).name} {family} {n}: berr/u {g.berr / u} steps {g.steps} ferr {g.ferr}")
        assert np.all(g.berr <= 2.0 * R.BERR_REF[dtype] * u), (what, g.berr / u)
        worst_berr = max(worst_berr, g.berr.max() / u)
        r, w = longdouble_rw(c.A, g.X, c.B)
        with np.errstate(invalid="ignore", divide="ignore"):
            be_l = np.where(w == 0, 0, np.abs(r) / w).max(axis=0).astype(np.float64)
        bound = 2.0 * (n + 2) * 2.0 ** -53 * (1.0 + g.berr)
        assert np.all(np.abs(be_l - g.berr) <= bound), (what, be_l, g.berr)
        worst_dev = max(worst_dev, float((np.abs(be_l - g.berr) / bound).max()))
        fe = R.true_forward_error(g.X, c.x_ref)
        assert np.all(fe <= g.ferr), (what, fe, g.ferr)
        worst_fe = max(worst_fe, float((fe / g.ferr).max()))
        xn = np.abs(g.X.astype(np.float64)).max(axis=0)
        for k in range(R.RANDOM_NRHS):
            wt = (np.abs(r[:, k]) + (n + 1) * np.longdouble(u) * w[:, k]).astype(np.float64)
            q = xn[k] * g.ferr[k] / R.weighted_inverse_norm(c.A, wt)
            gap = max(0.0, ref.est[k] / R.weighted_inverse_norm(c.A, ref.wt[:, k]) - 1.0)
            top = 1.0 + 2.0 * gap + 4.0 * n * eps
            if dtype == np.float32:
                assert 1.0 / 3.0 <= q <= top, (what, k, q, top)
            else:
                assert 1.0 / 6.0 <= q <= 2.0 * top, (what, k, q, top)
            lo, hi = min(lo, q), max(hi, q)
        g0 = gerfs(c.A, c.lu, c.ipiv, c.B, c.X_in, dtype, ferr=False)
        assert same_result(g, g0, ferr=False) and g0.ferr is None, what
    print(f"{np.dtype(dtype).name}: worst berr {worst_berr:.3f} u; |berr - longdouble| / bound {worst_dev:.3f}; true error / ferr {worst_fe:.3f}; "
          f"||x|| ferr / true weighted norm in [{lo:.3f}, {hi:.4f}]")


def test_float32_accurate_start_of_a_float64_system():
    for family, n in [("uniform", 257), ("graded", 513), ("hilbert", 65)]:
        c = R.random_input(family, n, np.float64)
        X32 = sla.lu_solve(sla.lu_factor(c.A.astype(np.float32)), c.B.astype(np.float32)).astype(np.float64)
        g = gerfs(c.A, c.lu, c.ipiv, c.B, X32, np.float64)
        assert np.all(g.steps >= 1) and np.all(g.berr <= 2.0 * R.BERR_REF[np.float64] * R.uof(np.float64)), (family, n, g.steps, g.berr)
        assert np.all(R.true_forward_error(g.X, c.x_ref) <= g.ferr)
        # max_iter = 1 stops a column that wanted more: the last iterate stays, berr is that iterate's
        g1 = gerfs(c.A, c.lu, c.ipiv, c.B, X32, np.float64, ferr=False, max_iter=1)
        assert np.all(g1.steps == 1) and same(g1.berr, berr(c.A, g1.X, c.B, np.float64)), (family, n, g1.steps)


def _wide_input(n, dtype, nrhs=17):
    """17 columns that need different numbers of steps: column k starts from LAPACK's solve scaled by 1 + (k % 3) 2^-9, and from the
    exact solution where k % 3 == 0"""
    c = R.random_input("uniform", n, dtype)
    rng = np.random.default_rng([5, n])
    x = rng.integers(-4, 5, size=(n, nrhs)).astype(np.float64)
    B = np.asfortranarray((c.A.astype(np.float64) @ x).astype(dtype))
    X = sla.lu_solve((c.lu, c.piv), B).astype(np.float64) * (1.0 + (np.arange(nrhs) % 3) * 2.0 ** -9)
    X[:, ::3] = x[:, ::3]
    return c, B, np.asfortranarray(X.astype(dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_structure_bit_for_bit(dtype):
    for n in (65, 513):
        c, B, X = _wide_input(n, dtype)
        full = gerfs(c.A, c.lu, c.ipiv, B, X, dtype)
        assert len(set(full.steps.tolist())) > 1, full.steps            # the columns of a pass really stop at different steps
        nine = gerfs(c.A, c.lu, c.ipiv, B[:, :9], X[:, :9], dtype)
        for k in (0, 5, 8, 16):
            one = gerfs(c.A, c.lu, c.ipiv, B[:, k:k + 1], X[:, k:k + 1], dtype)
            for other in ((full, nine) if k < 9 else (full,)):
                assert same(one.X[:, 0], other.X[:, k]) and one.berr[0] == other.berr[k] and one.ferr[0] == other.ferr[k] and one.steps[0] == other.steps[k], (n, k)
        padded = gerfs(c.A, c.lu, c.ipiv, B, X, dtype, pad=3)
        shifted = gerfs(c.A, c.lu, c.ipiv, B, X, dtype, pad=1, off=1)
        again = gerfs(c.A, c.lu, c.ipiv, B, X, dtype)
        for other in (padded, shifted, again):
            assert other.intact and same_result(full, other), n


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_handle_state_after_gerfs(dtype):
    n = 257
    c, B, X = _wide_input(n, dtype, 9)
    s = sfx(dtype)

    def others(h, first):
        if first:
            gerfs(c.A, c.lu, c.ipiv, B, X, dtype, h=h)
        out = []
        Fd, ip, Bd = to_dev_cm(c.lu), torch.from_numpy(c.ipiv.copy()).to("cuda:0"), to_dev_cm(B).clone()
        h.call(f"rflu_getrs_{s}_dev", n, 9, ptr(Fd), n, ptr(ip), ptr(Bd), Bd.stride(1))
        out.append(Bd.cpu().numpy())
        rc = ctypes.c_double(-1.0)
        h.call(f"rflu_gecon_{s}_dev", C.NORM_ONE, n, ptr(Fd), n, 1.0, ctypes.byref(rc))
        out.append(np.array([rc.value]))
        Fi, info = to_dev_cm(c.lu).clone(), ctypes.c_int64(-1)
        h.call(f"rflu_getri_{s}_dev", n, ptr(Fi), Fi.stride(1), ptr(ip), ctypes.byref(info))
        out.append(Fi.cpu().numpy())
        A64 = to_dev_cm(c.A.astype(np.float64))
        M = rf.lu_mixed(A64, handle=h)
        out.append(rf.ldiv_mixed(M, to_dev_cm(B.astype(np.float64)).clone(), handle=h).cpu().numpy())
        return out

    h1, h2 = _ffi.Handle(0), _ffi.Handle(0)
    try:
        for a, b in zip(others(h1, True), others(h2, False)):
            assert same(a, b)
    finally:
        h1.close()
        h2.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_special_values(dtype):
    n = 65
    c, B, X = _wide_input(n, dtype, 9)
    clean = gerfs(c.A, c.lu, c.ipiv, B, X, dtype)
    for which in ("X", "B"):
        Xn, Bn = X.copy(), B.copy()
        (Xn if which == "X" else Bn)[7, 4] = np.nan
        g = gerfs(c.A, c.lu, c.ipiv, Bn, Xn, dtype)
        keep = np.arange(9) != 4
        assert np.isnan(g.berr[4]) and np.isnan(g.ferr[4]) and g.steps[4] == 0, which
        assert same(g.X[:, 4], Xn[:, 4])
        assert same(g.X[:, keep], clean.X[:, keep]) and same(g.berr[keep], clean.berr[keep]) and same(g.ferr[keep], clean.ferr[keep]) and same(g.steps[keep], clean.steps[keep])
        assert np.isnan(berr(c.A, Xn, Bn, dtype)[4])
    # an exactly zero u_ii: info, nothing written
    Fz = np.array(c.lu)
    Fz[40, 40] = 0.0
    g = gerfs(c.A, Fz, c.ipiv, B, X, dtype)
    assert g.info == 41 and same(g.X, X) and np.all(np.isnan(g.berr)) and np.all(np.isnan(g.ferr)) and np.all(g.steps == -777)
    # b = 0 and x = 0
    Bz, Xz = B.copy(), X.copy()
    Bz[:, 2], Xz[:, 2] = 0.0, 0.0
    g = gerfs(c.A, c.lu, c.ipiv, Bz, Xz, dtype)
    assert g.berr[2] == 0.0 and g.ferr[2] == 0.0 and g.steps[2] == 0 and np.all(g.X[:, 2] == 0.0)
    # empty problems: success, the outputs of the nrhs columns are zeros
    g = gerfs(np.zeros((0, 0)), np.zeros((0, 0)), None, np.zeros((0, 3)), np.zeros((0, 3)), dtype)
    assert g.info == 0 and np.all(g.berr == 0.0) and np.all(g.ferr == 0.0) and np.all(g.steps == 0)
    g = gerfs(c.A, c.lu, c.ipiv, B[:, :0], X[:, :0], dtype)
    assert g.info == 0 and g.berr.size == 0
    assert berr(np.zeros((0, 0)), np.zeros((0, 2)), np.zeros((0, 2)), dtype).tolist() == [0.0, 0.0]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_argument_errors(dtype):
    n, nrhs = 5, 2
    h, s = handle(), sfx(dtype)
    td = torch.float64 if dtype == np.float64 else torch.float32
    M = torch.eye(n, dtype=td, device="cuda:0")
    V = torch.ones((nrhs, n), dtype=td, device="cuda:0")
    fe, be = np.zeros(nrhs), np.zeros(nrhs)
    st, info = np.zeros(nrhs, dtype=np.intc), ctypes.c_int64(0)
    P = lambda a: ctypes.c_void_p(a.ctypes.data)   # noqa: E731
    NULL = ctypes.c_void_p(0)
    good = [n, nrhs, ptr(M), n, ptr(M), n, NULL, ptr(V), n, ptr(V), n, P(fe), P(be), 5, P(st), ctypes.byref(info)]
    fn = getattr(h.lib, f"rflu_gerfs_{s}_dev")
    assert fn(h.ptr, *good) == 0
    for pos, val in [(0, -1), (1, -1), (3, n - 1), (5, n - 1), (8, n - 1), (10, n - 1), (12, NULL), (15, NULL), (2, NULL), (4, NULL), (7, NULL), (9, NULL)]:
        bad = list(good)
        bad[pos] = val
        assert fn(h.ptr, *bad) == 1, pos                                  # RFLU_ERR_ARG
        assert h.lib.rflu_last_error()
    bad = list(good)
    bad[0] = 65537                                                       # beyond the transposed chain with ferr: refused before anything is read
    bad[3] = bad[5] = bad[8] = bad[10] = 65537
    assert fn(h.ptr, *bad) == 1
    okb = [n, nrhs, ptr(M), n, ptr(V), n, ptr(V), n, P(be)]
    fb = getattr(h.lib, f"rflu_berr_{s}_dev")
    assert fb(h.ptr, *okb) == 0
    for pos, val in [(0, -1), (1, -1), (3, n - 1), (5, n - 1), (7, n - 1), (8, NULL), (2, NULL), (4, NULL), (6, NULL)]:
        bad = list(okb)
        bad[pos] = val
        assert fb(h.ptr, *bad) == 1, pos
    assert fn(None, *good) == 1


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_python_functions(dtype):
    n = 129
    c, B, X = _wide_input(n, dtype, 9)
    raw = gerfs(c.A, c.lu, c.ipiv, B, X, dtype)
    F = rf.LU(to_dev_cm(c.lu), torch.from_numpy(c.ipiv.copy()).to("cuda:0"), 0)
    Xt = to_dev_cm(X).clone()
    res = rf.refine_(F, to_dev_cm(c.A), to_dev_cm(B), Xt)
    assert same(Xt.cpu().numpy(), raw.X) and same(res.berr, raw.berr) and same(res.ferr, raw.ferr) and same(res.steps, raw.steps)
    Xn = X.copy()
    res = rf.refine_(rf.LU(np.asfortranarray(c.lu), c.ipiv, 0), c.A, B, Xn, ferr=False)
    assert same(Xn, raw.X) and same(res.berr, raw.berr) and res.ferr is None
    v = X[:, 3].copy()                                                    # a vector counts as one column
    res = rf.refine_(rf.LU(np.asfortranarray(c.lu), c.ipiv, 0), c.A, np.ascontiguousarray(B[:, 3]), v)
    assert same(v, raw.X[:, 3]) and res.berr[0] == raw.berr[3] and res.ferr[0] == raw.ferr[3]
    assert same(rf.backward_error(c.A, X, B), berr(c.A, X, B, dtype))
    assert same(rf.backward_error(to_dev_cm(c.A), to_dev_cm(X), to_dev_cm(B)), berr(c.A, X, B, dtype))
    Xs, res = rf.solve_refined(F, to_dev_cm(c.A), to_dev_cm(B))
    assert np.all(res.berr <= 2.0 * R.BERR_REF[dtype] * R.uof(dtype)) and same(res.berr, rf.backward_error(to_dev_cm(c.A), Xs, to_dev_cm(B)))
    Fz = np.array(c.lu)
    Fz[7, 7] = 0.0
    with pytest.raises(rf.SingularException):
        rf.refine_(rf.LU(np.asfortranarray(Fz), c.ipiv, 0), c.A, B, X.copy())
