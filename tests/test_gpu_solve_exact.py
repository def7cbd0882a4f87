"""-m gpu: the real solves (rflu_getrs_*, rflu_getrs_rm_*, rflu_getrs_trans_*, rflu_getrs_trans_rm_* in Float64 and Float32) through the raw
C ABI, on factors that were NOT made on the GPU: a wrong answer here is a wrong solve.

(a)-(d) use the exact inputs of tests/solve_cases.py (proven on the host in tests/test_solve_cases.py): every correct solve returns
x_true bit for bit, so the assertion is np.array_equal.  (e) holds the solves of LAPACK's factors of uniform(0, 1) matrices to the
componentwise backward error
        omega = max_i |P b - L (U x)|_i / (|L| |U| |x| + |P b|)_i          (transposed: U^T, L^T and z = P x)
evaluated in numpy.longdouble on the rounded factors: omega <= n eps (the textbook bound for substitution, gamma_n per triangle, holds
for any blocking with exact block inverses up to a modest constant; 1000 times below the residual bound of test_gpu_lu.py), and
omega <= 16 max(omega_ref, eps / 8) with omega_ref from scipy.linalg.lu_solve on the same factors and right-hand sides.  On the CPU
omega_ref was 0.13 .. 0.27 eps and a restatement of the block-inverse method 0.12 .. 0.60 eps, at most 4.4 times LAPACK's; 16 leaves
a factor of four for the GPU's summation order, and the floor eps / 8 keeps a lucky omega_ref from tightening the bound.

The three device paths by number of right-hand sides (driver.cpp: getrs_rm / getrs_trans_view): "narrow" = trsv_chain_kernel in passes
of 8 columns (NR = 1 instantiation for a last pass of one column) up to 32, "wide" = trsm_chain_kernel in passes of 64 columns as two
chains of 32 up to 320 (any number beyond 32 in the transposed solve), "recursive" = TRSM / GEMM splitting beyond (forward only).

(c) Blocks that wrap around the workgroups: block r belongs to workgroup r mod G, G = min(ceil(n / 64), 256), so only n > 16384 gives a
workgroup of the narrow chain a second block (n = 16449: 258 blocks) and only n > 49152 a fourth (n = 49217: 770 blocks, the last one
partial).  Whether the WIDE chain wraps at n = 16449 depends on how many trsm_chain_kernel workgroups fit on a compute unit (its G is
min(blocks, workgroups per CU * CUs / chains)); nobody has measured that, so it is NOT KNOWN whether nrhs = 40 and 97 there wrap.

Measured on an MI355X (all 219 cases pass; the whole file takes 20 s, no case more than 0.8 s, most of it the longdouble products of (e)):
  * (a)-(d): every result equal to x_true bit for bit, no exception for any path, so no path is held to (e)'s bound instead.
  * the n = 49217 cases, the longest solves: 0.07 s (forward, row-major) and 0.05 s (transposed, column-major) per test, building the
    9.7 GB of factors on the device included; the four n = 16449 tests 0.03 .. 0.39 s.
  * (e), worst over both directions and both precisions, per path:
        narrow     omega / eps 1.77 (transposed Float32, n = 65, nrhs = 9)     omega / omega_ref 17.6 (transposed Float32, n = 65, nrhs = 1)
        wide       omega / eps 2.23 (transposed Float32, n = 65, nrhs = 65)    omega / omega_ref 5.46 (forward Float64, n = 129, nrhs = 33)
        recursive  omega / eps 0.29 (forward Float32, n = 300, nrhs = 321)     omega / omega_ref 1.01 (the same case)
    The one ratio above 16 is the case the floor is there for: omega_ref = 0.059 eps, a lucky LAPACK result below eps / 8, and
    omega = 1.05 eps against the bound 16 eps / 8 = 2 eps.  Second worst ratio of the narrow path: 10.3 (forward Float64, n = 129, nrhs = 1).
    omega_ref itself was 0.06 .. 0.60 eps on these cases.
"""
import functools

import numpy as np
import pytest
import scipy.linalg as sla
import torch

from gpu_util import handle, ptr, sfx, tdtype
from helpers import rand_matrix
from solve_cases import solve_case

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
# entry -> (symbol, transposed solve, row-major factors and right-hand sides)
ENTRIES = {
    "getrs": ("rflu_getrs_{s}_dev", False, False),
    "getrs_rm": ("rflu_getrs_rm_{s}_dev", False, True),
    "getrs_trans": ("rflu_getrs_trans_{s}_dev", True, False),
    "getrs_trans_rm": ("rflu_getrs_trans_rm_{s}_dev", True, True),
}
PATH_VARS = ("RFLU_TRSV_MAX_RHS", "RFLU_TRSM_CHAIN_MAX_RHS", "RFLU_TRSM_CHAIN_SPLIT")
NAN = float("nan")


def path_of(nrhs, trans):
    if nrhs <= 32:
        return "narrow"
    return "wide" if (trans or nrhs <= 320) else "recursive"


def default_paths(monkeypatch):
    for v in PATH_VARS:
        monkeypatch.delenv(v, raising=False)


def bits(t):
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


@functools.lru_cache(maxsize=None)
def exact_rhs(n, nrhs, trans):
    """(x_true, B) of the exact case (n, nrhs) as int64, made once and never written to."""
    case = solve_case(n, nrhs, seed=n)
    return case.x_true, (case.b_transposed() if trans else case.b_forward())


def solve(entry, dtype, n, nrhs, F, ld, ipiv, B, pad=3):
    """One call of `entry` on device factors F (leading dimension ld) and the host right-hand sides B (n x nrhs): B goes into a NaN
    filled device buffer with `pad` extra elements per row (row-major) or column (column-major).  Returns (X as numpy, padding still NaN)."""
    sym, _, rm = ENTRIES[entry]
    Bh = torch.from_numpy(np.ascontiguousarray(B, dtype=dtype))
    if rm:
        ldb = nrhs + pad
        Bd = torch.full((n, ldb), NAN, dtype=tdtype(dtype), device="cuda:0")
        Bd[:, :nrhs] = Bh.to("cuda:0")
    else:
        ldb = n + pad
        Bd = torch.full((nrhs, ldb), NAN, dtype=tdtype(dtype), device="cuda:0")
        Bd[:, :n] = Bh.to("cuda:0").T
    handle().call(sym.format(s=sfx(dtype)), n, nrhs, ptr(F), ld, ptr(ipiv), ptr(Bd), ldb)
    if rm:
        return Bd[:, :nrhs].cpu().numpy(), (pad == 0 or bool(torch.isnan(Bd[:, nrhs:]).all()))
    return Bd[:, :n].T.cpu().numpy(), (pad == 0 or bool(torch.isnan(Bd[:, n:]).all()))


def explain(X, want):
    bad = np.argwhere(~((X == want) | (np.isnan(X) & np.isnan(want))))
    i, j = bad[0]
    return f"{len(bad)} of {want.size} elements differ, the first at (row {i}, column {j}): got {X[i, j]!r}, expected {want[i, j]!r}"


def exact_setup(entry, dtype, n, nrhs_max, pad=3):
    _, trans, rm = ENTRIES[entry]
    case = solve_case(n, nrhs_max, seed=n)
    ld = n + pad
    F = case.device_factors(tdtype(dtype), rm, ld, pad=NAN)
    ipiv = torch.from_numpy(case.ipiv).to("cuda:0")
    x_true, B = exact_rhs(n, nrhs_max, trans)
    return F, ld, ipiv, x_true, B, trans


# ---------------------------------------------------------------------------------------------------------------- (a) exact grid
GRID_N = [1, 2, 63, 64, 65, 127, 128, 129, 191, 257, 1000]
GRID_NRHS = [1, 2, 7, 8, 9, 16, 17, 31, 32, 33, 48, 63, 64, 65, 96, 97, 128, 129, 320, 321, 400]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("entry", list(ENTRIES))
@pytest.mark.parametrize("n", GRID_N)
def test_exact_grid(n, entry, dtype, monkeypatch):
    default_paths(monkeypatch)
    F, ld, ipiv, x_true, B, trans = exact_setup(entry, dtype, n, max(GRID_NRHS))
    F0, ipiv0 = F.clone(), ipiv.clone()
    for nrhs in GRID_NRHS:
        where = f"n={n} nrhs={nrhs} path={path_of(nrhs, trans)} entry={entry} {np.dtype(dtype).name}"
        X, pad_ok = solve(entry, dtype, n, nrhs, F, ld, ipiv, B[:, :nrhs], pad=3 if nrhs % 2 == 0 else 5)
        want = x_true[:, :nrhs].astype(dtype)
        assert X.dtype == want.dtype and X.shape == want.shape, where
        assert np.array_equal(X, want), f"{where}: {explain(X, want)}"
        assert pad_ok, f"{where}: the padding behind the right-hand sides was written"
        assert torch.equal(bits(F), bits(F0)), f"{where}: the factors (or their NaN padding) were written"
        assert torch.equal(ipiv, ipiv0), f"{where}: ipiv was written"


# ------------------------------------------------------------------------------------ (b) the three paths on the same input
FORCED = {   # path -> (RFLU_TRSV_MAX_RHS, RFLU_TRSM_CHAIN_MAX_RHS); None = the default
    "narrow": ("64", None),
    "wide": ("0", None),
    "recursive": ("0", "0"),
}


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("entry", ["getrs", "getrs_rm"])
@pytest.mark.parametrize("n", [65, 300, 1000])
def test_three_paths_same_input(n, entry, dtype, monkeypatch):
    """n: a partial second block; more than the 256 rows the fused strip kernel of the recursive path takes in one launch; several
    levels of its splitting.  (The transposed solve has no recursive path.)"""
    F, ld, ipiv, x_true, B, _ = exact_setup(entry, dtype, n, 64)
    for path, (trsv_max, chain_max) in FORCED.items():
        default_paths(monkeypatch)
        monkeypatch.setenv("RFLU_TRSV_MAX_RHS", trsv_max)
        if chain_max is not None:
            monkeypatch.setenv("RFLU_TRSM_CHAIN_MAX_RHS", chain_max)
        for nrhs in (1, 8, 9, 33, 64):
            X, pad_ok = solve(entry, dtype, n, nrhs, F, ld, ipiv, B[:, :nrhs])
            want = x_true[:, :nrhs].astype(dtype)
            where = f"n={n} nrhs={nrhs} forced path={path} entry={entry} {np.dtype(dtype).name}"
            assert np.array_equal(X, want), f"{where}: {explain(X, want)}"
            assert pad_ok, where


# ------------------------------------------------------------------------------ (c) blocks that wrap around the workgroups
def wrap_case(n, dtype, entry, nrhs_list, monkeypatch):
    default_paths(monkeypatch)
    _, trans, rm = ENTRIES[entry]
    case = solve_case(n, max(nrhs_list), seed=n)
    F = case.device_factors(tdtype(dtype), rm, n)   # read in place by both entries: no second n x n array anywhere
    ipiv = torch.from_numpy(case.ipiv).to("cuda:0")
    x_true, B = exact_rhs(n, max(nrhs_list), trans)
    check = int(bits(F).sum(dtype=torch.int64).item())
    try:
        for nrhs in nrhs_list:
            X, _ = solve(entry, dtype, n, nrhs, F, n, ipiv, B[:, :nrhs], pad=0)
            want = x_true[:, :nrhs].astype(dtype)
            where = f"n={n} nrhs={nrhs} path={path_of(nrhs, trans)} entry={entry} {np.dtype(dtype).name}"
            assert np.array_equal(X, want), f"{where}: {explain(X, want)}"
        assert int(bits(F).sum(dtype=torch.int64).item()) == check, "the factors were written"
    finally:
        del F
        torch.cuda.empty_cache()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("entry", ["getrs_rm", "getrs_trans"])
def test_second_block_per_workgroup_n16449(entry, dtype, monkeypatch):
    """258 blocks on 256 workgroups: workgroups 0 and 1 own two blocks each (bacc slot 1, ns += dir * G, one round of the far loop)."""
    wrap_case(16449, dtype, entry, [1, 9, 40, 97], monkeypatch)


@pytest.mark.parametrize("entry", ["getrs_rm", "getrs_trans"])
def test_all_four_slots_n49217_f32(entry, monkeypatch):
    """770 blocks on 256 workgroups: all four bacc slots, a partial last block; 9 right-hand sides = a pass of 8 and the NR = 1 pass.
    The factors (9.7 GB in Float32) are built on the device."""
    wrap_case(49217, np.float32, entry, [9], monkeypatch)


# ------------------------------------------------------------------------------------------------------ (d) column containment
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_nan_column_stays_in_its_column(entry, dtype, monkeypatch):
    default_paths(monkeypatch)
    n = 257
    F, ld, ipiv, x_true, B, trans = exact_setup(entry, dtype, n, 97)
    for nrhs in (8, 33, 64, 97):
        for j in (0, nrhs - 1):
            Bj = B[:, :nrhs].astype(dtype)
            Bj[:, j] = np.nan
            want = x_true[:, :nrhs].astype(dtype)
            want[:, j] = np.nan
            X, pad_ok = solve(entry, dtype, n, nrhs, F, ld, ipiv, Bj)
            where = f"n={n} nrhs={nrhs} NaN column {j} path={path_of(nrhs, trans)} entry={entry} {np.dtype(dtype).name}"
            assert np.isnan(X[:, j]).all(), f"{where}: column {j} is not all NaN"
            assert np.array_equal(X, want, equal_nan=True), f"{where}: {explain(X, want)}"
            assert pad_ok, where


# ------------------------------------------------------------------------- (e) rounding-level accuracy on general factors
LD = np.longdouble


@functools.lru_cache(maxsize=None)
def general_factors(n, dtype):
    """LAPACK getrf in `dtype` of a uniform(0, 1) matrix: (packed factors, 0-based pivots, perm with (P b)[i] = b[perm[i]], L, U in longdouble)."""
    A = rand_matrix(n, n, seed=5100 + n, dtype=dtype)
    lu, piv = sla.lu_factor(A)
    assert lu.dtype == dtype
    perm = np.arange(n)
    for k, t in enumerate(piv):
        perm[[k, t]] = perm[[t, k]]
    L = np.tril(lu, -1).astype(LD) + np.eye(n, dtype=LD)
    U = np.triu(lu).astype(LD)
    return np.asfortranarray(lu), piv, perm, L, U


def omega(n, dtype, trans, b, x):
    """Componentwise backward error of x as a solution with the ROUNDED factors, in longdouble."""
    assert np.finfo(LD).eps <= 2.0 ** -63, "numpy.longdouble is no wider than Float64 here: the reference needs an extended type"
    _, _, perm, L, U = general_factors(n, dtype)
    b, x = b.astype(LD), x.astype(LD)
    if not trans:
        pb = b[perm]
        num = np.abs(pb - L @ (U @ x))
        den = np.abs(L) @ (np.abs(U) @ np.abs(x)) + np.abs(pb)
    else:
        z = x[perm]
        num = np.abs(b - U.T @ (L.T @ z))
        den = np.abs(U.T) @ (np.abs(L.T) @ np.abs(z)) + np.abs(b)
    assert (den > 0).all()
    return float((num / den).max())


ROUNDING_CASES = [(n, nrhs) for n in (65, 129, 300, 700) for nrhs in (1, 8, 9, 33, 64, 65)] + [(300, 321)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("trans", [False, True], ids=["forward", "transposed"])
@pytest.mark.parametrize("n,nrhs", ROUNDING_CASES)
def test_rounding_level_backward_error(n, nrhs, trans, dtype, monkeypatch):
    default_paths(monkeypatch)
    eps = float(np.finfo(dtype).eps)
    lu, piv, _, _, _ = general_factors(n, dtype)
    B = rand_matrix(n, nrhs, seed=5200 + n + nrhs, dtype=dtype)
    entry = "getrs_trans" if trans else "getrs"
    F = torch.from_numpy(np.ascontiguousarray(lu.T)).to("cuda:0")   # row j of the tensor = column j of the factors
    ipiv = torch.from_numpy(piv.astype(np.int64) + 1).to("cuda:0")
    X, _ = solve(entry, dtype, n, nrhs, F, n, ipiv, B)
    Xref = sla.lu_solve((lu, piv), B, trans=1 if trans else 0)
    assert X.dtype == dtype and Xref.dtype == dtype
    w, wref = omega(n, dtype, trans, B, X), omega(n, dtype, trans, B, Xref)
    print(f"omega n={n} nrhs={nrhs} {'transposed' if trans else 'forward'} {np.dtype(dtype).name} path={path_of(nrhs, trans)}: "
          f"omega/eps = {w / eps:.3f}  omega/omega_ref = {w / wref:.3f}  (omega_ref/eps = {wref / eps:.3f})")
    assert np.isfinite(X).all()
    assert w <= n * eps
    assert w <= 16 * max(wref, eps / 8)


# --------------------------------------------------------------------------------------------------------------- (f) determinism
@pytest.mark.parametrize("trans,nrhs", [(False, 9), (False, 64), (False, 321), (True, 9), (True, 64)],
                         ids=["forward-narrow", "forward-wide", "forward-recursive", "transposed-narrow", "transposed-wide"])
def test_two_calls_give_the_same_bits(trans, nrhs, monkeypatch):
    default_paths(monkeypatch)
    n, dtype = 700, np.float64
    lu, piv, _, _, _ = general_factors(n, dtype)
    B = rand_matrix(n, nrhs, seed=5300 + nrhs, dtype=dtype)
    F = torch.from_numpy(np.ascontiguousarray(lu.T)).to("cuda:0")
    ipiv = torch.from_numpy(piv.astype(np.int64) + 1).to("cuda:0")
    entry = "getrs_trans" if trans else "getrs"
    X1, _ = solve(entry, dtype, n, nrhs, F, n, ipiv, B)
    X2, _ = solve(entry, dtype, n, nrhs, F, n, ipiv, B)
    assert np.isfinite(X1).all() and np.array_equal(X1, X2)
