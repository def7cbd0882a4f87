"""-m gpu: the complex solves -- ldiv!(F, B) ('N'), ldiv!(transpose(F), B) ('T') and ldiv!(F', B) ('C') in ComplexF64 and ComplexF32 --
through the raw C ABI, on factors that were NOT made on the GPU: a wrong answer here is a wrong solve.

Entries: rflu_getrs_{cf64,cf32}_dev ('N', column-major factors: always the wide path, the recursion on a row-major image),
rflu_getrs_trans_{cf64,cf32}_dev with conj = 0 / 1 ('T' / 'C': the narrow path up to 8 right-hand sides, the wide one beyond) and
rflu_mixed_solve_cf32_dev ('N' on ROW-major ComplexF32 factors, narrow up to 8 right-hand sides).  Every right-hand side goes into a
NaN-filled buffer with 3 extra elements per column, which must still be NaN afterwards; the factors (leading dimension n + 3, NaN
behind every column, so every other column of ComplexF32 factors sits off a 16-byte boundary) must be byte-identical after the call.

(a)-(d) use the exact inputs of tests/complex_solve_cases.py (proven on the host in tests/test_complex_solve_cases.py): every correct
solve returns x_true bit for bit in any order of summation, so the assertion is np.array_equal.  (e) holds the solves of LAPACK's
cgetrf / zgetrf factors of the random input to the componentwise backward error omega of complex_solve_cases.omega (numpy.clongdouble,
moduli, rounded factors):
    1. X is finite;
    2. omega <= 4 n eps: c = 4 from the standard model of complex arithmetic, complex_solve_cases.complex_c derives it (a complex
       product carries a relative error of at most sqrt(2) gamma_2, two triangles: 2 sqrt(2) n eps to first order);
    3. omega <= 16 max(omega_ref, eps / 8), omega_ref from scipy.linalg.lu_solve(trans = 0 / 1 / 2) on the same factors and right-hand
       sides.  On the CPU the restatements of the two device paths are at most 2.30 (narrow) and 3.40 (wide) times LAPACK
       (test_complex_solve_cases.py recomputes it); 16 = 4 * 3.40 rounded up to a power of two leaves the factor of four that
       tests/test_gpu_solve_exact.py allows the GPU's different summation order, the floor keeps a lucky omega_ref from tightening it.

Measured on an MI355X (all 303 cases pass; the whole file takes 38 s, no case more than 1.3 s, most of it the clongdouble products of (e)):
  * (a)-(d): every result equal to x_true bit for bit, no exception for any entry, operation, element type or path, so no path is
    held to (e)'s bound instead.
  * (e), worst over both element types, per path and operation (omega_ref itself was 0.037 .. 0.46 eps on these cases):
        narrow 'N'  omega / eps 0.27 (cf32 row-major, n = 65, nrhs = 8)   omega / omega_ref 1.82 (the same case)
        narrow 'T'  omega / eps 0.51 (cf64, n = 65, nrhs = 8)             omega / omega_ref 7.30 (cf32, n = 65, nrhs = 1)
        narrow 'C'  omega / eps 0.45 (cf32, n = 129, nrhs = 8)            omega / omega_ref 1.92 (the same case)
        wide   'N'  omega / eps 0.67 (cf64, n = 300, nrhs = 130)          omega / omega_ref 2.58 (cf64, n = 129, nrhs = 1)
        wide   'T'  omega / eps 0.59 (cf64, n = 65, nrhs = 33)            omega / omega_ref 2.91 (cf32, n = 700, nrhs = 9)
        wide   'C'  omega / eps 0.60 (cf32, n = 65, nrhs = 130)           omega / omega_ref 2.57 (the same case)
    The ratio 7.30 is the case the floor is there for: omega_ref = 0.062 eps, a lucky LAPACK result below eps / 8, and omega = 0.45 eps
    against the bound 16 eps / 8 = 2 eps.  Every other ratio is below 3.
  * mutations of the kernels in a scratch build (wrong numbers only), failing tests of test_gpu_complex.py + test_gpu_complex_adjoint.py
    (243 tests) / of this file (303): the odd-band tail of cgemv_sub_kernel<float, *> dropped 4 / 13; B not conjugated on the way out
    of the wide path 52 / 72; the r + 4 partner of phase 3 of ctrsv_block_kernel dropped 52 / 72; the last k of a partial K slab of
    cgemm_sub_kernel dropped 56 / 221.
"""
import ctypes
import functools

import numpy as np
import pytest
import scipy.linalg as sla
import torch

import complex_solve_cases as C
import gpu_util as G
import recursivefactorization.jl_amd as rf

pytestmark = pytest.mark.gpu

SFX = {np.complex128: "cf64", np.complex64: "cf32"}
TDTYPE = {np.complex128: torch.complex128, np.complex64: torch.complex64}
LAPACK_TRANS = {"N": 0, "T": 1, "C": 2}
NAN = complex(float("nan"), float("nan"))
PAD = 3
# (entry, operation, element type): every device entry in every instantiation
COMBOS = [(entry, trans, ctype) for ctype in C.CTYPES for entry, trans in (("getrs", "N"), ("getrs_trans", "T"), ("getrs_trans", "C"))]
COMBOS.append(("mixed_solve", "N", np.complex64))
COMBO_IDS = [f"{e}-{t}-{SFX[c]}" for e, t, c in COMBOS]


def path_of(entry, nrhs):
    return C.path_of(nrhs, column_major_forward=entry == "getrs")


def null():
    return ctypes.c_void_p(0)


def words(t):
    r = torch.view_as_real(t)
    return r.view(torch.int64 if r.dtype == torch.float64 else torch.int32)


def device_factors(entry, F, ld):
    """The packed factors F (n x n, any layout) on the device with leading dimension ld >= n and NaN in the padding: tensor row j is
    column j of F (column-major entries) or row j of F (rflu_mixed_solve_cf32_dev)."""
    n = F.shape[0]
    t = torch.full((n, ld), NAN, dtype=TDTYPE[F.dtype.type], device="cuda:0")
    src = np.ascontiguousarray(F if entry == "mixed_solve" else F.T)
    t[:, :n] = torch.from_numpy(src).to("cuda:0")
    return t


def solve(entry, trans, ctype, n, nrhs, dF, ld, dip, B):
    """One call of the entry on device factors dF and the host right-hand sides B (n x nrhs).  Returns (X as numpy, padding still NaN)."""
    ldb = n + PAD
    Bd = torch.full((nrhs, ldb), NAN, dtype=TDTYPE[ctype], device="cuda:0")
    Bd[:, :n] = torch.from_numpy(np.ascontiguousarray(np.asarray(B, dtype=ctype).T)).to("cuda:0")
    ip = G.ptr(dip) if dip is not None else null()
    h = G.handle()
    if entry == "getrs":
        h.call(f"rflu_getrs_{SFX[ctype]}_dev", n, nrhs, G.ptr(dF), ld, ip, G.ptr(Bd), ldb)
    elif entry == "getrs_trans":
        h.call(f"rflu_getrs_trans_{SFX[ctype]}_dev", n, nrhs, G.ptr(dF), ld, ip, G.ptr(Bd), ldb, 1 if trans == "C" else 0)
    else:
        assert ctype == np.complex64 and trans == "N"
        h.call("rflu_mixed_solve_cf32_dev", n, nrhs, G.ptr(dF), ld, ip, G.ptr(Bd), ldb)
    pad = torch.view_as_real(Bd[:, n:])
    return Bd[:, :n].T.cpu().numpy(), bool(torch.isnan(pad).all())


def explain(X, want):
    bad = np.argwhere(~((X == want) | (np.isnan(X) & np.isnan(want))))
    i, j = bad[0]
    return f"{len(bad)} of {want.size} elements differ, the first at (row {i}, column {j}): got {X[i, j]!r}, expected {want[i, j]!r}"


def exact_setup(entry, trans, ctype, n):
    c = C.case(n)
    ld = n + PAD
    dF = device_factors(entry, C.factors_cm(c, ctype), ld)
    dip = torch.from_numpy(np.array(c.ipiv)).to("cuda:0")
    return c, dF, ld, dip, C.rhs(c, trans), c.X.astype(ctype)


# ---------------------------------------------------------------------------------------------------------------- (a) exact grid
@pytest.mark.parametrize("entry,trans,ctype", COMBOS, ids=COMBO_IDS)
@pytest.mark.parametrize("n", C.GRID_N)
def test_exact_grid(n, entry, trans, ctype):
    c, dF, ld, dip, B, x_true = exact_setup(entry, trans, ctype, n)
    F0, ip0 = dF.clone(), dip.clone()
    for nrhs in C.GRID_NRHS:
        where = f"n={n} nrhs={nrhs} path={path_of(entry, nrhs)} entry={entry} op={trans} {SFX[ctype]}"
        X, pad_ok = solve(entry, trans, ctype, n, nrhs, dF, ld, dip, B[:, :nrhs])
        want = x_true[:, :nrhs]
        assert X.dtype == want.dtype and X.shape == want.shape, where
        assert np.array_equal(X, want), f"{where}: {explain(X, want)}"
        assert pad_ok, f"{where}: the padding behind the right-hand sides was written"
        assert torch.equal(words(dF), words(F0)), f"{where}: the factors (or their NaN padding) were written"
        assert torch.equal(dip, ip0), f"{where}: ipiv was written"


# -------------------------------------------------------------------------------------------------------------------- (b) NotIPIV
@pytest.mark.parametrize("entry,trans,ctype", COMBOS, ids=COMBO_IDS)
def test_notipiv(entry, trans, ctype):
    """ipiv = NULL.  'N': the right-hand side is the exact one with the interchanges already applied, P B, and the result x_true.
    'T' / 'C': the interchanges would come last, so the result is P x_true."""
    n = 257
    c, dF, ld, _, B, x_true = exact_setup(entry, trans, ctype, n)
    for nrhs in (3, 9):
        Bn = C.apply_p(c, B[:, :nrhs]) if trans == "N" else B[:, :nrhs]
        want = x_true[:, :nrhs] if trans == "N" else C.apply_p(c, x_true[:, :nrhs])
        X, pad_ok = solve(entry, trans, ctype, n, nrhs, dF, ld, None, Bn)
        where = f"NotIPIV n={n} nrhs={nrhs} entry={entry} op={trans} {SFX[ctype]}"
        assert np.array_equal(X, want), f"{where}: {explain(X, want)}"
        assert pad_ok, where


# ---------------------------------------------------------------------------------------------------------- (c) column containment
@pytest.mark.parametrize("entry,trans,ctype", COMBOS, ids=COMBO_IDS)
def test_nan_column_stays_in_its_column(entry, trans, ctype):
    n = 257
    c, dF, ld, dip, B, x_true = exact_setup(entry, trans, ctype, n)
    for nrhs in (8, 9, 33, 64, 130):
        for j in (0, nrhs - 1):
            for part in ("real", "imag"):
                Bj = B[:, :nrhs].astype(ctype)
                getattr(Bj, part)[:, j] = np.nan
                want = x_true[:, :nrhs].copy()
                want[:, j] = np.nan
                X, pad_ok = solve(entry, trans, ctype, n, nrhs, dF, ld, dip, Bj)
                where = f"n={n} nrhs={nrhs} NaN in the {part} part of column {j} path={path_of(entry, nrhs)} entry={entry} op={trans} {SFX[ctype]}"
                assert np.isnan(X[:, j]).all(), f"{where}: column {j} is not all NaN"
                keep = np.arange(nrhs) != j
                assert np.array_equal(X[:, keep], want[:, keep]), f"{where}: {explain(X[:, keep], want[:, keep])}"
                assert pad_ok, where


# ----------------------------------------------------------------------------------------- (d) host entries and Python functions
@pytest.mark.parametrize("ctype", C.CTYPES, ids=["cf64", "cf32"])
def test_host_entries_and_python_functions(ctype):
    """rflu_getrs_cf* / rflu_getrs_trans_cf* on host pointers, and ldiv_complex_ / ldiv_complex_transpose_ / ldiv_complex_adjoint_ on an
    LU built from the constructed factors, with NumPy arrays (host entry) and CUDA tensors (device entry)."""
    n = 257
    c = C.case(n)
    F = np.array(C.factors_cm(c, ctype), order="F")
    ipiv = np.array(c.ipiv)
    sfx = SFX[ctype]
    python = {"N": rf.ldiv_complex_, "T": rf.ldiv_complex_transpose_, "C": rf.ldiv_complex_adjoint_}
    dlu = rf.LU(G.to_dev_cm(F), torch.from_numpy(ipiv).to("cuda:0"), 0)
    hlu = rf.LU(F, ipiv, 0)
    F0 = F.copy(order="F")
    for trans in C.TRANS:
        for nrhs in (8, 9):
            want = c.X[:, :nrhs].astype(ctype)
            B = np.array(C.rhs(c, trans)[:, :nrhs].astype(ctype), order="F")
            where = f"n={n} nrhs={nrhs} op={trans} {sfx}"
            Bh = B.copy(order="F")
            args = (n, nrhs, ctypes.c_void_p(F.ctypes.data), n, ctypes.c_void_p(ipiv.ctypes.data), ctypes.c_void_p(Bh.ctypes.data), n)
            if trans == "N":
                G.handle().call(f"rflu_getrs_{sfx}", *args)
            else:
                G.handle().call(f"rflu_getrs_trans_{sfx}", *args, 1 if trans == "C" else 0)
            assert np.array_equal(Bh, want), f"host entry {where}: {explain(Bh, want)}"
            Bp = B.copy(order="F")
            assert python[trans](hlu, Bp) is Bp
            assert np.array_equal(Bp, want), f"{python[trans].__name__} on NumPy arrays {where}: {explain(Bp, want)}"
            dB = G.to_dev_cm(B)
            assert python[trans](dlu, dB) is dB
            Xd = dB.cpu().numpy()
            assert np.array_equal(Xd, want), f"{python[trans].__name__} on CUDA tensors {where}: {explain(Xd, want)}"
    assert np.array_equal(F.T.view(np.uint8), F0.T.view(np.uint8)), "the host factors were written"


# ------------------------------------------------------------------------------ (e) rounding-level accuracy on general factors
@functools.lru_cache(maxsize=None)
def general_device_factors(entry, n, ctype):
    lu, piv, _ = C.general_factors(n, ctype)
    return device_factors(entry, lu, n), torch.from_numpy(piv.astype(np.int64) + 1).to("cuda:0")


@functools.lru_cache(maxsize=None)
def reference_omegas(n, ctype, trans):
    """omega of scipy.linalg.lu_solve per column of the widest block (a narrower block is its first columns), computed once"""
    lu, piv, perm = C.general_factors(n, ctype)
    B = C.rand_rhs(n, C.NRHS_MAX, ctype)
    Xref = sla.lu_solve((lu, piv), B, trans=LAPACK_TRANS[trans], check_finite=False)
    assert Xref.dtype == np.dtype(ctype)
    return C.omega(lu, perm, B, Xref, trans, per_column=True)


@pytest.mark.parametrize("entry,trans,ctype", COMBOS, ids=COMBO_IDS)
@pytest.mark.parametrize("n,nrhs", [(n, nrhs) for n in C.ROUNDING_N for nrhs in C.ROUNDING_NRHS])
def test_rounding_level_backward_error(n, nrhs, entry, trans, ctype):
    eps = C.eps_of(ctype)
    lu, piv, perm = C.general_factors(n, ctype)
    dF, dip = general_device_factors(entry, n, ctype)
    F0 = dF.clone()
    B = C.rand_rhs(n, nrhs, ctype)
    assert np.array_equal(B, C.rand_rhs(n, C.NRHS_MAX, ctype)[:, :nrhs])          # what reference_omegas relies on
    X, pad_ok = solve(entry, trans, ctype, n, nrhs, dF, n, dip, B)
    assert X.dtype == np.dtype(ctype)
    w, wref = C.omega(lu, perm, B, X, trans), float(reference_omegas(n, ctype, trans)[:nrhs].max())
    print(f"omega n={n} nrhs={nrhs} op={trans} {SFX[ctype]} entry={entry} path={path_of(entry, nrhs)}: "
          f"omega/eps = {w / eps:.3f}  omega/omega_ref = {w / wref:.3f}  (omega_ref/eps = {wref / eps:.3f})")
    assert np.isfinite(X).all()
    assert pad_ok
    assert torch.equal(words(dF), words(F0))
    assert w <= C.complex_c(n) * eps
    assert w <= C.M_RATIO * max(wref, eps / 8)
