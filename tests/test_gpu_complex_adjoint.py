"""ldiv!(transpose(F), B) and ldiv!(F', B) for ComplexF64 / ComplexF32 factors on the GPU (csrc/complex_solve.hip, DESIGN.md section
4.6): rflu_getrs_trans_cf64 / _cf32, their _dev forms and the Python functions on top, against op(A) in complex128.  Inputs, shapes,
bars and the CPU restatement come from tests/complex_solve_ref.py, which tests/test_complex_adjoint_glue.py holds to the same bars.
conj = 0 is the transpose (LAPACK 'T'), conj = 1 the adjoint ('C')."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import complex_ref as CR
import complex_solve_ref as SR
import gpu_util as G
import helpers
import oracle as O
import recursivefactorization.jl_amd as rf
from recursivefactorization.jl_amd import _ffi

pytestmark = pytest.mark.gpu

SFX = ["cf64", "cf32"]
CONJ = [0, 1]


def _null():
    return ctypes.c_void_p(0)


@functools.lru_cache(maxsize=None)
def _dev_factors(n, sfx):
    """The device's own pivoted factors of the random input: (column-major device tensor, device ipiv).  Made once, only read."""
    F = rf.lu_complex_(G.to_dev_cm(SR.rand_input(n, CR.CTYPES[sfx])))
    assert F.info == 0
    return F.factors, F.ipiv


def _trans_dev(sfx, dF, lda, dip, dB, ldb, n, nrhs, conj):
    G.handle().call(f"rflu_getrs_trans_{sfx}_dev", n, nrhs, G.ptr(dF), lda, G.ptr(dip) if dip is not None else _null(), G.ptr(dB), ldb, conj)


def _solve_packed(sfx, F, ipiv, B, conj):
    """Raw device entry on packed column-major copies of host factors / right-hand sides; the solution on the host."""
    n, nrhs = B.shape
    dF, dB = G.to_dev_cm(F), G.to_dev_cm(B)
    dip = torch.from_numpy(np.ascontiguousarray(ipiv)).to("cuda:0") if ipiv is not None else None
    _trans_dev(sfx, dF, max(n, 1), dip, dB, max(n, 1), n, nrhs, conj)
    return dB.cpu().numpy()


# ---- 1. backward error, device entry --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx", SFX)
@pytest.mark.parametrize("conj", CONJ)
@pytest.mark.parametrize("n", SR.BE_SIZES)
def test_backward_error_device_entry(sfx, conj, n):
    """||op(A) X - B||_inf / (||op(A)||_inf ||X||_inf) <= E = 20 n eps for every nrhs of the size: both paths, the narrow / wide boundary
    8 | 9, the leaf, split and CNB boundaries.  A 'T' / 'C' mix-up misses this bar by orders of magnitude on these inputs (the CPU test
    shows it on the restatement).  The test prints each ratio; the worst seen on an MI355X is in DESIGN.md section 4.6."""
    ct = CR.CTYPES[sfx]
    A = SR.rand_input(n, ct)
    dF, dip = _dev_factors(n, sfx)
    E = SR.bar_E(n, ct)
    for nrhs in SR.be_nrhs(n):
        B = CR.rand_rhs(n, nrhs, ct)
        dB = G.to_dev_cm(B)
        _trans_dev(sfx, dF, max(n, 1), dip, dB, max(n, 1), n, nrhs, conj)
        be = SR.backward_error(A, dB.cpu().numpy(), B, conj)
        print(f"{sfx} conj={conj} n={n} nrhs={nrhs}: backward error {be / E:.4f} E")
        assert be <= E, (n, nrhs, be, E)


# ---- 2. the reference's solve check through the Python functions ---------------------------------------------------------------------------
@pytest.mark.parametrize("sfx", SFX)
@pytest.mark.parametrize("conj", CONJ)
def test_reference_solve_check_through_python(sfx, conj):
    """test/runtests.jl:21-28 with op(A): b = op(A)[:, end], the solution ~ e_n with atol = 100 E (2-norm, as isapprox takes it), with
    NumPy arrays (host entry) and CUDA tensors (device entry)."""
    ct = CR.CTYPES[sfx]
    solve = rf.ldiv_complex_adjoint_ if conj else rf.ldiv_complex_transpose_
    for n in helpers.REF_SIZES:
        A = SR.rand_input(n, ct)
        E = SR.bar_E(n, ct)
        e = np.zeros(n)
        e[-1] = 1
        b = np.ascontiguousarray(SR.op(A, conj)[:, -1]).astype(ct)
        Fh = rf.lu_complex(A)
        xh = b.copy()
        assert solve(Fh, xh) is xh
        dF, dip = _dev_factors(n, sfx)
        db = torch.from_numpy(b.copy()).to("cuda:0")
        out = solve(rf.LU(dF, dip, 0), db)
        assert out is db
        xd = db.cpu().numpy()
        assert np.array_equal(CR.bits(xd), CR.bits(xh)), n          # both entries run the same kernels on the same factors
        for x in (xh, xd):
            if np.all(np.isfinite(x)):
                d = float(np.linalg.norm(x.astype(np.complex128) - e))
                print(f"{sfx} conj={conj} n={n}: |x - e_n| = {d / (100 * E):.5f} of the bar")
                assert d <= 100 * E, (n, d, E)
        # a matrix right-hand side through both entries: the host one is the device one between two copies
        B = CR.rand_rhs(n, 3, ct)
        Xh = solve(Fh, np.array(B, order="F"))
        Xd = solve(rf.LU(dF, dip, 0), G.to_dev_cm(B)).cpu().numpy()
        assert np.array_equal(CR.bits(Xh), CR.bits(Xd))
        assert SR.backward_error(A, Xh, B, conj) <= E


# ---- 3. NotIPIV ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx", SFX)
@pytest.mark.parametrize("conj", CONJ)
def test_notipiv(sfx, conj):
    """test/runtests.jl:70-84, 116-128: NoPivot factors of A + 10 I, ipiv = NULL, ||op(A) X - B||_2 < 1000 n eps."""
    ct = CR.CTYPES[sfx]
    solve = rf.ldiv_complex_adjoint_ if conj else rf.ldiv_complex_transpose_
    for n in SR.NOPIV_SIZES:
        A = SR.nopivot_input(n, ct)
        F = rf.lu_complex_(G.to_dev_cm(A), None, rf.NoPivot())
        assert isinstance(F.ipiv, rf.NotIPIV) and F.info == 0
        bar = 1000 * n * SR.eps_of(ct)
        for nrhs in SR.NOPIV_NRHS:
            B = SR.nopivot_rhs(n, nrhs, ct)
            dB = G.to_dev_cm(B)
            _trans_dev(sfx, F.factors, n, None, dB, n, n, nrhs, conj)
            X = dB.cpu().numpy()
            r = float(np.linalg.norm(SR.op(A, conj) @ X.astype(np.complex128) - B.astype(np.complex128)))
            print(f"{sfx} conj={conj} n={n} nrhs={nrhs}: NoPivot residual {r / bar:.5f} of the bar")
            assert r < bar, (n, nrhs, r, bar)
            X2 = solve(F, G.to_dev_cm(B)).cpu().numpy()            # the Python function passes NULL for NotIPIV
            assert np.array_equal(CR.bits(X2), CR.bits(X))


# ---- 4. exact input: order of the interchanges, conjugation ----------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx", SFX)
@pytest.mark.parametrize("nrhs", [3, 9])
def test_exact_input_order_of_interchanges_and_conjugation(sfx, nrhs):
    """A scaled permutation (n = 130, shift 37, entries unit * 2^e): every operation is exact in both precisions and any order, so the
    solution equals B[(i + 37) mod n] / A[i, (i + 37) mod n] under == (the divisor conjugated for 'C'; == does not tell the sign of a
    zero).  The factorization has 129 non-trivial interchanges with 37 distinct targets: undoing them first-to-last gives another X
    (shown on the restatement by the CPU test).  nrhs = 3 is the narrow path, 9 the wide one."""
    ct = CR.CTYPES[sfx]
    A = SR.exact_input(ct)
    F, ipiv, info = CR.complex_generic_lufact(A, True)
    assert info == 0
    B = SR.exact_rhs(nrhs, ct)
    out = {}
    for conj in CONJ:
        X = _solve_packed(sfx, F, ipiv, B, conj)
        want = SR.exact_solution(A, B, conj)
        assert np.array_equal(X, want), f"conj={conj}: {int(np.count_nonzero(X != want))} entries differ"
        out[conj] = X
    assert not np.array_equal(out[0], out[1])


# ---- 5. layout ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx", SFX)
@pytest.mark.parametrize("conj", CONJ)
@pytest.mark.parametrize("n", [65, 300])
def test_layout_unaligned_f_and_leading_dimensions(sfx, conj, n):
    """lda = n + 3, F one real word past a 16-byte boundary, ldb = n + 5: results BIT-IDENTICAL to the aligned, packed call; the rows
    n .. ld - 1 of F and B (sentinels) untouched, F byte-identical after the call."""
    ct = CR.CTYPES[sfx]
    real = CR.real_of(ct)
    dF, dip = _dev_factors(n, sfx)
    Fh = dF.cpu().numpy()
    lda, ldb = n + 3, n + 5
    for nrhs in (1, 8, 9, 33):
        B = CR.rand_rhs(n, nrhs, ct)
        dB = G.to_dev_cm(B)
        _trans_dev(sfx, dF, n, dip, dB, n, n, nrhs, conj)
        want = dB.cpu().numpy()
        # F: column c at real word 1 + 2 * c * lda
        fbuf = np.full(1 + 2 * n * lda + 3, -7.0, dtype=real)
        fv = fbuf[1:1 + 2 * n * lda].reshape(n, lda, 2)            # [column, row, part]
        fv[:, :n, 0] = Fh.real.T
        fv[:, :n, 1] = Fh.imag.T
        bbuf = np.full(2 * nrhs * ldb, -5.0, dtype=real)
        bv = bbuf.reshape(nrhs, ldb, 2)
        bv[:, :n, 0] = B.real.T
        bv[:, :n, 1] = B.imag.T
        dfb, dbb = torch.from_numpy(fbuf).to("cuda:0"), torch.from_numpy(bbuf).to("cuda:0")
        assert dfb.data_ptr() % 16 == 0 and dbb.data_ptr() % 16 == 0
        G.handle().call(f"rflu_getrs_trans_{sfx}_dev", n, nrhs, ctypes.c_void_p(dfb.data_ptr() + np.dtype(real).itemsize), lda, G.ptr(dip),
                        G.ptr(dbb), ldb, conj)
        assert np.array_equal(dfb.cpu().numpy().view(np.uint8), fbuf.view(np.uint8))          # F only read
        ob = dbb.cpu().numpy().reshape(nrhs, ldb, 2)
        assert np.all(ob[:, n:, :] == -5.0)
        got = (ob[:, :n, 0] + 1j * ob[:, :n, 1]).T.astype(ct)
        assert np.array_equal(CR.bits(got), CR.bits(want)), (n, nrhs)


# ---- 6. determinism and neighbours -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx", SFX)
def test_determinism_and_neighbours_on_the_same_handle(sfx):
    """Two calls on the same input are bit-identical, narrow and wide; a forward ldiv_complex_ and a real lu at n = 300 on the same
    handle right after a transposed solve give the bits they gave before it (the workspaces are shared)."""
    ct = CR.CTYPES[sfx]
    n = 300
    dF, dip = _dev_factors(n, sfx)
    LUf = rf.LU(dF, dip, 0)
    Bf = CR.rand_rhs(n, 5, ct)
    R = np.asfortranarray(O.np_uniform(n, n, 12, CR.real_of(ct)))

    def neighbours():
        fwd = rf.ldiv_complex_(LUf, G.to_dev_cm(Bf)).cpu().numpy()
        real = rf.lu(R, check=False)
        return CR.bits(fwd), real.factors.copy(), np.asarray(real.ipiv).copy()

    before = neighbours()
    for nrhs in (1, 8, 9, 130):
        B = CR.rand_rhs(n, nrhs, ct)
        for conj in CONJ:
            runs = []
            for _ in range(2):
                dB = G.to_dev_cm(B)
                _trans_dev(sfx, dF, n, dip, dB, n, n, nrhs, conj)
                runs.append(CR.bits(dB.cpu().numpy()))
            assert np.array_equal(runs[0], runs[1]), (nrhs, conj)
        after = neighbours()
        for x, y in zip(before, after):
            assert np.array_equal(x, y), nrhs


# ---- 7. singular U ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx", SFX)
@pytest.mark.parametrize("conj", CONJ)
def test_singular_u(sfx, conj):
    """Factors with one zeroed u_ii: RFLU_OK from the raw entries, Inf / NaN in the output; the Python functions look at F.info first."""
    ct = CR.CTYPES[sfx]
    solve = rf.ldiv_complex_adjoint_ if conj else rf.ldiv_complex_transpose_
    for n, k in ((130, 40), (300, 290)):
        dF, dip = _dev_factors(n, sfx)
        Fh = np.array(dF.cpu().numpy(), order="F")
        Fh[k, k] = 0
        ipiv = dip.cpu().numpy()
        for nrhs in (2, 9):
            X = _solve_packed(sfx, Fh, ipiv, CR.rand_rhs(n, nrhs, ct), conj)          # no exception: status RFLU_OK
            assert not np.all(np.isfinite(X)), (n, nrhs)
        with pytest.raises(rf.SingularException):
            solve(rf.LU(G.to_dev_cm(Fh), dip, k + 1), G.to_dev_cm(CR.rand_rhs(n, 2, ct)))


# ---- 8. argument rules, device and host entries ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx", SFX)
def test_argument_rules(sfx):
    h = G.handle()
    ct = CR.CTYPES[sfx]
    n = 8
    dA = G.to_dev_cm(SR.rand_input(n, ct))
    dB = G.to_dev_cm(CR.rand_rhs(n, 2, ct))
    dip = torch.arange(1, n + 1, dtype=torch.int64, device="cuda:0")
    Ah = np.array(SR.rand_input(n, ct), order="F")
    Bh = np.array(CR.rand_rhs(n, 2, ct), order="F")
    iph = np.arange(1, n + 1, dtype=np.int64)
    keep_dev = (dA.clone(), dB.clone())
    keep_h = Bh.copy()
    for entry, F, ip, B in ((f"rflu_getrs_trans_{sfx}_dev", G.ptr(dA), G.ptr(dip), G.ptr(dB)),
                            (f"rflu_getrs_trans_{sfx}", ctypes.c_void_p(Ah.ctypes.data), ctypes.c_void_p(iph.ctypes.data),
                             ctypes.c_void_p(Bh.ctypes.data))):
        bad = [(n, 2, F, n, ip, B, n, 2), (n, 2, F, n, ip, B, n, -1),          # conj
               (-1, 2, F, n, ip, B, n, 0), (n, -2, F, n, ip, B, n, 1),         # negative sizes
               (n, 2, F, n - 1, ip, B, n, 0), (n, 2, F, n, ip, B, n - 1, 1),   # lda < n, ldb < n
               (n, 2, _null(), n, ip, B, n, 0), (n, 2, F, n, ip, _null(), n, 1)]
        for args in bad:
            with pytest.raises(_ffi.RfluError, match=r"status 1: \S"):
                h.call(entry, *args)
        # a failing call leaves B as it was (the host entry copies back only on success)
        assert np.array_equal(CR.bits(Bh), CR.bits(keep_h))
        assert torch.equal(torch.view_as_real(dA), torch.view_as_real(keep_dev[0]))
        assert torch.equal(torch.view_as_real(dB), torch.view_as_real(keep_dev[1]))
    # zero sizes succeed and touch nothing
    sent = torch.full((16,), 7.0, dtype=dA.dtype, device="cuda:0")
    keep = sent.clone()
    sh = np.full(16, 7.0, dtype=ct)
    for conj in CONJ:
        h.call(f"rflu_getrs_trans_{sfx}_dev", 0, 3, G.ptr(sent), 1, G.ptr(dip), G.ptr(sent), 1, conj)
        h.call(f"rflu_getrs_trans_{sfx}_dev", 4, 0, G.ptr(sent), 4, G.ptr(dip), G.ptr(sent), 4, conj)
        h.call(f"rflu_getrs_trans_{sfx}", 0, 3, ctypes.c_void_p(sh.ctypes.data), 1, _null(), ctypes.c_void_p(sh.ctypes.data), 1, conj)
        h.call(f"rflu_getrs_trans_{sfx}", 4, 0, ctypes.c_void_p(sh.ctypes.data), 4, _null(), ctypes.c_void_p(sh.ctypes.data), 4, conj)
    assert torch.equal(torch.view_as_real(sent), torch.view_as_real(keep)) and np.all(sh == 7.0)
    assert torch.equal(dip, torch.arange(1, n + 1, dtype=torch.int64, device="cuda:0"))
