"""-m gpu: the batched ComplexF64 / ComplexF32 inverse (rflu_getri_batched_cf64_dev / _cf32_dev, cgetri_batched_kernel of
csrc/batched_complex.hip) through inv_complex_batched and the raw C ABI.

Inputs, the CPU restatement of the kernel and the bars: tests/complex_batched_inv_cases.py; that the restatement alone stays far inside
the bar on every input used here is checked on the CPU in tests/test_complex_batched_inv_cases.py.
Bars.  Residual: complex_inv_cases.rho against op(A_b) in complex128, the larger of the right and the left one, <= rho_bar(n) (1.0 for
n >= 4, 4.0 for n <= 3).  The 'T' and 'C' results equal the transposed / conjugate-transposed 'N' result element for element (the
arithmetic is the same, only the store differs); the exact cases come back by ==; info is exact.  The tests print each figure.
Measured on an MI355X: worst residual 1.03 at n = 1 (bar 4), 0.36 at n = 2, 0.14 at n = 7 and 8, at most 0.07 from n = 31 on (bar 1),
0.02 in the loop above the limits; against ldiv_complex_batched_ on an explicit identity the largest element-wise difference was 0."""
import ctypes

import numpy as np
import pytest
import torch

import complex_batched_cases as CB
import complex_batched_inv_cases as BI
import complex_inv_cases as CI
import complex_ref as CR
import recursivefactorization.jl_amd as rf
from gpu_util import handle, ptr
from recursivefactorization.jl_amd import _ffi

pytestmark = pytest.mark.gpu

SFX = ["cf64", "cf32"]
TDTYPE = {"cf64": torch.complex128, "cf32": torch.complex64}
NULL = ctypes.c_void_p(0)
TRANS = {"N": 0, "T": 1, "C": 2}
LAYOUTS = ("cm", "rm")


def dev_cm(A):
    """(batch, r, c) host array -> device tensor of that shape whose matrices are column-major (stride(1) == 1)."""
    return torch.from_numpy(np.array(np.transpose(A, (0, 2, 1)), order="C", copy=True)).to("cuda:0").transpose(1, 2)


def dev_rm(A):
    return torch.from_numpy(np.array(A, order="C", copy=True)).to("cuda:0")


DEV = {"cm": dev_cm, "rm": dev_rm}


def host(t):
    return t.cpu().numpy()


def same_bits(X, Y):
    X, Y = np.asarray(X), np.asarray(Y)
    return X.shape == Y.shape and X.dtype == Y.dtype and np.array_equal(CR.bits(X), CR.bits(Y))


def factor(sfx, n, batch, layout, A=None):
    A = CB.host_batch(n, n, sfx, batch) if A is None else A
    return rf.lu_complex_batched_(DEV[layout](A), check=False)


def worst_of_batch(A, X, sfx, letter):
    return max(BI.worst_rho(A[b], X[b], sfx, letter) for b in range(A.shape[0]))


# ---- 1. residuals, the three letters from the store alone, both orientations ----------------------------------------------------------
RESIDUAL_CASES = ([(s, n, BI.BATCH) for s in SFX for n in BI.SIZES[s]]
                  + [(s, n, b) for s in SFX for n in BI.SMALL_BATCH_SIZES for b in BI.SMALL_BATCHES])


@pytest.mark.parametrize("sfx,n,batch", RESIDUAL_CASES)
def test_residuals_letters_and_orientations(sfx, n, batch):
    A = CB.host_batch(n, n, sfx, batch)
    for layout in LAYOUTS:
        F = factor(sfx, n, batch, layout)
        assert F.issuccess()
        before = F.factors.clone()
        X = {}
        for letter in BI.LETTERS:
            X[letter] = rf.inv_complex_batched(F, trans=letter)
            assert rf.last_path() == "hip-batched"
            assert X[letter].shape == (batch, n, n) and X[letter].dtype == TDTYPE[sfx] and X[letter].is_cuda
            assert X[letter].stride() == F.factors.stride(), (X[letter].stride(), F.factors.stride())
            assert not X[letter].is_conj()
            assert X[letter].data_ptr() != F.factors.data_ptr()
        assert torch.equal(F.factors, before)
        assert torch.equal(X["T"], X["N"].transpose(1, 2))
        assert torch.equal(X["C"], X["N"].transpose(1, 2).conj().resolve_conj())
        XA = rf.inv_complex_batched(rf.Adjoint(F))
        assert not XA.is_conj() and torch.equal(XA, X["C"])
        worst = {}
        for letter in BI.LETTERS:
            worst[letter] = worst_of_batch(A, host(X[letter]), sfx, letter)
        print(f"{sfx} n = {n} batch {batch} {layout}: worst rho " + " ".join(f"{k} {v:.4f}" for k, v in worst.items())
              + f" (bar {CI.rho_bar(n)})")
        for letter in BI.LETTERS:
            assert worst[letter] <= CI.rho_bar(n), (sfx, n, batch, layout, letter, worst[letter])


# ---- 2. exact inputs by == -------------------------------------------------------------------------------------------------------
def exact_lu(sfx, n, layout, copies=BI.EXACT_COPIES):
    F, ipiv, c = BI.exact_factors(n, sfx)
    fac = DEV[layout](np.stack([F] * copies))
    ip = torch.from_numpy(np.tile(ipiv, (copies, 1))).to("cuda:0")
    return rf.BatchedLU(fac, ip, torch.zeros(copies, dtype=torch.int64, device="cuda:0")), c


@pytest.mark.parametrize("sfx,n", [(s, n) for s in SFX for n in BI.EXACT_SIZES[s]])
def test_exact_cases_come_back_exactly(sfx, n):
    """Catches a reversed permutation, a conjugation in the wrong place and a swapped store branch: the three letters of an exact case
    are three different matrices (checked on the CPU)."""
    for layout in LAYOUTS:
        F, c = exact_lu(sfx, n, layout)
        for letter in BI.LETTERS:
            X = host(rf.inv_complex_batched(F, trans=letter))
            assert rf.last_path() == "hip-batched"
            want = BI.exact_inverse(c, sfx, letter)
            for b in range(BI.EXACT_COPIES):
                assert np.array_equal(X[b], want), (sfx, n, layout, letter, b, int(np.count_nonzero(X[b] != want)))


# ---- 3. a singular matrix stays alone ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx", SFX)
def test_a_singular_matrix_stays_alone(sfx):
    n, batch, bad, col = 33, BI.BATCH, 5, 7
    A = np.array(CB.host_batch(n, n, sfx, batch))
    A[bad][:, col] = 0
    for layout in LAYOUTS:
        F = factor(sfx, n, batch, layout, A)
        info = host(F.info)
        assert int(info[bad]) == col + 1 and not np.delete(info, bad).any()
        with pytest.raises(rf.SingularException) as ei:                       # from F.info, before anything is launched
            rf.inv_complex_batched(F)
        assert ei.value.info == col + 1 and ei.value.batch_index == bad
        G = rf.BatchedLU(F.factors, F.ipiv, torch.zeros_like(F.info))
        with pytest.raises(rf.SingularException) as ei:                       # from the library's own info
            rf.inv_complex_batched(G)
        assert ei.value.info == col + 1 and ei.value.batch_index == bad
        for letter in BI.LETTERS:
            X = host(rf.inv_complex_batched(F, trans=letter, check=False))
            assert not BI.finite(X[bad])
            keep = [b for b in range(batch) if b != bad]
            assert BI.finite(X[keep])
            w = max(BI.worst_rho(A[b], X[b], sfx, letter) for b in keep)
            assert w <= CI.rho_bar(n), (layout, letter, w)


@pytest.mark.parametrize("sfx", SFX)
def test_only_a_diagonal_entry_with_both_parts_zero_sets_info(sfx):
    n, b, i = 8, 2, 3
    for layout in LAYOUTS:
        for value, singular in ((1j, False), (2.0, False), (0.0, True)):
            F, _ = exact_lu(sfx, n, layout)
            F.factors[b, i, i] = value
            if singular:
                with pytest.raises(rf.SingularException) as ei:
                    rf.inv_complex_batched(F)
                assert ei.value.info == i + 1 and ei.value.batch_index == b
                X = host(rf.inv_complex_batched(F, check=False))
                assert not BI.finite(X[b]) and BI.finite(np.delete(X, b, axis=0))
            else:
                assert BI.finite(host(rf.inv_complex_batched(F)))


@pytest.mark.parametrize("sfx", SFX)
def test_a_nan_stays_in_its_own_matrix(sfx):
    n, batch, b = 33, BI.BATCH, 9
    for layout in LAYOUTS:
        F = factor(sfx, n, batch, layout)
        clean = host(rf.inv_complex_batched(F))
        F.factors[b, 20, 4] = complex(float("nan"), 0.0)
        X = host(rf.inv_complex_batched(F, check=False))
        assert not BI.finite(X[b])
        keep = [k for k in range(batch) if k != b]
        assert same_bits(X[keep], clean[keep])


# ---- 4. NotIPIV ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx,n", [(s, n) for s in SFX for n in BI.NOPIVOT_SIZES])
def test_notipiv(sfx, n):
    A = np.stack([CB.nopivot_matrix(n, sfx, b) for b in range(BI.NOPIVOT_BATCH)])
    for layout in LAYOUTS:
        F = rf.lu_complex_batched_(DEV[layout](A), None, rf.NoPivot(), check=False)
        assert isinstance(F.ipiv, rf.NotIPIV) and F.issuccess()
        for letter in BI.LETTERS:
            X = host(rf.inv_complex_batched(F, trans=letter))
            assert rf.last_path() == "hip-batched"
            w = worst_of_batch(A, X, sfx, letter)
            print(f"{sfx} n = {n} NoPivot {layout} {letter}: worst rho {w:.4f}")
            assert w <= CI.rho_bar(n), (layout, letter, w)


# ---- 5. order independence, determinism ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx,n", [("cf64", 33), ("cf64", 64), ("cf32", 32), ("cf32", 128)])
def test_order_independence_and_determinism(sfx, n):
    for layout in LAYOUTS:
        F = factor(sfx, n, BI.BATCH, layout)
        for letter in BI.LETTERS:
            X = host(rf.inv_complex_batched(F, trans=letter))
            assert same_bits(host(rf.inv_complex_batched(F, trans=letter)), X)          # two calls, the same bits
            for b in (0, 5, BI.BATCH - 1):                                              # alone as in the batch
                one = rf.BatchedLU(F.factors[b:b + 1], F.ipiv[b:b + 1], F.info[b:b + 1])
                assert same_bits(host(rf.inv_complex_batched(one, trans=letter))[0], X[b]), (layout, letter, b)


# ---- 6. the raw ABI: padded leading dimensions and strides ----------------------------------------------------------------------------
def strided(buf, batch, n, ld, stride, row_major):
    return buf.as_strided((batch, n, n), (stride, ld, 1) if row_major else (stride, 1, ld))


@pytest.mark.parametrize("sfx,n", [("cf64", 33), ("cf32", 65)])
def test_raw_abi_with_padding(sfx, n):
    batch = 7
    lda, ldi, sip = n + 3, n + 5, n + 2
    sF, sI = lda * n + 7, ldi * n + 11
    sentinel = complex(-7.5, 3.25)
    for row_major, layout in ((0, "cm"), (1, "rm")):
        F = factor(sfx, n, batch, layout)
        want = rf.inv_complex_batched(F)
        Fb = torch.zeros(batch * sF, dtype=TDTYPE[sfx], device="cuda:0")
        strided(Fb, batch, n, lda, sF, row_major).copy_(F.factors)
        ip = torch.zeros(batch * sip, dtype=torch.int64, device="cuda:0")
        ip.as_strided((batch, n), (sip, 1)).copy_(F.ipiv)
        for letter in BI.LETTERS:
            Xb = torch.full((batch * sI,), sentinel, dtype=TDTYPE[sfx], device="cuda:0")
            info = torch.full((batch,), -1, dtype=torch.int64, device="cuda:0")
            handle().call(f"rflu_getri_batched_{sfx}_dev", batch, n, ptr(Fb), lda, sF, row_major, ptr(ip), sip, ptr(Xb), ldi, sI,
                          TRANS[letter], ptr(info))
            assert handle().last_path() == _ffi.PATH_HIP_BATCHED
            assert not host(info).any()
            got = strided(Xb, batch, n, ldi, sI, row_major)
            ref = rf.inv_complex_batched(F, trans=letter)
            assert torch.equal(got, ref), (layout, letter)
            outside = torch.ones(batch * sI, dtype=torch.bool, device="cuda:0")
            strided(outside, batch, n, ldi, sI, row_major).fill_(False)
            assert bool((Xb[outside] == sentinel).all()), "an element outside the n x n outputs was written"
        assert torch.equal(rf.inv_complex_batched(F), want)


# ---- 7. agreement with the existing route ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx,n", [("cf64", 8), ("cf64", 33), ("cf64", 64), ("cf32", 33), ("cf32", 128)])
def test_agreement_with_ldiv_on_an_explicit_identity(sfx, n):
    """The same inputs through ldiv_complex_batched_ on an identity tensor meet the same bar.  Two kernels: no bit-for-bit claim."""
    batch = BI.BATCH
    A = CB.host_batch(n, n, sfx, batch)
    for layout in LAYOUTS:
        F = factor(sfx, n, batch, layout)
        X = host(rf.inv_complex_batched(F))
        eye = np.broadcast_to(np.eye(n, dtype=BI.CTYPES[sfx]), (batch, n, n))
        Y = host(rf.ldiv_complex_batched_(F, DEV[layout](eye)))
        wx, wy = worst_of_batch(A, X, sfx, "N"), worst_of_batch(A, Y, sfx, "N")
        diff = float(np.abs(X - Y).max())
        print(f"{sfx} n = {n} {layout}: rho inv_complex_batched {wx:.4f}, ldiv on I {wy:.4f}, largest element-wise difference {diff:.3e} "
              f"(largest |x| {float(np.abs(X).max()):.3e})")
        assert wx <= CI.rho_bar(n) and wy <= CI.rho_bar(n)


# ---- 8. the loop above the limits ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx", SFX)
def test_loop_above_the_limit(sfx):
    n, batch = BI.FALLBACK[sfx], BI.FALLBACK_BATCH
    A = CB.host_batch(n, n, sfx, batch)
    F = factor(sfx, n, batch, "cm")
    assert F.issuccess()
    before = F.factors.clone()
    for letter in BI.LETTERS:
        X = torch.empty((batch, n, n), dtype=TDTYPE[sfx], device="cuda:0").transpose(1, 2)
        info = torch.full((batch,), -1, dtype=torch.int64, device="cuda:0")
        handle().call(f"rflu_getri_batched_{sfx}_dev", batch, n, ptr(F.factors), n, n * n, 0, ptr(F.ipiv), n, ptr(X), n, n * n,
                      TRANS[letter], ptr(info))
        assert not host(info).any()
        assert torch.equal(rf.inv_complex_batched(F, trans=letter), X)
        w = worst_of_batch(A, host(X), sfx, letter)
        print(f"{sfx} n = {n} loop {letter}: worst rho {w:.4f}")
        assert w <= CI.rho_bar(n), (letter, w)
    assert torch.equal(F.factors, before)
    # one singular matrix: its info, a non-finite output of its own
    S = np.array(A)
    S[1][:, 4] = 0
    G = factor(sfx, n, batch, "cm", S)
    assert host(G.info).tolist() == [0, 5, 0]
    for letter in BI.LETTERS:
        with pytest.raises(rf.SingularException) as ei:
            rf.inv_complex_batched(rf.BatchedLU(G.factors, G.ipiv, torch.zeros_like(G.info)), trans=letter)
        assert ei.value.info == 5 and ei.value.batch_index == 1
        X = host(rf.inv_complex_batched(G, trans=letter, check=False))
        assert not BI.finite(X[1]) and BI.finite(X[[0, 2]])
        assert max(BI.worst_rho(S[b], X[b], sfx, letter) for b in (0, 2)) <= CI.rho_bar(n)
    # row-major above the limit is refused, in words
    R = rf.BatchedLU(dev_rm(A), F.ipiv, torch.zeros_like(F.info))
    with pytest.raises(_ffi.RfluError, match="column-major only"):
        rf.inv_complex_batched(R)


# ---- 9. the argument rules of the raw ABI ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx", SFX)
def test_argument_rules_of_the_raw_abi(sfx):
    n, batch = 8, 3
    F = factor(sfx, n, batch, "cm")
    X = torch.zeros((batch, n, n), dtype=TDTYPE[sfx], device="cuda:0")
    info = torch.zeros(batch, dtype=torch.int64, device="cuda:0")
    lib, h = _ffi.load(), handle()
    fn = getattr(lib, f"rflu_getri_batched_{sfx}_dev")

    def call(batch=batch, n=n, F_=ptr(F.factors), lda=n, sF=n * n, rm=0, ip=ptr(F.ipiv), sip=n, X_=ptr(X), ldi=n, sI=n * n, trans=0,
             info_=ptr(info)):
        return fn(h.ptr, batch, n, F_, lda, sF, rm, ip, sip, X_, ldi, sI, trans, info_)

    assert call() == 0
    assert call(ip=NULL) == 0                                                 # NotIPIV
    assert call(batch=0) == 0 and call(n=0) == 0                              # nothing to do
    assert call(batch=0, F_=NULL, X_=NULL, info_=NULL) == 0
    bad = [dict(batch=-1), dict(n=-1), dict(lda=n - 1), dict(ldi=n - 1), dict(sF=n * n - 1), dict(sI=n * n - 1), dict(sip=n - 1),
           dict(F_=NULL), dict(X_=NULL), dict(info_=NULL), dict(trans=3), dict(trans=-1)]
    for kw in bad:
        assert call(**kw) == 1, kw                                            # RFLU_ERR_ARG
        msg = lib.rflu_last_error()
        assert msg and b"getri_batched" in msg, (kw, msg)
    # a single matrix needs no stride
    assert call(batch=1, sF=0, sI=0, sip=0) == 0
