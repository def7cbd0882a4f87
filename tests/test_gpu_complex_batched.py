"""-m gpu: batched ComplexF64 / ComplexF32 LU and solve (rflu_getrf_batched_cf* / rflu_getrs_batched_cf*, csrc/batched_complex.hip)
through lu_complex_batched_ / ldiv_complex_batched_ and the raw C ABI.

Inputs and comparators: tests/complex_batched_cases.py (matrix b of a batch is rand_complex(m, n, ctype, seed0 = 12 + 37 b)); what the
bars below rest on is checked on the CPU in tests/test_complex_batched_cases.py.
Bars.  info equals the restatement's for every matrix.  ipiv equals it EXACTLY for ComplexF64 (no input sits on a pivot fork: the
smallest gap is 8e9 m eps) and follows the fork rule for ComplexF32.  Residual: the reference's own, test/runtests.jl:19-20:
||L U - A[p,:]||_inf < 20 m eps pivoted, < 10 sqrt(20 m eps) NoPivot (the restatement: at most 0.18 / 0.02 of them on these inputs).
max |l_ij| <= 1 + 4 eps with pivoting.  Solves: complex_solve_ref.backward_error <= 20 n eps against each letter's OWN operator (the
restatement: at most 0.03 of it).
Measured on an MI355X (the tests print each figure): worst residual 0.17 of 20 m eps pivoted (60 x 100, ComplexF32) and 0.017 of the
NoPivot bar (127 x 128); worst backward error 0.060 of 20 n eps at n = 1 and at most 0.0012 of it from n = 32 on, every letter and both
orientations; batched against single-matrix solve on the same factors: 0.9 .. 1.4 x the single path's own backward error."""
import ctypes

import numpy as np
import pytest
import torch

import complex_batched_cases as CB
import complex_ref as CR
import recursivefactorization.jl_amd as rf
from gpu_util import handle, ptr
from recursivefactorization.jl_amd import _ffi

pytestmark = pytest.mark.gpu

SFX = ["cf64", "cf32"]
CASES = [(sfx, shape, batch) for sfx in SFX for shape in CB.SHAPES[sfx] for batch in CB.BATCHES]
REAL_T = {"cf64": torch.float64, "cf32": torch.float32}
NULL = ctypes.c_void_p(0)


def dev_cm(A):
    """(batch, r, c) host array -> device tensor of that shape whose matrices are column-major (stride(1) == 1)."""
    return torch.from_numpy(np.array(np.transpose(A, (0, 2, 1)), order="C", copy=True)).to("cuda:0").transpose(1, 2)


def dev_rm(A):
    return torch.from_numpy(np.array(A, order="C", copy=True)).to("cuda:0")


def host(t):
    return t.cpu().numpy()


def same_bits(X, Y):
    return X.shape == Y.shape and X.dtype == Y.dtype and np.array_equal(CR.bits(X), CR.bits(Y))


def check_factorization(A, sfx, pivot, F, ip, info, ref, ref128=None):
    """The bars of the module docstring for one matrix; ``ref`` = the restatement's (factors, ipiv, info)."""
    m, n = A.shape
    mn, eps = min(m, n), CB.eps_of(sfx)
    _, ipr, infor = ref
    assert int(info) == infor, (int(info), infor)
    if pivot:
        if sfx == "cf64":
            assert np.array_equal(ip, ipr), f"ipiv differs first at step {int(np.flatnonzero(ip != ipr)[0])}"
        else:
            CB.check_ipiv_cf32(A, ip, ref128)
        assert np.abs(np.tril(F[:, :mn], -1)).max(initial=0.0) <= 1 + 4 * eps
    else:
        assert np.array_equal(ip, np.arange(1, mn + 1))
    if infor != 0:
        return float("nan")
    E = 20 * m * eps
    r = CR.residual_inf(A, F, ip)
    assert r < (E if pivot else 10 * np.sqrt(E)), (m, n, pivot, r, E)
    return r / (E if pivot else 10 * np.sqrt(E))


def check_batch(A, sfx, pivot, fac, ip, info):
    batch, m, n = A.shape
    worst = 0.0
    for b in range(batch):
        ref128 = CB.ref128_of_cf32(m, n, b) if (pivot and sfx == "cf32") else None
        worst = max(worst, check_factorization(A[b], sfx, pivot, fac[b], ip[b], info[b], CB.ref_factors(m, n, sfx, b, pivot), ref128))
    return worst


# ---- 1. factorization parity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx,shape,batch", CASES)
def test_factorization_parity_with_the_restatement(sfx, shape, batch):
    m, n = shape
    mn = min(m, n)
    A = CB.host_batch(m, n, sfx, batch)
    dA = dev_cm(A)
    F = rf.lu_complex_batched_(dA, check=False)
    assert rf.last_path() == "hip-batched"
    assert F.factors is dA and F.ipiv.shape == (batch, mn) and F.info.shape == (batch,) and F.info.is_cuda
    wp = check_batch(A, sfx, True, host(F.factors), host(F.ipiv), host(F.info))
    N = rf.lu_complex_batched_(dev_cm(A), None, rf.NoPivot(), check=False)
    assert rf.last_path() == "hip-batched" and isinstance(N.ipiv, rf.NotIPIV) and len(N.ipiv) == mn
    sign = -1 if rf.NOPIVOT_NEGATIVE_INFO else 1
    wn = check_batch(A, sfx, False, host(N.factors), np.tile(np.arange(1, mn + 1), (batch, 1)), sign * host(N.info))
    print(f"{sfx} {m}x{n} batch {batch}: worst residual {wp:.3f} of 20 m eps (pivoted), {wn:.4f} of 10 sqrt(20 m eps) (NoPivot)")
    # a poisoned user ipiv comes back as the identity with NoPivot (src/lu.jl:111-113), and the factors do not depend on it
    ipiv = torch.full((batch, mn), 2 ** 62, dtype=torch.int64, device="cuda:0")
    G = rf.lu_complex_batched_(dev_cm(A), ipiv, rf.Val(False), check=False)
    assert G.ipiv is ipiv and np.array_equal(host(ipiv), np.tile(np.arange(1, mn + 1), (batch, 1)))
    assert same_bits(host(G.factors), host(N.factors))


# ---- 2. exact inputs, bit for bit -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx,case", [(sfx, c) for c in CB.EXACT for sfx in c[2]])
def test_exact_inputs_bit_for_bit(sfx, case):
    """Every operation on these inputs is exact in both precisions and any order (complex_ref.exact_complex), so ipiv, info and every
    real and imaginary part of the factors equal the restatement's.  One exemption, asserted as such: a part that is a zero on BOTH
    sides may carry the other sign (the rule of test_gpu_complex.py::test_exact_inputs_tie_break_and_identical_factors)."""
    (m, n), empty, _, want = case
    E = CR.exact_complex(m, n, empty, CB.CTYPES[sfx])
    Fr, ipr, infor = CR.complex_generic_lufact(E, True)
    assert infor == want
    where = (1, 3, 4, 8)
    A = np.array(CB.host_batch(m, n, sfx, 9))
    A[list(where)] = E
    F = rf.lu_complex_batched_(dev_cm(A), check=False)
    fac, ip, info = host(F.factors), host(F.ipiv), host(F.info)
    for b in where:
        assert int(info[b]) == want
        assert np.array_equal(ip[b], ipr), f"matrix {b}: ipiv differs first at step {int(np.flatnonzero(ip[b] != ipr)[0])}"
        P, Pr = CR.parts(fac[b]), CR.parts(Fr)
        both_zero = (P == 0) & (Pr == 0)
        differ = CR.bits(P) != CR.bits(Pr)
        assert not np.any(differ & ~both_zero), f"matrix {b}: {int(np.count_nonzero(differ & ~both_zero))} parts differ in their bits"
    for b in set(range(9)) - set(where):
        assert int(info[b]) == 0


# ---- 3. special matrices inside one batch ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx,n", [("cf64", 32), ("cf64", 64), ("cf32", 32), ("cf32", 64), ("cf32", 128)])
def test_special_matrices_inside_one_batch(sfx, n):
    batch = 11
    base = CB.host_batch(n, n, sfx, batch)
    A = np.array(base)
    A[2][:, 7] = 0                                        # a zeroed column: info 8, the elimination continues
    A[4][n // 2 + 3, 2] = np.nan                          # a NaN below the diagonal: never chosen
    A[5] = 0                                              # nothing but zero pivots: info 1
    A[7] = CR.exact_complex(n, n, (), CB.CTYPES[sfx])     # every search a tie
    special = (2, 4, 5, 7)
    F = rf.lu_complex_batched_(dev_cm(A), check=False)
    F0 = rf.lu_complex_batched_(dev_cm(base), check=False)
    fac, ip, info = host(F.factors), host(F.ipiv), host(F.info)
    fac0, ip0, info0 = host(F0.factors), host(F0.ipiv), host(F0.info)
    for b in special:
        Fr, ipr, infor = CR.complex_generic_lufact(A[b], True)
        assert int(info[b]) == infor, f"special matrix {b}"
        if sfx == "cf64" or b in (5, 7):
            assert np.array_equal(ip[b], ipr), f"special matrix {b}"
        else:
            CB.check_ipiv_cf32(A[b], ip[b])
    assert info[2] == 8 and info[5] == 1 and info[4] == 0 and info[7] == 0
    assert np.all(np.isfinite(fac[2])) and CR.residual_inf(A[2], fac[2], ip[2]) < 20 * n * CB.eps_of(sfx)
    assert np.array_equal(ip[5], np.arange(1, n + 1)) and not np.any(fac[5])
    for b in range(batch):
        if b not in special:
            assert info[b] == 0 == info0[b] and np.array_equal(ip[b], ip0[b]) and same_bits(fac[b], fac0[b]), f"matrix {b} saw its neighbours"
    with pytest.raises(rf.SingularException) as ei:
        rf.lu_complex_batched_(dev_cm(A))
    assert ei.value.batch_index == 2 and ei.value.info == 8


# ---- 4. independence of order ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx,shape", [("cf64", (10, 12)), ("cf64", (64, 64)), ("cf32", (10, 12)), ("cf32", (64, 64)), ("cf32", (100, 60))])
def test_matrices_are_independent_of_their_order(sfx, shape):
    m, n = shape
    batch = max(CB.BATCHES)
    A = CB.host_batch(m, n, sfx, batch)
    perm = np.random.default_rng(7).permutation(batch)
    F = rf.lu_complex_batched_(dev_cm(A), check=False)
    G = rf.lu_complex_batched_(dev_cm(A[perm]), check=False)
    assert same_bits(host(G.factors), host(F.factors)[perm])
    assert np.array_equal(host(G.ipiv), host(F.ipiv)[perm]) and np.array_equal(host(G.info), host(F.info)[perm])
    if m == n:
        B = CB.rhs_batch(n, 9, sfx, batch)
        for trans in "NTC":
            X = host(rf.ldiv_complex_batched_(F, dev_cm(B), trans=trans))
            Y = host(rf.ldiv_complex_batched_(G, dev_cm(B[perm]), trans=trans))
            assert same_bits(Y, X[perm]), trans


# ---- 5. row-major batches and padding through the raw ABI -----------------------------------------------------------------------------
def _padded(img, lead, tail, fill=complex(float("nan"), float("nan"))):
    """(batch, cols, rows) memory images -> a (batch, stride) buffer with ld = rows + lead and `tail` elements between the matrices,
    everything else `fill`; returns (buffer, view of the images, ld, stride)."""
    batch, cols, rows = img.shape
    ld = rows + lead
    stride = ld * cols + tail
    buf = torch.full((batch, stride), fill, dtype=img.dtype, device="cuda:0")
    view = buf[:, :ld * cols].view(batch, cols, ld)
    view[:, :, :rows] = img
    return buf, view, ld, stride


def _untouched(buf, view, rows):
    pad = torch.view_as_real(view[:, :, rows:])
    tail = torch.view_as_real(buf[:, view.shape[1] * view.shape[2]:])
    return bool(torch.isnan(pad).all()) and bool(torch.isnan(tail).all())


@pytest.mark.parametrize("row_major", [1, 0])
@pytest.mark.parametrize("sfx,shape", [("cf64", (7, 9)), ("cf64", (50, 52)), ("cf64", (64, 64)), ("cf32", (7, 9)), ("cf32", (64, 64)),
                                       ("cf32", (100, 60)), ("cf32", (128, 128))])
def test_row_major_and_padding_through_the_raw_abi(sfx, shape, row_major):
    """lda = (contiguous dimension) + 3, strideA = lda * (other dimension) + 5, stride_ipiv = min(m, n) + 1, everything in between NaN /
    -7: the results equal the packed column-major call's bit for bit (the arithmetic happens in LDS, whatever the caller's layout), and
    the padding of A, ipiv and B comes back untouched."""
    m, n = shape
    batch, mn = 7, min(m, n)
    A = CB.host_batch(m, n, sfx, batch)
    h = handle()
    # the packed column-major call: the comparator (itself held to the restatement in test 1)
    packed = torch.from_numpy(np.array(np.transpose(A, (0, 2, 1)), order="C", copy=True)).to("cuda:0")   # (batch, n, m): column-major images
    ip0 = torch.zeros((batch, mn), dtype=torch.int64, device="cuda:0")
    info0 = torch.full((batch,), -1, dtype=torch.int64, device="cuda:0")
    h.call(f"rflu_getrf_batched_{sfx}_dev", batch, m, n, ptr(packed), m, m * n, 0, ptr(ip0), mn, 1, ptr(info0))
    assert h.last_path() == _ffi.PATH_HIP_BATCHED and bool((info0 == 0).all())
    fac0 = np.transpose(host(packed), (0, 2, 1))          # (batch, m, n)
    check_batch(A, sfx, True, fac0, host(ip0), host(info0))
    # the padded call in the orientation under test
    rows = n if row_major else m
    img = torch.from_numpy(np.array(A if row_major else np.transpose(A, (0, 2, 1)), order="C", copy=True)).to("cuda:0")
    buf, view, lda, stride = _padded(img, 3, 5)
    sip = mn + 1
    ip1 = torch.full((batch, sip), -7, dtype=torch.int64, device="cuda:0")
    info1 = torch.full((batch,), -1, dtype=torch.int64, device="cuda:0")
    h.call(f"rflu_getrf_batched_{sfx}_dev", batch, m, n, ptr(buf), lda, stride, row_major, ptr(ip1), sip, 1, ptr(info1))
    assert h.last_path() == _ffi.PATH_HIP_BATCHED
    fac1 = host(view[:, :, :rows])
    fac1 = fac1 if row_major else np.transpose(fac1, (0, 2, 1))
    assert same_bits(np.ascontiguousarray(fac1), np.ascontiguousarray(fac0))
    assert torch.equal(ip1[:, :mn], ip0) and torch.equal(info1, info0) and bool((ip1[:, mn:] == -7).all())
    assert _untouched(buf, view, rows)
    if m != n:
        return
    # the solve on the padded factors, B in their orientation with its own padding, against the packed column-major solve
    for nrhs in (1, 9):
        B = CB.rhs_batch(n, nrhs, sfx, batch)
        for trans, code in (("N", 0), ("T", 1), ("C", 2)):
            X0 = torch.from_numpy(np.array(np.transpose(B, (0, 2, 1)), order="C", copy=True)).to("cuda:0")   # (batch, nrhs, n)
            h.call(f"rflu_getrs_batched_{sfx}_dev", batch, n, nrhs, ptr(packed), n, n * n, 0, ptr(ip0), mn, ptr(X0), n, n * nrhs, code)
            assert h.last_path() == _ffi.PATH_HIP_BATCHED
            x0 = np.transpose(host(X0), (0, 2, 1))
            bimg = torch.from_numpy(np.array(B if row_major else np.transpose(B, (0, 2, 1)), order="C", copy=True)).to("cuda:0")
            brows = nrhs if row_major else n
            bbuf, bview, ldb, bstride = _padded(bimg, 2, 3)
            h.call(f"rflu_getrs_batched_{sfx}_dev", batch, n, nrhs, ptr(buf), lda, stride, row_major, ptr(ip1), sip, ptr(bbuf), ldb, bstride, code)
            x1 = host(bview[:, :, :brows])
            x1 = x1 if row_major else np.transpose(x1, (0, 2, 1))
            assert same_bits(np.ascontiguousarray(x1), np.ascontiguousarray(x0)), (nrhs, trans)
            assert _untouched(bbuf, bview, brows) and _untouched(buf, view, rows)
            for b in range(batch):
                assert CB.backward_error(A[b], x0[b], B[b], trans) <= CB.bar_E(n, sfx)


# ---- 6. solves ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx,n", [(sfx, n) for sfx in SFX for n in CB.SQUARE[sfx]])
def test_solves_meet_the_backward_error_bar_against_their_own_operator(sfx, n):
    batch = max(CB.BATCHES)
    A = CB.host_batch(n, n, sfx, batch)
    bar = CB.bar_E(n, sfx)
    worst = 0.0
    for dev in (dev_cm, dev_rm):
        F = rf.lu_complex_batched_(dev(A))
        for nrhs in CB.NRHS:
            B = CB.rhs_batch(n, nrhs, sfx, batch)
            for trans in "NTC":
                dB = dev(B)
                out = rf.ldiv_complex_batched_(F, dB, trans=trans)
                assert out is dB and rf.last_path() == "hip-batched"
                X = host(dB)
                for b in range(batch):
                    be = CB.backward_error(A[b], X[b], B[b], trans)
                    worst = max(worst, be / bar)
                    assert be <= bar, (dev.__name__, nrhs, trans, b, be, bar)
                if nrhs == 1:   # the same as a batch of vectors
                    dv = torch.from_numpy(np.array(B[:, :, 0], order="C", copy=True)).to("cuda:0")
                    rf.ldiv_complex_batched_(F, dv, trans=trans)
                    assert same_bits(host(dv), np.ascontiguousarray(X[:, :, 0]))
                if trans == "C":
                    dC = dev(B)
                    rf.ldiv_complex_batched_(rf.Adjoint(F), dC)
                    assert same_bits(host(dC), X), "Adjoint(F) is not trans='C'"
    print(f"{sfx} n={n}: worst backward error {worst:.4f} of 20 n eps")


@pytest.mark.parametrize("sfx", SFX)
def test_t_and_c_cannot_stand_in_for_each_other(sfx):
    """On matrices with non-zero imaginary parts the 'T' result fails the 'C' check (and every other pairing of the letters) by orders
    of magnitude: judged against another operator the residual is (op'(A) - op(A)) x, of the size of A's imaginary part (or of
    A - A^T) times x whatever the precision, so the backward error is of order 0.1.  Demanded: at least 100 x the LOOSER of the two
    precisions' bars (7.6e-3 at n = 32), which is 1e11 x the ComplexF64 bar."""
    n, batch, nrhs = 32, 7, 8
    A = CB.host_batch(n, n, sfx, batch)
    assert np.abs(A.imag).min() > 0
    B = CB.rhs_batch(n, nrhs, sfx, batch)
    F = rf.lu_complex_batched_(dev_cm(A))
    X = {t: host(rf.ldiv_complex_batched_(F, dev_cm(B), trans=t)) for t in "NTC"}
    bar, wrong = CB.bar_E(n, sfx), 100 * CB.bar_E(n, "cf32")
    for b in range(batch):
        for t in "NTC":
            assert CB.backward_error(A[b], X[t][b], B[b], t) <= bar
            for other in sorted(set("NTC") - {t}):
                assert CB.backward_error(A[b], X[t][b], B[b], other) > wrong, (b, t, other)


@pytest.mark.parametrize("sfx,n", [(sfx, n) for sfx in SFX for n in CB.SQUARE[sfx] if n > 1])
def test_notipiv_factors_of_shifted_matrices(sfx, n):
    """test/runtests.jl:116-128: NoPivot on rand + 10 I, NotIPIV pivots, ||A x - b|| < 1000 n eps -- here for every letter's operator."""
    batch = 7
    D = np.stack([CB.nopivot_matrix(n, sfx, b) for b in range(batch)])
    B = CB.rhs_batch(n, 3, sfx, batch)
    bound = 1000 * n * CB.eps_of(sfx)
    for dev in (dev_cm, dev_rm):
        F = rf.lu_complex_batched_(dev(D), None, rf.NoPivot())
        assert isinstance(F.ipiv, rf.NotIPIV) and rf.last_path() == "hip-batched"
        for trans in "NTC":
            X = host(rf.ldiv_complex_batched_(F, dev(B), trans=trans)).astype(np.complex128)
            for b in range(batch):
                M = D[b].astype(np.complex128)
                M = M if trans == "N" else (M.T if trans == "T" else M.conj().T)
                assert np.linalg.norm(M @ X[b] - B[b]) < bound, (dev.__name__, trans, b)


@pytest.mark.parametrize("sfx,n", [("cf64", 32), ("cf64", 64), ("cf32", 64), ("cf32", 128)])
def test_batched_solve_agrees_with_the_single_matrix_path(sfx, n):
    """Both paths solve with the SAME factors (the batched call's).  Each solution x satisfies op(A) x = b + r with its own residual r,
    so the two differ by op(A)^-1 (r_single - r_batched): measured like a backward error, ||op(A) (x_batched - x_single)||_inf /
    (||op(A)||_inf ||x_single||_inf), the difference of two equally good solutions is at most the sum of their backward errors.  The
    bar: 4 x the single-matrix path's own backward error (the worst over the batch, per letter)."""
    batch, nrhs = 7, 3
    A = CB.host_batch(n, n, sfx, batch)
    B = CB.rhs_batch(n, nrhs, sfx, batch)
    F = rf.lu_complex_batched_(dev_cm(A))
    single = {"N": rf.ldiv_complex_, "T": rf.ldiv_complex_transpose_, "C": rf.ldiv_complex_adjoint_}
    for trans in "NTC":
        X = host(rf.ldiv_complex_batched_(F, dev_cm(B), trans=trans))
        own, diff = 0.0, 0.0
        for b in range(batch):
            S = rf.LU(F.factors[b], F.ipiv[b], 0)
            assert S.factors.stride(0) == 1
            Y = torch.from_numpy(np.array(B[b].T, order="C", copy=True)).to("cuda:0").T
            y = host(single[trans](S, Y))
            own = max(own, CB.backward_error(A[b], y, B[b], trans))
            M = A[b].astype(np.complex128)
            M = M if trans == "N" else (M.T if trans == "T" else M.conj().T)
            d = M @ (X[b].astype(np.complex128) - y.astype(np.complex128))
            diff = max(diff, float(np.linalg.norm(d, np.inf) / (np.linalg.norm(M, np.inf) * np.linalg.norm(y, np.inf))))
        print(f"{sfx} n={n} {trans}: difference {diff:.3e}, single path's backward error {own:.3e}")
        assert diff <= 4 * own, (trans, diff, own)


@pytest.mark.parametrize("sfx", SFX)
def test_a_singular_matrix_spoils_only_its_own_solution(sfx):
    n, batch, bad = 50, 7, 4
    A = np.array(CB.host_batch(50, 52, sfx, batch)[:, :, :n])
    A[bad][:, 20] = 0
    with pytest.raises(rf.SingularException) as ei:
        rf.lu_complex_batched_(dev_cm(A))
    assert ei.value.batch_index == bad and ei.value.info == 21
    F = rf.lu_complex_batched_(dev_cm(A), check=False)
    assert not F.issuccess() and host(F.info).tolist() == [21 if b == bad else 0 for b in range(batch)]
    B = CB.rhs_batch(n, 2, sfx, batch)
    with pytest.raises(rf.SingularException) as ei:
        rf.ldiv_complex_batched_(F, dev_cm(B))
    assert ei.value.batch_index == bad
    for trans in "NTC":
        X = host(rf.ldiv_complex_batched_(F, dev_cm(B), trans=trans, check=False))
        assert np.isfinite(X).all(axis=(1, 2)).tolist() == [b != bad for b in range(batch)]
        for b in range(batch):
            if b != bad:
                assert CB.backward_error(A[b], X[b], B[b], trans) <= CB.bar_E(n, sfx)
    # NoPivot reports the same matrix with the sign convention of lu_
    N = np.stack([CB.nopivot_matrix(n, sfx, b) for b in range(batch)])
    N[bad] = np.triu(N[bad])
    N[bad][30, 30] = 0
    G = rf.lu_complex_batched_(dev_cm(N), None, rf.NoPivot(), check=False)
    assert int(host(G.info)[bad]) == (-31 if rf.NOPIVOT_NEGATIVE_INFO else 31) and np.count_nonzero(host(G.info)) == 1


# ---- 7. the loop above the one-launch limit --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx", SFX)
def test_larger_matrices_go_through_the_loop(sfx):
    m, n = CB.FALLBACK[sfx]
    batch = 3
    A = CB.host_batch(m, n, sfx, batch)
    F = rf.lu_complex_batched_(dev_cm(A), check=False)
    assert rf.last_path() == "hip-recursive"          # what the single-matrix complex path reports
    check_batch(A, sfx, True, host(F.factors), host(F.ipiv), host(F.info))
    N = rf.lu_complex_batched_(dev_cm(A), None, rf.NoPivot(), check=False)
    sign = -1 if rf.NOPIVOT_NEGATIVE_INFO else 1
    check_batch(A, sfx, False, host(N.factors), np.tile(np.arange(1, n + 1), (batch, 1)), sign * host(N.info))
    # a singular matrix of the loop reports its own info
    Z = np.array(A)
    Z[1][:, 4] = 0
    assert host(rf.lu_complex_batched_(dev_cm(Z), check=False).info).tolist() == [0, 5, 0]
    B = CB.rhs_batch(n, 9, sfx, batch)
    for trans in "NTC":
        X = host(rf.ldiv_complex_batched_(F, dev_cm(B), trans=trans))
        for b in range(batch):
            assert CB.backward_error(A[b], X[b], B[b], trans) <= CB.bar_E(n, sfx), (trans, b)
    # row-major above the limit: refused with a message that says why
    with pytest.raises(rf.RfluError, match=r"status 1: .*row-major.*column-major only"):
        rf.lu_complex_batched_(dev_rm(A), check=False)
    R = rf.BatchedLU(dev_rm(A), F.ipiv, F.info)
    with pytest.raises(rf.RfluError, match=r"status 1: .*row-major.*column-major only"):
        rf.ldiv_complex_batched_(R, dev_rm(B))


# ---- 8. determinism -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx", SFX)
def test_two_calls_return_the_same_bits(sfx):
    n = CB.LIMIT[sfx]
    batch = max(CB.BATCHES)
    A = CB.host_batch(n, n, sfx, batch)
    B = CB.rhs_batch(n, 9, sfx, batch)
    F, G = (rf.lu_complex_batched_(dev_cm(A), check=False) for _ in range(2))
    assert same_bits(host(F.factors), host(G.factors)) and torch.equal(F.ipiv, G.ipiv) and torch.equal(F.info, G.info)
    for trans in "NTC":
        X, Y = (host(rf.ldiv_complex_batched_(F, dev_cm(B), trans=trans)) for _ in range(2))
        assert same_bits(X, Y), trans


# ---- 9. zero sizes and argument errors through the raw ABI ----------------------------------------------------------------------------
@pytest.mark.parametrize("sfx", SFX)
def test_sizes_of_zero_and_argument_errors(sfx):
    ct = torch.complex128 if sfx == "cf64" else torch.complex64
    for shape in ((0, 4, 4), (3, 0, 5), (3, 5, 0)):
        F = rf.lu_complex_batched_(torch.empty(shape, dtype=ct, device="cuda:0"))
        assert F.info.shape == (shape[0],) and F.issuccess()
    h = handle()
    A = torch.full((4, 8, 8), 3.0, dtype=ct, device="cuda:0")
    ip = torch.full((4, 8), -7, dtype=torch.int64, device="cuda:0")
    info = torch.full((4,), -1, dtype=torch.int64, device="cuda:0")
    B = torch.full((4, 8), 5.0, dtype=ct, device="cuda:0")
    keep = [t.clone() for t in (A, ip, info, B)]
    f, s = f"rflu_getrf_batched_{sfx}_dev", f"rflu_getrs_batched_{sfx}_dev"
    for args in ((0, 8, 8, ptr(A), 8, 64, 0, ptr(ip), 8, 1, ptr(info)), (4, 0, 8, ptr(A), 8, 64, 0, ptr(ip), 8, 1, ptr(info)),
                 (4, 8, 0, ptr(A), 8, 64, 0, ptr(ip), 8, 1, ptr(info))):
        h.call(f, *args)
    for args in ((0, 8, 1, ptr(A), 8, 64, 0, ptr(ip), 8, ptr(B), 8, 8, 0), (4, 0, 1, ptr(A), 8, 64, 0, ptr(ip), 8, ptr(B), 8, 8, 1),
                 (4, 8, 0, ptr(A), 8, 64, 0, ptr(ip), 8, ptr(B), 8, 8, 2)):
        h.call(s, *args)
    bad_f = ((4, 8, 8, ptr(A), 7, 64, 0, ptr(ip), 8, 1, ptr(info)),          # lda < m
             (4, 8, 8, ptr(A), 8, 63, 0, ptr(ip), 8, 1, ptr(info)),          # matrices overlap
             (4, 8, 8, ptr(A), 8, 64, 0, ptr(ip), 7, 1, ptr(info)),          # pivots overlap
             (4, 8, 8, ptr(A), 8, 64, 0, NULL, 8, 1, ptr(info)),             # pivoting without ipiv
             (4, 8, 8, ptr(A), 8, 64, 0, ptr(ip), 8, 1, NULL),               # no info
             (4, 8, 8, NULL, 8, 64, 0, ptr(ip), 8, 1, ptr(info)),
             (-1, 8, 8, ptr(A), 8, 64, 0, ptr(ip), 8, 1, ptr(info)),
             (4, -8, 8, ptr(A), 8, 64, 0, ptr(ip), 8, 1, ptr(info)),
             (4, 8, -8, ptr(A), 8, 64, 0, ptr(ip), 8, 1, ptr(info)))
    bad_s = ((4, 8, 1, ptr(A), 8, 64, 0, ptr(ip), 8, ptr(B), 7, 8, 0),       # ldb < n
             (4, 8, 1, ptr(A), 8, 64, 0, ptr(ip), 8, ptr(B), 8, 7, 0),       # right-hand sides overlap
             (4, 8, 1, ptr(A), 7, 64, 0, ptr(ip), 8, ptr(B), 8, 8, 0),       # lda < n
             (4, 8, 1, ptr(A), 8, 64, 0, ptr(ip), 7, ptr(B), 8, 8, 0),       # pivots overlap
             (4, 8, 1, ptr(A), 8, 64, 0, ptr(ip), 8, NULL, 8, 8, 0),
             (4, 8, 1, NULL, 8, 64, 0, ptr(ip), 8, ptr(B), 8, 8, 0),
             (4, 8, -1, ptr(A), 8, 64, 0, ptr(ip), 8, ptr(B), 8, 8, 0),
             (-4, 8, 1, ptr(A), 8, 64, 0, ptr(ip), 8, ptr(B), 8, 8, 0),
             (4, 8, 1, ptr(A), 8, 64, 0, ptr(ip), 8, ptr(B), 8, 8, 3),       # trans is 0, 1 or 2
             (4, 8, 1, ptr(A), 8, 64, 0, ptr(ip), 8, ptr(B), 8, 8, -1))
    for name, rows in ((f, bad_f), (s, bad_s)):
        for args in rows:
            with pytest.raises(rf.RfluError, match=r"status 1: \S"):
                h.call(name, *args)
    for t, k in zip((A, ip, info, B), keep):
        assert torch.equal(t, k)
    # NULL ipiv is NotIPIV with pivot == 0, in the factorization and in the solve
    D = dev_cm(np.stack([CB.nopivot_matrix(8, sfx, b) for b in range(4)]))
    h.call(f, 4, 8, 8, ptr(D), 8, 64, 0, NULL, 0, 0, ptr(info))
    assert h.last_path() == _ffi.PATH_HIP_BATCHED and bool((info == 0).all())
    Bh = CB.rhs_batch(8, 1, sfx, 4)
    X = dev_cm(Bh)
    h.call(s, 4, 8, 1, ptr(D), 8, 64, 0, NULL, 0, ptr(X), 8, 8, 0)
    for b in range(4):
        assert CB.backward_error(CB.nopivot_matrix(8, sfx, b), host(X)[b], Bh[b], "N") <= CB.bar_E(8, sfx)
