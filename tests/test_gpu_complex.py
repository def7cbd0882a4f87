"""ComplexF64 / ComplexF32 lu!, lu and ldiv! on the GPU (csrc/complex.hip, csrc/complex_gemm.hip) against the CPU restatement of the
reference's algorithm (tests/complex_ref.py): the complex MFMA GEMM, the factorization through the device and the host entry, pivoted
and NoPivot, the solve, and the argument rules of the raw ABI.  Buffers go through gpu_util; every compute call through librflu."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import complex_ref as CR
import gpu_util as G
import helpers
import oracle as O
import recursivefactorization.jl_amd as rf
from recursivefactorization.jl_amd import _ffi

pytestmark = pytest.mark.gpu

SFX = ["cf64", "cf32"]
EPS = {"cf64": np.finfo(np.float64).eps, "cf32": np.finfo(np.float32).eps}
TORCH_REAL = {"cf64": torch.float64, "cf32": torch.float32}


def _null():
    return ctypes.c_void_p(0)


# ---- complex GEMM ------------------------------------------------------------------------------------------------------------------------
GEMM_SHAPES = [(1, 1, 1), (16, 16, 4), (64, 64, 64), (130, 70, 65), (128, 128, 16), (257, 300, 129), (384, 393, 266)]


def _gemm_inputs(M, N, K, sfx):
    ct = CR.CTYPES[sfx]
    real = CR.real_of(ct)

    def mat(r, c, seed):
        return (O.np_uniform(r, c, seed, real) + 1j * O.np_uniform(r, c, seed + 500, real)).astype(ct)

    return mat(M, K, 3 + M), mat(K, N, 5 + N), mat(M, N, 7 + K)


def _gemm_check(Cout, A, B, C, K, sfx):
    ref = C.astype(np.complex128) - A.astype(np.complex128) @ B.astype(np.complex128)
    bar = (2 * K + 4) * EPS[sfx] * 4        # tests/test_gpu_kernels.py's bar with K -> 2K: each part sums 2K products of entries in [0, 1)
    err = max(float(np.abs(Cout.real - ref.real).max()), float(np.abs(Cout.imag - ref.imag).max()))
    print(f"gemm {sfx} K={K}: max part error {err:.3e}, bar {bar:.3e}")
    assert err <= bar, (err, bar)


@pytest.mark.parametrize("sfx", SFX)
@pytest.mark.parametrize("shape", GEMM_SHAPES)
def test_complex_gemm(sfx, shape):
    M, N, K = shape
    A, B, C = _gemm_inputs(M, N, K, sfx)
    dA, dB, dC = G.to_dev_rm(A), G.to_dev_rm(B), G.to_dev_rm(C)
    G.handle().call(f"rflu_gemm_rm_{sfx}_dev", M, N, K, G.ptr(dA), K, G.ptr(dB), N, G.ptr(dC), N)
    _gemm_check(dC.cpu().numpy(), A, B, C, K, sfx)


@pytest.mark.parametrize("sfx", SFX)
def test_complex_gemm_strided_views_at_an_8_byte_offset(sfx):
    """Operands inside larger buffers, leading dimensions beyond the widths, every pointer 8 bytes off a 16-byte boundary:
    the element-by-element path.  The padding around the views must come back untouched."""
    M, N, K = 130, 70, 65
    lda, ldb, ldc = K + 3, N + 5, N + 7
    A, B, C = _gemm_inputs(M, N, K, sfx)
    real = CR.real_of(CR.CTYPES[sfx])
    off = 8 // np.dtype(real).itemsize           # reals in front of the view: 8 bytes

    def embed(X, ld):
        buf = np.full(off + 2 * X.shape[0] * ld + 4, -7.0, dtype=real)
        v = buf[off:off + 2 * X.shape[0] * ld].reshape(X.shape[0], ld, 2)
        v[:, :X.shape[1], 0] = X.real
        v[:, :X.shape[1], 1] = X.imag
        return buf

    hA, hB, hC = embed(A, lda), embed(B, ldb), embed(C, ldc)
    dA, dB, dC = (torch.from_numpy(x).to("cuda:0") for x in (hA, hB, hC))
    for t in (dA, dB, dC):
        assert t.data_ptr() % 16 == 0

    def p(t):
        return ctypes.c_void_p(t.data_ptr() + 8)

    G.handle().call(f"rflu_gemm_rm_{sfx}_dev", M, N, K, p(dA), lda, p(dB), ldb, p(dC), ldc)
    out = dC.cpu().numpy()
    v = out[off:off + 2 * M * ldc].reshape(M, ldc, 2)
    _gemm_check(v[:, :N, 0] + 1j * v[:, :N, 1], A, B, C, K, sfx)
    assert np.all(v[:, N:, :] == -7.0) and np.all(out[:off] == -7.0) and np.all(out[off + 2 * M * ldc:] == -7.0)


# ---- factorization -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rand(m, n, sfx, zero_col=-1):
    A = CR.rand_complex(m, n, CR.CTYPES[sfx])
    if zero_col >= 0:
        A[:, zero_col] = 0
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def _ref(m, n, sfx, pivot, zero_col=-1):
    """The restatement in the precision of the input: (factors, ipiv, info, relative Frobenius residual).  Computed once, never modified."""
    A = _rand(m, n, sfx, zero_col)
    F, ip, info = CR.complex_generic_lufact(A, pivot)
    F.setflags(write=False)
    ip.setflags(write=False)
    return F, ip, info, CR.residual_fro_rel(A, F, ip)


def _getrf_dev(A, sfx, pivot, ipiv="alloc"):
    """Raw device entry on a column-major copy: (factors, ipiv, info) on the host."""
    m, n = A.shape
    mn = min(m, n)
    dA = G.to_dev_cm(A)
    dip = torch.full((max(mn, 1),), -99, dtype=torch.int64, device="cuda:0") if ipiv == "alloc" else None
    info = ctypes.c_int64(-1)
    G.handle().call(f"rflu_getrf_{sfx}_dev", m, n, G.ptr(dA), max(m, 1), G.ptr(dip) if dip is not None else _null(), int(pivot),
                    ctypes.byref(info))
    return dA.cpu().numpy(), (dip.cpu().numpy()[:mn] if dip is not None else None), int(info.value)


def _check_ipiv_cf32(A32, ipiv_dev):
    """ComplexF32: equal to the restatement run in complex128 on the same Float32-valued input up to the first difference; there the
    device's choice must hold at least (1 - 8 m eps32) of the largest modulus of the restatement's state.  Returns the fork step or None."""
    m = A32.shape[0]
    _, ip, _, mods = CR.complex_generic_lufact(A32.astype(np.complex128), True, moduli=True)
    diff = np.flatnonzero(ip != ipiv_dev)
    if diff.size == 0:
        return None
    k = int(diff[0])
    a = mods[k]
    chosen = a[int(ipiv_dev[k]) - 1 - k]
    assert chosen >= (1 - 8 * m * EPS["cf32"]) * np.nanmax(a), (k, chosen, np.nanmax(a))
    return k


def _check_factorization(A, sfx, pivot, F, ip, info, ref, on_ref_shape):
    """The bars of one factorization against the restatement `ref` = (F, ipiv, info, residual); returns the residual ratio."""
    m, n = A.shape
    Fr, ipr, infor, resr = ref
    assert info == infor, (info, infor)
    if pivot:
        if sfx == "cf64":
            assert np.array_equal(ip, ipr), f"ipiv differs first at step {int(np.flatnonzero(ip != ipr)[0])}"
        else:
            fork = _check_ipiv_cf32(A, ip)
            print(f"  cf32 {m}x{n}: ipiv fork {'none' if fork is None else 'at step %d' % fork}")
            L = np.tril(F[:, :min(m, n)], -1)
            assert np.abs(L).max(initial=0.0) <= 1 + 4 * EPS["cf32"]
    else:
        assert np.array_equal(ip, np.arange(1, min(m, n) + 1))
    if infor != 0:
        return float("nan")
    if on_ref_shape:      # the reference's own bar, test/runtests.jl:21-31
        E = 20 * m * EPS[sfx]
        r = CR.residual_inf(A, F, ip)
        assert r < (E if pivot else 10 * np.sqrt(E)), (m, n, pivot, r, E)
    res = CR.residual_fro_rel(A, F, ip)
    ratio = res / resr if resr > 0 else (0.0 if res == 0 else float("inf"))
    if not on_ref_shape:  # a different summation order moves the constant, not the order: at most 4x the restatement's own residual
        assert res <= 4 * resr, (m, n, pivot, res, resr)
    return ratio


@pytest.mark.parametrize("sfx", SFX)
@pytest.mark.parametrize("shape", CR.REF_SHAPES + CR.EXTRA_SHAPES)
def test_factorization_device_and_host_entry(sfx, shape):
    """Both entries, pivoted and NoPivot, on the plain random input.  info and ipiv as the restatement's (ComplexF32: the fork rule),
    the reference's residual bar on the reference's shapes, at most 4x the restatement's relative residual on the larger ones.
    Measured on an MI355X, residual of the device over the restatement's on the same input and precision: on the larger shapes
    0.96 .. 1.03 (ComplexF64) and 0.85 .. 1.17 (ComplexF32), pivoted and NoPivot alike (777x650: 1.010 / 0.991 ComplexF64, 1.169 / 0.986
    ComplexF32; 650x777: 1.005 / 0.986 and 1.152 / 0.939; 2100x70: 1.002 / 0.969 and 1.095 / 0.933; 70x2100: 0.998 / 0.966 and 1.072 /
    0.881); on the reference's shapes from 10 x 10 on 0.87 .. 1.45, below that single roundings decide (0 .. 2.5).  No ComplexF32
    ipiv fork on any shape.  The test prints each ratio."""
    m, n = shape
    on_ref = shape in CR.REF_SHAPES
    A = _rand(m, n, sfx)
    for pivot in (True, False):
        ref = _ref(m, n, sfx, pivot)
        F, ip, info = _getrf_dev(A, sfx, pivot)
        ratio = _check_factorization(A, sfx, pivot, F, ip, info, ref, on_ref)
        assert rf.last_path() == "hip-recursive"
        # the host entry through the Python mirror: the same bits, NoPivot's info with the sign of Julia >= 1.11
        H = rf.lu_complex(A, rf.RowMaximum() if pivot else rf.NoPivot(), check=False)
        assert H.factors.dtype == A.dtype and np.array_equal(CR.bits(H.factors), CR.bits(F))
        assert H.info == (info if pivot else -info)
        if pivot:
            assert np.array_equal(H.ipiv, ip)
            assert np.array_equal(H.p, CR.perm_of(ip, m))
            k = min(m, n)
            assert np.array_equal(H.L, np.tril(F[:, :k], -1) + np.eye(m, k, dtype=F.dtype)) and np.array_equal(H.U, np.triu(F[:k, :]))
        else:
            assert isinstance(H.ipiv, rf.NotIPIV) and len(H.ipiv) == min(m, n)
        print(f"{sfx} {m}x{n} {'pivoted' if pivot else 'NoPivot'}: residual ratio device / restatement = {ratio:.3f}")


@pytest.mark.parametrize("sfx", SFX)
@pytest.mark.parametrize("shape", [(10, 12), (130, 130), (300, 302)])
def test_zeroed_column_sets_info_and_carries_on(sfx, shape):
    """test/runtests.jl:56-66: column 5 zeroed, check = false.  info as the restatement's, the elimination continues past it."""
    m, n = shape
    A = _rand(m, n, sfx, 4)
    Fr, ipr, infor, _ = _ref(m, n, sfx, True, 4)
    assert infor == 5
    for entry in ("dev", "host"):
        if entry == "dev":
            F, ip, info = _getrf_dev(A, sfx, True)
        else:
            H = rf.lu_complex(A, check=False)
            F, ip, info = H.factors, H.ipiv, H.info
            assert not H.issuccess()
        assert info == infor
        if sfx == "cf64":
            assert np.array_equal(ip, ipr)
        else:
            _check_ipiv_cf32(A, ip)
        assert np.all(np.isfinite(F))
        # L*U still reproduces the permuted input: the columns right of the zero one were eliminated
        E = 20 * m * EPS[sfx]
        assert CR.residual_inf(A, F, ip) < E
    with pytest.raises(rf.SingularException):
        rf.lu_complex(A)
    F2, _, info2 = _getrf_dev(A, sfx, False)
    assert info2 == _ref(m, n, sfx, False, 4)[2]


@pytest.mark.parametrize("sfx", SFX)
@pytest.mark.parametrize("case", list(zip(CR.EXACT_CASES, CR.EXACT_INFO)))
def test_exact_inputs_tie_break_and_identical_factors(sfx, case):
    """Moduli are powers of two, quotients powers of two times a unit, products have a zero factor: every operation is exact, so ipiv,
    info and the factors equal the restatement's in both precisions.  Ties, spread over the whole height, go to the lowest current row.
    Every real and every imaginary part is compared BIT FOR BIT, with one exemption that is asserted as such: a part that is a zero
    on BOTH sides may differ in the sign of that zero.  That sign is not a property of the algorithm but of the association of exact
    zero terms: the GEMM forms c - lr*ur + li*ui as one k-ordered chain per part, the restatement's numpy product (lr*ur - li*ui)
    first, and -0 - 0 + 0 = +0 where -0 - (0 - 0) = -0.  A zero against a non-zero, and any two non-zero parts that differ in a bit,
    fail.  README.md and DESIGN.md section 4.5 state the same deviation from "bit for bit"."""
    (m, n, empty), want = case
    A = CR.exact_complex(m, n, empty, CR.CTYPES[sfx])
    Fr, ipr, infor = CR.complex_generic_lufact(A, True)
    assert infor == want
    F, ip, info = _getrf_dev(A, sfx, True)
    assert info == want
    assert np.array_equal(ip, ipr), f"ipiv differs first at step {int(np.flatnonzero(ip != ipr)[0])}"
    P, Pr = CR.parts(F), CR.parts(Fr)          # real and imaginary parts as separate numbers
    both_zero = (P == 0) & (Pr == 0)           # the one exemption: the sign of a zero that is a zero on both sides
    differ = CR.bits(P) != CR.bits(Pr)
    assert not np.any(differ & ~both_zero), f"{int(np.count_nonzero(differ & ~both_zero))} parts differ in their bits"
    print(f"exact {sfx} {m}x{n}: {int(np.count_nonzero(differ))} of {P.size} parts are zeros of the other sign, every other part identical")
    H = rf.lu_complex(A, check=False)
    assert H.info == want and np.array_equal(H.ipiv, ipr) and np.array_equal(CR.bits(H.factors), CR.bits(F))


@pytest.mark.parametrize("sfx", SFX)
def test_nopivot_fills_a_user_ipiv_and_null_needs_nopivot(sfx):
    """test/runtests.jl:70-84: a caller's ipiv holds 1..min(m,n) after a NoPivot factorization; NULL plays NotIPIV with pivot == 0 only."""
    ct = CR.CTYPES[sfx]
    for m, n in ((50, 50), (40, 70), (70, 40)):
        A = np.asfortranarray(_rand(m, n, sfx) + 10 * np.eye(m, n)).astype(ct)
        F, ip, info = _getrf_dev(A, sfx, False)          # ipiv poisoned with -99 beforehand
        assert info == 0 and np.array_equal(ip, np.arange(1, min(m, n) + 1))
        F0, none, info0 = _getrf_dev(A, sfx, False, ipiv=None)
        assert none is None and info0 == 0 and np.array_equal(CR.bits(F0), CR.bits(F))
        hip = np.full(min(m, n), -5, dtype=np.int64)
        Ah = np.array(A, order="F")
        Hh = rf.lu_complex_(Ah, hip, rf.NoPivot())
        assert Hh.ipiv is hip and np.array_equal(hip, np.arange(1, min(m, n) + 1)) and np.array_equal(CR.bits(Ah), CR.bits(F))
    with pytest.raises(_ffi.RfluError, match="status 1.*ipiv"):
        _getrf_dev(_rand(8, 8, sfx), sfx, True, ipiv=None)


@pytest.mark.parametrize("sfx", SFX)
def test_nan_entry_is_never_chosen(sfx):
    """A NaN + 0i entry in a column that also has finite non-zero candidates: `NaN > x` is false, so it never wins."""
    A = np.array(_rand(50, 50, sfx), order="F")
    A[7, 0] = complex(np.nan, 0.0)
    A[30, 5] = complex(np.nan, 0.0)
    Fr, ipr, infor, mods = CR.complex_generic_lufact(A, True, moduli=True)
    F, ip, info = _getrf_dev(A, sfx, True)
    assert info == infor == 0
    for k, a in enumerate(mods):
        finite = np.isfinite(a) & (a > 0)
        if finite.any():
            assert not np.isnan(a[ipr[k] - 1 - k])
    if sfx == "cf64":
        assert np.array_equal(ip, ipr)
    else:
        _check_ipiv_cf32(A, ip)
    assert ip[0] != 8


def test_a_real_factorization_follows_on_the_same_handle():
    """The complex path shares the handle's workspaces with the real one: a real lu at n = 300 right behind it still meets its bar."""
    A = _rand(300, 300, "cf64")
    _getrf_dev(A, "cf64", True)
    assert rf.last_path() == "hip-recursive"
    R = np.asfortranarray(O.np_uniform(300, 300, 12))
    F = rf.lu(R, check=False)
    assert F.info == 0
    L, U = np.tril(F.factors, -1) + np.eye(300), np.triu(F.factors)
    assert np.linalg.norm(L @ U - R[F.p, :], np.inf) < 20 * 300 * np.finfo(np.float64).eps
    Fr, ipr, _, _ = _ref(300, 300, "cf64", True)
    F2, ip2, _ = _getrf_dev(A, "cf64", True)
    assert np.array_equal(ip2, ipr)


# ---- solve ---------------------------------------------------------------------------------------------------------------------------------
SQUARES = helpers.REF_SIZES + [63, 64, 65, 128]


def _backward_error(A, X, B):
    A, X, B = (np.asarray(t).astype(np.complex128) for t in (A, X, B))
    X = X.reshape(A.shape[0], -1)
    B = B.reshape(A.shape[0], -1)
    return float(np.linalg.norm(A @ X - B, np.inf) / (np.linalg.norm(A, np.inf) * np.linalg.norm(X, np.inf)))


@pytest.mark.parametrize("sfx", SFX)
def test_solve_on_the_square_shapes(sfx):
    """ldiv!(F, A[:, end]) ~ e_n with atol = 100 E (test/runtests.jl:21-28), and nrhs in {1, 3, 33, 70} with the normwise backward error
    ||A X - B||_inf / (||A||_inf ||X||_inf) <= E = 20 n eps; device entry for every nrhs, host entry for nrhs = 3."""
    worst = 0.0
    for n in SQUARES:
        A = _rand(n, n, sfx)
        E = 20 * n * EPS[sfx]
        dF = G.to_dev_cm(A)
        F = rf.lu_complex_(dF)
        b = G.to_dev_cm(A[:, -1:].copy())[:, 0]
        x = rf.ldiv_complex_(F, b).cpu().numpy()
        e = np.zeros(n)
        e[-1] = 1
        if np.all(np.isfinite(x)):
            assert np.abs(x - e).max() <= 100 * E, (n, np.abs(x - e).max())
        for nrhs in (1, 3, 33, 70):
            B = CR.rand_rhs(n, nrhs, CR.CTYPES[sfx])
            X = rf.ldiv_complex_(F, G.to_dev_cm(B)).cpu().numpy()
            be = _backward_error(A, X, B)
            worst = max(worst, be / E)
            assert be <= E, (n, nrhs, be, E)
        Hf = rf.lu_complex(A)
        B = CR.rand_rhs(n, 3, CR.CTYPES[sfx])
        X = rf.ldiv_complex_(Hf, np.array(B, order="F"))
        assert _backward_error(A, X, B) <= E
        v = np.array(B[:, 0])
        assert rf.ldiv_complex_(Hf, v) is v and _backward_error(A, v, B[:, 0]) <= E
    print(f"{sfx}: worst backward error {worst:.4f} E")


@pytest.mark.parametrize("sfx", SFX)
def test_solve_notipiv_strided_rhs_and_singular_u(sfx):
    ct = CR.CTYPES[sfx]
    n, nrhs = 130, 5
    E = 20 * n * EPS[sfx]
    # NotIPIV factors (NoPivot on a diagonally dominant matrix, no pivot vector)
    A = np.asfortranarray(_rand(n, n, sfx) + n * np.eye(n)).astype(ct)
    F = rf.lu_complex_(G.to_dev_cm(A), None, rf.NoPivot())
    assert isinstance(F.ipiv, rf.NotIPIV)
    B = CR.rand_rhs(n, nrhs, ct)
    X = rf.ldiv_complex_(F, G.to_dev_cm(B)).cpu().numpy()
    assert _backward_error(A, X, B) <= E
    # a right-hand side with ldb > n inside a larger buffer: the rows below stay as they were
    A = _rand(n, n, sfx)
    F = rf.lu_complex_(G.to_dev_cm(A))
    big = torch.full((nrhs, n + 5), -3.0, dtype=F.factors.dtype, device="cuda:0")
    view = big.T[:n, :]
    assert view.stride(0) == 1 and view.stride(1) == n + 5
    view.copy_(torch.from_numpy(np.ascontiguousarray(B)).to("cuda:0"))
    rf.ldiv_complex_(F, view)
    out = big.cpu().numpy()
    assert _backward_error(A, out[:, :n].T, B) <= E and np.all(out[:, n:] == -3.0)
    # a singular U: non-finite output, no error status (the raw entry; ldiv_complex_ checks info first)
    Z = _rand(n, n, sfx, 4)
    dZ = G.to_dev_cm(Z)
    S = rf.lu_complex_(dZ, check=False)
    assert S.info == 5
    with pytest.raises(rf.SingularException):
        rf.ldiv_complex_(S, G.to_dev_cm(B))
    dB = G.to_dev_cm(B)
    G.handle().call(f"rflu_getrs_{sfx}_dev", n, nrhs, G.ptr(dZ), n, G.ptr(S.ipiv), G.ptr(dB), n)
    assert not np.all(np.isfinite(dB.cpu().numpy()))


# ---- argument rules through the raw ABI -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx", SFX)
def test_argument_rules(sfx):
    h = G.handle()
    ct = CR.CTYPES[sfx]
    n = 8
    dA = G.to_dev_cm(_rand(n, n, sfx))
    dB = G.to_dev_cm(CR.rand_rhs(n, 2, ct))
    dip = torch.zeros(n, dtype=torch.int64, device="cuda:0")
    info = ctypes.c_int64(0)
    bi = ctypes.byref(info)
    bad = [
        (f"rflu_getrf_{sfx}_dev", (-1, n, G.ptr(dA), n, G.ptr(dip), 1, bi)),
        (f"rflu_getrf_{sfx}_dev", (n, -1, G.ptr(dA), n, G.ptr(dip), 1, bi)),
        (f"rflu_getrf_{sfx}_dev", (n, n, G.ptr(dA), n - 1, G.ptr(dip), 1, bi)),
        (f"rflu_getrf_{sfx}_dev", (n, n, _null(), n, G.ptr(dip), 1, bi)),
        (f"rflu_getrf_{sfx}_dev", (n, n, G.ptr(dA), n, G.ptr(dip), 1, _null())),
        (f"rflu_getrf_{sfx}_dev", (n, n, G.ptr(dA), n, _null(), 1, bi)),
        (f"rflu_getrs_{sfx}_dev", (-1, 2, G.ptr(dA), n, G.ptr(dip), G.ptr(dB), n)),
        (f"rflu_getrs_{sfx}_dev", (n, -2, G.ptr(dA), n, G.ptr(dip), G.ptr(dB), n)),
        (f"rflu_getrs_{sfx}_dev", (n, 2, G.ptr(dA), n - 1, G.ptr(dip), G.ptr(dB), n)),
        (f"rflu_getrs_{sfx}_dev", (n, 2, G.ptr(dA), n, G.ptr(dip), G.ptr(dB), n - 1)),
        (f"rflu_getrs_{sfx}_dev", (n, 2, _null(), n, G.ptr(dip), G.ptr(dB), n)),
        (f"rflu_getrs_{sfx}_dev", (n, 2, G.ptr(dA), n, G.ptr(dip), _null(), n)),
        (f"rflu_gemm_rm_{sfx}_dev", (-1, n, n, G.ptr(dA), n, G.ptr(dA), n, G.ptr(dA), n)),
        (f"rflu_gemm_rm_{sfx}_dev", (n, n, n, G.ptr(dA), n - 1, G.ptr(dA), n, G.ptr(dA), n)),
        (f"rflu_gemm_rm_{sfx}_dev", (n, n, n, G.ptr(dA), n, _null(), n, G.ptr(dA), n)),
    ]
    before = dA.clone()
    for name, args in bad:
        with pytest.raises(_ffi.RfluError, match=r"status 1: \S"):
            h.call(name, *args)
    assert torch.equal(torch.view_as_real(dA), torch.view_as_real(before))
    # zero sizes succeed and touch nothing
    sent = torch.full((16,), 7.0, dtype=dA.dtype, device="cuda:0")
    keep = sent.clone()
    for m0, n0 in ((0, 5), (5, 0), (0, 0)):
        info.value = -1
        h.call(f"rflu_getrf_{sfx}_dev", m0, n0, G.ptr(sent), max(m0, 1), G.ptr(dip), 1, bi)
        assert info.value == 0
    h.call(f"rflu_getrs_{sfx}_dev", 0, 3, G.ptr(sent), 1, G.ptr(dip), G.ptr(sent), 1)
    h.call(f"rflu_getrs_{sfx}_dev", 4, 0, G.ptr(sent), 4, G.ptr(dip), G.ptr(sent), 4)
    h.call(f"rflu_gemm_rm_{sfx}_dev", 4, 4, 0, G.ptr(sent), 1, G.ptr(sent), 4, G.ptr(sent), 4)
    h.call(f"rflu_gemm_rm_{sfx}_dev", 0, 4, 4, G.ptr(sent), 4, G.ptr(sent), 4, G.ptr(sent), 4)
    assert torch.equal(sent.real, keep.real) and torch.equal(sent.imag, keep.imag) and int(dip.abs().sum()) == 0
    # the host entry: a failed call leaves the caller's matrix as it was
    Ah = np.array(_rand(n, n, sfx), order="F")
    keep_h = Ah.copy()
    for args in ((n, n, ctypes.c_void_p(Ah.ctypes.data), n, _null(), 1, bi), (n, n, ctypes.c_void_p(Ah.ctypes.data), n - 1, _null(), 0, bi)):
        with pytest.raises(_ffi.RfluError, match=r"status 1: \S"):
            h.call(f"rflu_getrf_{sfx}", *args)
        assert np.array_equal(CR.bits(Ah), CR.bits(keep_h))
    Bh = np.array(CR.rand_rhs(n, 2, ct), order="F")
    keep_b = Bh.copy()
    with pytest.raises(_ffi.RfluError, match=r"status 1: \S"):
        h.call(f"rflu_getrs_{sfx}", n, 2, ctypes.c_void_p(Ah.ctypes.data), n, _null(), ctypes.c_void_p(Bh.ctypes.data), n - 1)
    assert np.array_equal(CR.bits(Bh), CR.bits(keep_b))
