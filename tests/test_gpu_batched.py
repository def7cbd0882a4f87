"""-m gpu: batched LU and solve (rflu_getrf_batched_* / rflu_getrs_batched_*, csrc/batched.hip) through lu_batched_ / ldiv_batched_
and the raw C ABI.

Inputs: matrix b of a batch is rand_matrix(m, n, seed=50000 + b, dtype); right-hand sides rand_matrix(n, nrhs, seed=70000 + b, dtype).
Bars.  ipiv and info equal oracle.lu(A) EXACTLY for every matrix (scripts/batched_fork_check.py: on these shapes and seeds, both
element types, the recursive oracle and LAPACK getrf agree on every pivot of all 26 000 matrices, worst residual 0.02 of the
reference bound -- no input sits on a rounding fork).  Factors: check_against_oracle of test_gpu_lu.py (residual < 20 m eps,
test/runtests.jl:19-20; factors within 50x that, scaled; NoPivot on rand + 10 I: 10 sqrt(E)).  max |l_ij| <= 1 exactly with pivoting.
Solves: rand + 10 I: ||A x - b|| < 1000 n eps(T), test/runtests.jl:124-126; plain rand, Float64: both bounds of
test_gpu_ldiv_adjoint.py::test_adjoint_solve_against_numpy -- LAPACK dgetrs on the same inputs (n = 8 .. 128, 200 matrices, nrhs 1
and 5, both directions): worst residual 5.2e-5 of its bound, worst solution error 1.9e-12 against 1e-6.
The solves are held to exact and rounding-level references, padded storage included, in tests/test_gpu_batched_solve_exact.py."""
import ctypes
import functools
import time

import numpy as np
import pytest
import torch

import oracle as O
import recursivefactorization.jl_amd as rf
from gpu_util import handle, ptr, sfx, tdtype, to_dev_cm
from helpers import rand_matrix, wilkinson
from test_gpu_lu import check_against_oracle

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (2, 2), (7, 7), (8, 8), (10, 12), (32, 32), (50, 52), (64, 64), (65, 65), (96, 96), (128, 128), (100, 60), (60, 100)]
CASES = [(s, 1000) for s in SHAPES] + [((64, 64), 1), ((64, 64), 257), ((128, 128), 1), ((128, 128), 257)]
DTYPES = [np.float64, np.float32]


@functools.lru_cache(maxsize=8)
def _host_batch(m, n, batch, dtype, diag):
    out = np.empty((batch, m, n), dtype=dtype)
    for b in range(batch):
        out[b] = rand_matrix(m, n, seed=50000 + b, dtype=dtype)
        if diag:
            out[b] += dtype(10) * np.eye(m, n, dtype=dtype)
    out.setflags(write=False)
    return out


def host_batch(m, n, batch, dtype, diag=False):
    return _host_batch(m, n, batch, np.dtype(dtype).type, diag)


def rhs_batch(n, nrhs, batch, dtype):
    return np.stack([rand_matrix(n, nrhs, seed=70000 + b, dtype=dtype) for b in range(batch)])


def dev_cm(A):
    """(batch, m, n) host array -> device tensor of that shape whose matrices are column-major (stride(1) == 1)."""
    return torch.from_numpy(np.array(np.transpose(A, (0, 2, 1)), order="C", copy=True)).to("cuda:0").transpose(1, 2)


def dev_rm(A):
    return torch.from_numpy(np.array(A, order="C", copy=True)).to("cuda:0")


def host(t):
    return t.cpu().numpy()


def check_batch_against_oracle(A, F, pivot=True):
    fac, info = host(F.factors), host(F.info)
    mn = min(A.shape[1:])
    ip = host(F.ipiv) if pivot else np.tile(np.arange(1, mn + 1), (A.shape[0], 1))
    for b in range(A.shape[0]):
        check_against_oracle(A[b], rf.LU(fac[b], ip[b], int(info[b])), pivot=pivot)
        if pivot:
            assert np.max(np.abs(np.tril(fac[b][:, :mn], -1)), initial=0.0) <= 1.0, f"matrix {b}: |l_ij| > 1 under partial pivoting"
    return fac, ip, info


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,batch", CASES)
def test_batched_lu_parity_with_the_oracle(shape, batch, dtype):
    m, n = shape
    A = host_batch(m, n, batch, dtype)
    dA = dev_cm(A)
    F = rf.lu_batched_(dA, check=False)
    assert rf.last_path() == "hip-batched"
    assert F.factors is dA and F.ipiv.shape == (batch, min(m, n)) and F.info.shape == (batch,) and F.info.is_cuda
    check_batch_against_oracle(A, F)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_batched_lu_nopivot(shape, dtype):
    m, n = shape
    batch, mn = 1000, min(m, n)
    A = host_batch(m, n, batch, dtype, diag=True)
    F = rf.lu_batched_(dev_cm(A), None, rf.NoPivot(), check=False)
    assert rf.last_path() == "hip-batched"
    assert isinstance(F.ipiv, rf.NotIPIV) and len(F.ipiv) == mn
    fac, _, _ = check_batch_against_oracle(A, F, pivot=False)
    # a poisoned user ipiv comes back as the identity (src/lu.jl:111-113), and the factors do not depend on it
    ipiv = torch.full((batch, mn), 2 ** 62, dtype=torch.int64, device="cuda:0")
    G = rf.lu_batched_(dev_cm(A), ipiv, rf.Val(False), check=False)
    assert G.ipiv is ipiv and np.array_equal(host(ipiv), np.tile(np.arange(1, mn + 1), (batch, 1)))
    assert np.array_equal(host(G.factors), fac)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [32, 64, 128])
def test_special_matrices_inside_one_batch(n, dtype):
    batch = 64
    base = host_batch(n, n, batch, dtype)
    A = base.copy()
    A[3][:, 7] = 0                                   # a zeroed column: info 8
    A[17] = wilkinson(n, dtype)                      # every column a tie
    A[40][n // 2 + 3, 2] = np.nan                    # a NaN below the diagonal
    A[63] = 0                                        # nothing but zero pivots: info 1
    special = (3, 17, 40, 63)
    F = rf.lu_batched_(dev_cm(A), check=False)
    F0 = rf.lu_batched_(dev_cm(base), check=False)
    fac, ip, info = host(F.factors), host(F.ipiv), host(F.info)
    fac0, ip0 = host(F0.factors), host(F0.ipiv)
    for b in special:
        _, ipo, infoo = O.lu(A[b])
        assert int(info[b]) == infoo and np.array_equal(ip[b], ipo), f"special matrix {b}"
    assert info[3] == 8 and info[63] == 1 and info[17] == 0
    for b in range(batch):
        if b not in special:
            assert info[b] == 0 and np.array_equal(ip[b], ip0[b]) and np.array_equal(fac[b], fac0[b]), f"matrix {b} saw its neighbours"
    with pytest.raises(rf.SingularException) as ei:
        rf.lu_batched_(dev_cm(A))
    assert ei.value.batch_index == 3 and ei.value.info == 8


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(10, 12), (64, 64), (100, 60)])
def test_matrices_are_independent_of_their_order(shape, dtype):
    m, n = shape
    batch = 1000
    A = host_batch(m, n, batch, dtype)
    perm = np.random.default_rng(7).permutation(batch)
    F = rf.lu_batched_(dev_cm(A), check=False)
    G = rf.lu_batched_(dev_cm(A[perm]), check=False)
    assert np.array_equal(host(G.factors), host(F.factors)[perm])
    assert np.array_equal(host(G.ipiv), host(F.ipiv)[perm])
    assert np.array_equal(host(G.info), host(F.info)[perm])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("row_major", [0, 1])
@pytest.mark.parametrize("shape", [(8, 8), (50, 52), (100, 60), (128, 128)])
def test_padding_through_the_raw_abi(shape, row_major, dtype):
    """lda = (contiguous dimension) + 3, strideA = lda * (other dimension) + 5, stride_ipiv = min(m, n) + 1, everything between the
    matrices NaN: bit-identical to the packed call, and the padding is still NaN afterwards."""
    m, n = shape
    batch, mn = 37, min(m, n)
    A = host_batch(m, n, batch, dtype)
    h = handle()
    td = tdtype(dtype)
    rows, cols = (n, m) if row_major else (m, n)      # rows = the contiguous dimension
    img = A if row_major else np.transpose(A, (0, 2, 1))   # (batch, cols, rows): the memory image of every matrix
    packed = torch.from_numpy(np.array(img, order="C", copy=True)).to("cuda:0")
    unfactored = packed.clone()
    ip0 = torch.zeros((batch, mn), dtype=torch.int64, device="cuda:0")
    info0 = torch.full((batch,), -1, dtype=torch.int64, device="cuda:0")
    h.call(f"rflu_getrf_batched_{sfx(dtype)}_dev", batch, m, n, ptr(packed), rows, rows * cols, row_major, ptr(ip0), mn, 1, ptr(info0))
    assert h.last_path() == 5
    lda, sip = rows + 3, mn + 1
    stride = lda * cols + 5
    buf = torch.full((batch, stride), float("nan"), dtype=td, device="cuda:0")
    view = buf[:, :lda * cols].view(batch, cols, lda)
    view[:, :, :rows] = unfactored
    ip1 = torch.full((batch, sip), -7, dtype=torch.int64, device="cuda:0")
    info1 = torch.full((batch,), -1, dtype=torch.int64, device="cuda:0")
    h.call(f"rflu_getrf_batched_{sfx(dtype)}_dev", batch, m, n, ptr(buf), lda, stride, row_major, ptr(ip1), sip, 1, ptr(info1))
    assert torch.equal(view[:, :, :rows], packed)
    assert torch.equal(ip1[:, :mn], ip0) and torch.equal(info1, info0) and bool((info0 == 0).all())
    assert bool(torch.isnan(view[:, :, rows:]).all()) and bool(torch.isnan(buf[:, lda * cols:]).all())
    assert bool((ip1[:, mn:] == -7).all())
    # and the packed result is the oracle's
    fac, ip = host(packed) if row_major else np.transpose(host(packed), (0, 2, 1)), host(ip0)
    for b in range(batch):
        check_against_oracle(A[b], rf.LU(fac[b], ip[b], 0))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_row_major_batches(shape, dtype):
    m, n = shape
    batch = 200
    A = host_batch(m, n, 1000, dtype)[:batch]
    Fc = rf.lu_batched_(dev_cm(A), check=False)
    dR = dev_rm(A)
    Fr = rf.lu_batched_(dR, check=False)
    assert rf.last_path() == "hip-batched" and Fr.factors is dR and dR.stride(2) == 1
    assert torch.equal(Fr.ipiv, Fc.ipiv) and torch.equal(Fr.info, Fc.info)
    check_batch_against_oracle(A, Fr)                 # factors equal to rounding: the oracle's bound, not bit equality


@pytest.mark.parametrize("dev", ["cm", "rm"])
def test_lu_batched_copies_and_keeps_the_layout(dev):
    A = host_batch(50, 52, 1000, np.float64)[:64]
    dA = dev_cm(A) if dev == "cm" else dev_rm(A)
    keep = dA.clone()
    F = rf.lu_batched(dA, check=False)
    assert torch.equal(dA, keep) and F.factors.data_ptr() != dA.data_ptr()
    assert (F.factors.stride(1) == 1) == (dev == "cm") and F.factors.shape == dA.shape
    G = rf.lu_batched_(dA, check=False)
    assert torch.equal(F.factors, G.factors) and torch.equal(F.ipiv, G.ipiv)


@pytest.mark.parametrize("dtype", DTYPES)
def test_larger_matrices_go_through_the_loop(dtype):
    A = host_batch(200, 200, 3, dtype)
    for dev in (dev_cm, dev_rm):
        F = rf.lu_batched_(dev(A), check=False)
        assert rf.last_path() == "hip-recursive"      # what the single-matrix path reports for this size
        check_batch_against_oracle(A, F)
    B = rhs_batch(200, 3, 3, dtype)
    D = host_batch(200, 200, 3, dtype, diag=True)
    F = rf.lu_batched_(dev_cm(D))
    for trans in (False, True):
        X = rf.ldiv_batched_(F, dev_cm(B), trans=trans)
        Dop = np.transpose(D, (0, 2, 1)) if trans else D
        res = np.linalg.norm(Dop.astype(np.float64) @ host(X) - B, axis=(1, 2))
        assert np.all(res < 1000 * 200 * np.finfo(dtype).eps), res.max()


def test_sizes_of_zero_and_argument_errors():
    for shape in ((0, 4, 4), (3, 0, 5), (3, 5, 0)):
        F = rf.lu_batched_(torch.empty(shape, dtype=torch.float64, device="cuda:0"))
        assert F.info.shape == (shape[0],) and F.issuccess()
    h = handle()
    A = torch.zeros((4, 8, 8), dtype=torch.float64, device="cuda:0")
    ip = torch.zeros((4, 8), dtype=torch.int64, device="cuda:0")
    info = torch.zeros(4, dtype=torch.int64, device="cuda:0")
    h.call("rflu_getrf_batched_f64_dev", 0, 8, 8, ptr(A), 8, 64, 0, ptr(ip), 8, 1, ptr(info))
    for args in ((4, 8, 8, ptr(A), 7, 64, 0, ptr(ip), 8, 1, ptr(info)),          # lda < m
                 (4, 8, 8, ptr(A), 8, 63, 0, ptr(ip), 8, 1, ptr(info)),          # matrices overlap
                 (4, 8, 8, ptr(A), 8, 64, 0, ptr(ip), 7, 1, ptr(info)),          # pivots overlap
                 (4, 8, 8, ptr(A), 8, 64, 0, None, 8, 1, ptr(info)),             # pivoting without ipiv
                 (4, 8, 8, ptr(A), 8, 64, 0, ptr(ip), 8, 1, None),               # no info
                 (4, 8, 8, None, 8, 64, 0, ptr(ip), 8, 1, ptr(info)),
                 (-1, 8, 8, ptr(A), 8, 64, 0, ptr(ip), 8, 1, ptr(info)),
                 (4, -8, 8, ptr(A), 8, 64, 0, ptr(ip), 8, 1, ptr(info))):
        with pytest.raises(rf.RfluError):
            h.call("rflu_getrf_batched_f64_dev", *args)
    B = torch.zeros((4, 8), dtype=torch.float64, device="cuda:0")
    h.call("rflu_getrs_batched_f64_dev", 4, 8, 0, ptr(A), 8, 64, 0, ptr(ip), 8, ptr(B), 8, 8, 0)
    for args in ((4, 8, 1, ptr(A), 8, 64, 0, ptr(ip), 8, ptr(B), 7, 8, 0),       # ldb < n
                 (4, 8, 1, ptr(A), 8, 64, 0, ptr(ip), 8, ptr(B), 8, 7, 0),       # right-hand sides overlap
                 (4, 8, 1, ptr(A), 8, 64, 0, ptr(ip), 8, None, 8, 8, 0),
                 (4, 8, -1, ptr(A), 8, 64, 0, ptr(ip), 8, ptr(B), 8, 8, 0)):
        with pytest.raises(rf.RfluError):
            h.call("rflu_getrs_batched_f64_dev", *args)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 7, 8, 33, 64, 100, 128])
def test_batched_solve_on_diagonally_shifted_matrices(n, dtype):
    """rand + 10 I, nrhs 1 / 3 / 70, forward and transposed, pivoted and NoPivot, both layouts: the reference's bound
    ||A x - b|| < 1000 n eps(T) (test/runtests.jl:124-126) for every matrix of the batch."""
    batch = 100
    D = host_batch(n, n, batch, dtype, diag=True)
    D64 = D.astype(np.float64)
    bound = 1000 * n * np.finfo(dtype).eps
    for pivot in (rf.RowMaximum(), rf.NoPivot()):
        for dev in (dev_cm, dev_rm):
            F = rf.lu_batched_(dev(D), None, pivot)
            assert isinstance(F.ipiv, rf.NotIPIV) == isinstance(pivot, rf.NoPivot)
            for nrhs in (1, 3, 70):
                B = rhs_batch(n, nrhs, batch, dtype)
                for trans in (False, True):
                    dB = dev(B)
                    out = rf.ldiv_batched_(rf.Adjoint(F) if trans and nrhs == 3 else F, dB, trans=trans and nrhs != 3)
                    assert out is dB and rf.last_path() == "hip-batched"
                    Dop = np.transpose(D64, (0, 2, 1)) if trans else D64
                    res = np.linalg.norm(Dop @ host(dB) - B, axis=(1, 2))
                    assert np.all(res < bound), (type(pivot).__name__, dev.__name__, nrhs, trans, res.max(), bound)
                    if nrhs == 1:   # the same as a batch of vectors
                        dv = torch.from_numpy(np.ascontiguousarray(B[:, :, 0])).to("cuda:0")
                        rf.ldiv_batched_(F, dv, trans=trans)
                        assert np.array_equal(host(dv), host(dB)[:, :, 0])


@pytest.mark.parametrize("n", [8, 32, 64, 96, 128])
def test_batched_solve_on_plain_random_matrices(n):
    EPS = np.finfo(np.float64).eps
    batch = 200
    A = host_batch(n, n, 1000, np.float64)[:batch]
    F = rf.lu_batched_(dev_cm(A))
    for nrhs in (1, 5):
        B = rhs_batch(n, nrhs, batch, np.float64)
        for trans in (False, True):
            X = host(rf.ldiv_batched_(F, dev_cm(B), trans=trans))
            Aop = np.transpose(A, (0, 2, 1)) if trans else A
            Xref = np.linalg.solve(Aop, B)
            worst_r = worst_e = 0.0
            for b in range(batch):
                scale = np.linalg.norm(A[b], 2) * np.linalg.norm(Xref[b]) + np.linalg.norm(B[b])
                res = np.linalg.norm(Aop[b] @ X[b] - B[b])
                err = np.linalg.norm(X[b] - Xref[b]) / np.linalg.norm(Xref[b])
                worst_r, worst_e = max(worst_r, res / (1000 * n * EPS * scale)), max(worst_e, err)
                assert res < 1000 * n * EPS * scale, (b, res)
                assert err < 1e-6, (b, err)
            print(f"n={n} nrhs={nrhs} trans={trans}: worst residual {worst_r:.3e} of its bound, worst solution error {worst_e:.3e}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [8, 32, 64, 128])
def test_batched_solve_agrees_with_the_single_matrix_path(n, dtype):
    """ldiv_batched_ on matrix b against lu_ / ldiv_ on the same matrix (plain rand, pivoted, 3 right-hand sides, both directions).
    Float64: 1e-6 relative.  Float32: LAPACK sgetrs against Float64 numpy.linalg.solve on these inputs (n = 8, 32, 64, 128, seeds
    50000 .. 50099, both directions) is off by at most 4.014e-4 relative (n = 64); two Float32 solves may differ by as much from each
    other, and the margin is that figure times 10: 4.0e-3."""
    tol = 1e-6 if dtype == np.float64 else 4.0e-3
    batch = 40
    A = host_batch(n, n, 1000, dtype)[:batch]
    B = rhs_batch(n, 3, batch, dtype)
    F = rf.lu_batched_(dev_cm(A))
    ipb = host(F.ipiv)
    for trans in (False, True):
        X = host(rf.ldiv_batched_(F, dev_cm(B), trans=trans))
        worst = 0.0
        for b in range(batch):
            S = rf.lu_(to_dev_cm(A[b]), None, True)
            assert np.array_equal(host(S.ipiv), ipb[b])
            Y = to_dev_cm(np.asfortranarray(B[b]))
            rf.ldiv_(rf.Adjoint(S) if trans else S, Y)
            y = host(Y)
            worst = max(worst, np.linalg.norm(X[b] - y) / np.linalg.norm(y))
        print(f"n={n} {np.dtype(dtype).name} trans={trans}: worst |x_batched - x_single| / |x_single| = {worst:.3e} (margin {tol:.1e})")
        assert worst < tol


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_singular_matrix_spoils_only_its_own_solution(dtype):
    n, batch, bad = 48, 10, 6
    A = host_batch(n, n, batch, dtype, diag=True).copy()
    A[bad][:, 20] = 0
    with pytest.raises(rf.SingularException) as ei:
        rf.lu_batched_(dev_cm(A))
    assert ei.value.batch_index == bad and ei.value.info == 21
    F = rf.lu_batched_(dev_cm(A), check=False)
    assert not F.issuccess() and host(F.info).tolist() == [21 if b == bad else 0 for b in range(batch)]
    B = rhs_batch(n, 2, batch, dtype)
    with pytest.raises(rf.SingularException) as ei:
        rf.ldiv_batched_(F, dev_cm(B))
    assert ei.value.batch_index == bad
    for trans in (False, True):
        X = host(rf.ldiv_batched_(F, dev_cm(B), trans=trans, check=False))
        finite = np.isfinite(X).all(axis=(1, 2))
        assert finite.tolist() == [b != bad for b in range(batch)]
        Aop = np.transpose(A, (0, 2, 1)) if trans else A
        good = [b for b in range(batch) if b != bad]
        res = np.linalg.norm(Aop[good].astype(np.float64) @ X[good] - B[good], axis=(1, 2))
        assert np.all(res < 1000 * n * np.finfo(dtype).eps)
    # NoPivot reports the same matrix with the sign convention of lu_
    N = host_batch(n, n, batch, dtype, diag=True).copy()
    N[bad] = np.triu(N[bad])
    N[bad][30, 30] = 0
    G = rf.lu_batched_(dev_cm(N), None, rf.NoPivot(), check=False)
    assert int(host(G.info)[bad]) == (-31 if rf.NOPIVOT_NEGATIVE_INFO else 31) and np.count_nonzero(host(G.info)) == 1


@pytest.mark.gpu_exclusive
def test_batched_call_beats_the_loop_over_single_factorizations():
    """2048 matrices of 64 x 64 Float64: the median of 5 batched calls against the median of 3 loops of rflu_getrf_f64_dev over the
    same matrices (what the library offered before).  The loop keeps one workgroup on one of 256 CUs busy at a time and pays a launch
    chain and a synchronisation per matrix, so a batched call that is not at least 16x faster is serving the batch serially."""
    batch, n = 2048, 64
    h = handle()
    src = dev_cm(host_batch(n, n, 1000, np.float64)[np.arange(batch) % 1000])
    work = torch.empty_like(src)
    assert work.stride(1) == 1 and work.stride(0) == n * n
    ipiv = torch.zeros((batch, n), dtype=torch.int64, device="cuda:0")
    info_d = torch.zeros(batch, dtype=torch.int64, device="cuda:0")

    def batched():
        work.copy_(src)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h.call("rflu_getrf_batched_f64_dev", batch, n, n, ptr(work), n, n * n, 0, ptr(ipiv), n, 1, ptr(info_d))
        return time.perf_counter() - t0

    def loop():
        work.copy_(src)
        torch.cuda.synchronize()
        info = ctypes.c_int64(0)
        a0, p0 = work.data_ptr(), ipiv.data_ptr()
        t0 = time.perf_counter()
        for b in range(batch):
            h.call("rflu_getrf_f64_dev", n, n, ctypes.c_void_p(a0 + b * n * n * 8), n, ctypes.c_void_p(p0 + b * n * 8), 1, 0, ctypes.byref(info))
        return time.perf_counter() - t0

    batched()                                          # warm-up: code object load, LDS attribute
    ip_batched = None
    tb = []
    for _ in range(5):
        tb.append(batched())
    ip_batched = ipiv.clone()
    assert h.last_path() == 5 and bool((info_d == 0).all())
    loop()
    tl = [loop() for _ in range(3)]
    assert torch.equal(ipiv, ip_batched)               # the same pivots from both
    t_b, t_l = float(np.median(tb)), float(np.median(tl))
    print(f"2048 x (64 x 64) Float64: batched {t_b * 1e3:.3f} ms, loop {t_l * 1e3:.1f} ms, ratio {t_l / t_b:.1f}x")
    assert t_l / t_b >= 16.0
