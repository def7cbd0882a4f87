"""-m gpu: inv / det / logabsdet from the LU factors (rflu_getri_* / rflu_logabsdet_* and their batched forms, csrc/inverse.hip and
csrc/batched.hip) through inv_ / inv / logabsdet / det / inv_batched / logabsdet_batched and the raw C ABI.

Inputs (tests/inv_cases.py): rand_matrix(n, n, seed=SEEDS.get(n, 91000 + n), dtype) (+ 10 I for NoPivot); matrix b of a batch is
rand_matrix(n, n, seed=93000 + b, dtype).  The module prints one summary line with the worst ratio per kind of check at its end (-s).

Bars.
  * Inverse: with everything promoted to Float64 on the host, rho_R = ||A X - I||_1 / (n eps_T ||A||_1 ||X||_1) and rho_L the same with
    X A; rho <= 1 for every size (LAPACK's xGET03 ratio, whose own acceptance threshold is 30).  numpy.linalg.inv (LAPACK getri) on
    exactly these inputs, both sides: worst rho 0.13 (n = 2, Float64) and 0.071 (n = 2, Float32), for n >= 63 0.0070 (n = 65, Float64)
    and 0.00060 (Float32); on the batch inputs (200 matrices each, n = 1 .. 128) worst 0.50 (n = 1); scripts/inv_cpu_bars.py prints
    the table.  Measured on an MI355X: 0.13 (n = 2, Float64) and 0.071 (Float32), for n >= 63 at most 0.011 (n = 200, Float64) and
    0.012 (n = 129, Float32); batched 0.50 (n = 1), 0.31 (n = 2), 0.11 (n = 7), at most 0.07 from n = 8 on.  The bar hides two orders of
    magnitude: tests/test_gpu_inv_exact.py holds the same entries to exact references.
  * logabsdet, tight (the reduction): against math.fsum(log|u_ii|) over the device's own downloaded factors,
    |d| <= (2 + ceil(log2 n)) eps64 sum|log|u_ii||  (one ulp per log, plus the pairwise-summation bound); sign exactly equal.
  * logabsdet, loose (ties it to A): against numpy.linalg.slogdet of the Float64-promoted A, 8 n eps_T absolute, equal sign.
    oracle.lu factors (the GPU's elimination order) of these inputs stay within 2.0 n eps64 (worst at n = 512: one ulp of the value)
    and 1.9 n eps32 (n = 1025) of the Float64 value (scripts/inv_cpu_bars.py; see SEEDS in tests/inv_cases.py for the four sizes whose default seed
    gives a matrix on which the oracle itself misses this absolute bar)."""
import ctypes
import math
import re

import numpy as np
import pytest
import torch

import recursivefactorization.jl_amd as rf
from gpu_util import handle, ptr, sfx, tdtype, to_dev_cm
from inv_cases import BATCH_CASES, SIZES, VARIANT_SIZES, header_constants, host_batch, matrix   # the inputs: one definition, tests/inv_cases.py

pytestmark = pytest.mark.gpu

W = header_constants()["GETRI_W"]                         # GETRI_W of csrc/rflu_internal.hpp; SIZES holds W-1, W, W+1 and 2W+1
assert {W - 1, W, W + 1, 2 * W + 1} <= set(SIZES)
DTYPES = [np.float64, np.float32]
SENTINEL = -7.25
WORST = {}                                                # kind of check -> (worst rho, where): one summary line per run


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    if WORST:
        print("\ntest_gpu_inv worst rho (bar 1.0): " + "; ".join(f"{k}: {v[0]:.4f} ({v[1]})" for k, v in sorted(WORST.items())))


def record(what, dtype, value):
    key = re.sub(r"\d+", "#", what.replace(np.dtype(dtype).name, "").strip()) + " " + np.dtype(dtype).name
    if value >= WORST.get(key, (-1.0, ""))[0]:
        WORST[key] = (value, what)


def host(t):
    return t.detach().cpu().numpy()


def rho(A, X, dtype):
    """(rho_R, rho_L) in Float64; a non-finite X gives inf."""
    A64, X64 = np.asarray(A, dtype=np.float64), np.asarray(X, dtype=np.float64)
    n = A64.shape[0]
    if not np.isfinite(X64).all():
        return math.inf, math.inf
    scale = n * float(np.finfo(dtype).eps) * np.linalg.norm(A64, 1) * np.linalg.norm(X64, 1)
    eye = np.eye(n)
    return np.linalg.norm(A64 @ X64 - eye, 1) / scale, np.linalg.norm(X64 @ A64 - eye, 1) / scale


def check_inverse(A, X, dtype, what):
    r, l = rho(A, X, dtype)
    print(f"{what}: rho_R = {r:.3e}, rho_L = {l:.3e}")
    record(what, dtype, max(r, l))
    assert r <= 1.0 and l <= 1.0, (what, r, l)


def host_logabsdet(fac, ipiv):
    """(fsum of log|u_ii|, sign, sum of |log|u_ii||) in Float64 from downloaded factors."""
    d = [float(v) for v in np.diagonal(fac)]
    logs = [math.log(abs(v)) for v in d]
    sign = -1.0 if (sum(v < 0 for v in d) + (0 if ipiv is None else int(np.sum(np.asarray(ipiv) != np.arange(1, len(d) + 1))))) % 2 else 1.0
    return math.fsum(logs), sign, math.fsum(abs(v) for v in logs)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_inverse_residuals(n, dtype):
    A = matrix(n, dtype)
    F = rf.lu(to_dev_cm(A))
    buf = F.factors
    X = rf.inv_(F)
    assert X is buf and F.factors is None                 # in place; F is invalid afterwards
    with pytest.raises(ValueError):
        rf.inv_(F)
    check_inverse(A, host(X), dtype, f"n={n} {np.dtype(dtype).name}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", VARIANT_SIZES)
def test_inverse_nopivot(n, dtype):
    A = matrix(n, dtype, diag=True)
    F = rf.lu(to_dev_cm(A), rf.NoPivot())
    assert isinstance(F.ipiv, rf.NotIPIV)
    check_inverse(A, host(rf.inv_(F)), dtype, f"nopivot n={n}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pad", [3, 16])
@pytest.mark.parametrize("n", VARIANT_SIZES)
def test_inverse_padded_leading_dimension(n, pad, dtype):
    """lda = n + 3 (odd: no 16-byte alignment of the columns) and n + 16; rows n .. lda-1 of every column come back bit-identical."""
    A, lda = matrix(n, dtype), n + pad
    store = torch.full((n, lda), SENTINEL, dtype=tdtype(dtype), device="cuda:0")
    V = store.T[:n, :]                                    # n x n, stride (1, lda): column-major with padding
    F0 = rf.lu(to_dev_cm(A))
    V.copy_(F0.factors)                                   # the factors, at a padded leading dimension
    X = rf.inv_(rf.LU(V, F0.ipiv, 0))
    assert X.data_ptr() == store.data_ptr() and X.stride() == (1, lda)
    assert torch.equal(store[:, n:], torch.full((n, pad), SENTINEL, dtype=tdtype(dtype), device="cuda:0"))
    check_inverse(A, host(X), dtype, f"lda=n+{pad} n={n}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", VARIANT_SIZES)
def test_inverse_row_major(n, dtype):
    A, ld = matrix(n, dtype), n + 5
    store = torch.full((n, ld), SENTINEL, dtype=tdtype(dtype), device="cuda:0")
    R = store[:, :n]
    F0 = rf.lu(to_dev_cm(A))
    R.copy_(F0.factors)                                   # the same factors held row-major, rows padded
    X = rf.inv_(rf.LU(R, F0.ipiv, 0))
    assert X.stride() == (ld, 1)
    assert torch.equal(store[:, n:], torch.full((n, 5), SENTINEL, dtype=tdtype(dtype), device="cuda:0"))   # the padding of every row
    check_inverse(A, host(X), dtype, f"row-major n={n}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", VARIANT_SIZES)
def test_inverse_host_entry_copy_and_adjoint(n, dtype):
    A = matrix(n, dtype)
    Fh = rf.lu(np.array(A, order="F"))
    fac_before = Fh.factors.copy()
    Xc = rf.inv(Fh)                                       # the copy leaves F intact
    assert np.array_equal(Fh.factors, fac_before) and Xc is not Fh.factors
    check_inverse(A, Xc, dtype, f"host inv (copy) n={n}")
    Xa = rf.inv(rf.Adjoint(Fh))                           # inv(A') = inv(A)'
    assert np.array_equal(Xa, Xc.T)
    check_inverse(A.T, Xa, dtype, f"host adjoint n={n}")
    assert rf.logabsdet(rf.Adjoint(Fh)) == rf.logabsdet(Fh)
    Xi = rf.inv_(Fh)
    assert np.array_equal(Xi, Xc) and Fh.factors is None
    # the same on the device: inv keeps the factors, Adjoint gives the transposed view
    Fd = rf.lu(to_dev_cm(A))
    keep = Fd.factors.clone()
    Xd = rf.inv(Fd)
    assert torch.equal(Fd.factors, keep)
    check_inverse(A, host(Xd), dtype, f"device inv (copy) n={n}")
    assert torch.equal(rf.inv(rf.Adjoint(Fd)), Xd.T)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [513, 2112])
def test_two_calls_are_bit_identical(n, dtype):
    F = rf.lu(to_dev_cm(matrix(n, dtype)))
    X1, X2 = rf.inv(F), rf.inv(F)
    assert torch.equal(X1, X2)
    assert rf.logabsdet(F) == rf.logabsdet(F)


@pytest.mark.parametrize("dtype", DTYPES)
def test_singular_matrix(dtype):
    n, col = 200, 40
    A = np.array(matrix(n, dtype), order="F")
    A[:, col] = 0
    F = rf.lu(to_dev_cm(A), check=False)
    assert F.info == col + 1
    h, before = handle(), F.factors.clone()
    info = ctypes.c_int64(-1)
    h.call(f"rflu_getri_{sfx(dtype)}_dev", n, ptr(F.factors), F.factors.stride(1), ptr(F.ipiv), ctypes.byref(info))   # RFLU_OK
    assert info.value == F.info and torch.equal(F.factors, before)
    with pytest.raises(rf.SingularException):
        rf.inv_(F)
    with pytest.raises(rf.SingularException) as ei:        # the library's own check, behind a factorization that claims success
        rf.inv_(rf.LU(F.factors, F.ipiv, 0))
    assert ei.value.info == col + 1 and torch.equal(F.factors, before)
    assert rf.logabsdet(F) == (-math.inf, 0.0) and rf.det(F) == 0.0
    fac = host(F.factors).copy()
    fac[3, 3] = np.nan
    G = rf.LU(to_dev_cm(fac), F.ipiv, 0)
    la, sg = rf.logabsdet(G)
    assert math.isnan(la) and math.isnan(sg)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_logabsdet_against_the_downloaded_factors_and_slogdet(n, dtype):
    A = matrix(n, dtype)
    F = rf.lu(to_dev_cm(A))
    la, sg = rf.logabsdet(F)
    want, wsign, mass = host_logabsdet(host(F.factors), host(F.ipiv))
    bar = (2 + math.ceil(math.log2(n))) * float(np.finfo(np.float64).eps) * mass
    print(f"n={n} {np.dtype(dtype).name}: logabs {la!r}, fsum {want!r}, |d| = {abs(la - want):.3e}, bar {bar:.3e}")
    assert sg == wsign and abs(la - want) <= bar
    s64, l64 = np.linalg.slogdet(np.asarray(A, dtype=np.float64))
    loose = 8 * n * float(np.finfo(dtype).eps)
    print(f"    slogdet {l64!r}: |d| = {abs(la - l64):.3e}, bar {loose:.3e}")
    assert sg == s64 and abs(la - l64) <= loose
    with np.errstate(over="ignore"):
        assert rf.det(F) == sg * float(np.exp(np.float64(la)))   # overflows only where the determinant itself does
    if sg > 0:
        assert rf.logdet(F) == la
    else:
        with pytest.raises(ValueError):
            rf.logdet(F)
    # the host entry (diagonal and ipiv only) and row-major factors run the same reduction on the same numbers
    Fh = rf.LU(np.array(host(F.factors), order="F"), host(F.ipiv), 0)
    assert rf.logabsdet(Fh) == (la, sg)
    Fr = rf.LU(F.factors.contiguous(), F.ipiv, 0)
    assert (n == 1 or Fr.factors.stride(1) == 1) and rf.logabsdet(Fr) == (la, sg)


def _dev_batch(A, row_major):
    if row_major:
        return torch.from_numpy(np.array(A, order="C", copy=True)).to("cuda:0")
    return torch.from_numpy(np.array(np.transpose(A, (0, 2, 1)), order="C", copy=True)).to("cuda:0").transpose(1, 2)


def check_batch_inverse(A, X, dtype, what, skip=()):
    A64, X64 = A.astype(np.float64), X.astype(np.float64)
    n = A.shape[1]
    worst = 0.0
    for b in range(A.shape[0]):
        if b in skip:
            continue
        r, l = rho(A64[b], X64[b], dtype)
        worst = max(worst, r, l)
    print(f"{what}: worst rho = {worst:.3e} (n = {n}, {A.shape[0]} matrices)")
    record(f"{what} n={n}", dtype, worst)
    assert worst <= 1.0, (what, worst)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("row_major", [False, True])
@pytest.mark.parametrize("n,batch", BATCH_CASES)
def test_batched_inverse_and_logabsdet(n, batch, row_major, dtype):
    A = host_batch(n, batch, dtype)
    F = rf.lu_batched(_dev_batch(A, row_major))
    before = F.factors.clone()
    X = rf.inv_batched(F)
    assert rf.last_path() == "hip-batched" and torch.equal(F.factors, before)
    assert X.shape == (batch, n, n) and (n == 1 or (X.stride(2) == 1) == row_major)
    check_batch_inverse(A, host(X), dtype, f"batched {'rm' if row_major else 'cm'}")
    assert torch.equal(rf.inv_batched(rf.Adjoint(F)), X.transpose(1, 2))
    la, sg = rf.logabsdet_batched(F)
    la, sg = host(la), host(sg)
    for b in range(batch):                                # bit for bit the single-matrix entry on the same factors
        assert rf.logabsdet(rf.LU(F.factors[b], F.ipiv[b], 0)) == (float(la[b]), float(sg[b])), b
    np.testing.assert_allclose(host(rf.det_batched(F)), sg * np.exp(la), rtol=8 * np.finfo(np.float64).eps)   # two exp routines, a few ulp


@pytest.mark.parametrize("dtype", DTYPES)
def test_batched_singular_matrix_stays_alone(dtype):
    n, batch, bad, col = 33, 200, 100, 5
    A = np.array(host_batch(n, batch, dtype))
    A[bad, :, col] = 0
    F = rf.lu_batched(_dev_batch(A, False), check=False)
    with pytest.raises(rf.SingularException) as ei:
        rf.inv_batched(F)
    assert ei.value.batch_index == bad and ei.value.info == col + 1
    # the library's own info, behind factors that claim success
    G = rf.BatchedLU(F.factors, F.ipiv, torch.zeros_like(F.info))
    with pytest.raises(rf.SingularException) as ei:
        rf.inv_batched(G)
    assert ei.value.batch_index == bad and ei.value.info == col + 1
    X = host(rf.inv_batched(F, check=False))
    assert not np.isfinite(X[bad]).all()
    check_batch_inverse(A, X, dtype, "batched, one singular", skip=(bad,))
    la, sg = (host(t) for t in rf.logabsdet_batched(F))
    assert la[bad] == -math.inf and sg[bad] == 0.0 and np.isfinite(np.delete(la, bad)).all() and (np.abs(np.delete(sg, bad)) == 1).all()
    assert host(rf.det_batched(F))[bad] == 0.0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("row_major", [False, True])
def test_batched_loop_fallback_above_128(row_major, dtype):
    n, batch = 200, 3
    A = host_batch(n, batch, dtype)
    F = rf.lu_batched(_dev_batch(A, row_major))
    X = rf.inv_batched(F)
    check_batch_inverse(A, host(X), dtype, f"loop fallback {'rm' if row_major else 'cm'}")
    la, sg = (host(t) for t in rf.logabsdet_batched(F))
    for b in range(batch):
        assert rf.logabsdet(rf.LU(F.factors[b], F.ipiv[b], 0)) == (float(la[b]), float(sg[b]))


def test_batched_logabsdet_over_several_chunks():
    n, batch = 1100, 2                                    # more than one chunk of 1024 diagonal entries per matrix
    F = rf.lu_batched(_dev_batch(host_batch(n, batch, np.float64), False))
    la, sg = (host(t) for t in rf.logabsdet_batched(F))
    for b in range(batch):
        assert rf.logabsdet(rf.LU(F.factors[b], F.ipiv[b], 0)) == (float(la[b]), float(sg[b]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("row_major", [0, 1])
def test_batched_raw_abi_with_padded_output(row_major, dtype):
    n, batch, ldi = 33, 50, 40
    A = host_batch(n, batch, dtype)
    F = rf.lu_batched(_dev_batch(A, bool(row_major)))
    fac = F.factors if row_major else F.factors.transpose(1, 2)   # the C-contiguous storage
    out = torch.full((batch, n, ldi), SENTINEL, dtype=tdtype(dtype), device="cuda:0")
    info = torch.full((batch,), -1, dtype=torch.int64, device="cuda:0")
    handle().call(f"rflu_getri_batched_{sfx(dtype)}_dev", batch, n, ptr(fac), n, n * n, row_major, ptr(F.ipiv), n, ptr(out), ldi, n * ldi,
                  ptr(info))
    assert not info.any().item()
    assert torch.equal(out[:, :, n:], torch.full((batch, n, ldi - n), SENTINEL, dtype=tdtype(dtype), device="cuda:0"))
    X = host(out[:, :, :n])
    check_batch_inverse(A, X if row_major else np.transpose(X, (0, 2, 1)), dtype, "raw ABI, ldi > n")


@pytest.mark.parametrize("dtype", DTYPES)
def test_raw_abi_argument_checks(dtype):
    h, s = handle(), sfx(dtype)
    lib, n = h.lib, 8
    F = torch.eye(n, dtype=tdtype(dtype), device="cuda:0")
    ip = torch.arange(1, n + 1, dtype=torch.int64, device="cuda:0")
    info, la, sg = ctypes.c_int64(7), ctypes.c_double(5.0), ctypes.c_double(5.0)
    null, ERR_ARG = ctypes.c_void_p(0), 1

    def bad(st):
        assert st == ERR_ARG and lib.rflu_last_error()

    for name in (f"rflu_getri_{s}_dev", f"rflu_getri_rm_{s}_dev", f"rflu_getri_{s}"):
        fn = getattr(lib, name)
        bad(fn(h.ptr, -1, ptr(F), n, ptr(ip), ctypes.byref(info)))
        bad(fn(h.ptr, n, ptr(F), n - 1, ptr(ip), ctypes.byref(info)))
        bad(fn(h.ptr, n, null, n, ptr(ip), ctypes.byref(info)))
        bad(fn(h.ptr, n, ptr(F), n, ptr(ip), null))
        assert fn(h.ptr, 0, null, 1, null, ctypes.byref(info)) == 0 and info.value == 0
        info.value = 7
    for name in (f"rflu_logabsdet_{s}_dev", f"rflu_logabsdet_{s}"):
        fn = getattr(lib, name)
        bad(fn(h.ptr, -1, ptr(F), n, ptr(ip), ctypes.byref(la), ctypes.byref(sg)))
        bad(fn(h.ptr, n, ptr(F), n - 1, ptr(ip), ctypes.byref(la), ctypes.byref(sg)))
        bad(fn(h.ptr, n, null, n, ptr(ip), ctypes.byref(la), ctypes.byref(sg)))
        bad(fn(h.ptr, n, ptr(F), n, ptr(ip), null, ctypes.byref(sg)))
        bad(fn(h.ptr, n, ptr(F), n, ptr(ip), ctypes.byref(la), null))
        assert fn(h.ptr, 0, null, 1, null, ctypes.byref(la), ctypes.byref(sg)) == 0 and (la.value, sg.value) == (0.0, 1.0)
        la.value = sg.value = 5.0
    Fb = torch.eye(n, dtype=tdtype(dtype), device="cuda:0").repeat(2, 1, 1)
    out, ipb = torch.empty_like(Fb), ip.repeat(2, 1)
    infob, dl, ds = torch.zeros(2, dtype=torch.int64, device="cuda:0"), torch.zeros(2, dtype=torch.float64, device="cuda:0"), torch.zeros(2, dtype=torch.float64, device="cuda:0")
    gb, lb = getattr(lib, f"rflu_getri_batched_{s}_dev"), getattr(lib, f"rflu_logabsdet_batched_{s}_dev")
    bad(gb(h.ptr, -1, n, ptr(Fb), n, n * n, 0, ptr(ipb), n, ptr(out), n, n * n, ptr(infob)))
    bad(gb(h.ptr, 2, -1, ptr(Fb), n, n * n, 0, ptr(ipb), n, ptr(out), n, n * n, ptr(infob)))
    bad(gb(h.ptr, 2, n, ptr(Fb), n - 1, n * n, 0, ptr(ipb), n, ptr(out), n, n * n, ptr(infob)))
    bad(gb(h.ptr, 2, n, ptr(Fb), n, n * n - 1, 0, ptr(ipb), n, ptr(out), n, n * n, ptr(infob)))
    bad(gb(h.ptr, 2, n, ptr(Fb), n, n * n, 0, ptr(ipb), n, ptr(out), n - 1, n * n, ptr(infob)))
    bad(gb(h.ptr, 2, n, ptr(Fb), n, n * n, 0, ptr(ipb), n - 1, ptr(out), n, n * n, ptr(infob)))
    bad(gb(h.ptr, 2, n, null, n, n * n, 0, ptr(ipb), n, ptr(out), n, n * n, ptr(infob)))
    bad(gb(h.ptr, 2, n, ptr(Fb), n, n * n, 0, ptr(ipb), n, null, n, n * n, ptr(infob)))
    bad(gb(h.ptr, 2, n, ptr(Fb), n, n * n, 0, ptr(ipb), n, ptr(out), n, n * n, null))
    assert gb(h.ptr, 0, n, null, n, n * n, 0, null, n, null, n, n * n, null) == 0
    assert gb(h.ptr, 2, 0, null, 1, 0, 0, null, 0, null, 1, 0, null) == 0
    bad(lb(h.ptr, -1, n, ptr(Fb), n, n * n, ptr(ipb), n, ptr(dl), ptr(ds)))
    bad(lb(h.ptr, 2, n, ptr(Fb), n - 1, n * n, ptr(ipb), n, ptr(dl), ptr(ds)))
    bad(lb(h.ptr, 2, n, null, n, n * n, ptr(ipb), n, ptr(dl), ptr(ds)))
    bad(lb(h.ptr, 2, n, ptr(Fb), n, n * n, ptr(ipb), n, null, ptr(ds)))
    assert lb(h.ptr, 0, n, null, n, n * n, null, n, null, null) == 0
    # and a well-formed call on the identity: inverse = identity, logabsdet = (0, 1)
    assert gb(h.ptr, 2, n, ptr(Fb), n, n * n, 0, ptr(ipb), n, ptr(out), n, n * n, ptr(infob)) == 0
    assert torch.equal(out, Fb) and not infob.any().item()
    assert lb(h.ptr, 2, n, ptr(Fb), n, n * n, ptr(ipb), n, ptr(dl), ptr(ds)) == 0
    assert host(dl).tolist() == [0.0, 0.0] and host(ds).tolist() == [1.0, 1.0]
