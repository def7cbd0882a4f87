"""-m gpu: inv / det / logabsdet from ComplexF64 / ComplexF32 LU factors (rflu_getri_c* / rflu_logabsdet_c* and the batched logabsdet,
csrc/inverse.hip) through inv_complex_ / inv_complex / logabsdet_complex / det_complex / logdet_complex /
logabsdet_complex_batched / det_complex_batched and the raw C ABI.

Inputs (tests/complex_inv_cases.py): rand_matrix(n, ctype): re and im uniform in [-1/2, 1/2) from numpy.random.default_rng(95000 + n) and
default_rng(96000 + 95000 + n) (SEEDS there replaces 95000 + n for seven sizes and says why), rounded to the element type; + n I for NoPivot; logdet_input(n, ctype): the same with scaled columns, for the comparison with slogdet; exact_case(n): constructed factors, exact inverse.

Bars.
  * Inverse: with everything promoted to complex128 on the host, rho_R = ||A X - I||_1 / (n eps_T ||A||_1 ||X||_1) and rho_L the same
    with X A.  n >= 4: rho <= 1, the bar tests/test_gpu_inv.py holds the real types to.  n <= 3: rho <= 4 -- one complex reciprocal and
    one complex product are bounded by about eight unit roundoffs, which is 4 eps.  numpy.linalg.inv (LAPACK zgetri / cgetri) on exactly
    these inputs, the larger of rho_R and rho_L (python scripts/complex_inv_cpu_bars.py; 65+, 200+, 513+ are the NoPivot inputs):
        n          1      2      3      63     64     65     65+    127    128    129    200    200+   511    512    513    513+   1025   1100   2112
        complex128 0.2500 0.1746 0.1316 0.0194 0.0116 0.0151 0.0438 0.0091 0.0097 0.0130 0.0065 0.0186 0.0062 0.0058 0.0071 0.0099 0.0056 0.0053 0.0026
        complex64  0.0370 0.1042 0.0514 0.0004 0.0004 0.0005 0.0028 0.0001 0.0001 0.0002 0.0001 0.0014 0.0000 0.0000 0.0000 0.0004 0.0000 0.0000 0.0000
    at most 0.044 for n >= 63: a 20-fold margin for the explicit 64x64 inverses and the MFMA summation order.
  * Exact inputs: every entry and every partial sum of any blocked inverse is exactly representable in Float32
    (tests/test_complex_inv_cases.py proves it over complex_inv_cases.partial_sum_bits), so the result equals the exact inverse by `==`.
  * logabsdet, tight (the reduction): against the Float64 sum of log(hypot(re, im)) over the device's own downloaded diagonal taken in
    the KERNEL'S OWN ORDER on the host (complex_inv_cases.kernel_order_logabsdet).  The order is the kernel's, the two libraries' `log`
    and `hypot` are not: each is within one ulp, so the two sums agree within
        (2 + ceil(log2 n)) eps64 sum|log|u_ii||  +  2 n eps64
    (the first term as tests/test_gpu_inv.py has it: one ulp per log on either side and the rounding of the additions; the second: a
    modulus off by one ulp on either side moves its log by eps64).  A bit-for-bit comparison is printed, not asserted: it would test
    the host's libm against the device's.  What IS bit for bit, and asserted: two runs, the host entry against the device entry, and the
    batched entry against the single-matrix one.
  * logabsdet, loose (ties it to A): against numpy.linalg.slogdet of the complex128-promoted A, 8 n eps_T absolute -- the bar
    tests/test_gpu_inv.py uses for the real types.  The input is complex_inv_cases.logdet_input(n, ctype): rand_matrix's matrix with
    its columns scaled by powers of two so that log|det| and the partial sums of log|u_jj| stay small.  The factorization is the
    same one (same pivots, same L, U's columns scaled exactly); what changes is that the reference can carry the bar.  On the unscaled
    matrix it cannot: at n = 2112 in complex128 the bar is four ulps of log|det| = 5135, and measured on an MI355X machine in units of
    n eps64, math.fsum being the exact sum, the device's value was 1.9 from the exact sum over its own diagonal, that sum 3.9 from
    the exact sum over the diagonal of scipy.linalg.lu_factor's (LAPACK zgetrf) factors (||PA - LU||_F / ||A||_F = 3.3e-14 device,
    3.4e-14 LAPACK), and numpy.linalg.slogdet 21.3 from the exact sum over LAPACK's diagonal -- 0.0 on another machine, on the same
    matrix.  The unscaled comparison failed there by 15.5 against 8 for that reason alone.  logdet_input's docstring has the reasoning;
    scripts/complex_inv_cpu_bars.py --logabs prints, for the scaled inputs, slogdet against the exact sum over LAPACK's diagonal (at
    most 1.4 n eps64) and tests/complex_ref.py's unblocked elimination in the element type against slogdet.
  * Phase: against the product of d / |d| over the downloaded diagonal in complex128 (kernel order) times the parity,
    |delta| <= 16 n eps64: n products of at most sqrt(5) unit roundoffs each, plus n normalisations of a few each."""
import ctypes
import math

import numpy as np
import pytest
import torch

import recursivefactorization.jl_amd as rf
import complex_inv_cases as C
from gpu_util import handle, ptr, to_dev_cm

pytestmark = pytest.mark.gpu

EPS64 = float(np.finfo(np.float64).eps)
SENTINEL = complex(-7.25, 3.5)
ERR_ARG = 1


def host(t):
    return t.detach().cpu().numpy()


def tctype(ctype):
    return torch.complex128 if np.dtype(ctype) == np.complex128 else torch.complex64


def bits(t):
    """The words of a complex tensor, for comparisons that are bit for bit."""
    r = torch.view_as_real(t.contiguous())
    return r.view(torch.int64 if r.dtype == torch.float64 else torch.int32)


def check_inverse(A, X, ctype, what):
    r, l = C.rho(A, X, ctype)
    n = A.shape[0]
    print(f"{what}: rho_R = {r:.3e}, rho_L = {l:.3e} (bar {C.rho_bar(n)})")
    assert r <= C.rho_bar(n) and l <= C.rho_bar(n), (what, r, l)


def padded_factors(F, lda, ctype):
    """(store, view): the n x n factors at leading dimension lda inside a sentinel-filled (n, lda) row-major store."""
    n = F.shape[0]
    store = torch.full((n, lda), SENTINEL, dtype=tctype(ctype), device="cuda:0")
    V = store.T[:n, :]
    V.copy_(F)
    return store, V


def logabs_bar(n, mass):
    return (2 + math.ceil(math.log2(max(n, 2)))) * EPS64 * mass + 2 * n * EPS64


@pytest.mark.parametrize("ctype", C.CDTYPES)
@pytest.mark.parametrize("n", C.SIZES)
def test_inverse_residuals(n, ctype):
    A = C.rand_matrix(n, ctype)
    F = rf.lu_complex(to_dev_cm(A))
    buf = F.factors
    X = rf.inv_complex_(F)
    assert X is buf and F.factors is None                 # in place; F is invalid afterwards
    with pytest.raises(ValueError):
        rf.inv_complex_(F)
    check_inverse(A, host(X), ctype, f"n={n} {np.dtype(ctype).name}")


@pytest.mark.parametrize("ctype", C.CDTYPES)
@pytest.mark.parametrize("n", C.EXACT_SIZES)
def test_exact_input_through_the_raw_abi(n, ctype):
    """Constructed factors: pins the order of the interchanges, the absence of any conjugation, and every block boundary."""
    c = C.exact_case(n)
    lda = n + 3
    h, s = handle(), C.csfx(ctype)
    ipiv = torch.from_numpy(np.array(c.ipiv)).to("cuda:0")
    for conj in (False, True):
        Fh = np.conj(c.F) if conj else c.F
        store, V = padded_factors(torch.from_numpy(np.ascontiguousarray(Fh.astype(ctype).T)).to("cuda:0").T, lda, ctype)
        info = ctypes.c_int64(-1)
        h.call(f"rflu_getri_{s}_dev", n, ptr(store), lda, ptr(ipiv), ctypes.byref(info))
        assert info.value == 0
        got = host(store)                                 # (n, lda): row j is column j of the result
        want = np.conj(c.X) if conj else c.X
        assert (got[:, :n].T == want.astype(ctype)).all(), f"n={n} conj={conj}: {(got[:, :n].T != want.astype(ctype)).sum()} entries differ"
        pad = torch.full((n, lda - n), SENTINEL, dtype=tctype(ctype), device="cuda:0")
        assert torch.equal(bits(store[:, n:]), bits(pad))  # beyond the matrix: the sentinel, bit for bit
    assert not (np.conj(c.X) == c.X).all()                 # the conjugated factors gave the conjugated inverse, not the same one


@pytest.mark.parametrize("ctype", C.CDTYPES)
@pytest.mark.parametrize("n", C.VARIANT_SIZES)
def test_layout_padding_and_misaligned_pointer(n, ctype):
    """lda = n + 3, n + 16 and a pointer one real element past a 16-byte boundary: the aligned call's result, bit for bit."""
    A = C.rand_matrix(n, ctype)
    F0 = rf.lu_complex(to_dev_cm(A))
    Xa = rf.inv_complex(F0)
    check_inverse(A, host(Xa), ctype, f"aligned n={n}")
    for pad in (3, 16):
        lda = n + pad
        store, V = padded_factors(F0.factors, lda, ctype)
        X = rf.inv_complex_(rf.LU(V, F0.ipiv, 0))
        assert X.data_ptr() == store.data_ptr() and X.stride() == (1, lda)
        assert torch.equal(bits(store[:, n:]), bits(torch.full((n, pad), SENTINEL, dtype=tctype(ctype), device="cuda:0")))
        assert torch.equal(bits(X.T), bits(Xa.T)), f"lda = n + {pad}"
    # one real element off: through the raw ABI, the buffer handled as real numbers
    lda = n + 3
    store, _ = padded_factors(F0.factors, lda, ctype)
    flat = torch.view_as_real(store).reshape(-1)
    rbuf = torch.full((flat.numel() + 1,), -7.25, dtype=flat.dtype, device="cuda:0")
    rbuf[1:] = flat
    info = ctypes.c_int64(-1)
    handle().call(f"rflu_getri_{C.csfx(ctype)}_dev", n, ctypes.c_void_p(rbuf.data_ptr() + rbuf.element_size()), lda, ptr(F0.ipiv),
                  ctypes.byref(info))
    assert info.value == 0 and rbuf[0].item() == -7.25
    got = torch.view_as_complex(rbuf[1:].clone().reshape(n, lda, 2))
    assert torch.equal(bits(got[:, :n]), bits(Xa.T)), "misaligned pointer"
    assert torch.equal(bits(got[:, n:]), bits(torch.full((n, 3), SENTINEL, dtype=tctype(ctype), device="cuda:0")))


@pytest.mark.parametrize("ctype", C.CDTYPES)
@pytest.mark.parametrize("n", C.VARIANT_SIZES)
def test_inverse_nopivot(n, ctype):
    A = C.rand_matrix(n, ctype, diag=True)
    F = rf.lu_complex(to_dev_cm(A), rf.NoPivot())
    assert isinstance(F.ipiv, rf.NotIPIV)
    check_inverse(A, host(rf.inv_complex_(F)), ctype, f"nopivot n={n}")


@pytest.mark.parametrize("ctype", C.CDTYPES)
def test_host_entry_copy_views_and_a_valid_factorization_afterwards(ctype):
    n = 200
    A = C.rand_matrix(n, ctype)
    Fh = rf.lu_complex(np.array(A, order="F"))
    fac_before = Fh.factors.copy()
    Xc = rf.inv_complex(Fh)                               # the copy leaves F intact
    assert np.array_equal(Fh.factors, fac_before) and Xc is not Fh.factors
    check_inverse(A, Xc, ctype, "host inv_complex (copy)")
    # inv(A') = inv(A)' and inv(transpose(A)) = transpose(inv(A)): the two differ, and neither is the plain result
    Xadj, Xtr = rf.inv_complex(rf.Adjoint(Fh)), rf.inv_complex(Fh, trans="T")
    assert np.array_equal(Xadj, Xc.conj().T) and np.array_equal(Xtr, Xc.T) and not np.array_equal(Xadj, Xtr)
    assert np.array_equal(rf.inv_complex(Fh, trans="C"), Xadj)
    check_inverse(A.conj().T, Xadj, ctype, "host adjoint")
    check_inverse(A.T, Xtr, ctype, "host transpose")
    # on the device: inv_complex keeps F valid -- ldiv_complex_ works afterwards -- and gives the host entry's bits
    Fd = rf.lu_complex(to_dev_cm(A))
    keep = Fd.factors.clone()
    B0 = to_dev_cm(np.asfortranarray(A[:, :3]))
    rf.ldiv_complex_(Fd, B0)
    Xd = rf.inv_complex(Fd)
    assert torch.equal(bits(Fd.factors), bits(keep))
    assert np.array_equal(host(Xd), Xc)
    assert torch.equal(rf.inv_complex(rf.Adjoint(Fd)).resolve_conj(), Xd.T.conj().resolve_conj())
    assert torch.equal(rf.inv_complex(Fd, trans="T"), Xd.T)
    B = to_dev_cm(np.asfortranarray(A[:, :3]))
    rf.ldiv_complex_(Fd, B)                               # the solve before inv_complex, bit for bit
    assert torch.equal(bits(B.T), bits(B0.T))
    Xi = rf.inv_complex_(Fh)
    assert np.array_equal(Xi, Xc) and Fh.factors is None


@pytest.mark.parametrize("ctype", C.CDTYPES)
def test_singular_factors(ctype):
    n, k = 130, 70
    A = C.rand_matrix(n, ctype)
    F0 = rf.lu_complex(to_dev_cm(A))
    fac = host(F0.factors).copy()
    fac[k - 1, k - 1] = 0
    F = rf.LU(to_dev_cm(fac), F0.ipiv, 0)                 # factors that claim success
    h, before = handle(), F.factors.clone()
    info = ctypes.c_int64(-1)
    h.call(f"rflu_getri_{C.csfx(ctype)}_dev", n, ptr(F.factors), F.factors.stride(1), ptr(F.ipiv), ctypes.byref(info))   # RFLU_OK
    assert info.value == k and torch.equal(bits(F.factors), bits(before))
    with pytest.raises(rf.SingularException) as ei:
        rf.inv_complex_(F)
    assert ei.value.info == k and F.factors is not None and torch.equal(bits(F.factors), bits(before))
    assert rf.logabsdet_complex(F) == (-math.inf, 0j) and rf.det_complex(F) == 0j
    # the host entry: info != 0 leaves the host array untouched
    Fh = np.array(fac, order="F")
    info.value = -1
    h.call(f"rflu_getri_{C.csfx(ctype)}", n, ctypes.c_void_p(Fh.ctypes.data), n, ctypes.c_void_p(host(F0.ipiv).ctypes.data), ctypes.byref(info))
    assert info.value == k and Fh.tobytes(order="F") == fac.tobytes(order="F")
    # a zero real part with a non-zero imaginary part is NOT singular
    fac[k - 1, k - 1] = 0.5j
    L, U = np.tril(fac.astype(np.complex128), -1) + np.eye(n), np.triu(fac.astype(np.complex128))
    A2 = np.zeros((n, n), dtype=np.complex128)
    A2[C.perm_of(host(F0.ipiv), n), :] = L @ U
    X = rf.inv_complex_(rf.LU(to_dev_cm(fac), F0.ipiv, 0))
    check_inverse(A2, host(X), ctype, "u_kk = 0 + 0.5i")
    fac[3, 3] = complex(np.nan, 1.0)
    la, sg = rf.logabsdet_complex(rf.LU(to_dev_cm(fac), F0.ipiv, 0))
    assert math.isnan(la) and math.isnan(sg.real) and math.isnan(sg.imag)


@pytest.mark.parametrize("ctype", C.CDTYPES)
@pytest.mark.parametrize("n", [513, 2112])
def test_two_calls_are_bit_identical(n, ctype):
    F = rf.lu_complex(to_dev_cm(C.rand_matrix(n, ctype)))
    X1, X2 = rf.inv_complex(F), rf.inv_complex(F)
    assert torch.equal(bits(X1.T), bits(X2.T))
    assert rf.logabsdet_complex(F) == rf.logabsdet_complex(F)


def check_logabsdet_against_diagonal(la, sg, diag, ipiv, what):
    n = len(diag)
    want, wphase, mass = C.kernel_order_logabsdet(diag, ipiv)
    bar = logabs_bar(n, mass)
    print(f"{what}: logabs {la!r}, host sum in kernel order {want!r}, |d| = {abs(la - want):.3e}, bar {bar:.3e}, bit-identical: {la == want}")
    assert abs(la - want) <= bar
    pbar = 16 * n * EPS64
    print(f"    phase {sg!r}, host product {wphase!r}, |d| = {abs(sg - wphase):.3e}, bar {pbar:.3e}")
    assert abs(sg - wphase) <= pbar and abs(abs(sg) - 1.0) <= 4 * EPS64


@pytest.mark.parametrize("ctype", C.CDTYPES)
@pytest.mark.parametrize("n", C.SIZES)
def test_logabsdet_against_the_downloaded_factors_and_slogdet(n, ctype):
    A = C.logdet_input(n, ctype)
    F = rf.lu_complex(to_dev_cm(A))
    la, sg = rf.logabsdet_complex(F)
    fac, ipiv = host(F.factors), host(F.ipiv)
    check_logabsdet_against_diagonal(la, sg, np.diagonal(fac), ipiv, f"n={n} {np.dtype(ctype).name}")
    s128, l128 = np.linalg.slogdet(np.asarray(A, dtype=np.complex128))
    loose = 8 * n * float(np.finfo(C.real_of(ctype)).eps)
    print(f"    slogdet {l128!r} {s128!r}: |d| = {abs(la - l128):.3e}, bar {loose:.3e}; phase |d| = {abs(sg - s128):.3e}")
    assert abs(la - l128) <= loose
    with np.errstate(over="ignore"):
        assert rf.det_complex(F) == sg * float(np.exp(np.float64(la)))
    assert rf.logdet_complex(F) == complex(la, float(np.angle(sg)))
    # det(A') is the conjugate of det(A); det(transpose(A)) = det(A)
    assert rf.logabsdet_complex(rf.Adjoint(F)) == (la, sg.conjugate()) and rf.logabsdet_complex(F, trans="T") == (la, sg)
    # the host entry (diagonal and ipiv only) runs the same reduction on the same numbers
    assert rf.logabsdet_complex(rf.LU(np.array(fac, order="F"), ipiv, 0)) == (la, sg)


@pytest.mark.parametrize("ctype", C.CDTYPES)
def test_logabsdet_over_several_chunks(ctype):
    """n = 5000: five chunks.  Only the diagonal and ipiv are read, so the `factors` are a diagonal and a list of interchanges."""
    n = 5000
    rng = np.random.default_rng(5000)
    d = ((rng.random(n) - 0.5) + 1j * (rng.random(n) - 0.5)).astype(ctype)
    ipiv = np.minimum(np.arange(1, n + 1) + rng.integers(0, 2, size=n), n).astype(np.int64)
    Fd = torch.zeros((n, n), dtype=tctype(ctype), device="cuda:0")
    Fd.diagonal().copy_(torch.from_numpy(d).to("cuda:0"))
    F = rf.LU(Fd.T, torch.from_numpy(ipiv).to("cuda:0"), 0)
    la, sg = rf.logabsdet_complex(F)
    check_logabsdet_against_diagonal(la, sg, d, ipiv, f"n={n} {np.dtype(ctype).name}")
    assert rf.logabsdet_complex(F) == (la, sg)
    lab, sgb = rf.logabsdet_complex_batched(rf.BatchedLU(Fd.T.unsqueeze(0), F.ipiv.unsqueeze(0), torch.zeros(1, dtype=torch.int64, device="cuda:0")))
    assert (float(host(lab)[0]), complex(host(sgb)[0])) == (la, sg)


@pytest.mark.parametrize("ctype", C.CDTYPES)
@pytest.mark.parametrize("n", C.EXACT_SIZES)
def test_logabsdet_of_the_exact_inputs(n, ctype):
    """det A = 2^k i^q by construction."""
    c = C.exact_case(n)
    F = rf.LU(to_dev_cm(c.F.astype(ctype)), torch.from_numpy(np.array(c.ipiv)).to("cuda:0"), 0)
    la, sg = rf.logabsdet_complex(F)
    d = np.abs(np.diagonal(c.F))
    mass = float(np.sum(d != 1)) * math.log(2.0)
    want = c.log2_absdet * math.log(2.0)
    print(f"n={n}: logabs {la!r}, want {want!r}, |d| = {abs(la - want):.3e}, bar {logabs_bar(n, mass):.3e}; phase {sg!r}, want {c.phase!r}")
    assert abs(la - want) <= logabs_bar(n, mass)
    assert abs(sg - c.phase) <= 16 * n * EPS64


def _dev_batch(A, row_major):
    if row_major:
        return torch.from_numpy(np.array(A, order="C", copy=True)).to("cuda:0")
    return torch.from_numpy(np.array(np.transpose(A, (0, 2, 1)), order="C", copy=True)).to("cuda:0").transpose(1, 2)


@pytest.mark.parametrize("ctype", C.CDTYPES)
@pytest.mark.parametrize("row_major", [False, True])
@pytest.mark.parametrize("n", [1, 7, 33, 64])
def test_batched_logabsdet_equals_the_single_entry(n, row_major, ctype):
    batch = 200
    rng = np.random.default_rng(98000 + n)
    A = ((rng.random((batch, n, n)) - 0.5) + 1j * (rng.random((batch, n, n)) - 0.5)).astype(ctype)
    F = rf.lu_complex_batched(_dev_batch(A, row_major))
    la, sg = rf.logabsdet_complex_batched(F)
    assert la.dtype == torch.float64 and sg.dtype == torch.complex128 and la.shape == sg.shape == (batch,)
    la, sg = host(la), host(sg)
    for b in range(batch):                                # bit for bit the single-matrix entry on the same factors
        Fb = F.factors[b] if not row_major else F.factors[b].T.contiguous().T
        assert rf.logabsdet_complex(rf.LU(Fb, F.ipiv[b], 0)) == (float(la[b]), complex(sg[b])), b
    np.testing.assert_allclose(host(rf.det_complex_batched(F)), sg * np.exp(la), rtol=8 * EPS64)
    lac, sgc = rf.logabsdet_complex_batched(rf.Adjoint(F))
    assert np.array_equal(host(lac), la) and np.array_equal(host(sgc), sg.conj())


def test_batched_logabsdet_over_several_chunks():
    n = 3000
    rng = np.random.default_rng(3000)
    d = (rng.random(n) - 0.5) + 1j * (rng.random(n) - 0.5)
    Fd = torch.zeros((1, n, n), dtype=torch.complex128, device="cuda:0")
    Fd[0].diagonal().copy_(torch.from_numpy(d).to("cuda:0"))
    ipiv = torch.from_numpy(np.minimum(np.arange(1, n + 1) + rng.integers(0, 2, size=n), n).astype(np.int64)).to("cuda:0")
    la, sg = rf.logabsdet_complex_batched(rf.BatchedLU(Fd, ipiv.unsqueeze(0), torch.zeros(1, dtype=torch.int64, device="cuda:0")))
    la, sg = float(host(la)[0]), complex(host(sg)[0])
    assert rf.logabsdet_complex(rf.LU(Fd[0].T, ipiv, 0)) == (la, sg)    # (a diagonal matrix is its own transpose)
    check_logabsdet_against_diagonal(la, sg, d, host(ipiv), "batched n=3000")


@pytest.mark.parametrize("ctype", C.CDTYPES)
def test_logabsdet_special_values(ctype):
    n = 40
    d = np.full(n, 1 + 1j, dtype=ctype)
    ip = torch.arange(1, n + 1, dtype=torch.int64, device="cuda:0")

    def both(diag):
        Fd = torch.zeros((n, n), dtype=tctype(ctype), device="cuda:0")
        Fd.diagonal().copy_(torch.from_numpy(diag).to("cuda:0"))
        single = rf.logabsdet_complex(rf.LU(Fd.T, ip, 0))
        lab, sgb = rf.logabsdet_complex_batched(rf.BatchedLU(Fd.unsqueeze(0), ip.unsqueeze(0), torch.zeros(1, dtype=torch.int64, device="cuda:0")))
        return single, (float(host(lab)[0]), complex(host(sgb)[0]))

    z = d.copy(); z[17] = 0
    single, batched = both(z)
    assert single == (-math.inf, 0j) and batched == (-math.inf, 0j)
    z = d.copy(); z[5] = complex(1.0, np.nan)
    for la, sg in both(z):
        assert math.isnan(la) and math.isnan(sg.real) and math.isnan(sg.imag)
    z = d.copy(); z[9] = complex(0.0, -2.0)               # a zero real part alone is no zero
    (la, sg), _ = both(z)
    assert math.isfinite(la) and abs(abs(sg) - 1) <= 4 * EPS64
    # n == 0
    E = torch.zeros((0, 0), dtype=tctype(ctype), device="cuda:0")
    assert rf.logabsdet_complex(rf.LU(E, ip[:0], 0)) == (0.0, 1 + 0j)
    lab, sgb = rf.logabsdet_complex_batched(rf.BatchedLU(torch.zeros((3, 0, 0), dtype=tctype(ctype), device="cuda:0"),
                                                         torch.zeros((3, 0), dtype=torch.int64, device="cuda:0"),
                                                         torch.zeros(3, dtype=torch.int64, device="cuda:0")))
    assert host(lab).tolist() == [0.0] * 3 and host(sgb).tolist() == [1 + 0j] * 3


@pytest.mark.parametrize("ctype", C.CDTYPES)
def test_raw_abi_argument_checks(ctype):
    h, s = handle(), C.csfx(ctype)
    lib, n = h.lib, 8
    F = torch.eye(n, dtype=tctype(ctype), device="cuda:0")
    Fh = np.eye(n, dtype=ctype, order="F")
    ip = torch.arange(1, n + 1, dtype=torch.int64, device="cuda:0")
    iph = np.arange(1, n + 1, dtype=np.int64)
    info, la, sr, si = ctypes.c_int64(7), ctypes.c_double(5.0), ctypes.c_double(5.0), ctypes.c_double(5.0)
    null = ctypes.c_void_p(0)

    def bad(st):
        assert st == ERR_ARG and lib.rflu_last_error()

    for name, f, p in ((f"rflu_getri_{s}_dev", ptr(F), ptr(ip)), (f"rflu_getri_{s}", ctypes.c_void_p(Fh.ctypes.data), ctypes.c_void_p(iph.ctypes.data))):
        fn = getattr(lib, name)
        bad(fn(h.ptr, -1, f, n, p, ctypes.byref(info)))
        bad(fn(h.ptr, n, f, n - 1, p, ctypes.byref(info)))
        bad(fn(h.ptr, n, null, n, p, ctypes.byref(info)))
        bad(fn(h.ptr, n, f, n, p, null))
        assert fn(h.ptr, 0, null, 1, null, ctypes.byref(info)) == 0 and info.value == 0
        info.value = 7
        assert fn(h.ptr, n, f, n, p, ctypes.byref(info)) == 0 and info.value == 0      # the identity: its own inverse
        info.value = 7
    assert torch.equal(F, torch.eye(n, dtype=tctype(ctype), device="cuda:0")) and np.array_equal(Fh, np.eye(n, dtype=ctype))
    for name, f, p in ((f"rflu_logabsdet_{s}_dev", ptr(F), ptr(ip)), (f"rflu_logabsdet_{s}", ctypes.c_void_p(Fh.ctypes.data), ctypes.c_void_p(iph.ctypes.data))):
        fn = getattr(lib, name)
        out = (ctypes.byref(la), ctypes.byref(sr), ctypes.byref(si))
        bad(fn(h.ptr, -1, f, n, p, *out))
        bad(fn(h.ptr, n, f, n - 1, p, *out))
        bad(fn(h.ptr, n, null, n, p, *out))
        bad(fn(h.ptr, n, f, n, p, null, out[1], out[2]))
        bad(fn(h.ptr, n, f, n, p, out[0], null, out[2]))
        bad(fn(h.ptr, n, f, n, p, out[0], out[1], null))
        assert fn(h.ptr, 0, null, 1, null, *out) == 0 and (la.value, sr.value, si.value) == (0.0, 1.0, 0.0)
        la.value = sr.value = si.value = 5.0
        assert fn(h.ptr, n, f, n, p, *out) == 0 and (la.value, sr.value, si.value) == (0.0, 1.0, 0.0)
        la.value = sr.value = si.value = 5.0
    Fb = torch.eye(n, dtype=tctype(ctype), device="cuda:0").repeat(2, 1, 1)
    ipb = ip.repeat(2, 1)
    dl, ds = torch.full((2,), 5.0, dtype=torch.float64, device="cuda:0"), torch.full((4,), 5.0, dtype=torch.float64, device="cuda:0")
    lb = getattr(lib, f"rflu_logabsdet_batched_{s}_dev")
    bad(lb(h.ptr, -1, n, ptr(Fb), n, n * n, ptr(ipb), n, ptr(dl), ptr(ds)))
    bad(lb(h.ptr, 2, -1, ptr(Fb), n, n * n, ptr(ipb), n, ptr(dl), ptr(ds)))
    bad(lb(h.ptr, 2, n, ptr(Fb), n - 1, n * n, ptr(ipb), n, ptr(dl), ptr(ds)))
    bad(lb(h.ptr, 2, n, ptr(Fb), n, n * n - 1, ptr(ipb), n, ptr(dl), ptr(ds)))
    bad(lb(h.ptr, 2, n, ptr(Fb), n, n * n, ptr(ipb), n - 1, ptr(dl), ptr(ds)))
    bad(lb(h.ptr, 2, n, null, n, n * n, ptr(ipb), n, ptr(dl), ptr(ds)))
    bad(lb(h.ptr, 2, n, ptr(Fb), n, n * n, ptr(ipb), n, null, ptr(ds)))
    bad(lb(h.ptr, 2, n, ptr(Fb), n, n * n, ptr(ipb), n, ptr(dl), null))
    assert lb(h.ptr, 0, n, null, n, n * n, null, n, null, null) == 0
    assert lb(h.ptr, 2, n, ptr(Fb), n, n * n, ptr(ipb), n, ptr(dl), ptr(ds)) == 0
    assert host(dl).tolist() == [0.0, 0.0] and host(ds).tolist() == [1.0, 0.0, 1.0, 0.0]
    assert lb(h.ptr, 2, 0, null, 1, 0, null, 0, ptr(dl), ptr(ds)) == 0                 # n == 0: the empty product for every matrix
    assert host(dl).tolist() == [0.0, 0.0] and host(ds).tolist() == [1.0, 0.0, 1.0, 0.0]
