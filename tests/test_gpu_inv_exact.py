"""-m gpu: the real inv / det / logabsdet (rflu_getri_{f64,f32}[_rm]_dev, rflu_getri_*, rflu_getri_batched_*_dev, rflu_logabsdet_*;
getri_view<E> of csrc/inverse.hip and getri_batched_kernel of csrc/batched.hip) held to EXACT references.  tests/test_gpu_inv.py holds
the same entries to a residual bar of 1.0 that a correct inverse meets with two orders of room; here

  * constructed factors (tests/inv_cases.py: exact_case) whose inverse is certified in integer arithmetic come back by `==`: every
    entry and every partial sum of any blocked inverse of them fits Float32 (tests/test_inv_cases.py proves it and shows that a
    skipped inner sweep, forward interchanges, an inverted permutation, exchanged store branches and a lost p1 half all change the
    result at the sizes used), so `==` is a fair demand whatever the blocking and the summation order;
  * padded leading dimensions, a pointer aligned to the element only and the row-major entry give the same bits wherever the GEMM's
    alignment test gives the same answer -- and only there: see test_storage_same_bits_within_a_class_of_alignment;
  * nothing a call leaves on the handle (the diagonal inverses in linv_tmp, which the cooperative solve's exchange area shares; D, Q
    and Hs in inv_work) changes a later call, NaN and Inf included;
  * the batched kernel agrees with the batched solve on an explicit identity -- see test_batched_inverse_against_the_solve_on_an_identity
    for what csrc/batched.hip says about the two.
Every compute call goes through the raw C ABI where a Python wrapper would hide the storage."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import inv_cases as C
import recursivefactorization.jl_amd as rf
from gpu_util import handle, ptr, sfx, tdtype, to_dev_cm
from recursivefactorization.jl_amd import _ffi

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
EPS64 = float(np.finfo(np.float64).eps)
NULL = ctypes.c_void_p(0)


def host(t):
    return t.detach().cpu().numpy()


def dev_ipiv(ipiv):
    return torch.from_numpy(np.array(ipiv, dtype=np.int64)).to("cuda:0")


def getri_dev(h, name, n, buf_ptr, ld, ipiv):
    """One raw call; returns info.  A status other than RFLU_OK raises."""
    info = ctypes.c_int64(-1)
    h.call(name, n, buf_ptr, ld, NULL if ipiv is None else ptr(ipiv), ctypes.byref(info))
    return info.value


def sentinel_like(t):
    return torch.full(t.shape, SENTINEL, dtype=t.dtype, device=t.device)


# ---- 1. exact, single matrix -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("n", C.EXACT_SIZES)
def test_exact_inverse_through_the_device_entries(n, dtype):
    """65, 130: one and two 64-row boundaries below the sweep width; 513: across the 512-wide block column, a last block of one row;
    577: a last block column of 65 rows (the width-64 recursion and the ks < w loop inside a partial block column); 1025: three block
    columns.  Column-major, row-major, and NotIPIV (U^-1 L^-1: the exact inverse with its column permutation undone)."""
    c = C.exact_case(n)
    h, s = handle(), sfx(dtype)
    want, want_nopiv = c.X.astype(dtype), c.Y.astype(dtype)
    ipiv = dev_ipiv(c.ipiv)
    F = to_dev_cm(c.F.astype(dtype))
    assert getri_dev(h, f"rflu_getri_{s}_dev", n, ptr(F), n, ipiv) == 0
    got = host(F)
    assert (got == want).all(), f"column-major n={n}: {(got != want).sum()} entries differ"
    R = torch.from_numpy(np.ascontiguousarray(c.F.astype(dtype))).to("cuda:0")        # the row-major image of the same factors
    assert getri_dev(h, f"rflu_getri_rm_{s}_dev", n, ptr(R), n, ipiv) == 0
    got = host(R)
    assert (got == want).all(), f"row-major n={n}: {(got != want).sum()} entries differ"
    F = to_dev_cm(c.F.astype(dtype))
    assert getri_dev(h, f"rflu_getri_{s}_dev", n, ptr(F), n, None) == 0
    got = host(F)
    assert (got == want_nopiv).all(), f"NotIPIV n={n}: {(got != want_nopiv).sum()} entries differ"
    R = torch.from_numpy(np.ascontiguousarray(c.F.astype(dtype))).to("cuda:0")
    assert getri_dev(h, f"rflu_getri_rm_{s}_dev", n, ptr(R), n, None) == 0
    assert (host(R) == want_nopiv).all(), f"row-major NotIPIV n={n}"


@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("n", [65, 513])
def test_exact_inverse_through_the_host_entry(n, dtype):
    c = C.exact_case(n)
    Fh = np.array(c.F.astype(dtype), order="F")
    ip = np.array(c.ipiv, dtype=np.int64)
    info = ctypes.c_int64(-1)
    handle().call(f"rflu_getri_{sfx(dtype)}", n, ctypes.c_void_p(Fh.ctypes.data), n, ctypes.c_void_p(ip.ctypes.data), ctypes.byref(info))
    assert info.value == 0 and np.array_equal(ip, c.ipiv)
    assert (Fh == c.X.astype(dtype)).all(), f"host entry n={n}: {(Fh != c.X.astype(dtype)).sum()} entries differ"


# ---- 2. storage: the same bits within a class of alignment ---------------------------------------------------------------------------
def vector_class(address, ld, dtype):
    """launch_gemm's `vec_ok` (csrc/gemm.hip) for the GEMMs of getri_view: every one of them has one operand inside the caller's matrix
    -- at an offset of whole 64-row blocks, so aligned as the matrix is -- and the other in a 16-byte aligned workspace whose leading
    dimension is a multiple of 16 elements.  True: 16-byte loads are possible, and K = 64 / 128 products with N <= 2 K go to
    gemm_skinny_kernel; False: every product goes to the tiled kernel with element loads."""
    return address % 16 == 0 and ld % (16 // np.dtype(dtype).itemsize) == 0


@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("n", C.VARIANT_SIZES)
def test_storage_same_bits_within_a_class_of_alignment(n, dtype):
    """The random input of tests/test_gpu_inv.py through the dense call (lda = n), lda = n + 3 and n + 16, a pointer one element past a
    16-byte boundary, and the row-major entry with ld = n + 5; the padding keeps its sentinel everywhere.

    What holds, and is asserted by torch.equal: calls whose storage gives launch_gemm the same answer to its alignment test return the
    same bits -- whatever lda, whatever the entry.  What does NOT hold for the real types (it does for the complex ones, whose GEMM has
    one order of summation): equality across the two classes.  Measured on an MI355X, all six cases: the dense call against
    lda = n + 3 differs in the last bits, because one of the two runs its K = 64 / 128 products through gemm_skinny_kernel, which adds
    the products of a sum in another order than the tiled kernel (n = 65: lda = 65 is odd, lda = 68 is not).  Keeping getri on the tiled
    kernel alone makes all five calls agree bit for bit (tried: 6 of 6 pass) and costs 8 % (n = 8192) to 28 % (n = 512) of the
    Float64 inverse's time and 12 % to 36 % of the Float32 one's (two builds alternating in one process, medians of 8), so it was not
    done and bit-identity across alignments is not claimed for the real path.  Across the classes both results
    meet the residual bar; their largest difference is printed.  Every size meets both classes."""
    h, s, T = handle(), sfx(dtype), tdtype(dtype)
    A = C.matrix(n, dtype)
    F0 = rf.lu(to_dev_cm(A))
    results = {True: [], False: []}

    def column_major(what, buf, address, lda, view, padding):
        assert getri_dev(h, f"rflu_getri_{s}_dev", n, ctypes.c_void_p(address), lda, F0.ipiv) == 0
        for pad in padding:
            assert torch.equal(pad, sentinel_like(pad)), f"{what}: the padding was written"
        results[vector_class(address, lda, dtype)].append((what, view.clone()))

    dense = F0.factors.clone()
    assert dense.stride() == (1, n)
    column_major("dense", dense, dense.data_ptr(), n, dense, [])
    for pad in (3, 16):
        lda = n + pad
        store = torch.full((n, lda), SENTINEL, dtype=T, device="cuda:0")
        store.T[:n, :].copy_(F0.factors)
        column_major(f"lda = n + {pad}", store, store.data_ptr(), lda, store.T[:n, :], [store[:, n:]])
    lda = n + 3                                           # one element past a 16-byte boundary
    buf = torch.full((n * lda + 1,), SENTINEL, dtype=T, device="cuda:0")
    assert buf.data_ptr() % 16 == 0
    view = buf[1:].view(n, lda)
    view.T[:n, :].copy_(F0.factors)
    column_major("pointer one element past a 16-byte boundary", buf, buf.data_ptr() + buf.element_size(), lda, view.T[:n, :], [buf[:1], view[:, n:]])
    ld = n + 5                                            # the row-major entry: the sweeps run in the handle's workspace, which is aligned
    store = torch.full((n, ld), SENTINEL, dtype=T, device="cuda:0")
    store[:, :n].copy_(F0.factors)
    assert getri_dev(h, f"rflu_getri_rm_{s}_dev", n, ptr(store), ld, F0.ipiv) == 0
    assert torch.equal(store[:, n:], sentinel_like(store[:, n:]))
    results[True].append(("row-major, ld = n + 5", store[:, :n].clone()))

    assert results[True] and results[False], "the size does not meet both classes"
    assert not vector_class(buf.data_ptr() + buf.element_size(), lda, dtype)
    for cls, members in results.items():
        first_what, first = members[0]
        r, l = C.rho(A, host(first), dtype)
        print(f"n={n} {np.dtype(dtype).name} {'16-byte loads' if cls else 'element loads'}: {[w for w, _ in members]}: rho_R = {r:.3e}, rho_L = {l:.3e}")
        assert r <= C.RHO_BAR and l <= C.RHO_BAR
        for what, X in members[1:]:
            assert torch.equal(X, first), f"{what} against {first_what}"
    a, b = results[True][0][1], results[False][0][1]
    print(f"    across the classes: bit-identical {torch.equal(a, b)}, largest difference {float((a - b).abs().max().item()):.3e} "
          f"(largest |x| {float(a.abs().max().item()):.3e})")


# ---- 3. state on the handle ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _factors(n, dtype):
    return rf.lu(to_dev_cm(C.matrix(n, dtype)))


def fresh_handle():
    h = _ffi.Handle(0)
    h.set_stream(None)
    return h


def inverse_on(h, n, dtype, factors=None):
    """rflu_getri_*_dev on a copy of the factors of the random n x n input (or of `factors`), on handle h."""
    F = _factors(n, dtype)
    X = (F.factors if factors is None else factors).clone()
    assert getri_dev(h, f"rflu_getri_{sfx(dtype)}_dev", n, ptr(X), n, F.ipiv) == 0
    return X


@functools.lru_cache(maxsize=None)
def quiet_inverse(n, dtype):
    """The same call as the first one a new handle ever sees."""
    h = fresh_handle()
    try:
        return inverse_on(h, n, dtype)
    finally:
        h.close()


@pytest.mark.parametrize("dtype", C.DTYPES)
def test_a_solve_survives_an_inverse_on_the_same_handle(dtype):
    """getri_view keeps its 2 * nb * 64 * 64 elements of diagonal inverses (Ginv, Hinv) at the start of Handle::linv_tmp; the cooperative
    solve (nrhs <= 32) keeps four arrays of nb * 64 * 64 elements there and, behind them, its tagged exchange area.  For the n = 513
    solve nb = 9: the area starts at element 4 * 9 * 4096 = 147456 and is 9 * 64 * 8 granules of 16 bytes = 73728 bytes long, i.e. it ends
    at element 156672 (Float64) or 165888 (Float32).  inv at n = 2112 has nb = 33 and writes 2 * 33 * 4096 = 270336 elements: all of the
    area.  Only `h->trsv_area = nullptr` in getri_view makes the next solve wipe it.  Solves with 1 and with 8 right-hand sides, before and
    after, against the same solves on a handle that has seen nothing else; finite factors throughout."""
    n, big = 513, 2112
    nb, nb_big = (n + C.NB - 1) // C.NB, (big + C.NB - 1) // C.NB
    assert 2 * nb_big * C.NB * C.NB >= 4 * nb * C.NB * C.NB + nb * C.NB * 8 * 16 // np.dtype(dtype).itemsize
    F = _factors(n, dtype)
    A = C.matrix(n, dtype)
    rhs = {k: to_dev_cm(np.asfortranarray(A[:, 5:5 + k])) for k in (1, 8)}

    def solves(h):
        out = {}
        for k, B0 in rhs.items():
            B = B0.clone()
            rf.ldiv_(F, B, handle=h)
            out[k] = B
        return out

    q = fresh_handle()
    try:
        quiet = solves(q)
    finally:
        q.close()
    h = fresh_handle()
    try:
        before = solves(h)
        X = inverse_on(h, big, dtype)
        after = solves(h)
    finally:
        h.close()
    assert torch.equal(X, quiet_inverse(big, dtype))
    for k in rhs:
        assert torch.isfinite(quiet[k]).all()
        assert torch.equal(before[k], quiet[k]) and torch.equal(after[k], quiet[k]), f"{k} right-hand sides"


@pytest.mark.parametrize("dtype", C.DTYPES)
def test_inverses_of_different_sizes_on_one_handle(dtype):
    """2112, then 65, then 513: inv_work (D, Q of the G sweep, then Hs) and linv_tmp (Ginv, Hinv) are sized by the first call and reused
    by the smaller ones at other leading dimensions; each result equals the one a new handle gives."""
    h = fresh_handle()
    try:
        for n in (2112, 65, 513):
            assert torch.equal(inverse_on(h, n, dtype), quiet_inverse(n, dtype)), n
    finally:
        h.close()


@pytest.mark.parametrize("dtype", C.DTYPES)
def test_nan_and_inf_leave_nothing_on_the_handle(dtype):
    """Factors of the n = 1025 input with one NaN in a strictly lower entry and one Inf on U's diagonal: ordinary data for these kernels
    (none of them waits for another workgroup), RFLU_OK, info == 0 (no diagonal entry is zero), a non-finite result.  Its workspaces
    cover those of the next calls -- inv_work: 512 x 1088 elements against 512 x 576 (n = 513) and 128 x 128 (n = 65); linv_tmp:
    2 * 17 * 4096 against 2 * 9 * 4096 and 2 * 2 * 4096 -- which must return the bits of the clean calls made before: nothing of D, Q, Hs,
    Ginv or Hinv leaks."""
    big = 1025
    h = fresh_handle()
    try:
        for n in (513, 65):
            assert torch.equal(inverse_on(h, n, dtype), quiet_inverse(n, dtype)), n
        bad = _factors(big, dtype).factors.clone()
        bad[700, 3] = float("nan")
        bad[40, 40] = float("inf")
        X = inverse_on(h, big, dtype, factors=bad)                              # asserts RFLU_OK and info == 0
        assert not torch.isfinite(X).all()
        for n in (513, 65):
            assert torch.equal(inverse_on(h, n, dtype), quiet_inverse(n, dtype)), f"n={n} after the non-finite call"
    finally:
        h.close()


# ---- 4. exact, batched ---------------------------------------------------------------------------------------------------------------
def exact_positions(batch):
    """Where the exact cases sit in a batch: EXACT_COPIES of them spread over the 67, every other matrix of a small batch."""
    if batch == C.EXACT_BATCH:
        return [5 + 13 * k for k in range(C.EXACT_COPIES)]
    return list(range(0, batch, 2))[:C.EXACT_COPIES]


@functools.lru_cache(maxsize=None)
def mixed_batch(n, batch, dtype):
    """(A, F, ipiv, exact): host arrays of a batch whose members at `exact` (position -> copy) are constructed factors and whose other
    members are the factors rflu_getrf_batched_* made of the random matrices host_batch(n, batch)."""
    A = np.array(C.host_batch(n, batch, dtype))
    G = rf.lu_batched(torch.from_numpy(A).to("cuda:0"))
    F, ipiv = host(G.factors).copy(), host(G.ipiv).copy()
    exact = {}
    for k, b in enumerate(exact_positions(batch)):
        c = C.exact_case(n, k)
        F[b], ipiv[b], A[b] = c.F.astype(dtype), c.ipiv, c.A.astype(dtype)
        exact[b] = k
    return A, F, ipiv, exact


def storage(M, row_major):
    """(batch, n, n) host matrices -> the C-contiguous device buffer of either orientation."""
    return torch.from_numpy(np.ascontiguousarray(M if row_major else np.transpose(M, (0, 2, 1)))).to("cuda:0")


def run_batched(F, ipiv, row_major, dtype, order=None):
    """rflu_getri_batched_*_dev with ldi = n + 3 into a sentinel-filled buffer; returns the inverses as (batch, n, n) host matrices."""
    if order is not None:
        F, ipiv = F[order], ipiv[order]
    batch, n = F.shape[0], F.shape[1]
    ldi = n + 3
    fac, ip = storage(F, row_major), torch.from_numpy(np.ascontiguousarray(ipiv)).to("cuda:0")
    out = torch.full((batch, n, ldi), SENTINEL, dtype=tdtype(dtype), device="cuda:0")
    info = torch.full((batch,), -1, dtype=torch.int64, device="cuda:0")
    h = handle()
    h.call(f"rflu_getri_batched_{sfx(dtype)}_dev", batch, n, ptr(fac), n, n * n, int(row_major), ptr(ip), n, ptr(out), ldi, n * ldi, ptr(info))
    assert h.last_path() == _ffi.PATH_HIP_BATCHED
    assert not info.any().item()
    assert torch.equal(out[:, :, n:], sentinel_like(out[:, :, n:])), "the padding of the output was written"
    X = host(out[:, :, :n])
    return X if row_major else np.transpose(X, (0, 2, 1))


def check_mixed(A, X, exact, dtype, what):
    n = A.shape[1]
    worst = 0.0
    for b in range(A.shape[0]):
        if b in exact:
            want = C.exact_case(n, exact[b]).X.astype(dtype)
            assert (X[b] == want).all(), f"{what}: exact member {b} (copy {exact[b]}): {(X[b] != want).sum()} entries differ"
        else:
            worst = max(worst, *C.rho(A[b], X[b], dtype))
    print(f"{what}: {len(exact)} exact members equal, worst rho of the {A.shape[0] - len(exact)} others = {worst:.3e}")
    assert worst <= C.RHO_BAR, (what, worst)


BATCHED_CASES = [(n, C.EXACT_BATCH) for n in C.BATCHED_EXACT_SIZES] + [(n, b) for n in (33, 64) for b in (1, 7)]


@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("n,batch", BATCHED_CASES)
def test_exact_members_of_a_batch(n, batch, dtype):
    """1 .. 128: both sides of 8 (a pass of BNR columns), of 64 (the p0 / p1 halves of the composed interchanges, threads per matrix)
    and the limit; constructed factors between random ones, both orientations, ldi = n + 3.  The reversed batch gives the reversed
    result, and inv_batched(Adjoint(F)) the transposed one."""
    A, F, ipiv, exact = mixed_batch(n, batch, dtype)
    rev = np.arange(batch)[::-1].copy()
    for row_major in (False, True):
        what = f"n={n} batch {batch} {'rm' if row_major else 'cm'} {np.dtype(dtype).name}"
        X = run_batched(F, ipiv, row_major, dtype)
        check_mixed(A, X, exact, dtype, what)
        Xr = run_batched(F, ipiv, row_major, dtype, order=rev)
        assert np.array_equal(Xr, X[rev]), f"{what}: the reversed batch"
        fac = storage(F, row_major)
        B = rf.BatchedLU(fac if row_major else fac.transpose(1, 2), torch.from_numpy(ipiv).to("cuda:0"),
                         torch.zeros(batch, dtype=torch.int64, device="cuda:0"))
        Xp = rf.inv_batched(B)
        assert rf.last_path() == "hip-batched" and np.array_equal(host(Xp), X)
        Xa = rf.inv_batched(rf.Adjoint(B))
        assert torch.equal(Xa, Xp.transpose(1, 2))
        for b, k in exact.items():
            assert (host(Xa[b]) == C.exact_case(n, k).X.T.astype(dtype)).all(), f"{what}: Adjoint, exact member {b}"


@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("n", [8, 33, 64, 128])
def test_batched_inverse_against_the_solve_on_an_identity(n, dtype):
    """ldiv_batched_ on an explicit identity against inv_batched.  csrc/batched.hip: getri_batched_kernel composes the interchanges
    with the same lines as getrs_batched_kernel, makes row r of a pass as 1 in column sperm[r] -- which IS row sperm[r] of the identity
    that the solve loads -- in the same passes of BNR columns, and calls the same bsubstitute<T, false>; only where the pass comes from
    and where it goes differ.  Found: the identical substitution on identical right-hand sides, so `==` is asserted, in both
    orientations; the largest element-wise difference is printed all the same."""
    batch = C.EXACT_BATCH
    A = C.host_batch(n, batch, dtype)
    for row_major in (False, True):
        dev = torch.from_numpy(np.array(A, order="C", copy=True)).to("cuda:0") if row_major else \
            torch.from_numpy(np.array(np.transpose(A, (0, 2, 1)), order="C", copy=True)).to("cuda:0").transpose(1, 2)
        F = rf.lu_batched(dev)
        X = rf.inv_batched(F)
        eye = torch.eye(n, dtype=tdtype(dtype), device="cuda:0").repeat(batch, 1, 1)      # symmetric: the same buffer in either orientation
        Y = rf.ldiv_batched_(F, eye if row_major else eye.transpose(1, 2))
        assert rf.last_path() == "hip-batched"
        Xh, Yh = host(X), host(Y)
        wx = max(max(C.rho(A[b], Xh[b], dtype)) for b in range(batch))
        wy = max(max(C.rho(A[b], Yh[b], dtype)) for b in range(batch))
        diff = float(np.abs(Xh.astype(np.float64) - Yh.astype(np.float64)).max())
        print(f"n={n} {'rm' if row_major else 'cm'} {np.dtype(dtype).name}: rho inv_batched {wx:.4f}, ldiv_batched_ on I {wy:.4f}, "
              f"largest element-wise difference {diff:.3e} (largest |x| {float(np.abs(Xh).max()):.3e})")
        assert wx <= C.RHO_BAR and wy <= C.RHO_BAR
        assert np.array_equal(Xh, Yh)


# ---- 5. det / logabsdet of the exact inputs ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("n", sorted(set(C.EXACT_SIZES + C.BATCHED_EXACT_SIZES)))
def test_logabsdet_of_the_exact_inputs(n, dtype):
    """det A = sign * 2^k by construction: the sign exactly, log|det| within the tight bar of tests/test_gpu_inv.py,
    (2 + ceil(log2 n)) eps64 sum|log|u_ii||; the batched entry gives the bits of the single one."""
    copies = C.EXACT_COPIES if n in C.BATCHED_EXACT_SIZES else 1
    cases = [C.exact_case(n, k) for k in range(copies)]
    fac = torch.from_numpy(np.ascontiguousarray(np.stack([c.F.T for c in cases]).astype(dtype))).to("cuda:0").transpose(1, 2)
    ipiv = torch.from_numpy(np.stack([c.ipiv for c in cases])).to("cuda:0")
    lab, sgb = rf.logabsdet_batched(rf.BatchedLU(fac, ipiv, torch.zeros(copies, dtype=torch.int64, device="cuda:0")))
    lab, sgb = host(lab), host(sgb)
    for k, c in enumerate(cases):
        la, sg = rf.logabsdet(rf.LU(fac[k], ipiv[k], 0))
        mass = float(np.sum(np.abs(np.diagonal(c.F)) != 1)) * math.log(2.0)
        want = c.log2_absdet * math.log(2.0)
        bar = (2 + math.ceil(math.log2(n))) * EPS64 * mass
        print(f"n={n} copy {k} {np.dtype(dtype).name}: logabs {la!r}, want {want!r}, |d| = {abs(la - want):.3e}, bar {bar:.3e}; sign {sg}, want {c.sign}")
        assert sg == c.sign and abs(la - want) <= bar
        assert (float(lab[k]), float(sgb[k])) == (la, sg)
        assert rf.det(rf.LU(fac[k], ipiv[k], 0)) == sg * float(np.exp(np.float64(la)))
