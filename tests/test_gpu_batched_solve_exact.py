"""-m gpu: the batched solves -- rflu_getrs_batched_{f64,f32}_dev (getrs_batched_kernel, csrc/batched.hip) and
rflu_getrs_batched_{cf64,cf32}_dev (cgetrs_batched_kernel, csrc/batched_complex.hip) -- held to EXACT and rounding-level references.
tests/test_gpu_batched.py and tests/test_gpu_complex_batched.py hold the same entries to residual bars that a correct substitution meets
with orders of magnitude of room; here

  (a) constructed members (tests/batched_solve_cases.py: member -- dense triangles, repeated interchange targets, a small-integer
      solution; tests/test_batched_solve_cases.py proves that every partial sum of either substitution in any order is a Float32 number
      and that each planted fault changes the answer) sit between members that rflu_getrf_batched_* factored from uniform matrices, in
      ONE launch, and come back equal to x_true by `==`; the others meet the bars of (c).  Every n on both sides of 8, 32, 64 and up to
      the limit, nrhs on both sides of one and two passes of BNR = 8, batches of 1, 3, 5 and 67, ipiv given and NULL, every operator
      (real: trans = 2 gives the bits of trans = 1), both orientations; one size above each limit goes through the loop;
  (b) padded lda / strideF / stride_ipiv / ldb / strideB and a B pointer one element past a 16-byte boundary give the bits of the packed
      call, every NaN sentinel behind F, ipiv and B is intact, F and ipiv are unchanged -- for the real entries the first such test;
  (c) on general factors (real pivoting, no diagonal shift) the componentwise backward error omega (numpy.longdouble / clongdouble on
      the rounded factors) meets omega <= n eps (real) / 4 n eps (complex), the derived bounds of tests/test_gpu_solve_exact.py and
      tests/complex_solve_cases.py, and omega <= 16 max(omega_ref, eps / 8) with omega_ref from LAPACK (scipy.linalg.lu_solve) on the
      same factors and right-hand sides, the project's margin and floor: on the CPU the restatement of the kernels' order of summation
      is at most 3.5 times LAPACK's omega (tests/test_batched_solve_cases.py), 16 leaves the factor of four for the fused operations;
  (d) the reversed batch gives the reversed result, two calls give the same bits, and ldiv_batched_ / ldiv_complex_batched_ (trans and
      Adjoint(F)) return the bits of the raw call;
  (e) the special interchange sequences -- the identity, ipiv[k] = n for every k, every k < 64 exchanged with a row >= 64 -- at n = 65 and
      128 by `==` (Float64, Float32, ComplexF32: a ComplexF64 matrix of the kernel has at most 64 rows and no p1 half).
Every compute call goes through the raw C ABI; every buffer is filled with a NaN sentinel before the data goes in.

What is NOT held here: rounding is not exercised by the exact cases (every operation on them is exact: a reciprocal a few ulps off,
or a Float32 product where Float64 was meant, returns the same bits) -- (c) covers that side; the loop above the limit is covered at
one size only.

Measured on an MI355X (all 286 cases pass; the whole file takes 23 s, the slowest case -- ComplexF32, n = 128, nrhs = 17, batch 67 --
2.2 s, most of it the clongdouble products of omega; no other case more than 1.6 s):
  * (a), (b), (d), (e): every constructed member equal to x_true, no exception for any type, operator, orientation, batch or
    interchange sequence; every padded call, reversed batch, repeated call and wrapper returned the bits it had to.  No kernel was
    changed: the tests found no fault in csrc/batched.hip or csrc/batched_complex.hip.
  * (c), worst over n, nrhs and the 67 members, omega / eps and omega / max(omega_ref, eps / 8) per type and operator (bars: n eps resp.
    4 n eps, i.e. 8 .. 128 resp. 32 .. 512 in these units, and 16):
        Float64     N 0.67, 3.99    T 0.79, 4.40
        Float32     N 0.85, 4.47    T 1.07, 3.43
        ComplexF64  N 0.50, 2.49    T 0.57, 2.73    C 0.50, 2.54
        ComplexF32  N 0.70, 4.36    T 0.55, 3.47    C 0.66, 3.26
    The general members of (a) (nrhs up to 17, ipiv NULL included) stay inside the same figures but for ComplexF64 (0.61, 3.80).
  * the loop above the limit (n = 129 / 65, the single-matrix solves): at most 1.17 eps (Float32 T) and 8.08 times LAPACK (Float64 T).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import batched_solve_cases as C
import complex_ref as CR
import recursivefactorization.jl_amd as rf
from gpu_util import handle, ptr
from recursivefactorization.jl_amd import _ffi

pytestmark = pytest.mark.gpu

TD = {"f64": torch.float64, "f32": torch.float32, "cf64": torch.complex128, "cf32": torch.complex64}
NULL = ctypes.c_void_p(0)
IPIV_SENTINEL = -7


def nan_of(sfx):
    return float("nan") if C.KIND[sfx] == "real" else complex(float("nan"), float("nan"))


def host(t):
    return t.detach().cpu().numpy()


def same_bits(X, Y):
    return X.shape == Y.shape and X.dtype == Y.dtype and np.array_equal(CR.bits(X), CR.bits(Y))


def words(t):
    """a tensor as integers, so that NaN sentinels compare equal to themselves"""
    if t.is_complex():
        t = torch.view_as_real(t)
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def all_nan(t):
    return bool(torch.isnan(torch.view_as_real(t) if t.is_complex() else t).all())


def strided(images, ld, stride, lead, sfx):
    """(batch, other, contiguous) host images -> (buffer, view of the images, mask of their elements): a flat NaN-filled device buffer of
    lead + batch * stride elements, member b's image at lead + b * stride with leading dimension ld"""
    batch, od, cd = images.shape
    buf = torch.full((lead + batch * stride,), nan_of(sfx), dtype=TD[sfx], device="cuda:0")
    mask = torch.zeros(buf.shape, dtype=torch.bool, device="cuda:0")
    assert buf.data_ptr() % 16 == 0 and stride >= ld * od and ld >= cd

    def inside(t):
        return t[lead:].view(batch, stride)[:, :ld * od].view(batch, od, ld)[:, :, :cd]

    view = inside(buf)
    view.copy_(torch.from_numpy(np.ascontiguousarray(images)).to("cuda:0"))
    inside(mask).fill_(True)
    return buf, view, mask


def images(M, row_major):
    return np.array(M if row_major else np.transpose(M, (0, 2, 1)), order="C", copy=True)


def raw_solve(sfx, F, ipiv, B, code, row_major, padded=False, batched=True):
    """One call of rflu_getrs_batched_*_dev on NaN-filled buffers: F (batch, n, n), ipiv (batch, n) or None (NULL), B (batch, n, nrhs)
    host arrays.  padded: the storage of part (b).  Asserts the status, the path, every sentinel and that F and ipiv are unchanged;
    returns X (batch, n, nrhs)."""
    batch, n, nrhs = B.shape
    p = 1 if padded else 0
    lda, sip = n + 3 * p, n + p
    sF = lda * n + 5 * p
    cd, od = (nrhs, n) if row_major else (n, nrhs)
    ldb = cd + 2 * p
    sB = ldb * od + 3 * p
    fbuf, _, _ = strided(images(F, row_major), lda, sF, 0, sfx)
    bbuf, bview, bmask = strided(images(B, row_major), ldb, sB, p, sfx)
    bptr = ctypes.c_void_p(bbuf.data_ptr() + p * bbuf.element_size())
    if ipiv is None:
        ipbuf, ipp = None, NULL
    else:
        ipbuf = torch.full((batch, sip), IPIV_SENTINEL, dtype=torch.int64, device="cuda:0")
        ipbuf[:, :n] = torch.from_numpy(np.array(ipiv, dtype=np.int64)).to("cuda:0")
        ipp = ptr(ipbuf)
    fkeep, ipkeep = fbuf.clone(), (None if ipbuf is None else ipbuf.clone())
    h = handle()
    h.call(f"rflu_getrs_batched_{sfx}_dev", batch, n, nrhs, ptr(fbuf), lda, sF, int(row_major), ipp, sip if ipiv is not None else 0,
           bptr, ldb, sB, code)
    if batched:
        assert h.last_path() == _ffi.PATH_HIP_BATCHED
    assert torch.equal(words(fbuf), words(fkeep)), "F was written"
    assert ipbuf is None or torch.equal(ipbuf, ipkeep), "ipiv was written"
    assert all_nan(bbuf[~bmask]), "a sentinel behind B was written"
    X = host(bview)
    return X if row_major else np.ascontiguousarray(np.transpose(X, (0, 2, 1)))


@functools.lru_cache(maxsize=4)
def gpu_factors(n, sfx, batch):
    """rflu_getrf_batched_*_dev on the general matrices 0 .. batch - 1, one launch (a loop above the limit): (F (batch, n, n), ipiv)"""
    A = C.general_batch(n, sfx, batch)
    dA = torch.from_numpy(images(A, False)).to("cuda:0")
    ip = torch.zeros((batch, n), dtype=torch.int64, device="cuda:0")
    info = torch.full((batch,), -1, dtype=torch.int64, device="cuda:0")
    handle().call(f"rflu_getrf_batched_{sfx}_dev", batch, n, n, ptr(dA), n, n * n, 0, ptr(ip), n, 1, ptr(info))
    assert not info.any().item()
    return np.ascontiguousarray(np.transpose(host(dA), (0, 2, 1))), host(ip)


def mixed(n, sfx, batch, given=True, which="random"):
    Fg, ipg = gpu_factors(n, sfx, batch)
    return C.mixed_batch(n, sfx, batch, lambda b: (Fg[b], ipg[b]), given=given, which=which)


WORST = {}   # (part, sfx, op) -> [omega / eps, omega / max(omega_ref, eps / 8)]: the running worst, printed by the tests


def check_rounding(part, sfx, F, ipiv, B, X, op, members, what):
    """both bars of (c) for `members` of the batch"""
    if not members:
        return
    n, eps = F.shape[1], C.eps_of(sfx)
    m = np.asarray(members)
    perm = C.perms_of(ipiv[m], n) if ipiv is not None else np.tile(np.arange(n), (len(m), 1))
    Xref = np.stack([C.lapack_solve(F[b], None if ipiv is None else ipiv[b], B[b], op) for b in m])
    w, wref = C.omega_batch(F[m], perm, B[m], X[m], op), C.omega_batch(F[m], perm, B[m], Xref, op)
    ratio = w / np.maximum(wref, C.FLOOR * eps)
    worst = WORST.setdefault((part, sfx, op), [0.0, 0.0])
    worst[0], worst[1] = max(worst[0], float(w.max() / eps)), max(worst[1], float(ratio.max()))
    print(f"{what} {op}: omega / eps {w.max() / eps:.3f}, omega / max(omega_ref, eps / 8) {ratio.max():.3f} "
          f"(omega_ref / eps {wref.min() / eps:.3f} .. {wref.max() / eps:.3f}); so far ({part}) {sfx} {op}: {worst[0]:.3f}, {worst[1]:.3f}")
    assert np.isfinite(X[m]).all(), what
    assert (w <= C.complex_c(sfx, n) * eps).all(), (what, op, float(w.max() / eps))
    assert (ratio <= C.M_RATIO).all(), (what, op, float(ratio.max()))


def check_exact(X, exact, nrhs, sfx, what):
    for b, c in exact.items():
        want = c.X[:, :nrhs].astype(C.DTYPE[sfx])
        assert (X[b] == want).all(), f"{what}: constructed member {b}: {int((X[b] != want).sum())} of {want.size} entries differ"


def run_mixed(part, sfx, n, nrhs, batch, given, which="random", batched=True, orientations=(False, True)):
    """the mixed batch through every operator and orientation: the constructed members by ==, the others by the bars of (c) (judged
    on the first orientation; the second must return its bits)"""
    kind = C.KIND[sfx]
    F, ipiv, B, exact = mixed(n, sfx, batch, given, which)
    others = [b for b in range(batch) if b not in exact]
    for op in C.OPS[kind]:
        Bop = np.ascontiguousarray(B[op][:, :, :nrhs])
        first = None
        for row_major in orientations:
            what = f"{sfx} n={n} nrhs={nrhs} batch {batch} ipiv {'given' if given else 'NULL'} {which} {'rm' if row_major else 'cm'}"
            X = raw_solve(sfx, F, ipiv, Bop, C.TRANS_CODE[op], row_major, batched=batched)
            check_exact(X, exact, nrhs, sfx, f"{what} {op}")
            if first is None:
                first = X
                check_rounding(part, sfx, F, ipiv, Bop, X, op, others, what)
            elif batched:      # the arithmetic happens in LDS, whatever the caller's layout
                assert same_bits(X, first), f"{what} {op}: not the bits of the other orientation"
            if kind == "real" and op == "T":   # include/rflu.h: the real entries read ANY non-zero value as transposed
                assert same_bits(raw_solve(sfx, F, ipiv, Bop, 2, row_major, batched=batched), X), f"{what}: trans = 2"


# ---- (a) exact members of a batch ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx,n,nrhs,batch,given", [(s, *c) for s in C.SFX for c in C.exact_grid(s)])
def test_exact_members_of_a_batch(sfx, n, nrhs, batch, given):
    run_mixed("a", sfx, n, nrhs, batch, given)


@pytest.mark.parametrize("sfx", C.SFX)
def test_one_size_above_the_limit_goes_through_the_loop(sfx):
    """129 (65 for ComplexF64), batch 3: the loop over the single-matrix path, member b at b * strideF / strideB / stride_ipiv.  The
    real constructed members are those of tests/solve_cases.py (batched_solve_cases.above_member says why); a row-major complex batch
    above the limit is refused by the library (tests/test_gpu_complex_batched.py asserts that), so the complex types run column-major."""
    n = C.ABOVE[sfx]
    for nrhs in (1, 9):
        run_mixed("loop", sfx, n, nrhs, C.ABOVE_BATCH, True, batched=False, orientations=(False, True) if C.KIND[sfx] == "real" else (False,))
        assert handle().last_path() != _ffi.PATH_HIP_BATCHED


# ---- (b) storage ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx", C.SFX)
@pytest.mark.parametrize("nrhs", C.STORAGE_NRHS)
@pytest.mark.parametrize("n", C.STORAGE_N)
def test_padded_storage_gives_the_bits_of_the_packed_call(n, nrhs, sfx):
    """lda = n + 3, strideF = lda * n + 5, stride_ipiv = n + 1, ldb = (contiguous dimension) + 2, strideB = ldb * (other dimension) + 3, B
    one element past a 16-byte boundary; a mixed batch of five.  raw_solve asserts the sentinels and that F and ipiv are unchanged.
    ComplexF64 at 65 and 128 is above its limit: the loop, column-major only."""
    kind, batch = C.KIND[sfx], 5
    loop = n > C.LIMIT[sfx]
    F, ipiv, B, exact = mixed(n, sfx, batch)
    for op in C.OPS[kind]:
        Bop = np.ascontiguousarray(B[op][:, :, :nrhs])
        for row_major in ((False,) if loop else (False, True)):
            what = f"{sfx} n={n} nrhs={nrhs} {'rm' if row_major else 'cm'} {op}"
            X0 = raw_solve(sfx, F, ipiv, Bop, C.TRANS_CODE[op], row_major, batched=not loop)
            X1 = raw_solve(sfx, F, ipiv, Bop, C.TRANS_CODE[op], row_major, padded=True, batched=not loop)
            check_exact(X1, exact, nrhs, sfx, what)
            assert same_bits(X1, X0), f"{what}: the padded call does not return the bits of the packed one"


# ---- (c) rounding level -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx,n", [(s, n) for s in C.SFX for n in C.ROUNDING_N if n <= C.LIMIT[s]])
@pytest.mark.parametrize("nrhs", C.ROUNDING_NRHS)
def test_rounding_level_backward_error(nrhs, sfx, n):
    batch = C.ROUNDING_BATCH
    F, ipiv = gpu_factors(n, sfx, batch)
    assert (ipiv != np.arange(1, n + 1)).any(axis=1).all(), "a member without an interchange"
    B = np.array(C.general_rhs_batch(n, nrhs, sfx, batch))
    for op in C.OPS[C.KIND[sfx]]:
        X = raw_solve(sfx, F, ipiv, B, C.TRANS_CODE[op], False)
        check_rounding("c", sfx, F, ipiv, B, X, op, list(range(batch)), f"{sfx} n={n} nrhs={nrhs} batch {batch}")
        assert same_bits(raw_solve(sfx, F, ipiv, B, C.TRANS_CODE[op], True), X), (op, "row-major")


# ---- (d) order and repetition --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx", C.SFX)
@pytest.mark.parametrize("n", [33, 64])
def test_reversed_batch_and_repeated_call(n, sfx):
    batch, nrhs = 67, 9
    F, ipiv, B, exact = mixed(n, sfx, batch)
    rev = np.arange(batch)[::-1].copy()
    for op in C.OPS[C.KIND[sfx]]:
        Bop = np.ascontiguousarray(B[op][:, :, :nrhs])
        for row_major in (False, True):
            X = raw_solve(sfx, F, ipiv, Bop, C.TRANS_CODE[op], row_major)
            assert same_bits(raw_solve(sfx, F, ipiv, Bop, C.TRANS_CODE[op], row_major), X), (op, row_major, "two calls")
            Xr = raw_solve(sfx, F[rev], ipiv[rev], Bop[rev], C.TRANS_CODE[op], row_major)
            assert same_bits(Xr, np.ascontiguousarray(X[rev])), (op, row_major, "the reversed batch")


def dev_batch(M, row_major):
    t = torch.from_numpy(images(M, row_major)).to("cuda:0")
    return t if row_major else t.transpose(1, 2)


@pytest.mark.parametrize("sfx", C.SFX)
def test_the_wrappers_return_the_bits_of_the_raw_call(sfx):
    """one exact batch (every member constructed) through ldiv_batched_ (trans=True and Adjoint(F)) and ldiv_complex_batched_ (the
    letters N, T, C and Adjoint(F))"""
    n, nrhs, batch = 33, 9, 5
    kind, dtype = C.KIND[sfx], C.DTYPE[sfx]
    cs = [C.member(n, kind, k) for k in range(batch)]
    F, ipiv = np.stack([c.F for c in cs]).astype(dtype), np.stack([c.ipiv for c in cs])
    for row_major in (False, True):
        L = rf.BatchedLU(dev_batch(F, row_major), torch.from_numpy(np.array(ipiv)).to("cuda:0"), torch.zeros(batch, dtype=torch.int64, device="cuda:0"))
        for op in C.OPS[kind]:
            B = np.stack([c.B[op][:, :nrhs] for c in cs]).astype(dtype)
            X = raw_solve(sfx, F, ipiv, B, C.TRANS_CODE[op], row_major)
            assert (X == np.stack([c.X[:, :nrhs] for c in cs]).astype(dtype)).all()
            calls = []
            if kind == "real":
                calls.append(lambda dB: rf.ldiv_batched_(L, dB, trans=op == "T"))
                if op == "T":
                    calls.append(lambda dB: rf.ldiv_batched_(rf.Adjoint(L), dB))
            else:
                calls.append(lambda dB: rf.ldiv_complex_batched_(L, dB, trans=op))
                if op == "C":
                    calls.append(lambda dB: rf.ldiv_complex_batched_(rf.Adjoint(L), dB))
            for call in calls:
                dB = dev_batch(B, row_major)
                assert call(dB) is dB and rf.last_path() == "hip-batched"
                assert same_bits(np.ascontiguousarray(host(dB)), X), (op, row_major)


# ---- (e) the special interchange sequences -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx", ["f64", "f32", "cf32"])
@pytest.mark.parametrize("which", C.INTERCHANGES)
@pytest.mark.parametrize("n", C.SPECIAL_N)
def test_special_interchange_sequences(n, which, sfx):
    run_mixed("e", sfx, n, 9, 5, True, which=which)
