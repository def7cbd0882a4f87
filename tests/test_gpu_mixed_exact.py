"""-m gpu: the real mixed-precision solve (rflu_mixed_getrf_f64_dev / rflu_mixed_getrs_f64_dev / rflu_residual_f64_dev; csrc/mixed.hip and
mixed_getrf / mixed_refine of csrc/driver.cpp) held to EXACT references.  tests/test_gpu_mixed.py accepts any run that reaches dsgesv's
rule within 10 steps, and refinement repairs what is wrong underneath it; here every comparison is `==`:

  A. the Float32 image that demote_relayout_kernel<VIN, VOUT> writes, element by element, through inputs whose factorization does no
     arithmetic on it (upper triangular; unit lower triangular with small multipliers), in all four variants of the kernel, with the
     padding of both matrices under sentinels, and ||A||_inf against the exact largest row sum; n = 1 for the values no larger matrix can
     hold: overflow, NaN and the Float32 subnormal range;
  B. the refinement loop step by step on constructed factors: c_k = 1 gives iters == 0 and x0, c_k = 1 + 2^-30 gives iters == 1 and
     c_k x0, mixed columns catch a wrong column, a rule that reads one column, a double update and an iters that is off by one; both
     residual paths, odd leading dimensions and unaligned pointers give the same bits; nothing stays on the handle after a NaN;
  C. the residual alone on small integers against int64 arithmetic.
Inputs, references and why each is exact: tests/mixed_cases.py, proved on the CPU by tests/test_mixed_cases.py.  Every call goes through
the raw C ABI."""
import ctypes

import numpy as np
import pytest
import torch

import mixed_cases as mc
from gpu_util import Store, handle, ptr
from recursivefactorization.jl_amd import _ffi

pytestmark = pytest.mark.gpu


def fresh_handle():
    h = _ffi.Handle(0)
    h.set_stream(None)
    return h


@pytest.fixture
def residual_path(request, monkeypatch):
    """RFLU_MIXED_GEMV_MAX_RHS as tests/test_gpu_mixed.py::test_residual_kernel_alone sets it; the default handle gets its own value back"""
    monkeypatch.setenv("RFLU_MIXED_GEMV_MAX_RHS", "1000000" if request.param == "residual_few" else "0")
    h = handle()
    h.reload_tuning()
    yield request.param
    monkeypatch.undo()
    h.reload_tuning()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- A. the demoted image ------------------------------------------------------------------------------------------------------------
def demote_variant(a_address, lda, f_address, ldf):
    """launch_demote_relayout's choice (csrc/mixed.hip): VIN = 16-byte loads of two adjacent rows of a column of A, possible when A sits
    on a 16-byte boundary and lda is even; VOUT = float4 stores of four adjacent columns of a row of F32, possible when F32 sits on a
    16-byte boundary and ldf is a multiple of 4."""
    return a_address % 16 == 0 and lda % 2 == 0, f_address % 16 == 0 and ldf % 4 == 0


def a_store(A, vin):
    n = A.shape[0]
    return Store(A, n + 2 - n % 2, off=0) if vin else Store(A, n + 1 + n % 2, off=1)       # even lda on a boundary / odd lda, 8 bytes off


def f_store(n, vout):
    blank = np.full((n, n), -7.25)
    return Store(blank, (n + 3) // 4 * 4 + 4, np.float32, off=0, row_major=True) if vout else Store(blank, n + 3, np.float32, off=1, row_major=True)


def mixed_getrf(h, n, sA, sF, name="rflu_mixed_getrf_f64_dev"):
    ipiv = torch.zeros(n, dtype=torch.int64, device="cuda:0")
    info, anorm = ctypes.c_int64(-1), ctypes.c_double(-1.0)
    args = (n, sA.ptr, sA.ld, sF.ptr, sF.ld, ptr(ipiv), 1) + ((0,) if "_f64_" in name else ()) + (ctypes.byref(anorm), ctypes.byref(info))
    h.call(name, *args)
    return ipiv.cpu().numpy(), anorm.value, info.value


@pytest.mark.parametrize("n", mc.DEMOTE_SIZES)
def test_demoted_image_element_by_element(n):
    """Both inputs of mixed_cases.demote_input through the four VIN x VOUT variants: the part of F32 that the factorization leaves alone
    equals numpy's IEEE conversion, the rest is what the elimination of a triangular matrix leaves (zeros, a unit diagonal), ipiv is the
    identity, info 0, ||A||_inf the exact largest row sum; A comes back bit for bit, padding included, and the padding of F32 keeps
    its sentinel.  Zeros are compared by value: -0 - (-0) may flip a sign."""
    h = handle()
    for kind in ("upper", "lower"):
        A = mc.demote_input(n, kind)
        want, vis, exact = mc.expected_image(A), mc.visible(kind)(n), mc.exact_anorm(A)
        whole = want if kind == "upper" else np.tril(want, -1) + np.eye(n, dtype=np.float32)
        seen = set()
        for vin in (True, False):
            for vout in (True, False):
                sA, sF = a_store(A, vin), f_store(n, vout)
                assert demote_variant(sA.address, sA.ld, sF.address, sF.ld) == (vin, vout)
                seen.add((vin, vout))
                A0 = sA.raw()
                ipiv, anorm, info = mixed_getrf(h, n, sA, sF)
                got = sF.get()
                what = f"n={n} {kind} VIN={vin} VOUT={vout}"
                bad = np.argwhere((got != want) & vis)
                assert bad.size == 0, f"{what}: {len(bad)} elements of the image differ, the first at {bad[0]}: {got[tuple(bad[0])]!r} for {want[tuple(bad[0])]!r}"
                assert np.array_equal(got, whole), f"{what}: outside the image"
                assert info == 0 and np.array_equal(ipiv, np.arange(1, n + 1)), what
                assert anorm == exact, f"{what}: anorm {anorm!r}, exact {exact!r}"
                assert same_bits(sA.raw(), A0), f"{what}: A was written"
                assert sF.padding_intact(), f"{what}: the padding of F32 was written"
        assert len(seen) == 4


F32_MAX = float(np.finfo(np.float32).max)
SPECIAL = [
    ("overflow to +Inf", 1e39), ("overflow to -Inf", -1e39),
    ("FLT_MAX + half an ulp: the tie goes to Inf", F32_MAX + 2.0 ** 103), ("the largest value that rounds to FLT_MAX", np.nextafter(F32_MAX + 2.0 ** 103, 0.0)),
    ("-(FLT_MAX + half an ulp)", -(F32_MAX + 2.0 ** 103)), ("FLT_MAX", F32_MAX), ("NaN", float("nan")),
    ("2^-149, the smallest subnormal", 2.0 ** -149), ("2^-150: the tie goes to zero", 2.0 ** -150), ("3 * 2^-150: the tie goes to 2^-148", 3 * 2.0 ** -150),
    ("just above 2^-150", np.nextafter(2.0 ** -150, 1.0)), ("2^-127, a subnormal", 2.0 ** -127), ("-2^-127", -(2.0 ** -127)),
    ("FLT_MIN - half an ulp: the tie goes to FLT_MIN", 2.0 ** -126 - 2.0 ** -150), ("the largest subnormal", 2.0 ** -126 - 2.0 ** -149),
]


@pytest.mark.parametrize("what,v", SPECIAL, ids=[w for w, _ in SPECIAL])
def test_special_values_convert_as_ieee(what, v):
    """n = 1: one call per value, no arithmetic touches it.  The reference is numpy's IEEE conversion: overflow and the tie at
    FLT_MAX + half an ulp to Inf, NaN stays NaN, and GRADUAL underflow: a Float64 in the Float32 subnormal range becomes the nearest
    subnormal (ties to even), not zero -- include/rflu.h states it.  info is that of the Float32 factorization: 1 where the image is
    zero.  Through the scalar forms (lda = ldf = 1) and, with padding, through the 16-byte forms."""
    h = handle()
    want = mc.expected_image(np.array([[v]]))
    for vin, vout in ((False, False), (True, True)):
        sA = Store(np.array([[v]]), 2 if vin else 1)
        sF = Store(np.array([[-7.25]]), 4 if vout else 1, np.float32, row_major=True)
        assert demote_variant(sA.address, sA.ld, sF.address, sF.ld) == (vin, vout)
        ipiv, anorm, info = mixed_getrf(h, 1, sA, sF)
        got = sF.get().astype(np.float32)
        print(f"{what}: {v!r} -> {got[0, 0]!r} (numpy: {want[0, 0]!r}), anorm {anorm!r}, info {info}")
        assert same_bits(got, want) or (np.isnan(want[0, 0]) and np.isnan(got[0, 0])), f"{what}: {got[0, 0]!r}, numpy gives {want[0, 0]!r}"
        assert info == (1 if want[0, 0] == 0 else 0) and ipiv[0] == 1
        assert anorm == abs(v) or (np.isnan(v) and np.isnan(anorm))
        assert sF.padding_intact()


# ---- B. the refinement loop ----------------------------------------------------------------------------------------------------------
def refine_stores(c, aligned):
    """(A, F32, ipiv) of a case on the device: dense on 16-byte boundaries, or lda = n + odd, ldf = n + 3 and pointers one word off"""
    n = c.n
    if aligned:
        sA, sF = Store(c.A, n), Store(c.F32, n, c.F32.real.dtype, row_major=True)
    else:
        sA, sF = Store(c.A, n + 1 + n % 2, off=1), Store(c.F32, n + 3, c.F32.real.dtype, off=1, row_major=True)
    return sA, sF, torch.from_numpy(np.array(c.ipiv)).to("cuda:0")


def mixed_getrs(h, c, stores, B, max_iter=30, aligned=True, name="rflu_mixed_getrs_f64_dev"):
    """One raw call; returns (X, iters) and asserts that B and the paddings are as they were."""
    sA, sF, ipiv = stores
    n, nrhs = B.shape
    blank = np.full((n, nrhs), -7.25 * (1 + 1j) if np.iscomplexobj(B) else -7.25)
    sB, sX = (Store(B, n), Store(blank, n)) if aligned else (Store(B, n + 3 + n % 2, off=1), Store(blank, n + 5 + n % 2, off=1))
    B0 = sB.raw()
    iters = ctypes.c_int(-99)
    h.call(name, n, nrhs, sA.ptr, sA.ld, sF.ptr, sF.ld, ptr(ipiv), c.anorm, sB.ptr, sB.ld, sX.ptr, sX.ld, max_iter, ctypes.byref(iters))
    assert same_bits(sB.raw(), B0) and sX.padding_intact()
    return sX.get(), iters.value


def explain(X, want):
    bad = np.argwhere(X != want)
    return f"{len(bad)} of {X.size} entries differ, columns {sorted(set(bad[:, 1].tolist()))[:8]}" if bad.size else ""


def check_refinement_steps(h, case, s, n, name):
    """Every nrhs of the case list at one n: all patterns, max_iter = 1, and the unaligned storage."""
    for nrhs in mc.REFINE_NRHS:
        c = case(n, nrhs)
        dense, odd = refine_stores(c, True), refine_stores(c, False)
        A0, F0 = dense[0].raw(), dense[1].raw()
        for pattern in mc.PATTERNS:
            B, want, mask = c.rhs(pattern, s)
            steps = 1 if mask.any() else 0
            what = f"n={n} nrhs={nrhs} {pattern}"
            X, iters = mixed_getrs(h, c, dense, B, name=name)
            assert iters == steps, f"{what}: iters = {iters}, {steps} expected"
            assert np.array_equal(X, want), f"{what}: {explain(X, want)}"
            if pattern == "mixed_a":
                X1, iters = mixed_getrs(h, c, dense, B, max_iter=1, name=name)
                assert iters == steps and same_bits(X1, X), f"{what} with max_iter = 1: iters = {iters}"
                Xo, iters = mixed_getrs(h, c, odd, B, aligned=False, name=name)
                assert iters == steps and same_bits(Xo, X), f"{what}, odd leading dimensions and unaligned pointers: iters = {iters}, {explain(Xo, want)}"
        assert same_bits(dense[0].raw(), A0) and same_bits(dense[1].raw(), F0)          # A and F32 are only read
        assert odd[0].padding_intact() and odd[1].padding_intact()


@pytest.mark.parametrize("residual_path", ["residual_few", "gemm"], indirect=True)
@pytest.mark.parametrize("n", mc.REFINE_N)
def test_refinement_step_by_step(n, residual_path):
    """mixed_cases.refine_case through rflu_mixed_getrs_f64_dev with B[:, k] = c_k A x0[:, k], c_k in {1, 1 + 2^-30}.
    'none': the Float32 solve between the two conversions returns x0 and the residual is exactly 0: iters == 0.  Scaled columns need
    exactly one step.  mixed_a scales the first, the last and every third column, mixed_b the others: an update that lands in another
    column, a rule that reads the first or the last column alone, an update applied twice and an iters off by one all change X or iters
    (tests/test_mixed_cases.py shows it on the restated loop)."""
    check_refinement_steps(handle(), mc.refine_case, mc.S_REAL, n, "rflu_mixed_getrs_f64_dev")


def check_handle_state(case, s, name, big=(513, 65), small=(65, 1)):
    h = fresh_handle()
    try:
        c = case(*big)
        B, want, _ = c.rhs("mixed_a", s)
        X, iters = mixed_getrs(h, c, refine_stores(c, True), B, name=name)
        assert iters == 1 and np.array_equal(X, want), explain(X, want)
        bad = np.array(B)
        bad[3, 2] = np.nan
        X, iters = mixed_getrs(h, c, refine_stores(c, True), bad, max_iter=2, name=name)
        assert iters < 0, iters
        assert np.isnan(X[:, 2]).any()
        c = case(*small)
        for pattern in ("all", "none"):
            B, want, mask = c.rhs(pattern, s)
            X, iters = mixed_getrs(h, c, refine_stores(c, True), B, name=name)
            assert iters == int(mask.any()) and np.array_equal(X, want), f"after the NaN call, {pattern}: iters = {iters}, {explain(X, want)}"
    finally:
        h.close()


def test_nothing_stays_on_the_handle():
    """One handle: n = 513 with 65 right-hand sides, then the same call with a NaN in B (never convergence: iters < 0), then n = 65 with
    one right-hand side, which must still come back by ==: nothing of mixed_rhs, mixed_r, mixed_part or the norms leaks into it."""
    check_handle_state(mc.refine_case, mc.S_REAL, "rflu_mixed_getrs_f64_dev")


# ---- C. the residual alone -----------------------------------------------------------------------------------------------------------
def check_residual(h, n, cplx, name):
    A, X, B, R = mc.residual_case(n, cplx)
    for aligned in (True, False):
        ld = (lambda pad: n + 2 - n % 2) if aligned else (lambda pad: n + pad + n % 2)      # even on a boundary / odd, one word off
        off = 0 if aligned else 1
        sA, sX, sB = Store(A, ld(1), off=off), Store(X, ld(3), off=off), Store(B, ld(5), off=off)
        assert cplx or (sA.address % 16 == 0 and sA.ld % 2 == 0) == aligned                 # launch_residual_few's `vec`
        for nrhs in mc.RESIDUAL_NRHS:
            sR = Store(np.full((n, nrhs), -7.25 * (1 + 1j) if cplx else -7.25), ld(7), off=off)
            h.call(name, n, nrhs, sA.ptr, sA.ld, sX.ptr, sX.ld, sB.ptr, sB.ld, sR.ptr, sR.ld)
            got = sR.get()
            assert np.array_equal(got, R[:, :nrhs]), f"n={n} nrhs={nrhs} aligned={aligned}: {explain(got, R[:, :nrhs])}"
            assert sR.padding_intact()


@pytest.mark.parametrize("residual_path", ["residual_few", "gemm"], indirect=True)
@pytest.mark.parametrize("n", mc.RESIDUAL_N)
def test_residual_of_small_integers_is_exact(n, residual_path):
    """R == B - A X in int64 for |entries| <= 4: every slice's share and every combine order is an exact integer, so a wrong row, a lost
    column slice or a share added twice shows, which the componentwise (n + 2) eps bar of tests/test_gpu_mixed.py need not see."""
    check_residual(handle(), n, False, "rflu_residual_f64_dev")
