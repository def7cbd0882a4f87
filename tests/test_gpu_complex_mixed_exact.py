"""-m gpu: the complex mixed-precision solve (rflu_mixed_getrf_cf64_dev / rflu_mixed_getrs_cf64_dev / rflu_residual_cf64_dev;
csrc/mixed.hip and mixed_getrf / mixed_refine of csrc/driver.cpp) held to EXACT references: the complex counterpart of
tests/test_gpu_mixed_exact.py, whose parts A, B and C it follows and whose helpers it uses.  Inputs: tests/complex_mixed_cases.py
(cdemote_input, crefine_case) and tests/mixed_cases.py (residual_case), proved on the CPU by tests/test_complex_mixed_cases.py and
tests/test_mixed_cases.py.  Every comparison is `==` except the norm of the random family, which keeps the (n + 2) eps bar of
tests/test_gpu_complex_mixed.py: hypot of two nonzero parts rounds."""
import numpy as np
import pytest

import complex_mixed_cases as cm
import mixed_cases as mc
from gpu_util import Store, handle
from test_gpu_mixed_exact import check_handle_state, check_refinement_steps, check_residual, mixed_getrf, residual_path, same_bits  # noqa: F401

pytestmark = pytest.mark.gpu

GETRF, GETRS, RESIDUAL = "rflu_mixed_getrf_cf64_dev", "rflu_mixed_getrs_cf64_dev", "rflu_residual_cf64_dev"


# ---- A. the demoted image ------------------------------------------------------------------------------------------------------------
def cdemote_variant(a_address, f_address, ldf):
    """launch_demote_relayout<CplxElem<double>>'s choice (csrc/mixed.hip): VIN = one 16-byte load per element of A, possible when A sits on a
    16-byte boundary, whatever lda (an element is 16 bytes); VOUT = float4 stores of two adjacent elements of a row of F32, possible
    when F32 sits on a 16-byte boundary and ldf is even."""
    return a_address % 16 == 0, f_address % 16 == 0 and ldf % 2 == 0


def ca_store(A, vin):
    n = A.shape[0]
    return Store(A, n + 1, off=0) if vin else Store(A, n + 2, off=1)                      # on a boundary / 8 bytes off


def cf_store(n, vout):
    blank = np.full((n, n), -7.25 * (1 + 1j))
    return Store(blank, n + 2 - n % 2, np.float32, off=0, row_major=True) if vout else Store(blank, n + 3, np.float32, off=1, row_major=True)


@pytest.mark.parametrize("fam", ["random", "axis"])
@pytest.mark.parametrize("n", cm.CDEMOTE_SIZES)
def test_demoted_image_element_by_element(n, fam):
    """As the real test, with both parts of every element; ||A||_inf by == for the on-axis family (every modulus is exact), within
    (n + 2) eps for the random one, and the same bits from all four variants either way."""
    h = handle()
    for kind in ("upper", "lower"):
        A = cm.cdemote_input(n, kind, fam)
        want, vis = cm.expected_cimage(A), mc.visible(kind)(n)
        whole = want if kind == "upper" else np.tril(want, -1) + np.eye(n, dtype=np.complex64)
        norms = []
        for vin in (True, False):
            for vout in (True, False):
                sA, sF = ca_store(A, vin), cf_store(n, vout)
                assert cdemote_variant(sA.address, sF.address, sF.ld) == (vin, vout)
                A0 = sA.raw()
                ipiv, anorm, info = mixed_getrf(h, n, sA, sF, GETRF)
                got = sF.get()
                what = f"n={n} {fam} {kind} VIN={vin} VOUT={vout}"
                bad = np.argwhere((got != want) & vis)
                assert bad.size == 0, f"{what}: {len(bad)} elements of the image differ, the first at {bad[0]}: {got[tuple(bad[0])]!r} for {want[tuple(bad[0])]!r}"
                assert np.array_equal(got, whole), f"{what}: outside the image"
                assert info == 0 and np.array_equal(ipiv, np.arange(1, n + 1)), what
                assert same_bits(sA.raw(), A0), f"{what}: A was written"
                assert sF.padding_intact(), f"{what}: the padding of F32 was written"
                norms.append(anorm)
        assert len(set(norms)) == 1, norms
        if fam == "axis":
            assert norms[0] == cm.exact_axis_anorm(A), f"n={n} {kind}: anorm {norms[0]!r}, exact {cm.exact_axis_anorm(A)!r}"
        else:
            assert abs(norms[0] - cm.anorm_inf(A)) <= (n + 2) * cm.EPS * norms[0]


SPECIAL = [("overflow", 1e39), ("FLT_MAX + half an ulp", float(np.finfo(np.float32).max) + 2.0 ** 103), ("NaN", float("nan")),
           ("2^-149", 2.0 ** -149), ("2^-150", 2.0 ** -150), ("3 * 2^-150", 3 * 2.0 ** -150), ("2^-127", 2.0 ** -127)]


@pytest.mark.parametrize("what,v", SPECIAL, ids=[w for w, _ in SPECIAL])
def test_special_values_convert_as_ieee(what, v):
    """n = 1, the special value in one part and a plain number in the other, both ways round: numpy's IEEE conversion of each part,
    gradual underflow included (include/rflu.h)."""
    h = handle()
    for z in (complex(v, 0.75), complex(-0.75, -v)):
        want = cm.expected_cimage(np.array([[z]]))
        for vin, vout in ((False, False), (True, True)):
            sA = Store(np.array([[z]]), 1, off=0 if vin else 1)
            sF = Store(np.array([[-7.25 * (1 + 1j)]]), 2 if vout else 1, np.float32, row_major=True)
            assert cdemote_variant(sA.address, sF.address, sF.ld) == (vin, vout)
            ipiv, anorm, info = mixed_getrf(h, 1, sA, sF, GETRF)
            got = sF.raw()[:2]
            ref = np.array([want[0, 0].real, want[0, 0].imag], dtype=np.float32)
            print(f"{what}: {z!r} -> {got!r} (numpy: {ref!r}), anorm {anorm!r}, info {info}")
            assert same_bits(got[~np.isnan(ref)], ref[~np.isnan(ref)]) and np.isnan(got[np.isnan(ref)]).all()
            assert info == 0 and ipiv[0] == 1                              # one part is +-3/4: the pivot is not zero
            assert sF.padding_intact()


# ---- B. the refinement loop ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("residual_path", ["residual_few", "gemm"], indirect=True)
@pytest.mark.parametrize("n", cm.REFINE_N)
def test_refinement_step_by_step(n, residual_path):
    """complex_mixed_cases.crefine_case through rflu_mixed_getrs_cf64_dev with c_k in {1, 1 + 2^-S_CPLX}; 8 and 9 right-hand sides are
    both sides of CNARROW (column-major ComplexF32 right-hand sides with element-wise conversions, or their row-major image through
    the transposing ones)."""
    check_refinement_steps(handle(), cm.crefine_case, cm.S_CPLX, n, GETRS)


def test_nothing_stays_on_the_handle():
    check_handle_state(cm.crefine_case, cm.S_CPLX, GETRS, big=(513, 65), small=(33, 1))


# ---- C. the residual alone -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("residual_path", ["residual_few", "gemm"], indirect=True)
@pytest.mark.parametrize("n", mc.RESIDUAL_N)
def test_residual_of_small_gaussian_integers_is_exact(n, residual_path):
    """R == B - A X in int64 pairs; 511, 512, 513 and 1025 are around two and four of cresidual_few's 256-row workgroups."""
    check_residual(handle(), n, True, RESIDUAL)
