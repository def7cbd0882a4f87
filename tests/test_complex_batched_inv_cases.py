"""What tests/test_gpu_complex_batched_inv.py relies on, checked on the CPU: the restatement of cgetri_batched_kernel
(tests/complex_batched_inv_cases.py) on every input of the GPU test stays far inside the residual bar, so the bar hides no failure of
the algorithm and leaves the kernel room for nothing but its own mistakes; the exact inputs come back exactly; no input is singular."""
import numpy as np
import pytest

import complex_batched_cases as CB
import complex_batched_inv_cases as BI
import complex_inv_cases as CI
import complex_ref as CR

SFX = ["cf64", "cf32"]


def _worst(sfx, n, batches, matrix=None, pivot=True):
    worst = 0.0
    for b in batches:
        A = CB.matrix(n, n, sfx, b) if matrix is None else matrix(n, sfx, b)
        F, ip, info = CB.ref_factors(n, n, sfx, b) if matrix is None else CR.complex_generic_lufact(A, pivot)
        assert info == 0, (sfx, n, b, info)                                   # no input is singular
        X = BI.restatement(F, ip if pivot else None)
        assert X.dtype == BI.CTYPES[sfx]
        for letter in BI.LETTERS:                                             # op(X) is the same numbers: the residuals swap sides
            worst = max(worst, BI.worst_rho(A, BI.op(X, letter), sfx, letter))
    return worst


@pytest.mark.parametrize("sfx,n", [(s, n) for s in SFX for n in BI.SIZES[s] + [BI.FALLBACK[s]]])
def test_the_restatement_stays_far_inside_the_bar(sfx, n):
    """Half the bar for n >= 2 and the bar at n = 1, on every matrix of the largest batch (the smaller batches are its head; the
    fallback sizes run FALLBACK_BATCH matrices).  Measured where this was written, b = 0 .. 66, the larger of the two residuals:
    1.03 (cf64) / 0.66 (cf32) at n = 1, <= 0.40 at n = 2 and 3, <= 0.14 at n = 7 and 8, <= 0.051 from n = 31 to 64, <= 0.030 for
    ComplexF32 at n = 65 .. 128, <= 0.02 at the two fallback sizes."""
    batches = range(BI.FALLBACK_BATCH if n == BI.FALLBACK[sfx] else BI.BATCH)
    w = _worst(sfx, n, batches)
    print(f"{sfx} n = {n}: worst rho of the restatement {w:.4f} (bar {CI.rho_bar(n)})")
    assert w <= BI.half_bar(n), (sfx, n, w)


@pytest.mark.parametrize("sfx,n", [(s, n) for s in SFX for n in BI.NOPIVOT_SIZES])
def test_the_restatement_on_the_nopivot_inputs(sfx, n):
    w = _worst(sfx, n, range(BI.NOPIVOT_BATCH), matrix=CB.nopivot_matrix, pivot=False)
    print(f"{sfx} n = {n} NoPivot: worst rho of the restatement {w:.4f}")
    assert w <= BI.half_bar(n), (sfx, n, w)


@pytest.mark.parametrize("sfx,n", [(s, n) for s in SFX for n in BI.EXACT_SIZES[s]])
def test_exact_cases_are_exact_under_the_kernels_order(sfx, n):
    """Gaussian-dyadic factors with an integer-certified inverse: every operation of the restatement is exact in both precisions, so
    it returns the certified inverse by ==, and so must the kernel, whichever products it fuses."""
    F, ipiv, c = BI.exact_factors(n, sfx)
    X = BI.restatement(F, ipiv)
    assert X.dtype == BI.CTYPES[sfx]
    assert np.array_equal(X, BI.exact_inverse(c, sfx, "N"))
    assert np.array_equal(X.astype(np.complex128), c.X)
    # the three letters of the exact case are three different matrices, so a swapped store or a misplaced conjugation cannot pass ==
    XT, XC = BI.exact_inverse(c, sfx, "T"), BI.exact_inverse(c, sfx, "C")
    if n > 1:
        assert not np.array_equal(X, XT) and not np.array_equal(XT, XC) and not np.array_equal(X, XC)
    # and a reversed permutation is another matrix too
    assert not np.array_equal(BI.restatement(F, ipiv[::-1].copy()), X)


def test_reciprocal_restates_smiths_formula():
    for ctype in (np.complex128, np.complex64):
        d = np.array([2, -2j, 0.5, 1j, 3 + 4j, 4 - 3j, 1e-3 + 1j], dtype=ctype)
        r = BI.reciprocal(d)
        assert r.dtype == d.dtype
        assert np.array_equal(r[:4], np.array([0.5, 0.5j, 2, -1j], dtype=ctype))
        assert np.allclose(r * d, 1, rtol=8 * np.finfo(CR.real_of(ctype)).eps, atol=0)
        z = BI.reciprocal(np.array([0, 1j, 1], dtype=ctype))
        assert not np.isfinite(z[0]) and np.isfinite(z[1:]).all()              # only BOTH parts zero is singular


def test_one_part_zero_is_not_singular_and_a_zeroed_column_is():
    """The hand-made factors of the GPU test: u_44 = 1j leaves a finite inverse, u_44 = 0 + 0j does not; a zeroed column of the input
    gives a u_ii with both parts exactly zero at that column."""
    F, ipiv, _ = BI.exact_factors(8, "cf64")
    G = np.array(F)
    G[3, 3] = 1j
    assert BI.finite(BI.restatement(G, ipiv))
    G[3, 3] = 0
    assert not BI.finite(BI.restatement(G, ipiv))
    A = np.array(CB.matrix(33, 33, "cf64", 5))
    A[:, 7] = 0
    Fz, _, info = CR.complex_generic_lufact(A, True)
    assert info == 8 and Fz[7, 7] == 0


def test_sizes_cover_the_switches():
    for sfx in SFX:
        s = set(BI.SIZES[sfx])
        assert {7, 8, 32, 33, 63, 64} <= s and max(s) == BI.LIMIT[sfx] and BI.FALLBACK[sfx] == BI.LIMIT[sfx] + 1
        assert set(BI.EXACT_SIZES[sfx]) <= s and set(BI.NOPIVOT_SIZES) <= s and set(BI.SMALL_BATCH_SIZES) <= s
    assert {64, 65, 127, 128} <= set(BI.SIZES["cf32"])
    for groups in (4, 2):
        assert BI.BATCH % groups and all(b % groups for b in BI.SMALL_BATCHES if b > 1)
    assert BI.BATCH <= 67
