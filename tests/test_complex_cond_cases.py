"""The yardsticks of the complex condition-estimate tests, proved on the CPU (no GPU, no torch): the numpy restatement of rflu_gecon_c*
and rflu_lange_c* (tests/complex_cond_cases.py) against LAPACK's zgecon / cgecon and the true norm of the inverse, the exact families
(real factors embedded as complex; axis-scaled factors that exercise the conjugation), planted faults those inputs must notice, and the
decision margin that admits an input to the rounding-level comparison on the GPU."""
import math
import os
import re

import numpy as np
import pytest

import complex_cond_cases as C
import cond_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "recursivefactorization.jl_amd", "csrc")
DTYPES = [np.complex128, np.complex64]
IDS = ["cf64", "cf32"]
NORMS = [C.NORM_ONE, C.NORM_INF]
RANDOM_SIZES = [1, 2, 3, 7, 8, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257]


def test_constants_match_the_sources():
    src = open(os.path.join(CSRC, "condest.hip")).read()   # one source for the real and the complex elements: the real constants
    assert int(re.search(r"constexpr int LN_CHUNK = (\d+);", src).group(1)) == C.LN_CHUNK
    assert int(re.search(r"constexpr int LN_THREADS = (\d+);", src).group(1)) == C.LN_THREADS
    assert int(re.search(r"constexpr int LN_GROUP = (\d+);", src).group(1)) == C.LN_GROUP
    assert int(re.search(r"constexpr int CS_CHUNK = (\d+);", src).group(1)) == R.CS_CHUNK
    assert int(re.search(r"constexpr int CS_THREADS = (\d+);", src).group(1)) == R.CS_THREADS
    hdr = open(os.path.join(ROOT, "recursivefactorization.jl_amd", "csrc", "rflu_internal.hpp")).read()
    for dtype, name in ((np.complex128, "CF64"), (np.complex64, "CF32")):
        assert int(re.search(rf"constexpr int64_t CBATCHED_MAX_DIM_{name} = (\d+);", hdr).group(1)) == C.CBATCHED_LIMIT[dtype]
        assert max(C.CBATCHED_SIZES[dtype]) == C.CBATCHED_LIMIT[dtype]


def test_norm_sums_are_the_kernels_order():
    rng = np.random.default_rng(5)
    for n in (1, 2, 255, 256, 257, 1024, 1025, 3000):
        a = rng.random(n)
        for fn in (C.line_sum_along, C.line_sum_across):
            assert abs(fn(a) - math.fsum(a)) <= n * np.finfo(np.float64).eps * math.fsum(a)
    ints = rng.integers(0, 1000, size=2500).astype(np.float64)
    assert C.line_sum_along(ints) == ints.sum() == C.line_sum_across(ints)
    a = np.zeros(300)
    a[0], a[4], a[12] = 2.0 ** 53, 1.0, 1.0         # the order is visible: threads 1 and 3 meet (s = 2) before they reach thread 0
    assert C.line_sum_along(a) == 2.0 ** 53 + 2.0 and C.line_sum_across(a) == 2.0 ** 53   # one after the other each is rounded away
    # the modulus: a NaN in either part wins over an Inf in the other
    z = np.array([[complex(np.inf, np.nan), 1.0], [2.0, 3.0]])
    assert math.isnan(C.lange_restatement(z, C.NORM_ONE, 0)) and math.isnan(C.lange_restatement(z, C.NORM_INF, 1))
    z = np.array([[complex(np.inf, 1.0), 1.0], [2.0, 3.0]])
    assert C.lange_restatement(z, C.NORM_ONE, 0) == math.inf
    g = rng.integers(-8, 9, size=(70, 33)) * C.UNITS[rng.integers(0, 4, size=(70, 33))]
    for norm in NORMS:
        for rm in (0, 1):
            assert C.lange_restatement(g, norm, rm) == np.abs(g).sum(axis=0 if norm == C.NORM_ONE else 1).max()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("family", C.FAMILIES)
def test_restatement_against_lapack_and_the_true_norm(family, dtype):
    """On a kept input of every size (C.pick_seed: LAPACK's own estimate reaches half the true norm; NO size and NO family may be left
    without one -- pick_seed raises otherwise, and the count is asserted) the restatement on LAPACK's factors stays within a factor of 3
    of zgecon / cgecon and at or above a third of the true ||(L U)^-1||, the bar of the real tests."""
    worst_true, worst_ref, cases = math.inf, 1.0, 0
    for n in RANDOM_SIZES:
        seed = C.pick_seed(family, n, dtype)
        assert C.kept(family, n, seed, dtype)
        lu, _ = C.lapack_factors(C.random_matrix(family, n, seed, dtype))
        LU = C.factor_product(lu)
        true = C.true_inverse_norms(LU)
        for norm in NORMS:
            anorm = float(np.linalg.norm(LU, 1 if norm == C.NORM_ONE else np.inf))
            _, est, solves = C.crcond_restatement(lu, norm, anorm, dtype, detail=True)
            ref = C.lapack_gecon(lu, anorm, norm)
            assert ref >= 0.5 * true[norm]
            assert est is not None and solves <= 11
            assert ref / 3 <= est <= 3 * ref, (family, n, seed, norm, est / ref)
            assert est >= true[norm] / 3, (family, n, seed, norm, est / true[norm])
            assert est <= true[norm] * (1 + 1e-3), (family, n, seed, norm, est / true[norm])
            worst_true = min(worst_true, est / true[norm])
            worst_ref = max(worst_ref, est / ref, ref / est)
            cases += 1
    print(f"{family} {np.dtype(dtype).name}: {cases} cases, worst est/true {worst_true:.3f}, worst ratio to LAPACK {worst_ref:.3f}")
    assert cases == 2 * len(RANDOM_SIZES)


@pytest.mark.parametrize("n", C.EXACT_SIZES)
def test_real_factors_embedded_as_complex(n):
    """The real exact factors with zero imaginary parts give the REAL restatement's rcond by ==, in both element types: sign(0) = +1 and
    phase(0) = 1 coincide, and the repeated-sign-vector test that the real estimator has and this one lacks never decides on them.
    Float32 is certified by cond_cases.vector_bits."""
    F, e = C.embedded_exact(n)
    assert max(R.vector_bits(n)) <= 24, (n, R.vector_bits(n))
    for norm in NORMS:
        an = R.case_anorm(e, norm)
        want = R.rcond_restatement(e.F, norm, an, np.float64)
        assert want == R.rcond_restatement(e.F, norm, an, np.float32)
        for dtype in DTYPES:
            assert C.crcond_restatement(F, norm, an, dtype) == want, (n, norm, dtype)


def test_axis_scaled_family():
    """Dense small integer factors with U's columns multiplied by powers of i: at least 16 (case, norm) pairs keep every vector of the
    trace on the axes, and on at least 6 of them M^T where M^H belongs changes the estimate.  On the qualifying pairs the restatement
    by substitution equals the one through the exact inverse in both element types: everything is a Gaussian integer."""
    good, notice = C.axis_search()
    print(f"axis-scaled: {len(good)} qualifying pairs of {2 * len(C.AXIS_SIZES) * C.AXIS_SEEDS}, {len(notice)} notice T for H")
    assert len(good) >= 16 and len(notice) >= 6
    assert len(C.axis_cases(C.NORM_ONE)) == 16 and sum(1 for c in C.axis_cases(C.NORM_ONE) if (c, C.NORM_ONE) in notice) >= 6
    assert len(C.axis_cases(C.NORM_INF)) >= 1
    for c, norm in good:
        an = C.axis_anorm(c, norm)
        want = C.crcond_restatement(c.F, norm, an, np.complex128, solvers=C.axis_solvers(c, np.complex128))
        assert 0 < want < math.inf
        for dtype in DTYPES:
            trace = []
            assert C.crcond_restatement(c.F, norm, an, dtype, trace=trace) == want
            assert all(C.on_axes(v) for _, v in trace)
        est = 1.0 / (want * an)
        true = np.abs(c.Y).sum(axis=0 if norm == C.NORM_ONE else 1).max()     # |D^-1 Y| = |Y|
        assert true / 3 <= est <= true * (1 + 1e-15)


def _exact_inputs():
    """(size, packed factors, norm, anorm) of every exact input, smallest first."""
    out = []
    good, _ = C.axis_search()
    for n in sorted(set(C.EXACT_SIZES + C.AXIS_SIZES)):
        if n in C.EXACT_SIZES:
            cases = [R.exact_factors(n)] + ([R.small_exact(s) for s in R.SMALL_SEEDS] if n == 3 else [])
            for e in cases:
                out += [(n, e.F.astype(np.complex128), norm, R.case_anorm(e, norm)) for norm in NORMS]
        out += [(n, c.F, norm, C.axis_anorm(c, norm)) for c, norm in good if c.n == n]
    return out


@pytest.mark.parametrize("fault", ["transpose", "phase_of_zero", "last_argmax", "no_closing", "drop_chunk", "swap_inf"])
def test_planted_faults_are_noticed(fault):
    """Each fault planted in the restatement changes the rcond of some exact input: the comparison by == on the GPU would see it."""
    first = None
    for n, F, norm, an in _exact_inputs():
        if C.crcond_restatement(F, norm, an, np.complex64, fault=fault) != C.crcond_restatement(F, norm, an, np.complex64):
            first = n
            break
    print(f"{fault}: first noticed at n = {first}")
    assert first is not None, fault
    if fault == "drop_chunk":
        assert first > R.CS_CHUNK      # only a second chunk can be dropped
    if fault == "transpose":
        assert first in C.AXIS_SIZES   # real factors cannot tell M^T from M^H


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_decision_margin_leaves_every_size_an_input_per_family(dtype):
    """The rounding-level comparison on the GPU takes only inputs on which every decision of the restatement (the top two moduli at an
    argmax, est against est_old, which covers |x_jlast| against |x_j|) has a relative gap above 64 n eps.  Every size keeps one per
    family (pick_seed raises otherwise), and the gap between the restatement in the element precision and one precision up -- what the
    GPU test multiplies by 8 -- is printed for the record in complex_cond_cases.py."""
    sizes = sorted(set(C.CGECON_SIZES + C.CBATCHED_SIZES[dtype]))
    for n in sizes:
        worst = 0.0
        for family in C.FAMILIES:
            seed = C.pick_seed(family, n, dtype, margin=True)
            assert C.kept(family, n, seed, dtype) and C.has_margin(family, n, seed, dtype)
            if n in C.CGECON_SIZES:
                lu, _ = C.lapack_factors(C.random_matrix(family, n, seed, dtype))
                for norm in NORMS:
                    _, est, _ = C.crcond_restatement(lu, norm, 1.0, dtype, detail=True)
                    _, up, _ = C.crcond_restatement(lu, norm, 1.0, C.wider(dtype), detail=True)
                    worst = max(worst, abs(est - up) / up)
        if n in C.CGECON_SIZES:
            print(f"{np.dtype(dtype).name} n={n}: restatement against one precision up, worst relative gap {worst:.2e}")
