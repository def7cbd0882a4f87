"""The yardsticks of the condition-estimate tests, proved on the CPU (no GPU, no torch): the numpy restatement of rflu_gecon_*
(tests/cond_cases.py) against LAPACK's own gecon and against the true norm of the inverse, the exactness certificate of the constructed
inputs, and planted faults that the exact inputs must notice."""
import os
import re

import numpy as np
import pytest

import cond_cases as C

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "recursivefactorization.jl_amd", "csrc")
RANDOM_SIZES = [1, 2, 3, 7, 8, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257, 513, 1000]
SEEDS = [0, 1, 2]


def test_constants_match_the_sources():
    src = open(os.path.join(CSRC, "condest.hip")).read()
    assert int(re.search(r"constexpr int CS_CHUNK = (\d+);", src).group(1)) == C.CS_CHUNK
    assert int(re.search(r"constexpr int CS_THREADS = (\d+);", src).group(1)) == C.CS_THREADS
    hdr = open(os.path.join(CSRC, "..", "..", "include", "rflu.h")).read()
    assert re.search(r"enum rflu_norm \{ RFLU_NORM_ONE = 1, RFLU_NORM_INF = 2 \};", hdr)


def test_kernel_sum_is_the_chunked_tree():
    rng = np.random.default_rng(5)
    for n in (1, 2, 255, 256, 257, 1024, 1025, 3000):
        a = rng.random(n)
        assert abs(C.kernel_sum(a) - np.sum(a)) <= n * np.finfo(np.float64).eps * np.sum(a)
    ints = rng.integers(0, 1000, size=2500).astype(np.float64)
    assert C.kernel_sum(ints) == ints.sum()                       # exact on integers, whatever the order
    assert C.kernel_sum(ints, drop_chunk=1) == ints.sum() - ints[1024:2048].sum()
    a = np.array([2.0 ** 53, 1.0, 0.0, 1.0] + [0.0] * 300)        # the order is visible: t = 1 and t = 3 meet (s = 2) before they
    assert C.kernel_sum(a) == 2.0 ** 53 + 2.0                     # reach t = 0 (s = 1); one after the other each would be rounded away


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("family", C.FAMILIES)
def test_restatement_against_lapack_and_the_true_norm(family, dtype):
    """On every random input the restatement and LAPACK's gecon (on LAPACK's factors) are lower bounds of the true ||A^-1|| up to
    rounding -- est <= true (1 + 1e-3) -- and neither falls below half of it; an input on which LAPACK's own estimate is below
    half is dropped (the GPU tests draw their inputs through C.pick_seed, which drops the same ones).  They agree closely, or the changed start / closing
    vector sent the iteration another way (counted and printed; both still meet the two bars).  `true` is the norm of the Float64
    inverse of the matrix the factors multiply to (for Float32 the factors' own rounding is not the estimator's business)."""
    worst_r, worst_l, other_branch, cases, dropped = 1.0, 1.0, 0, 0, 0
    for n in RANDOM_SIZES:
        for seed in SEEDS:
            A = C.random_matrix(family, n, seed, dtype)
            lu, _ = C.lapack_factors(A)
            L = np.tril(lu.astype(np.float64), -1) + np.eye(n)
            U = np.triu(lu.astype(np.float64))
            LU = L @ U
            for norm in (C.NORM_ONE, C.NORM_INF):
                anorm = float(np.linalg.norm(LU, 1 if norm == C.NORM_ONE else np.inf))
                true = C.true_inverse_norm(LU, norm)
                _, est, _ = C.rcond_restatement(lu, norm, anorm, dtype, detail=True)
                ref = C.lapack_gecon(lu, anorm, norm)
                if ref < 0.5 * true:          # an input on which LAPACK's own estimate is below half: not kept (C.kept says the same)
                    dropped += 1
                    assert not C.kept(family, n, seed, dtype)
                    continue
                assert est is not None and est <= true * (1 + 1e-3), (family, n, seed, norm, est / true)
                assert ref <= true * (1 + 1e-3), (family, n, seed, norm, ref / true)
                assert est >= 0.5 * true, (family, n, seed, norm, est / true)
                assert ref >= 0.5 * true, (family, n, seed, norm, ref / true)
                if abs(est - ref) > 1e-3 * true:
                    other_branch += 1
                worst_r, worst_l, cases = min(worst_r, est / true), min(worst_l, ref / true), cases + 1
    print(f"{family} {np.dtype(dtype).name}: {cases} cases, worst est/true restatement {worst_r:.3f}, LAPACK {worst_l:.3f}, "
          f"{other_branch} took another branch, {dropped} inputs dropped (LAPACK below 0.5)")
    assert other_branch <= cases // 4 and dropped <= cases // 10


@pytest.mark.parametrize("n", sorted(set(C.GECON_SIZES + C.BATCHED_SIZES)))
def test_exactness_certificate(n):
    """Every number any blocked substitution forms on any vector of the estimator fits Float32's 24 bits; the restatement returns the
    same estimate in Float32 and Float64, and that estimate is a lower bound of the exactly known norm."""
    bits_m, bits_mt = C.vector_bits(n)
    assert max(bits_m, bits_mt) <= 24, (n, bits_m, bits_mt)
    e = C.exact_factors(n)
    for norm in (C.NORM_ONE, C.NORM_INF):
        anorm = C.exact_anorm(n, norm)
        r32 = C.rcond_restatement(e.F, norm, anorm, np.float32, detail=True)
        r64 = C.rcond_restatement(e.F, norm, anorm, np.float64, detail=True)
        assert r32 == r64
        true = np.abs(e.Y).sum(axis=0 if norm == C.NORM_ONE else 1).max()
        assert true / 3 <= r64[1] <= true, (n, norm, r64, true)
        # every vector that entered a solve is a small-integer vector
        trace = []
        m, mt = C.triangular_solvers(e.F, np.float64)
        C.estimate(m, mt, n, np.float64, trace=trace)
        for _, v in trace:
            assert np.array_equal(v, np.rint(v)) and np.abs(v).max() <= max(2 * n - 2, 1)


def test_small_exact_cases_are_exact():
    for seed in C.SMALL_SEEDS:
        e = C.small_exact(seed)
        assert max(C.factor_bits(e)) <= 24
        for norm in (C.NORM_ONE, C.NORM_INF):
            an = C.case_anorm(e, norm)
            assert C.rcond_restatement(e.F, norm, an, np.float32, detail=True) == C.rcond_restatement(e.F, norm, an, np.float64, detail=True)


def _smallest_n_noticing(fault):
    for n in sorted(set(C.GECON_SIZES + C.BATCHED_SIZES)):
        for e in C.exact_cases(n):
            for norm in (C.NORM_ONE, C.NORM_INF):
                anorm = C.case_anorm(e, norm)
                if C.rcond_restatement(e.F, norm, anorm, np.float32, fault=fault) != C.rcond_restatement(e.F, norm, anorm, np.float32):
                    return n
    return None


@pytest.mark.parametrize("fault", ["sign_of_zero", "last_argmax", "no_closing", "swap_inf", "drop_chunk"])
def test_planted_faults_are_noticed(fault):
    """Each fault planted in the restatement changes the rcond of some exact case: the exact comparison on the GPU would see it."""
    n = _smallest_n_noticing(fault)
    print(f"{fault}: first noticed at n = {n}")
    assert n is not None, fault
    if fault == "drop_chunk":
        assert n > C.CS_CHUNK      # only a second chunk can be dropped
