"""CPU proofs of what tests/mixed_cases.py hands to tests/test_gpu_mixed_exact.py (no GPU): (A) the generator of the demotion inputs
meets every condition that makes == a fair demand -- the grid, the offsets with both parities, exact row sums in any order -- the
restated tile kernel returns numpy's IEEE image and the exact norm in all four variants, and each listed mutation changes what the two
inputs of a size show; (B) every refinement case meets the conditions on s, the restated loop returns c_k x0 with iters == 1 (0 for
c = 1), and each listed mutation of the loop changes X or iters; (C) the residual cases stay far inside Float64."""
import numpy as np
import pytest

import mixed_cases as mc


# ---- A -------------------------------------------------------------------------------------------------------------------------------
def test_family_offsets_parities_and_grid():
    rng = np.random.default_rng(7)
    v, m, k = mc.family((257, 257), rng)
    assert {(int(a), int(b)) for a, b in zip(k.ravel(), (m % 2).ravel())} == {(a, b) for a in range(len(mc.OFFSETS)) for b in (0, 1)}
    assert np.all(np.abs(v) < 2) and np.all(np.abs(v) > 0.49)
    assert np.array_equal(np.rint(v * 2.0 ** mc.GRID_BITS) * 2.0 ** -mc.GRID_BITS, v)            # on the grid 2^-40
    # what the offsets do: 0 and +-1/4 return f, the ties go to the even neighbour, +-(1/2 + 2^-16) leave f, +-(1/2 - 2^-16) do not
    ulp = np.where(np.abs(v) >= 1, 2.0 ** -23, 2.0 ** -24)
    f = np.sign(v) * (2.0 ** 23 + m) * ulp
    steps = (mc.expected_image(v).astype(np.float64) - f) / (np.sign(v) * ulp)
    off = mc.OFFSETS[k]
    want = np.where(np.abs(off) < 0.5, 0.0, np.where(np.abs(off) > 0.5, np.sign(off), np.where(m % 2 == 1, np.sign(off), 0.0)))
    assert np.array_equal(steps, want)
    # the lower family stays at or below 3/4 after rounding, the image is a normal Float32 everywhere
    w = mc.family((257, 257), rng, exps=(-1,), mbits=22)[0]
    assert np.all(np.abs(w) < 0.75) and np.all(np.abs(mc.expected_image(w)) <= 0.75) and np.all(np.abs(w) >= 0.5)


def test_row_sums_are_exact_in_any_order():
    """|v| < 2 on the grid 2^-40: a sum of up to 1025 moduli is below 2^12 on that grid = 52 bits.  Shown on the committed inputs by
    summing every row forwards, backwards and pairwise (numpy's sum) against integer arithmetic; the kernel's own order is
    test_restated_kernel_gives_the_ieee_image_and_the_exact_norm's."""
    assert 1025 * 2 < 2 ** 12 and 12 + mc.GRID_BITS <= 53 and max(mc.DEMOTE_SIZES) <= 1025
    for n in mc.DEMOTE_SIZES:
        for kind in ("upper", "lower"):
            A = mc.demote_input(n, kind)
            exact = mc.exact_anorm(A)
            absA = np.abs(A)
            fwd = np.zeros(n)
            bwd = np.zeros(n)
            for j in range(n):
                fwd, bwd = fwd + absA[:, j], bwd + absA[:, n - 1 - j]
            assert fwd.max() == exact and bwd.max() == exact and absA.sum(axis=1).max() == exact, (n, kind)


@pytest.mark.parametrize("n", mc.DEMOTE_SIZES)
def test_inputs_have_the_structure_the_trick_needs(n):
    U, L = mc.demote_input(n, "upper"), mc.demote_input(n, "lower")
    assert np.array_equal(U, np.triu(U)) and np.all(np.abs(np.diag(U)) >= 0.49) and np.all(np.isfinite(U))
    assert np.array_equal(L, np.tril(L)) and np.array_equal(np.diag(L), np.ones(n)) and np.all(np.abs(np.tril(L, -1)) <= 0.75)
    for A, kind in ((U, "upper"), (L, "lower")):
        vis = mc.visible(kind)(n)
        assert np.all(A[vis] != 0)                                      # a dropped element (a zero or the sentinel) is seen
        img = mc.expected_image(A)[vis]
        assert np.all(np.isfinite(img)) and np.all(np.abs(img) >= np.finfo(np.float32).tiny)
        if n >= 63:
            # entries differ from position to position: 2^23 mantissas, so at most a few of 10^5 entries share a value, and no entry
            # equals its neighbour in the row or in the column
            assert len(np.unique(img)) > 0.98 * img.size
            full = mc.expected_image(A)
            assert not np.any((full[1:] == full[:-1]) & vis[1:] & vis[:-1]) and not np.any((full[:, 1:] == full[:, :-1]) & vis[:, 1:] & vis[:, :-1])
    assert np.all(mc.visible("upper")(n) ^ mc.visible("lower")(n))      # the two calls show every element once


@pytest.mark.parametrize("n", mc.DEMOTE_SIZES)
def test_restated_kernel_gives_the_ieee_image_and_the_exact_norm(n):
    for kind in ("upper", "lower"):
        A = mc.demote_input(n, kind)
        for vin in (False, True):
            for vout in (False, True):
                F, anorm = mc.demote_restated(A, vin, vout)
                assert np.array_equal(F, mc.expected_image(A)) and anorm == mc.exact_anorm(A), (kind, vin, vout)


def applies(mutation, n):
    """the sizes at which a mutation can show at all"""
    return {"dropped_last_column": n % mc.DM_TJ != 0, "exchanged_rows": n >= 2, "missing_last_odd_row": n % 2 == 1}.get(mutation, True)


@pytest.mark.parametrize("mutation", mc.MUTATIONS)
def test_each_mutation_changes_what_the_two_inputs_show(mutation):
    """For every size at which the mutation can show (a partial tile, two rows, an odd last row; the roundings at every size from 63 on,
    where all offsets occur), the part of the image that the factorization leaves alone differs from the expected one for at least one
    of the two inputs.  exchanged_rows and missing_last_odd_row belong to the 16-byte load form (VIN) alone."""
    seen = []
    for n in mc.DEMOTE_SIZES:
        if not applies(mutation, n) or (mutation in ("truncation", "half_away") and n < 63):
            continue
        differs = False
        for kind in ("upper", "lower"):
            A = mc.demote_input(n, kind)
            F, _ = mc.demote_restated(A, True, True, mutation)
            vis = mc.visible(kind)(n)
            differs |= not np.array_equal(F[vis], mc.expected_image(A)[vis])
        assert differs, (mutation, n)
        seen.append(n)
    print(f"{mutation}: seen at n = {seen}")
    assert len(seen) >= 4


# ---- B -------------------------------------------------------------------------------------------------------------------------------
CASES = [(n, k) for n in mc.REFINE_N for k in mc.REFINE_NRHS]


@pytest.mark.parametrize("n,nrhs", CASES)
def test_refinement_cases_meet_the_conditions_and_the_restated_loop_is_exact(n, nrhs):
    c = mc.refine_case(n, nrhs)
    assert mc.S_REAL == 30
    assert np.array_equal(c.F32.astype(np.float64), np.tril(c.L, -1).astype(np.float64) + c.U)   # the packed factors are Float32 numbers
    assert c.anorm == np.abs(c.A).sum(axis=1).max() and np.array_equal(c.A, np.rint(c.A))
    for pattern in mc.PATTERNS:
        bits, margin = mc.refine_proof(c, pattern, mc.S_REAL)
        B, Xw, mask = c.rhs(pattern, mc.S_REAL)
        X, iters = mc.refine_restated(c, B, c.anorm)
        assert iters == (1 if mask.any() else 0), (pattern, iters)
        assert np.array_equal(X, Xw), pattern
        if mask.any():
            assert mc.refine_restated(c, B, c.anorm, max_iter=1)[1] == 1          # max_iter = 1 is enough
    print(f"n={n} nrhs={nrhs} seed {c.seed}: term sum {c.term_sum} = {bits} bits (+ {mc.S_REAL} <= 53), the rule is missed by {margin:.3e} at step 0")


def test_patterns_cover_first_and_last_both_ways():
    for nrhs in mc.REFINE_NRHS:
        a, b = mc.scaled_columns(nrhs, "mixed_a"), mc.scaled_columns(nrhs, "mixed_b")
        if nrhs >= 3:
            assert a[0] and a[-1] and not b[0] and not b[-1] and np.array_equal(a, ~b) and not a.all()
        assert mc.scaled_columns(nrhs, "all").all() and not mc.scaled_columns(nrhs, "none").any()


@pytest.mark.parametrize("mutation", mc.LOOP_MUTATIONS)
def test_each_mutation_of_the_loop_changes_x_or_iters(mutation):
    """A wrong column updated, a rule that reads the first or the last column alone, an update applied twice, iters off by one: each
    changes X or iters in one of the two mixed patterns, at every size with at least three columns."""
    for n, nrhs in CASES:
        if nrhs < 3:
            continue
        c = mc.refine_case(n, nrhs)
        caught = False
        for pattern in ("mixed_a", "mixed_b"):
            B, Xw, _ = c.rhs(pattern, mc.S_REAL)
            X, iters = mc.refine_restated(c, B, c.anorm, max_iter=3, mutation=mutation)
            caught |= iters != 1 or not np.array_equal(X, Xw)
        assert caught, (mutation, n, nrhs)


# ---- C -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("n", mc.RESIDUAL_N)
def test_residual_cases(n, cplx):
    A, X, B, R = mc.residual_case(n, cplx)
    parts = lambda M: np.concatenate([M.real.ravel(), M.imag.ravel()])          # noqa: E731
    for M in (A, X, B):
        assert np.all(np.abs(parts(M)) <= 4) and np.array_equal(parts(M), np.rint(parts(M)))
    assert (2 if cplx else 1) * 16 * n + 4 < 2 ** 53                             # every partial sum of every order is an exact integer
    assert np.array_equal(R, B - A @ X)
    assert np.any(R != B)
