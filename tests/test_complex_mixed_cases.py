"""CPU proofs of what tests/complex_mixed_cases.py hands to the GPU tests of the complex mixed-precision solve: (i) the refinement
restated in NumPy / SciPy converges on every grid input in the recorded number of steps, reaches the Float64 bars, and its UNREFINED
ComplexF32 solve misses the rule by many orders of magnitude (so the GPU test fails without refinement); the ill-conditioned input
stalls; (ii) the constructed solve cases satisfy P B = L U X exactly and keep every row's sum of moduli below 2^24 grid units, which is
what makes == the right comparison; (iii) the complex inputs of the exact tests of the demoted image and of the refinement loop
(tests/test_gpu_complex_mixed_exact.py) meet the conditions of tests/mixed_cases.py parts A and B, and the listed mutations show."""
import numpy as np
import pytest

import complex_mixed_cases as cm
import mixed_cases as mc


@pytest.mark.parametrize("n,nrhs", cm.GRID)
def test_cpu_refinement_converges_in_the_recorded_steps(n, nrhs):
    A, B = cm.grid_input(n, nrhs)
    X, iters, first = cm.cpu_refine(A, B)
    print(f"n={n} nrhs={nrhs}: {iters} steps on the CPU, the unrefined ComplexF32 solve is at {first:.3e} of the rule")
    assert iters == cm.CPU_STEPS[n]
    assert np.all(cm.rule_ratio(A, X, cm.residual_ld(A, X, B)) <= 1.0)
    res, bound, err = cm.float64_bars(A, B, X, np.linalg.solve(A, B), cm.norm2(A))
    assert res < bound and err < 1e-6
    if n >= 8:
        assert first > 1e6          # without refinement the rule is missed by orders of magnitude


def test_step_allowance_and_grid():
    assert sorted(cm.CPU_STEPS) == sorted(n for n, _ in cm.GRID)
    assert cm.GPU_STEP_ALLOWANCE == 2 * max(cm.CPU_STEPS.values()) >= 2
    # the grid crosses CNARROW = 8 right-hand sides, RESIDUAL_PASS = 8, the residual crossover 16, the 64-wide tiles of the demotion,
    # the 256-row blocks of the residual and of the narrow solve
    assert {nrhs for _, nrhs in cm.GRID} >= {1, 3, 8, 9, 33, 64}


def test_ill_conditioned_input_stalls_on_the_cpu():
    n = 300
    A = cm.ill_conditioned(n, 10)
    assert 1e9 < np.linalg.cond(A) < 1e11
    B = cm.uniform_complex(n, 2, 77)
    X, iters, _ = cm.cpu_refine(A, B)
    ratio = float(np.max(cm.rule_ratio(A, X, cm.residual_ld(A, X, B))))
    print(f"kappa 1e10 on the CPU: iters = {iters}, stalled at {ratio:.3e} of the rule")
    assert iters == -31 and not ratio <= 1e3
    assert cm.cpu_refine(A, B, max_iter=4)[1] == -5


def test_anorm_is_the_modulus_norm():
    A = np.array([[3 + 4j, 1j], [1, 1]], order="F")
    assert cm.anorm_inf(A) == 6.0          # hypot(3, 4) + 1, not |3| + |4| + 1


@pytest.mark.parametrize("nrhs", cm.EXACT_NRHS)
@pytest.mark.parametrize("n", cm.EXACT_N)
def test_exact_solve_cases_are_exact(n, nrhs):
    c = cm.exact_solve_case(n, nrhs)
    # structure: unit lower / upper with the stated entries, a diagonal from DIAG, interchanges that are no identity and repeat targets
    offdiag = set(np.unique(np.concatenate([np.tril(c.L, -1).ravel(), np.triu(c.U, 1).ravel()])))
    assert offdiag <= set(cm.GAUSS) and np.array_equal(np.diag(c.L), np.ones(n))
    assert set(np.diag(c.U)) <= set(cm.DIAG)
    assert np.all(c.ipiv >= np.arange(1, n + 1)) and np.all(c.ipiv <= n)
    if n >= 31:
        assert np.any(c.ipiv != np.arange(1, n + 1)) and len(set(c.ipiv)) < n
    # P B = L U X, exactly: every product below is of small Gaussian (half-)integers, far inside complex128
    Z = c.B.astype(np.complex128).copy()
    for k in range(n):
        p = c.ipiv[k] - 1
        if p != k:
            Z[[k, p]] = Z[[p, k]]
    assert np.array_equal(Z, c.L @ (c.U @ c.X.astype(np.complex128)))
    # the bound of exact_solve_case's docstring
    print(f"n={n} nrhs={nrhs}: largest row sums of moduli {c.fwd_sum:.0f} (forward), {c.bwd_sum:.0f} (backward) of 2^24 = {2 ** 24}")
    assert c.fwd_sum < 2 ** 24 and c.bwd_sum < 2 ** 24
    # a Float32 substitution in plain row order returns X by == (one of the orders the proof covers)
    W = c.W
    y = Z.astype(np.complex64)
    for i in range(n):
        y[i] = y[i] - (W[i, :i].astype(np.complex64) @ y[:i]).astype(np.complex64) if i else y[i]
    for i in range(n - 1, -1, -1):
        t = y[i] - (W[i, i + 1:] @ y[i + 1:]).astype(np.complex64) if i < n - 1 else y[i]
        y[i] = (t / W[i, i]).astype(np.complex64)
    assert np.array_equal(y, c.X)


# ---- the demoted image (tests/mixed_cases.py part A, complex) --------------------------------------------------------------------------
@pytest.mark.parametrize("n", cm.CDEMOTE_SIZES)
def test_cdemote_inputs_have_the_structure_the_trick_needs(n):
    for fam in ("random", "axis"):
        U, L = cm.cdemote_input(n, "upper", fam), cm.cdemote_input(n, "lower", fam)
        assert np.array_equal(U, np.triu(U)) and np.all(np.abs(np.diag(U)) >= 0.49) and np.all(np.isfinite(U))
        assert np.array_equal(L, np.tril(L)) and np.array_equal(np.diag(L), np.ones(n)) and np.all(np.abs(np.tril(L, -1)) <= 0.75)
        for A, kind in ((U, "upper"), (L, "lower")):
            vis = mc.visible(kind)(n)
            img = cm.expected_cimage(A)
            assert np.all(A[vis] != 0) and np.all(np.isfinite(img))
            parts = np.concatenate([img.real[vis], img.imag[vis]])
            assert np.all((parts == 0) | (np.abs(parts) >= np.finfo(np.float32).tiny))        # no subnormal anywhere
            if fam == "random":
                assert np.all(A.real[vis] != 0) and np.all(A.imag[vis] != 0)
            else:
                assert np.all((A.real[vis] != 0) ^ (A.imag[vis] != 0))
                if n >= 63:
                    assert np.any(A.real[vis] != 0) and np.any(A.imag[vis] != 0)
            if n >= 63:
                assert not np.any((img[1:] == img[:-1]) & vis[1:] & vis[:-1]) and not np.any((img[:, 1:] == img[:, :-1]) & vis[:, 1:] & vis[:, :-1])


@pytest.mark.parametrize("n", cm.CDEMOTE_SIZES)
def test_cdemote_restated_kernel_image_and_norm(n):
    """The restated tile kernel returns numpy's IEEE image; for the on-axis family its norm, summed in the kernel's order, equals the
    exact one and so does every other order; for the random family it stays within the (n + 2) eps bar of test_gpu_complex_mixed.py."""
    for kind in ("upper", "lower"):
        for fam in ("random", "axis"):
            A = cm.cdemote_input(n, kind, fam)
            F, anorm = cm.cdemote_restated(A)
            assert np.array_equal(F, cm.expected_cimage(A)), (kind, fam)
            if fam == "axis":
                exact = cm.exact_axis_anorm(A)
                assert np.array_equal(np.hypot(A.real, A.imag), np.abs(A.real) + np.abs(A.imag))     # hypot(x, 0) = |x|
                assert anorm == exact and cm.anorm_inf(A) == exact and np.abs(A)[:, ::-1].sum(axis=1).max() == exact
            else:
                assert abs(anorm - cm.anorm_inf(A)) <= (n + 2) * cm.EPS * anorm


@pytest.mark.parametrize("mutation", cm.CMUTATIONS)
def test_each_cdemote_mutation_changes_what_the_two_inputs_show(mutation):
    seen = []
    for n in cm.CDEMOTE_SIZES:
        if (mutation == "dropped_last_column" and n % cm.CDM_T == 0) or (mutation != "dropped_last_column" and n < 63):
            continue
        for fam in ("random", "axis"):
            differs = False
            for kind in ("upper", "lower"):
                A = cm.cdemote_input(n, kind, fam)
                vis = mc.visible(kind)(n)
                differs |= not np.array_equal(cm.cdemote_restated(A, mutation)[0][vis], cm.expected_cimage(A)[vis])
            assert differs, (mutation, n, fam)
        seen.append(n)
    assert len(seen) >= 4, seen


# ---- the refinement loop (tests/mixed_cases.py part B, complex) -------------------------------------------------------------------------
CREFINE = [(n, k) for n in cm.REFINE_N for k in cm.REFINE_NRHS]


@pytest.mark.parametrize("n,nrhs", CREFINE)
def test_crefine_cases_meet_the_conditions_and_the_restated_loop_is_exact(n, nrhs):
    c = cm.crefine_case(n, nrhs)
    assert c.fwd_sum < 2 ** 24 and c.bwd_sum < 2 ** 24                   # the ComplexF32 solve of b0 returns x0 (exact_solve_case)
    assert np.array_equal(2 * c.A, np.rint(2 * c.A.real) + 1j * np.rint(2 * c.A.imag))          # Gaussian integers times 1/2
    assert np.array_equal(c.F32.astype(np.complex128), np.tril(c.L, -1).astype(np.complex128) + c.U)
    for pattern in mc.PATTERNS:
        bits, margin = mc.refine_proof(c, pattern, cm.S_CPLX, grid=0.5)
        B, Xw, mask = c.rhs(pattern, cm.S_CPLX)
        X, iters = mc.refine_restated(c, B, c.anorm)
        assert iters == (1 if mask.any() else 0), (pattern, iters)
        assert np.array_equal(X, Xw), pattern
        if mask.any():
            assert mc.refine_restated(c, B, c.anorm, max_iter=1)[1] == 1
    print(f"n={n} nrhs={nrhs}: term sum {c.term_sum / 0.5:.0f} units of 1/2 = {bits} bits (+ {cm.S_CPLX} <= 53), the rule is missed by {margin:.3e} at step 0")


def test_s_cplx_is_the_largest_the_dense_cases_allow():
    """S_CPLX + 1 breaks a condition for at least one case (the margin of the rule at n = 513), S_CPLX breaks none."""
    broken = 0
    for n, nrhs in CREFINE:
        c = cm.crefine_case(n, nrhs)
        mc.refine_proof(c, "all", cm.S_CPLX, grid=0.5)
        try:
            mc.refine_proof(c, "all", cm.S_CPLX + 1, grid=0.5)
        except AssertionError:
            broken += 1
    assert broken >= 1


@pytest.mark.parametrize("mutation", mc.LOOP_MUTATIONS)
def test_each_mutation_of_the_complex_loop_changes_x_or_iters(mutation):
    for n, nrhs in CREFINE:
        if nrhs < 3 or n == 1:       # (n = 1 draws some zero columns, which meet the rule whatever is done to them)
            continue
        c = cm.crefine_case(n, nrhs)
        caught = False
        for pattern in ("mixed_a", "mixed_b"):
            B, Xw, _ = c.rhs(pattern, cm.S_CPLX)
            X, iters = mc.refine_restated(c, B, c.anorm, max_iter=3, mutation=mutation)
            caught |= iters != 1 or not np.array_equal(X, Xw)
        assert caught, (mutation, n, nrhs)
