"""CPU proofs of what tests/complex_mixed_cases.py hands to the GPU tests of the complex mixed-precision solve: (i) the refinement
restated in NumPy / SciPy converges on every grid input in the recorded number of steps, reaches the Float64 bars, and its UNREFINED
ComplexF32 solve misses the rule by many orders of magnitude (so the GPU test fails without refinement); the ill-conditioned input
stalls; (ii) the constructed solve cases satisfy P B = L U X exactly and keep every row's sum of moduli below 2^24 grid units, which is
what makes == the right comparison."""
import numpy as np
import pytest

import complex_mixed_cases as cm


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
