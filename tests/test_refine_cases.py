"""CPU: the references of the refinement tests hold what tests/refine_cases.py says of them.  No GPU.

  * random inputs: the restatement's final berr and LAPACK's own (gesvx) stay within BERR_REF, which is recomputed here; at most 2 steps;
    the restatement's estimate over the true ||A^-1 diag(wt)||_inf stays in [1/2, 1 + 1e-3]; true forward error / ferr <= 1/2;
  * exact inputs: the proof of every case, and the restatement returns x0 with steps == mask and berr == 0;
  * every planted fault is noticed, at the size stated."""
import numpy as np
import pytest

import mixed_cases as MC
import refine_cases as R

DTYPES = [np.float64, np.float32]
IDS = ["f64", "f32"]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_random_inputs_reference_bars(dtype):
    u = R.uof(dtype)
    worst_r = worst_l = 0.0
    inexact = []
    for family, n in R.RANDOM_INPUTS:
        c = R.random_input(family, n, dtype)
        if not c.exact_rhs:
            inexact.append((family, n))
        o = R.restated_random(family, n, dtype)
        worst_r = max(worst_r, o.berr.max() / u)
        worst_l = max(worst_l, R.lapack_berr(c, dtype).max() / u)
        assert o.steps.max() <= 2, (family, n, o.steps)
        fe = R.true_forward_error(o.X, c.x_ref)
        assert np.all(fe <= 0.5 * o.ferr), (family, n, fe, o.ferr)
        for k in range(R.RANDOM_NRHS):
            q = o.est[k] / R.weighted_inverse_norm(c.A, o.wt[:, k])
            assert 0.5 <= q <= 1.0 + 1e-3, (family, n, k, q)
    print(f"{np.dtype(dtype).name}: restatement berr <= {worst_r:.3f} u, gesvx berr <= {worst_l:.3f} u, inexact B: {inexact}")
    assert inexact == ([] if dtype == np.float64 else [("uniform", 2112)])
    assert max(worst_r, worst_l) <= R.BERR_REF[dtype]
    assert max(worst_r, worst_l) > R.BERR_REF[dtype] - 0.01          # the stored figure is the measured one, rounded up


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_exact_inputs_proof_and_restatement(dtype):
    lowest = np.inf
    for n in MC.REFINE_N:
        for nrhs in R.EXACT_NRHS:
            for pattern in MC.PATTERNS:
                for pivoted in (True, False):
                    e = R.exact_input(n, nrhs, pattern, dtype, pivoted)
                    lowest = min(lowest, R.exact_proof(e, dtype))
                    if n > 129 and (nrhs > 9 or not pivoted):
                        continue                                   # the restatement's loop over columns is slow: the proof covers these
                    lu, piv = e.F, (np.arange(n) if e.ipiv is None else e.ipiv - 1).astype(np.int32)
                    o = R.refine_restated(e.A, lu, piv, e.B, e.X_in, dtype, ferr=False)
                    assert np.array_equal(o.X.astype(np.float64), e.x0), (n, nrhs, pattern, pivoted)
                    assert np.array_equal(o.steps, e.mask.astype(np.int64)) and np.all(o.berr == 0.0)
    print(f"{np.dtype(dtype).name}: smallest berr0 of a scaled column = {lowest:.3g} u")
    assert lowest >= 2.0 ** 10


def _differs(a, b):
    return not (np.array_equal(a.X, b.X) and np.array_equal(a.berr, b.berr, equal_nan=True) and np.array_equal(a.steps, b.steps)
                and np.array_equal(a.ferr, b.ferr, equal_nan=True))


def _fault_input(n, dtype=np.float64):
    """a random input whose start is perturbed column by column: column 0 far off (refines), column 1 LAPACK's solve, column 2 exact"""
    c = R.random_input("uniform", n, dtype)
    X = np.array(c.X_in)
    X[:, 0] = (X[:, 0].astype(np.float64) * (1.0 + 2.0 ** -12)).astype(dtype)
    X[:, 2] = c.x_true[:, 2].astype(dtype)
    return c, np.asfortranarray(X)


# the smallest size of RANDOM_N (drop_slice: of those with two slices) at which the fault changes a result
NOTICED_AT = {"abs_x": 2, "no_abs_b": 1, "update_stopped": 65, "lstres_fixed": 63, "neighbour_berr": 1, "no_nuw": 1, "swap_m": 2, "drop_slice": 63}


@pytest.mark.parametrize("fault", R.FAULTS)
def test_planted_faults_are_noticed(fault):
    first = None
    for n in [1, 2, 3, 63, 64, 65]:
        c, X = _fault_input(n)
        kw = dict(max_iter=8) if fault == "lstres_fixed" else {}   # room to go on where the clean loop stops on stagnation
        clean = R.refine_restated(c.A, c.lu, c.piv, c.B, X, np.float64, **kw)
        bad = R.refine_restated(c.A, c.lu, c.piv, c.B, X, np.float64, fault=fault, **kw)
        if _differs(clean, bad):
            first = n
            break
    print(f"{fault}: first noticed at n = {first}")
    assert first == NOTICED_AT[fault]
