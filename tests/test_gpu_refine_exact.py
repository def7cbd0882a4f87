"""-m gpu: rflu_gerfs_* and rflu_berr_* on inputs whose every number is exactly representable (tests/refine_cases.py: exact_input, proved
on the CPU by tests/test_refine_cases.py; tests/mixed_cases.py: residual_case).  Everything is compared by `==`.

  * X_in[:, k] = c_k x0[:, k] with c_k in {1, 1 + 2^-s}: r = -2^-s b0 exactly, one step returns x0, the next berr is exactly 0:
    X == x0, steps == mask, berr == 0.0, with ipiv and with NULL (NotIPIV), nrhs in {1, 8, 9, 17}; ferr is asked for up to 9 columns
    and must be finite and not negative;
  * rflu_berr_* on integer A, X, B equals max |r| / w formed from the int64 r and w; a zero row contributes 0."""
import numpy as np
import pytest

import mixed_cases as MC
import refine_cases as R
from refine_gpu import berr, gerfs

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
IDS = ["f64", "f32"]


@pytest.mark.parametrize("pivoted", [True, False], ids=["ipiv", "notipiv"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_exact_one_step_returns_x0(dtype, pivoted):
    for n in MC.REFINE_N:
        for nrhs in R.EXACT_NRHS:
            for pattern in MC.PATTERNS:
                e = R.exact_input(n, nrhs, pattern, dtype, pivoted)
                g = gerfs(e.A, e.F, e.ipiv, e.B, e.X_in, dtype, ferr=nrhs <= 9)
                what = (n, nrhs, pattern)
                assert g.info == 0 and g.intact, what
                assert np.array_equal(g.X.astype(np.float64), e.x0), what
                assert np.array_equal(g.steps, e.mask.astype(np.int64)), (what, g.steps)
                assert np.all(g.berr == 0.0), (what, g.berr)
                if g.ferr is not None:
                    assert np.all(np.isfinite(g.ferr)) and np.all(g.ferr >= 0.0), (what, g.ferr)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_exact_max_iter_one_and_default(dtype):
    """max_iter = 1 is enough for these inputs (the step is taken, berr belongs to the X that comes back); max_iter = 0 means 5"""
    e = R.exact_input(129, 9, "mixed_a", dtype)
    for mi in (1, 0, -3):
        g = gerfs(e.A, e.F, e.ipiv, e.B, e.X_in, dtype, ferr=False, max_iter=mi)
        assert np.array_equal(g.X.astype(np.float64), e.x0) and np.array_equal(g.steps, e.mask.astype(np.int64)) and np.all(g.berr == 0.0)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", MC.RESIDUAL_N)
def test_berr_of_integer_inputs(n, dtype):
    A, X, B, Rr = MC.residual_case(n)
    if n >= 3:
        A, B, Rr = A.copy(), B.copy(), Rr.copy()
        A[2, :], B[2, :], Rr[2, :] = 0.0, 0.0, 0.0                      # a row whose terms are all zero contributes 0
    W = np.abs(B) + np.abs(A) @ np.abs(X)                                # integers far below 2^53
    with np.errstate(invalid="ignore", divide="ignore"):
        want = np.where(W == 0, 0.0, np.abs(Rr) / W).max(axis=0)
    for nrhs in MC.RESIDUAL_NRHS:
        got = berr(A, X[:, :nrhs], B[:, :nrhs], dtype)
        assert np.array_equal(got, want[:nrhs]), (n, nrhs, got, want[:nrhs])
    assert np.array_equal(berr(A, X, B, dtype, pad=3, off=1), want)      # padded leading dimensions, the element-load path
