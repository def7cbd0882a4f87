"""What tests/test_gpu_complex_batched.py relies on, checked on the CPU: the inputs of tests/complex_batched_cases.py sit on no pivot
fork in ComplexF64 (so exact ipiv equality is a legitimate demand there), the ComplexF32 fork rule accepts the restatement and refuses
a wrong pivot, the exact inputs have the info the GPU test expects, and the restatement's own solves sit far below the backward-error
bar, so the bar hides no failure."""
import numpy as np
import pytest

import complex_batched_cases as CB
import complex_ref as CR
import complex_solve_ref as CSR


@pytest.mark.parametrize("shape", CB.SHAPES["cf64"])
def test_cf64_inputs_sit_on_no_pivot_fork(shape):
    """Exact ipiv equality is demanded for ComplexF64.  It is legitimate when no search of the restatement sees two candidates closer
    than the rounding differences between two correct implementations (m eps); the demand here is a million times that.  Measured on
    these inputs: the smallest gap is 6.1e-5, at 33 x 31 (8e9 m eps64)."""
    m, n = shape
    for b in range(7):
        gap = CB.min_relative_gap(CB.matrix(m, n, "cf64", b))
        assert gap >= 1e6 * m * CB.eps_of("cf64"), (shape, b, gap)


def test_cf32_gaps_can_be_at_rounding_level():
    """Why ComplexF32 gets the fork rule instead: on these inputs a search can see two moduli within a few m eps32 of each other."""
    worst = min(CB.min_relative_gap(CB.matrix(m, n, "cf32", b)) / (m * CB.eps_of("cf32"))
                for (m, n) in [(100, 60), (128, 128)] for b in range(7))
    print(f"smallest ComplexF32 gap on 100x60 / 128x128, b < 7: {worst:.2f} m eps32")
    assert worst < 1e3


def test_cf32_fork_rule_accepts_the_restatement_and_refuses_a_wrong_row():
    m, n = 33, 31
    A = CB.matrix(m, n, "cf32", 3)
    _, ip, info = CB.ref_factors(m, n, "cf32", 3)
    assert info == 0
    # the restatement in the input precision passes (equal, or a fork inside the margin)
    CB.check_ipiv_cf32(A, ip)
    # a pivot that is not (nearly) the largest modulus does not
    _, ip128, _, mods = CR.complex_generic_lufact(A.astype(np.complex128), True, moduli=True)
    bad = ip128.copy()
    bad[0] = int(np.argmin(mods[0])) + 1
    assert bad[0] != ip128[0]
    with pytest.raises(AssertionError):
        CB.check_ipiv_cf32(A, bad)


@pytest.mark.parametrize("case", CB.EXACT)
def test_exact_inputs_have_the_expected_info(case):
    (m, n), empty, sfxs, want = case
    for sfx in sfxs:
        A = CR.exact_complex(m, n, empty, CB.CTYPES[sfx])
        assert max(m, n) <= CB.LIMIT[sfx]
        F, ip, info = CR.complex_generic_lufact(A, True)
        assert info == want
        # exact in both precisions: the complex64 factors are the complex128 ones
        F128, ip128, info128 = CR.complex_generic_lufact(A.astype(np.complex128), True)
        assert info128 == want and np.array_equal(ip, ip128) and np.array_equal(F.astype(np.complex128), F128)


@pytest.mark.parametrize("sfx", ["cf64", "cf32"])
def test_the_restatements_solves_sit_far_below_the_bar(sfx):
    """bar_E(n) = 20 n eps is the project's bar (test/runtests.jl:19).  The restatement's own solves, in the input precision, on every
    input of the GPU test: worst 0.03 of the bar at n = 1 and <= 0.003 of it from n = 7 on."""
    worst = {}
    for n in CB.SQUARE[sfx]:
        for b in range(max(CB.BATCHES)):
            A = CB.matrix(n, n, sfx, b)
            F, ip, info = CB.ref_factors(n, n, sfx, b)
            assert info == 0
            for nrhs in CB.NRHS:
                B = CB.rhs(n, nrhs, sfx, b)
                for trans in "NTC":
                    be = CB.backward_error(A, CB.ref_solve(F, ip, B, trans), B, trans)
                    assert be <= CB.bar_E(n, sfx), (n, b, nrhs, trans, be)
                    worst[n] = max(worst.get(n, 0.0), be / CB.bar_E(n, sfx))
    print({n: f"{w:.4f}" for n, w in worst.items()})
    assert all(w <= 0.1 for w in worst.values())


def test_t_and_c_are_different_operators_on_these_inputs():
    """A transposed solve judged against the adjoint operator misses the bar by orders of magnitude: a swapped flag cannot pass."""
    n, sfx = 32, "cf64"
    A, B = CB.matrix(n, n, sfx, 0), CB.rhs(n, 8, sfx, 0)
    assert np.abs(A.imag).min() > 0
    F, ip, _ = CB.ref_factors(n, n, sfx, 0)
    Xt = CB.ref_solve(F, ip, B, "T")
    assert CB.backward_error(A, Xt, B, "T") <= CB.bar_E(n, sfx)
    assert CB.backward_error(A, Xt, B, "C") > 1e6 * CB.bar_E(n, sfx)


def test_forward_solve_agrees_with_numpy_and_the_transposed_restatement():
    n, sfx = 33, "cf64"
    A = CB.matrix(n, n, sfx, 1)
    F, ip, _ = CB.ref_factors(n, n, sfx, 1)
    B = CB.rhs(n, 3, sfx, 1)
    X = CB.forward_solve(F, ip, B)
    assert np.allclose(X, np.linalg.solve(A, B), rtol=1e-9, atol=0)
    assert np.allclose(CSR.trans_solve(F, ip, B, 1), np.linalg.solve(A.conj().T, B), rtol=1e-9, atol=0)


def test_batches_leave_the_last_workgroup_partly_empty():
    """4, 2 and 1 matrices per 256-thread workgroup: 1, 7 and 67 are no multiple of 4 or 2, and 67 fills more than one workgroup of each."""
    for groups in (4, 2):
        assert all(b % groups for b in CB.BATCHES)
    assert max(CB.BATCHES) > 4 * 4
    for sfx, shapes in CB.SHAPES.items():
        sizes = {max(s) for s in shapes}
        assert {32, 33, 64} <= sizes and max(sizes) == CB.LIMIT[sfx] and max(CB.FALLBACK[sfx]) == CB.LIMIT[sfx] + 1
    assert {64, 65, 128} <= {max(s) for s in CB.SHAPES["cf32"]}
