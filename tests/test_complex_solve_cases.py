"""The inputs and restatements of tests/complex_solve_cases.py, proven on the host (no GPU).

1. The exact cases: for every n of GRID_N and 'N', 'T', 'C' the right-hand sides are complex64 numbers on the half-integer grid, the
   sums of moduli that bound every partial sum stay below 2^24 grid units, and four independent solves in complex64 and complex128
   (complex_solve_ref.trans_solve / a plain substitution, the narrow and the wide restatement) return X by np.array_equal.
2. The mutations: seven faults planted in the restatements.  EXACT_CATCHES states, per mutation and element type, the sizes of GRID_N at
   which the exact case differs from X -- asserted both ways, so the sizes at which a fault cannot show are stated too -- and
   test_mutation_table prints next to it what the old bar E = 20 n eps on the random input makes of the same fault.
3. The rounding level: omega of both restatements, of a plain substitution and of LAPACK's getrs on general_factors for the rounding
   cases of the GPU test; the worst ratio to LAPACK gives M_RATIO, the factor of assertion (e) 3 of tests/test_gpu_complex_solve_exact.py.
"""
import numpy as np
import pytest
import scipy.linalg as sla

import complex_solve_cases as C
import complex_solve_ref as SR

NAMES = {np.complex128: "ComplexF64", np.complex64: "ComplexF32"}
LAPACK_TRANS = {"N": 0, "T": 1, "C": 2}


def test_header_constants():
    assert C.header_constants() == {"CNB": C.CNB, "CNARROW": C.CNARROW, "CLEAF": C.CLEAF, "CGEMV_WAVES": C.CGEMV_WAVES, "CG_BK": C.CG_BK}
    assert C.CNARROW in C.GRID_NRHS and C.CNARROW + 1 in C.GRID_NRHS
    for b in (C.CLEAF, C.CNB):
        assert {b - 1, b, b + 1} <= set(C.GRID_N)


# ---- 1. the exact cases ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trans", C.TRANS)
@pytest.mark.parametrize("n", C.GRID_N)
def test_exact_case(n, trans):
    c = C.case(n)
    B = C.rhs(c, trans)
    B2 = C.rhs_pairs(n, trans)
    assert B.dtype == np.complex64 and B.shape == (n, C.NRHS_MAX)
    assert np.array_equal(B.astype(np.complex128) * 2, B2[0] + 1j * B2[1])          # B is exactly representable, on the half grid
    first, second = C.row_sums(c, trans)
    print(f"n={n} {trans}: row sums 2^{np.log2(first):.1f} and 2^{np.log2(second):.1f} grid units")
    assert first < C.FLOAT32_LIMIT and second < C.FLOAT32_LIMIT
    for ctype in C.CTYPES:
        F = C.factors_cm(c, ctype)
        Bt, Xt = B.astype(ctype), c.X.astype(ctype)
        assert np.array_equal(C.plain_substitution(F, c.ipiv, Bt[:, :9], trans), Xt[:, :9]), (NAMES[ctype], "plain substitution")
        assert np.array_equal(C.narrow_restatement(F, c.ipiv, Bt[:, :8], trans), Xt[:, :8]), (NAMES[ctype], "narrow")
        assert np.array_equal(C.wide_restatement(F, c.ipiv, Bt[:, :9], trans), Xt[:, :9]), (NAMES[ctype], "wide")
        # a split that the sub-solves and the GEMM share is another correct solve: the exact case cannot and need not tell it apart
        if ctype is np.complex64:
            assert np.array_equal(C.wide_restatement(F, c.ipiv, Bt[:, :9], trans, consistent_wrong_split=True), Xt[:, :9])
        if trans != "N" and n >= 31:
            # (n = 1, 2: at most one interchange, and a real u_11 is its own conjugate)
            wrong_order = SR.trans_solve(F, c.ipiv, Bt[:, :9], trans == "C", first_to_last=True)
            assert not np.array_equal(wrong_order, Xt[:, :9]), "undoing the interchanges first to last gives the same X"
            other = SR.trans_solve(F, c.ipiv, Bt[:, :9], trans != "C")
            assert not np.array_equal(other, Xt[:, :9]), "'T' and 'C' give the same X"
    if trans == "N":
        assert np.array_equal(C.apply_p(c, c.X), c.X[C.perm_of(c.ipiv, n)])


def test_the_widest_block_through_the_wide_restatement():
    """all 130 columns once, at the size with the uneven split"""
    c = C.case(97)
    for trans in C.TRANS:
        for ctype in C.CTYPES:
            X = C.wide_restatement(C.factors_cm(c, ctype), c.ipiv, C.rhs(c, trans).astype(ctype), trans)
            assert np.array_equal(X, c.X.astype(ctype))


# ---- 2. the mutations ------------------------------------------------------------------------------------------------------------------------
# mutation -> (path, the operations it applies to, {element type: the sizes of GRID_N at which the exact case differs from X})
ODD_BAND = [257, 513]                      # n odd and beyond one block: the band right of a block has odd length (1100 is even)
EXACT_CATCHES = {
    # EPL = 2 is ComplexF32 alone
    "odd_tail": ("narrow", C.TRANS, {np.complex64: ODD_BAND, np.complex128: []}),
    # a second round needs a band beyond 4 * 64 * EPL elements: 256 (ComplexF64: 513 has bands of 257 and 512), 512 (ComplexF32)
    "skip_round2": ("narrow", C.TRANS, {np.complex64: [1100], np.complex128: [513, 1100]}),
    # the branch is taken where the row's first band element is off a 16-byte boundary or the lane's pair crosses the band's end:
    # with F aligned and lda = n, ComplexF32 at odd n beyond one block; a ComplexF64 element is 16 bytes, the branch loads nothing
    "no_conj_elementwise": ("narrow", ("C",), {np.complex64: ODD_BAND, np.complex128: []}),
    "no_conj_out": ("wide", ("C",), {t: list(C.GRID_N) for t in C.CTYPES}),
    # phase 3 needs a second 32-row step
    "drop_r4": ("narrow", C.TRANS, {t: [n for n in C.GRID_N if n > 32] for t in C.CTYPES}),
    # the sizes at which some level of the recursion has n / 2 rounded down to 32 different from n1 (64 and 256 split evenly)
    "wrong_split": ("wide", C.TRANS, {t: [65, 97, 255, 257, 513, 1100] for t in C.CTYPES}),
    # a band right of the first block needs n > 256
    "one_term": ("narrow", C.TRANS, {t: [257, 513, 1100] for t in C.CTYPES}),
}
SMALLEST = {"one_term": 257, "odd_tail": 257, "skip_round2": 513, "no_conj_elementwise": 257, "no_conj_out": 1, "drop_r4": 33, "wrong_split": 65}


def _restate(path, F, ipiv, B, trans, mutation, **kw):
    if path == "narrow":
        return C.narrow_restatement(F, ipiv, B[:, :8], trans, mutation, **kw)
    return C.wide_restatement(F, ipiv, B[:, :9], trans, mutation)


def test_the_mutations_cover_the_list():
    assert set(EXACT_CATCHES) == set(C.MUTATIONS)
    for mut, (_, _, sizes) in EXACT_CATCHES.items():
        assert min(min(v) for v in sizes.values() if v) == SMALLEST[mut]


@pytest.mark.parametrize("mutation", C.MUTATIONS)
def test_exact_case_catches_mutation(mutation):
    path, ops, sizes = EXACT_CATCHES[mutation]
    for ctype in C.CTYPES:
        for trans in ops:
            differs = []
            for n in C.GRID_N:
                c = C.case(n)
                X = _restate(path, C.factors_cm(c, ctype), c.ipiv, C.rhs(c, trans).astype(ctype), trans, mutation)
                if not np.array_equal(X, c.X[:, :X.shape[1]].astype(ctype)):
                    differs.append(n)
            assert differs == sizes[ctype], (mutation, NAMES[ctype], trans, differs)


def test_unaligned_leading_dimension_reaches_the_elementwise_branch_at_even_n():
    """lda = n + 3 puts every other row of F off the 16-byte boundary: the GPU test's leading dimension.  Then the missing conjugation of
    the element-by-element branch shows at the even size 1100 too (ComplexF32)."""
    c = C.case(1100)
    F, B = C.factors_cm(c, np.complex64), C.rhs(c, "C")
    assert np.array_equal(C.narrow_restatement(F, c.ipiv, B[:, :8], "C", "no_conj_elementwise", ld=1100), c.X[:, :8])
    assert not np.array_equal(C.narrow_restatement(F, c.ipiv, B[:, :8], "C", "no_conj_elementwise", ld=1103), c.X[:, :8])


OLD_BAR_N = [257, 513, 1100]


def test_mutation_table():
    """What the old bar ||op(A) X - B||_inf / (||op(A)||_inf ||X||_inf) <= E = 20 n eps makes of the same faults on the random input
    (LAPACK's factors of complex_solve_ref.rand_input, right-hand sides complex_ref.rand_rhs).  Recorded, not asserted, but for two
    facts: the unmutated restatements pass the old bar everywhere, and there are ComplexF32 faults at n >= 513 that it lets through
    while the exact case catches them -- the gap the exact tests close."""
    rows, missed = [], []
    for n in OLD_BAR_N:
        for ctype in C.CTYPES:
            lu, piv, _ = C.general_factors(n, ctype)
            ipiv = piv.astype(np.int64) + 1
            B = C.rand_rhs(n, 9, ctype)
            for trans in ("T", "C"):
                for path in ("narrow", "wide"):
                    ok = C.old_bar_ratio(n, ctype, _restate(path, lu, ipiv, B, trans, None), B[:, :8 if path == "narrow" else 9], trans)
                    assert ok < 1.0, (n, NAMES[ctype], trans, path, ok)
                    rows.append((n, NAMES[ctype], trans, f"none ({path})", "-", ok))
                for mutation in C.MUTATIONS:
                    path, ops, sizes = EXACT_CATCHES[mutation]
                    if trans not in ops:
                        continue
                    X = _restate(path, lu, ipiv, B, trans, mutation)
                    ratio = C.old_bar_ratio(n, ctype, X, B[:, :X.shape[1]], trans)
                    exact = n in sizes[ctype]
                    rows.append((n, NAMES[ctype], trans, mutation, "caught" if exact else "cannot differ", ratio))
                    if exact and not ratio > 1.0:
                        missed.append((n, NAMES[ctype], trans, mutation, ratio))
    print("\n    n  type        op  mutation              exact case      old bar (backward error / E)")
    for n, name, trans, mutation, exact, ratio in rows:
        verdict = "" if mutation.startswith("none") else ("caught" if ratio > 1.0 else "NOT caught")
        print(f"{n:5d}  {name:10s}  {trans:2s}  {mutation:20s}  {exact:14s}  {ratio:12.5f} E  {verdict}")
    print(f"faults that the exact case catches and the old bar does not: {len(missed)}")
    assert any(name == "ComplexF32" and n >= 513 for n, name, _, _, _ in missed)


# ---- 3. the rounding level ---------------------------------------------------------------------------------------------------------------------
def _cpu_omegas(n, ctype, trans):
    """per column: omega of LAPACK's getrs and of the wide restatement; of a plain substitution and the narrow restatement (9 columns)"""
    lu, piv, perm = C.general_factors(n, ctype)
    ipiv = piv.astype(np.int64) + 1
    B = C.rand_rhs(n, C.NRHS_MAX, ctype)
    Xref = sla.lu_solve((lu, piv), B, trans=LAPACK_TRANS[trans], check_finite=False)
    assert Xref.dtype == np.dtype(ctype)
    out = {"lapack": C.omega(lu, perm, B, Xref, trans, per_column=True)}
    out["plain"] = C.omega(lu, perm, B[:, :9], C.plain_substitution(lu, ipiv, B[:, :9], trans), trans, per_column=True)
    out["narrow"] = C.omega(lu, perm, B[:, :9], C.narrow_restatement(lu, ipiv, B[:, :9], trans), trans, per_column=True)
    out["wide"] = C.omega(lu, perm, B, C.wide_restatement(lu, ipiv, B, trans), trans, per_column=True)
    return out


def test_cpu_omegas_and_the_factor_m():
    """omega / eps of LAPACK, a plain substitution and both restatements for the rounding cases (n, nrhs) of the GPU test, per operation
    and element type; a case of nrhs columns is the first nrhs columns of the widest block (rand_rhs counts down the columns, and no
    path lets one column see another).  M_RATIO = 4 * (the worst ratio of a restatement to LAPACK), rounded up to a power of two: the
    factor of four is what tests/test_gpu_solve_exact.py allows the GPU's different summation order."""
    worst = {"narrow": (0.0, None), "wide": (0.0, None), "plain": (0.0, None)}
    lo, hi = {k: np.inf for k in ("lapack", "plain", "narrow", "wide")}, {k: 0.0 for k in ("lapack", "plain", "narrow", "wide")}
    for ctype in C.CTYPES:
        eps = C.eps_of(ctype)
        for n in C.ROUNDING_N:
            for trans in C.TRANS:
                w = _cpu_omegas(n, ctype, trans)
                for nrhs in C.ROUNDING_NRHS:
                    ref = float(w["lapack"][:nrhs].max())
                    line = f"omega/eps n={n} nrhs={nrhs} {trans} {NAMES[ctype]}: lapack {ref / eps:.3f}"
                    for k in ("plain", "narrow", "wide"):
                        if k != "wide" and nrhs > 9:
                            continue
                        om = float(w[k][:nrhs].max())
                        line += f"  {k} {om / eps:.3f} ({om / ref:.2f} x)"
                        assert om <= C.complex_c(n) * eps
                        lo[k], hi[k] = min(lo[k], om / eps), max(hi[k], om / eps)
                        if om / ref > worst[k][0]:
                            worst[k] = (om / ref, (n, nrhs, trans, NAMES[ctype]))
                    lo["lapack"], hi["lapack"] = min(lo["lapack"], ref / eps), max(hi["lapack"], ref / eps)
                    print(line)
    for k in lo:
        print(f"{k}: omega = {lo[k]:.3f} .. {hi[k]:.3f} eps")
    for k, (r, where) in worst.items():
        print(f"worst ratio to LAPACK, {k}: {r:.2f} at (n, nrhs, op, type) = {where}")
    ratio = max(worst["narrow"][0], worst["wide"][0])
    m = 2.0 ** np.ceil(np.log2(4 * ratio))
    print(f"m = 4 * {ratio:.2f} rounded up to a power of two = {m:.0f}")
    assert m == C.M_RATIO
