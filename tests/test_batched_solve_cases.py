"""CPU: what tests/test_gpu_batched_solve_exact.py rests on (tests/batched_solve_cases.py), proven without a GPU.

  * the constants the grids were chosen for are the ones the sources state;
  * every constructed member used on the GPU meets the sum-of-moduli certificate (below 2^24 grid units), so `==` is a fair demand in any
    order of summation; the worst sums are printed;
  * the restatement of both kernels returns x_true by `==` in both element precisions, for every operator, orientation and pass count,
    packed and padded;
  * every planted fault changes the result at the size NOTICED names for it -- the smallest (n, nrhs, batch) of the GPU grids at which
    the GPU test relies on noticing it;
  * the restatement's componentwise backward error on the general inputs, next to LAPACK's on the same factors: both bars of the GPU
    test are met by this order of summation with the margin the docstring of test_restatement_meets_both_rounding_bars reports."""
import numpy as np
import pytest

import batched_solve_cases as C


def test_constants_match_the_sources():
    h = C.header_constants()
    assert h == {"BNR": C.BNR, "BT": C.BT, "BATCHED_MAX_DIM": C.BATCHED_MAX_DIM, "CBATCHED_MAX_DIM_CF32": C.CBATCHED_MAX_DIM_CF32,
                 "CBATCHED_MAX_DIM_CF64": C.CBATCHED_MAX_DIM_CF64}
    assert C.BNR == 8 and C.GRID_NRHS == [1, C.BNR - 1, C.BNR, C.BNR + 1, 2 * C.BNR, 2 * C.BNR + 1]
    for s in C.SFX:
        assert max(C.sizes(s)) == C.LIMIT[s] and C.ABOVE[s] == C.LIMIT[s] + 1
    # 64 | 128 | 256 threads per matrix: the sizes on both sides of 32 and 64, and 67 leaves a partly empty last workgroup for 4, 2, 1
    assert {31, 32, 33, 63, 64, 65} <= set(C.GRID_N) and all(67 % g for g in (4, 2)) and C.BT == 256
    for s in C.SFX:    # every value of every axis occurs in part (a)
        g = C.exact_grid(s)
        assert {c[0] for c in g} == set(C.sizes(s)) and {c[1] for c in g} == set(C.GRID_NRHS)
        assert {(c[2], c[3]) for c in g} == {(b, v) for b in C.BATCHES for v in (True, False)}


def members_used(kind):
    """every (n, copy, which) the GPU test builds for this kind"""
    ns = sorted(set(C.GRID_N) | {129, 65})
    out = [(n, k, w) for n in ns for k in range(5) for w in ("random", "identity")]
    return out + [(n, k, w) for n in C.SPECIAL_N for k in range(5) for w in C.INTERCHANGES]


@pytest.mark.parametrize("kind", ["real", "complex"])
def test_every_member_meets_the_certificate(kind):
    worst = {op: (0.0, None) for op in C.OPS[kind]}
    for n, k, w in members_used(kind):
        c = C.member(n, kind, k, w)
        for op, s in c.sums.items():
            assert s < C.FLOAT32_LIMIT, (n, k, w, op, s)
            worst[op] = max(worst[op], (s, (n, k, w)))
        assert c.ipiv.min() >= 1 and c.ipiv.max() <= n and np.all(c.ipiv >= np.arange(1, n + 1))
    print(f"{kind}: worst sum of moduli in grid units of 1/2, of 2^24 = {C.FLOAT32_LIMIT:.0f}: {worst}")


def test_the_special_interchanges_are_what_they_claim():
    for n in C.SPECIAL_N:
        ident, last, cross = (C.interchanges(n, w) for w in C.INTERCHANGES)
        assert np.array_equal(C.IC.compose_interchanges(ident, n), np.arange(n))
        assert np.array_equal(C.IC.compose_interchanges(last, n), np.roll(np.arange(n), 1))      # row n - 1 went through every position
        assert np.all(cross[:64] > 64) and np.array_equal(cross[64:], np.arange(65, n + 1))
        assert np.array_equal(C.IC.compose_interchanges(cross, n), C.CR.perm_of(cross, n))
        if n == 128:
            assert sorted(cross[:64]) == list(range(65, 129))
    # random interchanges repeat their targets: the composition is no product of disjoint exchanges
    ip = C.member(33, "real", 0).ipiv
    assert len(set(ip.tolist())) < 33


@pytest.mark.parametrize("sfx,n", [(s, n) for s in C.SFX for n in C.sizes(s)])
def test_restatement_returns_x_true(n, sfx):
    """two members (their own factors, interchanges and solution each), every nrhs of this n, every operator, both orientations"""
    kind, dtype = C.KIND[sfx], C.DTYPE[sfx]
    cs = [C.member(n, kind, k) for k in range(2)]
    F = np.stack([c.F for c in cs]).astype(dtype)
    ipiv = np.stack([c.ipiv for c in cs])
    for nrhs in C.nrhs_of(n):
        want = np.stack([c.X[:, :nrhs] for c in cs]).astype(dtype)
        for op in C.OPS[kind]:
            B = np.stack([c.B[op][:, :nrhs] for c in cs]).astype(dtype)
            for row_major in (False, True):
                X = C.solve_packed(F, ipiv, B, op, row_major)
                assert X.dtype == dtype and (X == want).all(), (n, nrhs, op, row_major, int((X != want).sum()))


@pytest.mark.parametrize("sfx", C.SFX)
def test_restatement_with_padded_storage(sfx):
    """the storage of part (b) of the GPU test: the padding keeps its sentinel, F and ipiv are only read"""
    n, nrhs, batch = 9, 9, 3
    kind, dtype = C.KIND[sfx], C.DTYPE[sfx]
    cs = [C.member(n, kind, k) for k in range(batch)]
    for row_major in (False, True):
        lda, sip = n + 3, n + 1
        sF = lda * n + 5
        ldb = (nrhs if row_major else n) + 2
        sB = ldb * (n if row_major else nrhs) + 3
        Fb, ip = np.full(batch * sF, np.nan, dtype=dtype), np.full(batch * sip, -7, dtype=np.int64)
        for op in C.OPS[kind]:
            Bb = np.full(batch * sB, np.nan, dtype=dtype)
            for b, c in enumerate(cs):
                i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
                Fb[b * sF + (i * lda + j if row_major else i + j * lda)] = c.F.astype(dtype)
                ip[b * sip: b * sip + n] = c.ipiv
                i, j = np.meshgrid(np.arange(n), np.arange(nrhs), indexing="ij")
                Bb[b * sB + (i * ldb + j if row_major else i + j * ldb)] = c.B[op][:, :nrhs].astype(dtype)
            out = C.restatement(Fb, lda, sF, ip, sip, Bb, ldb, sB, batch, n, nrhs, row_major, op)
            assert np.array_equal(np.isnan(out), np.isnan(Bb))
            for b, c in enumerate(cs):
                got = out[b * sB + (i * ldb + j if row_major else i + j * ldb)]
                assert (got == c.X[:, :nrhs].astype(dtype)).all(), (op, row_major, b)


# mutation -> (kind, n, nrhs, batch, operator, row_major): the smallest size of the GPU grids (n from GRID_N, nrhs from GRID_NRHS, batch
# from BATCHES; members as mixed_batch places them) at which the result of a CONSTRUCTED member changes.  Found by walking the grids
# (test_the_named_sizes_are_the_smallest repeats the walk).
NOTICED = {
    "backward_skips_last_column": ("real", 2, 1, 1, "N", False),
    "no_final_division": ("real", 1, 1, 1, "N", False),
    "inverse_perm": ("real", 7, 1, 1, "N", False),
    "gather_for_scatter": ("real", 7, 1, 1, "T", False),
    "ignore_p1": ("real", 65, 1, 1, "N", False),
    "ignore_j0": ("real", 1, 9, 1, "N", False),
    "neighbour_ipiv": ("real", 2, 1, 3, "N", False),
    "strideB_for_strideF": ("real", 2, 1, 3, "N", False),
    "t_for_c": ("complex", 1, 1, 1, "C", False),
    "c_for_t": ("complex", 1, 1, 1, "T", False),
    "recip_unconjugated": ("complex", 1, 1, 1, "C", False),
    "rm_load_as_cm": ("real", 2, 7, 1, "N", True),
}


def _cpu_factors(n, sfx):
    return lambda b: C.cpu_factors(n, sfx, b)


def noticed(mutation, sfx, n, nrhs, batch, op, row_major):
    """does the fault change a constructed member of the mixed batch of the GPU test?"""
    F, ipiv, B, exact = C.mixed_batch(n, sfx, batch, _cpu_factors(n, sfx))
    X = C.solve_packed(F, ipiv, B[op][:, :, :nrhs], op, row_major, mutation=mutation)
    good = C.solve_packed(F, ipiv, B[op][:, :, :nrhs], op, row_major)
    dtype = C.DTYPE[sfx]
    for b, c in exact.items():
        assert (good[b] == c.X[:, :nrhs].astype(dtype)).all()
    return any(not (X[b] == c.X[:, :nrhs].astype(dtype)).all() for b, c in exact.items())


def test_every_mutation_is_named():
    assert set(NOTICED) == set(C.MUTATIONS)


@pytest.mark.parametrize("mutation", C.MUTATIONS)
def test_every_mutation_is_noticed(mutation):
    kind, n, nrhs, batch, op, row_major = NOTICED[mutation]
    for sfx in C.SFX:
        if C.KIND[sfx] == kind:
            assert noticed(mutation, sfx, n, nrhs, batch, op, row_major), (mutation, sfx)
    # and the complex kernel's copies of the shared lines notice the shared faults too (at a size where a zero draw cannot hide them)
    if kind == "real":
        for sfx in ("cf64", "cf32"):
            if n <= C.LIMIT[sfx]:
                assert noticed(mutation, sfx, max(n, 9), max(nrhs, 7) if row_major else nrhs, batch, op, row_major), (mutation, sfx)


@pytest.mark.parametrize("mutation", C.MUTATIONS)
def test_the_named_sizes_are_the_smallest(mutation):
    """walk the batches, then nrhs, then n through the GPU grids up to the named size: nothing before it notices"""
    kind, n0, nrhs0, batch0, op, row_major = NOTICED[mutation]
    sfx = "f32" if kind == "real" else "cf32"
    target = (batch0, nrhs0, n0)
    for batch in C.BATCHES:
        for nrhs in C.GRID_NRHS:
            for n in C.GRID_N:
                if (batch, nrhs, n) >= target:
                    return
                if nrhs in C.nrhs_of(n):
                    assert not noticed(mutation, sfx, n, nrhs, batch, op, row_major), (mutation, n, nrhs, batch)


@pytest.mark.parametrize("sfx", C.SFX)
def test_restatement_meets_both_rounding_bars(sfx):
    """The restatement on the first CPU_MEMBERS general members (the CPU comparator's factors: partial pivoting, no diagonal shift, so
    interchanges occur), n in ROUNDING_N, nrhs 1 and 9, every operator: omega <= n eps (real) / 4 n eps (complex), and
    omega <= 16 max(omega_ref, eps / 8) with omega_ref from scipy.linalg.lu_solve on the same factors -- the project's margin is fair
    for this order of summation.  The test prints the worst omega / eps and omega / max(omega_ref, eps / 8) per operator; as committed:
        f64   N 0.47, 2.96    T 0.76, 2.49                        f32   N 0.64, 3.44    T 0.63, 2.22
        cf64  N 0.37, 2.02    T 0.41, 2.52    C 0.36, 1.92        cf32  N 0.36, 1.87    T 0.58, 2.34    C 0.46, 1.87
    so the worst ratio times four is 13.8, inside the project's 16: the margin stays as tests/test_gpu_solve_exact.py has it."""
    kind, dtype, eps = C.KIND[sfx], C.DTYPE[sfx], C.eps_of(sfx)
    worst = {op: [0.0, 0.0] for op in C.OPS[kind]}
    for n in C.ROUNDING_N:
        if n > C.LIMIT[sfx]:
            continue
        fac = [C.cpu_factors(n, sfx, b) for b in range(C.CPU_MEMBERS)]
        F, ipiv = np.stack([f for f, _ in fac]), np.stack([p for _, p in fac])
        assert (ipiv != np.arange(1, n + 1)).any()
        perm = C.perms_of(ipiv, n)
        for nrhs in C.ROUNDING_NRHS:
            B = np.array(C.general_rhs_batch(n, nrhs, sfx, C.CPU_MEMBERS))
            for op in C.OPS[kind]:
                X = C.solve_packed(F, ipiv, B, op)
                Xref = np.stack([C.lapack_solve(F[b], ipiv[b], B[b], op) for b in range(C.CPU_MEMBERS)])
                w, wref = C.omega_batch(F, perm, B, X, op), C.omega_batch(F, perm, B, Xref, op)
                assert X.dtype == dtype and (w <= C.complex_c(sfx, n) * eps).all(), (n, nrhs, op, w / eps)
                assert (w <= C.M_RATIO * np.maximum(wref, C.FLOOR * eps)).all(), (n, nrhs, op, w / eps, wref / eps)
                worst[op][0] = max(worst[op][0], float(w.max() / eps))
                worst[op][1] = max(worst[op][1], float((w / np.maximum(wref, C.FLOOR * eps)).max()))
    print(f"{sfx}: " + ", ".join(f"{op}: omega / eps {a:.2f}, omega / max(omega_ref, eps / 8) {r:.2f}" for op, (a, r) in worst.items()))
