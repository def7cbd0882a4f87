"""The exact solve inputs of tests/solve_cases.py, proven on the host (no GPU).

`chain` restates the arithmetic of the cooperative chain (trsv.hip) for one triangle in the element type under test:
    y_r = inv(D_rr) (b_r - sum over the FAR blocks c of T_rc x_c),     x_r = y_r - (inv(D_rr) T_rp) x_p,
p being the block solved right before r, with the far blocks taken in a shuffled order.  On the generator's inputs it must return
x_true BIT FOR BIT in Float32 and in Float64, every intermediate must be a multiple of 1/2 below 2^20, and so must the sums of absolute
values that bound every partial sum of every other order (an MFMA's, the recursive splitting's).
"""
import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse.linalg as spla

from solve_cases import NB, SolveCase, solve_case

SIZES = [1, 63, 64, 65, 129, 300, 1000]
LIMIT = float(2 ** 20)


class Stats:
    def __init__(self):
        self.largest = 0.0

    def note(self, v):
        v = np.asarray(v, dtype=np.float64)
        assert np.array_equal(2 * v, np.rint(2 * v)), "an intermediate is no multiple of 1/2"
        m = float(np.abs(v).max()) if v.size else 0.0
        assert m < LIMIT, m
        self.largest = max(self.largest, m)


def chain(tri, lower, b, dtype, rng, st):
    """One triangle (dense float64 `tri`, diagonal included) in blocks of NB rows, all arithmetic in `dtype`."""
    n = tri.shape[0]
    nb = (n + NB - 1) // NB
    x = np.zeros(b.shape, dtype=dtype)
    order = list(range(nb)) if lower else list(range(nb - 1, -1, -1))
    blk = lambda r: slice(r * NB, min(n, (r + 1) * NB))
    for q, r in enumerate(order):
        rs = blk(r)
        d = tri[rs, rs]
        dinv = sla.solve_triangular(d, np.eye(d.shape[0]), lower=lower)
        assert np.array_equal(d @ dinv, np.eye(d.shape[0]))
        assert np.isin(dinv, (0.0, 1.0, -1.0, 0.5, -0.5)).all(), "inverse of a diagonal block outside {0, +-1, +-1/2}"
        dinv = dinv.astype(dtype)
        p = order[q - 1] if q > 0 else None
        far = order[:max(q - 1, 0)]
        rng.shuffle(far)
        acc = b[rs].astype(dtype)
        bound = np.abs(acc).astype(np.float64)
        for c in far:
            t = tri[rs, blk(c)].astype(dtype)
            acc = acc - t @ x[blk(c)]
            assert acc.dtype == dtype
            st.note(acc)
            bound += np.abs(t).astype(np.float64) @ np.abs(x[blk(c)]).astype(np.float64)
        st.note(bound)
        y = dinv @ acc
        st.note(y)
        st.note(np.abs(dinv).astype(np.float64) @ np.abs(acc).astype(np.float64))
        if p is not None:
            m = dinv @ tri[rs, blk(p)].astype(dtype)
            st.note(m)
            st.note(np.abs(dinv).astype(np.float64) @ np.abs(tri[rs, blk(p)]))
            mx = m @ x[blk(p)]
            st.note(mx)
            st.note(np.abs(m).astype(np.float64) @ np.abs(x[blk(p)]).astype(np.float64))
            y = y - mx
        assert y.dtype == dtype
        st.note(y)
        x[rs] = y
    return x


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", SIZES)
def test_blockwise_restatement_returns_x_true_exactly(n, dtype):
    case = SolveCase(n, 12, seed=n)
    L, U = case.L().toarray().astype(np.float64), case.U().toarray().astype(np.float64)
    st = Stats()
    rng = np.random.default_rng(7 + n)
    want = case.x_true.astype(dtype)
    bf, bt = case.b_forward(), case.b_transposed()
    st.note(bf); st.note(bt)
    # forward: B <- U^-1 L^-1 P B
    z = chain(L, True, case.apply_p(bf), dtype, rng, st)
    x = chain(U, False, z, dtype, rng, st)
    assert x.dtype == dtype and np.array_equal(x, want)
    # transposed: B <- P^T L^-T U^-T B; the lower triangle is U^T, the upper one L^T
    z = chain(np.ascontiguousarray(U.T), True, bt, dtype, rng, st)
    x = case.apply_pt(chain(np.ascontiguousarray(L.T), False, z, dtype, rng, st))
    assert x.dtype == dtype and np.array_equal(x, want)
    print(f"n={n} {np.dtype(dtype).name}: largest intermediate {st.largest}, max|B| {max(np.abs(bf).max(), np.abs(bt).max())}")


@pytest.mark.parametrize("n", SIZES + [2, 3, 127, 128, 191, 257])
def test_factors_have_the_promised_shape(n):
    case = SolveCase(n, 3, seed=n)
    L, U, F = case.L().toarray(), case.U().toarray(), case.dense_factors()
    i = np.arange(n)
    assert np.array_equal(np.tril(L), L) and np.array_equal(np.diag(L), np.ones(n)) and np.isin(L, (-1, 0, 1)).all()
    assert np.array_equal(np.triu(U), U) and np.isin(np.diag(U), (-2, -1, 1, 2)).all() and np.isin(U, (-2, -1, 0, 1, 2)).all()
    assert np.array_equal(F, np.tril(L, -1) + U)
    for r0 in range(0, n, NB):   # bidiagonal inside every diagonal block, with the ratios of the docstring
        s = slice(r0, min(n, r0 + NB))
        assert np.array_equal(np.tril(L[s, s], -2), np.zeros_like(L[s, s])) and np.array_equal(np.triu(U[s, s], 2), np.zeros_like(U[s, s]))
    assert np.isin(U[i[:-1], i[1:]], (0, 1, -1, 2, -2)).all() and (np.abs(U[i[:-1], i[1:]]) % np.abs(U[i[1:], i[1:]]) == 0).all()
    assert (np.abs(U[i[:-1], i[1:]]) <= np.abs(U[i[1:], i[1:]])).all()
    if n > NB:   # three entries per row of L / column of U outside the diagonal block (fewer only where two fell on one place)
        rows = np.arange(NB, n)
        far_l = np.array([np.count_nonzero(L[r, :NB * (r // NB)]) for r in rows])
        far_u = np.array([np.count_nonzero(U[:NB * (c // NB), c]) for c in rows])
        assert far_l.max() <= 4 and far_u.max() <= 4 and far_l.mean() > 2.5 and far_u.mean() > 2.5
    # interchanges: valid, and more than half of them (and of the rows) move
    assert case.ipiv.dtype == np.int64 and (case.ipiv >= i + 1).all() and (case.ipiv <= n).all()
    if n >= 3:
        assert np.count_nonzero(case.ipiv != i + 1) > n / 2
        assert np.count_nonzero(case.perm() != i) > n / 2
    X = np.arange(3 * n).reshape(n, 3)
    Y = X.copy()
    for k, t in enumerate(case.ipiv):
        Y[[k, t - 1]] = Y[[t - 1, k]]
    assert np.array_equal(case.apply_p(X), Y) and np.array_equal(case.apply_pt(Y), X)
    # the right-hand sides against dense products with an explicit permutation matrix (Float64: exact on integers this small)
    P = np.eye(n)[case.perm()]
    A = P.T @ L.astype(np.float64) @ U.astype(np.float64)
    assert np.abs(A).max() < 2 ** 30
    assert np.array_equal(case.b_forward(), A @ case.x_true) and np.array_equal(case.b_transposed(), A.T @ case.x_true)


def test_columns_do_not_depend_on_nrhs_and_the_cache_returns_one_object():
    a, b = SolveCase(130, 5, seed=3), SolveCase(130, 9, seed=3)
    assert np.array_equal(a.ipiv, b.ipiv) and all(np.array_equal(u, v) for u, v in zip(a.packed(), b.packed()))
    assert solve_case(130, 5, 3) is solve_case(130, 5, 3)
    assert not np.array_equal(SolveCase(130, 5, seed=4).ipiv, a.ipiv)


@pytest.mark.parametrize("row_major", [True, False])
def test_device_builder_places_the_factors_by_index(row_major):
    torch = pytest.importorskip("torch")
    n, ld = 130, 135
    case = SolveCase(n, 1, seed=5)
    t = case.device_factors(torch.float32, row_major, ld, device="cpu", pad=float("nan"))
    assert tuple(t.shape) == (n, ld) and t.dtype == torch.float32
    got = t.numpy()
    F = case.dense_factors(np.float32)
    assert np.array_equal(got[:, :n], F if row_major else F.T) and np.isnan(got[:, n:]).all()


def test_bookkeeping_at_the_largest_size_without_dense_matrices():
    """n = 49217 = 3 * 16384 + 65 (all four slots of the narrow chain, partial last block): coordinate lists and sparse products only."""
    n, nrhs = 49217, 9
    case = SolveCase(n, nrhs, seed=1)
    i = np.arange(n)
    assert (case.ipiv >= i + 1).all() and (case.ipiv <= n).all() and np.count_nonzero(case.ipiv != i + 1) > n / 2
    assert np.count_nonzero(case.perm() != i) > n / 2 and np.array_equal(np.sort(case.perm()), i)
    r, c, v = case.packed()
    assert r.size < 10 * n and np.unique(r * n + c).size == r.size and (v != 0).all()
    lr, lc, lv = case.lower
    ur, uc, uv = case.upper
    assert (lr > lc).all() and np.isin(lv, (-1, 1)).all() and (ur <= uc).all() and np.isin(uv, (-2, -1, 1, 2)).all()
    assert np.count_nonzero(ur == uc) == n
    bf, bt = case.b_forward(), case.b_transposed()
    assert bf.dtype == np.int64 and bf.shape == (n, nrhs) and max(np.abs(bf).max(), np.abs(bt).max()) < 2 ** 20
    # sparse substitution in Float64 (exact on these values) gives x_true back
    L, U = case.L().astype(np.float64), case.U().astype(np.float64)
    z = spla.spsolve_triangular(L, case.apply_p(bf).astype(np.float64), lower=True, unit_diagonal=True)
    x = spla.spsolve_triangular(U, z, lower=False)
    assert np.array_equal(x, case.x_true)
    z = spla.spsolve_triangular(U.T.tocsr(), bt.astype(np.float64), lower=True)
    x = case.apply_pt(spla.spsolve_triangular(L.T.tocsr(), z, lower=False, unit_diagonal=True))
    assert np.array_equal(x, case.x_true)
    print(f"n={n}: {r.size} stored entries, max|B| {max(np.abs(bf).max(), np.abs(bt).max())}")
