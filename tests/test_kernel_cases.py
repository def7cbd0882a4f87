"""The exact kernel inputs of tests/kernel_cases.py, proven on the host (no GPU): the bounds that make every partial sum exact, the
independence of the result from the order of summation, a Float32 restatement of the recursive TRSM, the interchange patterns, and the
coverage floor -- every dispatch class the grids are there for is hit often enough, so that trimming a grid fails here."""
import collections

import numpy as np
import pytest

import kernel_cases as KC

EXACT = float(2 ** 24)     # integers below it are exact in Float32


# ------------------------------------------------------------------------------------------------------------------- bounds
@pytest.mark.parametrize("dtype", KC.REAL_DTYPES, ids=["f64", "f32"])
def test_real_gemm_bounds_for_every_grid_entry(dtype):
    worst = 0.0
    for pl in KC.real_placements(dtype):
        ops = KC.real_gemm_operands(dtype, pl)
        for op, lo in ((ops.A, 3), (ops.B, 3), (ops.C, 8)):
            assert op.buf.dtype == dtype and np.array_equal(op.buf, np.rint(op.buf)) and np.abs(op.buf).max() <= lo
        for M, N, K in KC.real_gemm_grid(pl):
            b = ops.bound(M, N, K)
            assert b <= 9 * K + 8 and b < EXACT, (pl, M, N, K, b)
            worst = max(worst, b)
    for dims in KC.GEMM_LARGE:
        ops = KC.real_gemm_operands(dtype, "P0", dims)
        b = ops.bound(*dims)
        assert b <= 9 * dims[2] + 8 and b < EXACT
        worst = max(worst, b)
    assert worst < 2 ** 14
    print(f"real GEMM {np.dtype(dtype).name}: largest bound {worst}")


@pytest.mark.parametrize("dtype", KC.REAL_DTYPES, ids=["cf64", "cf32"])
def test_complex_gemm_bounds_for_every_grid_entry(dtype):
    worst = 0.0
    for pl in KC.complex_placements(dtype):
        ops = KC.complex_gemm_operands(dtype, pl)
        for M, N, K in KC.complex_gemm_grid(pl):
            b = ops.bound(M, N, K)
            assert b <= 18 * K + 8 and b < EXACT, (pl, M, N, K, b)
            worst = max(worst, b)
    assert worst < 2 ** 14
    print(f"complex GEMM {np.dtype(dtype).name}: largest bound {worst}")


def test_placements_have_the_alignment_they_are_named_for():
    for dtype in KC.REAL_DTYPES:
        it = np.dtype(dtype).itemsize
        vw = 16 // it
        for pl in KC.real_placements(dtype):
            o = KC.real_gemm_operands(dtype, pl)
            al = [(op.off * it) % 16 for op in (o.A, o.B, o.C)]
            want = {"P0": [0, 0, 0], "P1": [0, 0, it], "P2": [it, 0, 0], "P3": [0, it, 0], "P4": [0, 0, 0], "P5": [8, 8, 0]}[pl]
            assert al == want, (pl, al)
            if pl == "P0":
                assert o.A.ld % 16 == 0 and o.B.ld % 16 == 0 and o.C.ld % 16 == 0
            assert (o.C.ld % 2 == 1) == (pl == "P1") and (o.A.ld % 2 == 1) == (pl == "P4") and (o.B.ld % 2 == 1) == (pl == "P4")
            assert KC.real_vec_ok(o.A.off, o.B.off, o.A.ld, o.B.ld, dtype) == (pl in ("P0", "P1"))
        for pl in KC.complex_placements(dtype):
            o = KC.complex_gemm_operands(dtype, pl)
            al = [(op.off * it) % 16 for op in (o.A, o.B, o.C)]
            want = {"Q0": [0, 0, 0], "Q1": [8, 8, 8], "Q2": [0, 0, 0], "Q3": [8, 0, 0], "Q4": [0, 0, 8]}[pl]
            assert al == want, (pl, al)
            assert (o.A.ld % 2 == 1) == (pl == "Q2") and (o.B.ld % 2 == 1) == (pl == "Q2")
            assert KC.complex_vec_ok(o.A.off, o.B.off, o.C.off, o.A.ld, o.B.ld, dtype) == (pl == "Q0")


def test_expected_buffers_change_the_window_only():
    for ops, (M, N, K) in ((KC.real_gemm_operands(np.float32, "P1"), (65, 130, 17)), (KC.complex_gemm_operands(np.float64, "Q1"), (33, 65, 17))):
        exp = ops.expected(M, N, K)
        assert exp.dtype == ops.dtype
        ref = ops.C.values(M, N) - ops.A.values(M, K) @ ops.B.values(K, N)
        assert np.array_equal(ops.C.values(M, N, buf=exp), ref) and np.abs(ref).max() > 8
        mask = np.ones(exp.size, dtype=bool)
        idx = np.lib.stride_tricks.as_strided(np.arange(exp.size)[ops.C.off:], shape=ops.C.view(M, N).shape,
                                              strides=tuple(s // ops.dtype.itemsize * 8 for s in ops.C.view(M, N).strides))
        mask[idx.ravel()] = False
        assert np.array_equal(exp[mask], ops.C.buf[mask]) and mask.sum() == exp.size - M * N * (2 if ops.cplx else 1)


# -------------------------------------------------------------------------------------------------------- order independence
def _int_ref(A, B, C):
    return C.astype(np.int64) - A.astype(np.int64) @ B.astype(np.int64)


@pytest.mark.parametrize("K", [17, 129, 512])
def test_real_gemm_is_order_independent_in_float32(K):
    rng = np.random.default_rng(K)
    M, N = 37, 41
    A = rng.integers(-3, 4, (M, K)).astype(np.float32)
    B = rng.integers(-3, 4, (K, N)).astype(np.float32)
    C = rng.integers(-8, 9, (M, N)).astype(np.float32)
    ref = _int_ref(A, B, C)
    up, down = C.copy(), C.copy()
    for k in range(K):
        up = up - np.outer(A[:, k], B[k])
        down = down - np.outer(A[:, K - 1 - k], B[K - 1 - k])
        assert up.dtype == np.float32
    acc = [np.zeros((M, N), np.float32) for _ in range(4)]
    for s, k0 in enumerate(range(0, K, 16)):
        acc[s % 4] = acc[s % 4] + A[:, k0:k0 + 16] @ B[k0:k0 + 16]
    slabs = C - ((acc[0] + acc[1]) + (acc[2] + acc[3]))
    whole = C - A @ B
    for got in (up, down, slabs, whole):
        assert got.dtype == np.float32 and np.array_equal(got, ref)


@pytest.mark.parametrize("K", [17, 129, 512])
def test_complex_gemm_is_order_independent_in_float32(K):
    rng = np.random.default_rng(100 + K)
    M, N = 23, 29
    Ar, Ai = (rng.integers(-3, 4, (M, K)).astype(np.float32) for _ in range(2))
    Br, Bi = (rng.integers(-3, 4, (K, N)).astype(np.float32) for _ in range(2))
    Cr, Ci = (rng.integers(-8, 9, (M, N)).astype(np.float32) for _ in range(2))
    i64 = lambda x: x.astype(np.int64)
    ref_r = i64(Cr) - (i64(Ar) @ i64(Br) - i64(Ai) @ i64(Bi))
    ref_i = i64(Ci) - (i64(Ar) @ i64(Bi) + i64(Ai) @ i64(Br))

    def chain(order, grouped):
        r, i = Cr.copy(), Ci.copy()
        for k in order:
            rr, ii = np.outer(Ar[:, k], Br[k]), np.outer(Ai[:, k], Bi[k])
            ri, ir = np.outer(Ar[:, k], Bi[k]), np.outer(Ai[:, k], Br[k])
            if grouped:
                r, i = r - (rr - ii), i - (ri + ir)
            else:
                r, i = r - rr + ii, i - ri - ir
        return r, i

    results = [chain(range(K), False), chain(range(K), True), chain(range(K - 1, -1, -1), False), chain(range(K - 1, -1, -1), True)]
    acc = [[np.zeros((M, N), np.float32) for _ in range(4)] for _ in range(2)]
    for s, k0 in enumerate(range(0, K, 16)):
        sl = slice(k0, k0 + 16)
        acc[0][s % 4] = acc[0][s % 4] + Ar[:, sl] @ Br[sl] - Ai[:, sl] @ Bi[sl]
        acc[1][s % 4] = acc[1][s % 4] + (Ar[:, sl] @ Bi[sl] + Ai[:, sl] @ Br[sl])
    results.append(tuple(c - ((a[0] + a[1]) + (a[2] + a[3])) for c, a in ((Cr, acc[0]), (Ci, acc[1]))))
    c64 = (Cr + 1j * Ci).astype(np.complex64) - (Ar + 1j * Ai).astype(np.complex64) @ (Br + 1j * Bi).astype(np.complex64)
    results.append((c64.real, c64.imag))
    for r, i in results:
        assert r.dtype == np.float32 and i.dtype == np.float32
        assert np.array_equal(r, ref_r) and np.array_equal(i, ref_i)


# ----------------------------------------------------------------------------------------------------------------------- TRSM
class Largest:
    def __init__(self):
        self.v = 0.0

    def note(self, x):
        x = np.asarray(x, dtype=np.float64)
        assert np.array_equal(x, np.rint(x)), "an intermediate is no integer"
        if x.size:
            self.v = max(self.v, float(np.abs(x).max()))
        assert self.v < 2 ** 20


def _block_inverse(Lb):
    """Explicit inverse of a unit lower block by forward substitution on the identity, in float64 (exact: entries in {0, +-1})."""
    n = Lb.shape[0]
    X = np.eye(n)
    for i in range(1, n):
        X[i] -= Lb[i, :i] @ X[:i]
    assert np.array_equal(Lb @ X, np.eye(n)) and np.isin(X, (0.0, 1.0, -1.0)).all()
    return X


def _trsm_fused(L, B, st):
    """trsm_fused_kernel: block rows top to bottom, acc = B_d - sum_{e<d} L_de X_e, X_d = inv(L_dd) acc; all in L's dtype."""
    n = L.shape[0]
    assert n <= KC.TRSM_FUSED_MAX
    X = np.zeros_like(B)
    for d0 in range(0, n, KC.NB):
        d1 = min(n, d0 + KC.NB)
        acc = B[d0:d1].copy()
        bound = np.abs(acc).astype(np.float64)
        for e0 in range(0, d0, KC.NB):
            acc = acc - L[d0:d1, e0:e0 + KC.NB] @ X[e0:e0 + KC.NB]
            bound += np.abs(L[d0:d1, e0:e0 + KC.NB]).astype(np.float64) @ np.abs(X[e0:e0 + KC.NB]).astype(np.float64)
            st.note(acc)
        st.note(bound)
        inv = _block_inverse(L[d0:d1, d0:d1].astype(np.float64)).astype(L.dtype)
        X[d0:d1] = inv @ acc
        st.note(np.abs(inv).astype(np.float64) @ np.abs(acc).astype(np.float64))
    assert X.dtype == L.dtype
    return X


def _trsm_rec(L, B, st):
    """driver.cpp: trsm_rec with the block inverses at hand -- fused up to 256 rows, else split at ((leaves + 1) / 2) * 64 with a GEMM between."""
    n = L.shape[0]
    if n <= KC.TRSM_FUSED_MAX:
        return _trsm_fused(L, B, st)
    leaves = (n + KC.NB - 1) // KC.NB
    n1 = ((leaves + 1) // 2) * KC.NB
    X1 = _trsm_rec(L[:n1, :n1], B[:n1], st)
    B2 = B[n1:] - L[n1:, :n1] @ X1
    st.note(B2)
    st.note(np.abs(B[n1:]).astype(np.float64) + np.abs(L[n1:, :n1]).astype(np.float64) @ np.abs(X1).astype(np.float64))
    return np.concatenate([X1, _trsm_rec(L[n1:, n1:], B2, st)])


@pytest.mark.parametrize("n", KC.TRSM_N)
def test_trsm_restatement_returns_x_true_exactly_in_float32(n):
    L, x_true, B = KC.trsm_case(n)
    assert np.array_equal(np.diag(L), np.ones(n)) and np.array_equal(np.tril(L), L) and np.isin(L, (-1, 0, 1)).all()
    assert x_true.shape == (n, max(KC.TRSM_NRHS)) and np.abs(x_true).max() <= 4 and np.array_equal(L @ x_true, B)
    st = Largest()
    st.note(B)
    X = _trsm_rec(L.astype(np.float32), B.astype(np.float32), st)
    assert X.dtype == np.float32 and np.array_equal(X, x_true)
    print(f"n={n}: largest intermediate or bound {st.v}, max|B| {np.abs(B).max()}")


def test_trsm_buffers_carry_the_sentinel_where_nothing_may_be_read_or_written():
    for kind in KC.TRSM_LDL:
        buf, ldl = KC.trsm_l_buffer(129, kind, np.float32)
        L, x_true, B = KC.trsm_case(129)
        assert buf.shape == (129, ldl) and ldl == (132 if kind == "plus3" else 144)
        assert np.array_equal(np.tril(buf[:, :129], -1), np.tril(L, -1))
        assert (buf[np.triu_indices(129)] == np.float32(KC.SENTINEL)).all() and (buf[:, 129:] == np.float32(KC.SENTINEL)).all()
    b, x = KC.trsm_b_buffer(129, 17, np.float64), KC.trsm_b_buffer(129, 17, np.float64, solved=True)
    assert b.shape == x.shape == (129, 20) and (b[:, 17:] == KC.SENTINEL).all() and (x[:, 17:] == KC.SENTINEL).all()
    assert np.array_equal(b[:, :17], B[:, :17]) and np.array_equal(x[:, :17], x_true[:, :17])
    assert np.isfinite(np.float32(KC.SENTINEL)) and [KC.trsm_class(n) for n in (1, 192, 193, 256, 257)] == ["fused", "fused", "fused_slot_reuse", "fused_slot_reuse", "recursive"]


# --------------------------------------------------------------------------------------------------------------- interchanges
@pytest.mark.parametrize("pattern", KC.LASWP_PATTERNS)
def test_laswp_sequential_reference_equals_the_composed_permutation(pattern):
    m, ld = KC.LASWP_M, 1041
    A = KC.laswp_matrix(ld, np.float32)
    assert A[m - 1, ld - 1] == m * ld - 1 and np.array_equal(A.astype(np.int64), np.arange(m * ld).reshape(m, ld))
    for k0, k1 in KC.LASWP_RANGES:
        ipiv, perm = KC.laswp_ipiv(pattern, k0, k1), KC.laswp_perm(pattern, k0, k1)
        assert np.array_equal(np.sort(perm), np.arange(m))
        for c0, ncols in ((17, 9), (16, 1000)):
            ref = KC.laswp_reference(A, c0, ncols, ipiv, k0, k1)
            want = A.copy()
            want[:, c0:c0 + ncols] = A[perm, c0:c0 + ncols]
            assert np.array_equal(ref, want)
        # the chunks' move lists, applied one chunk after the other, are the same permutation again
        rows = np.arange(m)
        for chunk in range(k0 // KC.NB, (k1 + KC.NB - 1) // KC.NB):
            dst, src = KC.laswp_chunk_moves(ipiv, chunk, k1)
            assert len(dst) <= 2 * KC.NB and len(set(dst)) == len(dst) and sorted(dst) == sorted(src)
            new = rows.copy()
            new[dst] = rows[src]
            rows = new
        assert np.array_equal(rows, perm)


def test_laswp_patterns_have_the_move_counts_they_are_there_for():
    for k0, k1 in KC.LASWP_RANGES:
        chunks = range(k0 // KC.NB, (k1 + KC.NB - 1) // KC.NB)
        count = lambda pattern: [len(KC.laswp_chunk_moves(KC.laswp_ipiv(pattern, k0, k1), c, k1)[0]) for c in chunks]
        pivots = [min(c * KC.NB + KC.NB, k1) - c * KC.NB for c in chunks]
        assert count("identity") == [0] * len(chunks)
        assert count("distinct_far") == [2 * p for p in pivots]            # 128 for a full chunk
        assert count("same_far") == [p + 1 for p in pivots]
        assert count("shift") == [p + 1 for p in pivots]
        assert count("next_chunk") == [2 * p for p in pivots]
    full = [len(KC.laswp_chunk_moves(KC.laswp_ipiv("distinct_far", 128, 328), c, 328)[0]) for c in (2, 3, 4, 5)]
    assert full == [128, 128, 128, 16]
    # (e): every row written by a chunk is read, and moved again, by the next one
    ipiv = KC.laswp_ipiv("next_chunk", 64, 214)
    d1, _ = KC.laswp_chunk_moves(ipiv, 1, 214)
    _, s2 = KC.laswp_chunk_moves(ipiv, 2, 214)
    assert set(range(128, 192)) <= set(d1) and set(range(128, 192)) <= set(s2)
    # (f): more than 64 moves in some chunk (both halves of the list), repeated targets and identity entries
    rnd = KC.laswp_ipiv("random", 64, 214)
    assert max(len(KC.laswp_chunk_moves(rnd, c, 214)[0]) for c in (1, 2, 3)) > KC.NB
    assert np.count_nonzero(rnd[64:214] == np.arange(65, 215)) > 0 and len(set(rnd[64:214])) < 150


def test_laswp_column_ranges_take_the_kernel_they_are_there_for():
    for dtype in KC.REAL_DTYPES:
        vwf = 16 // np.dtype(dtype).itemsize
        cls = collections.Counter()
        for ld in KC.LASWP_LD:
            for c0, ncols in KC.laswp_columns(dtype):
                c = KC.laswp_class(0, ld, c0, ncols, dtype)
                assert c == ("vec" if (ld == 1040 and c0 == KC.LASWP_VEC_C0) else "scalar")
                assert c0 + ncols <= 1040
                cls[c] += len(KC.LASWP_RANGES) * len(KC.LASWP_PATTERNS)
        assert KC.laswp_vec_ncols(dtype)[0] == vwf and cls["vec"] >= 8 and cls["scalar"] >= 8
        # strips of 8 lanes x VWF columns, 4 waves per workgroup: one strip, a partial workgroup, more than one workgroup
        strips = [-(-n // (8 * vwf)) for n in KC.laswp_vec_ncols(dtype)]
        assert min(strips) == 1 and 2 in strips and max(strips) > 4


# ------------------------------------------------------------------------------------------- coverage of the dispatch classes
FLOOR = 8


def _count(ops, grid):
    n = collections.Counter()
    for M, N, K in grid:
        cls, flags = ops.classify(M, N, K)
        n[cls] += 1
        n[cls, "n_tail" in flags] += 1
        n[cls, "m_tail" in flags, "n_tail" in flags] += 1
        n[cls, "K", K] += 1
    return n


@pytest.mark.parametrize("dtype", KC.REAL_DTYPES, ids=["f64", "f32"])
def test_real_gemm_grid_covers_every_dispatch_class(dtype):
    for pl in KC.real_placements(dtype):
        n = _count(KC.real_gemm_operands(dtype, pl), KC.real_gemm_grid(pl))
        if pl in ("P0", "P1"):      # vec_ok: everything but the scalar class
            for cls in ("skinny1", "skinny2", "interior", "full_vec_ktail", "edge_vec"):
                assert n[cls] >= FLOOR, (pl, cls, n[cls])
            assert n["scalar"] == 0
            for cls in ("skinny1", "skinny2"):
                assert n[cls, False] >= FLOOR and n[cls, True] >= FLOOR, (pl, cls)     # without / with an N tail
                assert n[cls, True, True] >= FLOOR                                       # an M tail and an N tail together
            # interior tiles with exactly two slabs (the Float64 SPLITC copy: slab(0), an empty loop, slab(nk - 1)) and with three
            assert n["interior", "K", 32] >= FLOOR and n["interior", "K", 48] >= FLOOR
            # a full tile with 16-byte loads and a K tail in one launch, at K below one slab, between one and two, beyond
            for K in (15, 17, 33, 129):
                assert n["full_vec_ktail", "K", K] >= FLOOR, (pl, K)
            assert n["full_vec_ktail", "K", 16] >= FLOOR        # one whole slab: too short for the interior copy
        else:                        # a misaligned A or B or an odd stride: the guarded scalar loads, whatever the shape
            assert n["scalar"] == len(KC.real_gemm_grid(pl)) >= FLOOR
            assert n["scalar", True, True] >= FLOOR and n["scalar", "K", 64] >= FLOOR and n["scalar", "K", 128] >= FLOOR


def test_real_gemm_skinny_launches_have_more_than_one_tile_column():
    ops = KC.real_gemm_operands(np.float64, "P0")
    both = [(M, N, K) for M, N, K in KC.real_gemm_grid("P0")
            if ops.classify(M, N, K)[0] in ("skinny1", "skinny2") and ops.classify(M, N, K)[1] == {"m_tail", "n_tail"} and N > KC.S_BN]
    assert len([c for c in both if c[2] == 64]) >= FLOOR and len([c for c in both if c[2] == 128]) >= FLOOR


def test_large_real_gemm_cases_have_the_remap_facts_claimed_for_them():
    facts = {d: KC.gemm_remap_facts(d[0], d[1]) for d in KC.GEMM_LARGE}
    cls = {d: KC.real_gemm_operands(np.float64, "P0", d).classify(*d) for d in KC.GEMM_LARGE}
    tiled = [d for d in KC.GEMM_LARGE if not cls[d][0].startswith("skinny")]
    assert len(tiled) == 5
    for d in tiled:
        tiles_m, tiles_n, rem, groups, last = facts[d]
        assert groups >= 2 and 1 <= last < KC.G_GROUP_M and rem != 0 and 9 <= tiles_m, (d, facts[d])
        order = KC.gemm_remap_tiles(d[0], d[1])      # the remap is a bijection onto the tiles
        assert sorted(order) == [(i, j) for i in range(tiles_m) for j in range(tiles_n)]
    assert facts[(1100, 300, 96)] == (9, 3, 3, 2, 1) and facts[(2049, 129, 32)] == (17, 2, 2, 3, 1) and facts[(1025, 385, 512)] == (9, 4, 4, 2, 1)
    assert cls[(1100, 300, 96)][0] == cls[(2049, 129, 32)][0] == cls[(1025, 385, 512)][0] == "interior"
    assert cls[(1100, 300, 100)][0] == "full_vec_ktail"
    assert cls[(2100, 130, 64)] == ("interior", {"m_tail", "n_tail"})          # N = 130 > 2 K: not the skinny kernel
    # the skinny launches: 18 and 33 tile rows of 64, an N tail and an M tail
    assert cls[(1100, 129, 128)] == ("skinny2", {"m_tail", "n_tail"}) and -(-1100 // KC.S_BM) == 18
    assert cls[(2100, 127, 64)] == ("skinny1", {"m_tail", "n_tail"}) and -(-2100 // KC.S_BM) == 33


@pytest.mark.parametrize("dtype", KC.REAL_DTYPES, ids=["cf64", "cf32"])
def test_complex_gemm_grid_covers_every_dispatch_class(dtype):
    for pl in KC.complex_placements(dtype):
        n = _count(KC.complex_gemm_operands(dtype, pl), KC.complex_gemm_grid(pl))
        if pl == "Q0":
            for cls in ("interior", "interior_ktail", "edge"):
                assert n[cls] >= FLOOR, (pl, cls, n[cls])
            assert n["scalar"] == 0
            assert n["interior", False, False] >= 3            # M = N = 64: the tile-boundary grid, at K = 16, 32, 64
            for K in (15, 17, 33, 129):                        # a K tail inside an interior tile
                assert n["interior_ktail", "K", K] >= FLOOR
        else:
            assert n["scalar"] == len(KC.complex_gemm_grid(pl)) >= FLOOR
            assert n["scalar", False, False] >= 3 and n["scalar", True, True] >= FLOOR
