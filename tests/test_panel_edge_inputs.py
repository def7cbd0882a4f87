"""Host test of the adversarial pivot-search inputs (tests/helpers.py, tests/panel_edge_cases.py).  Nothing here runs the library:
it proves that the fixtures tests/test_gpu_panel_edges.py feeds the kernels are sound -- the reference agrees with itself across
precisions and with LAPACK where LAPACK's rule is the reference's -- and that they can see the defects they target: a numpy
restatement of the unblocked leaf with a switchable defect gives another ipiv / info / factors on at least one family per defect."""
import numpy as np
import pytest
import scipy.linalg as sla

import oracle as O
import panel_edge_cases as C
from helpers import nopivot_lu_numpy, nopivot_zero_top


def lapack_getrf(A):
    f = sla.lapack.dgetrf if A.dtype == np.float64 else sla.lapack.sgetrf
    lu, piv, info = f(np.asfortranarray(A))
    return lu, piv.astype(np.int64) + 1, int(info)


def _id(case):
    fam, rows, w, dt = case[:4]
    return f"{fam}-{rows}x{w}-{np.dtype(dt).name}"


LEAF = C.leaf_cases()
WHOLE = [(fam, m, n, dt) for (fam, m, n) in C.WHOLE for dt in C.DTYPES]


# ---- the reference stays inside its own bars ---------------------------------------------------------------------------------
def _check_exact_family(ref, shape_key):
    fam, m, n = shape_key
    A64, F64, ip64, info64 = ref(fam, m, n, np.float64)
    A32, F32, ip32, info32 = ref(fam, m, n, np.float32)
    assert np.array_equal(A32.astype(np.float64), A64)
    assert info32 == info64 and np.array_equal(ip32, ip64)
    assert np.array_equal(F32.astype(np.float64), F64), "class_ties arithmetic must be exact in both precisions"
    for A, F, ip, info in ((A64, F64, ip64, info64), (A32, F32, ip32, info32)):
        lu, lpiv, linfo = lapack_getrf(A)
        assert linfo == info and np.array_equal(lpiv, ip)
        assert np.array_equal(lu, F)
    return ip64, info64


@pytest.mark.parametrize("case", [c for c in LEAF if c[0] in C.EXACT and c[3] == np.float64], ids=_id)
def test_class_ties_leaf_reference_is_exact(case):
    fam, rows, w, _ = case
    ip, info = _check_exact_family(C.leaf_reference, (fam, rows, w))
    if fam == "ties_singular":
        assert info == min(C.empty_classes(w)) + 1
    else:
        assert info == 0
    # the family does what it is for: most pivots are interchanges, and the tied maxima of a column sit in more than one block of 512 rows
    assert np.count_nonzero(ip != np.arange(1, w + 1)) >= (3 * w) // 4
    if rows >= 1300 and w == 64:
        A = C.leaf_reference(fam, rows, w, np.float64)[0]
        spans = 0
        for k in range(w - 1):
            col = np.abs(A[:, k])
            if col.max() > 0 and len(set(np.flatnonzero(col == col.max()) // 512)) >= 2:
                spans += 1
        assert spans >= w // 2


@pytest.mark.parametrize("case", [c for c in WHOLE if c[0] in ("ties", "ties_singular") and c[3] == np.float64], ids=_id)
def test_class_ties_whole_reference_is_exact(case):
    fam, m, n, _ = case
    ip, info = _check_exact_family(C.whole_reference, (fam, m, n))
    assert info == (min(C.WHOLE_EMPTY) + 1 if fam == "ties_singular" else 0)
    assert np.count_nonzero(ip != np.arange(1, min(m, n) + 1)) >= (3 * min(m, n)) // 4


def test_class_ties_engine_size_is_exact_for_lapack():
    # the engine case of the GPU file, (6144, 6144) with two empty classes, has LAPACK as its reference: the same bits from dgetrf and
    # sgetrf (exact arithmetic, so no summation order can show), info at the first empty class
    from helpers import class_ties
    n = 6144
    A = class_ties(n, n, np.float64, 8000 + 2 * n, empty=(3000, 5000))
    lu64, p64, i64 = lapack_getrf(A)
    lu32, p32, i32 = lapack_getrf(A.astype(np.float32))
    assert i64 == i32 == 3001 and np.array_equal(p64, p32) and np.array_equal(lu32.astype(np.float64), lu64)


@pytest.mark.parametrize("case", [c for c in LEAF if c[0] in C.LAPACK_PIVOTS], ids=_id)
def test_leaf_reference_pivots_equal_lapack(case):
    fam, rows, w, dt = case
    A, F, ip, info = C.leaf_reference(fam, rows, w, dt)
    _, lpiv, linfo = lapack_getrf(A)
    assert linfo == info
    assert np.array_equal(lpiv, ip)
    if fam == "zero2":
        assert info == min(C.zero2_columns(w)) + 1
    elif fam == "zero0":
        assert info == 1
    else:
        assert info == 0


@pytest.mark.parametrize("case", [c for c in WHOLE if c[0] in ("near", "zero_col")], ids=_id)
def test_whole_reference_pivots_equal_lapack(case):
    fam, m, n, dt = case
    A, F, ip, info = C.whole_reference(fam, m, n, dt)
    _, lpiv, linfo = lapack_getrf(A)
    assert linfo == info == (701 if fam == "zero_col" else 0)
    assert np.array_equal(lpiv, ip)


def test_near_ties_are_decided_by_the_low_word():
    # Float64: the top two candidates of every column share the high 32 bits of |a| and differ in the low word
    for rows, w in ((1300, 64), (4600, 64), (1300, 40)):
        A = C.leaf_reference("near", rows, w, np.float64)[0]
        for k in range(w - 1):
            col = np.abs(A[:, k])
            top = np.sort(col[col > 0])[-2:]
            assert top.size == 2
            bits = top.view(np.uint64)
            assert bits[0] >> np.uint64(32) == bits[1] >> np.uint64(32)
            assert bits[0] != bits[1]


@pytest.mark.parametrize("case", [c for c in LEAF if c[0] in C.ORACLE_ONLY], ids=_id)
def test_special_value_leaf_cases_hit_what_they_aim_at(case):
    fam, rows, w, dt = case
    A, F, ip, info = C.leaf_reference(fam, rows, w, dt)
    if fam == "nan":
        # a NaN never wins: column 0's pivot is the finite maximum, and the NaN rows are not chosen at their columns
        (r1, c1), (r2, c2) = C.nan_entries(rows, w)
        assert info == 0 and ip[c1] - 1 == int(np.nanargmax(np.abs(A[:, c1]))) != r1
    elif fam == "nan_diag":
        # the NaN sits in position j when column j comes up and everything else there is zero: it is the pivot (NaN != 0: no info)
        j = C.nan_diag_column(w)
        assert info == 0 and ip[j] == j + 1 and np.isnan(F[j, j])
        assert np.all(ip[j:] == np.arange(j + 1, w + 1))
    else:
        # |-Inf| == |+Inf|: a tie between two blocks of rows
        assert info == 0 and np.isinf(F[5, 5]) and np.isnan(F).any()


# ---- sensitivity: the unblocked leaf restated in numpy, with a switchable defect ----------------------------------------------------
DEFECTS = ("highest-index tie", "high word only, then lowest index", "NaN wins", "zero pivot stops the updates", "info not recorded")


def glu(A, defect=None, pivot=True):
    """_generic_lufact! (src/lu.jl:290-338) on a copy of A: (factors, ipiv 1-based, info)."""
    F = np.array(A, order="F", copy=True)
    m, n = F.shape
    mn = min(m, n)
    ipiv = np.arange(1, mn + 1, dtype=np.int64)
    info = 0
    one = F.dtype.type(1)
    with np.errstate(all="ignore"):
        for k in range(mn):
            kp = k
            if pivot:
                v = np.abs(F[k:, k])
                if defect == "NaN wins":
                    key = np.where(np.isnan(v), np.inf, v)
                else:
                    key = np.where(v > 0, v, 0)           # zero and NaN -> 0: never preferred
                if defect == "high word only, then lowest index":
                    key = (key.astype(np.float64).view(np.uint64) >> np.uint64(32)).astype(np.int64)
                best = np.flatnonzero(key == key.max())
                kp = k + int(best[-1] if defect == "highest-index tie" else best[0])
                ipiv[k] = kp + 1
            if F[kp, k] != 0:
                if kp != k:
                    F[[k, kp], :] = F[[kp, k], :]
                F[k + 1:, k] *= one / F[k, k]
            else:
                if info == 0 and defect != "info not recorded":
                    info = k + 1
                if defect == "zero pivot stops the updates":
                    continue
            if k + 1 < n:
                F[k + 1:, k + 1:] -= np.outer(F[k + 1:, k], F[k, k + 1:])
    return F, ipiv, info


def _same(a, b):
    return a[2] == b[2] and np.array_equal(a[1], b[1]) and np.array_equal(a[0], b[0], equal_nan=True)


SENS_ROWS, SENS_W = 1300, 64


@pytest.mark.parametrize("dtype", C.DTYPES, ids=lambda d: np.dtype(d).name)
def test_numpy_leaf_without_defect_reproduces_the_oracle(dtype):
    for fam in C.FAMILIES:
        A, F, ip, info = C.leaf_reference(fam, SENS_ROWS, SENS_W, dtype)
        G, gp, ginfo = glu(A)
        assert ginfo == info and np.array_equal(gp, ip), fam
        ok = np.isfinite(F)
        assert np.array_equal(np.isnan(G), np.isnan(F)) and np.array_equal(G[~ok & ~np.isnan(F)], F[~ok & ~np.isnan(F)]), fam
        assert np.max(np.abs(G[ok] - F[ok])) <= 200 * np.finfo(dtype).eps * max(1.0, float(np.max(np.abs(F[ok])))), fam
        if fam in C.EXACT:
            assert np.array_equal(G, F)


@pytest.mark.parametrize("defect", DEFECTS)
def test_every_defect_is_visible_in_some_family(defect):
    seen = []
    for dtype in C.DTYPES:
        for fam in C.FAMILIES:
            A = C.leaf_reference(fam, SENS_ROWS, SENS_W, dtype)[0]
            if not _same(glu(A), glu(A, defect)):
                seen.append((fam, np.dtype(dtype).name))
        # the NoPivot zero-pivot block (what the substitution kernel is checked with)
        Z = nopivot_zero_top(SENS_ROWS, SENS_W, dtype, 77, 37)
        if not _same(glu(Z, pivot=False), glu(Z, defect, pivot=False)):
            seen.append(("nopivot_zero_top", np.dtype(dtype).name))
    print(defect, "->", seen)
    assert seen, f"no family notices '{defect}'"
    # the families built for a defect are among those that see it
    want = {"highest-index tie": "ties", "high word only, then lowest index": "near", "NaN wins": "nan",
            "zero pivot stops the updates": "nopivot_zero_top", "info not recorded": "zero2"}[defect]
    assert (want, "float64") in seen


def test_nopivot_zero_top_reference():
    for w, j in ((64, 0), (64, 37), (64, 63), (40, 39)):
        Z = nopivot_zero_top(300, w, np.float64, 5, j)
        F, info = nopivot_lu_numpy(Z)
        G, _, ginfo = glu(Z, pivot=False)
        assert info == ginfo == j + 1
        assert np.allclose(F, G, rtol=0, atol=1e-12 * np.max(np.abs(F)))
        # column j is left unscaled below the top block
        assert np.array_equal(F[w:, j] if j == 0 else F[w:, j] != 0, Z[w:, j] if j == 0 else np.ones(300 - w, bool))
