"""The adversarial cases of the pivot search, shared by tests/test_panel_edge_inputs.py (host: the fixtures are sound and can see the
defects they target) and tests/test_gpu_panel_edges.py (the leaf kernels and whole factorizations against the oracle).

A leaf case is (family, rows, w, dtype): the rows x w block a leaf kernel factors (rows = m - r0).  References are computed once per
process and shared; nobody writes to them."""
import functools

import numpy as np

import oracle as O
from helpers import class_ties, near_ties, rand_matrix, with_inf, with_nan, zero_columns

DTYPES = (np.float64, np.float32)

# ---- which kernel serves which call (csrc/panel.hip: launch_panel, rows = m - r0): (id, environment, [(m, r0, c0, w)], dtypes)
LEAF_ROUTES = [
    ("single", {}, [(300, 0, 0, 64), (512, 0, 0, 64), (70, 0, 5, 7)], DTYPES),
    ("twotrip-g1", {"RFLU_PANEL_SINGLE": "0"}, [(200, 0, 0, 64)], DTYPES),
    ("tiny-local", {"RFLU_PANEL_SINGLE": "0"}, [(448, 0, 0, 64)], DTYPES),
    ("xcd-local", {}, [(1300, 0, 0, 64), (1428, 128, 3, 64), (4096, 0, 0, 64)], DTYPES),
    ("any-placement", {"RFLU_PANEL_LOCAL_ROWS": "0"}, [(1300, 0, 0, 64), (4600, 0, 0, 64)], DTYPES),
    ("any-placement-default", {}, [(4600, 0, 0, 64)], (np.float64,)),
    ("twotrip", {}, [(1300, 0, 0, 40), (1300, 64, 64, 40)], DTYPES),
    ("twotrip-w64", {"RFLU_PANEL_LOCAL": "0"}, [(1300, 0, 0, 64)], DTYPES),
    ("twotrip-two-rounds", {}, [(33300, 0, 0, 64)], (np.float64,)),
    ("slab-recursion", {}, [(1300, 0, 0, 256), (1364, 64, 0, 192)], DTYPES),
]

FAMILIES = ("ties", "ties_singular", "near", "zero2", "zero0", "nan", "nan_diag", "inf")
EXACT = ("ties", "ties_singular")           # every operation exact: factors compared bit for bit
LAPACK_PIVOTS = ("near", "zero2", "zero0")  # finite, tie-free up to the planted structure: ipiv / info equal LAPACK's
ORACLE_ONLY = ("nan", "nan_diag", "inf")    # optimised i?amax routines do not promise the reference's NaN rule


def leaf_cases():
    """Every (family, rows, w, dtype) the GPU file runs through a leaf kernel."""
    seen = []
    for _, _, shapes, dtypes in LEAF_ROUTES:
        for (m, r0, _, w) in shapes:
            for dt in dtypes:
                for fam in FAMILIES:
                    key = (fam, m - r0, w, dt)
                    if key not in seen:
                        seen.append(key)
    return seen


def empty_classes(w):
    return (w // 4, (5 * w) // 8)


def zero2_columns(w):
    # {17, 40}; a 40-wide block has no column 40: its last column instead; {3, 6} for w = 7
    return (3, 6) if w == 7 else (17, 39) if w == 40 else (17, 40)


def nan_entries(rows, w):
    """(a row of the last workgroup, column 0) and (a row of the second block of 512 -- of the upper half in a short block --, column 10)."""
    second = 512 + 77 if rows > 600 else rows // 2 + 1
    return [(rows - 3, 0), (second, min(10, w - 2))]


def nan_diag_column(w):
    return 4 if w == 7 else 12


def inf_entries(rows):
    """-Inf at the lower position, +Inf in another block of 512 rows (the upper half of a short block), both in column 5."""
    return [(100 if rows > 600 else 9, 5, -1), (512 + 200 if rows > 800 else rows // 2 + 5, 5, +1)]


# ---- seeds.  The random-based cases take 7000 + rows + w unless listed here: the first seed from there on with which the oracle's
# ipiv / info equal LAPACK's (another summation order: no near-tie in the random background decides anything) and, for nan_diag,
# with which the row that carries the NaN is still in its diagonal position when its column comes up.
SEED_TABLE = {
}


def seed_for(fam, rows, w, dtype):
    return SEED_TABLE.get((fam, rows, w, np.dtype(dtype).name), 7000 + rows + w)


def build_block(fam, rows, w, dtype, seed=None):
    seed = seed_for(fam, rows, w, dtype) if seed is None else seed
    if fam == "ties":
        return class_ties(rows, w, dtype, seed)
    if fam == "ties_singular":
        return class_ties(rows, w, dtype, seed, empty=empty_classes(w))
    if fam == "near":
        return near_ties(rows, w, dtype, seed)
    R = rand_matrix(rows, w, seed, dtype)
    if fam == "zero2":
        return zero_columns(R, zero2_columns(w))
    if fam == "zero0":
        return zero_columns(R, (0,))
    if fam == "nan":
        return with_nan(R, nan_entries(rows, w))
    if fam == "nan_diag":
        j = nan_diag_column(w)
        return with_nan(zero_columns(R, (j,)), [(j, j)])
    if fam == "inf":
        return with_inf(R, inf_entries(rows))
    raise KeyError(fam)


def oracle_block(A):
    """The reference on a block: the unblocked leaf for w <= 64, the recursion above (what a slab's panel entry runs)."""
    return O.generic_lufact(A) if A.shape[1] <= 64 else O.lu(A)


@functools.lru_cache(maxsize=None)
def leaf_reference(fam, rows, w, dtype):
    """(block, factors, ipiv, info) of a leaf case; read-only."""
    A = build_block(fam, rows, w, dtype)
    F, ipiv, info = oracle_block(A)
    for x in (A, F, ipiv):
        x.setflags(write=False)
    return A, F, ipiv, info


# ---- whole factorizations (the smallest sizes that leave the one-workgroup leaf behind): (id, m, n)
WHOLE = [("ties", 1500, 1100), ("near", 1500, 1100), ("ties_singular", 1300, 1300), ("zero_col", 1300, 1300), ("nan", 1300, 1300)]
WHOLE_EMPTY = (700, 900)
WHOLE_SEED_TABLE = {
}


def whole_seed(fam, m, n, dtype):
    return WHOLE_SEED_TABLE.get((fam, m, n, np.dtype(dtype).name), 8000 + m + n)


def build_whole(fam, m, n, dtype, seed=None):
    seed = whole_seed(fam, m, n, dtype) if seed is None else seed
    if fam == "ties":
        return class_ties(m, n, dtype, seed)
    if fam == "near":
        return near_ties(m, n, dtype, seed)
    if fam == "ties_singular":
        return class_ties(m, n, dtype, seed, empty=WHOLE_EMPTY)
    R = rand_matrix(m, n, seed, dtype)
    if fam == "zero_col":
        return zero_columns(R, (700,))
    if fam == "nan":
        return with_nan(R, [(900, 0)])
    raise KeyError(fam)


@functools.lru_cache(maxsize=None)
def whole_reference(fam, m, n, dtype):
    A = build_whole(fam, m, n, dtype)
    F, ipiv, info = O.lu(A)
    for x in (A, F, ipiv):
        x.setflags(write=False)
    return A, F, ipiv, info
