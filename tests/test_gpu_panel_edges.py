"""-m gpu: the pivot search of the leaf kernels on ties, near-ties, zero columns, NaN and Inf -- where several workgroups have to agree on a
winner -- and the NoPivot leaf with and without a zero pivot, through the C building block rflu_panel_rm_*_dev; then whole factorizations
of 1100 - 1500 columns on the recursive and stream schedules, and two singular matrices through the engine.

Reference: the CPU oracle's restatement of _generic_lufact! (src/lu.jl:290-338; O.lu for blocks wider than 64) on the block
A[r0:, c0:c0+w].  tests/test_panel_edge_inputs.py proves on the host that these inputs are sound and that they tell a wrong pivot
rule from the right one.

Which kernel serves which call (csrc/panel.hip: launch_panel, csrc/panel_local.hip: launch_panel_local; rows = m - r0, pivot = 1):

| kernel                                                   | how to reach it                                            | shapes (m, r0, c0, w)                         |
|----------------------------------------------------------|------------------------------------------------------------|-----------------------------------------------|
| panel_single (one workgroup, LDS only)                   | rows <= 512, default                                       | (300,0,0,64), (512,0,0,64), (70,0,5,7)        |
| panel_pivot_kernel, G == 1 branch                        | RFLU_PANEL_SINGLE=0, rows <= 256                           | (200,0,0,64)                                  |
| XCD-local panel_pivot_local_kernel, 64-row workgroups    | RFLU_PANEL_SINGLE=0, rows 257..512, w = 64 (tiny_local)    | (448,0,0,64)                                  |
| XCD-local panel_pivot_local_kernel (64-row workgroups up | default, w = 64, 513..4096 rows (Float32: ..8192)          | (1300,0,0,64), (1428,128,3,64), (4096,0,0,64) |
| to 1024 rows, 128 up to 2048, 256 above)                 |                                                            |                                               |
| any-placement panel_pivot_local_kernel (64-row           | RFLU_PANEL_LOCAL_ROWS=0; by default above 4096 rows        | (1300,0,0,64), (4600,0,0,64)                  |
| workgroups up to 2048 rows, 128 up to 4096, 256 above)   | (Float64) up to 64 workgroups of 512 rows                  |                                               |
| two-trip panel_pivot_kernel, G > 1                       | w < 64, or RFLU_PANEL_LOCAL=0                              | (1300,0,0,40), (1300,64,64,40), (1300,0,0,64) |
| the same, second polling round (G > 64)                  | rows > 32768                                               | (33300,0,0,64), Float64 only                  |
| Toledo recursion inside a slab (w > 64): leaves as above | -                                                          | (1300,0,0,256), (1364,64,0,192)               |
|   + laswp, inverse of the diagonal block, TRSM, GEMM     |                                                            |                                               |

pivot = 0: panel_nopivot_top_kernel (one workgroup), panel_nopivot_inv_kernel, then panel_nopivot_rows_mfma_kernel (info == 0) or
panel_nopivot_rows_kernel (the substitution that takes over after a zero pivot) -- both are launched, one returns at once.

Inputs per shape (tests/panel_edge_cases.py): class_ties, class_ties with two empty classes, near_ties, zero columns {17, 40} ({17, 39} in a
40-wide block, which has no column 40; {3, 6} for w = 7), zero column 0, NaN at (a row of the last workgroup, 0) and (a row of the second
block of 512, 10), a zero column with a NaN in its diagonal position, -Inf and +Inf in column 5 in two blocks of 512 rows with the -Inf at
the lower position (blocks of at most 512 rows: lower and upper half).

Bars: ipiv and info bit-exact (info = r0 + the block-relative value); factors bit for bit on the class_ties inputs (exact arithmetic),
otherwise within the leaf bar 200 eps max(1, max|F|) over the finite entries with the same NaN mask and the same infinities; nothing
outside [r0:, c0:c0+w] changes.  A returned RFLU_ERR_TIMEOUT raises and fails the test: run this file with -x."""
import ctypes

import numpy as np
import pytest
import scipy.linalg as sla
import torch

import oracle as O
import panel_edge_cases as C
import recursivefactorization.jl_amd as rf
from gpu_util import handle, ptr, sfx, to_dev_cm, to_dev_rm
from helpers import class_ties, nopivot_lu_numpy, nopivot_zero_top, rand_matrix
from test_gpu_lu import check_against_oracle, tol_E

pytestmark = pytest.mark.gpu


def _dn(dt):
    return np.dtype(dt).name


# ---- one leaf call -----------------------------------------------------------------------------------------------------------------------
def run_panel(block, geom, dtype, pivot=1):
    """The block embedded at [r0:, c0:c0+w] of an m x ld random background -> (background, result, ipiv, info)."""
    m, r0, c0, w = geom
    ld = c0 + w + 9
    A = np.array(O.np_uniform(m, ld, 1234 + m, dtype), order="C")
    A[r0:, c0:c0 + w] = block
    dA = to_dev_rm(A)
    dP = torch.full((m,), -7, dtype=torch.int64, device="cuda:0")
    info = ctypes.c_int64(-1)
    handle().call(f"rflu_panel_rm_{sfx(dtype)}_dev", m, r0, c0, w, ptr(dA), ld, ptr(dP), pivot, ctypes.byref(info))
    torch.cuda.synchronize()
    return A, dA.cpu().numpy(), dP.cpu().numpy(), int(info.value)


def assert_outside_untouched(A, got, geom):
    m, r0, c0, w = geom
    mask = np.ones_like(A, dtype=bool)
    mask[r0:, c0:c0 + w] = False
    assert np.array_equal(got[mask], A[mask], equal_nan=True)


def assert_factors(got, F, dtype, exact, bar=None):
    if exact:
        print("factors bitwise equal:", np.array_equal(got, F))
        assert np.array_equal(got, F)
        return
    nan = np.isnan(F)
    inf = np.isinf(F)
    assert np.array_equal(np.isnan(got), nan), "NaN masks differ"
    assert np.array_equal(got[inf], F[inf]), "infinities differ"
    fin = ~nan & ~inf
    scale = max(1.0, float(np.max(np.abs(F[fin]))))
    bar = 200 * np.finfo(dtype).eps * scale if bar is None else bar * scale
    err = float(np.max(np.abs(got[fin].astype(np.float64) - F[fin].astype(np.float64))))
    print(f"max factor error {err:.3e}, bar {bar:.3e}")
    assert err < bar


LEAF_PARAMS = [pytest.param(env, geom, dt, fam, id=f"{rid}-{'x'.join(map(str, geom))}-{_dn(dt)}-{fam}")
               for rid, env, shapes, dtypes in C.LEAF_ROUTES for geom in shapes for dt in dtypes for fam in C.FAMILIES]


@pytest.mark.parametrize("env,geom,dtype,fam", LEAF_PARAMS)
def test_leaf_pivot_search_on_adversarial_inputs(env, geom, dtype, fam, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m, r0, c0, w = geom
    block, F, ipiv, oinfo = C.leaf_reference(fam, m - r0, w, dtype)
    A, got, gp, info = run_panel(block, geom, dtype)
    print(f"info {info} (oracle {oinfo}, r0 {r0}); pivots off the diagonal: {int(np.count_nonzero(ipiv != np.arange(1, w + 1)))} of {w}")
    assert np.array_equal(gp[r0:r0 + w], ipiv + r0), f"first difference at step {int(np.argmax(gp[r0:r0 + w] != ipiv + r0))}"
    assert info == (r0 + oinfo if oinfo else 0)
    assert_factors(got[r0:, c0:c0 + w], F, dtype, fam in C.EXACT)
    assert_outside_untouched(A, got, geom)


@pytest.mark.parametrize("dtype", C.DTYPES, ids=_dn)
@pytest.mark.parametrize("fam", C.EXACT)
def test_xcd_local_and_any_placement_leaves_are_bit_identical_on_ties(fam, dtype, monkeypatch):
    geom = (1300, 0, 0, 64)
    block = C.leaf_reference(fam, 1300, 64, dtype)[0]
    _, got_l, gp_l, info_l = run_panel(block, geom, dtype)
    monkeypatch.setenv("RFLU_PANEL_LOCAL_ROWS", "0")
    _, got_a, gp_a, info_a = run_panel(block, geom, dtype)
    assert info_l == info_a and np.array_equal(gp_l, gp_a) and np.array_equal(got_l, got_a)


# ---- NoPivot -----------------------------------------------------------------------------------------------------------------------------
NOPIVOT_GEOMS = [(64, 0, 0, 64), (300, 0, 0, 64), (1300, 64, 64, 40), (5000, 128, 3, 64)]


def nopivot_bar(w, dtype):
    # the project's NoPivot bar, 10 sqrt(E) with E = 20 s eps (test/runtests.jl:19-20), on a w-column block
    return 10 * np.sqrt(20 * w * np.finfo(dtype).eps)


def check_nopivot(block, geom, dtype, want_info):
    m, r0, c0, w = geom
    F, ninfo = nopivot_lu_numpy(block)
    assert ninfo == want_info
    A, got, gp, info = run_panel(block, geom, dtype, pivot=0)
    assert info == (r0 + want_info if want_info else 0)
    assert np.array_equal(gp[r0:r0 + w], np.arange(r0 + 1, r0 + w + 1))
    assert_factors(got[r0:, c0:c0 + w], F, dtype, False, bar=nopivot_bar(w, dtype))
    assert_outside_untouched(A, got, geom)
    return got[r0:, c0:c0 + w]


def nopivot_regular(rows, w, dtype):
    B = rand_matrix(rows, w, 9100 + rows + w, dtype)
    B[:w] += dtype(10) * np.eye(w, dtype=dtype)
    return B


@pytest.mark.parametrize("dtype", C.DTYPES, ids=_dn)
@pytest.mark.parametrize("geom", NOPIVOT_GEOMS, ids=lambda g: "x".join(map(str, g)))
def test_nopivot_leaf_regular_and_zero_pivot(geom, dtype):
    m, r0, c0, w = geom
    rows = m - r0
    check_nopivot(nopivot_regular(rows, w, dtype), geom, dtype, 0)
    for j in (0, 37, w - 1):
        Z = nopivot_zero_top(rows, w, dtype, 9200 + rows + j, j)
        got = check_nopivot(Z, geom, dtype, j + 1)
        if j == 0:   # column 0 below the top block is left as it came: unscaled, and no elimination in front of it
            assert np.array_equal(got[w:, 0], Z[w:, 0])
    # info is cleared by the entry: a regular call right after a singular one gives the regular result
    check_nopivot(nopivot_regular(rows, w, dtype), geom, dtype, 0)


# ---- whole factorizations ----------------------------------------------------------------------------------------------------------------
SCHEDULES = [("recursive", {}, -1, "hip-recursive"), ("default", {}, 0, "hip-lookahead"),
             ("lookahead-to-the-end", {"RFLU_LEAFWISE": "0"}, 0, "hip-lookahead"), ("block128", {}, 128, "hip-lookahead")]


def check_whole(fam, A, Fo, ipo, infoo, F):
    lu_host = F.factors.cpu().numpy() if hasattr(F.factors, "cpu") else np.asarray(F.factors)
    ip = np.asarray(F.ipiv.cpu().numpy() if hasattr(F.ipiv, "cpu") else F.ipiv)
    if fam == "nan":
        # check_against_oracle's bars with equal_nan: its residual and factor bounds over the entries that are not NaN
        assert F.info == infoo == 0
        assert np.array_equal(ip, ipo), "ipiv must be bit-exact"
        nan = np.isnan(Fo)
        assert np.array_equal(np.isnan(lu_host), nan)
        L, U = O.unpack_lu(np.where(nan, 0.0, lu_host).astype(np.float64))
        p = O.perm_from_ipiv(ip, A.shape[0])
        rows_ok = ~nan.any(axis=1)
        R = (L @ U - np.asarray(A, dtype=np.float64)[p, :])[rows_ok]
        assert np.max(np.abs(R)) < tol_E(A)
        scale = max(1.0, float(np.max(np.abs(Fo[~nan]))))
        assert np.max(np.abs(lu_host[~nan] - Fo[~nan])) < 50 * tol_E(A) * scale
        return
    check_against_oracle(A, F)   # ipiv, info bit-exact; residual and factors when info == 0
    if infoo != 0:               # singular: the factors are still held to the same factor bound
        scale = max(1.0, float(np.max(np.abs(Fo))))
        assert np.max(np.abs(lu_host - Fo)) < 50 * tol_E(A) * scale
    if fam in ("ties", "ties_singular"):
        print("factors bitwise equal to the oracle's:", np.array_equal(lu_host, Fo))


WHOLE_PARAMS = [pytest.param(fam, m, n, dt, sched, id=f"{fam}-{m}x{n}-{_dn(dt)}-{sched[0]}")
                for fam, m, n in C.WHOLE for dt in C.DTYPES for sched in SCHEDULES]


@pytest.mark.parametrize("fam,m,n,dtype,sched", WHOLE_PARAMS)
def test_whole_factorizations_on_adversarial_inputs(fam, m, n, dtype, sched, monkeypatch):
    _, env, bs, path = sched
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    A, Fo, ipo, infoo = C.whole_reference(fam, m, n, dtype)
    assert infoo == (701 if fam in ("ties_singular", "zero_col") else 0)
    F = rf.lu(np.array(A, order="F"), True, check=False, blocksize=bs)        # host entry
    assert rf.last_path() == path
    check_whole(fam, A, Fo, ipo, infoo, F)
    Fd = rf.lu_(to_dev_cm(A), None, True, check=False, blocksize=bs)           # column-major device entry
    assert rf.last_path() == path
    check_whole(fam, A, Fo, ipo, infoo, Fd)
    if infoo != 0:
        assert F.info == Fd.info == infoo
        with pytest.raises(rf.SingularException):
            rf.lu(np.array(A, order="F"), True, blocksize=bs)
        with pytest.raises(rf.SingularException):
            rf.ldiv_(F, np.ones(m, dtype=dtype))


# ---- the engine, at a geometry the suite already runs --------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", ["ties_singular", "zero_col"])
def test_engine_on_singular_inputs(fam, monkeypatch):
    """(6144, 6144, block width 256) under RFLU_ENGINE=1: ipiv and info equal LAPACK dgetrf's on the host copy; factors equal to the stream
    schedule's within 1e-10 max|LU|."""
    n = 6144
    if fam == "ties_singular":
        A = class_ties(n, n, np.float64, 8000 + 2 * n, empty=(3000, 5000))
    else:
        A = O.fill_uniform(n, n, 40 + 2 * n, np.float64)
        A[:, 3000] = 0
    _, lpiv, linfo = sla.lapack.dgetrf(A)
    assert linfo == 3001
    monkeypatch.setenv("RFLU_ENGINE", "1")
    F = rf.lu_(to_dev_cm(A), None, True, check=False, blocksize=256)
    assert rf.last_path() == "hip-engine"
    assert F.info == linfo
    assert np.array_equal(F.ipiv.cpu().numpy(), lpiv.astype(np.int64) + 1)
    monkeypatch.setenv("RFLU_ENGINE", "0")
    G = rf.lu_(to_dev_cm(A), None, True, check=False, blocksize=256)
    assert rf.last_path() == "hip-lookahead"
    assert G.info == linfo and torch.equal(F.ipiv, G.ipiv)
    scale = float(G.factors.abs().max())
    d = float((F.factors - G.factors).abs().max())
    print(f"engine vs streams: max difference {d:.3e}, scale {scale:.3e}")
    assert d <= 1e-10 * scale
