"""-m gpu: the C ABI building blocks (rflu_gemm_rm_{f64,f32,cf64,cf32}_dev, rflu_trsm_rm_*, rflu_laswp_rm_*) on the EXACT inputs of
tests/kernel_cases.py (proven on the host in tests/test_kernel_cases.py): every correct kernel returns the same values, whatever its tiling,
its summation order and its precision, so every case is held to value equality of the WHOLE output buffer -- the view and everything around
it -- with the float64 / int64 reference, and its input operands must come back bit for bit.  Values, not bits: a zero may carry either sign
(tests/test_gpu_complex.py explains why for the complex GEMM).

One test per (primitive, element type, placement); the grid is looped inside it on device buffers that are restored from pristine copies.
The reference of a GEMM is one float64 BLAS product per K over the largest window, uploaded once; the expected buffer of a case is put
together from it and the pristine C by copies alone (no arithmetic on the device).  For the interchanges the expected buffer is the
pristine one gathered by the row permutation of the sequential swaps (tests/test_kernel_cases.py: the same as swapping the rows of the array).
Every case of a grid is run and asserted; a test reports ALL its failing cases with their predicted dispatch class (kernel_cases.*_class:
a prediction for the reader, never an input to what is expected), and the first of them element by element.

Not covered here: rounding (the inputs cannot show it, see kernel_cases.py), the experiments-only variants RFLU_GEMM_CFIRST_BELOW,
RFLU_LASWP_LPR, RFLU_SKINNY_WIDE and RFLU_GEMM_FLAGS, and the two-region "first columns first" order of gemm_sub_kernel, which no C ABI entry
reaches.  The last part holds two calls on the same uniform random inputs to the same bits, one case per primitive and dispatch class.

Measured on an MI355X (unmodified library: every one of the 10576 exact cases equal, nothing skipped): this file together with
test_gpu_kernels.py, 150 tests, 5.0 s of wall time, most of it the start of the process; the slowest function here is
test_real_gemm_exact[f64-P0], 0.65 s for 1368 cases (it also pays the first launches of the process), then the other three full real
grids 0.24 .. 0.26 s, the full complex grids (832 cases) 0.12 .. 0.13 s, the interchanges (540 cases per test) 0.08 .. 0.11 s, the
TRSM (204 cases per test) at most 0.08 s.  Cases: real GEMM 2 x 1368 + 3 x 45 per precision, + 45 (P5, Float32), + 7 large ones each =
5801; complex GEMM 832 + 27 (cf64), 832 + 4 x 27 (cf32) = 1799; TRSM 4 x 204 = 816; interchanges 4 x 540 = 2160; 30 determinism cases.
Six deliberate errors in scratch builds each failed exactly the cases they should (DESIGN.md section 4.1 has the table).
"""
import collections
import ctypes

import numpy as np
import pytest
import torch

import kernel_cases as KC
from gpu_util import handle, sfx, tdtype

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
IDS = ["f64", "f32"]


def dev(a):
    t = torch.from_numpy(np.array(a)).to("cuda:0")
    assert t.data_ptr() % 16 == 0
    return t


def bits(t):
    return t.view(torch.int64 if t.element_size() == 8 else torch.int32)


def addr(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + off * t.element_size())


def explain(got, want, off, step):
    """Count and first place of the differences between two flat buffers; (row, column) relative to the view at `off` with `step` elements per row."""
    bad = np.flatnonzero(got != want)
    k = int(bad[0])
    r, c = divmod(k - off, step)
    return (f"{bad.size} of {want.size} elements of the buffer differ, the first at flat index {k} = (row {r}, column {c}) of the view: "
            f"got {got[k]!r}, expected {want[k]!r}")


def report(failures, total, what):
    """failures: (case, class, detail or None).  One assertion per test, after EVERY case has run."""
    if not failures:
        return
    by_class = collections.Counter(cls for _, cls, _ in failures)
    lines = [f"{what}: {len(failures)} of {total} cases differ from the exact reference; by predicted class: {dict(by_class)}"]
    lines += [f"  {case} class={cls}: {detail}" for case, cls, detail in failures if detail]
    names = "; ".join(f"{case} {cls}" for case, cls, _ in failures)
    lines.append("  all of them: " + (names if len(names) <= 4000 else names[:4000] + " ..."))
    pytest.fail("\n".join(lines), pytrace=False)


# ==================================================================================================================== GEMM
def run_gemm_grid(symbol, ops, grid):
    """Every case of `grid` on the operands `ops`; returns the failing ones for `report`."""
    h = handle()
    w = 2 if ops.cplx else 1
    A, B, C = ops.A, ops.B, ops.C
    dA, dB, dC0 = dev(A.buf), dev(B.buf), dev(C.buf)
    A0, B0 = dA.clone(), dB.clone()
    dC, exp = dC0.clone(), dC0.clone()
    window = lambda t: torch.as_strided(t, (ops.Mmax, w * ops.Nmax), (w * C.ld, 1), C.off)
    failures, full_K, full, checked_host = [], None, None, 0
    for M, N, K in sorted(grid, key=lambda c: c[2]):
        if K != full_K:
            full_host = ops.expected_full(K)
            full, full_K = dev(full_host), K
        dC.copy_(dC0)
        h.call(symbol, M, N, K, addr(dA, A.off), A.ld, addr(dB, B.off), B.ld, addr(dC, C.off), C.ld)
        exp.copy_(dC0)
        window(exp)[:M, :w * N] = window(full)[:M, :w * N]
        ok_c = torch.equal(dC, exp)
        ok_in = torch.equal(bits(dA), bits(A0)) and torch.equal(bits(dB), bits(B0))
        if checked_host < 2 or not ok_c:      # the expected buffer built on the device is the one the host builds
            want = ops.expected(M, N, K, full=full_host)
            assert np.array_equal(exp.cpu().numpy(), want), "the test's own expected buffer is wrong"
            checked_host += 1
        if not (ok_c and ok_in):
            cls = ops.classify(M, N, K)
            detail = None
            if len(failures) < 3:
                detail = explain(dC.cpu().numpy(), want, C.off, w * C.ld) if not ok_c else "an input operand (A or B buffer) was written"
            failures.append((f"M={M} N={N} K={K}" + "".join(f" {f}" for f in sorted(cls[1])), cls[0], detail))
            if not ok_in:
                dA.copy_(A0)
                dB.copy_(B0)
    return failures


REAL_CASES = [(d, p) for d in DTYPES for p in KC.real_placements(d)]


@pytest.mark.parametrize("dtype,placement", REAL_CASES, ids=[f"{sfx(d)}-{p}" for d, p in REAL_CASES])
def test_real_gemm_exact(dtype, placement):
    ops = KC.real_gemm_operands(dtype, placement)
    grid = KC.real_gemm_grid(placement)
    report(run_gemm_grid(f"rflu_gemm_rm_{sfx(dtype)}_dev", ops, grid), len(grid), f"real GEMM {sfx(dtype)} {placement}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_real_gemm_large_cases_exact(dtype):
    """More than one group of 8 tile rows with a partial last group, nwg % 8 != 0, skinny launches with 18 and 33 tile rows."""
    failures = []
    for dims in KC.GEMM_LARGE:
        ops = KC.real_gemm_operands(dtype, "P0", dims)
        for case, cls, detail in run_gemm_grid(f"rflu_gemm_rm_{sfx(dtype)}_dev", ops, [dims]):
            failures.append((f"{case} (tiles_m, tiles_n, nwg % 8, groups, last group) = {KC.gemm_remap_facts(dims[0], dims[1])}", cls, detail))
    report(failures, len(KC.GEMM_LARGE), f"real GEMM {sfx(dtype)} P0, large cases")


COMPLEX_CASES = [(d, p) for d in DTYPES for p in KC.complex_placements(d)]


@pytest.mark.parametrize("dtype,placement", COMPLEX_CASES, ids=[f"c{sfx(d)}-{p}" for d, p in COMPLEX_CASES])
def test_complex_gemm_exact(dtype, placement):
    ops = KC.complex_gemm_operands(dtype, placement)
    grid = KC.complex_gemm_grid(placement)
    report(run_gemm_grid(f"rflu_gemm_rm_c{sfx(dtype)}_dev", ops, grid), len(grid), f"complex GEMM c{sfx(dtype)} {placement}")


# ==================================================================================================================== TRSM
@pytest.mark.parametrize("kind", KC.TRSM_LDL)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_trsm_exact(dtype, kind):
    """B sits one row into its buffer: a row of sentinels in front of it and one behind, three sentinel columns behind every row."""
    h = handle()
    td = tdtype(dtype)
    failures, total = [], 0
    for n in KC.TRSM_N:
        Lbuf, ldl = KC.trsm_l_buffer(n, kind, dtype)
        _, x_true, B = KC.trsm_case(n)
        dL, dRhs, dX = dev(Lbuf), dev(B.astype(dtype)), dev(x_true.astype(dtype))
        L0 = dL.clone()
        for nrhs in KC.TRSM_NRHS:
            total += 1
            ldb = nrhs + KC.TRSM_PAD
            dB = torch.full((n + 2, ldb), KC.SENTINEL, dtype=td, device="cuda:0")
            exp = dB.clone()
            dB[1:n + 1, :nrhs] = dRhs[:, :nrhs]
            exp[1:n + 1, :nrhs] = dX[:, :nrhs]
            h.call(f"rflu_trsm_rm_{sfx(dtype)}_dev", n, nrhs, addr(dL), ldl, addr(dB, ldb), ldb)
            ok_b, ok_l = torch.equal(dB, exp), torch.equal(bits(dL), bits(L0))
            if not (ok_b and ok_l):
                detail = None
                if len(failures) < 3:
                    want = np.full((n + 2, ldb), KC.SENTINEL, dtype=dtype)
                    want[1:n + 1] = KC.trsm_b_buffer(n, nrhs, dtype, solved=True)
                    assert np.array_equal(exp.cpu().numpy(), want), "the test's own expected buffer is wrong"
                    detail = explain(dB.cpu().numpy().ravel(), want.ravel(), ldb, ldb) if not ok_b else "the L buffer was written"
                failures.append((f"n={n} nrhs={nrhs} ldl={ldl} ldb={ldb}", KC.trsm_class(n), detail))
                if not ok_l:
                    dL.copy_(L0)
    report(failures, total, f"TRSM {sfx(dtype)} ldl {kind}")


# ============================================================================================================ interchanges
@pytest.mark.parametrize("ld", KC.LASWP_LD)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_laswp_exact(dtype, ld):
    """The m x ld matrix sits one row into its buffer (a guard row of -1 in front and behind); ipiv entries outside [k0, k1) name moves too."""
    h = handle()
    m = KC.LASWP_M
    host = np.full((m + 2, ld), -1, dtype=dtype)
    host[1:m + 1] = KC.laswp_matrix(ld, dtype)
    A0 = dev(host)
    dA, exp = A0.clone(), A0.clone()
    columns = KC.laswp_columns(dtype)
    failures, total = [], 0
    for k0, k1 in KC.LASWP_RANGES:
        for pattern in KC.LASWP_PATTERNS:
            ipiv_host = KC.laswp_ipiv(pattern, k0, k1)
            ipiv, perm = dev(ipiv_host), dev(KC.laswp_perm(pattern, k0, k1))
            ipiv0 = ipiv.clone()
            for c0, ncols in columns:
                total += 1
                dA.copy_(A0)
                h.call(f"rflu_laswp_rm_{sfx(dtype)}_dev", addr(dA, ld), ld, m, c0, ncols, addr(ipiv), k0, k1)
                exp.copy_(A0)
                exp[1:m + 1, c0:c0 + ncols] = A0[1:m + 1, c0:c0 + ncols].index_select(0, perm)
                ok_a, ok_p = torch.equal(dA, exp), torch.equal(ipiv, ipiv0)
                if not (ok_a and ok_p):
                    detail = None
                    if len(failures) < 3:
                        want = host.copy()
                        want[1:m + 1] = KC.laswp_reference(host[1:m + 1], c0, ncols, ipiv_host, k0, k1)
                        assert np.array_equal(exp.cpu().numpy(), want), "the test's own expected buffer is wrong"
                        detail = explain(dA.cpu().numpy().ravel(), want.ravel(), ld, ld) if not ok_a else "ipiv was written"
                    moves = max(len(KC.laswp_chunk_moves(ipiv_host, c, k1)[0]) for c in range(k0 // KC.NB, (k1 + KC.NB - 1) // KC.NB))
                    failures.append((f"pattern={pattern} pivots=[{k0}, {k1}) columns=[{c0}, {c0 + ncols}) largest move list {moves}",
                                     KC.laswp_class(ld, ld, c0, ncols, dtype), detail))
                    if not ok_p:
                        ipiv.copy_(ipiv0)
    report(failures, total, f"interchanges {sfx(dtype)} ld={ld}")


def test_device_side_expected_buffers_match_the_host_reference_once():
    """The sequential swaps of the array itself, uploaded, against the gather the laswp test builds on the device (one case, Float32)."""
    ld, c0, ncols, k0, k1 = 1041, 17, 333, 64, 214
    A = KC.laswp_matrix(ld, np.float32)
    ref = KC.laswp_reference(A, c0, ncols, KC.laswp_ipiv("random", k0, k1), k0, k1)
    dA, perm = dev(A), dev(KC.laswp_perm("random", k0, k1))
    exp = dA.clone()
    exp[:, c0:c0 + ncols] = dA[:, c0:c0 + ncols].index_select(0, perm)
    assert np.array_equal(exp.cpu().numpy(), ref)


# ============================================================================================================= determinism
def twice(call, out):
    """Two calls on the same inputs: `out` (restored in between) must hold the same BITS."""
    start = out.clone()
    call()
    first = out.clone()
    out.copy_(start)
    call()
    assert bool(torch.isfinite(first).all()) and not torch.equal(first, start)
    assert torch.equal(bits(first), bits(out))


def uniform(rng, shape, dtype, off8):
    """Uniform(-1, 1) in a flat device buffer that starts 8 * off8 bytes before the data: (tensor, element offset of the data)."""
    off = off8 * 8 // np.dtype(dtype).itemsize
    buf = np.zeros(off + int(np.prod(shape)), dtype=dtype)
    buf[off:] = rng.uniform(-1, 1, int(np.prod(shape)))
    return dev(buf), off


REAL_DET = {"skinny1": (200, 100, 64), "skinny2": (200, 132, 128), "interior": (257, 260, 96), "full_vec_ktail": (257, 260, 100),
            "edge_vec": (100, 100, 52), "scalar": (130, 72, 36)}


@pytest.mark.parametrize("cls", list(REAL_DET))
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_real_gemm_two_calls_give_the_same_bits(dtype, cls):
    M, N, K = REAL_DET[cls]
    off8 = 1 if cls == "scalar" else 0
    rng = np.random.default_rng(M + N + K)
    (dA, oa), (dB, ob), (dC, oc) = (uniform(rng, s, dtype, off8) for s in ((M, K), (K, N), (M, N)))
    assert KC.real_gemm_class(M, N, K, oa, ob, K, N, dtype)[0] == cls
    h = handle()
    twice(lambda: h.call(f"rflu_gemm_rm_{sfx(dtype)}_dev", M, N, K, addr(dA, oa), K, addr(dB, ob), N, addr(dC, oc), N), dC)


COMPLEX_DET = {"interior": (129, 132, 64), "interior_ktail": (129, 132, 68), "edge": (60, 36, 20), "scalar": (129, 132, 68)}


@pytest.mark.parametrize("cls", list(COMPLEX_DET))
@pytest.mark.parametrize("dtype", DTYPES, ids=["cf64", "cf32"])
def test_complex_gemm_two_calls_give_the_same_bits(dtype, cls):
    M, N, K = COMPLEX_DET[cls]
    off8 = 1 if cls == "scalar" else 0
    rng = np.random.default_rng(M + N + K)
    (dA, oa), (dB, ob), (dC, oc) = (uniform(rng, (r, 2 * c), dtype, off8) for r, c in ((M, K), (K, N), (M, N)))
    assert KC.complex_gemm_class(M, N, K, oa, ob, oc, K, N, dtype)[0] == cls
    h = handle()
    twice(lambda: h.call(f"rflu_gemm_rm_c{sfx(dtype)}_dev", M, N, K, addr(dA, oa), K, addr(dB, ob), N, addr(dC, oc), N), dC)


@pytest.mark.parametrize("n", [150, 256, 600], ids=["fused", "fused_slot_reuse", "recursive"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_trsm_two_calls_give_the_same_bits(dtype, n, request):
    assert KC.trsm_class(n) == request.node.callspec.id.split("-")[-1]
    nrhs = 100
    rng = np.random.default_rng(n)
    dL = dev((rng.uniform(-1, 1, (n, n)) * 0.5).astype(dtype))
    dB = dev(rng.uniform(-1, 1, (n, nrhs)).astype(dtype))
    h = handle()
    twice(lambda: h.call(f"rflu_trsm_rm_{sfx(dtype)}_dev", n, nrhs, addr(dL), n, addr(dB), nrhs), dB)


@pytest.mark.parametrize("cls,c0,ncols", [("vec", 16, 64), ("scalar", 17, 33)], ids=["vec", "scalar"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_laswp_two_calls_give_the_same_bits(dtype, cls, c0, ncols):
    m, ld, k0, k1 = 300, 128, 64, 214
    assert KC.laswp_class(0, ld, c0, ncols, dtype) == cls
    dA = dev(np.random.default_rng(9).uniform(-1, 1, (m, ld)).astype(dtype))
    ipiv = dev(KC.laswp_ipiv("random", k0, k1, m))
    h = handle()
    twice(lambda: h.call(f"rflu_laswp_rm_{sfx(dtype)}_dev", addr(dA), ld, m, c0, ncols, addr(ipiv), k0, k1), dA)
