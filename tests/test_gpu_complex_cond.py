"""-m gpu: complex operator norms and the complex condition estimate (rflu_lange_c*, rflu_gecon_c*, rflu_gecon_batched_c*;
csrc/condest.hip, cgecon_batched_kernel of csrc/batched_complex.hip, cgecon_dev of csrc/driver.cpp) and the Python functions
above them.  Outputs are written into NaN-filled words.

  * norms: matrices whose entries lie on the axes with small integer parts equal the integer reference by `==` (both norms, both
    layouts, padded lda full of NaN, pointers offset by one real and one complex element), random ones stay within (len + 2) eps64 of
    an fsum reference (one rounding per addition at most, two for the modulus); NaN in either part, (Inf, NaN), Inf alone, empty
    shapes; the batched entry gives the single entry's bits;
  * rcond of exact factors by `==` with the NumPy restatement (tests/complex_cond_cases.py; tests/test_complex_cond_cases.py proves the
    yardsticks): the real exact factors embedded as complex, and the axis-scaled family that notices M^T where M^H belongs -- single
    calls, and as members of batches between random members;
  * rcond at rounding level on the device's own lu_complex_ factors: est / ||(L U)^-1|| in [1/3, 1 + twice the restatement's own gap +
    4 n eps], and on inputs with a decision margin the device's estimate against the restatement's within 8 x (the restatement's gap
    to itself one precision up) + n eps;
  * every line of the special-value order, determinism, and a solve, an inverse and a factorization after gecon on the same handle.
Measured ratios are printed (pytest -s)."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import complex_cond_cases as C
import cond_cases as R
import recursivefactorization.jl_amd as rf
from gpu_util import handle, ptr
from recursivefactorization.jl_amd import _ffi

pytestmark = pytest.mark.gpu

DTYPES = [np.complex128, np.complex64]
IDS = ["cf64", "cf32"]
NORMS = [C.NORM_ONE, C.NORM_INF]
EPS64 = float(np.finfo(np.float64).eps)
NPORD = {C.NORM_ONE: 1, C.NORM_INF: np.inf}
PNORM = {C.NORM_ONE: 1, C.NORM_INF: math.inf}


def sfx(dtype):
    return "cf64" if np.dtype(dtype) == np.complex128 else "cf32"


def eps_of(dtype):
    return float(np.finfo(C.real_of(dtype)).eps)


def dev_cm(A, dtype):
    """numpy -> column-major complex device view (stride(0) == 1)."""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(A, dtype=dtype).T)).to("cuda:0").T


def dev_rm(A, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(A, dtype=dtype))).to("cuda:0")


def clange(t, norm, m, n, ld, row_major, dtype, h=None):
    out = ctypes.c_double(math.nan)
    (h or handle()).call(f"rflu_lange_{sfx(dtype)}_dev", norm, m, n, ptr(t), ld, row_major, ctypes.byref(out))
    return out.value


def clange_batched(t, norm, batch, m, n, ld, stride, row_major, dtype):
    out = torch.full((batch,), math.nan, dtype=torch.float64, device="cuda:0")
    handle().call(f"rflu_lange_batched_{sfx(dtype)}_dev", norm, batch, m, n, ptr(t), ld, stride, row_major, ptr(out))
    return out.cpu().numpy()


def cgecon(F, norm, anorm, dtype, kind="cm", h=None):
    """F: the packed factors as a numpy matrix; kind: cm (device) or host."""
    n = F.shape[0]
    out = ctypes.c_double(math.nan)
    h = h or handle()
    if kind == "host":
        Fh = np.asfortranarray(np.asarray(F, dtype=dtype))
        h.call(f"rflu_gecon_{sfx(dtype)}", norm, n, ctypes.c_void_p(Fh.ctypes.data), max(n, 1), float(anorm), ctypes.byref(out))
    else:
        t = dev_cm(F, dtype)
        h.call(f"rflu_gecon_{sfx(dtype)}_dev", norm, n, ptr(t), max(n, 1), float(anorm), ctypes.byref(out))
    return out.value


def cgecon_batched(Fs, norm, anorms, dtype, row_major):
    """Fs: list of packed factor matrices of one size."""
    batch, n = len(Fs), Fs[0].shape[0]
    stack = np.stack([np.asarray(F, dtype=dtype) if row_major else np.asarray(F, dtype=dtype).T for F in Fs])
    t = torch.from_numpy(np.ascontiguousarray(stack)).to("cuda:0")
    an = torch.tensor(list(anorms), dtype=torch.float64, device="cuda:0")
    out = torch.full((batch,), math.nan, dtype=torch.float64, device="cuda:0")
    handle().call(f"rflu_gecon_batched_{sfx(dtype)}_dev", norm, batch, n, ptr(t), max(n, 1), n * n, int(row_major), ptr(an), ptr(out))
    return out.cpu().numpy()


def same(a, b):
    return a == b or (a != a and b != b)


# ---- 1. norms ----------------------------------------------------------------------------------------------------------------------
NORM_SHAPES = [(1, 1), (3, 5), (255, 257), (1023, 3), (1025, 1025), (2112, 70)]


def padded(A, row_major, off, pad, dtype):
    """The lines of A behind a pointer `off` REAL elements into a NaN-filled buffer, `pad` complex elements of NaN behind every line.
    Returns (tensor whose data_ptr is the matrix, ld)."""
    m, n = A.shape
    length, cnt = (n, m) if row_major else (m, n)
    ld = length + pad
    rt = torch.float64 if np.dtype(dtype) == np.complex128 else torch.float32
    buf = torch.full((off + 2 * cnt * ld + 8,), math.nan, dtype=rt, device="cuda:0")
    lines = np.ascontiguousarray(np.asarray(A if row_major else A.T, dtype=dtype))
    buf[off:off + 2 * cnt * ld].view(cnt, ld, 2)[:, :length, :] = torch.view_as_real(torch.from_numpy(lines).to("cuda:0"))
    return buf[off:], ld


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", NORM_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_norms_exact_on_the_axes_and_random(shape, dtype):
    m, n = shape
    rng = np.random.default_rng([21, m, n])
    G = (rng.integers(-8, 9, size=(m, n)) * C.UNITS[rng.integers(0, 4, size=(m, n))]).astype(dtype)
    Ar = (rng.uniform(-1, 1, size=(m, n)) + 1j * rng.uniform(-1, 1, size=(m, n))).astype(dtype)
    mods = np.hypot(Ar.real.astype(np.float64), Ar.imag.astype(np.float64))
    offsets = [(0, 0), (0, 3), (1, 0), (1, 3)] + ([(2, 0), (2, 1), (3, 2)] if np.dtype(dtype) == np.complex64 else [(0, 4)])
    worst = 0.0
    for norm in NORMS:
        want = float(np.abs(G.astype(np.complex128)).sum(axis=0 if norm == C.NORM_ONE else 1).max())
        assert want == np.rint(want)
        lines = mods.T if norm == C.NORM_ONE else mods
        ref = max(math.fsum(line) for line in lines)
        length = lines.shape[1]
        for row_major in (0, 1):
            first = None
            for off, pad in offsets:
                t, ld = padded(G, row_major, off, pad, dtype)
                assert clange(t, norm, m, n, ld, row_major, dtype) == want, (m, n, norm, row_major, off, pad)
                t, ld = padded(Ar, row_major, off, pad, dtype)
                got = clange(t, norm, m, n, ld, row_major, dtype)
                first = got if first is None else first
                assert got == first, (m, n, norm, row_major, off, pad, got, first)       # the same bits whatever alignment and lda
                assert abs(got - ref) <= (length + 2) * EPS64 * ref, (m, n, norm, row_major, got, ref)
                worst = max(worst, abs(got - ref) / ((length + 2) * EPS64 * ref))
    print(f"lange {sfx(dtype)} {m}x{n}: worst |got - fsum| / ((len + 2) eps64 ref) = {worst:.3f}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_norms_nan_inf_empty_and_argument_rules(dtype):
    rng = np.random.default_rng(22)
    A = (rng.uniform(-1, 1, size=(65, 130)) + 1j * rng.uniform(-1, 1, size=(65, 130))).astype(dtype)
    for norm in NORMS:
        for row_major in (0, 1):
            to = dev_rm if row_major else dev_cm
            ld = 130 if row_major else 65
            for z in (complex(np.nan, 0.0), complex(0.0, np.nan), complex(np.inf, np.nan), complex(np.nan, -np.inf)):
                B = A.copy(); B[64, 129] = z
                assert math.isnan(clange(to(B, dtype), norm, 65, 130, ld, row_major, dtype)), (norm, row_major, z)
            B = A.copy(); B[0, 0] = complex(0.0, np.nan); B[3, 7] = complex(np.inf, 0.0)    # max must not drop the NaN behind a larger value
            assert math.isnan(clange(to(B, dtype), norm, 65, 130, ld, row_major, dtype))
            for z in (complex(np.inf, 1.0), complex(1.0, -np.inf), complex(-np.inf, np.inf)):
                B = A.copy(); B[3, 7] = z
                assert clange(to(B, dtype), norm, 65, 130, ld, row_major, dtype) == math.inf, (norm, row_major, z)
    z = dev_rm(np.zeros((2, 2)), dtype)
    for norm in NORMS:
        assert clange(z, norm, 0, 5, 1, 0, dtype) == 0.0 and clange(z, norm, 5, 0, 5, 0, dtype) == 0.0
    out = ctypes.c_double(0.0)
    for bad in (0, 3, -1):
        with pytest.raises(_ffi.RfluError):
            handle().call(f"rflu_lange_{sfx(dtype)}_dev", bad, 2, 2, ptr(z), 2, 0, ctypes.byref(out))
    with pytest.raises(_ffi.RfluError):
        handle().call(f"rflu_lange_{sfx(dtype)}_dev", 1, 2, 2, ptr(z), 1, 0, ctypes.byref(out))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_batched_norm_equals_the_single_entry(dtype):
    rng = np.random.default_rng(23)
    for n, batch in [(1, 7), (7, 67), (64, 7), (128, 7), (129, 3)]:
        A = (rng.uniform(-1, 1, size=(batch, n, n)) + 1j * rng.uniform(-1, 1, size=(batch, n, n))).astype(dtype)
        A[batch // 2, n - 1, n - 1] = complex(np.inf, np.nan)
        for row_major in (0, 1):
            t = torch.from_numpy(np.ascontiguousarray(A if row_major else A.transpose(0, 2, 1))).to("cuda:0")
            for norm in NORMS:
                got = clange_batched(t, norm, batch, n, n, n, n * n, row_major, dtype)
                for b in range(batch):
                    one = clange(t[b], norm, n, n, n, row_major, dtype)
                    assert same(got[b], one), (n, batch, b, norm, row_major, got[b], one)
                assert math.isnan(got[batch // 2]) and np.isfinite(np.delete(got, batch // 2)).all()
    out = torch.full((3,), math.nan, dtype=torch.float64, device="cuda:0")
    handle().call(f"rflu_lange_batched_{sfx(dtype)}_dev", 1, 3, 0, 4, ptr(out), 1, 1, 0, ptr(out))
    assert (out.cpu().numpy() == 0.0).all()                                              # empty matrices


# ---- 2. the estimate of one matrix, exact ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", C.EXACT_SIZES)
def test_embedded_real_exact_factors(n, dtype):
    """The real exact factors with zero imaginary parts return the REAL restatement's rcond by `==`: device and host entries, both norms.
    Float32 is certified by cond_cases.vector_bits at every one of these sizes (tests/test_complex_cond_cases.py asserts it)."""
    F, e = C.embedded_exact(n)
    for norm in NORMS:
        an = R.case_anorm(e, norm)
        want = R.rcond_restatement(e.F, norm, an, C.real_of(dtype))
        for kind in ("cm", "host"):
            got = cgecon(F, norm, an, dtype, kind)
            assert got == want, (n, norm, kind, got, want)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_axis_scaled_family_single(dtype):
    """Factors whose U has its columns multiplied by powers of i, every vector of the estimator's trace on the axes: `==` with the
    restatement, which a kernel that uses M^T where M^H belongs misses on at least 6 of the 1-norm cases."""
    _, notice = C.axis_search()
    hit = 0
    for norm in NORMS:
        for c in C.axis_cases(norm):
            an = C.axis_anorm(c, norm)
            want = C.crcond_restatement(c.F, norm, an, dtype)
            for kind in ("cm", "host"):
                got = cgecon(c.F, norm, an, dtype, kind)
                assert got == want, (c.n, c.seed, norm, kind, got, want)
            hit += (c, norm) in notice
    assert hit >= 6


def random_factors(family, n, seed, dtype):
    lu, _ = C.lapack_factors(C.random_matrix(family, n, seed, dtype))
    return lu


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_axis_scaled_family_in_batches(dtype):
    """The same cases as members of batches of 67 / 7 / 1 between random members, in both orientations: `==` for every one of them."""
    for norm in NORMS:
        cases = C.axis_cases(norm)
        for n in sorted({c.n for c in cases}):
            mine = [c for c in cases if c.n == n]
            for batch in C.BATCHES:
                Fs, ans, want = [], [], {}
                for b in range(batch):
                    if b % 2 == 0:
                        c = mine[(b // 2) % len(mine)]
                        Fs.append(c.F); ans.append(C.axis_anorm(c, norm))
                        want[b] = C.crcond_restatement(c.F, norm, ans[-1], dtype)
                    else:
                        Fs.append(random_factors(C.FAMILIES[(b // 2) % 3], n, b, dtype)); ans.append(1.0)
                for rm in (False, True):
                    got = cgecon_batched(Fs, norm, ans, dtype, rm)
                    for b, w in want.items():
                        assert got[b] == w, (n, batch, b, norm, rm, got[b], w)
                    assert (got[1::2] > 0).all()


# ---- 3. the estimate at rounding level ---------------------------------------------------------------------------------------------
def rounding(n, dtype):
    """4 n eps_T: gamma_n = n eps_T per triangle, two triangles, and as much again for the restatement the estimate is measured against.
    No condition number enters."""
    return 4.0 * n * eps_of(dtype)


def check_bars(est, restated, true, what, n, dtype):
    tol = 2.0 * abs(restated - true) / true + rounding(n, dtype)
    assert est <= true * (1.0 + tol), (what, "overestimate", est / true, tol)
    assert est >= true / 3.0, (what, "below a third", est / true)
    return est / true


def check_against_restatement(est, F, norm, restated, what, n, dtype):
    """On factors with a decision margin: the device's estimate against the restatement's on the same factors.  The bar is measured, not
    guessed: 8 times the relative gap between the restatement in the element precision and one precision up, plus n eps.  Returns the
    measured (difference, bar), or None when some decision of the restatement is too close to call."""
    if C.decision_margin(F, norm, dtype) <= C.margin_bar(n, dtype):
        return None
    _, up, _ = C.crcond_restatement(F, norm, 1.0, C.wider(dtype), detail=True)
    gap = abs(restated - up) / up
    bar = 8.0 * gap + n * eps_of(dtype)
    diff = abs(est - restated) / restated
    print(f"  {what}: |device - restatement| / restatement = {diff:.3e}, restatement's own gap {gap:.3e}, bar {bar:.3e}")
    assert diff <= bar, (what, diff, gap, bar)
    return diff, bar


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", C.CGECON_SIZES)
def test_random_rcond_on_the_devices_own_factors(n, dtype):
    lo, hi, compared = math.inf, 0.0, 0
    for family in C.FAMILIES:
        A = C.random_matrix(family, n, C.pick_seed(family, n, dtype, margin=True), dtype)
        dA = dev_cm(A, dtype)
        anorm = {norm: rf.opnorm_complex(dA, PNORM[norm]) for norm in NORMS}
        F = rf.lu_complex_(dA.clone(), check=False)
        assert F.info == 0
        lu_host = F.factors.cpu().numpy()
        true = C.true_inverse_norms(C.factor_product(lu_host))     # LAPACK's ipiv is no comparator: the pivot rule differs
        for norm in NORMS:
            assert anorm[norm] == pytest.approx(np.linalg.norm(A.astype(np.complex128), NPORD[norm]), rel=(n + 2) * EPS64)
            _, restated, solves = C.crcond_restatement(lu_host, norm, anorm[norm], dtype, detail=True)
            assert solves <= 11
            rc = rf.rcond_complex(F, anorm[norm], PNORM[norm])
            assert rc == cgecon(lu_host, norm, anorm[norm], dtype, "host"), (family, n, norm)     # the same kernels on the same layout
            est = 1.0 / (rc * anorm[norm])
            ratio = check_bars(est, restated, true[norm], (family, n, norm), n, dtype)
            lo, hi = min(lo, ratio), max(hi, ratio)
            compared += check_against_restatement(est, lu_host, norm, restated, (family, n, norm), n, dtype) is not None
    print(f"cgecon n={n} {sfx(dtype)}: est / true in [{lo:.4f}, {hi:.8f}], allowance {rounding(n, dtype):.2e}, {compared} of 6 compared "
          f"with the restatement")
    assert compared >= 1, "no input of this size kept its decision margin on the device's factors"


DISTINCT = 4      # kept inputs per family that the random members of a batch cycle through


@functools.lru_cache(maxsize=None)
def random_member(family, k, n, dtype):
    """The k-th kept input of a family at size n as (LAPACK's factors, anorm per norm, true ||(L U)^-1|| per norm)."""
    seed = -1
    for _ in range(k + 1):
        seed = C.pick_seed(family, n, dtype, seed + 1)
    lu = random_factors(family, n, seed, dtype)
    LU = C.factor_product(lu)
    return lu, {norm: float(np.linalg.norm(LU, NPORD[norm])) for norm in NORMS}, C.true_inverse_norms(LU)


def batch_members(n, batch, dtype):
    """Random members: member b is input (b // 3) % DISTINCT of family b % 3 (a batch of 67 repeats its twelve inputs in other slots)."""
    return [random_member(C.FAMILIES[b % 3], (b // 3) % DISTINCT, n, dtype) for b in range(batch)]


@functools.lru_cache(maxsize=None)
def restated_estimate(family, k, n, dtype, norm):
    F, an, _ = random_member(family, k, n, dtype)
    return C.crcond_restatement(F, norm, an[norm], dtype, detail=True)[1]


def batched_sizes():
    return [(n, dt) for dt in DTYPES for n in C.CBATCHED_SIZES[dt]]


@pytest.mark.parametrize("n,dtype", batched_sizes(), ids=lambda v: str(v) if isinstance(v, int) else sfx(v))
def test_batched_rcond(n, dtype):
    """Batches of 67 / 7 / 1 (never a multiple of the groups per workgroup: an invalid group exists), both orientations, both norms:
    EVERY member inside the bars, and those with a decision margin within the measured bar of the restatement."""
    lo, hi, compared = math.inf, 0.0, 0
    for batch in C.BATCHES:
        members = batch_members(n, batch, np.dtype(dtype).type)
        for norm in NORMS:
            anorms = [m[1][norm] for m in members]
            res = {rm: cgecon_batched([m[0] for m in members], norm, anorms, dtype, rm) for rm in (False, True)}
            for b, (F, an, trues) in enumerate(members):
                true = trues[norm]
                restated = restated_estimate(C.FAMILIES[b % 3], (b // 3) % DISTINCT, n, np.dtype(dtype).type, norm)
                assert res[False][b] == res[True][b], (n, batch, b, norm)       # the same LDS image from either orientation
                assert res[False][b] > 0
                est = 1.0 / (res[False][b] * an[norm])
                r = check_bars(est, restated, true, (n, batch, b, norm), n, dtype)
                lo, hi = min(lo, r), max(hi, r)
                if batch == 7:
                    compared += check_against_restatement(est, F, norm, restated, (n, batch, b, norm), n, dtype) is not None
    print(f"cgecon_batched n={n} {sfx(dtype)}: est / true in [{lo:.4f}, {hi:.8f}], allowance {rounding(n, dtype):.2e}, {compared} of 14 "
          f"compared with the restatement")
    assert compared >= 1


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_above_the_one_launch_limit(dtype):
    """One size above the limit (65 / 129): a column-major batch goes through the loop over the single entry and gives its bits; a
    row-major one is refused with "column-major only"."""
    n = C.CBATCHED_LIMIT[dtype] + 1
    members = batch_members(n, 3, np.dtype(dtype).type)
    for norm in NORMS:
        anorms = [m[1][norm] for m in members]
        got = cgecon_batched([m[0] for m in members], norm, anorms + [], dtype, False)
        for b, (F, an, trues) in enumerate(members):
            assert got[b] == cgecon(F, norm, an[norm], dtype), (n, b, norm)
            _, restated, _ = C.crcond_restatement(F, norm, an[norm], dtype, detail=True)
            check_bars(1.0 / (got[b] * an[norm]), restated, trues[norm], (n, b, norm), n, dtype)
        neg = cgecon_batched([m[0] for m in members], norm, [anorms[0], -1.0, anorms[2]], dtype, False)
        assert neg[0] == got[0] and math.isnan(neg[1]) and neg[2] == got[2]
        with pytest.raises(_ffi.RfluError, match="column-major only"):
            cgecon_batched([m[0] for m in members], norm, anorms, dtype, True)


# ---- 4. special values and state ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_special_values_in_their_order(dtype):
    rng = np.random.default_rng(24)
    h, s = handle(), sfx(dtype)
    nan = complex(np.nan, 0.0)
    for n in (3, 40, 130, 300):
        lu = random_factors("uniform", n, 1, dtype)
        fits = n <= C.CBATCHED_LIMIT[dtype]
        for norm in NORMS:
            good = cgecon(lu, norm, 1.0, dtype)
            assert 0 < good < math.inf
            cases = []                                            # (factors, anorm, expected)
            cases.append((lu, math.nan, math.nan))                # 2. anorm NaN
            cases.append((lu, 0.0, 0.0))                          # 3. anorm == 0
            Z = lu.copy(); Z[n // 2, n // 2] = 0
            cases.append((Z, 1.0, 0.0))                           # 4. a u_ii with both parts zero
            for z in (complex(0.0, np.nan), nan, complex(np.inf, np.nan)):
                for at in ((n - 1, 0), (0, n - 1), (n // 2, n // 2)):
                    Z = lu.copy(); Z[at] = z
                    cases.append((Z, 1.0, math.nan))              # 5. a NaN in either part of any factor entry
            Z = lu.copy(); Z[n - 1, 0] = nan
            cases.append((Z, 0.0, 0.0))                           # anorm = 0 with NaN factors: 0
            Z = lu.copy(); Z[n // 2, n // 2] = 0; Z[n - 1, 0] = complex(0.0, np.nan)
            cases.append((Z, 1.0, 0.0))                           # a zero u_ii with NaN factors: 0
            Z = lu.copy(); Z[n // 2, n // 2] = 1j
            cases.append((Z, 1.0, None))                          # u_ii = 1j is not singular
            for F, an, want in cases:
                for kind in ("cm", "host"):
                    got = cgecon(F, norm, an, dtype, kind)
                    assert (0 < got < math.inf) if want is None else same(got, want), (n, norm, kind, an, got, want)
            # the same as members of one batch (above the one-launch limit: the column-major loop over the single entry)
            Fs = [lu] + [c[0] for c in cases] + [lu]
            ans = [1.0] + [c[1] for c in cases] + [-1.0]
            for rm in ((False, True) if fits else (False,)):
                got = cgecon_batched(Fs, norm, ans, dtype, rm)
                assert got[0] > 0 and math.isnan(got[-1])         # a member's anorm < 0: NaN in its own output only
                for b, (F, an, want) in enumerate(cases):
                    g = got[1 + b]
                    assert (0 < g < math.inf) if want is None else same(g, want), (n, norm, rm, b, an, g, want)
                assert got[0] == cgecon_batched([lu], norm, [1.0], dtype, rm)[0]       # the neighbours touched nothing
            with pytest.raises(_ffi.RfluError):
                cgecon(lu, norm, -1.0, dtype)
            with pytest.raises(_ffi.RfluError):
                cgecon(lu, norm, -1.0, dtype, "host")
        with pytest.raises(_ffi.RfluError):
            cgecon(lu, 3, 1.0, dtype)
    out = ctypes.c_double(math.nan)
    t = dev_rm(np.zeros((2, 2)), dtype)
    h.call(f"rflu_gecon_{s}_dev", 1, 0, ptr(t), 1, 1.0, ctypes.byref(out))
    assert out.value == 1.0                                                   # 1. n == 0
    out = ctypes.c_double(math.nan)
    h.call(f"rflu_gecon_{s}", 1, 0, ctypes.c_void_p(0), 1, math.nan, ctypes.byref(out))
    assert out.value == 1.0                                                   # n == 0 comes before a NaN anorm
    with pytest.raises(_ffi.RfluError):
        h.call(f"rflu_gecon_{s}_dev", 1, 2, ptr(t), 1, 1.0, ctypes.byref(out))              # lda < n
    with pytest.raises(_ffi.RfluError):
        h.call(f"rflu_gecon_{s}_dev", 1, 2, ctypes.c_void_p(0), 2, 1.0, ctypes.byref(out))  # NULL
    # 6. overflow in the substitution: rcond = 0, not NaN
    rt = C.real_of(dtype)
    tiny = (np.diag(np.full(4, np.finfo(rt).tiny)) + np.triu(np.full((4, 4), np.finfo(rt).max / 2), 1)).astype(dtype)
    for norm in NORMS:
        assert cgecon(tiny, norm, 1.0, dtype) == 0.0
        assert cgecon_batched([tiny, np.eye(4)], norm, [1.0, 2.0], dtype, False).tolist() == [0.0, 0.5]
    # the batched entry's own rules
    an = torch.ones(4, dtype=torch.float64, device="cuda:0")
    o = torch.full((4,), math.nan, dtype=torch.float64, device="cuda:0")
    big = dev_rm(np.zeros((4, 3, 3)), dtype)
    h.call(f"rflu_gecon_batched_{s}_dev", 1, 4, 0, ptr(big), 1, 1, 0, ptr(an), ptr(o))
    assert (o.cpu().numpy() == 1.0).all()                                                    # n == 0
    h.call(f"rflu_gecon_batched_{s}_dev", 1, 0, 3, ptr(big), 3, 9, 0, ptr(an), ptr(o))       # batch == 0
    for args in ((3, 4, 3, ptr(big), 3, 9, 0, ptr(an), ptr(o)),                              # norm
                 (1, 4, 3, ptr(big), 2, 9, 0, ptr(an), ptr(o)),                              # lda < n
                 (1, 4, 3, ptr(big), 3, 8, 0, ptr(an), ptr(o)),                              # matrices overlap
                 (1, -1, 3, ptr(big), 3, 9, 0, ptr(an), ptr(o)),
                 (1, 4, 3, ptr(big), 3, 9, 0, ctypes.c_void_p(0), ptr(o))):
        with pytest.raises(_ffi.RfluError):
            h.call(f"rflu_gecon_batched_{s}_dev", *args)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_determinism_alignment_and_the_shared_workspace(dtype):
    """cgecon repeats itself bit for bit, also from a padded lda and a pointer aligned to the real type only; a solve, an inverse and a
    factorization that follow it on the same handle equal those of a fresh handle."""
    n = 300
    A = C.random_matrix("uniform", n, C.pick_seed("uniform", n, dtype), dtype)
    dA = dev_cm(A, dtype)
    anorm = rf.opnorm_complex(dA, 1)
    F = rf.lu_complex_(dA.clone(), check=False)
    lu_host = F.factors.cpu().numpy()
    rng = np.random.default_rng(3)
    B = dev_cm((rng.uniform(-1, 1, size=(n, 4)) + 1j * rng.uniform(-1, 1, size=(n, 4))).astype(dtype), dtype)
    fresh = _ffi.Handle(0)
    try:
        x_fresh = rf.ldiv_complex_(F, B.clone(), handle=fresh)
        inv_fresh = rf.inv_complex(F, handle=fresh)
        G_fresh = rf.lu_complex_(dA.clone(), check=False, handle=fresh)
    finally:
        fresh.close()
    used = _ffi.Handle(0)
    try:
        first = [rf.rcond_complex(F, anorm, p, handle=used) for p in (1, "inf")]
        for _ in range(2):
            assert [rf.rcond_complex(F, anorm, p, handle=used) for p in (1, "inf")] == first
        for off, pad in ((1, 0), (0, 3), (1, 3)):
            t, ld = padded(lu_host, 0, off, pad, dtype)
            for k, norm in enumerate(NORMS):
                out = ctypes.c_double(math.nan)
                used.call(f"rflu_gecon_{sfx(dtype)}_dev", norm, n, ptr(t), ld, anorm, ctypes.byref(out))
                assert out.value == first[k], (off, pad, norm)
        assert torch.equal(rf.ldiv_complex_(F, B.clone(), handle=used), x_fresh)
        assert rf.rcond_complex(F, anorm, 1, handle=used) == first[0]
        assert torch.equal(rf.inv_complex(F, handle=used), inv_fresh)
        assert rf.rcond_complex(F, anorm, "inf", handle=used) == first[1]
        G = rf.lu_complex_(dA.clone(), check=False, handle=used)
        assert torch.equal(G.factors, G_fresh.factors) and torch.equal(G.ipiv, G_fresh.ipiv)
        assert torch.equal(G.factors, F.factors)
    finally:
        used.close()


# ---- 5. the Python functions -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_cond_opnorm_adjoint_and_batched_functions(dtype):
    n = 40
    A = C.random_matrix("uniform", n, C.pick_seed("uniform", n, dtype), dtype)
    dA = dev_cm(A, dtype)
    before = dA.clone()
    lu_host = rf.lu_complex(dA, check=False).factors.cpu().numpy()            # the factors cond_complex computes inside
    true = C.true_inverse_norms(C.factor_product(lu_host))
    for p in (1, math.inf, "inf"):
        norm = C.NORM_ONE if p == 1 else C.NORM_INF
        ref = float(np.real(np.linalg.cond(A.astype(np.complex128), NPORD[norm])))
        got = rf.cond_complex(dA, p)
        anorm = rf.opnorm_complex(dA, p)
        _, restated, _ = C.crcond_restatement(lu_host, norm, anorm, dtype, detail=True)
        # the bars of the estimate: above, against the inverse of what the factors multiply to; below, a third of NumPy's value
        assert got <= anorm * true[norm] * (1 + 2 * abs(restated - true[norm]) / true[norm] + rounding(n, dtype)), (p, got, ref)
        assert got >= ref / 3, (p, got, ref)
        assert rf.cond_complex(A, p) == pytest.approx(got, rel=1e-3)          # NumPy input: the host entries on the same matrix
        q = math.inf if p == 1 else 1
        assert anorm == rf.opnorm_complex(A, p) == rf.opnorm_complex(rf.Adjoint(dA), q)
        assert anorm == pytest.approx(rf.opnorm_complex(dA.T.conj(), q), rel=(n + 2) * EPS64)   # the adjoint itself, torch's lazy conjugate
        assert rf.opnorm_complex(dev_rm(A, dtype), p) == pytest.approx(anorm, rel=(n + 2) * EPS64)   # another kernel, another order
    assert torch.equal(dA, before)
    F = rf.lu_complex(dA, check=False)
    a1, ai = rf.opnorm_complex(dA, 1), rf.opnorm_complex(dA, math.inf)
    assert rf.rcond_complex(rf.Adjoint(F), ai, 1) == rf.rcond_complex(F, ai, math.inf)      # ||A'||_1 = ||A||_inf
    assert rf.rcond_complex(rf.Adjoint(F), a1, "inf") == rf.rcond_complex(F, a1, 1)
    assert rf.cond_complex(dev_cm(np.ones((4, 4)), dtype), 1) == math.inf
    with pytest.raises(TypeError, match="real element types go to cond"):
        rf.cond_complex(torch.eye(3, dtype=torch.float32, device="cuda:0"))
    with pytest.raises(TypeError, match="opnorm_batched"):
        rf.opnorm_complex_batched(torch.zeros((2, 3, 3), dtype=torch.float64, device="cuda:0"))
    # batched functions: entry b is the single functions' value on matrix b
    batch, n = 7, 33
    seeds = []
    for b in range(batch):                                                    # kept inputs, each with a seed of its own
        seeds.append(C.pick_seed("graded", n, dtype, seeds[-1] + 1 if seeds else 0))
    host = np.stack([C.random_matrix("graded", n, sd, dtype) for sd in seeds])
    host[3] = 1.0                                                             # a singular member
    for t in (torch.from_numpy(host).to("cuda:0"), torch.from_numpy(np.ascontiguousarray(host.transpose(0, 2, 1))).to("cuda:0").transpose(1, 2)):
        for p in (1, math.inf):
            norm = C.NORM_ONE if p == 1 else C.NORM_INF
            nb = rf.opnorm_complex_batched(t, p).cpu().numpy()
            assert [rf.opnorm_complex(t[b], p) for b in range(batch)] == list(nb)
            cb = rf.cond_complex_batched(t, p).cpu().numpy()
            assert cb[3] == math.inf
            lus = rf.lu_complex_batched(t, check=False).factors.cpu().numpy()   # the factors cond_complex_batched computes inside
            for b in (0, 1, 2, 4, 5, 6):
                ref = float(np.real(np.linalg.cond(host[b].astype(np.complex128), NPORD[norm])))
                tr = C.true_inverse_norms(C.factor_product(lus[b]))[norm]
                _, restated, _ = C.crcond_restatement(lus[b], norm, nb[b], dtype, detail=True)
                assert cb[b] <= nb[b] * tr * (1 + 2 * abs(restated - tr) / tr + rounding(n, dtype)), (b, p, cb[b], ref)
                assert cb[b] >= ref / 3, (b, p, cb[b], ref)
            assert torch.equal(rf.opnorm_complex_batched(rf.Adjoint(t), p), rf.opnorm_complex_batched(t, math.inf if p == 1 else 1))
