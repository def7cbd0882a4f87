"""-m gpu: operator norms and the condition estimate (rflu_lange_*, rflu_gecon_*, rflu_gecon_batched_*; csrc/condest.hip,
gecon_batched_kernel of csrc/batched.hip, gecon_dev of csrc/driver.cpp) and the Python functions above them.

  * norms: integer matrices by `==` with NumPy, random ones within n eps64 of an fsum reference; padding full of NaN and a pointer aligned
    to the element only give the bits of the packed call; the batched entry gives the single entry's bits;
  * rcond of constructed factors (tests/cond_cases.py: every vector of every iteration has an exactly representable solution in Float32
    under any order of substitution; tests/test_cond_cases.py proves it and shows which planted faults those cases notice) equals the
    numpy restatement's by `==`, single and batched, both norms, both types, every storage;
  * rcond of random matrices meets three bars: est <= true (1 + tol) with true = ||(L U)^-1|| of the downloaded factors and tol = twice the restatement's own gap plus 4 n eps_T (no
    condition number), est >= true / 3 (Higham's bar; the CPU test holds the reference to
    1/2 on the same inputs), est >= the estimator's own first step recomputed through ldiv_ with NotIPIV;
  * special values, determinism, a solve and an inverse after gecon on the same handle, and -- the batched kernel's hazard -- members
    with different iteration counts in one workgroup.
Measured ratios are printed (pytest -s)."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import cond_cases as C
import recursivefactorization.jl_amd as rf
from gpu_util import handle, ptr, sfx, tdtype, to_dev_cm, to_dev_rm
from recursivefactorization.jl_amd import _ffi

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
NORMS = [C.NORM_ONE, C.NORM_INF]
EPS64 = float(np.finfo(np.float64).eps)
NPORD = {C.NORM_ONE: 1, C.NORM_INF: np.inf}


def lange(t, norm, m, n, ld, row_major, dtype, h=None):
    out = ctypes.c_double(-1.0)
    (h or handle()).call(f"rflu_lange_{sfx(dtype)}_dev", norm, m, n, ptr(t), ld, row_major, ctypes.byref(out))
    return out.value


def lange_batched(t, norm, batch, m, n, ld, stride, row_major, dtype):
    out = torch.full((batch,), -1.0, dtype=torch.float64, device="cuda:0")
    handle().call(f"rflu_lange_batched_{sfx(dtype)}_dev", norm, batch, m, n, ptr(t), ld, stride, row_major, ptr(out))
    return out.cpu().numpy()


def gecon(F, norm, anorm, dtype, kind="cm", h=None):
    """F: the packed factors as a numpy matrix; kind: cm / rm (device) or host."""
    n = F.shape[0]
    out = ctypes.c_double(-1.0)
    Fd = np.asarray(F, dtype=dtype)
    h = h or handle()
    if kind == "host":
        Fh = np.asfortranarray(Fd)
        h.call(f"rflu_gecon_{sfx(dtype)}", norm, n, ctypes.c_void_p(Fh.ctypes.data), max(n, 1), float(anorm), ctypes.byref(out))
    else:
        t = to_dev_cm(Fd) if kind == "cm" else to_dev_rm(Fd)
        h.call(f"rflu_gecon_{'rm_' if kind == 'rm' else ''}{sfx(dtype)}_dev", norm, n, ptr(t), max(n, 1), float(anorm), ctypes.byref(out))
    return out.value


def gecon_batched(Fs, norm, anorms, dtype, row_major):
    """Fs: list of packed factor matrices of one size."""
    batch, n = len(Fs), Fs[0].shape[0]
    stack = np.stack([np.asarray(F, dtype=dtype) if row_major else np.asarray(F, dtype=dtype).T for F in Fs])
    t = torch.from_numpy(np.ascontiguousarray(stack)).to("cuda:0")
    an = torch.tensor(list(anorms), dtype=torch.float64, device="cuda:0")
    out = torch.full((batch,), -1.0, dtype=torch.float64, device="cuda:0")
    handle().call(f"rflu_gecon_batched_{sfx(dtype)}_dev", norm, batch, n, ptr(t), max(n, 1), n * n, int(row_major), ptr(an), ptr(out))
    return out.cpu().numpy()


def same(a, b):
    return a == b or (a != a and b != b)


# ---- 1. norms ----------------------------------------------------------------------------------------------------------------------
NORM_SHAPES = [(m, n) for m in (1, 2, 63, 64, 65, 257) for n in (1, 2, 63, 64, 65, 257)] + [(1025, 3), (3, 1025), (1025, 1025)]


def fsum_norm(A, norm):
    B = np.abs(np.asarray(A, dtype=np.float64))
    lines = B.T if norm == C.NORM_ONE else B
    return max(math.fsum(line) for line in lines)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_norms_integer_and_random(dtype):
    rng = np.random.default_rng(11)
    worst = 0.0
    for m, n in NORM_SHAPES:
        Ai = rng.integers(-8, 9, size=(m, n)).astype(dtype)
        Ar = rng.uniform(-1, 1, size=(m, n)).astype(dtype)
        for norm in NORMS:
            for row_major in (0, 1):
                to = to_dev_rm if row_major else to_dev_cm
                ld = n if row_major else m
                assert lange(to(Ai), norm, m, n, ld, row_major, dtype) == np.linalg.norm(Ai.astype(np.float64), NPORD[norm]), (m, n, norm, row_major)
                got, ref = lange(to(Ar), norm, m, n, ld, row_major, dtype), fsum_norm(Ar, norm)
                worst = max(worst, abs(got - ref) / (max(m, n) * EPS64 * ref))
                assert abs(got - ref) <= max(m, n) * EPS64 * ref, (m, n, norm, row_major, got, ref)
    print(f"lange {np.dtype(dtype).name}: worst |got - fsum| / (n eps64 ref) = {worst:.3f}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_norms_padding_alignment_nan_inf_empty(dtype):
    rng = np.random.default_rng(12)
    td = tdtype(dtype)
    for m, n in [(1, 1), (2, 65), (63, 64), (65, 63), (257, 257), (1025, 3), (3, 1025)]:
        A = rng.uniform(-1, 1, size=(m, n)).astype(dtype)
        for norm in NORMS:
            for row_major in (0, 1):
                length, cnt = (n, m) if row_major else (m, n)
                packed = lange(to_dev_rm(A) if row_major else to_dev_cm(A), norm, m, n, length, row_major, dtype)
                for off, pad in ((0, 3), (1, 0), (1, 3), (0, 4)):      # NaN padding; a pointer aligned to the element only; both; 16-byte rows
                    ld = length + pad
                    buf = torch.full((off + cnt * ld + 8,), float("nan"), dtype=td, device="cuda:0")
                    view = buf[off:off + cnt * ld].view(cnt, ld)
                    view[:, :length] = torch.from_numpy(np.ascontiguousarray(A if row_major else A.T)).to("cuda:0")
                    got = lange(buf[off:], norm, m, n, ld, row_major, dtype)
                    assert got == packed, (m, n, norm, row_major, off, pad, got, packed)
    A = rng.uniform(-1, 1, size=(65, 130)).astype(dtype)
    for norm in NORMS:
        for row_major in (0, 1):
            to = to_dev_rm if row_major else to_dev_cm
            ld = 130 if row_major else 65
            B = A.copy(); B[64, 129] = np.nan
            assert math.isnan(lange(to(B), norm, 65, 130, ld, row_major, dtype))
            B = A.copy(); B[0, 0] = np.nan; B[3, 7] = np.inf       # max must not drop the NaN behind a larger value
            assert math.isnan(lange(to(B), norm, 65, 130, ld, row_major, dtype))
            B = A.copy(); B[3, 7] = -np.inf
            assert lange(to(B), norm, 65, 130, ld, row_major, dtype) == math.inf
    z = torch.zeros(4, dtype=td, device="cuda:0")
    for norm in NORMS:
        assert lange(z, norm, 0, 5, 1, 0, dtype) == 0.0 and lange(z, norm, 5, 0, 5, 0, dtype) == 0.0
    out = ctypes.c_double(0.0)
    for bad in (0, 3, -1):
        with pytest.raises(_ffi.RfluError):
            handle().call(f"rflu_lange_{sfx(dtype)}_dev", bad, 2, 2, ptr(z), 2, 0, ctypes.byref(out))
    with pytest.raises(_ffi.RfluError):
        handle().call(f"rflu_lange_{sfx(dtype)}_dev", 1, 2, 2, ptr(z), 1, 0, ctypes.byref(out))


def test_norm_across_more_line_groups_than_one_grid_dimension():
    """A row-major 1-norm of 65535 * 256 + 300 rows: more groups of 256 lines than the grid's y dimension holds, so workgroups wrap
    around the groups.  Small integers: the sum is exact."""
    m = 65535 * 256 + 300
    t = torch.ones((m, 1), dtype=torch.float32, device="cuda:0")
    t[m - 1, 0] = -3.0
    assert lange(t, C.NORM_ONE, m, 1, 1, 1, np.float32) == float(m + 2)
    assert lange(t, C.NORM_INF, m, 1, 1, 1, np.float32) == 3.0


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_batched_norm_equals_the_single_entry(dtype):
    rng = np.random.default_rng(13)
    for (m, n), batch in [((1, 1), 7), ((2, 3), 67), ((63, 65), 67), ((64, 64), 7), ((128, 128), 67), ((128, 5), 1), ((129, 7), 7), ((257, 130), 1)]:
        A = rng.uniform(-1, 1, size=(batch, m, n)).astype(dtype)
        A[batch // 2, m - 1, n - 1] = np.nan
        for row_major in (0, 1):
            t = torch.from_numpy(np.ascontiguousarray(A if row_major else A.transpose(0, 2, 1))).to("cuda:0")
            ld = n if row_major else m
            for norm in NORMS:
                got = lange_batched(t, norm, batch, m, n, ld, m * n, row_major, dtype)
                for b in range(batch):
                    one = lange(t[b], norm, m, n, ld, row_major, dtype)
                    assert same(got[b], one), (m, n, batch, b, norm, row_major, got[b], one)
                assert math.isnan(got[batch // 2]) and np.isfinite(np.delete(got, batch // 2)).all()


# ---- 2. the condition estimate of one matrix ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("n", C.GECON_SIZES)
def test_exact_rcond(n, dtype):
    for e in C.exact_cases(n):
        for norm in NORMS:
            anorm = C.case_anorm(e, norm)
            want = C.rcond_restatement(e.F, norm, anorm, dtype)
            for kind in ("cm", "rm", "host"):
                got = gecon(e.F, norm, anorm, dtype, kind)
                assert got == want, (n, norm, kind, got, want)


def random_case(family, n, dtype):
    """(A, the GPU's own lu of it, the downloaded factors, anorm by the GPU in both norms, true ||(L U)^-1|| in both norms).  `true` is
    taken from the product of the DOWNLOADED factors: the estimator estimates the inverse of what its factors multiply to, and the
    factorization's own backward error, which grows with cond(A), stays out of every bar."""
    A = C.random_matrix(family, n, C.pick_seed(family, n, dtype), dtype)
    dA = to_dev_cm(A)
    anorm = {norm: rf.opnorm(dA, 1 if norm == C.NORM_ONE else math.inf) for norm in NORMS}
    F = rf.lu_(dA.clone(), check=False)
    assert F.info == 0
    lu_host = F.factors.cpu().numpy()
    return A, F, lu_host, anorm, C.true_inverse_norms(C.factor_product(lu_host))


def first_step(F, n, norm, dtype):
    """sum |M ones| / n (1-norm) or sum |M^T ones| / n (Inf-norm) through ldiv_ with NotIPIV: shipped code on another route."""
    G = rf.LU(F.factors, rf.NotIPIV(n), 0)
    x = torch.ones(n, dtype=tdtype(dtype), device="cuda:0")
    rf.ldiv_(G if norm == C.NORM_ONE else rf.Adjoint(G), x)
    return math.fsum(np.abs(x.cpu().numpy().astype(np.float64))) / n


def rounding(n, dtype):
    """4 n eps_T: a substitution adds at most n terms per component, so gamma_n = n eps_T per triangle bounds its rounding relative to
    the moduli that are summed; two triangles, and as much again for the restatement, which the estimate is measured against.  No
    condition number enters: growth through cancellation is not allowed for, and a kernel that needs it fails here."""
    return 4.0 * n * float(np.finfo(dtype).eps)


def check_bars(est, restated, true, est1, what, n, dtype, est1_slack=1e-12):
    """tol: twice the relative gap between the restatement's estimate on the downloaded factors and the true norm of the inverse of
    their product, plus rounding(n, dtype) -- where the restatement hits the true norm exactly the gap is zero and alone would demand
    equal bits of two substitutions that add in different orders."""
    tol = 2.0 * abs(restated - true) / true + rounding(n, dtype)
    assert est <= true * (1.0 + tol), (what, "overestimate", est / true, tol)
    assert est >= true / 3.0, (what, "below a third", est / true)
    assert est >= est1 * (1.0 - est1_slack), (what, "below its own first step", est, est1)
    return est / true


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("n", C.GECON_SIZES)
def test_random_rcond_meets_the_bars(n, dtype):
    lo, hi = math.inf, 0.0
    for family in C.FAMILIES:
        A, F, lu_host, anorm, true = random_case(family, n, dtype)
        for norm in NORMS:
            assert anorm[norm] == pytest.approx(np.linalg.norm(A.astype(np.float64), NPORD[norm]), rel=n * EPS64)
            _, restated, _ = C.rcond_restatement(lu_host, norm, anorm[norm], dtype, detail=True)
            est1 = first_step(F, n, norm, dtype)
            rcs = {"cm": rf.rcond(F, anorm[norm], 1 if norm == C.NORM_ONE else "inf"),
                   "rm": gecon(lu_host, norm, anorm[norm], dtype, "rm"), "host": gecon(lu_host, norm, anorm[norm], dtype, "host")}
            assert rcs["cm"] == rcs["host"], (family, n, norm, rcs)          # the same kernels on the same layout
            for kind, rc in rcs.items():
                ratio = check_bars(1.0 / (rc * anorm[norm]), restated, true[norm], est1, (family, n, norm, kind), n, dtype)
                lo, hi = min(lo, ratio), max(hi, ratio)
    print(f"gecon n={n} {np.dtype(dtype).name}: est / true in [{lo:.4f}, {hi:.8f}], allowance {rounding(n, dtype):.2e}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_special_values_and_argument_rules(dtype):
    rng = np.random.default_rng(14)
    h, s = handle(), sfx(dtype)
    out = ctypes.c_double(-1.0)
    for n in (3, 65, 130):
        lu, _ = C.lapack_factors(rng.uniform(-1, 1, size=(n, n)).astype(dtype))
        for norm in NORMS:
            for kind in ("cm", "rm", "host"):
                Z = lu.copy(); Z[n // 2, n // 2] = 0
                assert gecon(Z, norm, 1.0, dtype, kind) == 0.0
                Z = lu.copy(); Z[n - 1, 0] = np.nan
                assert math.isnan(gecon(Z, norm, 1.0, dtype, kind))
                Z = lu.copy(); Z[0, n - 1] = np.nan
                assert math.isnan(gecon(Z, norm, 1.0, dtype, kind))
                Z = lu.copy(); Z[n // 2, n // 2] = np.nan
                assert math.isnan(gecon(Z, norm, 1.0, dtype, kind))
                Z = lu.copy(); Z[n // 2, n // 2] = 0; Z[n - 1, 0] = np.nan       # both: the zero u_ii decides (rflu.h)
                assert gecon(Z, norm, 1.0, dtype, kind) == 0.0
                if kind != "host":
                    assert gecon_batched([Z, lu], norm, [1.0, 1.0], dtype, kind == "rm")[0] == 0.0
                assert gecon(lu, norm, 0.0, dtype, kind) == 0.0
                assert math.isnan(gecon(lu, norm, math.nan, dtype, kind))
                with pytest.raises(_ffi.RfluError):
                    gecon(lu, norm, -1.0, dtype, kind)
            with pytest.raises(_ffi.RfluError):
                gecon(lu, 3, 1.0, dtype)
    t = torch.zeros(4, dtype=tdtype(dtype), device="cuda:0")
    for name in (f"rflu_gecon_{s}_dev", f"rflu_gecon_rm_{s}_dev"):
        h.call(name, 1, 0, ptr(t), 1, 1.0, ctypes.byref(out))
        assert out.value == 1.0                                               # n == 0
        with pytest.raises(_ffi.RfluError):
            h.call(name, 1, 2, ptr(t), 1, 1.0, ctypes.byref(out))             # lda < n
        with pytest.raises(_ffi.RfluError, match="exceeds"):
            h.call(name, 1, 65537, ptr(t), 65537, 1.0, ctypes.byref(out))     # the transposed chain's limit: refused before anything is read
    # overflow in the substitution: rcond = 0, not NaN
    tiny = np.diag(np.full(4, np.finfo(dtype).tiny, dtype=dtype)) + np.triu(np.full((4, 4), np.finfo(dtype).max / 2, dtype=dtype), 1)
    assert gecon(tiny, C.NORM_ONE, 1.0, dtype) == 0.0


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_determinism_and_the_shared_workspace(dtype):
    """gecon repeats itself bit for bit, and a solve and an inverse that follow it on the same handle equal those of a fresh handle."""
    n = 300
    A = C.random_matrix("uniform", n, C.pick_seed("uniform", n, dtype), dtype)
    dA = to_dev_cm(A)
    anorm = rf.opnorm(dA, 1)
    F = rf.lu_(dA.clone(), check=False)
    B = torch.from_numpy(np.ascontiguousarray(np.random.default_rng(3).uniform(-1, 1, size=(4, n)).astype(dtype))).to("cuda:0").T
    fresh = _ffi.Handle(0)
    try:
        x_fresh = rf.ldiv_(F, B.clone(), handle=fresh)
        inv_fresh = rf.inv(F, handle=fresh)
    finally:
        fresh.close()
    used = _ffi.Handle(0)
    try:
        first = [rf.rcond(F, anorm, p, handle=used) for p in (1, "inf")]
        for _ in range(3):
            assert [rf.rcond(F, anorm, p, handle=used) for p in (1, "inf")] == first
        assert torch.equal(rf.ldiv_(F, B.clone(), handle=used), x_fresh)
        assert rf.rcond(F, anorm, 1, handle=used) == first[0]
        assert torch.equal(rf.inv(F, handle=used), inv_fresh)
        G = rf.lu_(dA.clone(), check=False, handle=used)
        assert torch.equal(G.factors, F.factors) and torch.equal(G.ipiv, F.ipiv)
    finally:
        used.close()


# ---- 3. batched ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def batch_members(n, batch, dtype):
    """Exact members between random ones: (factors, anorm per norm, exact?, L U or None).  Every random member is a kept input
    (C.pick_seed: LAPACK's own estimate stays at or above half), each with a seed of its own."""
    exact = C.exact_cases(n)
    members = []
    next_seed = {f: 0 for f in C.FAMILIES}
    for b in range(batch):
        if b % 2 == 0:
            e = exact[(b // 2) % len(exact)]
            members.append((e.F, {norm: C.case_anorm(e, norm) for norm in NORMS}, True, None))
        else:
            family = C.FAMILIES[(b // 2) % 3]
            seed = C.pick_seed(family, n, dtype, next_seed[family])
            next_seed[family] = seed + 1
            lu, _ = C.lapack_factors(C.random_matrix(family, n, seed, dtype))
            LU = C.factor_product(lu)
            members.append((lu, {norm: float(np.linalg.norm(LU, NPORD[norm])) for norm in NORMS}, False, LU))
    return members


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("n", C.BATCHED_SIZES + [129])
def test_batched_rcond(n, dtype):
    """Batches of 67 / 7 / 1 (never a multiple of the groups per workgroup: an invalid group exists), both orientations; exact members
    by `==`, EVERY random member inside the three bars (the first step recomputed by substitution in the element type on the host,
    with the rounding allowance of the upper bar); n = 129 goes through the loop over the single entry."""
    lo, hi = math.inf, 0.0
    for batch in (C.BATCHES if n <= 128 else [7]):
        members = batch_members(n, batch, np.dtype(dtype).type)
        for norm in NORMS:
            anorms = [m[1][norm] for m in members]
            res = {rm: gecon_batched([m[0] for m in members], norm, anorms, dtype, rm) for rm in (False, True)}
            for b, (F, an, exact, LU) in enumerate(members):
                if exact:
                    want = C.rcond_restatement(F, norm, an[norm], dtype)
                    assert res[False][b] == want and res[True][b] == want, (n, batch, b, norm, res[False][b], res[True][b], want)
                    continue
                true = C.true_inverse_norm(LU, norm)
                _, restated, _ = C.rcond_restatement(F, norm, an[norm], dtype, detail=True)
                m_, mt_ = C.triangular_solvers(F, dtype)
                v = (m_ if norm == C.NORM_ONE else mt_)(np.ones(n, dtype=dtype))
                est1 = math.fsum(np.abs(v.astype(np.float64))) / n
                for rm in (False, True):
                    assert res[rm][b] > 0
                    r = check_bars(1.0 / (res[rm][b] * an[norm]), restated, true, est1, (n, batch, b, norm, rm), n, dtype,
                                   est1_slack=rounding(n, dtype))
                    lo, hi = min(lo, r), max(hi, r)
    print(f"gecon_batched n={n} {np.dtype(dtype).name}: est / true in [{lo:.4f}, {hi:.8f}], allowance {rounding(n, dtype):.2e}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("n", [3, 8, 31, 32])
def test_mixed_iteration_counts_in_one_workgroup(n, dtype):
    """Identity (converges at once), random, graded, singular, NaN and exact members in ADJACENT slots of one workgroup (four matrices
    per workgroup at n <= 32): the kernel returns, and the result of every member does not depend on its neighbours -- the reversed
    batch and every member alone give the same bits."""
    rng = np.random.default_rng(15)
    Fs, ans = [], []
    for k in range(11):
        kind = k % 6
        if kind == 0:
            F = np.eye(n)
        elif kind in (1, 2):
            F, _ = C.lapack_factors(C.random_matrix(C.FAMILIES[kind], n, k, dtype))
        elif kind == 3:
            F, _ = C.lapack_factors(rng.uniform(-1, 1, size=(n, n)).astype(dtype))
            F = F.copy(); F[n // 2, n // 2] = 0
        elif kind == 4:
            F, _ = C.lapack_factors(rng.uniform(-1, 1, size=(n, n)).astype(dtype))
            F = F.copy(); F[n - 1, 0] = np.nan
        else:
            F = C.exact_cases(n)[k % len(C.exact_cases(n))].F
        Fs.append(np.asarray(F, dtype=dtype))
        ans.append(1.0 + k)
    for norm in NORMS:
        for rm in (False, True):
            whole = gecon_batched(Fs, norm, ans, dtype, rm)
            rev = gecon_batched(Fs[::-1], norm, ans[::-1], dtype, rm)[::-1]
            for b in range(len(Fs)):
                alone = gecon_batched([Fs[b]], norm, [ans[b]], dtype, rm)[0]
                single = gecon(Fs[b], norm, ans[b], dtype, "rm" if rm else "cm")
                assert same(whole[b], rev[b]) and same(whole[b], alone), (n, norm, rm, b, whole[b], rev[b], alone)
                if b % 6 in (0, 3, 4, 5):          # exact arithmetic or a special value: the single entry agrees bit for bit
                    assert same(whole[b], single), (n, norm, rm, b, whole[b], single)
            assert whole[0] == 1.0 / (ans[0] * 1.0) and whole[3] == 0.0 and math.isnan(whole[4]) and whole[9] == 0.0 and math.isnan(whole[10])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_batched_special_values_and_argument_rules(dtype):
    h, s = handle(), sfx(dtype)
    n = 7
    lu, _ = C.lapack_factors(np.random.default_rng(16).uniform(-1, 1, size=(n, n)).astype(dtype))
    got = gecon_batched([lu] * 5, C.NORM_ONE, [1.0, 0.0, math.nan, -1.0, 2.0], dtype, False)
    assert got[0] > 0 and got[1] == 0.0 and math.isnan(got[2]) and math.isnan(got[3]) and got[4] == got[0] / 2
    t = torch.zeros(64, dtype=tdtype(dtype), device="cuda:0")
    an = torch.ones(4, dtype=torch.float64, device="cuda:0")
    out = torch.full((4,), -1.0, dtype=torch.float64, device="cuda:0")
    h.call(f"rflu_gecon_batched_{s}_dev", 1, 4, 0, ptr(t), 1, 1, 0, ptr(an), ptr(out))
    assert (out.cpu().numpy() == 1.0).all()                                              # n == 0
    h.call(f"rflu_gecon_batched_{s}_dev", 1, 0, 3, ptr(t), 3, 9, 0, ptr(an), ptr(out))   # batch == 0
    for args in ((3, 4, 3, ptr(t), 3, 9, 0, ptr(an), ptr(out)),                          # norm
                 (1, 4, 3, ptr(t), 2, 9, 0, ptr(an), ptr(out)),                          # lda < n
                 (1, 4, 3, ptr(t), 3, 8, 0, ptr(an), ptr(out)),                          # matrices overlap
                 (1, -1, 3, ptr(t), 3, 9, 0, ptr(an), ptr(out)),
                 (1, 4, 3, ptr(t), 3, 9, 0, ctypes.c_void_p(0), ptr(out))):
        with pytest.raises(_ffi.RfluError):
            h.call(f"rflu_gecon_batched_{s}_dev", *args)


# ---- 4. the Python functions -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_cond_opnorm_adjoint_and_batched_functions(dtype):
    for n in (5, 130):
        A = C.random_matrix("uniform", n, C.pick_seed("uniform", n, dtype), dtype)
        dA = to_dev_cm(A)
        before = dA.clone()
        lu_host = rf.lu(dA, check=False).factors.cpu().numpy()              # the factors cond computes inside (the schedule repeats itself)
        true = C.true_inverse_norms(C.factor_product(lu_host))
        for p, ord_ in ((1, 1), (math.inf, np.inf), ("inf", np.inf)):
            norm = C.NORM_ONE if p == 1 else C.NORM_INF
            ref = float(np.linalg.cond(A.astype(np.float64), ord_))
            got = rf.cond(dA, p)
            anorm = rf.opnorm(dA, p)
            _, restated, _ = C.rcond_restatement(lu_host, norm, anorm, dtype, detail=True)
            # the bars of the estimate: above, against the inverse of what the factors multiply to; below, a third of NumPy's value
            assert got <= anorm * true[norm] * (1 + 2 * abs(restated - true[norm]) / true[norm] + rounding(n, dtype)), (n, p, got, ref)
            assert got >= ref / 3, (n, p, got, ref)
            assert rf.cond(A, p) == pytest.approx(got, rel=1e-3)           # NumPy input: the host entries on the same matrix
            assert rf.opnorm(dA, p) == rf.opnorm(A, p) == rf.opnorm(rf.Adjoint(dA), 1 if p != 1 else math.inf)
            assert rf.opnorm(to_dev_rm(A), p) == pytest.approx(rf.opnorm(dA, p), rel=n * EPS64)   # another kernel, another order
        assert torch.equal(dA, before)
        F = rf.lu(dA, check=False)
        a1, ai = rf.opnorm(dA, 1), rf.opnorm(dA, math.inf)
        assert rf.rcond(rf.Adjoint(F), ai, 1) == rf.rcond(F, ai, math.inf)        # ||A^T||_1 = ||A||_inf
        assert rf.rcond(rf.Adjoint(F), a1, "inf") == rf.rcond(F, a1, 1)
    S = np.ones((4, 4), dtype=dtype)
    assert rf.cond(to_dev_cm(S), 1) == math.inf
    with pytest.raises(TypeError, match="complex"):
        rf.cond(torch.eye(3, dtype=torch.complex64, device="cuda:0"))
    with pytest.raises(TypeError, match="complex"):
        rf.opnorm_batched(torch.zeros((2, 3, 3), dtype=torch.complex128, device="cuda:0"))
    # batched functions: entry b is the single functions' value on matrix b
    batch, n = 7, 33
    seeds = []
    for b in range(batch):                                                 # kept inputs, each with a seed of its own
        seeds.append(C.pick_seed("graded", n, dtype, seeds[-1] + 1 if seeds else 0))
    host = np.stack([C.random_matrix("graded", n, sd, dtype) for sd in seeds])
    host[3] = 1.0                                                          # a singular member
    for t in (torch.from_numpy(host).to("cuda:0"), torch.from_numpy(np.ascontiguousarray(host.transpose(0, 2, 1))).to("cuda:0").transpose(1, 2)):
        for p in (1, math.inf):
            nb = rf.opnorm_batched(t, p).cpu().numpy()
            assert [rf.opnorm(t[b], p) for b in range(batch)] == list(nb)
            cb = rf.cond_batched(t, p).cpu().numpy()
            assert cb[3] == math.inf
            lus = rf.lu_batched(t, check=False).factors.cpu().numpy()      # the factors cond_batched computes inside
            norm = C.NORM_ONE if p == 1 else C.NORM_INF
            for b in (0, 1, 2, 4, 5, 6):
                ref = float(np.linalg.cond(host[b].astype(np.float64), 1 if p == 1 else np.inf))
                true = C.true_inverse_norm(C.factor_product(lus[b]), norm)
                _, restated, _ = C.rcond_restatement(lus[b], norm, nb[b], dtype, detail=True)
                assert cb[b] <= nb[b] * true * (1 + 2 * abs(restated - true) / true + rounding(n, dtype)), (b, p, cb[b], ref)
                assert cb[b] >= ref / 3, (b, p, cb[b], ref)
            assert torch.equal(rf.opnorm_batched(rf.Adjoint(t), p), rf.opnorm_batched(t, math.inf if p == 1 else 1))
