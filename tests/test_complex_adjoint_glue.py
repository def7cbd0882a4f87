"""The complex transposed / adjoint solve through the layers that can be checked without a GPU: the CPU restatement the GPU tests lean on
(tests/complex_solve_ref.py) against every bar of tests/test_gpu_complex_adjoint.py, the four symbols in include/rflu.h with their
ctypes bindings and the library's exports, the argument rules of the Python mirror, and the text of the Julia glue."""
import os
import re
import subprocess

import numpy as np
import pytest

import complex_ref as CR
import complex_solve_ref as SR
import helpers
import recursivefactorization.jl_amd as rf
from recursivefactorization.jl_amd import _ffi
from test_julia_glue import JL2C, JL_DIR, ROOT, c_prototypes, julia_ccalls

CTYPES = [np.complex128, np.complex64]
H, I, PI = "rflu_handle_t", "int64_t", "int64_t*"
ARGS = {}
for _s, _t in (("cf64", "double*"), ("cf32", "float*")):
    ARGS[f"rflu_getrs_trans_{_s}"] = [H, I, I, _t, I, PI, _t, I, "int"]
    ARGS[f"rflu_getrs_trans_{_s}_dev"] = [H, I, I, _t, I, PI, _t, I, "int"]


# ---- the restatement against the bars of the GPU tests -----------------------------------------------------------------------------------
@pytest.mark.parametrize("ctype", CTYPES)
def test_restatement_meets_the_backward_error_bar(ctype):
    worst = 0.0
    for n in SR.BE_SIZES:
        A = SR.rand_input(n, ctype)
        F, ipiv = SR.rand_factors(n, ctype)
        E = SR.bar_E(n, ctype)
        for nrhs in SR.be_nrhs(n):
            B = CR.rand_rhs(n, nrhs, ctype)
            for conj in (0, 1):
                X = SR.trans_solve(F, ipiv, B, conj)
                assert X.dtype == ctype
                be = SR.backward_error(A, X, B, conj)
                worst = max(worst, be / E)
                assert be <= E, (n, nrhs, conj, be, E)
                # the other solve on the same input is wrong by O(1), far beyond the bar in either precision: a 'T' / 'C' mix-up cannot pass
                if n >= 50:
                    assert SR.backward_error(A, X, B, 1 - conj) > 10 * E
    print(f"{np.dtype(ctype).name}: restatement's worst backward error {worst:.4f} E")


@pytest.mark.parametrize("ctype", CTYPES)
def test_restatement_meets_the_reference_solve_check(ctype):
    """test/runtests.jl:21-28 with op(A): b = op(A)[:, end], solution ~ e_n, atol = 100 E."""
    worst = 0.0
    for n in helpers.REF_SIZES:
        A = SR.rand_input(n, ctype)
        F, ipiv = SR.rand_factors(n, ctype)
        E = SR.bar_E(n, ctype)
        e = np.zeros(n)
        e[-1] = 1
        for conj in (0, 1):
            b = np.ascontiguousarray(SR.op(A, conj)[:, -1]).astype(ctype)
            x = SR.trans_solve(F, ipiv, b, conj)
            if np.all(np.isfinite(x)):
                d = float(np.linalg.norm(x.astype(np.complex128) - e))
                worst = max(worst, d / (100 * E))
                assert d <= 100 * E, (n, conj, d)
    print(f"{np.dtype(ctype).name}: restatement's worst e_n distance {worst:.5f} of the bar")


@pytest.mark.parametrize("ctype", CTYPES)
def test_restatement_meets_the_notipiv_bar(ctype):
    """test/runtests.jl:116-128: NoPivot factors of A + 10 I, no pivot vector, ||op(A) X - B||_2 < 1000 n eps."""
    worst = 0.0
    for n in SR.NOPIV_SIZES:
        A = SR.nopivot_input(n, ctype)
        F, _, info = CR.complex_generic_lufact(A, False)
        assert info == 0
        bar = 1000 * n * SR.eps_of(ctype)
        for nrhs in SR.NOPIV_NRHS:
            B = SR.nopivot_rhs(n, nrhs, ctype)
            for conj in (0, 1):
                X = SR.trans_solve(F, None, B, conj)
                r = float(np.linalg.norm(SR.op(A, conj) @ X.astype(np.complex128) - B.astype(np.complex128)))
                worst = max(worst, r / bar)
                assert r < bar, (n, nrhs, conj, r, bar)
    print(f"{np.dtype(ctype).name}: restatement's worst NoPivot residual {worst:.5f} of the bar")


@pytest.mark.parametrize("ctype", CTYPES)
def test_restatement_is_exact_and_the_order_of_the_interchanges_matters(ctype):
    A = SR.exact_input(ctype)
    assert np.array_equal(A.astype(np.complex128), SR.exact_input(np.complex128))
    F, ipiv, info = CR.complex_generic_lufact(A, True)
    assert info == 0
    k = np.arange(SR.EXACT_N)
    moved = ipiv - 1 != k
    print(f"exact input: {int(moved.sum())} non-trivial interchanges, {len(set(ipiv[moved]))} distinct targets")
    assert moved.sum() == 129 and len(set(ipiv[moved])) == 37
    for nrhs in (3, 9):
        B = SR.exact_rhs(nrhs, ctype)
        out = {}
        for conj in (0, 1):
            X = SR.trans_solve(F, ipiv, B, conj)
            assert np.array_equal(X, SR.exact_solution(A, B, conj)), (nrhs, conj)
            assert not np.array_equal(SR.trans_solve(F, ipiv, B, conj, first_to_last=True), X)
            out[conj] = X
        assert not np.array_equal(out[0], out[1])


# ---- header, bindings, exports ------------------------------------------------------------------------------------------------------------
def test_symbols_declared_and_bound():
    assert len(ARGS) == 4
    protos = c_prototypes()
    for sym, want in ARGS.items():
        assert sym in protos, f"{sym} is not declared in include/rflu.h"
        assert sym in _ffi.EXPORTS, f"{sym} is not bound in _ffi.py"
        cret, cparams = protos[sym]
        assert cret == "int" and cparams == want, (sym, cparams)
        # the forward entry of the same shape plus the trailing `conj`
        assert protos[sym.replace("_trans", "")][1] == cparams[:-1]
        res, args = _ffi.EXPORTS[sym]
        assert res is _ffi.c_int and len(args) == len(cparams)
        for ct, at in zip(cparams, args):
            expect = {"int64_t": _ffi.c_i64, "int": _ffi.c_int}.get(ct, _ffi.c_p)
            assert at is expect, (sym, ct, at)
    header = open(os.path.join(ROOT, "include", "rflu.h")).read()
    assert "There is no complex ldiv!(F', B)" not in header


def test_library_exports_the_symbols():
    if not os.path.exists(_ffi.LIB_PATH):
        pytest.skip("librflu.so has not been built")
    out = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for sym in ARGS:
        assert sym in exported, sym


def test_source_is_wired_and_documented():
    from recursivefactorization.jl_amd import build as B

    assert "complex_solve.hip" in B.SOURCES and "complex_solve.hip" in B.EXTRA_DEPS
    assert "complex_dev.hpp" in B.ALL_HEADERS
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "rflu_getrs_trans_cf64" in text, doc
        assert "There is no complex ldiv!(F', B)" not in text and "no complex `ldiv!(F', B)`" not in text, doc


# ---- the Python mirror: every rule that needs no device -----------------------------------------------------------------------------------
@pytest.mark.parametrize("fn", ["ldiv_complex_adjoint_", "ldiv_complex_transpose_"])
def test_python_argument_rules_come_before_the_library(fn):
    solve = getattr(rf, fn)
    Z = np.asfortranarray(np.eye(4, dtype=np.complex128))
    F = rf.LU(Z, rf.NotIPIV(4), 0)
    z4 = np.zeros(4, dtype=np.complex128)
    with pytest.raises(TypeError):
        solve(F, np.zeros(4, dtype=np.complex64))                                              # wrong dtype
    with pytest.raises(TypeError):
        solve(F, np.zeros(4))
    with pytest.raises(TypeError):
        solve(rf.LU(np.asfortranarray(np.eye(4)), rf.NotIPIV(4), 0), np.zeros(4))              # real factors
    with pytest.raises(ValueError):
        solve(rf.LU(np.asfortranarray(np.zeros((4, 5), dtype=np.complex128)), rf.NotIPIV(4), 0), z4)   # non-square factors
    with pytest.raises(ValueError):
        solve(F, np.zeros(5, dtype=np.complex128))                                             # wrong row count
    with pytest.raises(TypeError):
        solve(F, np.zeros((4, 3), dtype=np.complex128))                                        # row-major right-hand side
    with pytest.raises(rf.SingularException):
        solve(rf.LU(Z, rf.NotIPIV(4), 3), z4)
    with pytest.raises(rf.SingularException):
        solve(rf.LU(Z, rf.NotIPIV(4), -3), z4)
    with pytest.raises(TypeError, match=fn):
        solve(rf.Adjoint(F), z4)
    with pytest.raises(TypeError, match=fn):
        solve(rf.Transpose(F), z4)
    # n == 0 and nrhs == 0 return B itself and need no device
    E = rf.LU(np.zeros((0, 0), dtype=np.complex64, order="F"), rf.NotIPIV(0), 0)
    b0 = np.zeros(0, dtype=np.complex64)
    assert solve(E, b0) is b0
    B0 = np.zeros((0, 3), dtype=np.complex64, order="F")
    assert solve(E, B0) is B0
    Bn = np.zeros((4, 0), dtype=np.complex128, order="F")
    assert solve(F, Bn) is Bn


def test_the_forward_function_still_refuses_the_wrapper_and_names_the_new_one():
    Z = np.asfortranarray(np.eye(4, dtype=np.complex128))
    F = rf.LU(Z, rf.NotIPIV(4), 0)
    with pytest.raises(TypeError, match="ldiv_complex_adjoint_"):
        rf.ldiv_complex_(rf.Adjoint(F), np.zeros(4, dtype=np.complex128))
    assert rf.Transpose is rf.Adjoint
    for fn in (rf.ldiv_complex_adjoint_, rf.ldiv_complex_transpose_):
        assert "Transpose is Adjoint" in fn.__doc__
    for name in ("ldiv_complex_adjoint_", "ldiv_complex_transpose_"):
        assert name in rf.__all__
    Bn = np.zeros((4, 0), dtype=np.complex128, order="F")
    assert rf.ldiv_complex_(F, Bn) is Bn


# ---- the Julia glue as text --------------------------------------------------------------------------------------------------------------
def test_julia_glue():
    protos = c_prototypes()
    need = {"rflu_getrs_trans_cf64", "rflu_getrs_trans_cf32"}
    calls = [c for c in julia_ccalls() if c[1] in need]
    assert {c[1] for c in calls} == need and len(calls) == 2
    for fn, sym, ret, types, args in calls:
        cret, cparams = protos[sym]
        assert cret in JL2C[ret]
        assert len(types) == len(cparams) == len(args) == 9, (sym, types, args)
        for jt, ct in zip(types, cparams):
            assert ct in JL2C[jt], (sym, jt, ct)
        assert types[-1] == "Cint" and args[-1].strip() == "Cint(conj)"
    src = open(os.path.join(JL_DIR, "src", "RFLUAMD.jl")).read()
    assert "stays with the stdlib)" not in src
    src = re.sub(r"#[^\n]*", "", src)
    assert "const GPUComplexEltype = Union{ComplexF32, ComplexF64}" in src
    assert len(re.findall(r"function getrs_ctrans!\(", src)) == 2
    assert len(re.findall(r"function getrs_trans!\(", src)) == 2
    assert re.search(r"function getrs_ctrans!\(F::StridedMatrix\{ComplexF64\}, ipiv::Ptr\{Int64\}, B::StridedVecOrMat\{ComplexF64\}, conj::Bool\)", src)
    assert re.search(r"function getrs_ctrans!\(F::StridedMatrix\{ComplexF32\}, ipiv::Ptr\{Int64\}, B::StridedVecOrMat\{ComplexF32\}, conj::Bool\)", src)
    for wrapper, flag in (("AdjointLU", "true"), ("TransposeLU", "false")):
        m = re.search(r"function ldiv!\(Ft::" + wrapper + r"\{T\}, B::StridedVecOrMat\{T\}\) where \{T <: GPUComplexEltype\}(.*?)\nend\n", src, flags=re.S)
        assert m, f"no complex ldiv! method for {wrapper}"
        body = m.group(1)
        for needle in ("GPU_MIN_N[]", "available()", f"getrs_ctrans!(F.factors, p, B, {flag})", "GC.@preserve F B", "LinearAlgebra.ldiv!(Ft, B)",
                       "stride(F.factors, 1) == 1 && stride(B, 1) == 1 && size(F.factors, 1) == size(F.factors, 2) == size(B, 1)"):
            assert needle in body, (wrapper, needle)
    # the real method is still there, untouched
    assert re.search(r"function ldiv!\(Ft::Union\{AdjointLU\{T\}, TransposeLU\{T\}\}, B::StridedVecOrMat\{T\}\) where \{T <: GPUEltype\}", src)
    assert "getrs_trans!(F.factors, p, B)" in src
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "getrs_ctrans!" in integration
