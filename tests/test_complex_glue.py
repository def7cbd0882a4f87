"""ComplexF64 / ComplexF32 lu! and ldiv! through the layers that can be checked without a GPU: the ten symbols in include/rflu.h, their
ctypes bindings, the exports of the built library, the Julia ccalls, the argument checks the Python mirror makes before it touches the
library -- and the CPU restatement (tests/complex_ref.py) that the GPU tests compare against, pinned on its own."""
import os
import subprocess

import numpy as np
import pytest

import complex_ref as CR
import recursivefactorization.jl_amd as rf
from recursivefactorization.jl_amd import _ffi
from test_julia_glue import JL2C, ROOT, c_prototypes, julia_ccalls

H, I, PI = "rflu_handle_t", "int64_t", "int64_t*"
ARGS = {}
for _s, _t in (("cf64", "double*"), ("cf32", "float*")):
    ARGS[f"rflu_getrf_{_s}"] = [H, I, I, _t, I, PI, "int", PI]
    ARGS[f"rflu_getrf_{_s}_dev"] = [H, I, I, _t, I, PI, "int", PI]
    ARGS[f"rflu_getrs_{_s}"] = [H, I, I, _t, I, PI, _t, I]
    ARGS[f"rflu_getrs_{_s}_dev"] = [H, I, I, _t, I, PI, _t, I]
    ARGS[f"rflu_gemm_rm_{_s}_dev"] = [H, I, I, I, _t, I, _t, I, _t, I]


def test_symbols_declared_and_bound():
    assert len(ARGS) == 10
    protos = c_prototypes()
    for sym, want in ARGS.items():
        assert sym in protos, f"{sym} is not declared in include/rflu.h"
        assert sym in _ffi.EXPORTS, f"{sym} is not bound in _ffi.py"
        cret, cparams = protos[sym]
        assert cret == "int" and cparams == want, (sym, cparams)
        res, args = _ffi.EXPORTS[sym]
        assert res is _ffi.c_int and len(args) == len(cparams)
        for ct, at in zip(cparams, args):
            expect = {"int64_t": _ffi.c_i64, "int": _ffi.c_int}.get(ct, _ffi.c_p)
            assert at is expect, (sym, ct, at)


def test_library_exports_the_symbols():
    assert os.path.exists(_ffi.LIB_PATH), "librflu.so has not been built (build() comes first)"
    out = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for sym in ARGS:
        assert sym in exported, sym


def test_sources_are_wired_and_documented():
    from recursivefactorization.jl_amd import build as B

    for src in ("complex_gemm.hip", "complex.hip"):
        assert src in B.SOURCES, src            # the source list is also what sources_digest() hashes
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "rflu_getrf_cf64" in text and "rflu_getrs_cf64" in text, doc


def test_julia_ccalls_exist_and_match_the_header():
    protos = c_prototypes()
    need = {s for s in ARGS if "gemm" not in s}   # the six getrf / getrs entries are what the package binds
    calls = [c for c in julia_ccalls() if c[1] in need]
    assert {c[1] for c in calls} == need
    for fn, sym, ret, types, args in calls:
        cret, cparams = protos[sym]
        assert cret in JL2C[ret]
        assert len(types) == len(cparams) == len(args), (sym, types, args)
        for jt, ct in zip(types, cparams):
            assert ct in JL2C[jt], (sym, jt, ct)
    src = open(os.path.join(ROOT, "julia", "RFLUAMD", "src", "RFLUAMD.jl")).read()
    # lu! / ldiv! dispatch on the element type: the complex types are in the GPU set, the real-only entries keep the real set
    assert "const GPUAnyEltype = Union{Float32, Float64, ComplexF32, ComplexF64}" in src
    assert "gpu_ok(A::StridedMatrix{<:GPUAnyEltype}, ipiv)" in src and "B::StridedVecOrMat{T}) where {T <: GPUAnyEltype}" in src
    assert "getrf!(A::StridedMatrix{ComplexF64}" in src and "getrs!(F::StridedMatrix{ComplexF32}" in src
    assert "reinterpret(Ptr{Float64}, pointer(A))" in src


def test_argument_checks_come_before_the_library():
    Z = np.asfortranarray(np.eye(4, dtype=np.complex128))
    for bad in (np.float64, np.float32, np.int64):
        with pytest.raises(TypeError):
            rf.lu_complex_(np.asfortranarray(np.eye(4, dtype=bad)))
        with pytest.raises(TypeError):
            rf.lu_complex(np.eye(4, dtype=bad))
    with pytest.raises(ValueError, match="column-major"):
        rf.lu_complex_(np.ascontiguousarray(np.arange(12, dtype=np.complex128).reshape(3, 4)))
    with pytest.raises(ValueError):
        rf.lu_complex_(np.zeros(4, dtype=np.complex64))
    with pytest.raises(TypeError):
        rf.lu_complex_(Z, np.zeros(4, dtype=np.int32))
    with pytest.raises(ValueError):
        rf.lu_complex_(Z, np.zeros(3, dtype=np.int64))
    with pytest.raises(ValueError):
        rf.lu_complex_([[1j]])          # (no ndim: "lu! needs a matrix", as lu_ answers)
    with pytest.raises(TypeError):
        rf.lu_complex_(Z, None, "rowmax")
    # lu / lu_ keep refusing complex input, and now say where it goes
    with pytest.raises(TypeError, match="lu_complex"):
        rf.lu(Z)
    with pytest.raises(TypeError, match="lu_complex"):
        rf.lu_(Z)
    # ldiv_complex_: the checks that need no device
    F = rf.LU(Z, rf.NotIPIV(4), 0)
    with pytest.raises(rf.SingularException):
        rf.ldiv_complex_(rf.LU(Z, rf.NotIPIV(4), 3), np.zeros(4, dtype=np.complex128))
    with pytest.raises(TypeError):
        rf.ldiv_complex_(rf.Adjoint(F), np.zeros(4, dtype=np.complex128))
    with pytest.raises(ValueError):
        rf.ldiv_complex_(F, np.zeros(5, dtype=np.complex128))
    with pytest.raises(TypeError):
        rf.ldiv_complex_(F, np.zeros(4, dtype=np.complex64))
    with pytest.raises(TypeError):
        rf.ldiv_complex_(rf.LU(np.asfortranarray(np.eye(4)), rf.NotIPIV(4), 0), np.zeros(4))
    with pytest.raises(ValueError):
        rf.ldiv_complex_(rf.LU(np.asfortranarray(np.zeros((4, 5), dtype=np.complex128)), rf.NotIPIV(4), 0), np.zeros(4, dtype=np.complex128))


def test_empty_matrices_need_no_device():
    for shape in ((0, 0), (0, 5), (5, 0)):
        F = rf.lu_complex_(np.zeros(shape, dtype=np.complex64, order="F"))
        assert F.info == 0 and len(F.ipiv) == 0 and F.issuccess()
    G = rf.lu_complex_(np.zeros((0, 3), dtype=np.complex128, order="F"), None, rf.NoPivot())
    assert isinstance(G.ipiv, rf.NotIPIV)


# ---- the restatement itself ----------------------------------------------------------------------------------------------------------
def test_restatement_info_against_scipy_on_a_zeroed_column():
    import scipy.linalg

    for m, n in ((10, 12), (130, 130)):
        for ctype in (np.complex128, np.complex64):
            A = CR.rand_complex(m, n, ctype)
            A[:, 4] = 0                                       # test/runtests.jl:56-66
            _, _, info = CR.complex_generic_lufact(A, True)
            with pytest.warns(Warning):
                lu, piv = scipy.linalg.lu_factor(A[:, :m], check_finite=False)
            zero = np.flatnonzero(np.diag(lu) == 0)
            assert info == 5 and zero.size and zero[0] + 1 == info
            _, _, info_np = CR.complex_generic_lufact(A, False)
            assert info_np == 5


@pytest.mark.parametrize("ctype", [np.complex128, np.complex64])
def test_restatement_meets_the_reference_bar(ctype):
    eps = np.finfo(CR.real_of(ctype)).eps
    worst = {True: 0.0, False: 0.0}
    for m, n in CR.REF_SHAPES:
        A = CR.rand_complex(m, n, ctype)
        E = 20 * m * eps                                      # test/runtests.jl:21-31
        for pivot, bar in ((True, E), (False, 10 * np.sqrt(E))):
            F, ipiv, info = CR.complex_generic_lufact(A, pivot)
            assert info == 0
            r = CR.residual_inf(A, F, ipiv)
            worst[pivot] = max(worst[pivot], r / bar)
            assert r < bar, (m, n, pivot, r, bar)
    print(f"{np.dtype(ctype).name}: restatement at most {worst[True]:.3f} E pivoted, {worst[False]:.4f} of the NoPivot bar")


def test_restatement_is_exact_on_the_exact_inputs():
    for (m, n, empty), want in zip(CR.EXACT_CASES, CR.EXACT_INFO):
        A64 = CR.exact_complex(m, n, empty, np.complex128)
        A32 = CR.exact_complex(m, n, empty, np.complex64)
        assert np.array_equal(A32.astype(np.complex128), A64)
        F64, p64, i64 = CR.complex_generic_lufact(A64, True)
        F32, p32, i32 = CR.complex_generic_lufact(A32, True)
        assert i64 == i32 == want, (m, n, i64, i32)
        assert np.array_equal(p64, p32)
        assert F32.dtype == np.complex64
        assert np.array_equal(CR.bits(F32.astype(np.complex128)), CR.bits(F64)), (m, n)     # identical bits, signed zeros included
        # ties really occur and go to the lowest current row: L*U reproduces the permuted input exactly
        assert CR.residual_inf(A64, F64, p64) == 0.0 or want != 0
