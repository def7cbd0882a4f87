"""The transposed solve (ldiv!(F', B)) through the layers that can be checked without a GPU: the six rflu_getrs_trans_* symbols in
include/rflu.h, their ctypes bindings, the exports of the built library, and the Julia glue (ccalls and ldiv! methods; the ccalls'
types are checked against the header by tests/test_julia_glue.py, which picks them up by itself)."""
import os
import re
import subprocess

import pytest

from recursivefactorization.jl_amd import _ffi
from test_julia_glue import JL_DIR, ROOT, c_prototypes, julia_ccalls

SYMBOLS = ["rflu_getrs_trans_f64", "rflu_getrs_trans_f32", "rflu_getrs_trans_f64_dev", "rflu_getrs_trans_f32_dev",
           "rflu_getrs_trans_rm_f64_dev", "rflu_getrs_trans_rm_f32_dev"]


def test_symbols_declared_and_bound_with_matching_arity():
    protos = c_prototypes()
    for sym in SYMBOLS:
        assert sym in protos, f"{sym} is not declared in include/rflu.h"
        assert sym in _ffi.EXPORTS, f"{sym} is not bound in _ffi.py"
        cret, cparams = protos[sym]
        res, args = _ffi.EXPORTS[sym]
        assert cret == "int" and res is _ffi.c_int
        assert len(args) == len(cparams) == 8
        # the argument list of the forward entry of the same shape
        fwd = sym.replace("_trans", "")
        assert protos[fwd] == protos[sym]
        assert _ffi.EXPORTS[fwd] == _ffi.EXPORTS[sym]
        for ct, at in zip(cparams, args):
            want = _ffi.c_i64 if ct == "int64_t" else _ffi.c_p
            assert at is want, (sym, ct, at)


def test_library_exports_the_symbols():
    if not os.path.exists(_ffi.LIB_PATH):
        pytest.skip("librflu.so has not been built")
    out = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for sym in SYMBOLS:
        assert sym in exported, sym


def test_python_ldiv_no_longer_refuses_the_adjoint():
    src = open(os.path.join(ROOT, "recursivefactorization.jl_amd", "lu.py")).read()
    assert "NotImplementedError" not in src
    for name in ("rflu_getrs_{trans}{sfx}_dev", "rflu_getrs_{trans}rm_{sfx}_dev", 'rflu_getrs_{trans}{sfx}"'):
        assert name in src, name


def test_julia_glue_calls_the_host_symbols():
    bound = {c[1] for c in julia_ccalls()}
    assert "rflu_getrs_trans_f64" in bound and "rflu_getrs_trans_f32" in bound
    src = open(os.path.join(JL_DIR, "src", "RFLUAMD.jl")).read()
    src = re.sub(r"#[^\n]*", "", src)
    assert len(re.findall(r"function getrs_trans!\(", src)) == 2
    # ldiv! methods for both wrappers of an LU, on the wrapper types of Julia 1.9 and of 1.10 on
    assert re.search(r"Adjoint\{T, <:LU\{T", src) and re.search(r"Transpose\{T, <:LU\{T", src)
    assert re.search(r"AdjointFactorization\{T, <:LU\{T", src) and re.search(r"TransposeFactorization\{T, <:LU\{T", src)
    m = re.search(r"function ldiv!\(Ft::Union\{(\w+)\{T\}, (\w+)\{T\}\}, B::StridedVecOrMat\{T\}\) where \{T <: GPUEltype\}(.*?)\nend\n", src, flags=re.S)
    assert m, "no ldiv! method for the wrapped factorization"
    assert "Adjoint" in m.group(1) and "Transpose" in m.group(2)
    body = m.group(3)
    for needle in ("GPU_MIN_N[]", "available()", "getrs_trans!(F.factors, p, B)", "GC.@preserve F B", "LinearAlgebra.ldiv!(Ft, B)"):
        assert needle in body, needle
