"""The complex mixed-precision solve (ComplexF32 factors, ComplexF64 iterative refinement) through the layers that can be checked
without a GPU: the four symbols in include/rflu.h with the argument lists the interface fixes, their ctypes bindings, the exports of
the built library and its version, the Julia ccalls, and the argument checks the Python mirror makes BEFORE it touches the library."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import recursivefactorization.jl_amd as rf
from recursivefactorization.jl_amd import _ffi
from test_julia_glue import JL2C, ROOT, c_prototypes, julia_ccalls

ARGS = {
    "rflu_mixed_getrf_cf64_dev": ["rflu_handle_t", "int64_t", "double*", "int64_t", "float*", "int64_t", "int64_t*", "int", "double*", "int64_t*"],
    "rflu_mixed_getrs_cf64_dev": ["rflu_handle_t", "int64_t", "int64_t", "double*", "int64_t", "float*", "int64_t", "int64_t*", "double", "double*",
                                  "int64_t", "double*", "int64_t", "int", "int*"],
    "rflu_residual_cf64_dev": ["rflu_handle_t", "int64_t", "int64_t", "double*", "int64_t", "double*", "int64_t", "double*", "int64_t", "double*",
                               "int64_t"],
    "rflu_mixed_solve_cf32_dev": ["rflu_handle_t", "int64_t", "int64_t", "float*", "int64_t", "int64_t*", "float*", "int64_t"],
}


def test_symbols_declared_and_bound():
    protos = c_prototypes()
    for sym, want in ARGS.items():
        assert sym in protos, f"{sym} is not declared in include/rflu.h"
        assert sym in _ffi.EXPORTS, f"{sym} is not bound in _ffi.py"
        cret, cparams = protos[sym]
        assert cret == "int" and cparams == want, (sym, cparams)
        res, args = _ffi.EXPORTS[sym]
        assert res is _ffi.c_int and len(args) == len(cparams)
        for ct, at in zip(cparams, args):
            expect = {"int64_t": _ffi.c_i64, "int": _ffi.c_int, "double": _ffi.c_dbl}.get(ct, _ffi.c_p)
            assert at is expect, (sym, ct, at)


def test_library_exports_the_symbols_and_the_version():
    assert os.path.exists(_ffi.LIB_PATH), "librflu.so has not been built (build() comes first)"
    out = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for sym in ARGS:
        assert sym in exported, sym
    assert _ffi.load().rflu_version() >= 108   # needs no device


def test_sources_are_wired_and_use_no_atomics():
    csrc = os.path.join(ROOT, "recursivefactorization.jl_amd", "csrc")
    build = open(os.path.join(ROOT, "recursivefactorization.jl_amd", "build.py")).read()
    # the kernels of the real and of the complex refinement are one source: in SOURCES, and in EXTRA_DEPS with the complex headers
    assert '"mixed.hip", ' in build and '"mixed.hip": ["complex.hpp", "complex_dev.hpp"]' in build
    for name in ("mixed.hip", "complex_solve.hip"):
        code = re.sub(r"//[^\n]*", "", open(os.path.join(csrc, name)).read())
        assert "atomic" not in code, name                                                 # reproducible from run to run
    # cfma lives in the shared header, once
    assert "cfma(" in open(os.path.join(csrc, "complex_dev.hpp")).read()
    assert not re.search(r"__forceinline__ Cx<R> cfma\(", open(os.path.join(csrc, "complex_solve.hip")).read())
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "rflu_mixed_getrs_cf64_dev" in open(os.path.join(ROOT, doc)).read(), doc


def test_julia_ccalls_exist_and_match_the_header():
    protos = c_prototypes()
    calls = {c[1]: c for c in julia_ccalls() if c[1] in ARGS}
    assert sorted(calls) == sorted(ARGS)
    for sym, (fn, _, ret, types, args) in calls.items():
        cret, cparams = protos[sym]
        assert cret in JL2C[ret]
        assert len(types) == len(cparams) == len(args), sym
        for k, (jt, ct) in enumerate(zip(types, cparams)):
            assert ct in JL2C[jt], f"{sym}: argument {k + 1} is `{ct}` in rflu.h but `{jt}` in the ccall"
    src = open(os.path.join(ROOT, "julia", "RFLUAMD", "src", "RFLUAMD.jl")).read()
    for needle in ("function mixed_getrf_dev!(A::Ptr{ComplexF64}", "function mixed_getrs_dev!(A::Ptr{ComplexF64}", "mutable struct ComplexMixedLU",
                   "function lu_mixed(A::Ptr{ComplexF64}", "function ldiv_mixed!(X::Ptr{ComplexF64}",
                   # the real methods are still there
                   "function lu_mixed(A::Ptr{Float64}", "function ldiv_mixed!(X::Ptr{Float64}"):
        assert needle in src, needle


class _NoLibrary:
    """Stands in for the handle: any call into the library fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the library was touched ({name}) before the arguments were checked")


@pytest.fixture
def no_library(monkeypatch):
    monkeypatch.setattr(_ffi, "default_handle", lambda *a, **k: _NoLibrary())
    monkeypatch.setattr(_ffi, "load", lambda *a, **k: _NoLibrary())


class _FakeCuda(torch.Tensor):
    """A host tensor that says it lives on the GPU: the argument checks look at shapes, strides and dtypes only."""

    @staticmethod
    def __new__(cls, t):
        return torch.Tensor._make_subclass(cls, t)

    is_cuda = True
    __module__ = "torch"   # lu.py tells torch tensors from NumPy arrays by the module of their type


def _fake_cm(n, k, dtype=torch.complex128):
    return _FakeCuda(torch.zeros(k, n, dtype=dtype).T)


def test_exports_of_the_package():
    for name in ("lu_complex_mixed", "ldiv_complex_mixed", "lu_mixed", "ldiv_mixed", "MixedLU", "NotConvergedError"):
        assert hasattr(rf, name) and name in rf.__all__


def test_lu_complex_mixed_rejects_bad_arguments_before_the_library(no_library):
    with pytest.raises(TypeError):
        rf.lu_complex_mixed(_fake_cm(8, 8, torch.complex64))              # the ComplexF32 matrix goes to lu_complex directly
    with pytest.raises(TypeError, match="lu_mixed"):
        rf.lu_complex_mixed(_fake_cm(8, 8, torch.float64))                # a real matrix goes to lu_mixed
    with pytest.raises(TypeError):
        rf.lu_complex_mixed(np.zeros((8, 8), dtype=np.complex64))
    with pytest.raises(ValueError):
        rf.lu_complex_mixed(_fake_cm(8, 6))                               # not square
    with pytest.raises(ValueError):
        rf.lu_complex_mixed(np.zeros((6, 8), dtype=np.complex128))
    with pytest.raises(ValueError):
        rf.lu_complex_mixed(_FakeCuda(torch.zeros(8, dtype=torch.complex128)))        # a vector
    with pytest.raises(ValueError):
        rf.lu_complex_mixed(_FakeCuda(torch.zeros(8, 8, dtype=torch.complex128)))     # row-major
    with pytest.raises(TypeError):
        rf.lu_complex_mixed(_fake_cm(8, 8), pivot="yes")
    with pytest.raises(rf.RfluError):
        rf.lu_complex_mixed(torch.zeros(8, 8, dtype=torch.complex128).T)  # host tensor
    with pytest.raises(TypeError):
        rf.lu_complex_mixed(_fake_cm(8, 8), blocksize=64)                 # the complex path has no blocksize


def test_the_real_functions_keep_refusing_complex_input_and_name_the_new_ones(no_library):
    with pytest.raises(TypeError, match="lu_complex_mixed"):
        rf.lu_mixed(_fake_cm(8, 8))
    with pytest.raises(TypeError, match="lu_complex_mixed"):
        rf.lu_mixed(np.zeros((8, 8), dtype=np.complex128))
    F = rf.MixedLU(_fake_cm(8, 8), _FakeCuda(torch.zeros(8, 8, dtype=torch.complex64)), _FakeCuda(torch.zeros(8, dtype=torch.int64)), 0, 1.0)
    with pytest.raises(TypeError, match="ldiv_complex_mixed"):
        rf.ldiv_mixed(F, _fake_cm(8, 2))
    G = rf.MixedLU(_fake_cm(8, 8, torch.float64), _FakeCuda(torch.zeros(8, 8, dtype=torch.float32)), _FakeCuda(torch.zeros(8, dtype=torch.int64)), 0, 1.0)
    with pytest.raises(TypeError, match="ldiv_mixed"):
        rf.ldiv_complex_mixed(G, _fake_cm(8, 2, torch.float64))


def test_ldiv_complex_mixed_rejects_bad_arguments_before_the_library(no_library):
    F = rf.MixedLU(_fake_cm(8, 8), _FakeCuda(torch.zeros(8, 8, dtype=torch.complex64)), _FakeCuda(torch.zeros(8, dtype=torch.int64)), 0, 1.0)
    with pytest.raises(ValueError):
        rf.ldiv_complex_mixed(F, _fake_cm(7, 2))                          # wrong number of rows
    with pytest.raises(ValueError):
        rf.ldiv_complex_mixed(F, _FakeCuda(torch.zeros(7, dtype=torch.complex128)))
    with pytest.raises(TypeError):
        rf.ldiv_complex_mixed(F, _fake_cm(8, 2, torch.complex64))
    with pytest.raises(TypeError):
        rf.ldiv_complex_mixed(F, _fake_cm(8, 2, torch.float64))
    with pytest.raises(TypeError):
        rf.ldiv_complex_mixed(F, torch.zeros(2, 8, dtype=torch.complex128).T)         # host tensor
    with pytest.raises(ValueError):
        rf.ldiv_complex_mixed(F, _FakeCuda(torch.zeros(8, 2, dtype=torch.complex128)))   # row-major right-hand sides
    with pytest.raises(TypeError):
        rf.ldiv_complex_mixed(rf.LU(_fake_cm(8, 8), None, 0), _fake_cm(8, 2))
    # a zero pivot of the ComplexF32 factorization and no fallback: raised before anything is launched
    G = rf.MixedLU(_fake_cm(8, 8), _FakeCuda(torch.zeros(8, 8, dtype=torch.complex64)), _FakeCuda(torch.zeros(8, dtype=torch.int64)), 3, 1.0)
    with pytest.raises(rf.SingularException) as ei:
        rf.ldiv_complex_mixed(G, _fake_cm(8, 2), fallback=False)
    assert ei.value.info == 3
