"""The mixed-precision solve (Float32 factors, Float64 iterative refinement) through the layers that can be checked without a GPU: the
three symbols in include/rflu.h with the argument lists the interface fixes, their ctypes bindings, the exports of the built library,
the Julia ccalls, the argument checks the Python mirror makes BEFORE it touches the library, and the cache state machine of
linsolve.RF32MixedLUFactorization with lu_mixed / ldiv_mixed replaced."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import recursivefactorization.jl_amd as rf
from recursivefactorization.jl_amd import _ffi
from recursivefactorization.jl_amd import linsolve as LS
from test_julia_glue import JL2C, ROOT, c_prototypes, julia_ccalls

ARGS = {
    "rflu_mixed_getrf_f64_dev": ["rflu_handle_t", "int64_t", "double*", "int64_t", "float*", "int64_t", "int64_t*", "int", "int64_t", "double*",
                                 "int64_t*"],
    "rflu_mixed_getrs_f64_dev": ["rflu_handle_t", "int64_t", "int64_t", "double*", "int64_t", "float*", "int64_t", "int64_t*", "double", "double*",
                                 "int64_t", "double*", "int64_t", "int", "int*"],
    "rflu_residual_f64_dev": ["rflu_handle_t", "int64_t", "int64_t", "double*", "int64_t", "double*", "int64_t", "double*", "int64_t", "double*",
                              "int64_t"],
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
    assert _ffi.load().rflu_version() >= 103   # needs no device


def test_tuning_variable_and_sources_are_wired():
    csrc = os.path.join(ROOT, "recursivefactorization.jl_amd", "csrc")
    assert "mixed.hip" in open(os.path.join(ROOT, "recursivefactorization.jl_amd", "build.py")).read()
    assert 'env_get("RFLU_MIXED_GEMV_MAX_RHS", mixed_gemv_max_rhs)' in open(os.path.join(csrc, "driver.cpp")).read()
    assert "RFLU_MIXED_GEMV_MAX_RHS" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    # reproducible from run to run: the kernels of the mixed path use no atomics
    code = re.sub(r"//[^\n]*", "", open(os.path.join(csrc, "mixed.hip")).read())
    assert "atomic" not in code


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
    for needle in ("function lu_mixed(", "function ldiv_mixed!(", "struct RF32MixedLUAMDFactorization"):
        assert needle in src, needle
    ext = open(os.path.join(ROOT, "julia", "RFLUAMD", "ext", "RFLUAMDLinearSolveExt.jl")).read()
    for needle in ("alg::RF32MixedLUAMDFactorization{P}", "RFLUAMD.lu_mixed(", "RFLUAMD.ldiv_mixed!(", "ReturnCode.Failure"):
        assert needle in ext, needle
    assert "lu_mixed" in open(os.path.join(ROOT, "julia", "RFLUAMD", "test", "runtests.jl")).read()


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


def _fake_cm(n, k, dtype=torch.float64):
    return _FakeCuda(torch.zeros(k, n, dtype=dtype).T)


def test_exports_of_the_package():
    for name in ("lu_mixed", "ldiv_mixed", "MixedLU", "NotConvergedError"):
        assert hasattr(rf, name) and name in rf.__all__
    assert "RF32MixedLUFactorization" in LS.__all__
    assert rf.NotConvergedError(-31).iters == -31


def test_lu_mixed_rejects_bad_arguments_before_the_library(no_library):
    with pytest.raises(TypeError):
        rf.lu_mixed(_fake_cm(8, 8, torch.float32))                    # the Float32 matrix goes to lu directly
    with pytest.raises(TypeError):
        rf.lu_mixed(np.zeros((8, 8), dtype=np.float32))
    with pytest.raises(ValueError):
        rf.lu_mixed(_fake_cm(8, 6))                                   # not square
    with pytest.raises(ValueError):
        rf.lu_mixed(np.zeros((6, 8)))
    with pytest.raises(ValueError):
        rf.lu_mixed(_FakeCuda(torch.zeros(8, dtype=torch.float64)))   # a vector
    with pytest.raises(ValueError):
        rf.lu_mixed(_FakeCuda(torch.zeros(8, 8, dtype=torch.float64)))   # row-major
    with pytest.raises(TypeError):
        rf.lu_mixed(_fake_cm(8, 8), pivot="yes")
    with pytest.raises(rf.RfluError):
        rf.lu_mixed(torch.zeros(8, 8, dtype=torch.float64).T)         # host tensor


def test_ldiv_mixed_rejects_bad_arguments_before_the_library(no_library):
    F = rf.MixedLU(_fake_cm(8, 8), _FakeCuda(torch.zeros(8, 8, dtype=torch.float32)), _FakeCuda(torch.zeros(8, dtype=torch.int64)), 0, 1.0)
    with pytest.raises(ValueError):
        rf.ldiv_mixed(F, _fake_cm(7, 2))                              # wrong number of rows
    with pytest.raises(ValueError):
        rf.ldiv_mixed(F, _FakeCuda(torch.zeros(7, dtype=torch.float64)))
    with pytest.raises(TypeError):
        rf.ldiv_mixed(F, _fake_cm(8, 2, torch.float32))
    with pytest.raises(TypeError):
        rf.ldiv_mixed(F, torch.zeros(2, 8, dtype=torch.float64).T)    # host tensor
    with pytest.raises(ValueError):
        rf.ldiv_mixed(F, _FakeCuda(torch.zeros(8, 2, dtype=torch.float64)))   # row-major right-hand sides
    with pytest.raises(TypeError):
        rf.ldiv_mixed(rf.LU(_fake_cm(8, 8), None, 0), _fake_cm(8, 2))
    # a zero pivot of the Float32 factorization and no fallback: raised before anything is launched
    G = rf.MixedLU(_fake_cm(8, 8), _FakeCuda(torch.zeros(8, 8, dtype=torch.float32)), _FakeCuda(torch.zeros(8, dtype=torch.int64)), 3, 1.0)
    with pytest.raises(rf.SingularException) as ei:
        rf.ldiv_mixed(G, _fake_cm(8, 2), fallback=False)
    assert ei.value.info == 3


def test_mixed_cache_state_machine(monkeypatch):
    """Fresh -> one lu_mixed; a new b reuses the factors; assigning A makes the cache fresh again; cache.A is never written; a singular
    Float64 fallback is ReturnCode.Failure, anything else Success."""
    calls = {"lu": 0, "ldiv": 0}

    def fake_lu_mixed(A, pivot=True, *, blocksize=None, handle=None):
        calls["lu"] += 1
        return rf.MixedLU(A, None, None, 0, float(np.abs(A).sum(axis=1).max()))

    def fake_ldiv_mixed(F, B, *, max_iter=30, fallback=True, handle=None):
        calls["ldiv"] += 1
        assert fallback and max_iter == 7
        if np.linalg.matrix_rank(F.A) < F.A.shape[0]:
            raise rf.SingularException(1)
        return np.linalg.solve(F.A, B)

    monkeypatch.setattr(LS, "lu_mixed", fake_lu_mixed)
    monkeypatch.setattr(LS, "ldiv_mixed", fake_ldiv_mixed)
    rng = np.random.default_rng(3)
    A = np.asfortranarray(rng.standard_normal((12, 12)) + 12 * np.eye(12))
    A_before = A.copy()
    b1, b2 = rng.standard_normal(12), rng.standard_normal(12)
    cache = LS.init(A, b1, LS.RF32MixedLUFactorization(max_iter=7))
    assert cache.isfresh and cache.nfactor == 0 and cache.cacheval is None
    sol = LS.solve_(cache)
    assert sol.retcode is LS.ReturnCode.Success and sol.u is cache.u and not cache.isfresh
    assert cache.nfactor == 1 and calls == {"lu": 1, "ldiv": 1}
    assert np.allclose(A @ sol.u, b1)
    cache.b = b2                                  # a new right-hand side does not make the cache fresh
    sol = LS.solve_(cache)
    assert sol.retcode is LS.ReturnCode.Success and cache.nfactor == 1 and calls == {"lu": 1, "ldiv": 2}
    assert np.allclose(A @ sol.u, b2)
    assert np.array_equal(A, A_before) and cache.A is A      # the matrix is only read
    A2 = np.asfortranarray(A + np.eye(12))
    cache.A = A2                                  # assigning A does
    assert cache.isfresh
    sol = LS.solve_(cache)
    assert sol.retcode is LS.ReturnCode.Success and cache.nfactor == 2 and np.allclose(A2 @ sol.u, b2)
    S = A.copy(order="F"); S[:, 4] = 0
    cache.A = S
    u_before = cache.u.copy()
    sol = LS.solve_(cache)
    assert sol.retcode is LS.ReturnCode.Failure and cache.nfactor == 3 and np.array_equal(cache.u, u_before)
