"""inv / det / logabsdet from the LU factors through the layers that can be checked without a GPU: the 14 symbols in include/rflu.h with
the argument lists the interface fixes, their ctypes bindings, the exports of the built library, the Julia ccalls, and the argument
checks the Python mirror makes BEFORE it touches the library."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import recursivefactorization.jl_amd as rf
from recursivefactorization.jl_amd import _ffi
from test_julia_glue import JL2C, ROOT, c_prototypes, julia_ccalls

H, I, PI, PD = "rflu_handle_t", "int64_t", "int64_t*", "double*"
ARGS = {}
for _s, _t in (("f64", "double*"), ("f32", "float*")):
    ARGS[f"rflu_logabsdet_{_s}_dev"] = [H, I, _t, I, PI, PD, PD]
    ARGS[f"rflu_logabsdet_{_s}"] = [H, I, _t, I, PI, PD, PD]
    ARGS[f"rflu_logabsdet_batched_{_s}_dev"] = [H, I, I, _t, I, I, PI, I, PD, PD]
    ARGS[f"rflu_getri_{_s}_dev"] = [H, I, _t, I, PI, PI]
    ARGS[f"rflu_getri_rm_{_s}_dev"] = [H, I, _t, I, PI, PI]
    ARGS[f"rflu_getri_{_s}"] = [H, I, _t, I, PI, PI]
    ARGS[f"rflu_getri_batched_{_s}_dev"] = [H, I, I, _t, I, I, "int", PI, I, _t, I, I, PI]


def test_symbols_declared_and_bound():
    assert len(ARGS) == 14
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
    assert _ffi.load().rflu_version() >= 104   # needs no device


def test_source_is_wired_and_uses_no_read_modify_write_primitives():
    pkg = os.path.join(ROOT, "recursivefactorization.jl_amd")
    assert '"inverse.hip"' in open(os.path.join(pkg, "build.py")).read()
    from recursivefactorization.jl_amd import build as B

    assert "inverse.hip" in B.SOURCES            # the source list is also what sources_digest() hashes
    code = re.sub(r"//[^\n]*", "", open(os.path.join(pkg, "csrc", "inverse.hip")).read())
    assert "atomic" not in code
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "rflu_getri" in open(os.path.join(ROOT, doc)).read(), doc


def test_julia_ccalls_exist_and_match_the_header():
    protos = c_prototypes()
    calls = [c for c in julia_ccalls() if c[1] in ARGS]
    assert sorted({c[1] for c in calls}) == sorted(ARGS)
    for fn, sym, ret, types, args in calls:
        cret, cparams = protos[sym]
        assert cret in JL2C[ret]
        assert len(types) == len(cparams) == len(args), sym
        for k, (jt, ct) in enumerate(zip(types, cparams)):
            assert ct in JL2C[jt], f"{sym}: argument {k + 1} is `{ct}` in rflu.h but `{jt}` in the ccall"
    src = open(os.path.join(ROOT, "julia", "RFLUAMD", "src", "RFLUAMD.jl")).read()
    for needle in ("function getri!(", "function getri_dev!(", "function logabsdet_dev(", "function getri_batched_dev!(",
                   "function logabsdet_batched_dev!(", "LinearAlgebra.inv!(", "LinearAlgebra.det(", "LinearAlgebra.logabsdet("):
        assert needle in src, needle
    tests = open(os.path.join(ROOT, "julia", "RFLUAMD", "test", "runtests.jl")).read()
    assert "inv!" in tests and "logabsdet" in tests


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


def _fake_cm(m, n, dtype=torch.float64):
    return _FakeCuda(torch.zeros(n, m, dtype=dtype).T)


def _fake_ipiv(n):
    return _FakeCuda(torch.zeros(n, dtype=torch.int64))


def test_exports_of_the_package():
    for name in ("inv", "inv_", "det", "logabsdet", "logdet", "inv_batched", "logabsdet_batched", "det_batched"):
        assert hasattr(rf, name) and name in rf.__all__, name


SINGLE = [rf.inv_, rf.inv, rf.logabsdet, rf.det, rf.logdet]


@pytest.mark.parametrize("fn", SINGLE)
def test_single_matrix_entries_reject_bad_arguments_before_the_library(fn, no_library):
    with pytest.raises(ValueError):
        fn(rf.LU(_fake_cm(8, 6), _fake_ipiv(6), 0))                           # not square
    with pytest.raises(ValueError):
        fn(rf.LU(np.zeros((6, 8), order="F"), np.arange(1, 7), 0))
    with pytest.raises(TypeError):
        fn(rf.LU(_fake_cm(8, 8, torch.float16), _fake_ipiv(8), 0))            # wrong element type
    with pytest.raises(TypeError):
        fn(rf.LU(np.zeros((8, 8), dtype=np.int32, order="F"), np.arange(1, 9), 0))
    with pytest.raises(ValueError):
        fn(rf.LU(_FakeCuda(torch.zeros(8, 16, dtype=torch.float64)[:, ::2]), _fake_ipiv(8), 0))   # unit stride in no dimension
    with pytest.raises(ValueError):
        fn(rf.LU(np.zeros((8, 8), order="C"), np.arange(1, 9), 0))            # host factors are column-major
    with pytest.raises(TypeError):
        fn(rf.LU(_fake_cm(8, 8), np.arange(1, 9), 0))                         # GPU factors, host pivots
    with pytest.raises(TypeError):
        fn(rf.Adjoint(rf.Adjoint(rf.LU(_fake_cm(8, 8), _fake_ipiv(8), 0))))   # doubly wrapped
    with pytest.raises(TypeError):
        fn(_fake_cm(8, 8))                                                    # not a factorization
    with pytest.raises(rf.RfluError):
        fn(rf.LU(torch.zeros(8, 8, dtype=torch.float64).T, _fake_ipiv(8), 0))   # host tensor


@pytest.mark.parametrize("fn", [rf.inv_, rf.inv])
def test_inverse_of_a_singular_factorization_raises_before_the_library(fn, no_library):
    for F in (rf.LU(_fake_cm(8, 8), _fake_ipiv(8), 3), rf.LU(np.zeros((8, 8), order="F"), np.arange(1, 9), 3),
              rf.Adjoint(rf.LU(_fake_cm(8, 8), rf.NotIPIV(8), -3))):
        with pytest.raises(rf.SingularException) as ei:
            fn(F)
        assert ei.value.info == 3


def test_empty_matrix_needs_no_library(no_library):
    F = rf.LU(np.zeros((0, 0), order="F"), np.zeros(0, dtype=np.int64), 0)
    assert rf.logabsdet(F) == (0.0, 1.0) and rf.det(F) == 1.0 and rf.logdet(F) == 0.0
    assert rf.inv(F).shape == (0, 0)
    X = rf.inv_(F)
    assert X.shape == (0, 0) and F.factors is None
    with pytest.raises(ValueError):
        rf.logabsdet(F)                                                       # invalid after inv_


def test_logdet_of_a_negative_determinant(monkeypatch):
    import importlib

    L = importlib.import_module("recursivefactorization.jl_amd.lu")

    monkeypatch.setattr(L, "logabsdet", lambda F, handle=None: (1.5, -1.0))
    with pytest.raises(ValueError):
        rf.logdet(None)
    assert rf.det(None) == -np.exp(1.5)
    monkeypatch.setattr(L, "logabsdet", lambda F, handle=None: (-np.inf, 0.0))
    assert rf.det(None) == 0.0 and rf.logdet(None) == -np.inf


@pytest.mark.parametrize("fn", [rf.inv_batched, rf.logabsdet_batched, rf.det_batched])
def test_batched_entries_reject_bad_arguments_before_the_library(fn, no_library):
    info = _FakeCuda(torch.zeros(4, dtype=torch.int64))
    ipiv = _FakeCuda(torch.zeros(4, 8, dtype=torch.int64))
    with pytest.raises(ValueError):
        fn(rf.BatchedLU(_FakeCuda(torch.zeros(4, 8, 6, dtype=torch.float64)), ipiv, info))        # not square
    with pytest.raises(TypeError):
        fn(rf.BatchedLU(_FakeCuda(torch.zeros(4, 8, 8, dtype=torch.float16)), ipiv, info))
    with pytest.raises(ValueError):
        fn(rf.BatchedLU(_FakeCuda(torch.zeros(4, 16, 16, dtype=torch.float64)[:, ::2, ::2]), ipiv, info))
    with pytest.raises(TypeError):
        fn(rf.LU(_fake_cm(8, 8), _fake_ipiv(8), 0))                                                # not a batch
    with pytest.raises(TypeError):
        fn(rf.Adjoint(rf.Adjoint(rf.BatchedLU(_FakeCuda(torch.zeros(4, 8, 8, dtype=torch.float64)), ipiv, info))))
    bad = _FakeCuda(torch.tensor([0, 0, 5, 0], dtype=torch.int64))
    if fn is rf.inv_batched:
        with pytest.raises(rf.SingularException) as ei:
            fn(rf.BatchedLU(_FakeCuda(torch.zeros(4, 8, 8, dtype=torch.float64)), ipiv, bad))
        assert ei.value.info == 5 and ei.value.batch_index == 2
