"""The batched factorization and solve through the layers that can be checked without a GPU: the four rflu_get{rf,rs}_batched_*
symbols in include/rflu.h, their ctypes bindings, the exports of the built library, the Julia ccalls, the argument checks the Python
mirror makes BEFORE it touches the library, and the one structural promise of csrc/batched.hip: matrices never wait for each other."""
import os
import re
import subprocess

import pytest
import torch

import recursivefactorization.jl_amd as rf
from recursivefactorization.jl_amd import _ffi
from test_julia_glue import JL2C, ROOT, c_prototypes, julia_ccalls

SYMBOLS = ["rflu_getrf_batched_f64_dev", "rflu_getrf_batched_f32_dev", "rflu_getrs_batched_f64_dev", "rflu_getrs_batched_f32_dev"]
# the argument lists the issue fixes (strided, no arrays of pointers)
GETRF = ["rflu_handle_t", "int64_t", "int64_t", "int64_t", "{T}*", "int64_t", "int64_t", "int", "int64_t*", "int64_t", "int", "int64_t*"]
GETRS = ["rflu_handle_t", "int64_t", "int64_t", "int64_t", "{T}*", "int64_t", "int64_t", "int", "int64_t*", "int64_t", "{T}*", "int64_t",
         "int64_t", "int"]


def test_symbols_declared_and_bound():
    protos = c_prototypes()
    for sym in SYMBOLS:
        assert sym in protos, f"{sym} is not declared in include/rflu.h"
        assert sym in _ffi.EXPORTS, f"{sym} is not bound in _ffi.py"
        cret, cparams = protos[sym]
        T = "double" if "f64" in sym else "float"
        want = [p.format(T=T) for p in (GETRF if "getrf" in sym else GETRS)]
        assert cret == "int" and cparams == want, (sym, cparams)
        res, args = _ffi.EXPORTS[sym]
        assert res is _ffi.c_int and len(args) == len(cparams)
        for ct, at in zip(cparams, args):
            expect = {"int64_t": _ffi.c_i64, "int": _ffi.c_int}.get(ct, _ffi.c_p)
            assert at is expect, (sym, ct, at)


def test_path_enum_and_version_in_the_header():
    src = open(os.path.join(ROOT, "include", "rflu.h")).read()
    assert re.search(r"RFLU_PATH_HIP_BATCHED\s*=\s*5\b", src)
    assert _ffi.PATH_HIP_BATCHED == 5
    drv = open(os.path.join(ROOT, "recursivefactorization.jl_amd", "csrc", "driver.cpp")).read()
    m = re.search(r"int rflu_version\(void\) \{ return (\d+); \}", drv)
    assert m and int(m.group(1)) >= 102


def test_library_exports_the_symbols_and_the_version():
    assert os.path.exists(_ffi.LIB_PATH), "librflu.so has not been built (build() comes first)"
    out = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for sym in SYMBOLS:
        assert sym in exported, sym
    assert _ffi.load().rflu_version() >= 102   # needs no device


def test_julia_ccalls_exist_and_match_the_header():
    protos = c_prototypes()
    calls = {c[1]: c for c in julia_ccalls() if c[1] in SYMBOLS}
    assert sorted(calls) == sorted(SYMBOLS)
    for sym, (fn, _, ret, types, args) in calls.items():
        cret, cparams = protos[sym]
        assert cret in JL2C[ret]
        assert len(types) == len(cparams) == len(args), sym
        for k, (jt, ct) in enumerate(zip(types, cparams)):
            assert ct in JL2C[jt], f"{sym}: argument {k + 1} is `{ct}` in rflu.h but `{jt}` in the ccall"
    src = open(os.path.join(ROOT, "julia", "RFLUAMD", "src", "RFLUAMD.jl")).read()
    assert len(re.findall(r"function getrf_batched_dev!\(A::Ptr\{Float(64|32)\}", src)) == 2
    assert len(re.findall(r"function getrs_batched_dev!\(F::Ptr\{Float(64|32)\}", src)) == 2
    assert "getrf_batched_dev!" in open(os.path.join(ROOT, "julia", "RFLUAMD", "test", "runtests.jl")).read()


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


def _fake(*shape, dtype=torch.float64):
    return _FakeCuda(torch.zeros(*shape, dtype=dtype))


def test_exports_of_the_package():
    for name in ("lu_batched_", "lu_batched", "ldiv_batched_", "BatchedLU"):
        assert hasattr(rf, name) and name in rf.__all__
    assert "hip-batched" in open(os.path.join(ROOT, "recursivefactorization.jl_amd", "lu.py")).read()
    e = rf.SingularException(5, 17)
    assert e.info == 5 and e.batch_index == 17 and rf.SingularException(3).batch_index is None


def test_lu_batched_rejects_bad_arguments_before_the_library(no_library):
    with pytest.raises(ValueError):
        rf.lu_batched_(_fake(8, 8))                                   # 2-D
    with pytest.raises(ValueError):
        rf.lu_batched_(_FakeCuda(torch.zeros(4, 16, 16, dtype=torch.float64)[:, ::2, ::2]))   # no unit stride
    with pytest.raises(ValueError):
        rf.lu_batched_(_FakeCuda(torch.zeros(8, 8, dtype=torch.float64).expand(4, 8, 8)))     # overlapping matrices
    with pytest.raises(TypeError):
        rf.lu_batched_(torch.zeros(4, 8, 8, dtype=torch.float64))     # host tensor
    with pytest.raises(TypeError):
        rf.lu_batched_(_fake(4, 8, 8, dtype=torch.float16))
    A = _fake(4, 8, 6)
    with pytest.raises(ValueError):
        rf.lu_batched_(A, _fake(4, 8, dtype=torch.int64))             # ipiv must be (batch, min(m, n))
    with pytest.raises(ValueError):
        rf.lu_batched_(A, _fake(3, 6, dtype=torch.int64))
    with pytest.raises(TypeError):
        rf.lu_batched_(A, _fake(4, 6, dtype=torch.int32))
    with pytest.raises(TypeError):
        rf.lu_batched_(A, torch.zeros(4, 6, dtype=torch.int64))       # host ipiv
    with pytest.raises(TypeError):
        rf.lu_batched_(A, None, pivot="yes")


def test_ldiv_batched_rejects_bad_arguments_before_the_library(no_library):
    F = rf.BatchedLU(_fake(4, 8, 8), _fake(4, 8, dtype=torch.int64), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError):
        rf.ldiv_batched_(F, _fake(4, 7))                              # wrong n
    with pytest.raises(ValueError):
        rf.ldiv_batched_(F, _fake(3, 8, 2))                           # wrong batch
    with pytest.raises(ValueError):
        rf.ldiv_batched_(F, _fake(8))                                 # 1-D
    with pytest.raises(TypeError):
        rf.ldiv_batched_(F, _fake(4, 8, dtype=torch.float32))
    with pytest.raises(TypeError):
        rf.ldiv_batched_(F, torch.zeros(4, 8, dtype=torch.float64))   # host right-hand sides
    with pytest.raises(ValueError):
        rf.ldiv_batched_(F, _FakeCuda(torch.zeros(4, 3, 8, dtype=torch.float64).transpose(1, 2)))   # column-major B, row-major factors
    with pytest.raises(ValueError):
        rf.ldiv_batched_(rf.BatchedLU(_fake(4, 8, 6), _fake(4, 6, dtype=torch.int64), torch.zeros(4, dtype=torch.int64)), _fake(4, 8))
    with pytest.raises(TypeError):
        rf.ldiv_batched_(rf.LU(_fake(8, 8), None, 0), _fake(4, 8))
    # a singular matrix is reported with its index before anything is launched
    G = rf.BatchedLU(_fake(4, 8, 8), _fake(4, 8, dtype=torch.int64), torch.tensor([0, 0, 3, 5]))
    with pytest.raises(rf.SingularException) as ei:
        rf.ldiv_batched_(G, _fake(4, 8))
    assert ei.value.info == 3 and ei.value.batch_index == 2


def test_batched_kernels_wait_for_nobody():
    """The matrices of a batch are independent and must stay so: csrc/batched_kernels.hpp, which holds what the kernels share, and
    csrc/batched.hip, which holds the kernels of the real elements, use none of the project's polling helpers, no cooperative launch, no atomics, no
    cache-bypassing exchange loads, no sleep -- and do not include the headers that carry them."""
    csrc = os.path.join(ROOT, "recursivefactorization.jl_amd", "csrc")
    mine = ("batched_kernels.hpp", "batched.hip")
    codes = [re.sub(r"//[^\n]*", "", open(os.path.join(csrc, fn)).read()) for fn in mine]
    assert re.findall(r'#include\s+"([^"]+)"', codes[0]) == ["rflu_internal.hpp"]
    assert re.findall(r'#include\s+"([^"]+)"', codes[1]) == ["batched_kernels.hpp"]
    code = "\n".join(codes)
    # the project's own helpers and idioms for waiting on another workgroup (panel*.hip, trsv.hip, laswp.hip, engine.hip)
    helpers = set()
    for fn in os.listdir(csrc):
        if fn in mine or fn == "batched_complex.hip" or not fn.endswith((".hip", ".hpp", ".cpp")):
            continue
        src = open(os.path.join(csrc, fn)).read()
        helpers |= set(re.findall(r"\b(\w*(?:poll|spin|gate_wait|lds_wait)\w*)\s*\(", src, flags=re.I))
    assert helpers, "the scan for the poll helpers found nothing: the pattern is stale"
    for name in sorted(helpers):
        assert not re.search(rf"\b{re.escape(name)}\s*\(", code), name
    for needle in ("SPIN_LIMIT", "s_sleep", "hipLaunchCooperativeKernel", "atomic", "AUX_SC1", "__builtin_amdgcn_raw_buffer", "while (", "while("):
        assert needle not in code, needle
    build = open(os.path.join(ROOT, "recursivefactorization.jl_amd", "build.py")).read()
    assert "batched.hip" in build and "batched_kernels.hpp" in build
