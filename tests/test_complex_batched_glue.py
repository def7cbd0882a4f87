"""The complex batched factorization and solve through the layers that can be checked without a GPU: the four
rflu_get{rf,rs}_batched_cf{64,32}_dev symbols in include/rflu.h, their ctypes bindings, the exports of the built library, the Julia
ccalls, the argument checks the Python mirror makes BEFORE it touches the library, the build list, the documents, and the structural
promise of csrc/batched_kernels.hpp and csrc/batched_complex.hip: matrices never wait for each other."""
import os
import re
import subprocess

import pytest
import torch

import recursivefactorization.jl_amd as rf
from recursivefactorization.jl_amd import _ffi, build
from test_julia_glue import JL2C, ROOT, c_prototypes, julia_ccalls

SYMBOLS = ["rflu_getrf_batched_cf64_dev", "rflu_getrf_batched_cf32_dev", "rflu_getrs_batched_cf64_dev", "rflu_getrs_batched_cf32_dev"]
GETRF = ["rflu_handle_t", "int64_t", "int64_t", "int64_t", "{T}*", "int64_t", "int64_t", "int", "int64_t*", "int64_t", "int", "int64_t*"]
GETRS = ["rflu_handle_t", "int64_t", "int64_t", "int64_t", "{T}*", "int64_t", "int64_t", "int", "int64_t*", "int64_t", "{T}*", "int64_t",
         "int64_t", "int"]
CSRC = os.path.join(ROOT, "recursivefactorization.jl_amd", "csrc")


def test_symbols_declared_and_bound():
    protos = c_prototypes()
    for sym in SYMBOLS:
        assert sym in protos, f"{sym} is not declared in include/rflu.h"
        assert sym in _ffi.EXPORTS, f"{sym} is not bound in _ffi.py"
        cret, cparams = protos[sym]
        T = "double" if "cf64" in sym else "float"
        want = [p.format(T=T) for p in (GETRF if "getrf" in sym else GETRS)]
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
    for sym in SYMBOLS:
        assert sym in exported, sym
    assert _ffi.load().rflu_version() >= 105   # needs no device


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
        R = "Float64" if "cf64" in sym else "Float32"
        assert any(f"reinterpret(Ptr{{{R}}}" in a for a in args), f"{sym}: the complex pointer is not reinterpreted to Ptr{{{R}}}"
    src = open(os.path.join(ROOT, "julia", "RFLUAMD", "src", "RFLUAMD.jl")).read()
    assert len(re.findall(r"function getrf_batched_dev!\(A::Ptr\{ComplexF(64|32)\}", src)) == 2
    assert len(re.findall(r"function getrs_batched_dev!\(F::Ptr\{ComplexF(64|32)\}", src)) == 2
    assert "ComplexF64, ComplexF32" in open(os.path.join(ROOT, "julia", "RFLUAMD", "test", "runtests.jl")).read()


def test_build_list_limits_and_documents():
    assert "batched_complex.hip" in build.SOURCES and "batched_kernels.hpp" in build.ALL_HEADERS
    assert sorted(build.EXTRA_DEPS["batched_complex.hip"]) == ["batched_kernels.hpp", "complex.hpp", "complex_dev.hpp"]
    assert build.EXTRA_DEPS["batched.hip"] == ["batched_kernels.hpp"]
    hdr = open(os.path.join(CSRC, "rflu_internal.hpp")).read()
    assert re.search(r"CBATCHED_MAX_DIM_CF32\s*=\s*128\b", hdr) and re.search(r"CBATCHED_MAX_DIM_CF64\s*=\s*64\b", hdr)
    assert "batched_attr_set[3][4]" in hdr   # one array of dynamic-LDS flags: [getrf | getrs | getri][f64, f32, cf64, cf32]
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "rflu_getrf_batched_cf64_dev" in open(os.path.join(ROOT, doc)).read(), doc
    api = open(os.path.join(ROOT, "include", "rflu.h")).read()
    assert "There is no batched / mixed / inverse form" not in api
    assert "column-major only" in api          # the row-major restriction above the limits is documented
    assert "4.7" in open(os.path.join(ROOT, "DESIGN.md")).read()


def test_the_real_batched_file_stays_real_only():
    """Geometry, wave maximum and launch are shared through batched_kernels.hpp; the complex element stays out of it and out of the real
    file, so that a change to complex_dev.hpp does not rebuild the real kernels."""
    for fn in ("batched.hip", "batched_kernels.hpp"):
        code = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, fn)).read())
        assert "Cx<" not in code, fn
        assert not any("complex" in inc for inc in re.findall(r'#include\s+["<]([^">]+)[">]', code)), fn


def test_complex_batched_kernels_wait_for_nobody():
    """As tests/test_batched_glue.py asks of the real elements: none of the project's helpers for waiting on another workgroup, no
    cooperative launch, no read-modify-write on shared words, no loop without a trip count -- in batched_kernels.hpp, which holds what the
    kernels share, and in batched_complex.hip, which holds the kernels of the complex elements."""
    mine = ("batched_kernels.hpp", "batched_complex.hip")
    codes = [re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, fn)).read()) for fn in mine]
    assert re.findall(r'#include\s+"([^"]+)"', codes[0]) == ["rflu_internal.hpp"]
    assert re.findall(r'#include\s+"([^"]+)"', codes[1]) == ["complex_dev.hpp", "batched_kernels.hpp"]
    code = "\n".join(codes)
    helpers = set()
    for fn in os.listdir(CSRC):
        if fn in mine or fn == "batched.hip" or not fn.endswith((".hip", ".hpp", ".cpp")):
            continue
        helpers |= set(re.findall(r"\b(\w*(?:poll|spin|gate_wait|lds_wait)\w*)\s*\(", open(os.path.join(CSRC, fn)).read(), flags=re.I))
    assert helpers, "the scan for the poll helpers found nothing: the pattern is stale"
    for name in sorted(helpers):
        assert not re.search(rf"\b{re.escape(name)}\s*\(", code), name
    for needle in ("SPIN_LIMIT", "s_sleep", "hipLaunchCooperativeKernel", "atomic", "AUX_SC1", "__builtin_amdgcn_raw_buffer", "while (", "while("):
        assert needle not in code, needle
    # one barrier per pivot column, for every element: each of the two factorization loops holds exactly one
    real = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "batched.hip")).read())
    for src, head, tail, last in ((real, "getrf_batched_kernel(BFactorArgs<T> a)", "struct BSolveArgs", "if (updprev && c == 0) s[r + (mn - 1) * ld] = lprev;"),
                                  (codes[1], "cgetrf_batched_kernel(CFactorArgs<R> a)", "struct CSolveArgs", "if (updprev && c == 0) S.put(r, mn - 1, lprev);")):
        body = src[src.index(head):src.index(tail)]
        loop = body[body.index("for (int k = 0; k < mn; ++k)"):body.index(last)]
        assert loop.count("__syncthreads()") == 2   # the one inside the loop and the one that closes the last step


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


def _fake(*shape, dtype=torch.complex128):
    return _FakeCuda(torch.zeros(*shape, dtype=dtype))


def test_exports_of_the_package():
    for name in ("lu_complex_batched_", "lu_complex_batched", "ldiv_complex_batched_"):
        assert hasattr(rf, name) and name in rf.__all__


def test_lu_complex_batched_rejects_bad_arguments_before_the_library(no_library):
    with pytest.raises(ValueError):
        rf.lu_complex_batched_(_fake(8, 8))                                   # 2-D
    with pytest.raises(ValueError):
        rf.lu_complex_batched_(_FakeCuda(torch.zeros(4, 16, 16, dtype=torch.complex128)[:, ::2, ::2]))   # no unit stride
    with pytest.raises(ValueError):
        rf.lu_complex_batched_(_FakeCuda(torch.zeros(8, 8, dtype=torch.complex64).expand(4, 8, 8)))      # overlapping matrices
    with pytest.raises(TypeError):
        rf.lu_complex_batched_(torch.zeros(4, 8, 8, dtype=torch.complex128))  # host tensor
    with pytest.raises(TypeError, match="lu_batched_"):
        rf.lu_complex_batched_(_fake(4, 8, 8, dtype=torch.float64))           # real batches have their own function
    A = _fake(4, 8, 6)
    with pytest.raises(ValueError):
        rf.lu_complex_batched_(A, _fake(4, 8, dtype=torch.int64))             # ipiv must be (batch, min(m, n))
    with pytest.raises(ValueError):
        rf.lu_complex_batched_(A, _fake(3, 6, dtype=torch.int64))
    with pytest.raises(TypeError):
        rf.lu_complex_batched_(A, _fake(4, 6, dtype=torch.int32))
    with pytest.raises(TypeError):
        rf.lu_complex_batched_(A, torch.zeros(4, 6, dtype=torch.int64))       # host ipiv
    with pytest.raises(TypeError):
        rf.lu_complex_batched_(A, None, pivot="yes")
    with pytest.raises(ValueError):
        rf.lu_complex_batched(_fake(8, 8))


def test_ldiv_complex_batched_rejects_bad_arguments_before_the_library(no_library):
    F = rf.BatchedLU(_fake(4, 8, 8), _fake(4, 8, dtype=torch.int64), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError):
        rf.ldiv_complex_batched_(F, _fake(4, 7))                              # wrong n
    with pytest.raises(ValueError):
        rf.ldiv_complex_batched_(F, _fake(3, 8, 2))                           # wrong batch
    with pytest.raises(ValueError):
        rf.ldiv_complex_batched_(F, _fake(8))                                 # 1-D
    with pytest.raises(TypeError):
        rf.ldiv_complex_batched_(F, _fake(4, 8, dtype=torch.complex64))
    with pytest.raises(TypeError):
        rf.ldiv_complex_batched_(F, torch.zeros(4, 8, dtype=torch.complex128))   # host right-hand sides
    with pytest.raises(ValueError):
        rf.ldiv_complex_batched_(F, _FakeCuda(torch.zeros(4, 3, 8, dtype=torch.complex128).transpose(1, 2)))   # column-major B, row-major factors
    with pytest.raises(ValueError):
        rf.ldiv_complex_batched_(rf.BatchedLU(_fake(4, 8, 6), _fake(4, 6, dtype=torch.int64), torch.zeros(4, dtype=torch.int64)), _fake(4, 8))
    with pytest.raises(TypeError):
        rf.ldiv_complex_batched_(rf.LU(_fake(8, 8), None, 0), _fake(4, 8))
    with pytest.raises(TypeError):                                            # real factors have their own function
        rf.ldiv_complex_batched_(rf.BatchedLU(_fake(4, 8, 8, dtype=torch.float64), _fake(4, 8, dtype=torch.int64),
                                              torch.zeros(4, dtype=torch.int64)), _fake(4, 8, dtype=torch.float64))
    with pytest.raises(TypeError):                                            # host pivots
        rf.ldiv_complex_batched_(rf.BatchedLU(_fake(4, 8, 8), torch.zeros(4, 8, dtype=torch.int64), torch.zeros(4, dtype=torch.int64)), _fake(4, 8))
    for bad in ("H", "n", True, 1, None):
        with pytest.raises(ValueError):
            rf.ldiv_complex_batched_(F, _fake(4, 8), trans=bad)
    with pytest.raises(TypeError):
        rf.ldiv_complex_batched_(rf.Adjoint(rf.Adjoint(F)), _fake(4, 8))      # doubly wrapped
    with pytest.raises(ValueError):
        rf.ldiv_complex_batched_(rf.Adjoint(F), _fake(4, 8), trans="T")       # the wrapper already says 'C'
    # a singular matrix is reported with its index before anything is launched
    G = rf.BatchedLU(_fake(4, 8, 8), _fake(4, 8, dtype=torch.int64), torch.tensor([0, 0, 3, 5]))
    with pytest.raises(rf.SingularException) as ei:
        rf.ldiv_complex_batched_(G, _fake(4, 8))
    assert ei.value.info == 3 and ei.value.batch_index == 2


def test_adjoint_wrapper_means_c(monkeypatch):
    """Adjoint(F) reaches the library as trans = 2 (LAPACK 'C'), 'T' as 1, 'N' as 0."""
    seen = []

    class _Recorder:
        def set_stream(self, *_):
            pass

        def call(self, name, *args):
            seen.append((name, args[-1]))

    monkeypatch.setattr(_ffi, "default_handle", lambda *a, **k: _Recorder())
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a, **k: type("S", (), {"cuda_stream": 0})())
    F = rf.BatchedLU(_fake(4, 8, 8), _fake(4, 8, dtype=torch.int64), torch.zeros(4, dtype=torch.int64))
    for arg, kw in ((F, {}), (F, {"trans": "T"}), (F, {"trans": "C"}), (rf.Adjoint(F), {})):
        rf.ldiv_complex_batched_(arg, _fake(4, 8), **kw)
    assert seen == [("rflu_getrs_batched_cf64_dev", 0), ("rflu_getrs_batched_cf64_dev", 1), ("rflu_getrs_batched_cf64_dev", 2),
                    ("rflu_getrs_batched_cf64_dev", 2)]


def test_existing_functions_keep_their_errors_and_name_the_new_ones(no_library):
    with pytest.raises(TypeError, match="lu_complex_batched_"):
        rf.lu_batched_(_fake(4, 8, 8))
    with pytest.raises(TypeError, match="ldiv_complex_batched_"):
        rf.ldiv_batched_(rf.BatchedLU(_fake(4, 8, 8), _fake(4, 8, dtype=torch.int64), torch.zeros(4, dtype=torch.int64)), _fake(4, 8))
    with pytest.raises(ValueError):
        rf.lu_complex_(_fake(4, 8, 8))                                        # the single-matrix function keeps refusing 3-D input
