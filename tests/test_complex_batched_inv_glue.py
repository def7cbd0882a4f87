"""The complex batched inverse through the layers that can be checked without a GPU: the two rflu_getri_batched_cf{64,32}_dev symbols
in include/rflu.h, their ctypes bindings, the exports of the built library and its version, the Julia ccalls, the argument checks
inv_complex_batched makes BEFORE it touches the library, what reaches the library for each letter and for Adjoint(F), the documents,
and where the kernel stands in csrc/batched_complex.hip."""
import os
import re
import subprocess

import pytest
import torch

import recursivefactorization.jl_amd as rf
from recursivefactorization.jl_amd import _ffi
from test_complex_batched_glue import _FakeCuda, _NoLibrary, _fake
from test_julia_glue import JL2C, ROOT, c_prototypes, julia_ccalls

SYMBOLS = ["rflu_getri_batched_cf64_dev", "rflu_getri_batched_cf32_dev"]
GETRI = ["rflu_handle_t", "int64_t", "int64_t", "{T}*", "int64_t", "int64_t", "int", "int64_t*", "int64_t", "{T}*", "int64_t", "int64_t",
         "int", "int64_t*"]
CSRC = os.path.join(ROOT, "recursivefactorization.jl_amd", "csrc")


@pytest.fixture
def no_library(monkeypatch):
    monkeypatch.setattr(_ffi, "default_handle", lambda *a, **k: _NoLibrary())
    monkeypatch.setattr(_ffi, "load", lambda *a, **k: _NoLibrary())


def _lu(batch=4, n=8, dtype=torch.complex128, info=None):
    return rf.BatchedLU(_fake(batch, n, n, dtype=dtype), _fake(batch, n, dtype=torch.int64),
                        torch.zeros(batch, dtype=torch.int64) if info is None else torch.tensor(info))


def test_symbols_declared_and_bound():
    protos = c_prototypes()
    for sym in SYMBOLS:
        assert sym in protos, f"{sym} is not declared in include/rflu.h"
        assert sym in _ffi.EXPORTS, f"{sym} is not bound in _ffi.py"
        cret, cparams = protos[sym]
        T = "double" if "cf64" in sym else "float"
        assert cret == "int" and cparams == [p.format(T=T) for p in GETRI], (sym, cparams)
        res, args = _ffi.EXPORTS[sym]
        assert res is _ffi.c_int and len(args) == len(cparams)
        for ct, at in zip(cparams, args):
            expect = {"int64_t": _ffi.c_i64, "int": _ffi.c_int}.get(ct, _ffi.c_p)
            assert at is expect, (sym, ct, at)
    # the real entries keep their argument list: `trans` belongs to the complex ones alone
    assert len(_ffi.EXPORTS["rflu_getri_batched_f64_dev"][1]) == len(GETRI) - 1


def test_library_exports_the_symbols_and_the_version():
    assert os.path.exists(_ffi.LIB_PATH), "librflu.so has not been built (build() comes first)"
    out = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for sym in SYMBOLS:
        assert sym in exported, sym
    assert _ffi.load().rflu_version() >= 107   # needs no device
    assert int(re.search(r"int rflu_version\(void\) \{ return (\d+); \}", open(os.path.join(CSRC, "driver.cpp")).read()).group(1)) >= 107


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
        assert sum(f"reinterpret(Ptr{{{R}}}" in a for a in args) == 2, f"{sym}: F and Ainv are reinterpreted to Ptr{{{R}}}"
        assert "batched_trans_code(trans)" in args[-2] and args[-1].strip() == "info"
    src = open(os.path.join(ROOT, "julia", "RFLUAMD", "src", "RFLUAMD.jl")).read()
    heads = re.findall(r"function getri_batched_dev!\(Ainv::Ptr\{ComplexF(64|32)\}[^)]*\)", src)
    assert sorted(heads) == ["32", "64"]
    for m in re.finditer(r"function getri_batched_dev!\(Ainv::Ptr\{ComplexF(?:64|32)\}[^)]*\)", src):
        assert m.group(0).rstrip(")").endswith("trans::AbstractChar")         # the letter comes last
    assert "complex batched getri" in open(os.path.join(ROOT, "julia", "RFLUAMD", "test", "runtests.jl")).read()


def test_documents_and_header():
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "rflu_getri_batched_cf64_dev" in text and "inv_complex_batched" in text, doc
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "4.9" in design and "cgetri_batched_kernel" in design
    api = open(os.path.join(ROOT, "include", "rflu.h")).read()
    assert "Not here: a batched complex getri" not in api and "a batched complex getri" not in api
    block = api[api.index("BATCHED COMPLEX:"):]
    assert "rflu_getri_batched_c*" in block[:block.index("int rflu_getri_batched_cf64_dev")]
    readme = open(os.path.join(ROOT, "README.md")).read()
    for fn in ("tests/test_gpu_complex_batched_inv.py", "tests/complex_batched_inv_cases.py", "scripts/microbench_complex_batched_inv.py"):
        assert fn in readme, f"{fn} is missing from the layout table"


def test_the_kernel_stands_behind_the_existing_ones():
    """Moved code alone has cost the existing kernels time before, so the new kernel and its launch come after everything the file
    held; and it is built from the parts of the solve: the same load, the same substitution, no second substitution of its own."""
    code = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "batched_complex.hip")).read())
    last_old = code.index("template int launch_cgetrs_batched<float>")
    assert code.index("struct CInvArgs") > last_old and code.index("cgetri_batched_kernel(CInvArgs<R> a)") > last_old
    body = code[code.index("cgetri_batched_kernel(CInvArgs<R> a)"):code.index("int launch_cgetri_batched(")]
    assert body.count("cbload_matrix<R>(") == 1 and body.count("cbsubstitute<R, 0>(") == 1 and "cbsubstitute<R, 1>" not in body
    assert body.count("__ballot(") == 2 and "atomic" not in code
    launch = code[code.index("int launch_cgetri_batched("):]
    assert "batched_geo(n, n, sizeof(Cx<R>), true, true)" in launch and "launch_batched(h, 2, 2 + (sizeof(R) == 4)" in launch
    assert "batched_attr_set[3][4]" in open(os.path.join(CSRC, "rflu_internal.hpp")).read()


def test_exports_of_the_package():
    assert hasattr(rf, "inv_complex_batched") and "inv_complex_batched" in rf.__all__


def test_inv_complex_batched_rejects_bad_arguments_before_the_library(no_library):
    with pytest.raises(TypeError):
        rf.inv_complex_batched(_fake(4, 8, 8))                                # not a factorization
    with pytest.raises(TypeError):
        rf.inv_complex_batched(rf.LU(_fake(8, 8), None, 0))                   # not a batch
    ipiv, info = _fake(4, 8, dtype=torch.int64), torch.zeros(4, dtype=torch.int64)
    with pytest.raises(TypeError):
        rf.inv_complex_batched(rf.BatchedLU(_fake(8, 8), ipiv, info))         # 2-D
    with pytest.raises(TypeError):
        rf.inv_complex_batched(rf.BatchedLU(torch.zeros(4, 8, 8, dtype=torch.complex128), ipiv, info))   # host factors
    with pytest.raises(ValueError, match="square"):
        rf.inv_complex_batched(rf.BatchedLU(_fake(4, 8, 6), _fake(4, 6, dtype=torch.int64), info))
    for real in (torch.float64, torch.float32):
        with pytest.raises(TypeError, match="real batches"):
            rf.inv_complex_batched(_lu(dtype=real))
    with pytest.raises(ValueError):                                           # neither column-major nor row-major
        rf.inv_complex_batched(rf.BatchedLU(_FakeCuda(torch.zeros(4, 16, 16, dtype=torch.complex64)[:, ::2, ::2]), ipiv, info))
    with pytest.raises(ValueError):                                           # overlapping matrices
        rf.inv_complex_batched(rf.BatchedLU(_FakeCuda(torch.zeros(8, 8, dtype=torch.complex64).expand(4, 8, 8)), ipiv, info))
    with pytest.raises(TypeError):                                            # host pivots
        rf.inv_complex_batched(rf.BatchedLU(_fake(4, 8, 8), torch.zeros(4, 8, dtype=torch.int64), info))
    for bad in ("H", "n", True, 1, None):
        with pytest.raises(ValueError, match="trans"):
            rf.inv_complex_batched(_lu(), trans=bad)
    with pytest.raises(TypeError):
        rf.inv_complex_batched(rf.Adjoint(rf.Adjoint(_lu())))                 # doubly wrapped
    with pytest.raises(ValueError, match="already means"):
        rf.inv_complex_batched(rf.Adjoint(_lu()), trans="T")                  # the wrapper already says 'C'
    # a singular matrix is reported with its index before anything is launched
    with pytest.raises(rf.SingularException) as ei:
        rf.inv_complex_batched(_lu(info=[0, 0, 3, 5]))
    assert ei.value.info == 3 and ei.value.batch_index == 2
    # nothing to do needs no library
    X = rf.inv_complex_batched(rf.BatchedLU(_fake(0, 8, 8), _fake(0, 8, dtype=torch.int64), torch.zeros(0, dtype=torch.int64)))
    assert X.shape == (0, 8, 8)
    assert rf.inv_complex_batched(rf.BatchedLU(_fake(4, 0, 0), _fake(4, 0, dtype=torch.int64), info)).shape == (4, 0, 0)


def test_inv_batched_keeps_refusing_complex_factors(no_library):
    with pytest.raises(TypeError):
        rf.inv_batched(_lu())


class _Recorder:
    """Stands in for the handle: records the entry and its arguments; ``info`` (what the library would have written) stays zero."""

    def __init__(self):
        self.seen = []

    def set_stream(self, *_):
        pass

    def call(self, name, *args):
        self.seen.append((name, args))


def test_what_reaches_the_library(monkeypatch):
    """Adjoint(F) reaches the library as trans = 2 (LAPACK 'C'), 'T' as 1, 'N' as 0; the output is a new dense tensor in the orientation
    of the factors with ldi = n and strideI = n * n, never a conjugated view."""
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a, **k: type("S", (), {"cuda_stream": 0})())
    rec = _Recorder()
    batch, n = 4, 8
    rm = _lu(batch, n)
    cm = rf.BatchedLU(_FakeCuda(torch.zeros(batch, n, n, dtype=torch.complex64).transpose(1, 2)), rm.ipiv, rm.info)
    for F, sfx, row_major in ((rm, "cf64", 1), (cm, "cf32", 0)):
        for arg, kw, code in ((F, {}, 0), (F, {"trans": "T"}, 1), (F, {"trans": "C"}, 2), (rf.Adjoint(F), {}, 2)):
            X = rf.inv_complex_batched(arg, handle=rec, **kw)
            name, a = rec.seen[-1]
            assert name == f"rflu_getri_batched_{sfx}_dev"
            assert (a[0], a[1], a[3], a[4], a[5], a[7], a[9], a[10], a[11]) == (batch, n, n, n * n, row_major, n, n, n * n, code)
            assert a[8].value == X.data_ptr() and a[2].value == F.factors.data_ptr() and a[6].value == F.ipiv.data_ptr()
            assert X.shape == (batch, n, n) and X.stride() == F.factors.stride() and not X.is_conj() and X.dtype == F.factors.dtype
    assert len(rec.seen) == 8
    nopiv = rf.BatchedLU(rm.factors, rf.NotIPIV(n), rm.info)
    rf.inv_complex_batched(nopiv, handle=rec)
    assert rec.seen[-1][1][6].value in (0, None) and rec.seen[-1][1][7] == 0   # NULL ipiv = NotIPIV
