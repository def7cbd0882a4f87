"""Complex inv / det / logabsdet through the layers that can be checked without a GPU: the ten rflu_getri_c* / rflu_logabsdet_c* symbols
in include/rflu.h with the argument lists the interface fixes, their ctypes bindings, the exports of the built library, the Julia
ccalls, the build list and the documents, the argument checks the Python mirror makes BEFORE it touches the library, what the wrappers
do with the adjoint and the transpose (against a stub handle), and a NumPy transcription of the two sweeps of
csrc/inverse.hip (one source for real and complex elements) -- same index arithmetic -- against numpy.linalg.inv."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import recursivefactorization.jl_amd as rf
import complex_inv_cases as C
from recursivefactorization.jl_amd import _ffi, build
from test_inv_glue import _FakeCuda, _NoLibrary
from test_julia_glue import JL2C, ROOT, c_prototypes, julia_ccalls

H, I, PI, PD = "rflu_handle_t", "int64_t", "int64_t*", "double*"
ARGS = {}
for _s, _t in (("cf64", "double*"), ("cf32", "float*")):
    ARGS[f"rflu_getri_{_s}_dev"] = [H, I, _t, I, PI, PI]
    ARGS[f"rflu_getri_{_s}"] = [H, I, _t, I, PI, PI]
    ARGS[f"rflu_logabsdet_{_s}_dev"] = [H, I, _t, I, PI, PD, PD, PD]
    ARGS[f"rflu_logabsdet_{_s}"] = [H, I, _t, I, PI, PD, PD, PD]
    ARGS[f"rflu_logabsdet_batched_{_s}_dev"] = [H, I, I, _t, I, I, PI, I, PD, PD]
CSRC = os.path.join(ROOT, "recursivefactorization.jl_amd", "csrc")
COMPLEX_FNS = ("inv_complex", "inv_complex_", "det_complex", "logabsdet_complex", "logdet_complex", "logabsdet_complex_batched",
               "det_complex_batched")


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


def test_library_exports_the_symbols_and_the_version():
    assert os.path.exists(_ffi.LIB_PATH), "librflu.so has not been built (build() comes first)"
    out = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for sym in ARGS:
        assert sym in exported, sym
    assert _ffi.load().rflu_version() >= 106   # needs no device


def test_source_is_wired_and_documented():
    # one source serves the real and the complex elements: inverse.hip, built against the complex headers; its complex twin is gone
    assert "inverse.hip" in build.SOURCES                    # the source list is also what sources_digest() hashes
    assert "complex_inverse.hip" not in build.SOURCES and "complex_inverse.hip" not in build.EXTRA_DEPS
    assert not os.path.exists(os.path.join(CSRC, "complex_inverse.hip"))
    assert sorted(build.EXTRA_DEPS["inverse.hip"]) == ["complex.hpp", "complex_dev.hpp"]
    text = open(os.path.join(CSRC, "inverse.hip")).read()
    code = re.sub(r"//[^\n]*", "", text)
    for needle in ("atomic", "while (", "while(", "hipLaunchCooperativeKernel", "conj"):   # nothing waits, nothing is conjugated
        assert needle not in code, needle
    assert '#include "complex_dev.hpp"' in text and "Cx<" in code
    for elem in ("RealElem<double>", "RealElem<float>", "CplxElem<double>", "CplxElem<float>"):   # the four element types, one text
        assert f"RFLU_INVERSE_FOR({elem})" in code, elem
    solve = open(os.path.join(CSRC, "complex_solve.hip")).read()
    assert "static int launch_claswp_rev" not in solve and "launch_claswp_rev" in open(os.path.join(CSRC, "complex.hpp")).read()
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "rflu_getri_cf64" in text and "inv_complex" in text, doc
    assert "4.8" in open(os.path.join(ROOT, "DESIGN.md")).read()
    api = open(os.path.join(ROOT, "include", "rflu.h")).read()
    assert "there is no mixed / inverse form" not in api
    assert int(re.search(r"int rflu_version\(void\) \{ return (\d+); \}", open(os.path.join(CSRC, "driver.cpp")).read()).group(1)) >= 106


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
        R = "Float64" if "cf64" in sym else "Float32"
        assert any(f"reinterpret(Ptr{{{R}}}" in a for a in args), f"{sym}: the complex pointer is not reinterpreted to Ptr{{{R}}}"
    src = open(os.path.join(ROOT, "julia", "RFLUAMD", "src", "RFLUAMD.jl")).read()
    for needle in (r"function getri!\(F::StridedMatrix\{ComplexF(64|32)\}", r"function getri_dev!\(F::Ptr\{ComplexF(64|32)\}",
                   r"function logabsdet_dev\(F::Ptr\{ComplexF(64|32)\}", r"function logabsdet_host\(F::StridedMatrix\{ComplexF(64|32)\}",
                   r"function logabsdet_batched_dev!\(logabs::Ptr\{Float64\}, sign::Ptr\{ComplexF64\}, F::Ptr\{ComplexF(64|32)\}"):
        assert len(re.findall(needle, src)) == 2, needle
    assert "complex inv!" in open(os.path.join(ROOT, "julia", "RFLUAMD", "test", "runtests.jl")).read()


def test_exports_of_the_package():
    for name in COMPLEX_FNS:
        assert hasattr(rf, name) and name in rf.__all__, name


# ---- the argument checks, before the library ----------------------------------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    monkeypatch.setattr(_ffi, "default_handle", lambda *a, **k: _NoLibrary())
    monkeypatch.setattr(_ffi, "load", lambda *a, **k: _NoLibrary())


def _fake_cm(m, n, dtype=torch.complex128):
    return _FakeCuda(torch.zeros(n, m, dtype=dtype).T)


def _fake_ipiv(n):
    return _FakeCuda(torch.zeros(n, dtype=torch.int64))


SINGLE = [rf.inv_complex_, rf.inv_complex, rf.logabsdet_complex, rf.det_complex, rf.logdet_complex]


@pytest.mark.parametrize("fn", SINGLE)
def test_single_matrix_entries_reject_bad_arguments_before_the_library(fn, no_library):
    with pytest.raises(TypeError):
        fn(_fake_cm(8, 8))                                                    # not a factorization
    with pytest.raises(TypeError):
        fn(rf.BatchedLU(_FakeCuda(torch.zeros(4, 8, 8, dtype=torch.complex128)), None, None))
    F = rf.LU(np.zeros((0, 0), dtype=np.complex128, order="F"), np.zeros(0, dtype=np.int64), 0)
    rf.inv_complex_(F)
    with pytest.raises(ValueError, match="no longer valid"):
        fn(F)                                                                 # invalidated by inv_complex_
    with pytest.raises(ValueError, match="square"):
        fn(rf.LU(_fake_cm(8, 6), _fake_ipiv(6), 0))
    with pytest.raises(ValueError, match="square"):
        fn(rf.LU(np.zeros((6, 8), dtype=np.complex64, order="F"), np.arange(1, 7), 0))
    for real in (torch.float64, torch.float32):
        with pytest.raises(TypeError, match="real factors go to inv"):
            fn(rf.LU(_fake_cm(8, 8, real), _fake_ipiv(8), 0))                 # real factors handed to the complex functions
    with pytest.raises(TypeError, match="real factors go to inv"):
        fn(rf.LU(np.zeros((8, 8), order="F"), np.arange(1, 9), 0))
    with pytest.raises(ValueError, match="the complex path is column-major only"):
        fn(rf.LU(_FakeCuda(torch.zeros(8, 8, dtype=torch.complex128)), _fake_ipiv(8), 0))   # a row-major CUDA tensor
    with pytest.raises(ValueError, match="the complex path is column-major only"):
        fn(rf.LU(np.zeros((8, 8), dtype=np.complex128, order="C"), np.arange(1, 9), 0))
    with pytest.raises(TypeError):
        fn(rf.LU(_fake_cm(8, 8), np.arange(1, 9), 0))                         # GPU factors, host pivots
    with pytest.raises(TypeError):
        fn(rf.Adjoint(rf.Adjoint(rf.LU(_fake_cm(8, 8), _fake_ipiv(8), 0))))   # doubly wrapped
    with pytest.raises(ValueError, match="trans"):
        fn(rf.LU(_fake_cm(8, 8), _fake_ipiv(8), 0), trans="H")
    with pytest.raises(ValueError, match="already means"):
        fn(rf.Adjoint(rf.LU(_fake_cm(8, 8), _fake_ipiv(8), 0)), trans="T")    # nothing is guessed: the wrapper and a letter together
    with pytest.raises(rf.RfluError):
        fn(rf.LU(torch.zeros(8, 8, dtype=torch.complex128).T, _fake_ipiv(8), 0))   # host tensor


@pytest.mark.parametrize("fn", [rf.inv_complex_, rf.inv_complex])
def test_inverse_of_a_singular_factorization_raises_before_the_library(fn, no_library):
    for F in (rf.LU(_fake_cm(8, 8), _fake_ipiv(8), 3), rf.LU(np.zeros((8, 8), dtype=np.complex64, order="F"), np.arange(1, 9), 3),
              rf.Adjoint(rf.LU(_fake_cm(8, 8), rf.NotIPIV(8), -3))):
        with pytest.raises(rf.SingularException) as ei:
            fn(F)
        assert ei.value.info == 3


@pytest.mark.parametrize("fn", [rf.logabsdet_complex_batched, rf.det_complex_batched])
def test_batched_entries_reject_bad_arguments_before_the_library(fn, no_library):
    info = _FakeCuda(torch.zeros(4, dtype=torch.int64))
    ipiv = _FakeCuda(torch.zeros(4, 8, dtype=torch.int64))
    with pytest.raises(ValueError):
        fn(rf.BatchedLU(_FakeCuda(torch.zeros(4, 8, 6, dtype=torch.complex128)), ipiv, info))        # not square
    with pytest.raises(TypeError, match="real batches"):
        fn(rf.BatchedLU(_FakeCuda(torch.zeros(4, 8, 8, dtype=torch.float64)), ipiv, info))
    with pytest.raises(ValueError):
        fn(rf.BatchedLU(_FakeCuda(torch.zeros(4, 16, 16, dtype=torch.complex64)[:, ::2, ::2]), ipiv, info))
    with pytest.raises(TypeError):
        fn(rf.LU(_fake_cm(8, 8), _fake_ipiv(8), 0))                                                    # not a batch
    with pytest.raises(TypeError):
        fn(rf.Adjoint(rf.Adjoint(rf.BatchedLU(_FakeCuda(torch.zeros(4, 8, 8, dtype=torch.complex128)), ipiv, info))))


def test_the_real_functions_still_refuse_complex_factors(no_library):
    for fn in (rf.inv_, rf.inv, rf.det, rf.logabsdet, rf.logdet):
        for F in (rf.LU(_fake_cm(8, 8), _fake_ipiv(8), 0), rf.LU(np.zeros((8, 8), dtype=np.complex64, order="F"), np.arange(1, 9), 0)):
            with pytest.raises(TypeError, match="lu / lu_ serve Float64/Float32 only"):
                fn(F)


def test_empty_matrix_needs_no_library(no_library):
    F = rf.LU(np.zeros((0, 0), dtype=np.complex128, order="F"), np.zeros(0, dtype=np.int64), 0)
    assert rf.logabsdet_complex(F) == (0.0, 1 + 0j) and rf.det_complex(F) == 1 + 0j and rf.logdet_complex(F) == 0j
    assert rf.inv_complex(F).shape == (0, 0)
    X = rf.inv_complex_(F)
    assert X.shape == (0, 0) and F.factors is None


# ---- what the wrappers do with A' and transpose(A): against a stub handle -------------------------------------------------------------
class _StubHandle:
    """Answers rflu_getri_c* by leaving the buffer as it is (info = 0) and rflu_logabsdet_c* with a fixed (logabs, sign)."""

    def __init__(self, logabs=1.5, sign=complex(0.6, 0.8)):
        self.logabs, self.sign, self.calls = logabs, sign, []

    def set_stream(self, s):
        pass

    def call(self, name, *args):
        self.calls.append(name)
        if "getri" in name:
            args[-1]._obj.value = 0
        else:
            assert "logabsdet" in name
            args[-3]._obj.value, args[-2]._obj.value, args[-1]._obj.value = self.logabs, self.sign.real, self.sign.imag


def _host_factors(n=5):
    rng = np.random.default_rng(3)
    return np.asfortranarray(rng.random((n, n)) + 1j * rng.random((n, n)))


def test_adjoint_conjugates_and_transpose_does_not():
    fac = _host_factors()
    F = rf.LU(fac.copy(order="F"), np.arange(1, 6), 0)
    h = _StubHandle()
    X = rf.inv_complex(F, handle=h)                                           # the stub's "inverse" is the buffer itself
    assert np.array_equal(X, fac) and np.array_equal(F.factors, fac)
    Xc, Xt = rf.inv_complex(rf.Adjoint(F), handle=h), rf.inv_complex(F, trans="T", handle=h)
    assert np.array_equal(Xc, fac.conj().T) and np.array_equal(Xt, fac.T) and not np.array_equal(Xc, Xt)
    assert np.array_equal(rf.inv_complex(F, trans="C", handle=h), Xc)
    assert np.array_equal(rf.inv_complex(rf.Transpose(F), handle=h), Xc)      # Transpose IS Adjoint here, so it says "C" -- use trans="T"
    assert h.calls == ["rflu_getri_cf64"] * 5
    la, sg = rf.logabsdet_complex(F, handle=h)
    assert (la, sg) == (1.5, complex(0.6, 0.8))
    assert rf.logabsdet_complex(rf.Adjoint(F), handle=h) == (1.5, complex(0.6, -0.8))
    assert rf.logabsdet_complex(F, trans="C", handle=h) == (1.5, complex(0.6, -0.8))
    assert rf.logabsdet_complex(F, trans="T", handle=h) == (1.5, complex(0.6, 0.8))
    d = complex(0.6, 0.8) * float(np.exp(np.float64(1.5)))
    assert rf.det_complex(F, handle=h) == d and rf.det_complex(F, trans="T", handle=h) == d
    assert rf.det_complex(rf.Adjoint(F), handle=h) == d.conjugate()
    ld = rf.logdet_complex(F, handle=h)
    assert ld == complex(1.5, float(np.angle(complex(0.6, 0.8)))) and abs(ld.imag - math.atan2(0.8, 0.6)) < 1e-15                           # the imaginary part is angle(sign)
    assert rf.logdet_complex(rf.Adjoint(F), handle=h) == ld.conjugate() and rf.logdet_complex(F, trans="T", handle=h) == ld
    # inv_complex_ invalidates F as inv_ does, and hands back the buffer itself
    buf = F.factors
    assert rf.inv_complex_(F, handle=h) is buf and F.factors is None


def test_det_of_a_singular_factorization_is_zero():
    F = rf.LU(_host_factors(), np.arange(1, 6), 0)
    h = _StubHandle(logabs=-math.inf, sign=0j)
    assert rf.logabsdet_complex(F, handle=h) == (-math.inf, 0j)
    d = rf.det_complex(F, handle=h)
    assert d == 0j and isinstance(d, complex)
    assert rf.det_complex(rf.Adjoint(F), handle=h) == 0j


def test_a_singular_info_from_the_library_leaves_the_factorization_valid():
    class Singular(_StubHandle):
        def call(self, name, *args):
            args[-1]._obj.value = 4

    F = rf.LU(_host_factors(), np.arange(1, 6), 0)
    with pytest.raises(rf.SingularException) as ei:
        rf.inv_complex_(F, handle=Singular())
    assert ei.value.info == 4 and F.factors is not None


# ---- the two sweeps, transcribed ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [128, 512])
@pytest.mark.parametrize("n", [1, 2, 63, 65, 129, 513, 700])
def test_numpy_transcription_of_the_sweeps(n, W):
    import complex_ref as R

    A = C.rand_matrix(n, np.complex128)
    F, ipiv, info = R.complex_generic_lufact(A)
    assert info == 0
    X = C.getri_transcription(F, ipiv, W)
    r, l = C.rho(A, X, np.complex128)
    r0, l0 = C.rho(A, np.linalg.inv(A), np.complex128)
    print(f"n={n} W={W}: rho_R = {r:.3e}, rho_L = {l:.3e} (numpy.linalg.inv: {r0:.3e}, {l0:.3e})")
    assert r <= C.rho_bar(n) and l <= C.rho_bar(n)
    assert np.abs(X - np.linalg.inv(A)).max() <= 64 * n * np.finfo(np.float64).eps * np.linalg.cond(A, 1) * np.abs(X).max()


@pytest.mark.parametrize("n", C.EXACT_SIZES)
def test_the_transcription_and_its_mutations_on_the_exact_inputs(n):
    """What the GPU test's exact cases catch: the conjugated H, the skipped width-64 recursion, the interchanges applied forwards."""
    c = C.exact_case(n)
    assert np.array_equal(C.getri_transcription(c.F, c.ipiv), c.X)
    assert not np.array_equal(C.getri_transcription(c.F, c.ipiv, conj_h=True), c.X)
    assert not np.array_equal(C.getri_transcription(c.F, c.ipiv, recurse=False), c.X)
    assert not np.array_equal(C.getri_transcription(c.F, c.ipiv, reverse=False), c.X)
    assert np.array_equal(C.getri_transcription(np.conj(c.F), c.ipiv), np.conj(c.X))
