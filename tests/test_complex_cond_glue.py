"""opnorm_complex / rcond_complex / cond_complex and their batched forms through the layers that can be checked without a GPU: the ten
symbols in include/rflu.h with the argument lists of the real entries of the same name, their ctypes bindings, the exports of the built
library, the Julia ccalls, the source list of the build, and the argument checks the Python mirror makes BEFORE it touches the library."""
import math
import os
import subprocess

import numpy as np
import pytest

import recursivefactorization.jl_amd as rf
from recursivefactorization.jl_amd import _ffi
from test_julia_glue import JL2C, ROOT, c_prototypes, julia_ccalls

H, I, N, D, PD = "rflu_handle_t", "int64_t", "int", "double", "double*"
ARGS = {}
for _s, _t in (("cf64", "double*"), ("cf32", "float*")):
    ARGS[f"rflu_lange_{_s}_dev"] = [H, N, I, I, _t, I, N, PD]
    ARGS[f"rflu_lange_batched_{_s}_dev"] = [H, N, I, I, I, _t, I, I, N, PD]
    ARGS[f"rflu_gecon_{_s}_dev"] = [H, N, I, _t, I, D, PD]
    ARGS[f"rflu_gecon_{_s}"] = [H, N, I, _t, I, D, PD]
    ARGS[f"rflu_gecon_batched_{_s}_dev"] = [H, N, I, I, _t, I, I, N, PD, PD]
NEW = ("opnorm_complex", "rcond_complex", "cond_complex", "opnorm_complex_batched", "rcond_complex_batched", "cond_complex_batched")


def test_symbols_declared_and_bound():
    assert len(ARGS) == 10
    protos = c_prototypes()
    for sym, want in ARGS.items():
        assert sym in protos, f"{sym} is not declared in include/rflu.h"
        assert sym in _ffi.EXPORTS, f"{sym} is not bound in _ffi.py"
        cret, cparams = protos[sym]
        assert cret == "int" and cparams == want, (sym, cparams)
        real = sym.replace("_cf64", "_f64").replace("_cf32", "_f32")
        assert cparams == protos[real][1], (sym, "the argument list is that of the real entry")
        res, args = _ffi.EXPORTS[sym]
        assert res is _ffi.c_int and len(args) == len(cparams)
        for ct, at in zip(cparams, args):
            expect = {"int64_t": _ffi.c_i64, "int": _ffi.c_int, "double": _ffi.c_dbl}.get(ct, _ffi.c_p)
            assert at is expect, (sym, ct, at)
    for s in ("cf64", "cf32"):          # the single-matrix complex path is column-major only
        assert f"rflu_gecon_rm_{s}_dev" not in protos and f"rflu_gecon_rm_{s}_dev" not in _ffi.EXPORTS


def test_library_exports_the_symbols_and_the_version():
    assert os.path.exists(_ffi.LIB_PATH), "librflu.so has not been built (build() comes first)"
    out = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for sym in ARGS:
        assert sym in exported, sym
    assert _ffi.load().rflu_version() >= 110   # needs no device


def test_source_is_wired_and_documented():
    pkg = os.path.join(ROOT, "recursivefactorization.jl_amd")
    from recursivefactorization.jl_amd import build as B

    assert "condest.hip" in B.SOURCES and "complex_condest.hip" not in B.SOURCES + list(B.EXTRA_DEPS)   # one source, real and complex
    assert not os.path.exists(os.path.join(pkg, "csrc", "complex_condest.hip"))
    condest = open(os.path.join(pkg, "csrc", "condest.hip")).read()
    assert "RFLU_CONDEST_FOR(CplxElem<double>)" in condest and "RFLU_CONDEST_FOR(CplxElem<float>)" in condest
    assert "cgecon_batched_kernel" in open(os.path.join(pkg, "csrc", "batched_complex.hip")).read()
    solve = open(os.path.join(pkg, "csrc", "complex_solve.hip")).read()
    assert "template int csolve_fwd_narrow<double>(" in solve
    hdr = open(os.path.join(ROOT, "include", "rflu.h")).read()
    assert "COMPLEX NORMS, CONDITION" in hdr and "NO rflu_gecon_rm_c*" in hdr and "NO size limit" in hdr
    assert "M^H" in hdr and "NO repeated-sign-vector test" in hdr
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "rflu_gecon_cf64" in open(os.path.join(ROOT, doc)).read() or "rflu_gecon_{cf64,cf32}" in open(os.path.join(ROOT, doc)).read(), doc
    assert "4.12" in open(os.path.join(ROOT, "DESIGN.md")).read()


def test_julia_binds_the_entries():
    calls = {c[1]: c for c in julia_ccalls()}
    protos = c_prototypes()
    for sym in ARGS:
        assert sym in calls, f"{sym} has no ccall in julia/RFLUAMD"
        _, _, ret, types, args = calls[sym]
        assert ret == "Cint" and len(types) == len(args) == len(protos[sym][1])
        for jt, ct in zip(types, protos[sym][1]):
            assert ct in JL2C[jt], (sym, jt, ct)
    src = open(os.path.join(ROOT, "julia", "RFLUAMD", "src", "RFLUAMD.jl")).read()
    assert "function rcond(F::LU{T, <:StridedMatrix{T}}, anorm::Real; p::Real = 1) where {T <: GPUComplexEltype}" in src
    for jt in ("ComplexF64", "ComplexF32"):
        for name in ("function lange_dev(A::Ptr{%s}", "function gecon_dev!(F::Ptr{%s}", "function gecon_host(F::StridedMatrix{%s}",
                     "function gecon_batched_dev!(rcond::Ptr{Float64}, F::Ptr{%s}"):
            assert name % jt in src, name % jt


def test_exports():
    for name in NEW:
        assert name in rf.__all__ and callable(getattr(rf, name))
        assert "|conj z| = |z|" in " ".join(getattr(rf, name).__doc__.split()), name      # why no trans letter is needed


# ---- the argument rules of the Python functions: every one of these raises before the library (or a device) is touched
def _lu_of(a):
    return rf.LU(np.asfortranarray(a), rf.NotIPIV(a.shape[0]), 0)


@pytest.mark.parametrize("p", [2, 0, "fro", "1", None, True, -1, math.nan])
def test_p_must_be_one_or_inf(p):
    a = np.eye(3, dtype=np.complex128)
    for call in (lambda: rf.opnorm_complex(a, p), lambda: rf.rcond_complex(_lu_of(a), 1.0, p), lambda: rf.cond_complex(a, p)):
        with pytest.raises(ValueError):
            call()


def test_real_input_is_refused_with_the_real_names():
    for dt in (np.float64, np.float32):
        a = np.eye(3, dtype=dt)
        for call, name in ((lambda: rf.opnorm_complex(a), "opnorm"), (lambda: rf.rcond_complex(_lu_of(a), 1.0), "rcond"),
                           (lambda: rf.cond_complex(a), "cond")):
            with pytest.raises(TypeError, match=rf"real element types go to {name}$"):
                call()


def test_the_real_functions_still_refuse_complex_and_name_the_new_ones():
    for dt in (np.complex128, np.complex64):
        a = np.eye(3, dtype=dt)
        for call, name in ((lambda: rf.opnorm(a), "opnorm_complex"), (lambda: rf.rcond(_lu_of(a), 1.0), "rcond_complex"),
                           (lambda: rf.cond(a), "cond_complex")):
            with pytest.raises(TypeError, match="complex") as ei:
                call()
            assert name in str(ei.value)


class _Recorder:
    """Stands in for a handle: records the call instead of making it."""
    device = 0

    def __init__(self):
        self.calls = []

    def set_stream(self, s):
        pass

    def call(self, name, *args):
        self.calls.append((name, args))


def test_adjoint_swaps_the_norm_and_host_factors_take_the_host_entry():
    for dt, s in ((np.complex128, "cf64"), (np.complex64, "cf32")):
        F = _lu_of(np.eye(3, dtype=dt))
        for p, code in ((1, _ffi.NORM_ONE), (math.inf, _ffi.NORM_INF), ("inf", _ffi.NORM_INF)):
            rec = _Recorder()
            rf.rcond_complex(F, 2.0, p, handle=rec)
            rf.rcond_complex(rf.Adjoint(F), 2.0, p, handle=rec)
            (n0, a0), (n1, a1) = rec.calls
            assert n0 == n1 == f"rflu_gecon_{s}"
            assert a0[0] == code and a1[0] == (_ffi.NORM_ONE + _ffi.NORM_INF - code)
            assert a0[1] == 3 and a0[3] == 3 and a0[4] == 2.0


def test_shape_and_type_rules():
    e = np.eye(3, dtype=np.complex128)
    with pytest.raises(ValueError):
        rf.rcond_complex(rf.LU(np.zeros((3, 4), order="F", dtype=np.complex128), rf.NotIPIV(3), 0), 1.0)
    with pytest.raises(ValueError):
        rf.rcond_complex(rf.LU(np.ascontiguousarray(e + np.triu(e, 1) + np.ones((3, 3))), rf.NotIPIV(3), 0), 1.0)   # row-major host factors
    with pytest.raises(ValueError):
        rf.cond_complex(np.zeros((3, 4), dtype=np.complex64))
    with pytest.raises(ValueError):
        rf.opnorm_complex(np.zeros(3, dtype=np.complex64))
    with pytest.raises(TypeError):
        rf.rcond_complex(e, 1.0)                                                         # not an LU
    with pytest.raises(ValueError):
        rf.rcond_complex(_lu_of(e), -1.0)                                                # anorm < 0
    with pytest.raises(TypeError):
        rf.rcond_complex(rf.Adjoint(rf.Adjoint(_lu_of(e))), 1.0)
    with pytest.raises(TypeError):
        rf.opnorm_complex(rf.Adjoint(rf.Adjoint(e)))
    with pytest.raises(TypeError):
        rf.opnorm_complex(np.eye(3, dtype=np.int64))
    with pytest.raises(TypeError):
        rf.opnorm_complex_batched(np.zeros((2, 3, 3), dtype=np.complex128))              # a batch lives on the device
    with pytest.raises(TypeError):
        rf.rcond_complex_batched(_lu_of(e), None)                                        # not a BatchedLU
    with pytest.raises(ValueError):
        rf.cond_complex_batched(np.zeros((2, 3, 3), dtype=np.complex128))
    # the empty matrix needs no device
    assert rf.opnorm_complex(np.zeros((0, 3), dtype=np.complex64)) == 0.0
    assert rf.rcond_complex(_lu_of(np.zeros((0, 0), dtype=np.complex128)), 1.0) == 1.0
    assert rf.cond_complex(np.zeros((0, 0), dtype=np.complex128)) == 1.0
