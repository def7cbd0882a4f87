"""refine_ / solve_refined / backward_error through the layers that can be checked without a GPU: the four symbols in include/rflu.h with
the argument lists the interface fixes, their ctypes bindings, the exports of the built library, the Julia ccalls, the source list of
the build, and every refusal the Python mirror makes BEFORE it touches the library."""
import os
import subprocess

import numpy as np
import pytest

import recursivefactorization.jl_amd as rf
from recursivefactorization.jl_amd import _ffi
from test_julia_glue import JL2C, ROOT, c_prototypes, julia_ccalls

H, I, N, PD, PI, PN = "rflu_handle_t", "int64_t", "int", "double*", "int64_t*", "int*"
ARGS = {}
for _s, _t in (("f64", "double*"), ("f32", "float*")):
    ARGS[f"rflu_gerfs_{_s}_dev"] = [H, I, I, _t, I, _t, I, PI, _t, I, _t, I, PD, PD, N, PN, PI]
    ARGS[f"rflu_berr_{_s}_dev"] = [H, I, I, _t, I, _t, I, _t, I, PD]


def test_symbols_declared_and_bound():
    assert len(ARGS) == 4
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
    assert _ffi.load().rflu_version() >= 111   # needs no device


def test_source_is_wired_and_documented():
    pkg = os.path.join(ROOT, "recursivefactorization.jl_amd")
    from recursivefactorization.jl_amd import build as B

    assert "refine.hip" in B.SOURCES            # the source list is also what sources_digest() hashes
    src = open(os.path.join(pkg, "csrc", "refine.hip")).read()
    for name in ("absresidual_few_kernel", "absresidual_combine_kernel", "berr_reduce_kernel"):
        assert name in src, name
    import refine_cases as R
    assert f"AR_ROWS = {R.AR_ROWS}, AR_MIN_CJ = {R.AR_MIN_CJ}, AR_TARGET_WGS = {R.AR_TARGET_WGS}" in src   # the restatement's split is the kernel's
    assert f"REFINE_PASS = {R.REFINE_PASS};" in open(os.path.join(pkg, "csrc", "rflu_internal.hpp")).read()
    hdr = open(os.path.join(ROOT, "include", "rflu.h")).read()
    assert "FOUR DELIBERATE DIFFERENCES" in hdr and "safe1 / safe2" in hdr
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "gerfs" in open(os.path.join(ROOT, doc)).read(), doc
    assert "4.13" in open(os.path.join(ROOT, "DESIGN.md")).read()


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
    for name in ("function gerfs_dev!(", "function berr_dev(", "function refine!(F::LU"):
        assert name in src, name


def test_exports():
    for name in ("refine_", "solve_refined", "backward_error"):
        assert name in rf.__all__ and callable(getattr(rf, name))
    assert rf.Refinement._fields == ("ferr", "berr", "steps")


# ---- the refusals of the Python functions: every one of these raises before the library (or a device) is touched
def _lu_of(a):
    return rf.LU(np.asfortranarray(a), rf.NotIPIV(a.shape[0]), 0)


def test_refusals_name_what_is_served():
    a, b = np.asfortranarray(np.eye(3)), np.ones((3, 2), order="F")
    x = b.copy(order="F")
    F = _lu_of(a)
    rowmajor = np.ascontiguousarray(np.arange(9.0).reshape(3, 3))
    for dt in (np.complex128, np.complex64):
        with pytest.raises(TypeError, match="complex"):
            rf.refine_(_lu_of(a.astype(dt)), a.astype(dt), b.astype(dt), x.astype(dt))
        with pytest.raises(TypeError, match="complex"):
            rf.refine_(F, a.astype(dt), b, x)
        with pytest.raises(TypeError, match="complex"):
            rf.backward_error(a.astype(dt), x.astype(dt), b.astype(dt))
    for call in (lambda: rf.refine_(rf.Adjoint(F), a, b, x), lambda: rf.solve_refined(rf.Adjoint(F), a, b)):
        with pytest.raises(TypeError, match="ldiv_"):
            call()
    with pytest.raises(TypeError, match="transposed"):
        rf.backward_error(rf.Adjoint(a), x, b)
    with pytest.raises(ValueError, match="column-major"):
        rf.refine_(rf.LU(rowmajor, rf.NotIPIV(3), 0), a, b, x)              # row-major factors
    with pytest.raises(ValueError, match="column-major"):
        rf.refine_(F, rowmajor, b, x)                                       # row-major A
    with pytest.raises(ValueError, match="column-major"):
        rf.backward_error(rowmajor, x, b)
    mixed = rf.MixedLU.__new__(rf.MixedLU)
    batched = rf.BatchedLU.__new__(rf.BatchedLU)
    for call in (lambda: rf.refine_(mixed, a, b, x), lambda: rf.solve_refined(mixed, a, b)):
        with pytest.raises(TypeError, match="ldiv_mixed"):
            call()
    for call in (lambda: rf.refine_(batched, a, b, x), lambda: rf.solve_refined(batched, a, b)):
        with pytest.raises(TypeError, match="BatchedLU"):
            call()
    with pytest.raises(TypeError):
        rf.refine_(a, a, b, x)                                              # not an LU
    with pytest.raises(rf.SingularException):
        rf.refine_(rf.LU(np.asfortranarray(a), rf.NotIPIV(3), 2), a, b, x)  # a factorization that failed
    with pytest.raises(ValueError):
        rf.refine_(F, a, b, np.ones((3, 3), order="F"))                     # X and B differ in columns
    with pytest.raises(TypeError):
        rf.refine_(F, a, b.astype(np.float32), x)                           # one element type
    with pytest.raises(ValueError):
        rf.backward_error(np.zeros((3, 4)), x, b)
