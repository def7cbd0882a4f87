"""opnorm / rcond / cond through the layers that can be checked without a GPU: the 16 symbols in include/rflu.h with the argument lists
the interface fixes, their ctypes bindings, the exports of the built library, the Julia ccalls, the source list of the build, and the
argument checks the Python mirror makes BEFORE it touches the library."""
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
for _s, _t in (("f64", "double*"), ("f32", "float*")):
    ARGS[f"rflu_lange_{_s}_dev"] = [H, N, I, I, _t, I, N, PD]
    ARGS[f"rflu_lange_batched_{_s}_dev"] = [H, N, I, I, I, _t, I, I, N, PD]
    ARGS[f"rflu_gecon_{_s}_dev"] = [H, N, I, _t, I, D, PD]
    ARGS[f"rflu_gecon_rm_{_s}_dev"] = [H, N, I, _t, I, D, PD]
    ARGS[f"rflu_gecon_{_s}"] = [H, N, I, _t, I, D, PD]
    ARGS[f"rflu_gecon_batched_{_s}_dev"] = [H, N, I, I, _t, I, I, N, PD, PD]


def test_symbols_declared_and_bound():
    assert len(ARGS) == 12
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
    assert (_ffi.NORM_ONE, _ffi.NORM_INF) == (1, 2)


def test_library_exports_the_symbols_and_the_version():
    assert os.path.exists(_ffi.LIB_PATH), "librflu.so has not been built (build() comes first)"
    out = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for sym in ARGS:
        assert sym in exported, sym
    assert _ffi.load().rflu_version() >= 109   # needs no device


def test_source_is_wired_and_documented():
    pkg = os.path.join(ROOT, "recursivefactorization.jl_amd")
    from recursivefactorization.jl_amd import build as B

    assert "condest.hip" in B.SOURCES            # the source list is also what sources_digest() hashes
    assert os.path.exists(os.path.join(pkg, "csrc", "condest.hip"))
    assert "gecon_batched_kernel" in open(os.path.join(pkg, "csrc", "batched.hip")).read()
    hdr = open(os.path.join(ROOT, "include", "rflu.h")).read()
    assert "TWO DELIBERATE DIFFERENCES" in hdr and "(-1)^i (n - 1 + i)" in hdr     # the header states both changes to xLACN2
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "rflu_gecon" in open(os.path.join(ROOT, doc)).read(), doc
    assert "4.11" in open(os.path.join(ROOT, "DESIGN.md")).read()


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
    for name in ("function lange_dev(", "function gecon_dev!(", "function gecon_batched_dev!(", "function rcond(F::LU"):
        assert name in src, name


def test_exports():
    for name in ("opnorm", "rcond", "cond", "opnorm_batched", "rcond_batched", "cond_batched"):
        assert name in rf.__all__ and callable(getattr(rf, name))


# ---- the argument rules of the Python functions: every one of these raises before the library (or a device) is touched
def _lu_of(a):
    return rf.LU(np.asfortranarray(a), rf.NotIPIV(a.shape[0]), 0)


@pytest.mark.parametrize("p", [2, 0, "fro", "1", None, True, -1, math.nan])
def test_p_must_be_one_or_inf(p):
    a = np.eye(3)
    for call in (lambda: rf.opnorm(a, p), lambda: rf.rcond(_lu_of(a), 1.0, p), lambda: rf.cond(a, p)):
        with pytest.raises(ValueError):
            call()


def test_complex_is_not_served_yet():
    for dt in (np.complex128, np.complex64):
        a = np.eye(3, dtype=dt)
        for call in (lambda: rf.opnorm(a), lambda: rf.rcond(_lu_of(a), 1.0), lambda: rf.cond(a)):
            with pytest.raises(TypeError, match="complex"):
                call()


def test_shape_and_type_rules():
    with pytest.raises(ValueError):
        rf.rcond(rf.LU(np.zeros((3, 4), order="F"), rf.NotIPIV(3), 0), 1.0)          # non-square factors, as inv_
    with pytest.raises(ValueError):
        rf.cond(np.zeros((3, 4)))
    with pytest.raises(ValueError):
        rf.opnorm(np.zeros(3))
    with pytest.raises(TypeError):
        rf.rcond(np.eye(3), 1.0)                                                         # not an LU
    with pytest.raises(ValueError):
        rf.rcond(_lu_of(np.eye(3)), -1.0)                                                # anorm < 0
    with pytest.raises(TypeError):
        rf.rcond(rf.Adjoint(rf.Adjoint(_lu_of(np.eye(3)))), 1.0)
    with pytest.raises(TypeError):
        rf.opnorm(np.eye(3, dtype=np.int64))
    with pytest.raises(TypeError):
        rf.opnorm_batched(np.zeros((2, 3, 3)))                                           # a batch lives on the device
    with pytest.raises(TypeError):
        rf.rcond_batched(_lu_of(np.eye(3)), None)                                        # not a BatchedLU
    with pytest.raises(ValueError):
        rf.cond_batched(np.zeros((2, 3, 3)))
    # the empty matrix needs no device
    assert rf.opnorm(np.zeros((0, 3))) == 0.0
    assert rf.rcond(_lu_of(np.zeros((0, 0))), 1.0) == 1.0
    assert rf.cond(np.zeros((0, 0))) == 1.0
