"""-m gpu: the staging of the host-pointer solve / inverse / determinant entries (csrc/host_entry.cpp: getrs_host, getri_host,
logabsdet_host) with PADDED column strides.  The Python mirror always passes lda = max(n, 1), so only the raw C ABI reaches
lda > n and ldb > n: every entry must give, to the bit, what it gives for lda = ldb = n, and must leave the padding rows alone.
n = 200 crosses three 64-row blocks with a partial last one; NoPivot factors are solved with ipiv = NULL."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from gpu_util import handle, ptr, sfx
from oracle import oracle as O

pytestmark = pytest.mark.gpu

N, NRHS, PAD_A, PAD_B = 200, 3, 3, 5


def hptr(a):
    return ctypes.c_void_p(a.ctypes.data)


@functools.lru_cache(maxsize=None)
def _factors(dtype, pivot):
    """(F, ipiv or None, B): factors of a device factorization, downloaded; shared by the cases and never written."""
    A = O.fill_uniform(N, N, 31, dtype)
    if not pivot:
        A[np.arange(N), np.arange(N)] += 10.0
    dA = torch.from_numpy(np.ascontiguousarray(A.T)).to("cuda:0")     # the column-major image of A
    dip = torch.zeros(N, dtype=torch.int64, device="cuda:0")
    info = ctypes.c_int64(-1)
    handle().call(f"rflu_getrf_{sfx(dtype)}_dev", N, N, ptr(dA), N, ptr(dip) if pivot else None, int(pivot), 0, ctypes.byref(info))
    assert info.value == 0
    F = np.asfortranarray(dA.cpu().numpy().T)
    ipiv = dip.cpu().numpy() if pivot else None
    B = np.asfortranarray(O.fill_uniform(N, NRHS, 32, dtype))
    for a in (F, B) + ((ipiv,) if pivot else ()):
        a.setflags(write=False)
    return F, ipiv, B


def _padded(X, pad):
    P = np.full((X.shape[0] + pad, X.shape[1]), np.nan, dtype=X.dtype, order="F")
    P[:X.shape[0], :] = X
    return P


def _same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


@pytest.mark.parametrize("pivot", [True, False], ids=["ipiv", "null_ipiv"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("entry", ["getrs", "getrs_trans"])
def test_host_solve_with_padded_strides(entry, dtype, pivot):
    F, ipiv, B = _factors(dtype, pivot)
    ip = hptr(ipiv) if pivot else None
    name = f"rflu_{entry}_{sfx(dtype)}"
    Ft, Bt = F.copy(order="F"), B.copy(order="F")
    handle().call(name, N, NRHS, hptr(Ft), N, ip, hptr(Bt), N)
    Fp, Bp = _padded(F, PAD_A), _padded(B, PAD_B)
    handle().call(name, N, NRHS, hptr(Fp), N + PAD_A, ip, hptr(Bp), N + PAD_B)
    assert np.isfinite(Bt).all() and not _same_bits(Bt, B)
    assert _same_bits(Bp[:N], Bt)
    assert np.isnan(Bp[N:]).all() and np.isnan(Fp[N:]).all()
    assert _same_bits(Fp[:N], F) and _same_bits(Ft, F)     # the factors are read only


@pytest.mark.parametrize("pivot", [True, False], ids=["ipiv", "null_ipiv"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_host_inverse_with_a_padded_stride(dtype, pivot):
    F, ipiv, _ = _factors(dtype, pivot)
    ip = hptr(ipiv) if pivot else None
    name = f"rflu_getri_{sfx(dtype)}"
    Ft, info = F.copy(order="F"), ctypes.c_int64(-1)
    handle().call(name, N, hptr(Ft), N, ip, ctypes.byref(info))
    assert info.value == 0
    Fp, info = _padded(F, PAD_A), ctypes.c_int64(-1)
    handle().call(name, N, hptr(Fp), N + PAD_A, ip, ctypes.byref(info))
    assert info.value == 0
    assert np.isfinite(Ft).all() and not _same_bits(Ft, F)
    assert _same_bits(Fp[:N], Ft)
    assert np.isnan(Fp[N:]).all()


@pytest.mark.parametrize("pivot", [True, False], ids=["ipiv", "null_ipiv"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_host_logabsdet_with_a_padded_stride(dtype, pivot):
    F, ipiv, _ = _factors(dtype, pivot)
    ip = hptr(ipiv) if pivot else None
    name = f"rflu_logabsdet_{sfx(dtype)}"

    def run(M, ld):
        la, sg = ctypes.c_double(np.nan), ctypes.c_double(np.nan)
        handle().call(name, N, hptr(M), ld, ip, ctypes.byref(la), ctypes.byref(sg))
        return la.value, sg.value

    Fp = _padded(F, PAD_A)
    tight, padded = run(F, N), run(Fp, N + PAD_A)
    assert np.isfinite(tight[0]) and tight[1] in (1.0, -1.0)
    assert np.float64(padded[0]).tobytes() == np.float64(tight[0]).tobytes() and padded[1] == tight[1]
    assert np.isnan(Fp[N:]).all() and _same_bits(Fp[:N], F)
