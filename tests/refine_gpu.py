"""Raw C-ABI calls of rflu_gerfs_* / rflu_berr_* for the -m gpu tests: operands in gpu_util.Store buffers (leading dimension, offset
from a 16-byte boundary, sentinels in the padding), host outputs filled with NaN / -777 before the call."""
import ctypes

import numpy as np
import torch

from gpu_util import Store, handle, ptr, sfx


class Got:
    """X (downloaded), ferr, berr, steps, info, intact (every sentinel of A, F, B, X still there; A, F, B unchanged)"""


def gerfs(A, F, ipiv, B, X, dtype, ferr=True, max_iter=5, h=None, pad=0, off=0, status=False):
    n, nrhs = B.shape
    ld = max(n, 1) + pad
    sa, sf, sb, sx = (Store(np.asarray(M, dtype=dtype), ld, real=dtype, off=off) for M in (A, F, B, X))
    ip = None if ipiv is None else torch.from_numpy(np.ascontiguousarray(ipiv, dtype=np.int64)).to("cuda:0")
    g = Got()
    g.ferr = np.full(nrhs, np.nan) if ferr else None
    g.berr = np.full(nrhs, np.nan)
    steps = np.full(nrhs, -777, dtype=np.intc)
    info = ctypes.c_int64(-1)
    h = h or handle()
    args = (n, nrhs, sa.ptr, ld, sf.ptr, ld, ctypes.c_void_p(0) if ip is None else ptr(ip), sb.ptr, ld, sx.ptr, ld,
            ctypes.c_void_p(g.ferr.ctypes.data if ferr else 0), ctypes.c_void_p(g.berr.ctypes.data), int(max_iter),
            ctypes.c_void_p(steps.ctypes.data), ctypes.byref(info))
    if status:
        return getattr(h.lib, f"rflu_gerfs_{sfx(dtype)}_dev")(h.ptr, *args)
    h.call(f"rflu_gerfs_{sfx(dtype)}_dev", *args)
    g.X, g.steps, g.info = np.array(sx.get(), dtype=dtype), steps.astype(np.int64), int(info.value)
    g.intact = bool(all(s.padding_intact() for s in (sa, sf, sb, sx)) and np.array_equal(sa.get(), np.asarray(A, dtype=dtype), equal_nan=True)
                    and np.array_equal(sf.get(), np.asarray(F, dtype=dtype), equal_nan=True) and np.array_equal(sb.get(), np.asarray(B, dtype=dtype), equal_nan=True))
    return g


def berr(A, X, B, dtype, h=None, pad=0, off=0):
    n, nrhs = B.shape
    ld = max(n, 1) + pad
    sa, sx, sb = (Store(np.asarray(M, dtype=dtype), ld, real=dtype, off=off) for M in (A, X, B))
    out = np.full(nrhs, np.nan)
    (h or handle()).call(f"rflu_berr_{sfx(dtype)}_dev", n, nrhs, sa.ptr, ld, sx.ptr, ld, sb.ptr, ld, ctypes.c_void_p(out.ctypes.data))
    assert all(s.padding_intact() for s in (sa, sx, sb))
    assert np.array_equal(sx.get(), np.asarray(X, dtype=dtype), equal_nan=True)
    return out


def same(a, b):
    """bit for bit, NaN equal to NaN"""
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def same_result(a, b, ferr=True):
    return same(a.X, b.X) and same(a.berr, b.berr) and same(a.steps, b.steps) and a.info == b.info and (not ferr or same(a.ferr, b.ferr))
