"""-m gpu: the real and the complex operator norms agree with EACH OTHER, bit for bit (rflu_lange_{f64,f32,cf64,cf32}_dev and their
batched entries; one kernel source, csrc/condest.hip).

For a real matrix A the complex matrices A + 0i and 0 + iA have the moduli |a| exactly (hypot(x, 0) = hypot(0, x) = |x|), and the
kernels add them in the order they add a real matrix, so the three norms are the same Float64 word -- whatever the layout, the norm,
the pointer's alignment and the padding, and in the batched entry as in the single one.  No tolerance anywhere.

Shapes: the smallest that reach every path -- 5x3 / 3x5 (less than a quad, one workgroup), 33x7 (a ragged quad), 130x129 (above the
one-workgroup batched limit of 128), 1030x3 / 3x1030 (two chunks of 1024 in a line, a ragged last quad; 1030 positions across), 300x260
(two groups of 256 lines, two blocks of 256 sums).  Padding holds NaN: a norm that reads it cannot pass."""
import ctypes
import math
import struct

import numpy as np
import pytest
import torch

from gpu_util import handle, ptr

pytestmark = pytest.mark.gpu

SHAPES = [(5, 3), (3, 5), (33, 7), (130, 129), (1030, 3), (3, 1030), (300, 260)]
REALS = [np.float64, np.float32]
IDS = ["f64", "f32"]
NORMS = [1, 2]   # RFLU_NORM_ONE, RFLU_NORM_INF
SMALL = 128      # the batched entry runs one workgroup per matrix up to this max(m, n)


def bits(x):
    return struct.pack("<d", float(x))


def tdt(real):
    return torch.float64 if real == np.float64 else torch.float32


def layouts(length):
    """(off, ld): `off` real words between a 16-byte boundary and the matrix, ld in elements.  ld4 is padded and a multiple of 4, so with
    off = 0 every line of every element type starts on a 16-byte boundary (the 16-byte loads); ld4 + 1 leaves that to ComplexF64 alone;
    off = 1 takes it from all four."""
    ld4 = (length + 3) // 4 * 4 + 4
    return [(0, ld4), (0, ld4 + 1), (1, ld4)]


def lines_of(A, row_major):
    return np.ascontiguousarray(A if row_major else A.T)


def real_store(lines, ld, off, real, batch=1, stride=0):
    """the lines (batch x cnt x len, or cnt x len) in a NaN-filled real buffer; returns the tensor whose data_ptr is element 0"""
    lines = lines.reshape((batch,) + lines.shape[-2:])
    cnt, length = lines.shape[-2:]
    stride = stride or cnt * ld
    buf = torch.full((off + batch * stride + 8,), math.nan, dtype=tdt(real), device="cuda:0")
    src = torch.from_numpy(lines).to("cuda:0")
    for b in range(batch):
        buf[off + b * stride:off + b * stride + cnt * ld].view(cnt, ld)[:, :length] = src[b]
    return buf[off:]


def cplx_store(re, im, ld, off, real, batch=1, stride=0):
    """the same for the complex matrix re + i im: interleaved pairs, ld and stride in complex elements, off in real words"""
    re, im = (x.reshape((batch,) + x.shape[-2:]) for x in (re, im))
    cnt, length = re.shape[-2:]
    stride = stride or cnt * ld
    buf = torch.full((off + 2 * batch * stride + 8,), math.nan, dtype=tdt(real), device="cuda:0")
    pair = torch.from_numpy(np.stack([re, im], axis=-1)).to("cuda:0")
    for b in range(batch):
        buf[off + 2 * b * stride:off + 2 * (b * stride + cnt * ld)].view(cnt, ld, 2)[:, :length, :] = pair[b]
    return buf[off:]


def lange(sfx, t, norm, m, n, ld, row_major):
    out = ctypes.c_double(-1.0)
    handle().call(f"rflu_lange_{sfx}_dev", norm, m, n, ptr(t), ld, row_major, ctypes.byref(out))
    return out.value


def lange_batched(sfx, t, norm, batch, m, n, ld, stride, row_major):
    out = torch.full((batch,), -1.0, dtype=torch.float64, device="cuda:0")
    handle().call(f"rflu_lange_batched_{sfx}_dev", norm, batch, m, n, ptr(t), ld, stride, row_major, ptr(out))
    return out.cpu().numpy()


def matrix(shape, real, seed):
    rng = np.random.default_rng(seed)
    return ((rng.random(shape) - 0.5) * np.exp2(rng.integers(-6, 7, shape))).astype(real)


@pytest.mark.parametrize("real", REALS, ids=IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_complex_norm_of_an_embedded_real_matrix_is_the_real_norm(shape, real):
    m, n = shape
    sr, sc = ("f64", "cf64") if real == np.float64 else ("f32", "cf32")
    A = matrix(shape, real, 100 * m + n)
    zero = np.zeros_like
    for row_major in (0, 1):
        L = lines_of(A, row_major)
        expect = {1: np.abs(A.astype(np.float64)).sum(axis=0).max(), 2: np.abs(A.astype(np.float64)).sum(axis=1).max()}
        for off, ld in layouts(L.shape[1]):
            tr = real_store(L, ld, off, real)
            t0 = cplx_store(L, zero(L), ld, off, real)
            ti = cplx_store(zero(L), L, ld, off, real)
            for norm in NORMS:
                what = f"{m}x{n} {sr} row_major={row_major} norm={norm} off={off} ld={ld}"
                r = lange(sr, tr, norm, m, n, ld, row_major)
                # a guard, so that the equalities below are not between two wrong words: two Float64 sums of at most 1030 non-negative
                # terms in different orders differ by less than 2 * 1030 * 2^-53 = 2.3e-13 of the sum
                assert math.isfinite(r) and abs(r - expect[norm]) <= 1e-12 * expect[norm], what
                assert bits(lange(sc, t0, norm, m, n, ld, row_major)) == bits(r), f"A + 0i, {what}"
                assert bits(lange(sc, ti, norm, m, n, ld, row_major)) == bits(r), f"0 + iA, {what}"


@pytest.mark.parametrize("real", REALS, ids=IDS)
@pytest.mark.parametrize("shape", [s for s in SHAPES if max(s) <= SMALL], ids=lambda s: f"{s[0]}x{s[1]}")
def test_batched_complex_norm_is_the_single_real_norm(shape, real):
    m, n = shape
    sr, sc = ("f64", "cf64") if real == np.float64 else ("f32", "cf32")
    batch = 3
    As = [matrix(shape, real, 1000 * m + 10 * n + b) for b in range(batch)]
    for row_major in (0, 1):
        L = np.stack([lines_of(A, row_major) for A in As])
        cnt, length = L.shape[1:]
        for off, ld in layouts(length):
            stride = cnt * ld + 3   # odd: the members start at every alignment
            tr = real_store(L, ld, off, real, batch, stride)
            t0 = cplx_store(L, np.zeros_like(L), ld, off, real, batch, stride)
            ti = cplx_store(np.zeros_like(L), L, ld, off, real, batch, stride)
            for norm in NORMS:
                what = f"{m}x{n} {sr} row_major={row_major} norm={norm} off={off} ld={ld}"
                single = [lange(sr, tr[b * stride:], norm, m, n, ld, row_major) for b in range(batch)]
                assert all(math.isfinite(v) and v > 0.0 for v in single), what
                for name, got in (("real batched", lange_batched(sr, tr, norm, batch, m, n, ld, stride, row_major)),
                                  ("A + 0i batched", lange_batched(sc, t0, norm, batch, m, n, ld, stride, row_major)),
                                  ("0 + iA batched", lange_batched(sc, ti, norm, batch, m, n, ld, stride, row_major))):
                    assert [bits(v) for v in got] == [bits(v) for v in single], f"{name}, {what}"


@pytest.mark.parametrize("real", REALS, ids=IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_nan_in_an_imaginary_part_alone_is_kept(shape, real):
    """a NaN only in an imaginary part gives NaN, and Inf + i NaN gives NaN, not Inf: in the last element (a ragged quad) and inside"""
    m, n = shape
    sc = "cf64" if real == np.float64 else "cf32"
    A = matrix(shape, real, 7 * m + n)
    for (i, j) in ((m - 1, n - 1), (m // 2, n // 3)):
        for re_part in (A[i, j], np.inf):
            Re, Im = A.copy(), np.zeros_like(A)
            Re[i, j], Im[i, j] = re_part, np.nan
            for row_major in (0, 1):
                Lr, Li = lines_of(Re, row_major), lines_of(Im, row_major)
                for off, ld in layouts(Lr.shape[1]):
                    t = cplx_store(Lr, Li, ld, off, real)
                    for norm in NORMS:
                        what = f"{m}x{n} {sc} ({re_part}, NaN) at ({i}, {j}) row_major={row_major} norm={norm} off={off} ld={ld}"
                        assert math.isnan(lange(sc, t, norm, m, n, ld, row_major)), what
                        if max(m, n) <= SMALL:
                            assert math.isnan(lange_batched(sc, t, norm, 1, m, n, ld, Lr.shape[0] * ld, row_major)[0]), f"batched, {what}"
