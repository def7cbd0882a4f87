"""-m gpu: the real and the complex logabsdet agree with EACH OTHER, bit for bit (rflu_logabsdet_{f64,f32,cf64,cf32} -- device, host
and batched entries; one kernel source, csrc/inverse.hip).

For a real diagonal d the complex diagonal d + 0i has the moduli |d_i| exactly (hypot(x, 0) = |x|), the logs are added in one order
for both families, and the phase is a product of factors +-1 + 0i, which is exact, as is its renormalisation (a division by 1).  So
logabs is the same Float64 word, sign_re is the real sign and sign_im is zero -- in the single, the host and the batched entry, without
pivots and with an odd and an even number of interchanges.  An exact zero gives (-Inf, 0) and (-Inf, 0 + 0i), a NaN gives NaN in
every output, and so does a NaN that sits in an imaginary part alone.  No tolerance anywhere but in the one guard against two equal
wrong words.

Sizes: 1 and 5 (less than a thread's four entries, one workgroup), 255 / 257 (around one entry per thread), 1024 / 1025 (one chunk, one
chunk and one entry), 2049 (three chunks, a ragged last one).  The diagonal is spread: ld = n + 1, so dstride = n + 2 > 1, and every
word between the diagonal entries holds NaN: a reduction that reads one cannot pass."""
import ctypes
import math
import struct

import numpy as np
import pytest
import torch

from gpu_util import handle

pytestmark = pytest.mark.gpu

SIZES = [1, 5, 255, 257, 1024, 1025, 2049]
REALS = [np.float64, np.float32]
IDS = ["f64", "f32"]
BATCH = 2


def bits(x):
    return struct.pack("<d", float(x))


def diagonal(n, real, seed):
    rng = np.random.default_rng(seed)
    d = ((rng.random(n) - 0.5) * np.exp2(rng.integers(-6, 7, n))).astype(real)
    d[d == 0] = real(0.375)
    return d


def pivot_cases(n):
    """(name, ipiv or None, number of interchanges): ipiv[i] != i + 1 is an interchange"""
    ident = np.arange(1, n + 1, dtype=np.int64)
    odd, even = ident.copy(), ident.copy()
    cases = [("no ipiv", None, 0)]
    if n >= 2:
        odd[0] = n
        cases.append(("odd", odd, 1))
    if n >= 3:
        even[0] = even[1] = n
    cases.append(("even", even, 2 if n >= 3 else 0))
    return cases


class Spread:
    """BATCH diagonals (member b: the diagonal rolled by b) as the diagonals of n x n matrices with ld = n + 1 in a NaN-filled real buffer,
    on the host and on the device; complex when `im` is given (interleaved pairs)"""

    def __init__(self, re, im, real):
        n = len(re)
        self.n, self.ld, self.w = n, n + 1, 1 if im is None else 2
        self.sfx = ("c" if im is not None else "") + ("f64" if real == np.float64 else "f32")
        self.host = np.full(BATCH * n * self.ld * self.w, np.nan, dtype=real)
        v = self.host.reshape(BATCH, n * self.ld, self.w)
        for b in range(BATCH):
            v[b, ::self.ld + 1, 0][:n] = np.roll(re, b)
            if im is not None:
                v[b, ::self.ld + 1, 1][:n] = np.roll(im, b)
        self.dev = torch.from_numpy(self.host).to("cuda:0")

    def words(self, host, ipiv, member=0):
        """(logabs, sign) or (logabs, sign_re, sign_im) of one member through the single-matrix device or host entry"""
        out = [ctypes.c_double(-7.0) for _ in range(1 + self.w)]
        skip = member * self.n * self.ld * self.w * self.host.itemsize
        if host:
            f, p = ctypes.c_void_p(self.host.ctypes.data + skip), (ctypes.c_void_p(ipiv.ctypes.data) if ipiv is not None else None)
        else:
            self._piv = torch.from_numpy(ipiv).to("cuda:0") if ipiv is not None else None
            f, p = ctypes.c_void_p(self.dev.data_ptr() + skip), (ctypes.c_void_p(self._piv.data_ptr()) if ipiv is not None else None)
        handle().call(f"rflu_logabsdet_{self.sfx}" + ("" if host else "_dev"), self.n, f, self.ld, p, *[ctypes.byref(o) for o in out])
        return tuple(o.value for o in out)

    def batched(self, ipiv):
        """the same for every member through the batched entry (every member with the same ipiv)"""
        la = torch.full((BATCH,), -7.0, dtype=torch.float64, device="cuda:0")
        sg = torch.full((BATCH * self.w,), -7.0, dtype=torch.float64, device="cuda:0")
        piv = torch.from_numpy(np.tile(ipiv, BATCH)).to("cuda:0") if ipiv is not None else None
        handle().call(f"rflu_logabsdet_batched_{self.sfx}_dev", BATCH, self.n, ctypes.c_void_p(self.dev.data_ptr()), self.ld, self.n * self.ld,
                      ctypes.c_void_p(piv.data_ptr()) if piv is not None else None, self.n, ctypes.c_void_p(la.data_ptr()),
                      ctypes.c_void_p(sg.data_ptr()))
        la, sg = la.cpu().numpy(), sg.cpu().numpy().reshape(BATCH, self.w)
        return [(la[b],) + tuple(sg[b]) for b in range(BATCH)]

    def everything(self, ipiv):
        """[(entry, member, words)] of the device, host and batched entries"""
        got = [("dev", b, self.words(False, ipiv, b)) for b in range(BATCH)] + [("host", b, self.words(True, ipiv, b)) for b in range(BATCH)]
        return got + [("batched", b, w) for b, w in enumerate(self.batched(ipiv))]


@pytest.mark.parametrize("real", REALS, ids=IDS)
@pytest.mark.parametrize("n", SIZES)
def test_complex_logabsdet_of_an_embedded_real_diagonal_is_the_real_one(n, real):
    d = diagonal(n, real, 4100 + n)
    R, C = Spread(d, None, real), Spread(d, np.zeros_like(d), real)
    logs = np.log(np.abs(d.astype(np.float64)))
    for name, ipiv, swaps in pivot_cases(n):
        what = f"n={n} {R.sfx} {name}"
        la, sg = R.words(False, ipiv)
        # a guard, so that the equalities below are not between two wrong words: n logs, each within an ulp or two, and n additions that
        # each round by at most 2^-53 of a partial sum no larger than sum |log|
        assert abs(la - logs.sum()) <= (n + 4) * 2.0 ** -52 * np.abs(logs).sum(), what
        assert sg == (-1.0) ** (int((d < 0).sum()) + swaps), what
        want = [R.words(False, ipiv, b) for b in range(BATCH)]   # the rolled diagonal: the same entries in other threads and chunks
        assert want[0] == (la, sg)
        for entry, b, w in R.everything(ipiv):
            assert (bits(w[0]), w[1]) == (bits(want[b][0]), want[b][1]), f"real {entry} member {b}, {what}"
        for entry, b, w in C.everything(ipiv):
            assert bits(w[0]) == bits(want[b][0]), f"complex {entry} member {b}: logabs, {what}"
            assert w[1] == want[b][1] and w[2] == 0.0, f"complex {entry} member {b}: sign {w[1:]}, {what}"


@pytest.mark.parametrize("real", REALS, ids=IDS)
@pytest.mark.parametrize("n", SIZES)
def test_an_exact_zero_gives_minus_infinity_and_sign_zero_in_both_families(n, real):
    d = diagonal(n, real, 4200 + n)
    d[n // 2] = 0
    R, C = Spread(d, None, real), Spread(d, np.zeros_like(d), real)
    for name, ipiv, _ in pivot_cases(n):
        for entry, b, w in R.everything(ipiv):
            assert w == (-math.inf, 0.0), f"real {entry} member {b}, n={n} {R.sfx} {name}: {w}"
        for entry, b, w in C.everything(ipiv):
            assert w == (-math.inf, 0.0, 0.0), f"complex {entry} member {b}, n={n} {C.sfx} {name}: {w}"


@pytest.mark.parametrize("real", REALS, ids=IDS)
@pytest.mark.parametrize("n", SIZES)
def test_a_nan_is_kept_in_every_output_also_from_an_imaginary_part_alone(n, real):
    d = diagonal(n, real, 4300 + n)
    k = (2 * n) // 3
    dn = d.copy()
    dn[k] = np.nan
    im = np.zeros_like(d)
    im[k] = np.nan
    for S, name in ((Spread(dn, None, real), "real NaN"), (Spread(dn, np.zeros_like(d), real), "NaN + 0i"), (Spread(d, im, real), "x + i NaN")):
        for pname, ipiv, _ in pivot_cases(n):
            for entry, b, w in S.everything(ipiv):
                assert all(math.isnan(x) for x in w), f"{name}: {entry} member {b}, n={n} {S.sfx} {pname}: {w}"
