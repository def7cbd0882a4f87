"""Batched complex inverse (rflu_getri_batched_cf64_dev / _cf32_dev): one call against what a caller had before.

    microbench_complex_batched_inv.py [--batch 4096] [--reps 9] [--loop 64] [--out profiles/complex_batched_inv_sizes.txt]

For ComplexF64 (n = 8, 16, 32, 64) and ComplexF32 (the same and 128), packed column-major factors of rand + 10 I, in ONE process and
alternating call by call:
  * getri   one rflu_getri_batched_c*_dev call ('N'; 'T' and 'C' are the same arithmetic and another store, timed once each after it);
  * getrs_I rflu_getrs_batched_c*_dev on an explicit identity tensor of the size of the batch.  The identity is refilled before every
            call, outside the timed window (the solve overwrites it); its bytes are counted in the column "I MiB";
  * loop    rflu_getri_c*_dev (the single-matrix complex inverse, in place on a copy) over the first --loop matrices, host-timed
            (every call of that path ends in a stream synchronise) and scaled to the batch.
Microseconds per call: the median of --reps calls, each timed with a pair of events on the handle's stream after two warm-up calls.
GFLOP/s counts 8 n^3 per inverse for both batched routes (what they execute: n right-hand sides through both triangles).  GB/s of
getri: 2 * batch * n^2 * sizeof(element) / time, its one load and one store.  No GPU, no numbers: the script fails."""
import argparse
import ctypes
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from recursivefactorization.jl_amd import _ffi

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--loop", type=int, default=64, help="matrices of the single-matrix loop (scaled to the batch)")
ap.add_argument("--out", default=None, help="also write the table to this file")
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("microbench_complex_batched_inv.py measures an MI355X; no GPU is visible")

SIZES = {"cf64": [8, 16, 32, 64], "cf32": [8, 16, 32, 64, 128]}
h = _ffi.default_handle(0)
stream = torch.cuda.current_stream()
h.set_stream(stream.cuda_stream)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def ptr(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + off)


def event_us(call, before=None):
    if before:
        before()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    call()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def host_us(call, before=None):
    if before:
        before()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    call()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


batch, nloop = args.batch, min(args.loop, args.batch)
say(f"scripts/microbench_complex_batched_inv.py  (batch {batch}, packed column-major factors of rand + 10 I; getri and getrs on an explicit "
    f"identity: median of {args.reps} event-timed calls, alternating; loop: rflu_getri_c*_dev over {nloop} matrices, host-timed, scaled to "
    f"the batch; device {torch.cuda.get_device_name(0)})")
say(f"{'type':6s}{'n':>5s} | {'getri us':>10s}{'GFLOP/s':>9s}{'GB/s':>8s}{'T us':>9s}{'C us':>9s} | {'getrs_I us':>11s}{'GFLOP/s':>9s}{'I MiB':>8s}"
    f"{'x getri':>9s} | {'loop us':>12s}{'x getri':>9s}")
for sfx, ctype, rtype in (("cf64", torch.complex128, torch.float64), ("cf32", torch.complex64, torch.float32)):
    csize = 16 if sfx == "cf64" else 8
    for n in SIZES[sfx]:
        eye = 10 * torch.eye(n, dtype=rtype, device="cuda")
        A = torch.complex(torch.rand((batch, n, n), dtype=rtype, device="cuda") + eye, torch.rand((batch, n, n), dtype=rtype, device="cuda"))
        ipiv = torch.zeros((batch, n), dtype=torch.int64, device="cuda")
        info = torch.zeros(batch, dtype=torch.int64, device="cuda")
        h.call(f"rflu_getrf_batched_{sfx}_dev", batch, n, n, ptr(A), n, n * n, 0, ptr(ipiv), n, 1, ptr(info))
        assert not bool(info.any())
        X = torch.empty_like(A)
        I0 = torch.eye(n, dtype=ctype, device="cuda").expand(batch, n, n).contiguous()
        Y = torch.empty_like(I0)
        W = torch.empty((nloop, n, n), dtype=ctype, device="cuda")
        one = ctypes.c_int64(0)

        def getri(trans=0):
            h.call(f"rflu_getri_batched_{sfx}_dev", batch, n, ptr(A), n, n * n, 0, ptr(ipiv), n, ptr(X), n, n * n, trans, ptr(info))

        def getrs_identity():
            h.call(f"rflu_getrs_batched_{sfx}_dev", batch, n, n, ptr(A), n, n * n, 0, ptr(ipiv), n, ptr(Y), n, n * n, 0)

        def loop():
            for b in range(nloop):
                h.call(f"rflu_getri_{sfx}_dev", n, ptr(W, b * n * n * csize), n, ptr(ipiv, b * n * 8), ctypes.byref(one))

        refill = lambda: Y.copy_(I0)
        recopy = lambda: W.copy_(A[:nloop])
        for _ in range(2):
            event_us(getri)
            event_us(getrs_identity, refill)
        host_us(loop, recopy)
        t_i, t_s, t_l = [], [], []
        for i in range(args.reps):
            t_i.append(event_us(getri))
            t_s.append(event_us(getrs_identity, refill))
            if i < 3:
                t_l.append(host_us(loop, recopy))
        t_i, t_s, t_l = float(np.median(t_i)), float(np.median(t_s)), float(np.median(t_l)) * batch / nloop
        t_t = float(np.median([event_us(lambda: getri(1)) for _ in range(args.reps)]))
        t_c = float(np.median([event_us(lambda: getri(2)) for _ in range(args.reps)]))
        getri()
        assert h.last_path() == _ffi.PATH_HIP_BATCHED and not bool(info.any())
        refill()
        getrs_identity()
        # both routes on the same factors: they agree to rounding (no bit-for-bit claim between two kernels)
        assert (X - Y).abs().amax().item() <= 1000 * n * torch.finfo(rtype).eps * X.abs().amax().item()
        flop = 8.0 * n ** 3 * batch
        say(f"{sfx:6s}{n:5d} | {t_i:10.1f}{flop / t_i / 1e3:9.1f}{2.0 * batch * n * n * csize / t_i / 1e3:8.1f}{t_t:9.1f}{t_c:9.1f} | "
            f"{t_s:11.1f}{flop / t_s / 1e3:9.1f}{batch * n * n * csize / 2 ** 20:8.1f}{t_s / t_i:9.2f} | {t_l:12.0f}{t_l / t_i:9.1f}")
        del A, X, I0, Y, W
h.set_stream(None)
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
