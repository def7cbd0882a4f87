"""Batched complex LU and solve (rflu_getrf_batched_cf* / rflu_getrs_batched_cf*): one batched call against what a caller had before.

    microbench_complex_batched.py [--batch 4096] [--reps 9] [--loop-reps 3] [--out profiles/complex_batched_sizes.txt]

For ComplexF64 (n = 8, 16, 32, 64) and ComplexF32 (the same and 96, 128), packed column-major, rand + 10 I, in ONE process:
  * the batched factorization, the batched solve with 1 and with 8 right-hand sides ('N'; 'T' and 'C' run the same kernel by rows):
    microseconds per call, the median of --reps calls, each timed with a pair of events on the handle's stream after two warm-up calls
    (the factorization works on a fresh copy of the input every time; the copy is outside the timed window);
  * the loop over the single-matrix complex device path on the same handle and the same matrices (rflu_getrf_c*_dev, rflu_getrs_c*_dev),
    host-timed around the loop (every call of that path ends in a stream synchronise), the median of --loop-reps loops after one
    warm-up loop, batched calls and loops alternating;
  * for the factorization, the real batched kernel of the same precision on the real parts of the same matrices; a complex
    factorization is 4 x the real flop count (8 n^3 / 3 against 2 n^3 / 3), so "x real" = 4 means the same arithmetic rate.
GFLOP/s: 8 n^3 / 3 per factorization, 8 n^2 nrhs per solve.  GB/s: 2 * batch * n^2 * sizeof(element) / time, the one load and one
store of the factorization.  No GPU, no numbers: the script fails."""
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
ap.add_argument("--loop-reps", type=int, default=3)
ap.add_argument("--out", default=None, help="also write the table to this file")
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("microbench_complex_batched.py measures an MI355X; no GPU is visible")

SIZES = {"cf64": [8, 16, 32, 64], "cf32": [8, 16, 32, 64, 96, 128]}
h = _ffi.default_handle(0)
stream = torch.cuda.current_stream()
h.set_stream(stream.cuda_stream)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def ptr(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + off)


def event_us(call, before):
    before()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    call()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def host_us(call, before):
    before()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    call()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


def alternate(batched, loop, before):
    """(median us of the batched call, median us of the loop): warm-ups first, then the two alternating"""
    for _ in range(2):
        event_us(batched, before)
    host_us(loop, before)
    tb, tl = [], []
    for i in range(max(args.reps, args.loop_reps)):
        if i < args.reps:
            tb.append(event_us(batched, before))
        if i < args.loop_reps:
            tl.append(host_us(loop, before))
    return float(np.median(tb)), float(np.median(tl))


batch = args.batch
say(f"scripts/microbench_complex_batched.py  (batch {batch}, packed column-major, rand + 10 I; batched: median of {args.reps} event-timed "
    f"calls; loop over the single-matrix complex path: median of {args.loop_reps} host-timed loops; device {torch.cuda.get_device_name(0)})")
say(f"{'type':6s}{'n':>5s} | {'getrf us':>10s}{'GFLOP/s':>9s}{'GB/s':>8s}{'loop us':>12s}{'ratio':>8s}{'real us':>10s}{'x real':>8s} | "
    f"{'getrs1 us':>10s}{'GFLOP/s':>9s}{'loop us':>12s}{'ratio':>8s} | {'getrs8 us':>10s}{'GFLOP/s':>9s}{'loop us':>12s}{'ratio':>8s}")
for sfx, ctype, rtype, rsfx in (("cf64", torch.complex128, torch.float64, "f64"), ("cf32", torch.complex64, torch.float32, "f32")):
    csize = 16 if sfx == "cf64" else 8
    for n in SIZES[sfx]:
        eye = 10 * torch.eye(n, dtype=rtype, device="cuda")
        src = torch.complex(torch.rand((batch, n, n), dtype=rtype, device="cuda") + eye, torch.rand((batch, n, n), dtype=rtype, device="cuda"))
        A = torch.empty_like(src)
        ipiv = torch.zeros((batch, n), dtype=torch.int64, device="cuda")
        info = torch.zeros(batch, dtype=torch.int64, device="cuda")
        one = ctypes.c_int64(0)

        def getrf():
            h.call(f"rflu_getrf_batched_{sfx}_dev", batch, n, n, ptr(A), n, n * n, 0, ptr(ipiv), n, 1, ptr(info))

        def getrf_loop():
            for b in range(batch):
                h.call(f"rflu_getrf_{sfx}_dev", n, n, ptr(A, b * n * n * csize), n, ptr(ipiv, b * n * 8), 1, ctypes.byref(one))

        t_f, t_fl = alternate(getrf, getrf_loop, lambda: A.copy_(src))
        A.copy_(src)
        getrf()
        assert h.last_path() == _ffi.PATH_HIP_BATCHED and not bool(info.any())
        # the real batched kernel of the same precision on the real parts
        rsrc = src.real.contiguous()
        RA = torch.empty_like(rsrc)

        def getrf_real():
            h.call(f"rflu_getrf_batched_{rsfx}_dev", batch, n, n, ptr(RA), n, n * n, 0, ptr(ipiv), n, 1, ptr(info))

        for _ in range(2):
            event_us(getrf_real, lambda: RA.copy_(rsrc))
        t_r = float(np.median([event_us(getrf_real, lambda: RA.copy_(rsrc)) for _ in range(args.reps)]))
        A.copy_(src)
        getrf()      # A and ipiv hold the complex factors again
        row = (f"{sfx:6s}{n:5d} | {t_f:10.1f}{8.0 * n ** 3 / 3.0 * batch / t_f / 1e3:9.1f}{2.0 * batch * n * n * csize / t_f / 1e3:8.1f}"
               f"{t_fl:12.0f}{t_fl / t_f:8.1f}{t_r:10.1f}{t_f / t_r:8.2f} |")
        for nrhs in (1, 8):
            B0 = torch.complex(torch.rand((batch, nrhs, n), dtype=rtype, device="cuda"), torch.rand((batch, nrhs, n), dtype=rtype, device="cuda"))
            B = torch.empty_like(B0)    # (batch, nrhs, n) C-contiguous: column-major n x nrhs right-hand sides

            def getrs():
                h.call(f"rflu_getrs_batched_{sfx}_dev", batch, n, nrhs, ptr(A), n, n * n, 0, ptr(ipiv), n, ptr(B), n, n * nrhs, 0)

            def getrs_loop():
                for b in range(batch):
                    h.call(f"rflu_getrs_{sfx}_dev", n, nrhs, ptr(A, b * n * n * csize), n, ptr(ipiv, b * n * 8), ptr(B, b * n * nrhs * csize), n)

            t_s, t_sl = alternate(getrs, getrs_loop, lambda: B.copy_(B0))
            B.copy_(B0)
            getrs()
            # A holds column-major factors of the transposes of `src`'s matrices (a C-contiguous matrix read column-major)
            res = (torch.bmm(src.transpose(1, 2), B.transpose(1, 2)) - B0.transpose(1, 2)).abs().amax().item()
            assert res < 1000 * n * torch.finfo(rtype).eps, res
            row += f" {t_s:10.1f}{8.0 * n * n * nrhs * batch / t_s / 1e3:9.1f}{t_sl:12.0f}{t_sl / t_s:8.1f} |"
            del B, B0
        say(row)
        del src, A, rsrc, RA
h.set_stream(None)
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
