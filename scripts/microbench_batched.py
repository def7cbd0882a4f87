"""Batched LU and solve (rflu_getrf_batched_* / rflu_getrs_batched_*): time per call over the sizes the path was written for.

    microbench_batched.py [--n 8 16 32 64 96 128] [--batch 256 4096 65536] [--reps 9] [--out profiles/batched_sizes.txt]

For Float64 and Float32, every n and batch (combinations whose matrices exceed 2 GiB are skipped): the batched factorization and the
batched solve with one right-hand side, packed column-major, on rand + 10 I.  Per case: microseconds per call (median of --reps
repeats, each timed with a pair of events on the handle's stream after two warm-up calls; the factorization works on a fresh copy of
the input every time, the copy is outside the timed window), matrices per second, GFLOP/s at 2 n^3 / 3 per factorization
(2 n^2 per solve), and the effective HBM bandwidth 2 * batch * n^2 * sizeof(T) / time -- the one load and one store, the only traffic
the factorization has.  At batch 256 also the loop over rflu_getrf_*_dev on the same handle: what a caller had without the batched
entry.  No GPU, no numbers: the script fails."""
import argparse
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import recursivefactorization.jl_amd as rf
from recursivefactorization.jl_amd import _ffi

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, nargs="+", default=[8, 16, 32, 64, 96, 128])
ap.add_argument("--batch", type=int, nargs="+", default=[256, 4096, 65536])
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--out", default=None, help="also write the table to this file")
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("microbench_batched.py measures an MI355X; no GPU is visible")

h = _ffi.default_handle(0)
h.set_stream(None)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def ptr(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + off)


def median_us(call, before, stream):
    """median over --reps of the event time of `call`, `before` (restoring the input) outside the window; two warm-up rounds"""
    ts = []
    for i in range(args.reps + 2):
        before()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        e1.synchronize()
        if i >= 2:
            ts.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(ts))


say(f"scripts/microbench_batched.py  (packed column-major, rand + 10 I, median of {args.reps} event-timed calls; device {torch.cuda.get_device_name(0)})")
say(f"{'type':8s}{'n':>5s}{'batch':>8s} | {'getrf us':>10s}{'Mmat/s':>9s}{'GFLOP/s':>10s}{'GB/s':>9s} | {'getrs1 us':>10s}{'Mmat/s':>9s}{'GFLOP/s':>10s} | loop of single getrf (batch 256)")
stream = torch.cuda.current_stream()
h.set_stream(stream.cuda_stream)
for dtype, sfx, esize in ((torch.float64, "f64", 8), (torch.float32, "f32", 4)):
    for n in args.n:
        for batch in args.batch:
            if batch * n * n * esize > 2 << 30:
                say(f"{sfx:8s}{n:5d}{batch:8d} | skipped: the batch exceeds 2 GiB")
                continue
            src = torch.rand((batch, n, n), dtype=dtype, device="cuda") + 10 * torch.eye(n, dtype=dtype, device="cuda")
            A = torch.empty_like(src)
            ipiv = torch.zeros((batch, n), dtype=torch.int64, device="cuda")
            info = torch.zeros(batch, dtype=torch.int64, device="cuda")
            B0 = torch.rand((batch, n), dtype=dtype, device="cuda")
            B = torch.empty_like(B0)

            def getrf():
                h.call(f"rflu_getrf_batched_{sfx}_dev", batch, n, n, ptr(A), n, n * n, 0, ptr(ipiv), n, 1, ptr(info))

            def getrs():
                h.call(f"rflu_getrs_batched_{sfx}_dev", batch, n, 1, ptr(A), n, n * n, 0, ptr(ipiv), n, ptr(B), n, n, 0)

            t_f = median_us(getrf, lambda: A.copy_(src), stream)
            assert h.last_path() == _ffi.PATH_HIP_BATCHED and not bool(info.any())
            t_s = median_us(getrs, lambda: B.copy_(B0), stream)
            # A holds column-major factors of the transposes of `src`'s matrices (a C-contiguous matrix read column-major)
            res = (torch.bmm(src.transpose(1, 2), B.unsqueeze(2)).squeeze(2) - B0).norm(dim=1).max().item()
            assert res < 1000 * n * torch.finfo(dtype).eps, res
            extra = ""
            if batch == 256:
                one = ctypes.c_int64(0)

                def loop():
                    for b in range(batch):
                        h.call(f"rflu_getrf_{sfx}_dev", n, n, ptr(A, b * n * n * esize), n, ptr(ipiv, b * n * 8), 1, 0, ctypes.byref(one))

                t_l = median_us(loop, lambda: A.copy_(src), stream)
                extra = f"{t_l:10.0f} us = {t_l / batch:7.1f} us per matrix, {t_l / t_f:7.1f}x the batched call"
            fl_f, fl_s = 2.0 * n ** 3 / 3.0 * batch, 2.0 * n * n * batch
            say(f"{sfx:8s}{n:5d}{batch:8d} | {t_f:10.1f}{batch / t_f:9.3f}{fl_f / t_f / 1e3:10.1f}{2.0 * batch * n * n * esize / t_f / 1e3:9.1f} | "
                f"{t_s:10.1f}{batch / t_s:9.3f}{fl_s / t_s / 1e3:10.1f} | {extra}")
            del src, A, B, B0
h.set_stream(None)
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
