"""sha1 of what the batched entries (rflu_getrf_batched_*, rflu_getrs_batched_*, rflu_getri_batched_*) write, one line per case: factors
(the whole buffer, padding included), ipiv, info, the solutions for nrhs = 1, 8, 9, 17 and every trans the element accepts, and for
real elements the inverse.  Two builds that claim identical arithmetic print identical lines.  Inputs come from NumPy with fixed seeds;
batch 5, so that a workgroup holds groups beyond the end of the batch.  usage: [RFLU_LIB=...] python scripts/batched_checksum.py"""
import ctypes, hashlib, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from recursivefactorization.jl_amd import _ffi

h = _ffi.Handle(0); h.set_stream(None)
BATCH, PAD = 5, 3
ELEMENTS = (("f64", np.float64, 128), ("f32", np.float32, 128), ("cf64", np.complex128, 64), ("cf32", np.complex64, 128))
SHAPES = [(n, n) for n in (1, 7, 32, 33, 64, 65, 100, 128)] + [(10, 12), (100, 60), (60, 100)]


def sha(*ts):
    d = hashlib.sha1()
    for t in ts:
        d.update(t.cpu().numpy().tobytes())
    return d.hexdigest()[:16]


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def rand(rng, dt, *shape):
    a = rng.uniform(-1.0, 1.0, shape)
    return (a + 1j * rng.uniform(-1.0, 1.0, shape)).astype(dt) if np.iscomplexobj(dt()) else a.astype(dt)


def image(M, row_major, ld):
    """(batch, rows, cols) -> the strided buffer the library reads: (batch, lines, ld), a line = a column (or a row if row_major)"""
    L = M if row_major else M.transpose(0, 2, 1)
    buf = np.full((L.shape[0], L.shape[1], ld), 7, dtype=M.dtype)
    buf[:, :, :L.shape[2]] = L
    return torch.from_numpy(buf).cuda()


def case(sfx, dt, m, n, row_major, pad, pivot, special):
    rng = np.random.RandomState(1000 * m + n + (77 if special else 0))
    M = rand(rng, dt, BATCH, m, n)
    if special:   # a tied column, a zero column, a NaN
        M[1, 5, 0] = M[1, 2, 0] = 3; M[1, 9, 4] = -M[1, 6, 4]; M[2, :, 3] = 0; M[3, 4, 2] = np.nan
    lda = (n if row_major else m) + pad
    A = image(M, row_major, lda)
    mn = min(m, n)
    ipiv = torch.zeros((BATCH, mn), dtype=torch.int64, device="cuda") if pivot else None
    info = torch.full((BATCH,), -1, dtype=torch.int64, device="cuda")
    h.call(f"rflu_getrf_batched_{sfx}_dev", BATCH, m, n, ptr(A), lda, A[0].numel(), row_major, ptr(ipiv), mn, pivot, ptr(info))
    assert h.last_path() == _ffi.PATH_HIP_BATCHED
    line = f"{sfx} {m}x{n} {'rm' if row_major else 'cm'} lda={lda} pivot={pivot}{' special' if special else ''}: factors {sha(A)} ipiv {sha(ipiv) if pivot else '-'} info {sha(info)}"
    if m == n:
        sols = []
        for nrhs in (1, 8, 9, 17):
            X0 = rand(rng, dt, BATCH, n, nrhs)
            ldb = (nrhs if row_major else n) + pad
            for trans in range(3 if sfx[0] == "c" else 2):
                B = image(X0, row_major, ldb)
                h.call(f"rflu_getrs_batched_{sfx}_dev", BATCH, n, nrhs, ptr(A), lda, A[0].numel(), row_major, ptr(ipiv), n, ptr(B), ldb, B[0].numel(), trans)
                sols.append(B)
        line += f" solutions {sha(*sols)}"
        if sfx[0] != "c":
            Y = image(np.zeros((BATCH, n, n), dtype=dt), row_major, lda)
            info.fill_(-1)
            h.call(f"rflu_getri_batched_{sfx}_dev", BATCH, n, ptr(A), lda, A[0].numel(), row_major, ptr(ipiv), n, ptr(Y), lda, Y[0].numel(), ptr(info))
            line += f" inverse {sha(Y, info)}"
    print(line, flush=True)


for sfx, dt, lim in ELEMENTS:
    for m, n in SHAPES:
        if max(m, n) > lim:
            continue
        for row_major in (0, 1):
            for pad in (0, PAD):
                for pivot in (0, 1):
                    case(sfx, dt, m, n, row_major, pad, pivot, False)
    for n in (33, 64):
        for row_major in (0, 1):
            case(sfx, dt, n, n, row_major, 0, 1, True)
