"""sha1 of what the inv / logabsdet entries write, one line per case: rflu_getri_*_dev (with and without ipiv), rflu_getri_rm_*_dev
(real), rflu_getri_* (host), rflu_getri_batched_*_dev above the one-launch limit (complex: trans 0 / 1 / 2), rflu_logabsdet_* (dev, host,
batched), for f64, f32, cf64, cf32.  Hashed: the whole output buffer with its padding, info, the logabsdet words.  Two builds that claim
identical arithmetic print identical lines.  The "factors" are NumPy arrays with fixed seeds (any matrix with a nonzero diagonal is a
packed LU; ipiv[i] is drawn from [i + 1, n]), every getri case three ways: lda = n, lda = n + 3, and a pointer one real word off a
16-byte boundary.  usage: [RFLU_LIB=...] python scripts/inv_checksum.py"""
import ctypes, hashlib, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from recursivefactorization.jl_amd import _ffi

h = _ffi.Handle(0); h.set_stream(None)
ELEMENTS = (("f64", np.float64, np.float64), ("f32", np.float32, np.float32), ("cf64", np.complex128, np.float64), ("cf32", np.complex64, np.float32))
GETRI_N = (1, 63, 64, 65, 129, 513, 577, 1100)     # one block, the 64-row edges, W + 1, a ragged second block column, 2 W + 76
LOGABSDET_N = GETRI_N + (1023, 1024, 1025, 2049)   # ... and the chunk edges of the reduction
LAYOUTS = ((0, 0), (3, 0), (3, 1))                 # (lda - n, real words between a 16-byte boundary and the matrix)
FILL = 7.0


def sha(*xs):
    d = hashlib.sha1()
    for x in xs:
        d.update((x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)).tobytes())
    return d.hexdigest()[:16]


def factors(n, dt, seed, special=None):
    """n x n: the element (i, j) of the packed factors at [i, j]; |u_ii| in [1/2, 3/2), the rest scaled so that the inverse stays tame"""
    rng = np.random.RandomState(seed)
    cplx = np.iscomplexobj(dt())
    draw = lambda: rng.uniform(-1.0, 1.0, (n, n)) + (1j * rng.uniform(-1.0, 1.0, (n, n)) if cplx else 0.0)
    F = draw() / np.sqrt(n)
    d = draw().diagonal()
    F[np.arange(n), np.arange(n)] = d / np.abs(d) * rng.uniform(0.5, 1.5, n)
    if special == "zero":
        F[2, 2] = 0
    if special == "nan":
        F[n // 2, n // 3] = np.nan
        F[n - 2, n - 2] = complex(0.75, np.nan) if cplx else np.nan   # complex: in an imaginary part alone
    ipiv = np.array([rng.randint(i + 1, n + 1) for i in range(n)], dtype=np.int64)
    return F.astype(dt), ipiv


def store(F, ld, off, rt, lines_are_columns=True, batch=1):
    """`batch` copies of F, column-major (or row-major) with leading dimension ld, in a FILL-ed real buffer whose first word is on a 16-byte
    boundary and whose word `off` is element 0: (the buffer, its (batch, n, ld) view in F's type)"""
    n = F.shape[0]
    words = batch * n * ld * (2 if np.iscomplexobj(F) else 1)
    raw = np.full(off + words + 2 + 4, FILL, dtype=rt)
    a = (-raw.ctypes.data // raw.itemsize) % (16 // raw.itemsize)
    buf = raw[a:a + off + words + 2]
    body = buf[off:off + words].view(F.dtype).reshape(batch, n, ld)
    body[:, :, :n] = F.T if lines_are_columns else F
    return buf, body


def dev(buf, body):
    t = torch.from_numpy(buf).cuda()
    assert t.data_ptr() % 16 == 0
    return t, ctypes.c_void_p(t.data_ptr() + body.ctypes.data - buf.ctypes.data)


def host_ptr(body):
    return ctypes.c_void_p(body.ctypes.data)


def tptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def logabsdet_words(sfx, call):
    out = [ctypes.c_double(-7.0) for _ in range(3 if sfx[0] == "c" else 2)]
    call(*[ctypes.byref(o) for o in out])
    return np.array([o.value for o in out])


def getri_cases(sfx, dt, rt, n, special=None):
    F, ipiv = factors(n, dt, 100 + n, special)
    dipiv = torch.from_numpy(ipiv).cuda()
    tag = f"{sfx} n={n}{' ' + special if special else ''}"
    for pad, off in LAYOUTS:
        ld = n + pad
        where = f"{tag} lda={ld} off={off}"
        for piv in (dipiv, None):
            info = ctypes.c_int64(-1)
            t, p = dev(*store(F, ld, off, rt))
            h.call(f"rflu_getri_{sfx}_dev", n, p, ld, tptr(piv), ctypes.byref(info))
            print(f"getri_dev {where} ipiv={'yes' if piv is not None else 'no'}: {sha(t)} info {info.value}", flush=True)
        if sfx[0] != "c":
            info = ctypes.c_int64(-1)
            t, p = dev(*store(F, ld, off, rt, lines_are_columns=False))
            h.call(f"rflu_getri_rm_{sfx}_dev", n, p, ld, tptr(dipiv), ctypes.byref(info))
            print(f"getri_rm_dev {where}: {sha(t)} info {info.value}", flush=True)
        info = ctypes.c_int64(-1)
        buf, body = store(F, ld, off, rt)
        h.call(f"rflu_getri_{sfx}", n, host_ptr(body), ld, ctypes.c_void_p(ipiv.ctypes.data), ctypes.byref(info))
        print(f"getri_host {where}: {sha(buf)} info {info.value}", flush=True)


def batched_cases(sfx, dt, rt, n=129, batch=2):
    """above the one-launch limit (128 x 128 at most): the loop over the single-matrix entry; member 1 is singular"""
    F, ipiv = factors(n, dt, 7000 + n)
    dipiv = torch.from_numpy(np.stack([ipiv, ipiv[::-1].copy().clip(np.arange(1, n + 1))])).cuda()
    for pad, off in LAYOUTS:
        ld = n + pad
        buf, body = store(F, ld, off, rt, batch=batch)
        body[1, 2, 2] = 0                                           # u_33 of member 1
        tf, pf = dev(buf, body)
        for row_major in ((0, 1) if sfx[0] != "c" else (0,)):
            for trans in ((0, 1, 2) if sfx[0] == "c" else (None,)):
                ty, py = dev(*store(np.zeros_like(F), ld, off, rt, batch=batch))
                info = torch.full((batch,), -1, dtype=torch.int64, device="cuda")
                tail = (ld, n * ld) + ((trans,) if trans is not None else ()) + (tptr(info),)
                h.call(f"rflu_getri_batched_{sfx}_dev", batch, n, pf, ld, n * ld, row_major, tptr(dipiv), n, py, *tail)
                print(f"getri_batched {sfx} n={n} lda={ld} off={off} row_major={row_major} trans={trans}: {sha(ty, info)}", flush=True)


def logabsdet_cases(sfx, dt, rt, n, special=None):
    F, ipiv = factors(n, dt, 500 + n, special)
    dipiv = torch.from_numpy(ipiv).cuda()
    pad, off = 3, 1
    ld = n + pad
    where = f"{sfx} n={n}{' ' + special if special else ''}"
    buf, body = store(F, ld, off, rt, batch=2)
    body[1][np.arange(n), np.arange(n)] *= -1.25                    # member 1 of the batch: another diagonal
    t, p = dev(buf, body)
    for piv, hpiv in ((dipiv, ipiv), (None, None)):
        w = logabsdet_words(sfx, lambda *o: h.call(f"rflu_logabsdet_{sfx}_dev", n, p, ld, tptr(piv), *o))
        print(f"logabsdet_dev {where} ipiv={'yes' if piv is not None else 'no'}: {sha(w)}", flush=True)
        w = logabsdet_words(sfx, lambda *o: h.call(f"rflu_logabsdet_{sfx}", n, host_ptr(body), ld,
                                                   ctypes.c_void_p(hpiv.ctypes.data) if hpiv is not None else None, *o))
        print(f"logabsdet_host {where} ipiv={'yes' if piv is not None else 'no'}: {sha(w)}", flush=True)
    parts = 2 if sfx[0] == "c" else 1
    la = torch.full((2,), -7.0, dtype=torch.float64, device="cuda")
    sg = torch.full((2 * parts,), -7.0, dtype=torch.float64, device="cuda")
    h.call(f"rflu_logabsdet_batched_{sfx}_dev", 2, n, p, ld, n * ld, tptr(torch.stack([dipiv, dipiv])), n, tptr(la), tptr(sg))
    print(f"logabsdet_batched {where}: {sha(la, sg)}", flush=True)


for sfx, dt, rt in ELEMENTS:
    for n in GETRI_N:
        getri_cases(sfx, dt, rt, n)
    for special in ("zero", "nan"):
        getri_cases(sfx, dt, rt, 65, special)
        logabsdet_cases(sfx, dt, rt, 65, special)
    batched_cases(sfx, dt, rt)
    for n in LOGABSDET_N:
        logabsdet_cases(sfx, dt, rt, n)
