"""Host-side mirror of RecursiveFactorization.jl's public surface for the LU hot path, served by librflu.so.

Reference interface mirrored (citations into /root/reference/src/lu.jl):
    lu(A, pivot = Val(true), thread = Val(false); kwargs...)                       :19-21   -> ``lu``
    lu!(A, pivot = Val(true), thread = Val(false); check, kwargs...)               :67-83   -> ``lu_``  (ipiv=None)
    lu!(A, ipiv, pivot, thread; check = Val(true), blocksize, threshold)           :97-130  -> ``lu_``
    normalize_pivot: Val(true)/RowMaximum(), Val(false)/NoPivot()                  :10-17   -> ``pivot`` accepts both
    NotIPIV (lazy identity pivots for NoPivot)                                     :27-40   -> ``NotIPIV``
    LU(A, ipiv, info), checknonsingular(info) -> SingularException                 :128-129 -> ``LU``, ``SingularException``
    ldiv!(F, B) (stdlib for pivoted LU; the package's own for NotIPIV)             :60-64   -> ``ldiv_``
    (no counterpart: many small systems at once, getrfBatched / getrsBatched)               -> ``lu_batched_`` / ``lu_batched`` /
                                                                                             ``ldiv_batched_`` / ``BatchedLU``
    NoPivot failures carry a NEGATIVE info on Julia >= 1.11                        :25,250,324 -> ``NOPIVOT_NEGATIVE_INFO``
    (no counterpart here; LinearSolve.jl's RF32MixedLUFactorization: Float32 factors,      -> ``lu_mixed`` / ``ldiv_mixed`` / ``MixedLU``
     Float64 iterative refinement)
    (no counterpart: the same for ComplexF64, LAPACK zcgesv's scheme)                       -> ``lu_complex_mixed`` /
                                                                                             ``ldiv_complex_mixed``
    lu / lu! / ldiv! with T = ComplexF64 / ComplexF32 (test/runtests.jl:33-84)              -> ``lu_complex`` / ``lu_complex_`` /
                                                                                             ``ldiv_complex_`` (names of their own: ``lu``
                                                                                             keeps raising ``TypeError`` on complex input)
    ldiv!(F', B) / ldiv!(transpose(F), B) for complex factors                               -> ``ldiv_complex_adjoint_`` /
                                                                                             ``ldiv_complex_transpose_``
    (no counterpart: many small complex systems at once)                                    -> ``lu_complex_batched_`` /
                                                                                             ``lu_complex_batched`` /
                                                                                             ``ldiv_complex_batched_``
    inv / inv!, det, logabsdet, logdet on the LU object (stdlib LinearAlgebra)            -> ``inv`` / ``inv_`` / ``det`` / ``logabsdet`` /
                                                                                             ``logdet``; batched: ``inv_batched`` /
                                                                                             ``logabsdet_batched`` / ``det_batched``
    (no counterpart: LAPACK gerfs, the refinement and error bounds of gesvx)                -> ``refine_`` / ``solve_refined`` /
                                                                                             ``backward_error`` / ``Refinement``
    Adjoint/Transpose wrappers                                                     :85-87   -> ``Adjoint`` / ``lu(A.T ...)``;
                                                                                             ``ldiv_(Adjoint(F), B)`` solves A' x = b

Same names, argument meaning and error behaviour; Julia's ``!`` is spelled ``_``.  What differs, deliberately:
  * every Float64/Float32 matrix goes to the HIP path, whatever its size -- ``threshold`` (the reference's
    recursive/unblocked crossover, :90,114) is accepted and ignored, and there is NO CPU fallback: other element types
    raise ``TypeError`` (the Julia glue in INTEGRATION.md keeps the reference's own CPU code for those);
  * ``thread`` is accepted and ignored (the GPU path has no thread flag);
  * ``blocksize``: ``None``/0 = library default (pure Toledo recursion below 1024 columns; above, right-looking block
    columns of 256 ... 2048 by matrix size, block-column lookahead for the tall panels and the leaf-wise schedule for
    panels of at most 8192 rows, see include/rflu.h); negative = pure
    recursion; 64/128/256... = width of the outer right-looking block column.

Inputs: a NumPy array (host; staged through HBM by ``rflu_getrf_*``) or a ``torch`` tensor on the GPU
(column-major view, i.e. ``stride(0) == 1``, -> ``rflu_getrf_*_dev``; C-contiguous -> ``rflu_getrf_rm_*_dev``).
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import NamedTuple

import numpy as np

from . import _ffi

NOPIVOT_NEGATIVE_INFO = True  # the convention of Julia >= 1.11 (src/lu.jl:25)


class SingularException(ArithmeticError):
    """LinearAlgebra.SingularException(info): raised by ``check`` when a pivot is exactly zero (src/lu.jl:128)."""

    def __init__(self, info: int, batch_index: int | None = None):
        where = "" if batch_index is None else f", matrix {batch_index} of the batch"
        super().__init__(f"matrix is singular to working precision (info = {info}{where})")
        self.info = info
        self.batch_index = batch_index   # lu_batched_ / ldiv_batched_: 0-based index of the first failing matrix; None elsewhere


class RowMaximum:
    """LinearAlgebra.RowMaximum(): partial pivoting (== Val(true), src/lu.jl:13)."""


class NoPivot:
    """LinearAlgebra.NoPivot(): no pivoting (== Val(false), src/lu.jl:14)."""


class Val:
    """Julia's Val{x}: ``Val(True)`` / ``Val(False)`` are accepted wherever the reference takes ``Val``."""

    def __init__(self, x):
        self.x = x


def normalize_pivot(pivot) -> bool:
    """src/lu.jl:10-17."""
    if isinstance(pivot, Val):
        pivot = pivot.x
    if isinstance(pivot, RowMaximum) or pivot is RowMaximum:
        return True
    if isinstance(pivot, NoPivot) or pivot is NoPivot:
        return False
    if isinstance(pivot, (bool, np.bool_)):
        return bool(pivot)
    raise TypeError(f"pivot must be Val(true/false), RowMaximum() or NoPivot(), got {pivot!r}")


def _as_bool(flag) -> bool:
    return bool(flag.x) if isinstance(flag, Val) else bool(flag)


class NotIPIV:
    """Zero-storage identity pivot vector (src/lu.jl:27-40): ``getindex(::NotIPIV, i) = i``."""

    def __init__(self, length: int):
        self.len = int(length)

    def __len__(self):
        return self.len

    def __getitem__(self, i):
        if isinstance(i, slice):
            return NotIPIV(len(range(*i.indices(self.len))))
        if not 0 <= i < self.len:
            raise IndexError(i)
        return i + 1  # 1-based pivot values, like every ipiv here

    def __array__(self, dtype=None, copy=None):
        return np.arange(1, self.len + 1, dtype=dtype or np.int64)


@dataclass
class LU:
    """LinearAlgebra.LU{T}: packed factors (aliasing the caller's matrix for ``lu_``), 1-based ipiv, info."""

    factors: object
    ipiv: object
    info: int

    def issuccess(self) -> bool:
        return self.info == 0

    def _host(self):
        f = self.factors
        if hasattr(f, "detach"):
            f = f.detach().cpu().numpy()
        p = self.ipiv
        if hasattr(p, "detach"):
            p = p.detach().cpu().numpy()
        return np.asarray(f), np.asarray(p)

    @property
    def L(self):
        f, _ = self._host()
        m, n = f.shape
        k = min(m, n)
        return np.tril(f[:, :k], -1) + np.eye(m, k, dtype=f.dtype)

    @property
    def U(self):
        f, _ = self._host()
        return np.triu(f[: min(f.shape), :])

    @property
    def p(self):
        """Row permutation (0-based) such that L*U == A[p, :]."""
        f, ip = self._host()
        perm = np.arange(f.shape[0])
        for i, t in enumerate(ip):
            j = int(t) - 1
            if j != i:
                perm[i], perm[j] = perm[j], perm[i]
        return perm


class Adjoint:
    """``A'`` / ``transpose(A)`` wrapper for real matrices: lu(A') = adjoint(lu(parent(A))) (src/lu.jl:85-87)."""

    def __init__(self, parent):
        self.parent = parent


Transpose = Adjoint


def _checknonsingular(info: int):
    if info != 0:
        raise SingularException(abs(info))


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


def _sfx(dtype) -> str:
    name = str(dtype).replace("torch.", "")
    if name == "float64":
        return "f64"
    if name == "float32":
        return "f32"
    raise TypeError(
        f"lu / lu_ serve Float64/Float32 only (got {dtype}); ComplexF64/ComplexF32 matrices go to lu_complex / lu_complex_, and the "
        "reference routes other element types through its generic CPU code (src/lu.jl:122-123), which this package does not carry"
    )


def lu_(A, ipiv=None, pivot=True, thread=False, *, check=True, blocksize=None, threshold=None, handle=None) -> LU:
    """``lu!``: factor ``A`` in place.  ``ipiv`` None -> allocate (``NotIPIV`` for NoPivot), like src/lu.jl:67-83."""
    del thread, threshold  # accepted for signature parity; the HIP path has neither knob
    if isinstance(A, Adjoint):
        return Adjoint(lu_(A.parent, ipiv, pivot, check=check, blocksize=blocksize, handle=handle))
    piv = normalize_pivot(pivot)
    bs = int(blocksize or 0)
    info = ctypes.c_int64(0)
    if getattr(A, "ndim", None) != 2:
        raise ValueError("lu! needs a matrix")
    m, n = int(A.shape[0]), int(A.shape[1])
    mn = min(m, n)

    if _is_torch(A):
        import torch

        if not A.is_cuda:
            raise _ffi.RfluError("torch input must live on the MI355X (device='cuda'); host data goes in as NumPy")
        sfx = _sfx(A.dtype)
        h = handle or _ffi.default_handle(A.device.index or 0)
        h.set_stream(torch.cuda.current_stream(A.device).cuda_stream)
        if ipiv is None:
            ipiv_t = torch.empty(mn, dtype=torch.int64, device=A.device) if piv else None
        else:
            ipiv_t = ipiv
            if not (_is_torch(ipiv_t) and ipiv_t.is_cuda and ipiv_t.dtype == torch.int64 and ipiv_t.is_contiguous()):
                raise TypeError("ipiv for a GPU matrix must be a contiguous int64 CUDA tensor")
            if ipiv_t.numel() < mn:
                raise ValueError("ipiv is shorter than min(m, n)")
        ip_ptr = ctypes.c_void_p(ipiv_t.data_ptr() if ipiv_t is not None else 0)
        if m > 0 and n > 0:
            if A.stride(0) == 1 and A.stride(1) >= max(m, 1):  # column-major view (Julia layout)
                h.call(f"rflu_getrf_{sfx}_dev", m, n, ctypes.c_void_p(A.data_ptr()), A.stride(1), ip_ptr, int(piv), bs,
                       ctypes.byref(info))
            elif A.stride(1) == 1 and A.stride(0) >= max(n, 1):  # row-major: the library's internal layout
                h.call(f"rflu_getrf_rm_{sfx}_dev", m, n, ctypes.c_void_p(A.data_ptr()), A.stride(0), ip_ptr, int(piv), bs,
                       ctypes.byref(info))
            else:
                raise ValueError("matrix must be dense column-major or row-major (unit stride in one dimension)")
        out_ipiv = ipiv_t if ipiv_t is not None else NotIPIV(mn)
    else:
        if not isinstance(A, np.ndarray):
            raise TypeError("A must be a numpy.ndarray or a CUDA torch.Tensor")
        sfx = _sfx(A.dtype)
        if not A.flags.f_contiguous:
            raise ValueError("lu! works in place on column-major (Fortran-ordered) arrays; use lu() to copy")
        h = handle or _ffi.default_handle(0)
        h.set_stream(None)
        if ipiv is None:
            ipiv_a = np.empty(mn, dtype=np.int64) if piv else None
        else:
            ipiv_a = ipiv
            if not (isinstance(ipiv_a, np.ndarray) and ipiv_a.dtype == np.int64 and ipiv_a.flags.c_contiguous):
                raise TypeError("ipiv must be a contiguous int64 numpy array (Julia BlasInt)")
            if ipiv_a.size < mn:
                raise ValueError("ipiv is shorter than min(m, n)")
        ip_ptr = ctypes.c_void_p(ipiv_a.ctypes.data if ipiv_a is not None else 0)
        if m > 0 and n > 0:
            h.call(f"rflu_getrf_{sfx}", m, n, ctypes.c_void_p(A.ctypes.data), max(m, 1), ip_ptr, int(piv), bs,
                   ctypes.byref(info))
        out_ipiv = ipiv_a if ipiv_a is not None else NotIPIV(mn)

    inf = int(info.value)
    if not piv and NOPIVOT_NEGATIVE_INFO:
        inf = -inf
    if _as_bool(check):
        _checknonsingular(inf)
    return LU(A, out_ipiv, inf)


def lu(A, pivot=True, thread=False, **kwargs) -> LU:
    """``lu``: out of place, ``lu!(copy(A), ...)`` (src/lu.jl:19-21)."""
    if isinstance(A, Adjoint):
        return Adjoint(lu(A.parent, pivot, thread, **kwargs))
    if _is_torch(A):
        C = A.clone()
        if C.stride(0) != 1 and C.stride(1) != 1:
            C = A.contiguous()
    else:
        C = np.array(A, order="F", copy=True)
    return lu_(C, None, pivot, thread, **kwargs)


def ldiv_(F: LU, B, *, handle=None):
    """``ldiv!(F, B)``: overwrite ``B`` (a vector or an n x k matrix) with ``A \\ B`` using the factorization ``F``.

    Mirrors stdlib ``ldiv!(::LU, B)`` on the object ``lu!`` returns -- what LinearSolve's ``solve!`` calls right after the
    factorization -- and the package's own ``ldiv!`` for ``NotIPIV`` factors (/root/reference/src/lu.jl:60-64; tested at
    test/runtests.jl:21-28, 116-128).  Served by ``rflu_getrs_*`` (interchanges, fused unit-lower TRSM, upper solve).
    Raises ``SingularException`` when ``F.info != 0`` (the solve would divide by an exactly zero pivot).

    ``ldiv_(Adjoint(F), B)`` / ``ldiv_(Transpose(F), B)`` overwrite ``B`` with ``A' \\ B`` (stdlib ``ldiv!(::AdjointFactorization{<:Any,<:LU}, B)``,
    LAPACK getrs with trans = 'T'), served by ``rflu_getrs_trans_*`` under the same layout rules.
    """
    trans = ""
    if isinstance(F, Adjoint):
        F, trans = F.parent, "trans_"
        if isinstance(F, Adjoint):
            raise TypeError("ldiv! of a doubly wrapped factorization: unwrap it first")
    if F.info != 0:
        raise SingularException(abs(F.info))
    A = F.factors
    n = int(A.shape[0])
    if A.shape[0] != A.shape[1]:
        raise ValueError("ldiv! needs a square factorization")
    if B.shape[0] != n:
        raise ValueError("right-hand side has the wrong number of rows")
    nrhs = 1 if B.ndim == 1 else int(B.shape[1])
    nopiv = isinstance(F.ipiv, NotIPIV)
    if _is_torch(A):
        import torch

        if not (_is_torch(B) and B.is_cuda and B.dtype == A.dtype):
            raise TypeError("B must be a CUDA tensor of the factorization's dtype")
        sfx = _sfx(A.dtype)
        h = handle or _ffi.default_handle(A.device.index or 0)
        h.set_stream(torch.cuda.current_stream(A.device).cuda_stream)
        ip = ctypes.c_void_p(0 if nopiv else F.ipiv.data_ptr())
        if B.ndim == 1 and n > 1 and B.stride(0) != 1:
            # a strided vector view (e.g. a column of a row-major tensor) would be read and written at the wrong addresses
            raise ValueError("a vector right-hand side must be contiguous (stride 1); copy the view first")
        if A.stride(0) == 1:  # column-major factors -> column-major right-hand sides
            if B.ndim == 2 and not (B.stride(0) == 1 and B.stride(1) >= n):
                raise ValueError("B must be column-major like the factors")
            ldb = n if B.ndim == 1 else B.stride(1)
            h.call(f"rflu_getrs_{trans}{sfx}_dev", n, nrhs, ctypes.c_void_p(A.data_ptr()), A.stride(1), ip,
                   ctypes.c_void_p(B.data_ptr()), ldb)
        else:                 # row-major factors (rflu_getrf_rm) -> row-major right-hand sides
            if B.ndim == 2 and not (B.stride(1) == 1 and B.stride(0) >= nrhs):
                raise ValueError("B must be row-major like the factors (unit column stride, row stride >= nrhs)")
            ldb = 1 if B.ndim == 1 else B.stride(0)
            h.call(f"rflu_getrs_{trans}rm_{sfx}_dev", n, nrhs, ctypes.c_void_p(A.data_ptr()), A.stride(0), ip,
                   ctypes.c_void_p(B.data_ptr()), ldb)
        return B
    if not (isinstance(B, np.ndarray) and B.dtype == A.dtype and (B.ndim == 1 and B.flags.c_contiguous or B.flags.f_contiguous)):
        raise TypeError("B must be a column-major numpy array of the factorization's dtype")
    sfx = _sfx(A.dtype)
    h = handle or _ffi.default_handle(0)
    h.set_stream(None)
    ipiv = None if nopiv else np.ascontiguousarray(F.ipiv, dtype=np.int64)
    h.call(f"rflu_getrs_{trans}{sfx}", n, nrhs, ctypes.c_void_p(A.ctypes.data), max(n, 1),
           ctypes.c_void_p(0 if ipiv is None else ipiv.ctypes.data), ctypes.c_void_p(B.ctypes.data), max(n, 1))
    return B


def _csfx(dtype) -> str:
    name = str(dtype).replace("torch.", "")
    if name == "complex128":
        return "cf64"
    if name == "complex64":
        return "cf32"
    raise TypeError(f"lu_complex / lu_complex_ serve ComplexF64/ComplexF32 only (got {dtype}); real matrices go to lu / lu_")


def lu_complex_(A, ipiv=None, pivot=True, thread=False, *, check=True, blocksize=None, threshold=None, handle=None) -> LU:
    """``lu!`` for a ``complex128`` / ``complex64`` matrix, in place (``rflu_getrf_cf64`` / ``rflu_getrf_cf32`` and their ``_dev`` forms).

    The pivot of a column is the row of largest modulus ``abs(z)`` (strict ``>``, the lowest row on ties) -- the reference's rule, not
    LAPACK's ``|re| + |im|``, so ``scipy.linalg.lu_factor`` may choose other rows.  ``A``: a column-major NumPy array (host entry) or a
    column-major CUDA tensor (``stride(0) == 1``, device entry); row-major storage is refused.  Returns the same ``LU`` as ``lu_``:
    ``ipiv``, ``info``, ``check`` -> ``SingularException`` and the NoPivot sign of ``info`` follow the same rules.  ``blocksize``,
    ``threshold`` and ``thread`` are accepted and ignored: the complex path has one schedule, the Toledo recursion on one stream."""
    del thread, threshold, blocksize
    if isinstance(A, Adjoint):
        return Adjoint(lu_complex_(A.parent, ipiv, pivot, check=check, handle=handle))
    piv = normalize_pivot(pivot)
    info = ctypes.c_int64(0)
    if getattr(A, "ndim", None) != 2:
        raise ValueError("lu! needs a matrix")
    m, n = int(A.shape[0]), int(A.shape[1])
    mn = min(m, n)

    if _is_torch(A):
        import torch

        if not A.is_cuda:
            raise _ffi.RfluError("torch input must live on the MI355X (device='cuda'); host data goes in as NumPy")
        sfx = _csfx(A.dtype)
        if m > 1 and n > 0 and not (A.stride(0) == 1 and (n <= 1 or A.stride(1) >= m)):
            raise ValueError("lu_complex_ works in place on column-major tensors (stride(0) == 1); use lu_complex() to copy")
        if ipiv is None:
            ipiv_t = torch.empty(mn, dtype=torch.int64, device=A.device) if piv else None
        else:
            ipiv_t = ipiv
            if not (_is_torch(ipiv_t) and ipiv_t.is_cuda and ipiv_t.dtype == torch.int64 and ipiv_t.is_contiguous()):
                raise TypeError("ipiv for a GPU matrix must be a contiguous int64 CUDA tensor")
            if ipiv_t.numel() < mn:
                raise ValueError("ipiv is shorter than min(m, n)")
        if m > 0 and n > 0:
            h = handle or _ffi.default_handle(A.device.index or 0)
            h.set_stream(torch.cuda.current_stream(A.device).cuda_stream)
            h.call(f"rflu_getrf_{sfx}_dev", m, n, ctypes.c_void_p(A.data_ptr()), A.stride(1) if n > 1 else max(m, 1),
                   ctypes.c_void_p(ipiv_t.data_ptr() if ipiv_t is not None else 0), int(piv), ctypes.byref(info))
        out_ipiv = ipiv_t if ipiv_t is not None else NotIPIV(mn)
    else:
        if not isinstance(A, np.ndarray):
            raise TypeError("A must be a numpy.ndarray or a CUDA torch.Tensor")
        sfx = _csfx(A.dtype)
        if not A.flags.f_contiguous:
            raise ValueError("lu! works in place on column-major (Fortran-ordered) arrays; use lu() to copy")
        if ipiv is None:
            ipiv_a = np.empty(mn, dtype=np.int64) if piv else None
        else:
            ipiv_a = ipiv
            if not (isinstance(ipiv_a, np.ndarray) and ipiv_a.dtype == np.int64 and ipiv_a.flags.c_contiguous):
                raise TypeError("ipiv must be a contiguous int64 numpy array (Julia BlasInt)")
            if ipiv_a.size < mn:
                raise ValueError("ipiv is shorter than min(m, n)")
        if m > 0 and n > 0:
            h = handle or _ffi.default_handle(0)
            h.set_stream(None)
            h.call(f"rflu_getrf_{sfx}", m, n, ctypes.c_void_p(A.ctypes.data), max(m, 1),
                   ctypes.c_void_p(ipiv_a.ctypes.data if ipiv_a is not None else 0), int(piv), ctypes.byref(info))
        out_ipiv = ipiv_a if ipiv_a is not None else NotIPIV(mn)

    inf = int(info.value)
    if not piv and NOPIVOT_NEGATIVE_INFO:
        inf = -inf
    if _as_bool(check):
        _checknonsingular(inf)
    return LU(A, out_ipiv, inf)


def lu_complex(A, pivot=True, thread=False, **kwargs) -> LU:
    """``lu`` for a complex matrix: ``lu_complex_`` on a column-major copy."""
    if isinstance(A, Adjoint):
        return Adjoint(lu_complex(A.parent, pivot, thread, **kwargs))
    if _is_torch(A):
        C = A.T.contiguous().T   # column-major copy
        if C.data_ptr() == A.data_ptr():
            C = A.T.clone().T
    else:
        C = np.array(A, order="F", copy=True)
    return lu_complex_(C, None, pivot, thread, **kwargs)


def _ldiv_complex_call(F, B, handle, entry: str, extra: tuple, what: str):
    """The checks and the call shared by ``ldiv_complex_``, ``ldiv_complex_transpose_`` and ``ldiv_complex_adjoint_``: shape, dtype,
    column-major layout, ``F.info != 0`` -> ``SingularException``, the side of the bus; ``n == 0`` / ``nrhs == 0`` return ``B`` without
    touching a device.  ``entry`` is the C entry without its suffixes (``rflu_getrs`` / ``rflu_getrs_trans``), ``extra`` its trailing
    arguments."""
    if isinstance(F, Adjoint):
        if entry == "rflu_getrs":
            raise TypeError("ldiv_complex_: an Adjoint-wrapped complex factorization is not served here (adjoint and transpose differ, and "
                            "Transpose is an alias of Adjoint): call ldiv_complex_adjoint_ or ldiv_complex_transpose_ with the plain LU")
        raise TypeError(f"{what} takes the plain LU that lu_complex_ returned, not an Adjoint wrapper (Transpose is an alias of Adjoint, "
                        "so the wrapper cannot say which of the two solves is meant): the function's name does")
    if F.info != 0:
        raise SingularException(abs(F.info))
    A = F.factors
    sfx = _csfx(A.dtype)
    n = int(A.shape[0])
    if A.shape[0] != A.shape[1]:
        raise ValueError("ldiv! needs a square factorization")
    if B.shape[0] != n:
        raise ValueError("right-hand side has the wrong number of rows")
    nrhs = 1 if B.ndim == 1 else int(B.shape[1])
    nopiv = isinstance(F.ipiv, NotIPIV)
    if _is_torch(A):
        import torch

        if not (_is_torch(B) and B.is_cuda and B.dtype == A.dtype):
            raise TypeError("B must be a CUDA tensor of the factorization's dtype")
        if n > 1 and A.stride(0) != 1:
            raise ValueError("the factors must be column-major, as lu_complex_ leaves them")
        if B.ndim == 1 and n > 1 and B.stride(0) != 1:
            raise ValueError("a vector right-hand side must be contiguous (stride 1); copy the view first")
        if B.ndim == 2 and n > 1 and not (B.stride(0) == 1 and (nrhs <= 1 or B.stride(1) >= n)):
            raise ValueError("B must be column-major like the factors")
        if n == 0 or nrhs == 0:
            return B
        h = handle or _ffi.default_handle(A.device.index or 0)
        h.set_stream(torch.cuda.current_stream(A.device).cuda_stream)
        ldb = B.stride(1) if (B.ndim == 2 and nrhs > 1 and n > 1) else max(n, 1)
        h.call(f"{entry}_{sfx}_dev", n, nrhs, ctypes.c_void_p(A.data_ptr()), A.stride(1) if n > 1 else 1,
               ctypes.c_void_p(0 if nopiv else F.ipiv.data_ptr()), ctypes.c_void_p(B.data_ptr()), ldb, *extra)
        return B
    if not (isinstance(B, np.ndarray) and B.dtype == A.dtype and (B.ndim == 1 and B.flags.c_contiguous or B.flags.f_contiguous)):
        raise TypeError("B must be a column-major numpy array of the factorization's dtype")
    if n == 0 or nrhs == 0:
        return B
    h = handle or _ffi.default_handle(0)
    h.set_stream(None)
    ipiv = None if nopiv else np.ascontiguousarray(F.ipiv, dtype=np.int64)
    h.call(f"{entry}_{sfx}", n, nrhs, ctypes.c_void_p(A.ctypes.data), max(n, 1),
           ctypes.c_void_p(0 if ipiv is None else ipiv.ctypes.data), ctypes.c_void_p(B.ctypes.data), max(n, 1), *extra)
    return B


def ldiv_complex_(F: LU, B, *, handle=None):
    """``ldiv!(F, B)`` with the factors ``lu_complex_`` returned: overwrite ``B`` (a vector or a column-major n x k matrix of the factors'
    dtype, on the factors' side of the bus) with ``A \\ B`` (``rflu_getrs_cf64`` / ``rflu_getrs_cf32`` and their ``_dev`` forms).  Raises
    ``SingularException`` when ``F.info != 0``.  An ``Adjoint`` factorization raises ``TypeError``: ``ldiv!(F', B)`` and
    ``ldiv!(transpose(F), B)`` are ``ldiv_complex_adjoint_`` and ``ldiv_complex_transpose_``."""
    return _ldiv_complex_call(F, B, handle, "rflu_getrs", (), "ldiv_complex_")


def ldiv_complex_adjoint_(F: LU, B, *, handle=None):
    """``ldiv!(F', B)`` for complex factors: overwrite ``B`` with ``A' \\ B``, ``A'`` the conjugate transpose (``rflu_getrs_trans_cf64`` /
    ``_cf32`` and their ``_dev`` forms with ``conj = 1``, LAPACK's ``'C'``).  ``F`` is the plain ``LU`` that ``lu_complex_`` returned and
    ``B`` as for ``ldiv_complex_``; the factors are only read.

    This is a function of its own rather than a dispatch on a wrapper because in this package ``Transpose is Adjoint`` (one wrapper class,
    right for real matrices), while for a complex factorization the adjoint and the transpose are different solves: a wrapper could
    silently mean the wrong one, a function name cannot.  An ``Adjoint``-wrapped argument therefore raises ``TypeError``."""
    return _ldiv_complex_call(F, B, handle, "rflu_getrs_trans", (1,), "ldiv_complex_adjoint_")


def ldiv_complex_transpose_(F: LU, B, *, handle=None):
    """``ldiv!(transpose(F), B)`` for complex factors: overwrite ``B`` with ``transpose(A) \\ B``, no conjugation (``rflu_getrs_trans_cf64``
    / ``_cf32`` and their ``_dev`` forms with ``conj = 0``, LAPACK's ``'T'``).  Arguments as for ``ldiv_complex_adjoint_``, and a function
    of its own for the same reason: ``Transpose is Adjoint`` here, so a wrapper could not tell this solve from the adjoint one.  An
    ``Adjoint``-wrapped argument raises ``TypeError``."""
    return _ldiv_complex_call(F, B, handle, "rflu_getrs_trans", (0,), "ldiv_complex_transpose_")


def _unwrap_adjoint(F, what: str):
    if isinstance(F, Adjoint):
        F = F.parent
        if isinstance(F, Adjoint):
            raise TypeError(f"{what} of a doubly wrapped factorization: unwrap it first")
        return F, True
    return F, False


def _square_factors(F, what: str):
    """Shape, element type and layout of the factors of ``inv`` / ``det`` / ``logabsdet`` -- before anything touches the library.
    Returns (A, n, sfx, kind, ld) with kind in "cm" / "rm" (CUDA tensors) / "host" (column-major NumPy)."""
    if not isinstance(F, LU):
        raise TypeError(f"{what} needs the LU that lu / lu_ returned")
    A = F.factors
    if A is None:
        raise ValueError(f"{what}: this factorization is no longer valid (inv_ overwrote its factors with the inverse)")
    if getattr(A, "ndim", None) != 2 or A.shape[0] != A.shape[1]:
        raise ValueError(f"{what} needs a square factorization")
    sfx = _sfx(A.dtype)
    n = int(A.shape[0])
    if _is_torch(A):
        if not A.is_cuda:
            raise _ffi.RfluError("torch factors must live on the MI355X (device='cuda'); host data goes in as NumPy")
        if not isinstance(F.ipiv, NotIPIV) and not (_is_torch(F.ipiv) and F.ipiv.is_cuda and str(F.ipiv.dtype) == "torch.int64"
                                                      and F.ipiv.numel() >= n and (n <= 1 or F.ipiv.stride(0) == 1)):
            raise TypeError("ipiv of GPU factors must be a contiguous int64 CUDA tensor of length n (or NotIPIV)")
        if n <= 1 or (A.stride(0) == 1 and A.stride(1) >= n):
            return A, n, sfx, "cm", (int(A.stride(1)) if n > 1 else 1)
        if A.stride(1) == 1 and A.stride(0) >= n:
            return A, n, sfx, "rm", int(A.stride(0))
        raise ValueError(f"{what}: the factors must be dense column-major or row-major (unit stride in one dimension)")
    if not isinstance(A, np.ndarray):
        raise TypeError("factors must be a numpy.ndarray or a CUDA torch.Tensor")
    if not A.flags.f_contiguous:
        raise ValueError(f"{what}: host factors must be column-major (Fortran-ordered), as lu_ leaves them")
    return A, n, sfx, "host", max(n, 1)


def _ipiv_arg(F, kind: str):
    """(keep-alive object, pointer) of the pivots: NULL for NotIPIV."""
    if isinstance(F.ipiv, NotIPIV):
        return None, ctypes.c_void_p(0)
    if kind == "host":
        ip = np.ascontiguousarray(F.ipiv, dtype=np.int64)
        return ip, ctypes.c_void_p(ip.ctypes.data)
    return F.ipiv, ctypes.c_void_p(F.ipiv.data_ptr())


def _handle_for(A, kind: str, handle):
    if kind == "host":
        h = handle or _ffi.default_handle(0)
        h.set_stream(None)
        return h, ctypes.c_void_p(A.ctypes.data)
    import torch

    h = handle or _ffi.default_handle(A.device.index or 0)
    h.set_stream(torch.cuda.current_stream(A.device).cuda_stream)
    return h, ctypes.c_void_p(A.data_ptr())


def inv_(F, *, handle=None):
    """``LinearAlgebra.inv!(F::LU)``: overwrite the factors with ``inv(A)`` (LAPACK getri, ``rflu_getri_*``) and return the array that
    held them.  About 4n^3/3 flops and no n x n workspace, against 2n^3 and three more n x n arrays for ``ldiv_(F, I)``.

    ``F`` IS INVALID AFTERWARDS: its storage holds the inverse, so ``F.factors`` is set to ``None`` and any later use of ``F`` raises.
    Use ``inv(F)`` to keep the factorization.  Layout rules exactly as ``ldiv_``: a column-major or row-major CUDA tensor
    (``rflu_getri_*_dev`` / ``rflu_getri_rm_*_dev``) or a column-major NumPy array (``rflu_getri_*``).  Raises ``SingularException(info)``
    when ``F.info != 0`` or the library finds an exactly zero ``u_ii`` -- the factors are then untouched and ``F`` stays valid.
    ``inv_(Adjoint(F))`` returns the transposed view of ``inv_(F)``: inv(A') = inv(A)'."""
    F, adj = _unwrap_adjoint(F, "inv!")
    A, n, sfx, kind, ld = _square_factors(F, "inv!")
    if F.info != 0:
        raise SingularException(abs(F.info))
    if n > 0:
        keep, ip = _ipiv_arg(F, kind)
        h, ap = _handle_for(A, kind, handle)
        info = ctypes.c_int64(0)
        name = {"cm": f"rflu_getri_{sfx}_dev", "rm": f"rflu_getri_rm_{sfx}_dev", "host": f"rflu_getri_{sfx}"}[kind]
        h.call(name, n, ap, ld, ip, ctypes.byref(info))
        del keep
        if info.value != 0:
            raise SingularException(int(info.value))
    F.factors = None
    return A.T if adj else A


def inv(F, *, handle=None):
    """``inv(F::LU)``: ``inv_`` on a copy of the factors; ``F`` stays intact."""
    G, adj = _unwrap_adjoint(F, "inv")
    A = _square_factors(G, "inv")[0]
    C = A.clone() if _is_torch(A) else np.array(A, order="F", copy=True)
    X = inv_(LU(C, G.ipiv, G.info), handle=handle)
    return X.T if adj else X


def logabsdet(F, *, handle=None):
    """``logabsdet(F::LU)`` -> ``(log|det A|, sign det A)`` as Python floats (``rflu_logabsdet_*``): the sum of ``log|u_ii|`` in Float64
    for both element types, the sign from the diagonal's signs and the parity of the interchanges.  Only the diagonal and ``ipiv`` are
    read (the host entry copies nothing else).  A zero ``u_ii`` gives ``(-inf, 0.0)``, a NaN ``(nan, nan)``; ``n == 0`` gives ``(0.0, 1.0)``.
    ``Adjoint(F)``: the same value."""
    F, _ = _unwrap_adjoint(F, "logabsdet")
    A, n, sfx, kind, ld = _square_factors(F, "logabsdet")
    if n == 0:
        return 0.0, 1.0
    keep, ip = _ipiv_arg(F, kind)
    h, ap = _handle_for(A, kind, handle)
    la, sg = ctypes.c_double(0.0), ctypes.c_double(1.0)
    h.call(f"rflu_logabsdet_{sfx}" + ("" if kind == "host" else "_dev"), n, ap, ld, ip, ctypes.byref(la), ctypes.byref(sg))
    del keep
    return float(la.value), float(sg.value)


def det(F, *, handle=None) -> float:
    """``det(F::LU)`` = ``sign * exp(logabs)`` of ``logabsdet``; 0.0 for a singular ``F`` as in Julia.  It differs from Julia's running
    product of the diagonal by rounding only (and overflows / underflows only where the determinant itself does)."""
    la, sg = logabsdet(F, handle=handle)
    with np.errstate(over="ignore"):
        return 0.0 if sg == 0.0 else sg * float(np.exp(np.float64(la)))


def logdet(F, *, handle=None) -> float:
    """``logdet(F::LU)``: ``log(det A)``; raises ``ValueError`` (Julia: DomainError) for a negative determinant."""
    la, sg = logabsdet(F, handle=handle)
    if sg < 0.0:
        raise ValueError("logdet: the determinant is negative; use logabsdet")
    return la


def _norm_code(p, what: str) -> int:
    """``p`` of ``opnorm`` / ``rcond`` / ``cond``: 1, or ``math.inf`` / ``"inf"``; anything else raises ``ValueError``."""
    if isinstance(p, str):
        if p.lower() == "inf":
            return _ffi.NORM_INF
    elif isinstance(p, (int, float)) and not isinstance(p, bool):
        if p == 1:
            return _ffi.NORM_ONE
        if p == float("inf"):
            return _ffi.NORM_INF
    raise ValueError(f"{what}: p must be 1 or inf (math.inf / \"inf\"), got {p!r}")


_COMPLEX_COND = {"opnorm": "opnorm_complex", "rcond": "rcond_complex", "cond": "cond_complex", "opnorm_batched": "opnorm_complex_batched",
                 "rcond_batched": "rcond_complex_batched", "cond_batched": "cond_complex_batched"}
_REAL_COND = {v: k for k, v in _COMPLEX_COND.items()}


def _cond_sfx(dtype, what: str) -> str:
    if str(dtype).replace("torch.", "") in ("complex128", "complex64"):
        raise TypeError(f"{what} serves Float64/Float32 only (got {dtype}); complex element types go to {_COMPLEX_COND[what]}")
    return _sfx(dtype)


def _ccond_sfx(dtype, what: str) -> str:
    name = str(dtype).replace("torch.", "")
    if name == "complex128":
        return "cf64"
    if name == "complex64":
        return "cf32"
    raise TypeError(f"{what} serves ComplexF64/ComplexF32 only (got {dtype}); real element types go to {_REAL_COND[what]}")


def _swap_norm(code: int) -> int:
    return _ffi.NORM_INF if code == _ffi.NORM_ONE else _ffi.NORM_ONE


def opnorm(A, p=1, *, handle=None) -> float:
    """``opnorm(A, 1)`` / ``opnorm(A, Inf)``: the largest column / row sum of ``|a_ij|`` of an m x n matrix (LAPACK lange,
    ``rflu_lange_*_dev``), as a Python float.  Float64 sums in a fixed order for both element types: bit-identical from run to run and
    whatever the alignment.  ``A``: a column-major or row-major CUDA tensor, or a NumPy array (copied to the device).  A NaN anywhere
    gives NaN; an empty matrix gives 0.  Take it BEFORE ``lu_`` overwrites ``A``: ``rcond`` needs it.  ``Adjoint(A)`` swaps 1 and inf."""
    code = _norm_code(p, "opnorm")
    if isinstance(A, Adjoint):
        A, code = A.parent, _swap_norm(code)
        if isinstance(A, Adjoint):
            raise TypeError("opnorm of a doubly wrapped matrix: unwrap it first")
    if getattr(A, "ndim", None) != 2:
        raise ValueError("opnorm needs a matrix")
    sfx = _cond_sfx(A.dtype, "opnorm")
    m, n = int(A.shape[0]), int(A.shape[1])
    if m == 0 or n == 0:
        return 0.0
    import torch

    if not _is_torch(A):
        if not isinstance(A, np.ndarray):
            raise TypeError("A must be a numpy.ndarray or a CUDA torch.Tensor")
        dev = torch.device("cuda", handle.device if handle is not None else 0)
        if A.flags.f_contiguous and not A.flags.c_contiguous:   # a Fortran-ordered array stays column-major on the device
            A = torch.from_numpy(np.ascontiguousarray(A.T)).to(dev).T
        else:
            A = torch.from_numpy(np.ascontiguousarray(A)).to(dev)
    if not A.is_cuda:
        raise _ffi.RfluError("torch input must live on the MI355X (device='cuda'); host data goes in as NumPy")
    if A.stride(0) == 1 and (A.stride(1) >= m or n == 1):
        row_major, ld = 0, (int(A.stride(1)) if n > 1 else m)
    elif A.stride(1) == 1 and (A.stride(0) >= n or m == 1):
        row_major, ld = 1, (int(A.stride(0)) if m > 1 else n)
    else:
        raise ValueError("opnorm: the matrix must be dense column-major or row-major (unit stride in one dimension)")
    h = handle or _ffi.default_handle(A.device.index or 0)
    h.set_stream(torch.cuda.current_stream(A.device).cuda_stream)
    out = ctypes.c_double(0.0)
    h.call(f"rflu_lange_{sfx}_dev", code, m, n, ctypes.c_void_p(A.data_ptr()), ld, row_major, ctypes.byref(out))
    return float(out.value)


def rcond(F, anorm, p=1, *, handle=None) -> float:
    """The reciprocal condition number ``1 / (||A|| ||inv(A)||)`` in the 1- or inf-norm from the factors (LAPACK gecon,
    ``rflu_gecon_*``): ``anorm = opnorm(A, p)`` taken before the factorization, ``||inv(A)||`` estimated by Higham's method with at most
    11 solves of one right-hand side -- 2n^2 flops each against 2n^3/3 for the factorization; ``F`` is only read.  The estimate is a
    lower bound of ``||inv(A)||`` up to rounding, so ``rcond`` errs towards well-conditioned by a small factor at most.
    Layouts as ``inv_``: column-major or row-major CUDA factors, or column-major NumPy factors.  ``n == 0`` gives 1, ``anorm == 0`` or an
    exactly zero ``u_ii`` gives 0, a NaN ``anorm`` or a NaN in the factors gives NaN; ``anorm < 0`` raises.  ``Adjoint(F)`` swaps 1 and inf."""
    code = _norm_code(p, "rcond")
    F, adj = _unwrap_adjoint(F, "rcond")
    if isinstance(F, LU) and F.factors is not None:
        _cond_sfx(F.factors.dtype, "rcond")
    A, n, sfx, kind, ld = _square_factors(F, "rcond")
    if adj:
        code = _swap_norm(code)
    anorm = float(anorm)
    if anorm < 0.0:
        raise ValueError("rcond: anorm must not be negative")
    if n == 0:
        return 1.0
    h, ap = _handle_for(A, kind, handle)
    out = ctypes.c_double(0.0)
    name = {"cm": f"rflu_gecon_{sfx}_dev", "rm": f"rflu_gecon_rm_{sfx}_dev", "host": f"rflu_gecon_{sfx}"}[kind]
    h.call(name, code, n, ap, ld, anorm, ctypes.byref(out))
    return float(out.value)


def cond(A, p=1, *, handle=None) -> float:
    """``cond(A, 1)`` / ``cond(A, Inf)`` as Julia computes them: ``opnorm``, then ``lu`` on a copy (``check=False``), then ``1 / rcond``;
    ``inf`` when ``rcond == 0`` (a singular matrix).  ``A`` stays intact."""
    code = _norm_code(p, "cond")
    if isinstance(A, Adjoint):
        A, code = A.parent, _swap_norm(code)
        if isinstance(A, Adjoint):
            raise TypeError("cond of a doubly wrapped matrix: unwrap it first")
    if getattr(A, "ndim", None) != 2 or A.shape[0] != A.shape[1]:
        raise ValueError("cond needs a square matrix")
    _cond_sfx(A.dtype, "cond")
    if A.shape[0] == 0:
        return 1.0
    p = 1 if code == _ffi.NORM_ONE else float("inf")
    anorm = opnorm(A, p, handle=handle)
    rc = rcond(lu(A, check=False, handle=handle), anorm, p, handle=handle)
    return float("inf") if rc == 0.0 else 1.0 / rc


# ---- iterative refinement with error bounds (LAPACK gerfs, what gesvx runs behind getrf / getrs) ---------------------------------------
class Refinement(NamedTuple):
    """What ``refine_`` found per right-hand side: ``ferr`` (forward error bound, ``None`` when skipped), ``berr`` (componentwise
    backward error of the returned solution), ``steps`` (corrections applied); NumPy arrays of length nrhs."""

    ferr: object
    berr: object
    steps: object


def _refine_dtype(dtype, what: str) -> str:
    if str(dtype).replace("torch.", "") in ("complex128", "complex64"):
        raise TypeError(f"{what} serves Float64/Float32 only (got {dtype}); complex element types are not served: refine a complex "
                        "solution with ldiv_complex_mixed, or check it on the CPU")
    return _sfx(dtype)


def _refine_factors(F, what: str):
    """The refusals of ``refine_`` / ``solve_refined`` that concern the factorization -- before anything touches the library."""
    if isinstance(F, Adjoint):
        raise TypeError(f"{what} serves A x = b only (LAPACK trans = 'N'), not Adjoint(F): solve with ldiv_(Adjoint(F), B) and check "
                        "the result with backward_error on the transposed matrix")
    if isinstance(F, MixedLU):
        raise TypeError(f"{what} needs factors in the working precision (lu / lu_); a MixedLU is refined by ldiv_mixed itself")
    if isinstance(F, BatchedLU):
        raise TypeError(f"{what} serves one factorization (lu / lu_), not a BatchedLU: refine the members one by one")
    if not isinstance(F, LU):
        raise TypeError(f"{what} needs the LU that lu / lu_ returned")
    if F.factors is not None and hasattr(F.factors, "dtype"):
        _refine_dtype(F.factors.dtype, what)
    A, n, sfx, kind, ld = _square_factors(F, what)
    if kind == "rm":
        raise ValueError(f"{what} serves column-major factors only (lu_ on a column-major tensor); row-major factors: transpose the "
                         "system into column-major storage first")
    return A, n, sfx, kind, ld


def _refine_operand(M, n: int, name: str, what: str, sfx: str, dev, matrix: bool = False):
    """A column-major device view of an operand with n rows: (tensor, ncols, ld, was_numpy).  A vector counts as one column.
    dev None: the checks alone, nothing is copied (every operand is checked before the first one travels)."""
    import torch

    if getattr(M, "ndim", None) not in ((2,) if matrix else (1, 2)) or int(M.shape[0]) != n or (matrix and int(M.shape[1]) != n):
        raise ValueError(f"{what}: {name} must be {'n x n' if matrix else 'a vector of n entries or an n x nrhs matrix'}")
    if _refine_dtype(M.dtype, what) != sfx:
        raise TypeError(f"{what}: {name} must have the element type of the other operands")
    cols = 1 if M.ndim == 1 else int(M.shape[1])
    host = not _is_torch(M)
    if host:
        if not isinstance(M, np.ndarray):
            raise TypeError(f"{what}: {name} must be a numpy.ndarray or a CUDA torch.Tensor")
        if matrix and n > 1 and M.flags.c_contiguous and not M.flags.f_contiguous:
            raise ValueError(f"{what}: a row-major {name} is not served; pass it column-major (np.asfortranarray)")
        if dev is None:
            return None, cols, max(n, 1), host
        M = torch.from_numpy(np.ascontiguousarray(M.T)).to(dev).T if M.ndim == 2 else torch.from_numpy(np.ascontiguousarray(M)).to(dev)
    elif not M.is_cuda:
        raise _ffi.RfluError("torch input must live on the MI355X (device='cuda'); host data goes in as NumPy")
    if M.ndim == 1:
        if n > 1 and M.stride(0) != 1:
            raise ValueError(f"{what}: a vector {name} must be contiguous (stride 1)")
        return M, 1, max(n, 1), host
    if n > 1 and not (M.stride(0) == 1 and (cols <= 1 or M.stride(1) >= n)):
        raise ValueError(f"{what}: {name} must be column-major (unit row stride, column stride >= n); a row-major {name} is not served")
    return M, cols, (max(int(M.stride(1)), n, 1) if cols > 1 else max(n, 1)), host


def refine_(F, A, B, X, *, max_iter=5, ferr=True, handle=None) -> Refinement:
    """Refine the computed solution ``X`` of ``A X = B`` IN PLACE in the working precision and say how good it is (LAPACK gerfs with
    trans = 'N', ``rflu_gerfs_*_dev``): per right-hand side the componentwise backward error ``berr = max_i |b - A x|_i / (|b| + |A| |x|)_i``
    of the returned ``X``, LAPACK's forward error bound ``ferr >= ||x - x_true||_inf / ||x||_inf`` (up to the estimator's slack) and
    the corrections applied.  ``A`` is the ORIGINAL matrix (a copy taken before ``lu_``), ``F`` its column-major factors.  Residuals
    are accumulated in Float64 for both element types.  ``ferr=False`` skips the bound, which costs up to 11 one-column solves per
    right-hand side.  CUDA tensors must be column-major (a vector counts as one column); NumPy arrays are copied up and ``X`` is copied
    back.  Raises ``SingularException`` for an exactly zero ``u_ii`` (``X`` is then untouched)."""
    import torch

    Ff, n, sfx, kind, ldf = _refine_factors(F, "refine!")
    if F.info != 0:
        raise SingularException(abs(F.info))
    cols = [_refine_operand(M, n, name, "refine!", sfx, None, matrix=mat)[1] for M, name, mat in ((A, "A", True), (B, "B", False), (X, "X", False))]
    if cols[1] != cols[2]:
        raise ValueError("refine!: X and B must have the same number of columns")
    dev = torch.device("cuda", handle.device if handle is not None else 0) if kind == "host" else Ff.device
    Fd = _refine_operand(Ff, n, "the factors", "refine!", sfx, dev, matrix=True)[0] if kind == "host" else Ff
    Ad, _, lda, _ = _refine_operand(A, n, "A", "refine!", sfx, dev, matrix=True)
    Bd, nrhs, ldb, _ = _refine_operand(B, n, "B", "refine!", sfx, dev)
    Xd, nx, ldx, x_host = _refine_operand(X, n, "X", "refine!", sfx, dev)
    if nx != nrhs:
        raise ValueError("refine!: X and B must have the same number of columns")
    if kind == "host":
        ldf = max(int(Fd.stride(1)), n, 1) if n > 1 else 1
    if isinstance(F.ipiv, NotIPIV):
        keep, ip = None, ctypes.c_void_p(0)
    else:
        keep = F.ipiv if _is_torch(F.ipiv) else torch.from_numpy(np.ascontiguousarray(F.ipiv, dtype=np.int64)).to(dev)
        ip = ctypes.c_void_p(keep.data_ptr())
    berr = np.zeros(nrhs, dtype=np.float64)
    fe = np.zeros(nrhs, dtype=np.float64) if ferr else None
    steps = np.zeros(nrhs, dtype=np.intc)
    if n > 0 and nrhs > 0:
        h = handle or _ffi.default_handle(Ad.device.index or 0)
        h.set_stream(torch.cuda.current_stream(Ad.device).cuda_stream)
        info = ctypes.c_int64(0)
        h.call(f"rflu_gerfs_{sfx}_dev", n, nrhs, ctypes.c_void_p(Ad.data_ptr()), lda, ctypes.c_void_p(Fd.data_ptr()), ldf, ip,
               ctypes.c_void_p(Bd.data_ptr()), ldb, ctypes.c_void_p(Xd.data_ptr()), ldx,
               ctypes.c_void_p(fe.ctypes.data if ferr else 0), ctypes.c_void_p(berr.ctypes.data), int(max_iter),
               ctypes.c_void_p(steps.ctypes.data), ctypes.byref(info))
        if info.value != 0:
            raise SingularException(int(info.value))
        if x_host:
            X[...] = Xd.cpu().numpy()
    del keep
    return Refinement(fe, berr, steps.astype(np.int64))


def solve_refined(F, A, B, **kw):
    """``(X, Refinement)``: a copy of ``B``, ``ldiv_(F, X)``, then ``refine_(F, A, B, X, **kw)`` -- LAPACK gesvx without equilibration."""
    _refine_factors(F, "solve_refined")
    X = B.clone() if _is_torch(B) else np.array(B, order="F", copy=True)
    ldiv_(F, X, handle=kw.get("handle"))
    return X, refine_(F, A, B, X, **kw)


def backward_error(A, X, B, *, handle=None):
    """The componentwise (Oettli-Prager) backward error ``max_i |b - A x|_i / (|b| + |A| |x|)_i`` of every column of ANY ``X``
    (``rflu_berr_*_dev``), as a NumPy array of length nrhs.  Float64 sums for both element types; a row whose terms are all zero
    contributes 0; needs no factors.  Operands as ``refine_``: column-major CUDA tensors, or NumPy arrays (copied up)."""
    import torch

    if isinstance(A, Adjoint):
        raise TypeError("backward_error serves A x = b only, not Adjoint(A): pass the transposed matrix in column-major storage")
    if getattr(A, "ndim", None) != 2 or A.shape[0] != A.shape[1]:
        raise ValueError("backward_error needs a square matrix")
    sfx = _refine_dtype(A.dtype, "backward_error")
    n = int(A.shape[0])
    cols = [_refine_operand(M, n, name, "backward_error", sfx, None, matrix=mat)[1] for M, name, mat in ((A, "A", True), (X, "X", False), (B, "B", False))]
    if cols[1] != cols[2]:
        raise ValueError("backward_error: X and B must have the same number of columns")
    dev = A.device if _is_torch(A) else torch.device("cuda", handle.device if handle is not None else 0)
    Ad, _, lda, _ = _refine_operand(A, n, "A", "backward_error", sfx, dev, matrix=True)
    Xd, nrhs, ldx, _ = _refine_operand(X, n, "X", "backward_error", sfx, dev)
    Bd, nb, ldb, _ = _refine_operand(B, n, "B", "backward_error", sfx, dev)
    if nb != nrhs:
        raise ValueError("backward_error: X and B must have the same number of columns")
    berr = np.zeros(nrhs, dtype=np.float64)
    if n > 0 and nrhs > 0:
        h = handle or _ffi.default_handle(Ad.device.index or 0)
        h.set_stream(torch.cuda.current_stream(Ad.device).cuda_stream)
        h.call(f"rflu_berr_{sfx}_dev", n, nrhs, ctypes.c_void_p(Ad.data_ptr()), lda, ctypes.c_void_p(Xd.data_ptr()), ldx,
               ctypes.c_void_p(Bd.data_ptr()), ldb, ctypes.c_void_p(berr.ctypes.data))
    return berr


def _complex_trans(F, trans, what: str):
    """The plain factorization and which of the three matrices is meant: "N" (A), "T" (transpose(A)) or "C" (A', the conjugate
    transpose) -- LAPACK's letters, as in ``ldiv_complex_batched_``.  ``Transpose is Adjoint`` in this package, so a wrapper cannot say
    "T"; ``Adjoint(F)`` means "C" and takes no ``trans`` besides the default."""
    if not isinstance(trans, str) or trans not in _CBATCHED_TRANS:
        raise ValueError(f'{what}: trans must be "N", "T" or "C", got {trans!r}')
    if isinstance(F, Adjoint):
        F = F.parent
        if isinstance(F, Adjoint):
            raise TypeError(f"{what} of a doubly wrapped factorization: unwrap it first")
        if trans != "N":
            raise ValueError(f'{what}: Adjoint(F) already means trans="C": pass the plain factorization together with trans')
        trans = "C"
    return F, trans


def _complex_square_factors(F, what: str):
    """``_square_factors`` for the complex functions -- before anything touches the library.  Returns (A, n, sfx, kind, ld) with kind
    "cm" (a column-major CUDA tensor) or "host" (a column-major NumPy array)."""
    if not isinstance(F, LU):
        raise TypeError(f"{what} needs the LU that lu_complex / lu_complex_ returned")
    A = F.factors
    if A is None:
        raise ValueError(f"{what}: this factorization is no longer valid (inv_complex_ overwrote its factors with the inverse)")
    if getattr(A, "ndim", None) != 2 or A.shape[0] != A.shape[1]:
        raise ValueError(f"{what} needs a square factorization")
    name = str(A.dtype).replace("torch.", "")
    if name not in ("complex128", "complex64"):
        raise TypeError(f"{what} serves ComplexF64/ComplexF32 factors only (got {A.dtype}); real factors go to inv / inv_ / det / "
                        "logabsdet / logdet")
    sfx = "cf64" if name == "complex128" else "cf32"
    n = int(A.shape[0])
    if _is_torch(A):
        if not A.is_cuda:
            raise _ffi.RfluError("torch factors must live on the MI355X (device='cuda'); host data goes in as NumPy")
        if not isinstance(F.ipiv, NotIPIV) and not (_is_torch(F.ipiv) and F.ipiv.is_cuda and str(F.ipiv.dtype) == "torch.int64"
                                                      and F.ipiv.numel() >= n and (n <= 1 or F.ipiv.stride(0) == 1)):
            raise TypeError("ipiv of GPU factors must be a contiguous int64 CUDA tensor of length n (or NotIPIV)")
        if n <= 1 or (A.stride(0) == 1 and A.stride(1) >= n):
            return A, n, sfx, "cm", (int(A.stride(1)) if n > 1 else 1)
        raise ValueError(f"{what}: the complex path is column-major only: the factors must be a column-major tensor (stride(0) == 1), as "
                         "lu_complex_ leaves them; row-major complex factors are not served")
    if not isinstance(A, np.ndarray):
        raise TypeError("factors must be a numpy.ndarray or a CUDA torch.Tensor")
    if not A.flags.f_contiguous:
        raise ValueError(f"{what}: the complex path is column-major only: host factors must be Fortran-ordered, as lu_complex_ leaves them")
    return A, n, sfx, "host", max(n, 1)


def _complex_view(X, trans: str):
    if trans == "N":
        return X
    if trans == "T":
        return X.T
    return X.T.conj()   # torch: a lazy conjugate view; NumPy has no such view, so a conjugated copy of the transposed view


def inv_complex_(F, *, trans="N", handle=None):
    """``LinearAlgebra.inv!(F::LU)`` for ``complex128`` / ``complex64`` factors: overwrite them with ``inv(A)`` (``rflu_getri_cf64`` /
    ``_cf32`` and their ``_dev`` forms) and return the array that held them.  About 4n^3/3 complex multiply-adds and no n x n workspace,
    against 2n^3 and an n x n identity for ``ldiv_complex_(F, I)``.

    ``F`` IS INVALID AFTERWARDS, exactly as after ``inv_``: ``F.factors`` is set to ``None``; use ``inv_complex`` to keep it.  The
    factors: a column-major CUDA tensor or a Fortran-ordered NumPy array; row-major complex factors are refused (the complex path is
    column-major only).  Raises ``SingularException(info)`` when ``F.info != 0`` or the library finds a ``u_ii`` with both parts zero
    -- the factors are then untouched and ``F`` stays valid.

    For complex matrices the adjoint and the transpose differ, and ``Transpose is Adjoint`` in this package, so which one is meant is
    said in LAPACK's letters as in ``ldiv_complex_batched_``: ``trans="T"`` returns the transposed view of the result
    (inv(transpose(A)) = transpose(inv(A))), ``trans="C"`` -- or ``Adjoint(F)`` -- the conjugate-transposed one (inv(A') = inv(A)')."""
    F, trans = _complex_trans(F, trans, "inv_complex_")
    A, n, sfx, kind, ld = _complex_square_factors(F, "inv_complex_")
    if F.info != 0:
        raise SingularException(abs(F.info))
    if n > 0:
        keep, ip = _ipiv_arg(F, kind)
        h, ap = _handle_for(A, kind, handle)
        info = ctypes.c_int64(0)
        h.call(f"rflu_getri_{sfx}" + ("" if kind == "host" else "_dev"), n, ap, ld, ip, ctypes.byref(info))
        del keep
        if info.value != 0:
            raise SingularException(int(info.value))
    F.factors = None
    return _complex_view(A, trans)


def inv_complex(F, *, trans="N", handle=None):
    """``inv(F::LU)`` for complex factors: ``inv_complex_`` on a copy of the factors; ``F`` stays intact.  ``trans`` / ``Adjoint(F)`` as
    there."""
    G, trans = _complex_trans(F, trans, "inv_complex")
    A = _complex_square_factors(G, "inv_complex")[0]
    C = A.clone() if _is_torch(A) else np.array(A, order="F", copy=True)
    return _complex_view(inv_complex_(LU(C, G.ipiv, G.info), handle=handle), trans)


def logabsdet_complex(F, *, trans="N", handle=None):
    """``logabsdet(F::LU)`` for complex factors -> ``(log|det A|, det A / |det A|)`` as a Python ``float`` and ``complex``
    (``rflu_logabsdet_cf64`` / ``_cf32`` and their ``_dev`` forms): the sum of ``log(hypot(re, im))`` over the diagonal and the product of
    its unit phases times the parity of the interchanges, in Float64 and in a fixed order for both element types.  Only the diagonal and
    ``ipiv`` are read.  A ``u_ii`` with both parts zero gives ``(-inf, 0j)``, a NaN ``(nan, nan+nanj)``; ``n == 0`` gives ``(0.0, 1+0j)``.
    ``trans="T"``: the same value (det(transpose(A)) = det(A)); ``trans="C"`` or ``Adjoint(F)``: the conjugate phase (det(A') is the
    conjugate of det(A))."""
    F, trans = _complex_trans(F, trans, "logabsdet_complex")
    A, n, sfx, kind, ld = _complex_square_factors(F, "logabsdet_complex")
    if n == 0:
        return 0.0, complex(1.0, 0.0)
    keep, ip = _ipiv_arg(F, kind)
    h, ap = _handle_for(A, kind, handle)
    la, sr, si = ctypes.c_double(0.0), ctypes.c_double(1.0), ctypes.c_double(0.0)
    h.call(f"rflu_logabsdet_{sfx}" + ("" if kind == "host" else "_dev"), n, ap, ld, ip, ctypes.byref(la), ctypes.byref(sr), ctypes.byref(si))
    del keep
    sign = complex(sr.value, si.value)
    return float(la.value), (sign.conjugate() if trans == "C" else sign)


def det_complex(F, *, trans="N", handle=None) -> complex:
    """``det(F::LU)`` for complex factors = ``sign * exp(logabs)`` of ``logabsdet_complex``; ``0j`` for a singular ``F``."""
    la, sg = logabsdet_complex(F, trans=trans, handle=handle)
    with np.errstate(over="ignore"):
        return complex(0.0, 0.0) if sg == 0 else sg * float(np.exp(np.float64(la)))


def logdet_complex(F, *, trans="N", handle=None) -> complex:
    """``logdet(F::LU)`` for complex factors: ``complex(logabs, angle(sign))`` of ``logabsdet_complex`` (Julia's ``log(det(F))`` on its
    principal branch; no domain error, a complex logarithm has none)."""
    la, sg = logabsdet_complex(F, trans=trans, handle=handle)
    return complex(la, float(np.angle(sg)))


def opnorm_complex(A, p=1, *, handle=None) -> float:
    """``opnorm(A, 1)`` / ``opnorm(A, Inf)`` of a ``complex128`` / ``complex64`` m x n matrix: the largest column / row sum of the moduli
    ``hypot(re, im)`` (LAPACK zlange / clange, ``rflu_lange_cf64_dev`` / ``_cf32_dev``), as a Python float.  Shapes and rules are those
    of ``opnorm``: Float64 moduli and sums in a fixed order for both element types, bit-identical from run to run and whatever the
    alignment; a column-major or row-major CUDA tensor, or a NumPy array (copied to the device).  A NaN in either part of any element
    gives NaN, even next to an Inf; an empty matrix gives 0.  Take it BEFORE ``lu_complex_`` overwrites ``A``.  ``Adjoint(A)`` swaps 1
    and inf; no ``trans`` letter is needed, because |conj z| = |z|: the transposed and the adjoint view have the same norms."""
    code = _norm_code(p, "opnorm_complex")
    if isinstance(A, Adjoint):
        A, code = A.parent, _swap_norm(code)
        if isinstance(A, Adjoint):
            raise TypeError("opnorm_complex of a doubly wrapped matrix: unwrap it first")
    if getattr(A, "ndim", None) != 2:
        raise ValueError("opnorm_complex needs a matrix")
    sfx = _ccond_sfx(A.dtype, "opnorm_complex")
    m, n = int(A.shape[0]), int(A.shape[1])
    if m == 0 or n == 0:
        return 0.0
    import torch

    if not _is_torch(A):
        if not isinstance(A, np.ndarray):
            raise TypeError("A must be a numpy.ndarray or a CUDA torch.Tensor")
        dev = torch.device("cuda", handle.device if handle is not None else 0)
        if A.flags.f_contiguous and not A.flags.c_contiguous:   # a Fortran-ordered array stays column-major on the device
            A = torch.from_numpy(np.ascontiguousarray(A.T)).to(dev).T
        else:
            A = torch.from_numpy(np.ascontiguousarray(A)).to(dev)
    if not A.is_cuda:
        raise _ffi.RfluError("torch input must live on the MI355X (device='cuda'); host data goes in as NumPy")
    if A.is_conj():
        A = A.resolve_conj()   # the moduli are the same; the library reads plain memory
    if A.stride(0) == 1 and (A.stride(1) >= m or n == 1):
        row_major, ld = 0, (int(A.stride(1)) if n > 1 else m)
    elif A.stride(1) == 1 and (A.stride(0) >= n or m == 1):
        row_major, ld = 1, (int(A.stride(0)) if m > 1 else n)
    else:
        raise ValueError("opnorm_complex: the matrix must be dense column-major or row-major (unit stride in one dimension)")
    h = handle or _ffi.default_handle(A.device.index or 0)
    h.set_stream(torch.cuda.current_stream(A.device).cuda_stream)
    out = ctypes.c_double(0.0)
    h.call(f"rflu_lange_{sfx}_dev", code, m, n, ctypes.c_void_p(A.data_ptr()), ld, row_major, ctypes.byref(out))
    return float(out.value)


def rcond_complex(F, anorm, p=1, *, handle=None) -> float:
    """``rcond`` for the ``LU`` that ``lu_complex`` / ``lu_complex_`` returned (LAPACK zgecon / cgecon, ``rflu_gecon_cf64`` / ``_cf32``
    and their ``_dev`` forms): ``anorm = opnorm_complex(A, p)`` taken before the factorization, ``||inv(A)||`` estimated by Higham's
    method (zlacn2: the pair of operators is M and its ADJOINT, the iterate is the phase vector ``v_i / |v_i|``) with at most 11 solves of
    one right-hand side; ``F`` is only read.  The factors: a column-major CUDA tensor or a Fortran-ordered NumPy array (the complex path
    is column-major only).  ``n == 0`` gives 1, ``anorm == 0`` or a ``u_ii`` with both parts zero gives 0, a NaN ``anorm`` or a NaN in
    the factors gives NaN; ``anorm < 0`` raises.  ``Adjoint(F)`` swaps 1 and inf; no ``trans`` letter is needed, because |conj z| = |z|:
    transpose(A) and A' have the same norms and the same condition number."""
    code = _norm_code(p, "rcond_complex")
    F, adj = _unwrap_adjoint(F, "rcond_complex")
    if isinstance(F, LU) and F.factors is not None:
        _ccond_sfx(F.factors.dtype, "rcond_complex")
    A, n, sfx, kind, ld = _complex_square_factors(F, "rcond_complex")
    if adj:
        code = _swap_norm(code)
    anorm = float(anorm)
    if anorm < 0.0:
        raise ValueError("rcond_complex: anorm must not be negative")
    if n == 0:
        return 1.0
    h, ap = _handle_for(A, kind, handle)
    out = ctypes.c_double(0.0)
    h.call(f"rflu_gecon_{sfx}" + ("" if kind == "host" else "_dev"), code, n, ap, ld, anorm, ctypes.byref(out))
    return float(out.value)


def cond_complex(A, p=1, *, handle=None) -> float:
    """``cond(A, 1)`` / ``cond(A, Inf)`` of a complex matrix as Julia computes them: ``opnorm_complex``, then ``lu_complex`` on a copy
    (``check=False``), then ``1 / rcond_complex``; ``inf`` when ``rcond == 0`` (a singular matrix).  ``A`` stays intact.  ``Adjoint(A)``
    swaps 1 and inf, which also serves transpose(A): |conj z| = |z|, so the two have the same condition number."""
    code = _norm_code(p, "cond_complex")
    if isinstance(A, Adjoint):
        A, code = A.parent, _swap_norm(code)
        if isinstance(A, Adjoint):
            raise TypeError("cond_complex of a doubly wrapped matrix: unwrap it first")
    if getattr(A, "ndim", None) != 2 or A.shape[0] != A.shape[1]:
        raise ValueError("cond_complex needs a square matrix")
    _ccond_sfx(A.dtype, "cond_complex")
    if A.shape[0] == 0:
        return 1.0
    p = 1 if code == _ffi.NORM_ONE else float("inf")
    anorm = opnorm_complex(A, p, handle=handle)
    rc = rcond_complex(lu_complex(A, check=False, handle=handle), anorm, p, handle=handle)
    return float("inf") if rc == 0.0 else 1.0 / rc


class NotConvergedError(ArithmeticError):
    """``ldiv_mixed(..., fallback=False)``: the refinement did not reach Float64 backward error within ``max_iter`` steps."""

    def __init__(self, iters: int):
        super().__init__(f"mixed-precision refinement did not converge ({-iters - 1} steps taken); the matrix is too ill-conditioned for "
                         "Float32 factors -- use lu / ldiv_ in Float64")
        self.iters = iters


@dataclass
class MixedLU:
    """Float32 factors of a Float64 matrix, for ``ldiv_mixed``: ``A`` (the caller's matrix, untouched -- the residuals need it),
    ``F32`` (n x n Float32, row-major, packed L\\U), ``ipiv`` (int64 CUDA tensor, 1-based; ``NotIPIV`` for NoPivot), ``info`` of the
    FLOAT32 factorization, ``anorm`` = ||A||_inf, and from the last ``ldiv_mixed``: ``iters`` (>= 0 refinement steps, converged; < 0 not
    converged) and ``fell_back`` (the Float64 factorization served it)."""

    A: object
    F32: object
    ipiv: object
    info: int
    anorm: float
    iters: int = 0
    fell_back: bool = False
    _f64: object = None   # the Float64 factorization of a copy of A, once a fallback needed it

    def issuccess(self) -> bool:
        return self.info == 0


def _check_mixed_matrix(A, cplx=False):
    """Shape, element type and layout of ``lu_mixed``'s / ``lu_complex_mixed``'s matrix -- before anything touches the library."""
    name = "lu_complex_mixed" if cplx else "lu_mixed"
    if getattr(A, "ndim", None) != 2:
        raise ValueError(f"{name} needs a matrix")
    dt = str(A.dtype).replace("torch.", "")
    if cplx and dt != "complex128":
        raise TypeError(f"lu_complex_mixed factors a ComplexF64 matrix in ComplexF32 and refines in ComplexF64 (got {A.dtype}); "
                        "a ComplexF32 matrix goes to lu_complex / lu_complex_ directly, a Float64 one to lu_mixed")
    if not cplx and dt != "float64":
        raise TypeError(f"lu_mixed factors a Float64 matrix in Float32 and refines in Float64 (got {A.dtype}); "
                        "a Float32 matrix goes to lu / lu_ directly, a ComplexF64 one to lu_complex_mixed / ldiv_complex_mixed")
    if A.shape[0] != A.shape[1]:
        raise ValueError(f"{name} needs a square matrix")


def _lu_mixed_call(A, pivot, blocksize, handle, cplx: bool) -> MixedLU:
    """``lu_mixed`` (``cplx`` false) and ``lu_complex_mixed``: the same checks, staging and call; the complex entry has no blocksize."""
    name = "lu_complex_mixed" if cplx else "lu_mixed"
    piv = normalize_pivot(pivot)
    _check_mixed_matrix(A, cplx)
    import torch

    if not _is_torch(A):
        if not isinstance(A, np.ndarray):
            raise TypeError("A must be a numpy.ndarray or a CUDA torch.Tensor")
        A = torch.from_numpy(np.ascontiguousarray(A.T)).to("cuda:0").T   # column-major on the device
    elif not A.is_cuda:
        raise _ffi.RfluError("torch input must live on the MI355X (device='cuda'); host data goes in as NumPy")
    n = int(A.shape[0])
    if n > 1 and not (A.stride(0) == 1 and A.stride(1) >= n):
        raise ValueError(f"{name}: the matrix must be dense column-major (stride(0) == 1, stride(1) >= n)")
    lda = int(A.stride(1)) if n > 1 else max(n, 1)
    ldf = (max(n, 1) + 15) // 16 * 16
    F32 = torch.empty((n, ldf), dtype=torch.complex64 if cplx else torch.float32, device=A.device)[:, :n]
    ipiv_t = torch.empty(n, dtype=torch.int64, device=A.device) if piv else None
    info, anorm = ctypes.c_int64(0), ctypes.c_double(0.0)
    if n > 0:
        h = handle or _ffi.default_handle(A.device.index or 0)
        h.set_stream(torch.cuda.current_stream(A.device).cuda_stream)
        head = (n, ctypes.c_void_p(A.data_ptr()), lda, ctypes.c_void_p(F32.data_ptr()), ldf,
                ctypes.c_void_p(ipiv_t.data_ptr() if ipiv_t is not None else 0), int(piv))
        if cplx:
            h.call("rflu_mixed_getrf_cf64_dev", *head, ctypes.byref(anorm), ctypes.byref(info))
        else:
            h.call("rflu_mixed_getrf_f64_dev", *head, int(blocksize or 0), ctypes.byref(anorm), ctypes.byref(info))
    inf = int(info.value)
    if not piv and NOPIVOT_NEGATIVE_INFO:
        inf = -inf
    return MixedLU(A, F32, ipiv_t if ipiv_t is not None else NotIPIV(n), inf, float(anorm.value))


def lu_mixed(A, pivot=True, *, blocksize=None, handle=None) -> MixedLU:
    """Factor a Float32 copy of the Float64 matrix ``A`` (``rflu_mixed_getrf_f64_dev``): one pass demotes ``A`` into the library's
    row-major layout and yields ||A||_inf, the Float32 factorization runs in place there.  ``A`` is NOT modified and is kept by
    reference.  ``A``: a CUDA Float64 tensor, column-major (``stride(0) == 1``) like the other device entries; a NumPy array is staged
    through a torch tensor.  A zero pivot of the Float32 factorization is reported in ``info``, never raised: ``ldiv_mixed`` decides.
    A complex matrix raises ``TypeError``: it goes to ``lu_complex_mixed``."""
    return _lu_mixed_call(A, pivot, blocksize, handle, False)


def lu_complex_mixed(A, pivot=True, *, handle=None) -> MixedLU:
    """``lu_mixed`` for a ComplexF64 matrix (``rflu_mixed_getrf_cf64_dev``, LAPACK ``zcgesv``'s scheme): one pass demotes ``A`` into a
    ComplexF32 row-major image and yields ||A||_inf (the largest row sum of moduli), the ComplexF32 recursion factors it in place.
    Returns the same ``MixedLU``: ``F32`` is a complex64 row-major tensor, ``info`` that of the ComplexF32 factorization (the pivot is
    the row of largest modulus, as in ``lu_complex_``).  ``A`` is NOT modified and is kept by reference; there is no ``blocksize``."""
    return _lu_mixed_call(A, pivot, None, handle, True)


def ldiv_mixed(F: MixedLU, B, *, max_iter=30, fallback=True, handle=None):
    """``A \\ B`` to Float64 backward error with the Float32 factors ``F`` (``rflu_mixed_getrs_f64_dev``): solve, Float64 residual, and
    while some column misses ``||r||_inf <= ||x||_inf ||A||_inf eps sqrt(n)`` another Float32 solve of the residual.  Returns a NEW ``X``
    (``B`` is only read; a NumPy ``B`` gives a NumPy ``X``).  ``F.iters`` records the steps.

    When the Float32 factorization hit a zero pivot (``F.info != 0``) or the refinement does not converge within ``max_iter`` steps:
    ``fallback=True`` solves with the Float64 ``lu`` / ``ldiv_`` of a copy of ``A`` (kept in ``F`` for later calls) and sets
    ``F.fell_back``; a matrix that is singular in Float64 too raises ``SingularException`` as ``lu`` does.  ``fallback=False`` raises
    ``SingularException`` / ``NotConvergedError`` instead.  The library itself never falls back.  Complex factors (from
    ``lu_complex_mixed``) raise ``TypeError``: they go to ``ldiv_complex_mixed``."""
    return _ldiv_mixed_call(F, B, max_iter, fallback, handle, False)


def ldiv_complex_mixed(F: MixedLU, B, *, max_iter=30, fallback=True, handle=None):
    """``ldiv_mixed`` with the ComplexF32 factors ``lu_complex_mixed`` returned (``rflu_mixed_getrs_cf64_dev``): the same loop, rule and
    return value, the norms as largest moduli.  Every ComplexF32 solve works on the row-major factors as they lie.  ``fallback=True``
    goes through ``lu_complex`` / ``ldiv_complex_`` in ComplexF64 (also when an entry of ``A`` overflows Float32 and the Inf it becomes
    turns into NaN in the elimination, which ends as non-convergence); ``fallback=False`` raises ``SingularException`` /
    ``NotConvergedError``."""
    return _ldiv_mixed_call(F, B, max_iter, fallback, handle, True)


def _ldiv_mixed_call(F, B, max_iter, fallback, handle, cplx: bool):
    """``ldiv_mixed`` (``cplx`` false) and ``ldiv_complex_mixed``: the same checks, staging, call and fallback rule."""
    name, maker, want = ("ldiv_complex_mixed", "lu_complex_mixed", "complex128") if cplx else ("ldiv_mixed", "lu_mixed", "float64")
    if not isinstance(F, MixedLU):
        raise TypeError(f"{name} needs the MixedLU that {maker} returned")
    A = F.A
    if str(A.dtype).replace("torch.", "") != want:
        raise TypeError(f"{name} needs the MixedLU that {maker} returned; these factors belong to "
                        f"{'ldiv_mixed' if cplx else 'ldiv_complex_mixed'}")
    n = int(A.shape[0])
    if getattr(B, "ndim", 0) not in (1, 2):
        raise ValueError("B must be a vector or a matrix")
    if B.shape[0] != n:
        raise ValueError("right-hand side has the wrong number of rows")
    if str(B.dtype).replace("torch.", "") != want:
        raise TypeError("B must be ComplexF64 like A" if cplx else "B must be Float64 like A")
    import torch

    host = not _is_torch(B)
    if host:
        if not isinstance(B, np.ndarray):
            raise TypeError("B must be a numpy.ndarray or a CUDA torch.Tensor")
        Bd = torch.from_numpy(np.ascontiguousarray(B.T)).to(A.device).T if B.ndim == 2 else torch.from_numpy(np.ascontiguousarray(B)).to(A.device)
    else:
        if not B.is_cuda:
            raise TypeError("B must be a CUDA tensor (or a NumPy array, which is staged)")
        Bd = B
    nrhs = 1 if Bd.ndim == 1 else int(Bd.shape[1])
    if Bd.ndim == 1:
        if n > 1 and Bd.stride(0) != 1:
            raise ValueError("a vector right-hand side must be contiguous (stride 1); copy the view first")
        ldb = max(n, 1)
    else:
        if n > 1 and not (Bd.stride(0) == 1 and (nrhs <= 1 or Bd.stride(1) >= n)):
            raise ValueError("B must be column-major like A")
        ldb = int(Bd.stride(1)) if (nrhs > 1 and n > 1) else max(n, 1)
    X = torch.empty(n, dtype=A.dtype, device=A.device) if Bd.ndim == 1 else torch.empty((nrhs, n), dtype=A.dtype, device=A.device).T
    F.fell_back = False
    F.iters = 0
    ok = F.info == 0
    if ok and n > 0 and nrhs > 0:
        h = handle or _ffi.default_handle(A.device.index or 0)
        h.set_stream(torch.cuda.current_stream(A.device).cuda_stream)
        iters = ctypes.c_int(0)
        h.call("rflu_mixed_getrs_cf64_dev" if cplx else "rflu_mixed_getrs_f64_dev", n, nrhs, ctypes.c_void_p(A.data_ptr()), int(A.stride(1)) if n > 1 else 1,
               ctypes.c_void_p(F.F32.data_ptr()), int(F.F32.stride(0)) if n > 1 else 1,
               ctypes.c_void_p(0 if isinstance(F.ipiv, NotIPIV) else F.ipiv.data_ptr()), float(F.anorm), ctypes.c_void_p(Bd.data_ptr()), ldb,
               ctypes.c_void_p(X.data_ptr()), max(n, 1), int(max_iter), ctypes.byref(iters))
        F.iters = int(iters.value)
        ok = F.iters >= 0
    if not ok:
        if not fallback:
            if F.info != 0:
                raise SingularException(abs(F.info))
            raise NotConvergedError(F.iters)
        if F._f64 is None:   # check=True: SingularException when Float64 is singular too
            F._f64 = (lu_complex if cplx else lu)(A, not isinstance(F.ipiv, NotIPIV), handle=handle)
        X.copy_(Bd)
        (ldiv_complex_ if cplx else ldiv_)(F._f64, X, handle=handle)
        F.fell_back = True
    return X.cpu().numpy() if host else X


@dataclass
class BatchedLU:
    """``batch`` factorizations in one object: ``factors`` (batch, m, n) aliasing the caller's tensor, ``ipiv`` (batch, min(m, n))
    int64 on the device, 1-based (``NotIPIV`` for NoPivot without a pivot buffer), ``info`` int64 CUDA tensor of length ``batch``
    (0 or the first zero pivot of that matrix; negative for NoPivot under ``NOPIVOT_NEGATIVE_INFO``, as ``lu_`` reports it)."""

    factors: object
    ipiv: object
    info: object

    def issuccess(self) -> bool:
        return not bool((self.info != 0).any().item())


def _batched_layout(A, what: str):
    """(row_major, ld, batch stride) of a (batch, r, c) tensor whose matrices are dense column-major or row-major and do not overlap."""
    b, r, c = (int(x) for x in A.shape)
    s0, s1, s2 = (int(x) for x in A.stride())
    if s1 == 1 and (s2 >= max(r, 1) or c <= 1):
        row_major, ld, span = 0, (s2 if c > 1 else max(r, 1)), (c - 1) * (s2 if c > 1 else 0) + r
    elif s2 == 1 and (s1 >= max(c, 1) or r <= 1):
        row_major, ld, span = 1, (s1 if r > 1 else max(c, 1)), (r - 1) * (s1 if r > 1 else 0) + c
    else:
        raise ValueError(f"{what}: every matrix must be dense column-major (stride(1) == 1) or row-major (stride(2) == 1)")
    if b > 1 and r > 0 and c > 0 and s0 < span:
        raise ValueError(f"{what}: the matrices of the batch overlap (batch stride {s0} < {span})")
    return row_major, ld, (s0 if b > 1 else max(span, 1))


def _batched_sfx(dtype, what: str) -> str:
    """``_sfx`` for the real batched functions: a complex batch is pointed at the functions that serve it."""
    if str(dtype).replace("torch.", "") in ("complex128", "complex64"):
        raise TypeError(f"{what} serves Float64/Float32 only (got {dtype}); ComplexF64/ComplexF32 batches go to lu_complex_batched_ / "
                        "lu_complex_batched / ldiv_complex_batched_")
    return _sfx(dtype)


def _check_batched_info(info_t, piv: bool):
    bad = (info_t != 0).nonzero()
    if bad.numel():
        i = int(bad[0, 0].item())
        raise SingularException(abs(int(info_t[i].item())), i)


def _lu_batched_call(A, ipiv, pivot, check, handle, what: str, sfx_of) -> BatchedLU:
    """The checks and the call shared by ``lu_batched_`` and ``lu_complex_batched_``; ``sfx_of`` maps the dtype to the entry's suffix
    or raises ``TypeError``.  Every check comes before the library is touched."""
    piv = normalize_pivot(pivot)
    if not _is_torch(A):
        raise TypeError(f"{what} works on CUDA torch tensors (the batch lives in HBM)")
    if A.ndim != 3:
        raise ValueError(f"{what} needs a 3-D tensor (batch, m, n)")
    import torch

    if not A.is_cuda:
        raise TypeError(f"{what}: the batch must live on the MI355X (device='cuda')")
    sfx = sfx_of(A.dtype, what)
    batch, m, n = (int(x) for x in A.shape)
    mn = min(m, n)
    row_major, ld, stride_a = _batched_layout(A, what)
    if ipiv is None:
        ipiv_t = torch.empty((batch, mn), dtype=torch.int64, device=A.device) if piv else None
    else:
        ipiv_t = ipiv
        if not (_is_torch(ipiv_t) and ipiv_t.is_cuda and ipiv_t.dtype == torch.int64):
            raise TypeError("ipiv for a batch must be an int64 CUDA tensor")
        if ipiv_t.ndim != 2 or ipiv_t.shape[0] != batch or ipiv_t.shape[1] != mn:
            raise ValueError(f"ipiv must have shape (batch, min(m, n)) = ({batch}, {mn})")
        if mn > 1 and ipiv_t.stride(1) != 1 or batch > 1 and ipiv_t.stride(0) < mn:
            raise ValueError("ipiv: unit stride along a row and a batch stride of at least min(m, n)")
    stride_ip = 0 if ipiv_t is None else (int(ipiv_t.stride(0)) if batch > 1 else max(mn, 1))
    info_t = torch.zeros(batch, dtype=torch.int64, device=A.device)
    if batch > 0 and m > 0 and n > 0:
        h = handle or _ffi.default_handle(A.device.index or 0)
        h.set_stream(torch.cuda.current_stream(A.device).cuda_stream)
        h.call(f"rflu_getrf_batched_{sfx}_dev", batch, m, n, ctypes.c_void_p(A.data_ptr()), ld, stride_a, row_major,
               ctypes.c_void_p(ipiv_t.data_ptr() if ipiv_t is not None else 0), stride_ip, int(piv), ctypes.c_void_p(info_t.data_ptr()))
    if not piv and NOPIVOT_NEGATIVE_INFO:
        info_t = -info_t
    if _as_bool(check):
        _check_batched_info(info_t, piv)
    return BatchedLU(A, ipiv_t if ipiv_t is not None else NotIPIV(mn), info_t)


def _batched_copy(A, what: str):
    """A copy of a batch that keeps the layout of its matrices (``lu_batched`` / ``lu_complex_batched``)."""
    if not _is_torch(A) or A.ndim != 3:
        raise ValueError(f"{what} needs a 3-D CUDA tensor (batch, m, n)")
    C = A.transpose(1, 2).contiguous().transpose(1, 2) if (A.stride(1) == 1 and A.shape[2] > 1) else A.contiguous()
    return C.clone() if C.data_ptr() == A.data_ptr() else C


def _ldiv_batched_call(F, B, trans: int, check, handle, what: str, made_by: str, sfx_of):
    """The checks and the call shared by ``ldiv_batched_`` and ``ldiv_complex_batched_``; ``trans`` is the C entry's value."""
    if not isinstance(F, BatchedLU):
        raise TypeError(f"{what} needs the BatchedLU that {made_by} returned")
    A = F.factors
    import torch

    batch, m, n = (int(x) for x in A.shape)
    if m != n:
        raise ValueError("ldiv! needs square factorizations")
    if not (_is_torch(B) and B.is_cuda and B.dtype == A.dtype):
        raise TypeError("B must be a CUDA tensor of the factorization's dtype")
    if B.ndim not in (2, 3) or B.shape[0] != batch or B.shape[1] != n:
        raise ValueError(f"B must have shape (batch, n) or (batch, n, nrhs) with batch = {batch}, n = {n}")
    row_major, ld, stride_f = _batched_layout(A, what)
    nrhs = 1 if B.ndim == 2 else int(B.shape[2])
    if B.ndim == 2:
        if n > 1 and B.stride(1) != 1 or batch > 1 and B.stride(0) < n:
            raise ValueError("a batch of vectors must have unit stride along a vector and a batch stride of at least n")
        ldb, stride_b = (n if not row_major else 1), (int(B.stride(0)) if batch > 1 else max(n, 1))
    else:
        b_rm, ldb, stride_b = _batched_layout(B, f"{what} (B)")
        if b_rm != row_major and n > 1 and nrhs > 1:
            raise ValueError("B must have the orientation of the factors (column-major with column-major, row-major with row-major)")
        if b_rm != row_major:   # a single row or column fits both readings: take the factors'
            ldb = max(nrhs, 1) if row_major else max(n, 1)
    nopiv = isinstance(F.ipiv, NotIPIV)
    if not nopiv and not (_is_torch(F.ipiv) and F.ipiv.is_cuda and F.ipiv.dtype == torch.int64):
        raise TypeError("ipiv of a batch must be an int64 CUDA tensor (or NotIPIV)")
    if _as_bool(check):
        _check_batched_info(F.info, True)
    if batch > 0 and n > 0 and nrhs > 0:
        sfx = sfx_of(A.dtype, what)
        h = handle or _ffi.default_handle(A.device.index or 0)
        h.set_stream(torch.cuda.current_stream(A.device).cuda_stream)
        stride_ip = 0 if nopiv else (int(F.ipiv.stride(0)) if batch > 1 else max(n, 1))
        h.call(f"rflu_getrs_batched_{sfx}_dev", batch, n, nrhs, ctypes.c_void_p(A.data_ptr()), ld, stride_f, row_major,
               ctypes.c_void_p(0 if nopiv else F.ipiv.data_ptr()), stride_ip, ctypes.c_void_p(B.data_ptr()), ldb, stride_b, trans)
    return B


def lu_batched_(A, ipiv=None, pivot=True, *, check=True, handle=None) -> BatchedLU:
    """``lu!`` on every matrix of a batch at once: ``A`` is a 3-D CUDA tensor (batch, m, n) whose matrices are dense column-major
    (``stride(1) == 1``, e.g. a C-contiguous (batch, n, m) tensor seen through ``.transpose(1, 2)``) or row-major (``stride(2) == 1``),
    at any batch stride that keeps them apart; factored in place by ``rflu_getrf_batched_*_dev``.  Up to 128 rows and columns the whole
    batch is ONE kernel launch (``last_path() == "hip-batched"``); larger matrices are looped over the single-matrix path.

    ``ipiv``: None -> allocated, (batch, min(m, n)) int64 (``NotIPIV`` for NoPivot); or a CUDA int64 tensor of that shape with unit
    stride along a row -- with NoPivot it comes back filled with the identity (src/lu.jl:111-113).  ``check=True`` copies ``info``
    back and raises ``SingularException`` with the first failing matrix's ``info`` and its index in ``batch_index``."""
    return _lu_batched_call(A, ipiv, pivot, check, handle, "lu_batched_", _batched_sfx)


def lu_batched(A, pivot=True, **kwargs) -> BatchedLU:
    """``lu`` on every matrix of a batch: ``lu_batched_`` on a copy that keeps the layout of ``A``'s matrices."""
    return lu_batched_(_batched_copy(A, "lu_batched"), None, pivot, **kwargs)


def ldiv_batched_(F, B, *, trans=False, check=True, handle=None):
    """``ldiv!`` on every system of a batch: overwrite ``B`` -- (batch, n) or (batch, n, nrhs), in the orientation of the factors --
    with ``A_b \\ B_b``, or with ``A_b' \\ B_b`` for ``trans=True`` / ``Adjoint(F)``.  Served by ``rflu_getrs_batched_*_dev`` (one launch
    up to n = 128).  ``check=True`` raises ``SingularException`` (with ``batch_index``) when some ``F.info`` is non-zero; with
    ``check=False`` the solve runs and only the singular matrices' own right-hand sides come back non-finite."""
    if isinstance(F, Adjoint):
        F, trans = F.parent, not trans
        if isinstance(F, Adjoint):
            raise TypeError("ldiv! of a doubly wrapped factorization: unwrap it first")
    return _ldiv_batched_call(F, B, int(bool(trans)), check, handle, "ldiv_batched_", "lu_batched_", _batched_sfx)


def _batched_square(F, what: str):
    F, adj = _unwrap_adjoint(F, what)
    if not isinstance(F, BatchedLU):
        raise TypeError(f"{what} needs the BatchedLU that lu_batched_ returned")
    A = F.factors
    if not (_is_torch(A) and A.is_cuda) or A.ndim != 3:
        raise TypeError(f"{what}: the factors must be a 3-D CUDA tensor")
    if A.shape[1] != A.shape[2]:
        raise ValueError(f"{what} needs square factorizations")
    sfx = _sfx(A.dtype)
    row_major, ld, stride_f = _batched_layout(A, what)
    return F, adj, A, sfx, row_major, ld, stride_f


def inv_batched(F, *, check=True, handle=None):
    """``inv`` of every matrix of a batch from its factors (``rflu_getri_batched_*_dev``; one launch up to n = 128, no identity tensor
    anywhere): returns a NEW (batch, n, n) CUDA tensor in the orientation of the factors; ``F`` stays intact.  ``check=True`` raises
    ``SingularException`` (with ``batch_index``) when some ``F.info`` is non-zero; with ``check=False`` only the singular matrices' own
    inverses come back non-finite.  ``Adjoint(F)``: the transposed views."""
    F, adj, A, sfx, row_major, ld, stride_f = _batched_square(F, "inv_batched")
    import torch

    batch, n = int(A.shape[0]), int(A.shape[1])
    if _as_bool(check):
        _check_batched_info(F.info, True)
    X = torch.empty((batch, n, n), dtype=A.dtype, device=A.device)
    if not row_major:
        X = X.transpose(1, 2)
    if batch > 0 and n > 0:
        h = handle or _ffi.default_handle(A.device.index or 0)
        h.set_stream(torch.cuda.current_stream(A.device).cuda_stream)
        nopiv = isinstance(F.ipiv, NotIPIV)
        stride_ip = 0 if nopiv else (int(F.ipiv.stride(0)) if batch > 1 else max(n, 1))
        info_t = torch.zeros(batch, dtype=torch.int64, device=A.device)
        h.call(f"rflu_getri_batched_{sfx}_dev", batch, n, ctypes.c_void_p(A.data_ptr()), ld, stride_f, row_major,
               ctypes.c_void_p(0 if nopiv else F.ipiv.data_ptr()), stride_ip, ctypes.c_void_p(X.data_ptr()), n, n * n,
               ctypes.c_void_p(info_t.data_ptr()))
        if _as_bool(check):
            _check_batched_info(info_t, True)
    return X.transpose(1, 2) if adj else X


def logabsdet_batched(F, *, handle=None):
    """``logabsdet`` of every matrix of a batch (``rflu_logabsdet_batched_*_dev``, one launch): ``(logabs, sign)``, two Float64 CUDA
    tensors of length ``batch``; entry b is bit-identical to ``logabsdet`` on matrix b's factors."""
    F, _, A, sfx, row_major, ld, stride_f = _batched_square(F, "logabsdet_batched")
    import torch

    batch, n = int(A.shape[0]), int(A.shape[1])
    la = torch.zeros(batch, dtype=torch.float64, device=A.device)
    sg = torch.ones(batch, dtype=torch.float64, device=A.device)
    if batch > 0 and n > 0:
        h = handle or _ffi.default_handle(A.device.index or 0)
        h.set_stream(torch.cuda.current_stream(A.device).cuda_stream)
        nopiv = isinstance(F.ipiv, NotIPIV)
        stride_ip = 0 if nopiv else (int(F.ipiv.stride(0)) if batch > 1 else max(n, 1))
        h.call(f"rflu_logabsdet_batched_{sfx}_dev", batch, n, ctypes.c_void_p(A.data_ptr()), ld, stride_f,
               ctypes.c_void_p(0 if nopiv else F.ipiv.data_ptr()), stride_ip, ctypes.c_void_p(la.data_ptr()), ctypes.c_void_p(sg.data_ptr()))
    return la, sg


def det_batched(F, *, handle=None):
    """``det`` of every matrix of a batch: ``sign * exp(logabs)`` of ``logabsdet_batched`` (0.0 for a singular matrix), a Float64 CUDA
    tensor of length ``batch``."""
    import torch

    la, sg = logabsdet_batched(F, handle=handle)
    return torch.where(sg == 0, torch.zeros_like(sg), sg * torch.exp(la))


def opnorm_batched(A, p=1, *, handle=None):
    """``opnorm(A_b, p)`` of every matrix of a (batch, m, n) CUDA tensor (``rflu_lange_batched_*_dev``; one workgroup per matrix up to
    128 x 128): a Float64 CUDA tensor of length ``batch``, entry b bit-identical to ``opnorm`` on matrix b.  ``Adjoint(A)`` swaps 1 and inf."""
    code = _norm_code(p, "opnorm_batched")
    if isinstance(A, Adjoint):
        A, code = A.parent, _swap_norm(code)
    if not _is_torch(A) or A.ndim != 3:
        raise TypeError("opnorm_batched needs a 3-D CUDA tensor (batch, m, n)")
    sfx = _cond_sfx(A.dtype, "opnorm_batched")
    if not A.is_cuda:
        raise TypeError("opnorm_batched: the batch must live on the MI355X (device='cuda')")
    import torch

    batch, m, n = (int(x) for x in A.shape)
    row_major, ld, stride_a = _batched_layout(A, "opnorm_batched")
    out = torch.zeros(batch, dtype=torch.float64, device=A.device)
    if batch > 0 and m > 0 and n > 0:
        h = handle or _ffi.default_handle(A.device.index or 0)
        h.set_stream(torch.cuda.current_stream(A.device).cuda_stream)
        h.call(f"rflu_lange_batched_{sfx}_dev", code, batch, m, n, ctypes.c_void_p(A.data_ptr()), ld, stride_a, row_major,
               ctypes.c_void_p(out.data_ptr()))
    return out


def rcond_batched(F, anorm, p=1, *, handle=None):
    """``rcond`` of every matrix of a batch from its factors (``rflu_gecon_batched_*_dev``: ONE launch up to n = 128, the whole estimator
    inside the kernel on the factors held in LDS; larger matrices are looped over ``rflu_gecon_*``).  ``anorm``: a Float64 CUDA tensor of
    length ``batch`` (``opnorm_batched`` before the factorization).  Returns a Float64 CUDA tensor of length ``batch``; a singular member
    gives 0 and a NaN member NaN in its own entry only.  ``Adjoint(F)`` swaps 1 and inf."""
    code = _norm_code(p, "rcond_batched")
    G, adj = _unwrap_adjoint(F, "rcond_batched")
    if isinstance(G, BatchedLU) and _is_torch(G.factors):
        _cond_sfx(G.factors.dtype, "rcond_batched")
    F, adj, A, sfx, row_major, ld, stride_f = _batched_square(F, "rcond_batched")
    if adj:
        code = _swap_norm(code)
    import torch

    batch, n = int(A.shape[0]), int(A.shape[1])
    if not (_is_torch(anorm) and anorm.is_cuda and anorm.dtype == torch.float64 and anorm.ndim == 1 and anorm.shape[0] == batch
            and (batch <= 1 or anorm.stride(0) == 1)):
        raise TypeError("rcond_batched: anorm must be a contiguous Float64 CUDA tensor of length batch")
    out = torch.ones(batch, dtype=torch.float64, device=A.device)
    if batch > 0 and n > 0:
        h = handle or _ffi.default_handle(A.device.index or 0)
        h.set_stream(torch.cuda.current_stream(A.device).cuda_stream)
        h.call(f"rflu_gecon_batched_{sfx}_dev", code, batch, n, ctypes.c_void_p(A.data_ptr()), ld, stride_f, row_major,
               ctypes.c_void_p(anorm.data_ptr()), ctypes.c_void_p(out.data_ptr()))
    return out


def cond_batched(A, p=1, *, handle=None):
    """``cond(A_b, p)`` of every matrix of a (batch, n, n) CUDA tensor: ``opnorm_batched``, ``lu_batched`` on a copy (``check=False``),
    ``1 / rcond_batched``; ``inf`` where ``rcond == 0``.  A Float64 CUDA tensor of length ``batch``."""
    code = _norm_code(p, "cond_batched")
    if isinstance(A, Adjoint):
        A, code = A.parent, _swap_norm(code)
    if not _is_torch(A) or A.ndim != 3 or A.shape[1] != A.shape[2]:
        raise ValueError("cond_batched needs a 3-D CUDA tensor (batch, n, n)")
    _cond_sfx(A.dtype, "cond_batched")
    import torch

    p = 1 if code == _ffi.NORM_ONE else float("inf")
    anorm = opnorm_batched(A, p, handle=handle)
    rc = rcond_batched(lu_batched(A, check=False, handle=handle), anorm, p, handle=handle)
    return torch.where(rc == 0, torch.full_like(rc, float("inf")), 1.0 / rc)


def _cbatched_sfx(dtype, what: str) -> str:
    name = str(dtype).replace("torch.", "")
    if name == "complex128":
        return "cf64"
    if name == "complex64":
        return "cf32"
    raise TypeError(f"{what} serves ComplexF64/ComplexF32 only (got {dtype}); real batches go to lu_batched_ / ldiv_batched_")


def lu_complex_batched_(A, ipiv=None, pivot=True, *, check=True, handle=None) -> BatchedLU:
    """``lu!`` on every matrix of a ``complex128`` / ``complex64`` batch at once: ``lu_batched_`` for complex elements, served by
    ``rflu_getrf_batched_cf64_dev`` / ``_cf32_dev``.  ``A``: a 3-D CUDA tensor (batch, m, n) whose matrices are dense column-major
    (``stride(1) == 1``) or row-major (``stride(2) == 1``) at any batch stride that keeps them apart; factored in place.  Per matrix the
    rule of ``lu_complex_``: the pivot is the row of largest modulus ``abs(z)`` (strict ``>``, the lowest row on ties), not LAPACK's
    ``|re| + |im|``.  Up to 128 (``complex64``) / 64 (``complex128``) rows and columns the whole batch is ONE kernel launch
    (``last_path() == "hip-batched"``); larger column-major matrices are looped over the single-matrix complex path, larger row-major
    ones are refused by the library (that path is column-major only).

    ``ipiv``, ``check`` -> ``SingularException`` with ``batch_index``, the NoPivot sign of ``info`` and the returned ``BatchedLU`` are
    those of ``lu_batched_``."""
    return _lu_batched_call(A, ipiv, pivot, check, handle, "lu_complex_batched_", _cbatched_sfx)


def lu_complex_batched(A, pivot=True, **kwargs) -> BatchedLU:
    """``lu`` on every matrix of a complex batch: ``lu_complex_batched_`` on a copy that keeps the layout of ``A``'s matrices."""
    return lu_complex_batched_(_batched_copy(A, "lu_complex_batched"), None, pivot, **kwargs)


_CBATCHED_TRANS = {"N": 0, "T": 1, "C": 2}


def ldiv_complex_batched_(F, B, *, trans="N", check=True, handle=None):
    """``ldiv!`` on every system of a complex batch: overwrite ``B`` -- (batch, n) or (batch, n, nrhs), in the orientation of the
    factors -- with ``A_b \\ B_b`` (``trans="N"``), ``transpose(A_b) \\ B_b`` (``"T"``) or ``A_b' \\ B_b`` (``"C"``, the conjugate
    transpose); LAPACK's letters, because for complex matrices the last two differ and a flag could not say which is meant.
    ``Adjoint(F)`` means ``"C"`` (and takes no ``trans`` besides the default); a doubly wrapped factorization is refused.  Served by
    ``rflu_getrs_batched_cf64_dev`` / ``_cf32_dev``.  ``check`` as in ``ldiv_batched_``."""
    if not isinstance(trans, str) or trans not in _CBATCHED_TRANS:
        raise ValueError(f'trans must be "N", "T" or "C", got {trans!r}')
    if isinstance(F, Adjoint):
        F = F.parent
        if isinstance(F, Adjoint):
            raise TypeError("ldiv! of a doubly wrapped factorization: unwrap it first")
        if trans != "N":
            raise ValueError('Adjoint(F) already means trans="C": pass the plain BatchedLU together with trans')
        trans = "C"
    return _ldiv_batched_call(F, B, _CBATCHED_TRANS[trans], check, handle, "ldiv_complex_batched_", "lu_complex_batched_", _cbatched_sfx)


def logabsdet_complex_batched(F, *, trans="N", handle=None):
    """``logabsdet_complex`` of every matrix of the ``BatchedLU`` that ``lu_complex_batched_`` returned
    (``rflu_logabsdet_batched_cf64_dev`` / ``_cf32_dev``, one launch, any n, both orientations of the factors -- only diagonals are
    read): ``(logabs, sign)``, a Float64 and a ``complex128`` CUDA tensor of length ``batch``; entry b is bit-identical to
    ``logabsdet_complex`` on matrix b's factors.  ``trans`` / ``Adjoint(F)`` as in ``logabsdet_complex``."""
    F, trans = _complex_trans(F, trans, "logabsdet_complex_batched")
    if not isinstance(F, BatchedLU):
        raise TypeError("logabsdet_complex_batched needs the BatchedLU that lu_complex_batched_ returned")
    A = F.factors
    if not (_is_torch(A) and A.is_cuda) or A.ndim != 3:
        raise TypeError("logabsdet_complex_batched: the factors must be a 3-D CUDA tensor")
    if A.shape[1] != A.shape[2]:
        raise ValueError("logabsdet_complex_batched needs square factorizations")
    sfx = _cbatched_sfx(A.dtype, "logabsdet_complex_batched")
    row_major, ld, stride_f = _batched_layout(A, "logabsdet_complex_batched")
    import torch

    batch, n = int(A.shape[0]), int(A.shape[1])
    la = torch.zeros(batch, dtype=torch.float64, device=A.device)
    sg = torch.zeros((batch, 2), dtype=torch.float64, device=A.device)
    sg[:, 0] = 1.0
    if batch > 0 and n > 0:
        h = handle or _ffi.default_handle(A.device.index or 0)
        h.set_stream(torch.cuda.current_stream(A.device).cuda_stream)
        nopiv = isinstance(F.ipiv, NotIPIV)
        stride_ip = 0 if nopiv else (int(F.ipiv.stride(0)) if batch > 1 else max(n, 1))
        h.call(f"rflu_logabsdet_batched_{sfx}_dev", batch, n, ctypes.c_void_p(A.data_ptr()), ld, stride_f,
               ctypes.c_void_p(0 if nopiv else F.ipiv.data_ptr()), stride_ip, ctypes.c_void_p(la.data_ptr()), ctypes.c_void_p(sg.data_ptr()))
    sign = torch.view_as_complex(sg)
    return la, (sign.conj().resolve_conj() if trans == "C" else sign)


def det_complex_batched(F, *, trans="N", handle=None):
    """``det_complex`` of every matrix of a complex batch: ``sign * exp(logabs)`` of ``logabsdet_complex_batched`` (0 for a singular
    matrix), a ``complex128`` CUDA tensor of length ``batch``."""
    import torch

    la, sg = logabsdet_complex_batched(F, trans=trans, handle=handle)
    return torch.where(sg == 0, torch.zeros_like(sg), sg * torch.exp(la))


def inv_complex_batched(F, *, trans="N", check=True, handle=None):
    """``inv`` of every matrix of the ``BatchedLU`` that ``lu_complex_batched_`` returned (``rflu_getri_batched_cf64_dev`` /
    ``_cf32_dev``; one launch up to n = 64 for ``complex128`` and n = 128 for ``complex64``, no identity tensor anywhere): returns a NEW
    dense (batch, n, n) CUDA tensor in the orientation of the factors that holds ``inv(A_b)`` (``trans="N"``), ``inv(transpose(A_b))``
    (``"T"``) or ``inv(A_b')`` (``"C"``, or ``Adjoint(F)``; LAPACK's letters as in ``ldiv_complex_batched_``).  The three cost the
    same: the kernel stores the one result transposed, and conjugated for ``"C"``, so what comes back is plain memory and never a lazily
    conjugated view (``is_conj()`` is false).  ``F`` stays intact.  ``check=True`` raises ``SingularException`` (with ``batch_index``)
    when some ``F.info`` is non-zero or the library finds a ``u_ii`` with both parts zero; with ``check=False`` only the singular
    matrices' own inverses come back non-finite.  Larger column-major matrices are looped over the single-matrix complex path, larger
    row-major ones are refused by the library (that path is column-major only)."""
    F, trans = _complex_trans(F, trans, "inv_complex_batched")
    if not isinstance(F, BatchedLU):
        raise TypeError("inv_complex_batched needs the BatchedLU that lu_complex_batched_ returned")
    A = F.factors
    if not (_is_torch(A) and A.is_cuda) or A.ndim != 3:
        raise TypeError("inv_complex_batched: the factors must be a 3-D CUDA tensor")
    if A.shape[1] != A.shape[2]:
        raise ValueError("inv_complex_batched needs square factorizations")
    sfx = _cbatched_sfx(A.dtype, "inv_complex_batched")
    row_major, ld, stride_f = _batched_layout(A, "inv_complex_batched")
    import torch

    nopiv = isinstance(F.ipiv, NotIPIV)
    if not nopiv and not (_is_torch(F.ipiv) and F.ipiv.is_cuda and F.ipiv.dtype == torch.int64):
        raise TypeError("ipiv of a batch must be an int64 CUDA tensor (or NotIPIV)")
    batch, n = int(A.shape[0]), int(A.shape[1])
    if _as_bool(check):
        _check_batched_info(F.info, True)
    X = torch.empty((batch, n, n), dtype=A.dtype, device=A.device)
    if not row_major:
        X = X.transpose(1, 2)
    if batch > 0 and n > 0:
        h = handle or _ffi.default_handle(A.device.index or 0)
        h.set_stream(torch.cuda.current_stream(A.device).cuda_stream)
        stride_ip = 0 if nopiv else (int(F.ipiv.stride(0)) if batch > 1 else max(n, 1))
        info_t = torch.zeros(batch, dtype=torch.int64, device=A.device)
        h.call(f"rflu_getri_batched_{sfx}_dev", batch, n, ctypes.c_void_p(A.data_ptr()), ld, stride_f, row_major,
               ctypes.c_void_p(0 if nopiv else F.ipiv.data_ptr()), stride_ip, ctypes.c_void_p(X.data_ptr()), n, n * n,
               _CBATCHED_TRANS[trans], ctypes.c_void_p(info_t.data_ptr()))
        if _as_bool(check):
            _check_batched_info(info_t, True)
    return X


def opnorm_complex_batched(A, p=1, *, handle=None):
    """``opnorm_complex(A_b, p)`` of every matrix of a complex (batch, m, n) CUDA tensor (``rflu_lange_batched_cf64_dev`` / ``_cf32_dev``;
    one workgroup per matrix up to 128 x 128): a Float64 CUDA tensor of length ``batch``, entry b bit-identical to ``opnorm_complex`` on
    matrix b.  ``Adjoint(A)`` swaps 1 and inf (|conj z| = |z|: no ``trans`` letter is needed)."""
    code = _norm_code(p, "opnorm_complex_batched")
    if isinstance(A, Adjoint):
        A, code = A.parent, _swap_norm(code)
    if not _is_torch(A) or A.ndim != 3:
        raise TypeError("opnorm_complex_batched needs a 3-D CUDA tensor (batch, m, n)")
    sfx = _ccond_sfx(A.dtype, "opnorm_complex_batched")
    if not A.is_cuda:
        raise TypeError("opnorm_complex_batched: the batch must live on the MI355X (device='cuda')")
    import torch

    if A.is_conj():
        A = A.resolve_conj()
    batch, m, n = (int(x) for x in A.shape)
    row_major, ld, stride_a = _batched_layout(A, "opnorm_complex_batched")
    out = torch.zeros(batch, dtype=torch.float64, device=A.device)
    if batch > 0 and m > 0 and n > 0:
        h = handle or _ffi.default_handle(A.device.index or 0)
        h.set_stream(torch.cuda.current_stream(A.device).cuda_stream)
        h.call(f"rflu_lange_batched_{sfx}_dev", code, batch, m, n, ctypes.c_void_p(A.data_ptr()), ld, stride_a, row_major,
               ctypes.c_void_p(out.data_ptr()))
    return out


def rcond_complex_batched(F, anorm, p=1, *, handle=None):
    """``rcond_complex`` of every matrix of the ``BatchedLU`` that ``lu_complex_batched_`` returned (``rflu_gecon_batched_cf64_dev`` /
    ``_cf32_dev``: ONE launch up to n = 64 for ``complex128`` and n = 128 for ``complex64``, the whole estimator inside the kernel on the
    factors held in LDS; larger column-major matrices are looped over ``rflu_gecon_c*``, larger row-major ones are refused).  ``anorm``: a
    Float64 CUDA tensor of length ``batch`` (``opnorm_complex_batched`` before the factorization).  Returns a Float64 CUDA tensor of
    length ``batch``; a singular member gives 0 and a NaN member NaN in its own entry only.  ``Adjoint(F)`` swaps 1 and inf (|conj z| =
    |z|: no ``trans`` letter is needed)."""
    code = _norm_code(p, "rcond_complex_batched")
    G, adj = _unwrap_adjoint(F, "rcond_complex_batched")
    if not isinstance(G, BatchedLU):
        raise TypeError("rcond_complex_batched needs the BatchedLU that lu_complex_batched_ returned")
    A = G.factors
    if not (_is_torch(A) and A.is_cuda) or A.ndim != 3:
        raise TypeError("rcond_complex_batched: the factors must be a 3-D CUDA tensor")
    if A.shape[1] != A.shape[2]:
        raise ValueError("rcond_complex_batched needs square factorizations")
    sfx = _ccond_sfx(A.dtype, "rcond_complex_batched")
    row_major, ld, stride_f = _batched_layout(A, "rcond_complex_batched")
    if adj:
        code = _swap_norm(code)
    import torch

    batch, n = int(A.shape[0]), int(A.shape[1])
    if not (_is_torch(anorm) and anorm.is_cuda and anorm.dtype == torch.float64 and anorm.ndim == 1 and anorm.shape[0] == batch
            and (batch <= 1 or anorm.stride(0) == 1)):
        raise TypeError("rcond_complex_batched: anorm must be a contiguous Float64 CUDA tensor of length batch")
    out = torch.ones(batch, dtype=torch.float64, device=A.device)
    if batch > 0 and n > 0:
        h = handle or _ffi.default_handle(A.device.index or 0)
        h.set_stream(torch.cuda.current_stream(A.device).cuda_stream)
        h.call(f"rflu_gecon_batched_{sfx}_dev", code, batch, n, ctypes.c_void_p(A.data_ptr()), ld, stride_f, row_major,
               ctypes.c_void_p(anorm.data_ptr()), ctypes.c_void_p(out.data_ptr()))
    return out


def cond_complex_batched(A, p=1, *, handle=None):
    """``cond_complex(A_b, p)`` of every matrix of a complex (batch, n, n) CUDA tensor: ``opnorm_complex_batched``, ``lu_complex_batched``
    on a copy (``check=False``), ``1 / rcond_complex_batched``; ``inf`` where ``rcond == 0``.  A Float64 CUDA tensor of length ``batch``.
    ``Adjoint(A)`` swaps 1 and inf (|conj z| = |z|: no ``trans`` letter is needed)."""
    code = _norm_code(p, "cond_complex_batched")
    if isinstance(A, Adjoint):
        A, code = A.parent, _swap_norm(code)
    if not _is_torch(A) or A.ndim != 3 or A.shape[1] != A.shape[2]:
        raise ValueError("cond_complex_batched needs a 3-D CUDA tensor (batch, n, n)")
    _ccond_sfx(A.dtype, "cond_complex_batched")
    import torch

    p = 1 if code == _ffi.NORM_ONE else float("inf")
    anorm = opnorm_complex_batched(A, p, handle=handle)
    rc = rcond_complex_batched(lu_complex_batched(A, check=False, handle=handle), anorm, p, handle=handle)
    return torch.where(rc == 0, torch.full_like(rc, float("inf")), 1.0 / rc)


def last_path(device: int = 0) -> str:
    """Which implementation served the last factorization on ``device`` (``enum rflu_path`` of include/rflu.h: "hip-recursive" /
    "hip-blocked" / "hip-lookahead" / "hip-engine" / "hip-batched" / "none")."""
    return {0: "none", 1: "hip-recursive", 2: "hip-blocked", 3: "hip-lookahead", 4: "hip-engine",
            5: "hip-batched"}[_ffi.default_handle(device).last_path()]
