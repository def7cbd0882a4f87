"""recursivefactorization.jl_amd -- MI355X-native recursive LU behind RecursiveFactorization.jl's ``lu`` / ``lu!`` API.

The product is ``librflu.so`` (hand-written HIP for gfx950, C ABI in ``include/rflu.h``); this package is the thin
host-side mirror of the reference's interface.  No CPU fallback exists: without the built library and a gfx950 device
every call raises.
"""
from ._ffi import Handle, RfluError, default_handle  # noqa: F401
from .lu import (  # noqa: F401
    LU,
    BatchedLU,
    cond,
    cond_batched,
    MixedLU,
    NotConvergedError,
    NOPIVOT_NEGATIVE_INFO,
    Adjoint,
    NoPivot,
    NotIPIV,
    RowMaximum,
    SingularException,
    Transpose,
    Val,
    det,
    det_batched,
    det_complex,
    det_complex_batched,
    inv,
    inv_,
    inv_batched,
    inv_complex,
    inv_complex_,
    inv_complex_batched,
    last_path,
    ldiv_,
    ldiv_batched_,
    ldiv_complex_,
    ldiv_complex_adjoint_,
    ldiv_complex_batched_,
    ldiv_complex_mixed,
    ldiv_complex_transpose_,
    ldiv_mixed,
    logabsdet,
    logabsdet_batched,
    logabsdet_complex,
    logabsdet_complex_batched,
    logdet,
    logdet_complex,
    lu,
    lu_,
    lu_batched,
    lu_batched_,
    lu_complex,
    lu_complex_,
    lu_complex_batched,
    lu_complex_batched_,
    lu_complex_mixed,
    lu_mixed,
    normalize_pivot,
    opnorm,
    opnorm_batched,
    rcond,
    rcond_batched,
)

from .butterfly import (  # noqa: F401,E402
    ButterflyWorkspace,
    butterfly_mul_,
    butterfly_solve_,
    butterfly_workspace,
)

from . import linsolve  # noqa: F401,E402  (LinearSolve.jl's RFLUFactorization cache protocol)

__all__ = [
    "linsolve",
    "ButterflyWorkspace", "butterfly_workspace", "butterfly_solve_", "butterfly_mul_",
    "lu", "lu_", "ldiv_", "LU", "lu_batched", "lu_batched_", "ldiv_batched_", "BatchedLU", "lu_mixed", "ldiv_mixed", "MixedLU", "NotConvergedError", "NotIPIV", "RowMaximum", "NoPivot", "Val", "Adjoint", "Transpose", "SingularException",
    "lu_complex", "lu_complex_", "ldiv_complex_", "ldiv_complex_adjoint_", "ldiv_complex_transpose_",
    "lu_complex_batched", "lu_complex_batched_", "ldiv_complex_batched_", "lu_complex_mixed", "ldiv_complex_mixed",
    "inv", "inv_", "det", "logabsdet", "logdet", "inv_batched", "logabsdet_batched", "det_batched",
    "inv_complex", "inv_complex_", "det_complex", "logabsdet_complex", "logdet_complex", "logabsdet_complex_batched", "det_complex_batched",
    "inv_complex_batched",
    "opnorm", "rcond", "cond", "opnorm_batched", "rcond_batched", "cond_batched",
    "normalize_pivot", "last_path", "Handle", "RfluError", "default_handle", "NOPIVOT_NEGATIVE_INFO",
]
