"""
    RFLUAMD

Julia host glue for `librflu.so`, the MI355X (gfx950) implementation of RecursiveFactorization.jl's `lu!` hot path
(`lu!` -> `recurse!` -> `reckernel!`, RecursiveFactorization `src/lu.jl:97-338`).  The C ABI is `include/rflu.h`; every
`ccall` below is checked mechanically against that header by `tests/test_julia_glue.py` (arity and argument types), because
Julia is not available in the image this repository is built in.

Surface (the reference's own, `src/lu.jl:19-21, 67-83, 97-130`):

    RFLUAMD.lu(A, pivot = Val(true), thread = Val(false); check, blocksize, threshold)
    RFLUAMD.lu!(A, pivot = Val(true), thread = Val(false); check, blocksize, threshold)
    RFLUAMD.lu!(A, ipiv, pivot = Val(true), thread = Val(false); check, blocksize, threshold)   # what RFLUFactorization calls

returning a genuine `LinearAlgebra.LU(A, ipiv, info)` that aliases the caller's arrays.  `Float64` / `Float32` strided
column-major matrices with at least `GPU_MIN_N[]` columns go to the GPU (so do `ComplexF64` / `ComplexF32` ones, for `lu!`, `ldiv!(F, B)`, `ldiv!(F', B)` and `ldiv!(transpose(F), B)`); everything else (other element types, non-strided
storage, small sizes, no device) goes to `RecursiveFactorization.lu!` when that package is loaded, else to
`LinearAlgebra.lu!`/`generic_lufact!` -- the same fall-back rules the reference applies (`src/lu.jl:74-77, 92-93, 114-126`).
"""
module RFLUAMD

using LinearAlgebra
using LinearAlgebra: BlasInt, LU, RowMaximum, NoPivot, checknonsingular
using Libdl

export RFLUAMDFactorization, RF32MixedLUAMDFactorization

const librflu = get(ENV, "RFLU_LIB", "librflu.so")
const HANDLE = Ref{Ptr{Cvoid}}(C_NULL)
const HANDLE_LOCK = ReentrantLock()
"below this many columns the CPU recursion wins (PCIe staging + launch latency); `ENV[\"RFLU_MIN_N\"]` overrides"
const GPU_MIN_N = Ref{Int}(parse(Int, get(ENV, "RFLU_MIN_N", "1024")))
"Julia >= 1.11 reports NoPivot failures with a negative info (RecursiveFactorization src/lu.jl:25)"
const NOPIVOT_NEGATIVE_INFO = VERSION >= v"1.11.0-DEV"   # as src/lu.jl:25

# rflu_status (include/rflu.h)
const RFLU_OK = Cint(0)

last_error() = unsafe_string(ccall((:rflu_last_error, librflu), Cstring, ()))

function handle()
    lock(HANDLE_LOCK) do
        if HANDLE[] == C_NULL
            st = ccall((:rflu_create, librflu), Cint, (Ref{Ptr{Cvoid}}, Cint), HANDLE, Cint(0))
            st == RFLU_OK || error("rflu_create failed: ", last_error())
            atexit() do
                ccall((:rflu_destroy, librflu), Cint, (Ptr{Cvoid},), HANDLE[])
                HANDLE[] = C_NULL
            end
        end
        HANDLE[]
    end
end

"`true` when librflu.so loads and finds a gfx950 device (no CPU fallback lives inside the library)"
function available()
    Libdl.dlopen(librflu; throw_error = false) === nothing && return false
    try
        return handle() != C_NULL
    catch
        return false
    end
end

"which implementation served the last factorization: 1 recursive, 2 blocked (profiling), 3 lookahead, 4 engine, 5 batched (rflu_path)"
last_path() = Int(ccall((:rflu_last_path, librflu), Cint, (Ptr{Cvoid},), handle()))

normalize_pivot(t::Val{T}) where {T} = t                     # RecursiveFactorization src/lu.jl:10-17
normalize_pivot(::RowMaximum) = Val(true)
normalize_pivot(::NoPivot) = Val(false)

"zero-storage identity pivots for NoPivot (RecursiveFactorization src/lu.jl:27-40); the C ABI takes NULL for it"
struct NotIPIV <: AbstractVector{BlasInt}
    len::Int
end
Base.size(A::NotIPIV) = (A.len,)
Base.getindex(::NotIPIV, i::Int) = i
Base.view(::NotIPIV, r::AbstractUnitRange) = NotIPIV(length(r))
init_pivot(::Val{false}, minmn) = NotIPIV(minmn)
init_pivot(::Val{true}, minmn) = Vector{BlasInt}(undef, minmn)

# ---- the C ABI, one method per element type (literal ccall tuples: tests/test_julia_glue.py parses them) ------------------
function getrf!(A::StridedMatrix{Float64}, ipiv::Ptr{Int64}, pivot::Bool, blocksize::Integer)
    m, n = size(A)
    info = Ref{Int64}(0)
    st = ccall((:rflu_getrf_f64, librflu), Cint,
               (Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Int64, Ptr{Int64}, Cint, Int64, Ref{Int64}),
               handle(), m, n, A, stride(A, 2), ipiv, Cint(pivot), blocksize, info)
    st == RFLU_OK || error("librflu: ", last_error())
    return BlasInt(info[])
end

function getrf!(A::StridedMatrix{Float32}, ipiv::Ptr{Int64}, pivot::Bool, blocksize::Integer)
    m, n = size(A)
    info = Ref{Int64}(0)
    st = ccall((:rflu_getrf_f32, librflu), Cint,
               (Ptr{Cvoid}, Int64, Int64, Ptr{Float32}, Int64, Ptr{Int64}, Cint, Int64, Ref{Int64}),
               handle(), m, n, A, stride(A, 2), ipiv, Cint(pivot), blocksize, info)
    st == RFLU_OK || error("librflu: ", last_error())
    return BlasInt(info[])
end

"device-resident variant for a matrix that already lives in HBM (e.g. the buffer of an AMDGPU.jl ROCArray)"
function getrf_dev!(A::Ptr{Float64}, m::Integer, n::Integer, lda::Integer, ipiv::Ptr{Int64}, pivot::Bool, blocksize::Integer)
    info = Ref{Int64}(0)
    st = ccall((:rflu_getrf_f64_dev, librflu), Cint,
               (Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Int64, Ptr{Int64}, Cint, Int64, Ref{Int64}),
               handle(), m, n, A, lda, ipiv, Cint(pivot), blocksize, info)
    st == RFLU_OK || error("librflu: ", last_error())
    return BlasInt(info[])
end

function getrf_dev!(A::Ptr{Float32}, m::Integer, n::Integer, lda::Integer, ipiv::Ptr{Int64}, pivot::Bool, blocksize::Integer)
    info = Ref{Int64}(0)
    st = ccall((:rflu_getrf_f32_dev, librflu), Cint,
               (Ptr{Cvoid}, Int64, Int64, Ptr{Float32}, Int64, Ptr{Int64}, Cint, Int64, Ref{Int64}),
               handle(), m, n, A, lda, ipiv, Cint(pivot), blocksize, info)
    st == RFLU_OK || error("librflu: ", last_error())
    return BlasInt(info[])
end

"""
    getrf_batched_dev!(A, batch, m, n, lda, strideA, row_major, ipiv, stride_ipiv, pivot, info)

`batch` independent `m x n` matrices that live in HBM, factored in one call (`rflu_getrf_batched_*_dev`, include/rflu.h): matrix `b`
starts `b*strideA` elements after `A`, its pivots `b*stride_ipiv` entries after `ipiv` (`C_NULL` with `pivot = false` plays NotIPIV);
`info` is a DEVICE pointer to `batch` entries (0 or the first zero pivot, positive convention -- the caller applies
`NOPIVOT_NEGATIVE_INFO` and `checknonsingular`).  Up to 128 rows and columns one kernel launch serves the whole batch.
"""
function getrf_batched_dev!(A::Ptr{Float64}, batch::Integer, m::Integer, n::Integer, lda::Integer, strideA::Integer, row_major::Bool,
                            ipiv::Ptr{Int64}, stride_ipiv::Integer, pivot::Bool, info::Ptr{Int64})
    st = ccall((:rflu_getrf_batched_f64_dev, librflu), Cint,
               (Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Float64}, Int64, Int64, Cint, Ptr{Int64}, Int64, Cint, Ptr{Int64}),
               handle(), batch, m, n, A, lda, strideA, Cint(row_major), ipiv, stride_ipiv, Cint(pivot), info)
    st == RFLU_OK || error("librflu: ", last_error())
    return nothing
end

function getrf_batched_dev!(A::Ptr{Float32}, batch::Integer, m::Integer, n::Integer, lda::Integer, strideA::Integer, row_major::Bool,
                            ipiv::Ptr{Int64}, stride_ipiv::Integer, pivot::Bool, info::Ptr{Int64})
    st = ccall((:rflu_getrf_batched_f32_dev, librflu), Cint,
               (Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Float32}, Int64, Int64, Cint, Ptr{Int64}, Int64, Cint, Ptr{Int64}),
               handle(), batch, m, n, A, lda, strideA, Cint(row_major), ipiv, stride_ipiv, Cint(pivot), info)
    st == RFLU_OK || error("librflu: ", last_error())
    return nothing
end

"""
    getrs_batched_dev!(F, batch, n, nrhs, lda, strideF, row_major, ipiv, stride_ipiv, B, ldb, strideB, trans)

The solve that follows `getrf_batched_dev!`: `B` (`n x nrhs` per matrix, in the orientation of `F`, device memory) is overwritten with
`A \\ B`, or with `A' \\ B` when `trans` is set.  A singular matrix leaves Inf/NaN in its own right-hand sides only.
"""
function getrs_batched_dev!(F::Ptr{Float64}, batch::Integer, n::Integer, nrhs::Integer, lda::Integer, strideF::Integer, row_major::Bool,
                            ipiv::Ptr{Int64}, stride_ipiv::Integer, B::Ptr{Float64}, ldb::Integer, strideB::Integer, trans::Bool)
    st = ccall((:rflu_getrs_batched_f64_dev, librflu), Cint,
               (Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Float64}, Int64, Int64, Cint, Ptr{Int64}, Int64, Ptr{Float64}, Int64, Int64, Cint),
               handle(), batch, n, nrhs, F, lda, strideF, Cint(row_major), ipiv, stride_ipiv, B, ldb, strideB, Cint(trans))
    st == RFLU_OK || error("librflu: ", last_error())
    return B
end

function getrs_batched_dev!(F::Ptr{Float32}, batch::Integer, n::Integer, nrhs::Integer, lda::Integer, strideF::Integer, row_major::Bool,
                            ipiv::Ptr{Int64}, stride_ipiv::Integer, B::Ptr{Float32}, ldb::Integer, strideB::Integer, trans::Bool)
    st = ccall((:rflu_getrs_batched_f32_dev, librflu), Cint,
               (Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Float32}, Int64, Int64, Cint, Ptr{Int64}, Int64, Ptr{Float32}, Int64, Int64, Cint),
               handle(), batch, n, nrhs, F, lda, strideF, Cint(row_major), ipiv, stride_ipiv, B, ldb, strideB, Cint(trans))
    st == RFLU_OK || error("librflu: ", last_error())
    return B
end

# The complex batches (`rflu_get{rf,rs}_batched_cf64_dev` / `_cf32_dev`, include/rflu.h): the same argument lists, pointers to
# `ComplexF64` / `ComplexF32` device memory `reinterpret`ed to the real type, `lda` / `ldb` and every stride in COMPLEX elements.  One
# launch up to 64 (`ComplexF64`) / 128 (`ComplexF32`) rows and columns; larger column-major batches are looped, larger row-major ones
# are an error.  The solve takes `trans` as LAPACK's letter: 'N' (A), 'T' (transpose(A)) or 'C' (A'), which differ for these elements.
function getrf_batched_dev!(A::Ptr{ComplexF64}, batch::Integer, m::Integer, n::Integer, lda::Integer, strideA::Integer, row_major::Bool,
                            ipiv::Ptr{Int64}, stride_ipiv::Integer, pivot::Bool, info::Ptr{Int64})
    st = ccall((:rflu_getrf_batched_cf64_dev, librflu), Cint,
               (Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Float64}, Int64, Int64, Cint, Ptr{Int64}, Int64, Cint, Ptr{Int64}),
               handle(), batch, m, n, reinterpret(Ptr{Float64}, A), lda, strideA, Cint(row_major), ipiv, stride_ipiv, Cint(pivot), info)
    st == RFLU_OK || error("librflu: ", last_error())
    return nothing
end

function getrf_batched_dev!(A::Ptr{ComplexF32}, batch::Integer, m::Integer, n::Integer, lda::Integer, strideA::Integer, row_major::Bool,
                            ipiv::Ptr{Int64}, stride_ipiv::Integer, pivot::Bool, info::Ptr{Int64})
    st = ccall((:rflu_getrf_batched_cf32_dev, librflu), Cint,
               (Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Float32}, Int64, Int64, Cint, Ptr{Int64}, Int64, Cint, Ptr{Int64}),
               handle(), batch, m, n, reinterpret(Ptr{Float32}, A), lda, strideA, Cint(row_major), ipiv, stride_ipiv, Cint(pivot), info)
    st == RFLU_OK || error("librflu: ", last_error())
    return nothing
end

function batched_trans_code(trans::AbstractChar)
    trans == 'N' && return Cint(0)
    trans == 'T' && return Cint(1)
    trans == 'C' && return Cint(2)
    throw(ArgumentError("trans must be 'N', 'T' or 'C'"))
end

function getrs_batched_dev!(F::Ptr{ComplexF64}, batch::Integer, n::Integer, nrhs::Integer, lda::Integer, strideF::Integer, row_major::Bool,
                            ipiv::Ptr{Int64}, stride_ipiv::Integer, B::Ptr{ComplexF64}, ldb::Integer, strideB::Integer, trans::AbstractChar)
    st = ccall((:rflu_getrs_batched_cf64_dev, librflu), Cint,
               (Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Float64}, Int64, Int64, Cint, Ptr{Int64}, Int64, Ptr{Float64}, Int64, Int64, Cint),
               handle(), batch, n, nrhs, reinterpret(Ptr{Float64}, F), lda, strideF, Cint(row_major), ipiv, stride_ipiv, reinterpret(Ptr{Float64}, B), ldb, strideB, batched_trans_code(trans))
    st == RFLU_OK || error("librflu: ", last_error())
    return B
end

function getrs_batched_dev!(F::Ptr{ComplexF32}, batch::Integer, n::Integer, nrhs::Integer, lda::Integer, strideF::Integer, row_major::Bool,
                            ipiv::Ptr{Int64}, stride_ipiv::Integer, B::Ptr{ComplexF32}, ldb::Integer, strideB::Integer, trans::AbstractChar)
    st = ccall((:rflu_getrs_batched_cf32_dev, librflu), Cint,
               (Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Float32}, Int64, Int64, Cint, Ptr{Int64}, Int64, Ptr{Float32}, Int64, Int64, Cint),
               handle(), batch, n, nrhs, reinterpret(Ptr{Float32}, F), lda, strideF, Cint(row_major), ipiv, stride_ipiv, reinterpret(Ptr{Float32}, B), ldb, strideB, batched_trans_code(trans))
    st == RFLU_OK || error("librflu: ", last_error())
    return B
end

"`ldiv!(F, B)` on the GPU: B <- U^-1 L^-1 P B (stdlib `ldiv!(::LU, B)`; the package's own for NotIPIV, src/lu.jl:60-64)"
function getrs!(F::StridedMatrix{Float64}, ipiv::Ptr{Int64}, B::StridedVecOrMat{Float64})
    n = size(F, 1)
    st = ccall((:rflu_getrs_f64, librflu), Cint,
               (Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Int64, Ptr{Int64}, Ptr{Float64}, Int64),
               handle(), n, size(B, 2), F, stride(F, 2), ipiv, B, B isa AbstractVector ? n : stride(B, 2))
    st == RFLU_OK || error("librflu: ", last_error())
    return B
end

function getrs!(F::StridedMatrix{Float32}, ipiv::Ptr{Int64}, B::StridedVecOrMat{Float32})
    n = size(F, 1)
    st = ccall((:rflu_getrs_f32, librflu), Cint,
               (Ptr{Cvoid}, Int64, Int64, Ptr{Float32}, Int64, Ptr{Int64}, Ptr{Float32}, Int64),
               handle(), n, size(B, 2), F, stride(F, 2), ipiv, B, B isa AbstractVector ? n : stride(B, 2))
    st == RFLU_OK || error("librflu: ", last_error())
    return B
end

# ---- ComplexF64 / ComplexF32 (rflu_get{rf,rs}_cf64 / _cf32, include/rflu.h): the same interleaved storage as Julia's Complex{T}, so the
# pointers are `reinterpret`ed to the real type and every leading dimension stays in complex elements.  No blocksize: one schedule.
function getrf!(A::StridedMatrix{ComplexF64}, ipiv::Ptr{Int64}, pivot::Bool, blocksize::Integer)
    m, n = size(A)
    info = Ref{Int64}(0)
    st = ccall((:rflu_getrf_cf64, librflu), Cint,
               (Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Int64, Ptr{Int64}, Cint, Ref{Int64}),
               handle(), m, n, reinterpret(Ptr{Float64}, pointer(A)), stride(A, 2), ipiv, Cint(pivot), info)
    st == RFLU_OK || error("librflu: ", last_error())
    return BlasInt(info[])
end

function getrf!(A::StridedMatrix{ComplexF32}, ipiv::Ptr{Int64}, pivot::Bool, blocksize::Integer)
    m, n = size(A)
    info = Ref{Int64}(0)
    st = ccall((:rflu_getrf_cf32, librflu), Cint,
               (Ptr{Cvoid}, Int64, Int64, Ptr{Float32}, Int64, Ptr{Int64}, Cint, Ref{Int64}),
               handle(), m, n, reinterpret(Ptr{Float32}, pointer(A)), stride(A, 2), ipiv, Cint(pivot), info)
    st == RFLU_OK || error("librflu: ", last_error())
    return BlasInt(info[])
end

"device-resident complex variant: `A` points at interleaved (re, im) pairs in HBM, `lda` in complex elements"
function getrf_complex_dev!(A::Ptr{Float64}, m::Integer, n::Integer, lda::Integer, ipiv::Ptr{Int64}, pivot::Bool)
    info = Ref{Int64}(0)
    st = ccall((:rflu_getrf_cf64_dev, librflu), Cint,
               (Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Int64, Ptr{Int64}, Cint, Ref{Int64}),
               handle(), m, n, A, lda, ipiv, Cint(pivot), info)
    st == RFLU_OK || error("librflu: ", last_error())
    return BlasInt(info[])
end

function getrf_complex_dev!(A::Ptr{Float32}, m::Integer, n::Integer, lda::Integer, ipiv::Ptr{Int64}, pivot::Bool)
    info = Ref{Int64}(0)
    st = ccall((:rflu_getrf_cf32_dev, librflu), Cint,
               (Ptr{Cvoid}, Int64, Int64, Ptr{Float32}, Int64, Ptr{Int64}, Cint, Ref{Int64}),
               handle(), m, n, A, lda, ipiv, Cint(pivot), info)
    st == RFLU_OK || error("librflu: ", last_error())
    return BlasInt(info[])
end

"`ldiv!(F, B)` for complex factors on the GPU (`ldiv!(F', B)` and `ldiv!(transpose(F), B)` are served by `getrs_ctrans!` below)"
function getrs!(F::StridedMatrix{ComplexF64}, ipiv::Ptr{Int64}, B::StridedVecOrMat{ComplexF64})
    n = size(F, 1)
    st = ccall((:rflu_getrs_cf64, librflu), Cint,
               (Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Int64, Ptr{Int64}, Ptr{Float64}, Int64),
               handle(), n, size(B, 2), reinterpret(Ptr{Float64}, pointer(F)), stride(F, 2), ipiv, reinterpret(Ptr{Float64}, pointer(B)), B isa AbstractVector ? n : stride(B, 2))
    st == RFLU_OK || error("librflu: ", last_error())
    return B
end

function getrs!(F::StridedMatrix{ComplexF32}, ipiv::Ptr{Int64}, B::StridedVecOrMat{ComplexF32})
    n = size(F, 1)
    st = ccall((:rflu_getrs_cf32, librflu), Cint,
               (Ptr{Cvoid}, Int64, Int64, Ptr{Float32}, Int64, Ptr{Int64}, Ptr{Float32}, Int64),
               handle(), n, size(B, 2), reinterpret(Ptr{Float32}, pointer(F)), stride(F, 2), ipiv, reinterpret(Ptr{Float32}, pointer(B)), B isa AbstractVector ? n : stride(B, 2))
    st == RFLU_OK || error("librflu: ", last_error())
    return B
end

function getrs_complex_dev!(F::Ptr{Float64}, n::Integer, nrhs::Integer, lda::Integer, ipiv::Ptr{Int64}, B::Ptr{Float64}, ldb::Integer)
    st = ccall((:rflu_getrs_cf64_dev, librflu), Cint,
               (Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Int64, Ptr{Int64}, Ptr{Float64}, Int64),
               handle(), n, nrhs, F, lda, ipiv, B, ldb)
    st == RFLU_OK || error("librflu: ", last_error())
    return B
end

function getrs_complex_dev!(F::Ptr{Float32}, n::Integer, nrhs::Integer, lda::Integer, ipiv::Ptr{Int64}, B::Ptr{Float32}, ldb::Integer)
    st = ccall((:rflu_getrs_cf32_dev, librflu), Cint,
               (Ptr{Cvoid}, Int64, Int64, Ptr{Float32}, Int64, Ptr{Int64}, Ptr{Float32}, Int64),
               handle(), n, nrhs, F, lda, ipiv, B, ldb)
    st == RFLU_OK || error("librflu: ", last_error())
    return B
end

"`ldiv!(F', B)` / `ldiv!(transpose(F), B)` on the GPU: B <- P^T L^-T U^-T B (LAPACK getrs with trans = 'T'; real types, so one routine)"
function getrs_trans!(F::StridedMatrix{Float64}, ipiv::Ptr{Int64}, B::StridedVecOrMat{Float64})
    n = size(F, 1)
    st = ccall((:rflu_getrs_trans_f64, librflu), Cint,
               (Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Int64, Ptr{Int64}, Ptr{Float64}, Int64),
               handle(), n, size(B, 2), F, stride(F, 2), ipiv, B, B isa AbstractVector ? n : stride(B, 2))
    st == RFLU_OK || error("librflu: ", last_error())
    return B
end

function getrs_trans!(F::StridedMatrix{Float32}, ipiv::Ptr{Int64}, B::StridedVecOrMat{Float32})
    n = size(F, 1)
    st = ccall((:rflu_getrs_trans_f32, librflu), Cint,
               (Ptr{Cvoid}, Int64, Int64, Ptr{Float32}, Int64, Ptr{Int64}, Ptr{Float32}, Int64),
               handle(), n, size(B, 2), F, stride(F, 2), ipiv, B, B isa AbstractVector ? n : stride(B, 2))
    st == RFLU_OK || error("librflu: ", last_error())
    return B
end

"""
    getrs_ctrans!(F, ipiv, B, conj)

The transposed solves for complex factors on the GPU (`rflu_getrs_trans_cf64` / `_cf32`), which differ for these element types:
`conj = false` is `ldiv!(transpose(F), B)` (B <- P^T L^-T U^-T B, LAPACK 'T'), `conj = true` is `ldiv!(F', B)` (B <- P^T L^-H U^-H B,
LAPACK 'C').  The factors are only read, in place.
"""
function getrs_ctrans!(F::StridedMatrix{ComplexF64}, ipiv::Ptr{Int64}, B::StridedVecOrMat{ComplexF64}, conj::Bool)
    n = size(F, 1)
    st = ccall((:rflu_getrs_trans_cf64, librflu), Cint,
               (Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Int64, Ptr{Int64}, Ptr{Float64}, Int64, Cint),
               handle(), n, size(B, 2), reinterpret(Ptr{Float64}, pointer(F)), stride(F, 2), ipiv, reinterpret(Ptr{Float64}, pointer(B)), B isa AbstractVector ? n : stride(B, 2), Cint(conj))
    st == RFLU_OK || error("librflu: ", last_error())
    return B
end

function getrs_ctrans!(F::StridedMatrix{ComplexF32}, ipiv::Ptr{Int64}, B::StridedVecOrMat{ComplexF32}, conj::Bool)
    n = size(F, 1)
    st = ccall((:rflu_getrs_trans_cf32, librflu), Cint,
               (Ptr{Cvoid}, Int64, Int64, Ptr{Float32}, Int64, Ptr{Int64}, Ptr{Float32}, Int64, Cint),
               handle(), n, size(B, 2), reinterpret(Ptr{Float32}, pointer(F)), stride(F, 2), ipiv, reinterpret(Ptr{Float32}, pointer(B)), B isa AbstractVector ? n : stride(B, 2), Cint(conj))
    st == RFLU_OK || error("librflu: ", last_error())
    return B
end

"""
    getri!(F, ipiv) -> info

LAPACK getri on HOST factors (`rflu_getri_*`, include/rflu.h): the packed `L\\U` in `F` (column-major, as `getrf!` left it) is
overwritten by `inv(A)`; about 4n^3/3 flops and no n x n workspace on the device.  Returns 0, or the index of the first exactly
zero `u_ii` -- `F` is then untouched.  `ipiv = C_NULL` plays NotIPIV.
"""
function getri!(F::StridedMatrix{Float64}, ipiv::Ptr{Int64})
    info = Ref{Int64}(0)
    st = ccall((:rflu_getri_f64, librflu), Cint,
               (Ptr{Cvoid}, Int64, Ptr{Float64}, Int64, Ptr{Int64}, Ref{Int64}),
               handle(), size(F, 1), F, stride(F, 2), ipiv, info)
    st == RFLU_OK || error("librflu: ", last_error())
    return info[]
end

function getri!(F::StridedMatrix{Float32}, ipiv::Ptr{Int64})
    info = Ref{Int64}(0)
    st = ccall((:rflu_getri_f32, librflu), Cint,
               (Ptr{Cvoid}, Int64, Ptr{Float32}, Int64, Ptr{Int64}, Ref{Int64}),
               handle(), size(F, 1), F, stride(F, 2), ipiv, info)
    st == RFLU_OK || error("librflu: ", last_error())
    return info[]
end

"""
    getri_dev!(F, n, ld, ipiv; row_major = false) -> info

The same on factors that live in HBM: column-major (`rflu_getri_*_dev`, in place, no layout change) or row-major
(`rflu_getri_rm_*_dev`, one layout change each way through the handle's workspace).
"""
function getri_dev!(F::Ptr{Float64}, n::Integer, ld::Integer, ipiv::Ptr{Int64}; row_major::Bool = false)
    info = Ref{Int64}(0)
    st = row_major ?
         ccall((:rflu_getri_rm_f64_dev, librflu), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}, Int64, Ptr{Int64}, Ref{Int64}),
               handle(), n, F, ld, ipiv, info) :
         ccall((:rflu_getri_f64_dev, librflu), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}, Int64, Ptr{Int64}, Ref{Int64}),
               handle(), n, F, ld, ipiv, info)
    st == RFLU_OK || error("librflu: ", last_error())
    return info[]
end

function getri_dev!(F::Ptr{Float32}, n::Integer, ld::Integer, ipiv::Ptr{Int64}; row_major::Bool = false)
    info = Ref{Int64}(0)
    st = row_major ?
         ccall((:rflu_getri_rm_f32_dev, librflu), Cint, (Ptr{Cvoid}, Int64, Ptr{Float32}, Int64, Ptr{Int64}, Ref{Int64}),
               handle(), n, F, ld, ipiv, info) :
         ccall((:rflu_getri_f32_dev, librflu), Cint, (Ptr{Cvoid}, Int64, Ptr{Float32}, Int64, Ptr{Int64}, Ref{Int64}),
               handle(), n, F, ld, ipiv, info)
    st == RFLU_OK || error("librflu: ", last_error())
    return info[]
end

"""
    logabsdet_dev(F, n, ld, ipiv) -> (logabs, sign)
    logabsdet_host(F, ipiv) -> (logabs, sign)

`logabsdet(::LU)` from the diagonal of the factors and the parity of `ipiv` (`rflu_logabsdet_*`): Float64 arithmetic for both element
types, bit-identical from run to run.  The diagonal is at `F[i*(ld+1)]` in both layouts.  The host form copies the diagonal and
`ipiv` only.
"""
function logabsdet_dev(F::Ptr{Float64}, n::Integer, ld::Integer, ipiv::Ptr{Int64})
    out = zeros(Float64, 2)
    st = GC.@preserve out ccall((:rflu_logabsdet_f64_dev, librflu), Cint,
               (Ptr{Cvoid}, Int64, Ptr{Float64}, Int64, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}),
               handle(), n, F, ld, ipiv, pointer(out, 1), pointer(out, 2))
    st == RFLU_OK || error("librflu: ", last_error())
    return out[1], out[2]
end

function logabsdet_dev(F::Ptr{Float32}, n::Integer, ld::Integer, ipiv::Ptr{Int64})
    out = zeros(Float64, 2)
    st = GC.@preserve out ccall((:rflu_logabsdet_f32_dev, librflu), Cint,
               (Ptr{Cvoid}, Int64, Ptr{Float32}, Int64, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}),
               handle(), n, F, ld, ipiv, pointer(out, 1), pointer(out, 2))
    st == RFLU_OK || error("librflu: ", last_error())
    return out[1], out[2]
end

function logabsdet_host(F::StridedMatrix{Float64}, ipiv::Ptr{Int64})
    out = zeros(Float64, 2)
    st = GC.@preserve out ccall((:rflu_logabsdet_f64, librflu), Cint,
               (Ptr{Cvoid}, Int64, Ptr{Float64}, Int64, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}),
               handle(), size(F, 1), F, stride(F, 2), ipiv, pointer(out, 1), pointer(out, 2))
    st == RFLU_OK || error("librflu: ", last_error())
    return out[1], out[2]
end

function logabsdet_host(F::StridedMatrix{Float32}, ipiv::Ptr{Int64})
    out = zeros(Float64, 2)
    st = GC.@preserve out ccall((:rflu_logabsdet_f32, librflu), Cint,
               (Ptr{Cvoid}, Int64, Ptr{Float32}, Int64, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}),
               handle(), size(F, 1), F, stride(F, 2), ipiv, pointer(out, 1), pointer(out, 2))
    st == RFLU_OK || error("librflu: ", last_error())
    return out[1], out[2]
end

"""
    getri_batched_dev!(Ainv, ldi, strideI, F, batch, n, lda, strideF, row_major, ipiv, stride_ipiv, info)
    logabsdet_batched_dev!(logabs, sign, F, batch, n, lda, strideF, ipiv, stride_ipiv)

The batched forms on device memory (`rflu_getri_batched_*_dev`, `rflu_logabsdet_batched_*_dev`): `Ainv` out of place in the orientation
of `F`, `info` a DEVICE pointer to `batch` entries; `logabs` / `sign` DEVICE pointers to `batch` Float64 values.
"""
function getri_batched_dev!(Ainv::Ptr{Float64}, ldi::Integer, strideI::Integer, F::Ptr{Float64}, batch::Integer, n::Integer, lda::Integer,
                            strideF::Integer, row_major::Bool, ipiv::Ptr{Int64}, stride_ipiv::Integer, info::Ptr{Int64})
    st = ccall((:rflu_getri_batched_f64_dev, librflu), Cint,
               (Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Int64, Int64, Cint, Ptr{Int64}, Int64, Ptr{Float64}, Int64, Int64, Ptr{Int64}),
               handle(), batch, n, F, lda, strideF, Cint(row_major), ipiv, stride_ipiv, Ainv, ldi, strideI, info)
    st == RFLU_OK || error("librflu: ", last_error())
    return Ainv
end

function getri_batched_dev!(Ainv::Ptr{Float32}, ldi::Integer, strideI::Integer, F::Ptr{Float32}, batch::Integer, n::Integer, lda::Integer,
                            strideF::Integer, row_major::Bool, ipiv::Ptr{Int64}, stride_ipiv::Integer, info::Ptr{Int64})
    st = ccall((:rflu_getri_batched_f32_dev, librflu), Cint,
               (Ptr{Cvoid}, Int64, Int64, Ptr{Float32}, Int64, Int64, Cint, Ptr{Int64}, Int64, Ptr{Float32}, Int64, Int64, Ptr{Int64}),
               handle(), batch, n, F, lda, strideF, Cint(row_major), ipiv, stride_ipiv, Ainv, ldi, strideI, info)
    st == RFLU_OK || error("librflu: ", last_error())
    return Ainv
end

function logabsdet_batched_dev!(logabs::Ptr{Float64}, sign::Ptr{Float64}, F::Ptr{Float64}, batch::Integer, n::Integer, lda::Integer,
                                strideF::Integer, ipiv::Ptr{Int64}, stride_ipiv::Integer)
    st = ccall((:rflu_logabsdet_batched_f64_dev, librflu), Cint,
               (Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Int64, Int64, Ptr{Int64}, Int64, Ptr{Float64}, Ptr{Float64}),
               handle(), batch, n, F, lda, strideF, ipiv, stride_ipiv, logabs, sign)
    st == RFLU_OK || error("librflu: ", last_error())
    return nothing
end

function logabsdet_batched_dev!(logabs::Ptr{Float64}, sign::Ptr{Float64}, F::Ptr{Float32}, batch::Integer, n::Integer, lda::Integer,
                                strideF::Integer, ipiv::Ptr{Int64}, stride_ipiv::Integer)
    st = ccall((:rflu_logabsdet_batched_f32_dev, librflu), Cint,
               (Ptr{Cvoid}, Int64, Int64, Ptr{Float32}, Int64, Int64, Ptr{Int64}, Int64, Ptr{Float64}, Ptr{Float64}),
               handle(), batch, n, F, lda, strideF, ipiv, stride_ipiv, logabs, sign)
    st == RFLU_OK || error("librflu: ", last_error())
    return nothing
end

# `p` of the norm entries as the C enum rflu_norm
function norm_code(p::Real)
    p == 1 && return Cint(1)
    p == Inf && return Cint(2)
    throw(ArgumentError("p must be 1 or Inf, got $p"))
end

"""
    lange_dev(A, m, n, lda; p = 1, row_major = false) -> Float64
    gecon_dev!(F, n, ld, anorm; p = 1, row_major = false) -> Float64
    gecon_host(F, anorm; p = 1) -> Float64
    gecon_batched_dev!(rcond, F, batch, n, lda, strideF, row_major, anorm; p = 1)

Operator norm and reciprocal condition number on device memory (`rflu_lange_*_dev`, `rflu_gecon_*`): `p` is `1` or `Inf`; `anorm` is the
norm of `A` in the same `p`, taken BEFORE the factorization.  Float64 sums in a fixed order for both element types.  The estimator is
Higham's (LAPACK `gecon`) with an all-ones start vector and an integer closing vector (include/rflu.h); the factors are only read.
The batched form takes DEVICE pointers to `batch` Float64 values for `anorm` and `rcond`.
"""
function lange_dev(A::Ptr{Float64}, m::Integer, n::Integer, lda::Integer; p::Real = 1, row_major::Bool = false)
    out = zeros(Float64, 1)
    st = GC.@preserve out ccall((:rflu_lange_f64_dev, librflu), Cint,
               (Ptr{Cvoid}, Cint, Int64, Int64, Ptr{Float64}, Int64, Cint, Ptr{Float64}),
               handle(), norm_code(p), m, n, A, lda, Cint(row_major), pointer(out, 1))
    st == RFLU_OK || error("librflu: ", last_error())
    return out[1]
end

function lange_dev(A::Ptr{Float32}, m::Integer, n::Integer, lda::Integer; p::Real = 1, row_major::Bool = false)
    out = zeros(Float64, 1)
    st = GC.@preserve out ccall((:rflu_lange_f32_dev, librflu), Cint,
               (Ptr{Cvoid}, Cint, Int64, Int64, Ptr{Float32}, Int64, Cint, Ptr{Float64}),
               handle(), norm_code(p), m, n, A, lda, Cint(row_major), pointer(out, 1))
    st == RFLU_OK || error("librflu: ", last_error())
    return out[1]
end

"`lange_batched_dev!(out, A, batch, m, n, lda, strideA, row_major; p = 1)`: the norm of every matrix of a batch into the DEVICE array `out`"
function lange_batched_dev!(out::Ptr{Float64}, A::Ptr{Float64}, batch::Integer, m::Integer, n::Integer, lda::Integer, strideA::Integer,
                            row_major::Bool; p::Real = 1)
    st = ccall((:rflu_lange_batched_f64_dev, librflu), Cint,
               (Ptr{Cvoid}, Cint, Int64, Int64, Int64, Ptr{Float64}, Int64, Int64, Cint, Ptr{Float64}),
               handle(), norm_code(p), batch, m, n, A, lda, strideA, Cint(row_major), out)
    st == RFLU_OK || error("librflu: ", last_error())
    return nothing
end

function lange_batched_dev!(out::Ptr{Float64}, A::Ptr{Float32}, batch::Integer, m::Integer, n::Integer, lda::Integer, strideA::Integer,
                            row_major::Bool; p::Real = 1)
    st = ccall((:rflu_lange_batched_f32_dev, librflu), Cint,
               (Ptr{Cvoid}, Cint, Int64, Int64, Int64, Ptr{Float32}, Int64, Int64, Cint, Ptr{Float64}),
               handle(), norm_code(p), batch, m, n, A, lda, strideA, Cint(row_major), out)
    st == RFLU_OK || error("librflu: ", last_error())
    return nothing
end

function gecon_dev!(F::Ptr{Float64}, n::Integer, ld::Integer, anorm::Real; p::Real = 1, row_major::Bool = false)
    out = zeros(Float64, 1)
    st = if row_major
        GC.@preserve out ccall((:rflu_gecon_rm_f64_dev, librflu), Cint,
               (Ptr{Cvoid}, Cint, Int64, Ptr{Float64}, Int64, Cdouble, Ptr{Float64}),
               handle(), norm_code(p), n, F, ld, Cdouble(anorm), pointer(out, 1))
    else
        GC.@preserve out ccall((:rflu_gecon_f64_dev, librflu), Cint,
               (Ptr{Cvoid}, Cint, Int64, Ptr{Float64}, Int64, Cdouble, Ptr{Float64}),
               handle(), norm_code(p), n, F, ld, Cdouble(anorm), pointer(out, 1))
    end
    st == RFLU_OK || error("librflu: ", last_error())
    return out[1]
end

function gecon_dev!(F::Ptr{Float32}, n::Integer, ld::Integer, anorm::Real; p::Real = 1, row_major::Bool = false)
    out = zeros(Float64, 1)
    st = if row_major
        GC.@preserve out ccall((:rflu_gecon_rm_f32_dev, librflu), Cint,
               (Ptr{Cvoid}, Cint, Int64, Ptr{Float32}, Int64, Cdouble, Ptr{Float64}),
               handle(), norm_code(p), n, F, ld, Cdouble(anorm), pointer(out, 1))
    else
        GC.@preserve out ccall((:rflu_gecon_f32_dev, librflu), Cint,
               (Ptr{Cvoid}, Cint, Int64, Ptr{Float32}, Int64, Cdouble, Ptr{Float64}),
               handle(), norm_code(p), n, F, ld, Cdouble(anorm), pointer(out, 1))
    end
    st == RFLU_OK || error("librflu: ", last_error())
    return out[1]
end

function gecon_host(F::StridedMatrix{Float64}, anorm::Real; p::Real = 1)
    out = zeros(Float64, 1)
    st = GC.@preserve out ccall((:rflu_gecon_f64, librflu), Cint,
               (Ptr{Cvoid}, Cint, Int64, Ptr{Float64}, Int64, Cdouble, Ptr{Float64}),
               handle(), norm_code(p), size(F, 1), F, stride(F, 2), Cdouble(anorm), pointer(out, 1))
    st == RFLU_OK || error("librflu: ", last_error())
    return out[1]
end

function gecon_host(F::StridedMatrix{Float32}, anorm::Real; p::Real = 1)
    out = zeros(Float64, 1)
    st = GC.@preserve out ccall((:rflu_gecon_f32, librflu), Cint,
               (Ptr{Cvoid}, Cint, Int64, Ptr{Float32}, Int64, Cdouble, Ptr{Float64}),
               handle(), norm_code(p), size(F, 1), F, stride(F, 2), Cdouble(anorm), pointer(out, 1))
    st == RFLU_OK || error("librflu: ", last_error())
    return out[1]
end

function gecon_batched_dev!(rcond::Ptr{Float64}, F::Ptr{Float64}, batch::Integer, n::Integer, lda::Integer, strideF::Integer, row_major::Bool,
                            anorm::Ptr{Float64}; p::Real = 1)
    st = ccall((:rflu_gecon_batched_f64_dev, librflu), Cint,
               (Ptr{Cvoid}, Cint, Int64, Int64, Ptr{Float64}, Int64, Int64, Cint, Ptr{Float64}, Ptr{Float64}),
               handle(), norm_code(p), batch, n, F, lda, strideF, Cint(row_major), anorm, rcond)
    st == RFLU_OK || error("librflu: ", last_error())
    return nothing
end

function gecon_batched_dev!(rcond::Ptr{Float64}, F::Ptr{Float32}, batch::Integer, n::Integer, lda::Integer, strideF::Integer, row_major::Bool,
                            anorm::Ptr{Float64}; p::Real = 1)
    st = ccall((:rflu_gecon_batched_f32_dev, librflu), Cint,
               (Ptr{Cvoid}, Cint, Int64, Int64, Ptr{Float32}, Int64, Int64, Cint, Ptr{Float64}, Ptr{Float64}),
               handle(), norm_code(p), batch, n, F, lda, strideF, Cint(row_major), anorm, rcond)
    st == RFLU_OK || error("librflu: ", last_error())
    return nothing
end

# ---- inv! / logabsdet from ComplexF64 / ComplexF32 factors (rflu_getri_c* / rflu_logabsdet_c*, csrc/inverse.hip): the methods of
# getri! / getri_dev! / logabsdet_dev / logabsdet_host / logabsdet_batched_dev! for the complex pointer and matrix types.  Column-major
# only (there is no row-major complex entry); the sign is det / |det|, a ComplexF64 (batched: `sign` points at `batch` ComplexF64 values).
function getri!(F::StridedMatrix{ComplexF64}, ipiv::Ptr{Int64})
    info = Ref{Int64}(0)
    st = ccall((:rflu_getri_cf64, librflu), Cint,
               (Ptr{Cvoid}, Int64, Ptr{Float64}, Int64, Ptr{Int64}, Ref{Int64}),
               handle(), size(F, 1), reinterpret(Ptr{Float64}, pointer(F)), stride(F, 2), ipiv, info)
    st == RFLU_OK || error("librflu: ", last_error())
    return info[]
end

function getri_dev!(F::Ptr{ComplexF64}, n::Integer, ld::Integer, ipiv::Ptr{Int64})
    info = Ref{Int64}(0)
    st = ccall((:rflu_getri_cf64_dev, librflu), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}, Int64, Ptr{Int64}, Ref{Int64}),
               handle(), n, reinterpret(Ptr{Float64}, F), ld, ipiv, info)
    st == RFLU_OK || error("librflu: ", last_error())
    return info[]
end

function logabsdet_dev(F::Ptr{ComplexF64}, n::Integer, ld::Integer, ipiv::Ptr{Int64})
    out = zeros(Float64, 3)
    st = GC.@preserve out ccall((:rflu_logabsdet_cf64_dev, librflu), Cint,
               (Ptr{Cvoid}, Int64, Ptr{Float64}, Int64, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
               handle(), n, reinterpret(Ptr{Float64}, F), ld, ipiv, pointer(out, 1), pointer(out, 2), pointer(out, 3))
    st == RFLU_OK || error("librflu: ", last_error())
    return out[1], complex(out[2], out[3])
end

function logabsdet_host(F::StridedMatrix{ComplexF64}, ipiv::Ptr{Int64})
    out = zeros(Float64, 3)
    st = GC.@preserve out ccall((:rflu_logabsdet_cf64, librflu), Cint,
               (Ptr{Cvoid}, Int64, Ptr{Float64}, Int64, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
               handle(), size(F, 1), reinterpret(Ptr{Float64}, pointer(F)), stride(F, 2), ipiv, pointer(out, 1), pointer(out, 2), pointer(out, 3))
    st == RFLU_OK || error("librflu: ", last_error())
    return out[1], complex(out[2], out[3])
end

function logabsdet_batched_dev!(logabs::Ptr{Float64}, sign::Ptr{ComplexF64}, F::Ptr{ComplexF64}, batch::Integer, n::Integer, lda::Integer,
                                strideF::Integer, ipiv::Ptr{Int64}, stride_ipiv::Integer)
    st = ccall((:rflu_logabsdet_batched_cf64_dev, librflu), Cint,
               (Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Int64, Int64, Ptr{Int64}, Int64, Ptr{Float64}, Ptr{Float64}),
               handle(), batch, n, reinterpret(Ptr{Float64}, F), lda, strideF, ipiv, stride_ipiv, logabs, reinterpret(Ptr{Float64}, sign))
    st == RFLU_OK || error("librflu: ", last_error())
    return nothing
end

function getri!(F::StridedMatrix{ComplexF32}, ipiv::Ptr{Int64})
    info = Ref{Int64}(0)
    st = ccall((:rflu_getri_cf32, librflu), Cint,
               (Ptr{Cvoid}, Int64, Ptr{Float32}, Int64, Ptr{Int64}, Ref{Int64}),
               handle(), size(F, 1), reinterpret(Ptr{Float32}, pointer(F)), stride(F, 2), ipiv, info)
    st == RFLU_OK || error("librflu: ", last_error())
    return info[]
end

function getri_dev!(F::Ptr{ComplexF32}, n::Integer, ld::Integer, ipiv::Ptr{Int64})
    info = Ref{Int64}(0)
    st = ccall((:rflu_getri_cf32_dev, librflu), Cint, (Ptr{Cvoid}, Int64, Ptr{Float32}, Int64, Ptr{Int64}, Ref{Int64}),
               handle(), n, reinterpret(Ptr{Float32}, F), ld, ipiv, info)
    st == RFLU_OK || error("librflu: ", last_error())
    return info[]
end

function logabsdet_dev(F::Ptr{ComplexF32}, n::Integer, ld::Integer, ipiv::Ptr{Int64})
    out = zeros(Float64, 3)
    st = GC.@preserve out ccall((:rflu_logabsdet_cf32_dev, librflu), Cint,
               (Ptr{Cvoid}, Int64, Ptr{Float32}, Int64, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
               handle(), n, reinterpret(Ptr{Float32}, F), ld, ipiv, pointer(out, 1), pointer(out, 2), pointer(out, 3))
    st == RFLU_OK || error("librflu: ", last_error())
    return out[1], complex(out[2], out[3])
end

function logabsdet_host(F::StridedMatrix{ComplexF32}, ipiv::Ptr{Int64})
    out = zeros(Float64, 3)
    st = GC.@preserve out ccall((:rflu_logabsdet_cf32, librflu), Cint,
               (Ptr{Cvoid}, Int64, Ptr{Float32}, Int64, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
               handle(), size(F, 1), reinterpret(Ptr{Float32}, pointer(F)), stride(F, 2), ipiv, pointer(out, 1), pointer(out, 2), pointer(out, 3))
    st == RFLU_OK || error("librflu: ", last_error())
    return out[1], complex(out[2], out[3])
end

function logabsdet_batched_dev!(logabs::Ptr{Float64}, sign::Ptr{ComplexF64}, F::Ptr{ComplexF32}, batch::Integer, n::Integer, lda::Integer,
                                strideF::Integer, ipiv::Ptr{Int64}, stride_ipiv::Integer)
    st = ccall((:rflu_logabsdet_batched_cf32_dev, librflu), Cint,
               (Ptr{Cvoid}, Int64, Int64, Ptr{Float32}, Int64, Int64, Ptr{Int64}, Int64, Ptr{Float64}, Ptr{Float64}),
               handle(), batch, n, reinterpret(Ptr{Float32}, F), lda, strideF, ipiv, stride_ipiv, logabs, reinterpret(Ptr{Float64}, sign))
    st == RFLU_OK || error("librflu: ", last_error())
    return nothing
end

# the batched complex inverse (rflu_getri_batched_cf64_dev / _cf32_dev, csrc/batched_complex.hip): the real methods' arguments and a
# trailing `trans`: Ainv_b <- inv(A_b) ('N'), inv(transpose(A_b)) ('T') or inv(A_b') ('C'), out of place in the orientation of `F`
function getri_batched_dev!(Ainv::Ptr{ComplexF64}, ldi::Integer, strideI::Integer, F::Ptr{ComplexF64}, batch::Integer, n::Integer, lda::Integer,
                            strideF::Integer, row_major::Bool, ipiv::Ptr{Int64}, stride_ipiv::Integer, info::Ptr{Int64}, trans::AbstractChar)
    st = ccall((:rflu_getri_batched_cf64_dev, librflu), Cint,
               (Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Int64, Int64, Cint, Ptr{Int64}, Int64, Ptr{Float64}, Int64, Int64, Cint, Ptr{Int64}),
               handle(), batch, n, reinterpret(Ptr{Float64}, F), lda, strideF, Cint(row_major), ipiv, stride_ipiv, reinterpret(Ptr{Float64}, Ainv), ldi, strideI, batched_trans_code(trans), info)
    st == RFLU_OK || error("librflu: ", last_error())
    return Ainv
end

function getri_batched_dev!(Ainv::Ptr{ComplexF32}, ldi::Integer, strideI::Integer, F::Ptr{ComplexF32}, batch::Integer, n::Integer, lda::Integer,
                            strideF::Integer, row_major::Bool, ipiv::Ptr{Int64}, stride_ipiv::Integer, info::Ptr{Int64}, trans::AbstractChar)
    st = ccall((:rflu_getri_batched_cf32_dev, librflu), Cint,
               (Ptr{Cvoid}, Int64, Int64, Ptr{Float32}, Int64, Int64, Cint, Ptr{Int64}, Int64, Ptr{Float32}, Int64, Int64, Cint, Ptr{Int64}),
               handle(), batch, n, reinterpret(Ptr{Float32}, F), lda, strideF, Cint(row_major), ipiv, stride_ipiv, reinterpret(Ptr{Float32}, Ainv), ldi, strideI, batched_trans_code(trans), info)
    st == RFLU_OK || error("librflu: ", last_error())
    return Ainv
end

# ---- operator norms and the condition estimate for ComplexF64 / ComplexF32 (rflu_lange_c* / rflu_gecon_c*, csrc/condest.hip and
# cgecon_batched_kernel of csrc/batched_complex.hip): the methods of lange_dev / lange_batched_dev! / gecon_dev! / gecon_host /
# gecon_batched_dev! for the complex pointer and matrix types.  Moduli are hypot(re, im) in Float64; the estimator is LAPACK zlacn2 on M
# and M' with the start and closing vectors of include/rflu.h.  A single matrix is column-major only (there is no rflu_gecon_rm_c*, so
# gecon_dev! takes no row_major); leading dimensions and strides count complex elements.
function lange_dev(A::Ptr{ComplexF64}, m::Integer, n::Integer, lda::Integer; p::Real = 1, row_major::Bool = false)
    out = zeros(Float64, 1)
    st = GC.@preserve out ccall((:rflu_lange_cf64_dev, librflu), Cint,
               (Ptr{Cvoid}, Cint, Int64, Int64, Ptr{Float64}, Int64, Cint, Ptr{Float64}),
               handle(), norm_code(p), m, n, reinterpret(Ptr{Float64}, A), lda, Cint(row_major), pointer(out, 1))
    st == RFLU_OK || error("librflu: ", last_error())
    return out[1]
end

function lange_batched_dev!(out::Ptr{Float64}, A::Ptr{ComplexF64}, batch::Integer, m::Integer, n::Integer, lda::Integer, strideA::Integer,
                            row_major::Bool; p::Real = 1)
    st = ccall((:rflu_lange_batched_cf64_dev, librflu), Cint,
               (Ptr{Cvoid}, Cint, Int64, Int64, Int64, Ptr{Float64}, Int64, Int64, Cint, Ptr{Float64}),
               handle(), norm_code(p), batch, m, n, reinterpret(Ptr{Float64}, A), lda, strideA, Cint(row_major), out)
    st == RFLU_OK || error("librflu: ", last_error())
    return nothing
end

function gecon_dev!(F::Ptr{ComplexF64}, n::Integer, ld::Integer, anorm::Real; p::Real = 1)
    out = zeros(Float64, 1)
    st = GC.@preserve out ccall((:rflu_gecon_cf64_dev, librflu), Cint,
               (Ptr{Cvoid}, Cint, Int64, Ptr{Float64}, Int64, Cdouble, Ptr{Float64}),
               handle(), norm_code(p), n, reinterpret(Ptr{Float64}, F), ld, Cdouble(anorm), pointer(out, 1))
    st == RFLU_OK || error("librflu: ", last_error())
    return out[1]
end

function gecon_host(F::StridedMatrix{ComplexF64}, anorm::Real; p::Real = 1)
    out = zeros(Float64, 1)
    st = GC.@preserve out ccall((:rflu_gecon_cf64, librflu), Cint,
               (Ptr{Cvoid}, Cint, Int64, Ptr{Float64}, Int64, Cdouble, Ptr{Float64}),
               handle(), norm_code(p), size(F, 1), reinterpret(Ptr{Float64}, pointer(F)), stride(F, 2), Cdouble(anorm), pointer(out, 1))
    st == RFLU_OK || error("librflu: ", last_error())
    return out[1]
end

function gecon_batched_dev!(rcond::Ptr{Float64}, F::Ptr{ComplexF64}, batch::Integer, n::Integer, lda::Integer, strideF::Integer, row_major::Bool,
                            anorm::Ptr{Float64}; p::Real = 1)
    st = ccall((:rflu_gecon_batched_cf64_dev, librflu), Cint,
               (Ptr{Cvoid}, Cint, Int64, Int64, Ptr{Float64}, Int64, Int64, Cint, Ptr{Float64}, Ptr{Float64}),
               handle(), norm_code(p), batch, n, reinterpret(Ptr{Float64}, F), lda, strideF, Cint(row_major), anorm, rcond)
    st == RFLU_OK || error("librflu: ", last_error())
    return nothing
end

function lange_dev(A::Ptr{ComplexF32}, m::Integer, n::Integer, lda::Integer; p::Real = 1, row_major::Bool = false)
    out = zeros(Float64, 1)
    st = GC.@preserve out ccall((:rflu_lange_cf32_dev, librflu), Cint,
               (Ptr{Cvoid}, Cint, Int64, Int64, Ptr{Float32}, Int64, Cint, Ptr{Float64}),
               handle(), norm_code(p), m, n, reinterpret(Ptr{Float32}, A), lda, Cint(row_major), pointer(out, 1))
    st == RFLU_OK || error("librflu: ", last_error())
    return out[1]
end

function lange_batched_dev!(out::Ptr{Float64}, A::Ptr{ComplexF32}, batch::Integer, m::Integer, n::Integer, lda::Integer, strideA::Integer,
                            row_major::Bool; p::Real = 1)
    st = ccall((:rflu_lange_batched_cf32_dev, librflu), Cint,
               (Ptr{Cvoid}, Cint, Int64, Int64, Int64, Ptr{Float32}, Int64, Int64, Cint, Ptr{Float64}),
               handle(), norm_code(p), batch, m, n, reinterpret(Ptr{Float32}, A), lda, strideA, Cint(row_major), out)
    st == RFLU_OK || error("librflu: ", last_error())
    return nothing
end

function gecon_dev!(F::Ptr{ComplexF32}, n::Integer, ld::Integer, anorm::Real; p::Real = 1)
    out = zeros(Float64, 1)
    st = GC.@preserve out ccall((:rflu_gecon_cf32_dev, librflu), Cint,
               (Ptr{Cvoid}, Cint, Int64, Ptr{Float32}, Int64, Cdouble, Ptr{Float64}),
               handle(), norm_code(p), n, reinterpret(Ptr{Float32}, F), ld, Cdouble(anorm), pointer(out, 1))
    st == RFLU_OK || error("librflu: ", last_error())
    return out[1]
end

function gecon_host(F::StridedMatrix{ComplexF32}, anorm::Real; p::Real = 1)
    out = zeros(Float64, 1)
    st = GC.@preserve out ccall((:rflu_gecon_cf32, librflu), Cint,
               (Ptr{Cvoid}, Cint, Int64, Ptr{Float32}, Int64, Cdouble, Ptr{Float64}),
               handle(), norm_code(p), size(F, 1), reinterpret(Ptr{Float32}, pointer(F)), stride(F, 2), Cdouble(anorm), pointer(out, 1))
    st == RFLU_OK || error("librflu: ", last_error())
    return out[1]
end

function gecon_batched_dev!(rcond::Ptr{Float64}, F::Ptr{ComplexF32}, batch::Integer, n::Integer, lda::Integer, strideF::Integer, row_major::Bool,
                            anorm::Ptr{Float64}; p::Real = 1)
    st = ccall((:rflu_gecon_batched_cf32_dev, librflu), Cint,
               (Ptr{Cvoid}, Cint, Int64, Int64, Ptr{Float32}, Int64, Int64, Cint, Ptr{Float64}, Ptr{Float64}),
               handle(), norm_code(p), batch, n, reinterpret(Ptr{Float32}, F), lda, strideF, Cint(row_major), anorm, rcond)
    st == RFLU_OK || error("librflu: ", last_error())
    return nothing
end

# ---- dispatch: who serves a call (RecursiveFactorization src/lu.jl:92-93, 114-126) -------------------------------------------
const GPUEltype = Union{Float32, Float64}                                  # every entry serves these
const GPUAnyEltype = Union{Float32, Float64, ComplexF32, ComplexF64}       # lu! and ldiv!(F, B) serve the complex types as well
const GPUComplexEltype = Union{ComplexF32, ComplexF64}                     # ldiv!(F', B) / ldiv!(transpose(F), B): two different solves
gpu_ok(A::StridedMatrix{<:GPUAnyEltype}, ipiv) =
    stride(A, 1) == 1 && min(size(A)...) >= GPU_MIN_N[] && (ipiv isa Vector{Int64} || ipiv isa NotIPIV) && available()
gpu_ok(A, ipiv) = false

const CPU_FALLBACK = Ref{Any}(nothing)   # set to RecursiveFactorization.lu! by the user / an extension when that package is loaded
function cpu_lu!(A, ipiv, pivot, thread; check, kwargs...)
    f = CPU_FALLBACK[]
    f === nothing || return f(A, ipiv, pivot, thread; check = check, kwargs...)
    F = LinearAlgebra.lu!(A, pivot === Val(true) ? RowMaximum() : NoPivot(); check = check)
    ipiv isa AbstractVector && !(ipiv isa NotIPIV) && copyto!(ipiv, F.ipiv)
    return LU(F.factors, ipiv isa NotIPIV ? F.ipiv : ipiv, F.info)
end

"""
    lu!(A, ipiv, pivot = Val(true), thread = Val(false); check = Val(true), blocksize = 0, threshold = 0)

The method LinearSolve's `RFLUFactorization` calls (RecursiveFactorization `src/lu.jl:97-130`), served by the MI355X.
`blocksize`: 0 = library default, negative = pure Toledo recursion, 64/128/256... = outer block-column width (see rflu.h);
`threshold` and `thread` are accepted for signature parity (the GPU path has neither knob).
"""
function lu!(A::AbstractMatrix{T}, ipiv::AbstractVector{<:Integer}, pivot = Val(true), thread = Val(false);
             check::Union{Bool, Val{true}, Val{false}} = Val(true), blocksize::Integer = 0,
             threshold::Integer = 0) where {T}
    pivot = normalize_pivot(pivot)
    check isa Bool && (check = Val(check))
    gpu_ok(A, ipiv) || return cpu_lu!(A, ipiv, pivot, thread; check = check === Val(true))
    mnmin = min(size(A)...)
    if pivot === Val(false) && !(ipiv isa NotIPIV)
        copyto!(ipiv, 1:mnmin)                                  # src/lu.jl:111-113 (the library fills it as well)
    end
    p = ipiv isa NotIPIV ? Ptr{Int64}(C_NULL) : pointer(ipiv)
    info = GC.@preserve A ipiv getrf!(A, p, pivot === Val(true), blocksize)
    (pivot === Val(false) && NOPIVOT_NEGATIVE_INFO) && (info = -info)   # src/lu.jl:249-254, 323-326
    check === Val(true) && checknonsingular(info)                       # src/lu.jl:128
    return LU(A, ipiv, info)                                            # src/lu.jl:129
end

function lu!(A::AbstractMatrix, pivot = Val(true), thread = Val(false); check = Val(true), kwargs...)   # src/lu.jl:67-83
    npivot = normalize_pivot(pivot)
    return lu!(A, init_pivot(npivot, min(size(A)...)), npivot, thread; check = check, kwargs...)
end

lu(A::AbstractMatrix, pivot = Val(true), thread = Val(false); kwargs...) = lu!(copy(A), pivot, thread; kwargs...)   # :19-21

for (f, T) in [(:adjoint, :Adjoint), (:transpose, :Transpose)], lufn in (:lu, :lu!)      # src/lu.jl:85-87
    @eval $lufn(A::$T, args...; kwargs...) = $f($lufn(parent(A), args...; kwargs...))
end

"solve with the factors on the GPU when they are large enough, else stdlib `ldiv!`"
function ldiv!(F::LU{T, <:StridedMatrix{T}}, B::StridedVecOrMat{T}) where {T <: GPUAnyEltype}
    # the same layout conditions as `gpu_ok` for lu!: getrs! passes stride(F, 2) / stride(B, 2) as leading dimensions, i.e. it
    # assumes unit row stride and a square factorization; anything else (a strided view, an LU from a non-unit-stride CPU
    # fallback, a B with the wrong number of rows) stays with the stdlib
    lay_ok = stride(F.factors, 1) == 1 && stride(B, 1) == 1 && size(F.factors, 1) == size(F.factors, 2) == size(B, 1)
    if lay_ok && size(F.factors, 1) >= GPU_MIN_N[] && available() && (F.ipiv isa Vector{Int64} || F.ipiv isa NotIPIV)
        p = F.ipiv isa NotIPIV ? Ptr{Int64}(C_NULL) : pointer(F.ipiv)
        GC.@preserve F B getrs!(F.factors, p, B)
        return B
    end
    return LinearAlgebra.ldiv!(F, B)
end

# ---- inv! / det / logabsdet on the LU object: the GPU under the conditions of `ldiv!(F, B)`, else the stdlib ------------------------------
lu_on_gpu(F::LU) = stride(F.factors, 1) == 1 && size(F.factors, 1) == size(F.factors, 2) && size(F.factors, 1) >= GPU_MIN_N[] &&
                   available() && (F.ipiv isa Vector{Int64} || F.ipiv isa NotIPIV)

"`inv!(F)`: the factors are overwritten by `inv(A)` (LAPACK getri on the GPU) -- `F` is invalid afterwards; SingularException as the stdlib"
function inv!(F::LU{T, <:StridedMatrix{T}}) where {T <: GPUEltype}
    lu_on_gpu(F) || return LinearAlgebra.inv!(F)
    checknonsingular(F.info)
    p = F.ipiv isa NotIPIV ? Ptr{Int64}(C_NULL) : pointer(F.ipiv)
    info = GC.@preserve F getri!(F.factors, p)
    checknonsingular(info)
    return F.factors
end

"`logabsdet(F)`: (log|det A|, sign) with the element type of `F`, summed in Float64 on the GPU; only the diagonal and ipiv travel"
function logabsdet(F::LU{T, <:StridedMatrix{T}}) where {T <: GPUEltype}
    lu_on_gpu(F) || return LinearAlgebra.logabsdet(F)
    p = F.ipiv isa NotIPIV ? Ptr{Int64}(C_NULL) : pointer(F.ipiv)
    la, sg = GC.@preserve F logabsdet_host(F.factors, p)
    return T(la), T(sg)
end

"`det(F)` = sign * exp(logabs): equal to the stdlib's running product up to rounding, 0 for a singular `F`"
function det(F::LU{T, <:StridedMatrix{T}}) where {T <: GPUEltype}
    lu_on_gpu(F) || return LinearAlgebra.det(F)
    la, sg = logabsdet(F)
    return iszero(sg) ? zero(T) : sg * exp(la)
end

"""
    rcond(F::LU, anorm; p = 1)

`1 / (opnorm(A, p) * opnorm(inv(A), p))` estimated from the factors on the GPU (LAPACK gecon; `anorm = opnorm(A, p)` taken before
`lu!`), `p` 1 or Inf; the stdlib's `LAPACK.gecon!` where the GPU path does not apply.
"""
function rcond(F::LU{T, <:StridedMatrix{T}}, anorm::Real; p::Real = 1) where {T <: GPUEltype}
    lu_on_gpu(F) || return LinearAlgebra.LAPACK.gecon!(p == 1 ? '1' : 'I', copy(F.factors), T(anorm))
    return GC.@preserve F gecon_host(F.factors, anorm; p = p)
end

# rcond of a complex LU: LAPACK zgecon / cgecon's place.  The real type of anorm is that of the element; |conj z| = |z|, so F' and
# transpose(F) share their condition number and only swap p = 1 and p = Inf, which is left to the caller as for the real method.
function rcond(F::LU{T, <:StridedMatrix{T}}, anorm::Real; p::Real = 1) where {T <: GPUComplexEltype}
    lu_on_gpu(F) || return LinearAlgebra.LAPACK.gecon!(p == 1 ? '1' : 'I', copy(F.factors), real(T)(anorm))
    return GC.@preserve F gecon_host(F.factors, anorm; p = p)
end

# the complex element types: the same three on the GPU.  The sign is the unit complex number det / |det|; adjoint / transpose wrappers of
# an LU are left to the stdlib (det(F') is the conjugate, det(transpose(F)) the plain value: LinearAlgebra derives both from these).
function inv!(F::LU{T, <:StridedMatrix{T}}) where {T <: GPUComplexEltype}
    lu_on_gpu(F) || return LinearAlgebra.inv!(F)
    checknonsingular(F.info)
    p = F.ipiv isa NotIPIV ? Ptr{Int64}(C_NULL) : pointer(F.ipiv)
    info = GC.@preserve F getri!(F.factors, p)
    checknonsingular(info)
    return F.factors
end

function logabsdet(F::LU{T, <:StridedMatrix{T}}) where {T <: GPUComplexEltype}
    lu_on_gpu(F) || return LinearAlgebra.logabsdet(F)
    p = F.ipiv isa NotIPIV ? Ptr{Int64}(C_NULL) : pointer(F.ipiv)
    la, sg = GC.@preserve F logabsdet_host(F.factors, p)
    return real(T)(la), T(sg)
end

function det(F::LU{T, <:StridedMatrix{T}}) where {T <: GPUComplexEltype}
    lu_on_gpu(F) || return LinearAlgebra.det(F)
    la, sg = logabsdet(F)
    return iszero(sg) ? zero(T) : sg * exp(la)
end

# What `F'` and `transpose(F)` of an LU are: AdjointFactorization / TransposeFactorization from Julia 1.10 on (where the transpose of a
# real factorization is its adjoint), the array wrappers Adjoint / Transpose in Julia 1.9, the oldest version Project.toml admits.
@static if isdefined(LinearAlgebra, :AdjointFactorization)
    const AdjointLU{T} = LinearAlgebra.AdjointFactorization{T, <:LU{T, <:StridedMatrix{T}}}
    const TransposeLU{T} = LinearAlgebra.TransposeFactorization{T, <:LU{T, <:StridedMatrix{T}}}
else
    const AdjointLU{T} = Adjoint{T, <:LU{T, <:StridedMatrix{T}}}
    const TransposeLU{T} = Transpose{T, <:LU{T, <:StridedMatrix{T}}}
end

"solve A' x = b / transpose(A) x = b with the factors of A on the GPU (same conditions as `ldiv!(F, B)`), else stdlib `ldiv!`"
function ldiv!(Ft::Union{AdjointLU{T}, TransposeLU{T}}, B::StridedVecOrMat{T}) where {T <: GPUEltype}
    F = parent(Ft)
    lay_ok = stride(F.factors, 1) == 1 && stride(B, 1) == 1 && size(F.factors, 1) == size(F.factors, 2) == size(B, 1)
    if lay_ok && size(F.factors, 1) >= GPU_MIN_N[] && available() && (F.ipiv isa Vector{Int64} || F.ipiv isa NotIPIV)
        p = F.ipiv isa NotIPIV ? Ptr{Int64}(C_NULL) : pointer(F.ipiv)
        GC.@preserve F B getrs_trans!(F.factors, p, B)
        return B
    end
    return LinearAlgebra.ldiv!(Ft, B)
end

"solve A' x = b (the conjugate transpose) with complex factors of A on the GPU (same conditions as `ldiv!(F, B)`), else stdlib `ldiv!`"
function ldiv!(Ft::AdjointLU{T}, B::StridedVecOrMat{T}) where {T <: GPUComplexEltype}
    F = parent(Ft)
    lay_ok = stride(F.factors, 1) == 1 && stride(B, 1) == 1 && size(F.factors, 1) == size(F.factors, 2) == size(B, 1)
    if lay_ok && size(F.factors, 1) >= GPU_MIN_N[] && available() && (F.ipiv isa Vector{Int64} || F.ipiv isa NotIPIV)
        p = F.ipiv isa NotIPIV ? Ptr{Int64}(C_NULL) : pointer(F.ipiv)
        GC.@preserve F B getrs_ctrans!(F.factors, p, B, true)
        return B
    end
    return LinearAlgebra.ldiv!(Ft, B)
end

"solve transpose(A) x = b (no conjugation) with complex factors of A on the GPU (same conditions as `ldiv!(F, B)`), else stdlib `ldiv!`"
function ldiv!(Ft::TransposeLU{T}, B::StridedVecOrMat{T}) where {T <: GPUComplexEltype}
    F = parent(Ft)
    lay_ok = stride(F.factors, 1) == 1 && stride(B, 1) == 1 && size(F.factors, 1) == size(F.factors, 2) == size(B, 1)
    if lay_ok && size(F.factors, 1) >= GPU_MIN_N[] && available() && (F.ipiv isa Vector{Int64} || F.ipiv isa NotIPIV)
        p = F.ipiv isa NotIPIV ? Ptr{Int64}(C_NULL) : pointer(F.ipiv)
        GC.@preserve F B getrs_ctrans!(F.factors, p, B, false)
        return B
    end
    return LinearAlgebra.ldiv!(Ft, B)
end

"""
    RFLUAMDFactorization(; pivot = Val(true), blocksize = 0)

LinearSolve.jl algorithm with the cache protocol of `RFLUFactorization{P,T}`: `cacheval = (fact, ipiv)`, `lu!(A, ipiv,
Val(P), Val(false); check = false)` when the cache is fresh, `issuccess(fact)` -> `ReturnCode.Failure`, then `ldiv!`.
The methods live in the package extension `ext/RFLUAMDLinearSolveExt.jl` (loaded with LinearSolve).
"""
struct RFLUAMDFactorization{P}
    blocksize::Int
    RFLUAMDFactorization(::Val{P}, blocksize::Integer = 0) where {P} = new{P}(Int(blocksize))
end
RFLUAMDFactorization(; pivot = Val(true), blocksize::Integer = 0) = RFLUAMDFactorization(normalize_pivot(pivot), blocksize)

# ---- mixed precision: Float32 factors of a Float64 matrix + Float64 iterative refinement (rflu_mixed_*_f64_dev, include/rflu.h) ----
# Device pointers, like the batched entries: the matrix stays in HBM (the buffer of an AMDGPU.jl ROCArray) and is only read.
"raw entry: Float32 row-major factors of the column-major Float64 `A` into `F32` (ldf >= n); returns `(info, anorm)`"
function mixed_getrf_dev!(A::Ptr{Float64}, n::Integer, lda::Integer, F32::Ptr{Float32}, ldf::Integer, ipiv::Ptr{Int64}, pivot::Bool,
                          blocksize::Integer)
    info = Ref{Int64}(0)
    anorm = Ref{Float64}(0.0)
    st = GC.@preserve anorm ccall((:rflu_mixed_getrf_f64_dev, librflu), Cint,
               (Ptr{Cvoid}, Int64, Ptr{Float64}, Int64, Ptr{Float32}, Int64, Ptr{Int64}, Cint, Int64, Ptr{Float64}, Ref{Int64}),
               handle(), n, A, lda, F32, ldf, ipiv, Cint(pivot), blocksize, Base.unsafe_convert(Ptr{Float64}, anorm), info)
    st == RFLU_OK || error("librflu: ", last_error())
    return BlasInt(info[]), anorm[]
end

"raw entry: `X <- A \\ B` by refinement; returns `iters` (>= 0 converged after that many steps, < 0 not converged: do not use `X`)"
function mixed_getrs_dev!(A::Ptr{Float64}, n::Integer, nrhs::Integer, lda::Integer, F32::Ptr{Float32}, ldf::Integer, ipiv::Ptr{Int64},
                          anorm::Float64, B::Ptr{Float64}, ldb::Integer, X::Ptr{Float64}, ldx::Integer, max_iter::Integer)
    iters = Ref{Cint}(0)
    st = GC.@preserve iters ccall((:rflu_mixed_getrs_f64_dev, librflu), Cint,
               (Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Int64, Ptr{Float32}, Int64, Ptr{Int64}, Cdouble, Ptr{Float64}, Int64, Ptr{Float64},
                Int64, Cint, Ptr{Cint}),
               handle(), n, nrhs, A, lda, F32, ldf, ipiv, anorm, B, ldb, X, ldx, Cint(max_iter), Base.unsafe_convert(Ptr{Cint}, iters))
    st == RFLU_OK || error("librflu: ", last_error())
    return Int(iters[])
end

"raw entry: `R <- B - A X` in Float64, everything column-major in HBM"
function residual_dev!(R::Ptr{Float64}, ldr::Integer, A::Ptr{Float64}, n::Integer, nrhs::Integer, lda::Integer, X::Ptr{Float64},
                       ldx::Integer, B::Ptr{Float64}, ldb::Integer)
    st = ccall((:rflu_residual_f64_dev, librflu), Cint,
               (Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Int64),
               handle(), n, nrhs, A, lda, X, ldx, B, ldb, R, ldr)
    st == RFLU_OK || error("librflu: ", last_error())
    return R
end

"""
    MixedLU

What `lu_mixed` returns: the untouched Float64 matrix `A` (device pointer, `n`, `lda`), its Float32 factors `F32` (row-major, `ldf`),
`ipiv` (`C_NULL` = NotIPIV), `info` of the Float32 factorization, `anorm = ||A||_inf` and the `iters` of the last `ldiv_mixed!`.
The caller owns every buffer and keeps it alive.
"""
mutable struct MixedLU
    A::Ptr{Float64}
    n::Int
    lda::Int
    F32::Ptr{Float32}
    ldf::Int
    ipiv::Ptr{Int64}
    info::BlasInt
    anorm::Float64
    iters::Int
end

"""
    lu_mixed(A, n, lda, F32, ldf, ipiv, pivot = Val(true); blocksize = 0) -> MixedLU

Factor a Float32 copy of the `n x n` column-major Float64 matrix at the device pointer `A` into the caller's `F32` (`n x ldf` Float32,
row-major) and `ipiv` (`n` Int64; `C_NULL` with `Val(false)`).  `A` is not modified.  A zero pivot of the Float32 factorization is
reported in `info` (negative for NoPivot under `NOPIVOT_NEGATIVE_INFO`), never thrown: the caller falls back to `lu!` in Float64.
"""
function lu_mixed(A::Ptr{Float64}, n::Integer, lda::Integer, F32::Ptr{Float32}, ldf::Integer, ipiv::Ptr{Int64}, pivot = Val(true);
                  blocksize::Integer = 0)
    pivot = normalize_pivot(pivot)
    info, anorm = mixed_getrf_dev!(A, n, lda, F32, ldf, ipiv, pivot === Val(true), blocksize)
    (pivot === Val(false) && NOPIVOT_NEGATIVE_INFO) && (info = -info)
    return MixedLU(A, Int(n), Int(lda), F32, Int(ldf), ipiv, info, anorm, 0)
end

"""
    ldiv_mixed!(X, ldx, F::MixedLU, B, ldb, nrhs; max_iter = 30) -> Bool

`X <- A \\ B` (device pointers, column-major) by Float32 solves and Float64 residuals.  `true`: converged, `F.iters` steps were taken.
`false`: the Float32 factorization hit a zero pivot or the refinement did not converge within `max_iter` steps (`F.iters < 0`);
`X` must not be used and the caller solves with the Float64 factorization instead (the LinearSolve extension does).
"""
function ldiv_mixed!(X::Ptr{Float64}, ldx::Integer, F::MixedLU, B::Ptr{Float64}, ldb::Integer, nrhs::Integer; max_iter::Integer = 30)
    F.info == 0 || return false
    F.iters = mixed_getrs_dev!(F.A, F.n, nrhs, F.lda, F.F32, F.ldf, F.ipiv, F.anorm, B, ldb, X, ldx, max_iter)
    return F.iters >= 0
end

# ---- iterative refinement with error bounds: LAPACK gerfs, trans = 'N' (rflu_gerfs_*_dev / rflu_berr_*_dev, include/rflu.h) ----
# Device pointers, column-major, like the mixed-precision entries.  A is the ORIGINAL matrix, F / ipiv what getrf_dev! left (C_NULL =
# NotIPIV); A, F and B are only read, X is refined in place.  Residuals are accumulated in Float64 for both element types.
"raw entry: refine `X` in place; returns `(info, ferr, berr, steps)` (`ferr` is `nothing` when skipped; `info != 0`: a zero `u_ii`, nothing written)"
function gerfs_dev!(X::Ptr{Float64}, ldx::Integer, A::Ptr{Float64}, n::Integer, nrhs::Integer, lda::Integer, F::Ptr{Float64}, ldf::Integer,
                    ipiv::Ptr{Int64}, B::Ptr{Float64}, ldb::Integer; max_iter::Integer = 5, ferr::Bool = true)
    fe, be, steps, info = zeros(Float64, max(nrhs, 1)), zeros(Float64, max(nrhs, 1)), zeros(Cint, max(nrhs, 1)), Ref{Int64}(0)
    st = GC.@preserve fe be steps ccall((:rflu_gerfs_f64_dev, librflu), Cint,
               (Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Ptr{Int64}, Ptr{Float64}, Int64, Ptr{Float64}, Int64,
                Ptr{Float64}, Ptr{Float64}, Cint, Ptr{Cint}, Ref{Int64}),
               handle(), n, nrhs, A, lda, F, ldf, ipiv, B, ldb, X, ldx, ferr ? pointer(fe, 1) : Ptr{Float64}(C_NULL), pointer(be, 1),
               Cint(max_iter), pointer(steps, 1), info)
    st == RFLU_OK || error("librflu: ", last_error())
    return BlasInt(info[]), (ferr ? fe[1:nrhs] : nothing), be[1:nrhs], Int.(steps[1:nrhs])
end

function gerfs_dev!(X::Ptr{Float32}, ldx::Integer, A::Ptr{Float32}, n::Integer, nrhs::Integer, lda::Integer, F::Ptr{Float32}, ldf::Integer,
                    ipiv::Ptr{Int64}, B::Ptr{Float32}, ldb::Integer; max_iter::Integer = 5, ferr::Bool = true)
    fe, be, steps, info = zeros(Float64, max(nrhs, 1)), zeros(Float64, max(nrhs, 1)), zeros(Cint, max(nrhs, 1)), Ref{Int64}(0)
    st = GC.@preserve fe be steps ccall((:rflu_gerfs_f32_dev, librflu), Cint,
               (Ptr{Cvoid}, Int64, Int64, Ptr{Float32}, Int64, Ptr{Float32}, Int64, Ptr{Int64}, Ptr{Float32}, Int64, Ptr{Float32}, Int64,
                Ptr{Float64}, Ptr{Float64}, Cint, Ptr{Cint}, Ref{Int64}),
               handle(), n, nrhs, A, lda, F, ldf, ipiv, B, ldb, X, ldx, ferr ? pointer(fe, 1) : Ptr{Float64}(C_NULL), pointer(be, 1),
               Cint(max_iter), pointer(steps, 1), info)
    st == RFLU_OK || error("librflu: ", last_error())
    return BlasInt(info[]), (ferr ? fe[1:nrhs] : nothing), be[1:nrhs], Int.(steps[1:nrhs])
end

"raw entry: the componentwise backward error `max_i |b - A x|_i / (|b| + |A| |x|)_i` of every column of any `X`; needs no factors"
function berr_dev(A::Ptr{Float64}, n::Integer, nrhs::Integer, lda::Integer, X::Ptr{Float64}, ldx::Integer, B::Ptr{Float64}, ldb::Integer)
    be = zeros(Float64, max(nrhs, 1))
    st = GC.@preserve be ccall((:rflu_berr_f64_dev, librflu), Cint,
               (Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Ptr{Float64}),
               handle(), n, nrhs, A, lda, X, ldx, B, ldb, pointer(be, 1))
    st == RFLU_OK || error("librflu: ", last_error())
    return be[1:nrhs]
end

function berr_dev(A::Ptr{Float32}, n::Integer, nrhs::Integer, lda::Integer, X::Ptr{Float32}, ldx::Integer, B::Ptr{Float32}, ldb::Integer)
    be = zeros(Float64, max(nrhs, 1))
    st = GC.@preserve be ccall((:rflu_berr_f32_dev, librflu), Cint,
               (Ptr{Cvoid}, Int64, Int64, Ptr{Float32}, Int64, Ptr{Float32}, Int64, Ptr{Float32}, Int64, Ptr{Float64}),
               handle(), n, nrhs, A, lda, X, ldx, B, ldb, pointer(be, 1))
    st == RFLU_OK || error("librflu: ", last_error())
    return be[1:nrhs]
end

"""
    refine!(F::LU, A, B, X, nrhs; factors, ipiv = C_NULL, lda, ldf, ldb, ldx, max_iter = 5, ferr = true) -> (ferr, berr, steps)

LAPACK gerfs for the system `F` factored: refine the computed solution at the device pointer `X` (`n x nrhs`, column-major) of
`A X = B` in place and return, per right-hand side, the forward error bound (`nothing` with `ferr = false`: the bound costs up to 11
one-column solves per right-hand side), the componentwise backward error of the returned `X` and the corrections applied.  `F`
supplies the size and `info`; the factors live in HBM at `factors` (column-major, as `getrf_dev!` left them) with their pivots at
`ipiv` (`C_NULL` for NotIPIV).  `A` is the original matrix.  Leading dimensions default to `n`.  Throws `SingularException` for a
zero `u_ii`; `X` is then untouched.  `F'`, complex element types, row-major storage and batches are not served.
"""
function refine!(F::LU{T}, A::Ptr{T}, B::Ptr{T}, X::Ptr{T}, nrhs::Integer; factors::Ptr{T}, ipiv::Ptr{Int64} = Ptr{Int64}(C_NULL),
                 lda::Integer = size(F.factors, 1), ldf::Integer = size(F.factors, 1), ldb::Integer = size(F.factors, 1),
                 ldx::Integer = size(F.factors, 1), max_iter::Integer = 5, ferr::Bool = true) where {T <: GPUEltype}
    checknonsingular(F.info)
    n = LinearAlgebra.checksquare(F.factors)
    info, fe, be, steps = gerfs_dev!(X, max(ldx, 1), A, n, nrhs, max(lda, 1), factors, max(ldf, 1), ipiv, B, max(ldb, 1);
                                     max_iter = max_iter, ferr = ferr)
    checknonsingular(info)
    return fe, be, steps
end

# ---- complex mixed precision: ComplexF32 factors of a ComplexF64 matrix + ComplexF64 refinement (rflu_mixed_*_cf64_dev) ----
# The C entries take double* / float* to interleaved (re, im) pairs, which is the storage of Complex{T}: the pointers are reinterpreted.
# Leading dimensions count complex elements.  There is no blocksize.
"raw entry: ComplexF32 row-major factors of the column-major ComplexF64 `A` into `F32` (ldf >= n); returns `(info, anorm)`"
function mixed_getrf_dev!(A::Ptr{ComplexF64}, n::Integer, lda::Integer, F32::Ptr{ComplexF32}, ldf::Integer, ipiv::Ptr{Int64}, pivot::Bool)
    info = Ref{Int64}(0)
    anorm = Ref{Float64}(0.0)
    st = GC.@preserve anorm ccall((:rflu_mixed_getrf_cf64_dev, librflu), Cint,
               (Ptr{Cvoid}, Int64, Ptr{Float64}, Int64, Ptr{Float32}, Int64, Ptr{Int64}, Cint, Ptr{Float64}, Ref{Int64}),
               handle(), n, Ptr{Float64}(A), lda, Ptr{Float32}(F32), ldf, ipiv, Cint(pivot), Base.unsafe_convert(Ptr{Float64}, anorm), info)
    st == RFLU_OK || error("librflu: ", last_error())
    return BlasInt(info[]), anorm[]
end

"raw entry: `X <- A \\ B` by refinement in ComplexF64; returns `iters` (>= 0 converged, < 0 not converged: do not use `X`)"
function mixed_getrs_dev!(A::Ptr{ComplexF64}, n::Integer, nrhs::Integer, lda::Integer, F32::Ptr{ComplexF32}, ldf::Integer, ipiv::Ptr{Int64},
                          anorm::Float64, B::Ptr{ComplexF64}, ldb::Integer, X::Ptr{ComplexF64}, ldx::Integer, max_iter::Integer)
    iters = Ref{Cint}(0)
    st = GC.@preserve iters ccall((:rflu_mixed_getrs_cf64_dev, librflu), Cint,
               (Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Int64, Ptr{Float32}, Int64, Ptr{Int64}, Cdouble, Ptr{Float64}, Int64, Ptr{Float64},
                Int64, Cint, Ptr{Cint}),
               handle(), n, nrhs, Ptr{Float64}(A), lda, Ptr{Float32}(F32), ldf, ipiv, anorm, Ptr{Float64}(B), ldb, Ptr{Float64}(X), ldx,
               Cint(max_iter), Base.unsafe_convert(Ptr{Cint}, iters))
    st == RFLU_OK || error("librflu: ", last_error())
    return Int(iters[])
end

"raw entry: `R <- B - A X` in ComplexF64, everything column-major in HBM"
function residual_dev!(R::Ptr{ComplexF64}, ldr::Integer, A::Ptr{ComplexF64}, n::Integer, nrhs::Integer, lda::Integer, X::Ptr{ComplexF64},
                       ldx::Integer, B::Ptr{ComplexF64}, ldb::Integer)
    st = ccall((:rflu_residual_cf64_dev, librflu), Cint,
               (Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Int64),
               handle(), n, nrhs, Ptr{Float64}(A), lda, Ptr{Float64}(X), ldx, Ptr{Float64}(B), ldb, Ptr{Float64}(R), ldr)
    st == RFLU_OK || error("librflu: ", last_error())
    return R
end

"raw entry (building block): `B <- U^-1 L^-1 P B` with the row-major ComplexF32 factors `F32`, `B` column-major in HBM"
function mixed_solve_dev!(B::Ptr{ComplexF32}, ldb::Integer, F32::Ptr{ComplexF32}, n::Integer, nrhs::Integer, ldf::Integer, ipiv::Ptr{Int64})
    st = ccall((:rflu_mixed_solve_cf32_dev, librflu), Cint,
               (Ptr{Cvoid}, Int64, Int64, Ptr{Float32}, Int64, Ptr{Int64}, Ptr{Float32}, Int64),
               handle(), n, nrhs, Ptr{Float32}(F32), ldf, ipiv, Ptr{Float32}(B), ldb)
    st == RFLU_OK || error("librflu: ", last_error())
    return B
end

"""
    ComplexMixedLU

`MixedLU` for a ComplexF64 matrix: `A` (device pointer, untouched), its ComplexF32 factors `F32` (row-major, `ldf`), `ipiv`, `info` of the
ComplexF32 factorization, `anorm = ||A||_inf` (row sums of moduli) and the `iters` of the last `ldiv_mixed!`.
"""
mutable struct ComplexMixedLU
    A::Ptr{ComplexF64}
    n::Int
    lda::Int
    F32::Ptr{ComplexF32}
    ldf::Int
    ipiv::Ptr{Int64}
    info::BlasInt
    anorm::Float64
    iters::Int
end

"""
    lu_mixed(A::Ptr{ComplexF64}, n, lda, F32::Ptr{ComplexF32}, ldf, ipiv, pivot = Val(true)) -> ComplexMixedLU

The complex form of `lu_mixed` (LAPACK `zcgesv`'s scheme): a ComplexF32 copy of `A` is factored into the caller's `F32` (`n x ldf`,
row-major).  `A` is not modified.  A zero pivot of the ComplexF32 factorization is reported in `info`, never thrown.
"""
function lu_mixed(A::Ptr{ComplexF64}, n::Integer, lda::Integer, F32::Ptr{ComplexF32}, ldf::Integer, ipiv::Ptr{Int64}, pivot = Val(true))
    pivot = normalize_pivot(pivot)
    info, anorm = mixed_getrf_dev!(A, n, lda, F32, ldf, ipiv, pivot === Val(true))
    (pivot === Val(false) && NOPIVOT_NEGATIVE_INFO) && (info = -info)
    return ComplexMixedLU(A, Int(n), Int(lda), F32, Int(ldf), ipiv, info, anorm, 0)
end

"""
    ldiv_mixed!(X::Ptr{ComplexF64}, ldx, F::ComplexMixedLU, B::Ptr{ComplexF64}, ldb, nrhs; max_iter = 30) -> Bool

`X <- A \\ B` by ComplexF32 solves and ComplexF64 residuals; `false` means `X` must not be used (zero pivot or no convergence) and the
caller solves with the ComplexF64 factorization instead.
"""
function ldiv_mixed!(X::Ptr{ComplexF64}, ldx::Integer, F::ComplexMixedLU, B::Ptr{ComplexF64}, ldb::Integer, nrhs::Integer;
                     max_iter::Integer = 30)
    F.info == 0 || return false
    F.iters = mixed_getrs_dev!(F.A, F.n, nrhs, F.lda, F.F32, F.ldf, F.ipiv, F.anorm, B, ldb, X, ldx, max_iter)
    return F.iters >= 0
end

"""
    device_pointer(x) -> Ptr

The HBM address of a device array.  RFLUAMD does not depend on a GPU array package: the package that owns the array type adds the
method (for AMDGPU.jl: `RFLUAMD.device_pointer(x::ROCArray{T}) where {T} = Ptr{T}(UInt(pointer(x)))`).
"""
function device_pointer end

"""
    RF32MixedLUAMDFactorization(; pivot = Val(true), blocksize = 0, max_iter = 30)

LinearSolve.jl algorithm in the place of `RF32MixedLUFactorization`: Float32 factors, Float64 refinement, `cache.A` is NOT overwritten.
Serves device arrays (see `device_pointer`).  `ReturnCode.Failure` only when the Float64 fallback is singular as well.
"""
struct RF32MixedLUAMDFactorization{P}
    blocksize::Int
    max_iter::Int
    RF32MixedLUAMDFactorization(::Val{P}, blocksize::Integer = 0, max_iter::Integer = 30) where {P} = new{P}(Int(blocksize), Int(max_iter))
end
RF32MixedLUAMDFactorization(; pivot = Val(true), blocksize::Integer = 0, max_iter::Integer = 30) =
    RF32MixedLUAMDFactorization(normalize_pivot(pivot), blocksize, max_iter)

end # module
