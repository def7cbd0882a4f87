# LinearSolve.jl extension: RFLUAMDFactorization as a drop-in for RFLUFactorization (same cache protocol).
# LinearSolve's own `solve!(cache, ::RFLUFactorization{P,T})` does, in order:
#     fact, ipiv = cacheval; if cache.isfresh: resize ipiv; fact = RecursiveFactorization.lu!(A, ipiv, Val(P), Val(T), check = false);
#     cache.cacheval = (fact, ipiv); !issuccess(fact) -> ReturnCode.Failure; y = ldiv!(cache.u, fact, cache.b)
# (RecursiveFactorization README.md:36-37 names it; the call shape is src/lu.jl:97-130 with check = false).
module RFLUAMDLinearSolveExt

using LinearAlgebra
using LinearSolve
using RFLUAMD
using RFLUAMD: RFLUAMDFactorization, RF32MixedLUAMDFactorization

# the algorithm type takes part in LinearSolve's factorization machinery
LinearSolve.needs_concrete_A(::RFLUAMDFactorization) = true

function LinearSolve.init_cacheval(alg::RFLUAMDFactorization{P}, A, b, u, Pl, Pr, maxiters::Int, abstol, reltol,
                                   verbose, assumptions::LinearSolve.OperatorAssumptions) where {P}
    A isa AbstractMatrix || return nothing
    ipiv = Vector{LinearAlgebra.BlasInt}(undef, min(size(A)...))
    # a well-typed placeholder factorization, like LinearSolve's ArrayInterface.lu_instance
    fact = LinearAlgebra.LU(similar(A, 0, 0), similar(ipiv, 0), zero(LinearAlgebra.BlasInt))
    return (fact, ipiv)
end

function LinearSolve.solve!(cache::LinearSolve.LinearCache, alg::RFLUAMDFactorization{P}; kwargs...) where {P}
    A = convert(AbstractMatrix, cache.A)
    fact, ipiv = LinearSolve.@get_cacheval(cache, :RFLUAMDFactorization)
    if cache.isfresh
        if length(ipiv) != min(size(A)...)
            ipiv = Vector{LinearAlgebra.BlasInt}(undef, min(size(A)...))
        end
        fact = RFLUAMD.lu!(A, ipiv, Val(P), Val(false); check = false, blocksize = alg.blocksize)
        cache.cacheval = (fact, ipiv)
        if !LinearAlgebra.issuccess(fact)
            return SciMLBase.build_linear_solution(alg, cache.u, nothing, cache; retcode = ReturnCode.Failure)
        end
        cache.isfresh = false
    end
    y = RFLUAMD.ldiv!(LinearSolve.@get_cacheval(cache, :RFLUAMDFactorization)[1], copyto!(cache.u, cache.b))
    return SciMLBase.build_linear_solution(alg, y, nothing, cache; retcode = ReturnCode.Success)
end

# ---- RF32MixedLUAMDFactorization: Float32 factors + Float64 refinement on device arrays; cache.A stays as it is -------------------
# cacheval = (mixed, F32, ipiv, f64): the MixedLU, the buffers it points into, and the Float64 fallback factorization once one was needed.
LinearSolve.needs_concrete_A(::RF32MixedLUAMDFactorization) = true

function LinearSolve.init_cacheval(alg::RF32MixedLUAMDFactorization, A, b, u, Pl, Pr, maxiters::Int, abstol, reltol, verbose,
                                   assumptions::LinearSolve.OperatorAssumptions)
    return nothing
end

function LinearSolve.solve!(cache::LinearSolve.LinearCache, alg::RF32MixedLUAMDFactorization{P}; kwargs...) where {P}
    A = cache.A
    n = size(A, 1)
    if cache.isfresh
        F32 = similar(A, Float32, n, n)                      # row-major n x n, ldf = n
        ipiv = similar(A, Int64, n)
        mixed = GC.@preserve A F32 ipiv RFLUAMD.lu_mixed(RFLUAMD.device_pointer(A), n, stride(A, 2), RFLUAMD.device_pointer(F32), n,
                                                         P ? RFLUAMD.device_pointer(ipiv) : Ptr{Int64}(C_NULL), Val(P); blocksize = alg.blocksize)
        cache.cacheval = (mixed, F32, ipiv, nothing)
        cache.isfresh = false
    end
    mixed, F32, ipiv, f64 = cache.cacheval
    nrhs = size(cache.b, 2)
    ok = f64 === nothing && GC.@preserve A F32 ipiv cache RFLUAMD.ldiv_mixed!(RFLUAMD.device_pointer(cache.u), max(n, 1), mixed,
                                                                            RFLUAMD.device_pointer(cache.b), max(n, 1), nrhs; max_iter = alg.max_iter)
    if !ok   # zero pivot in Float32 or no convergence: the Float64 factorization of a COPY of A, kept for the solves that follow
        if f64 === nothing
            f64 = LinearAlgebra.lu!(copy(A), P ? RowMaximum() : NoPivot(); check = false)
            cache.cacheval = (mixed, F32, ipiv, f64)
        end
        if !LinearAlgebra.issuccess(f64)
            cache.isfresh = true
            return SciMLBase.build_linear_solution(alg, cache.u, nothing, cache; retcode = ReturnCode.Failure)
        end
        LinearAlgebra.ldiv!(cache.u, f64, cache.b)
    end
    return SciMLBase.build_linear_solution(alg, cache.u, nothing, cache; retcode = ReturnCode.Success)
end

end # module
