# Mirrors RecursiveFactorization's test/runtests.jl:14-68 (info equality with LAPACK, residual bound, solve check) through
# RFLUAMD; sizes from GPU_MIN_N up take the MI355X path (asserted through rflu_last_path).  Needs Julia + a gfx950 device.
using Test, LinearAlgebra, Random
using RFLUAMD
Random.seed!(12)
const baselu = LinearAlgebra.lu
function testlu(A, MF, BF, p)
    @test MF.info == BF.info
    iszero(MF.info) || return
    E = 20size(A, 1) * eps(real(one(float(first(A)))))
    @test norm(MF.L * MF.U - A[MF.p, :], Inf) < (p ? E : 10sqrt(E))
end
@testset "RFLUAMD lu / lu!" begin
    RFLUAMD.GPU_MIN_N[] = 64
    for _p in (true, false), T in (Float64, Float32), s in (64, 130, 300, 1000)
        for m in (s, s + 2)
            A = rand(T, s, m)
            _p || (A = A + T(10) * Matrix{T}(I, s, m))          # the reference's NoPivot inputs are diagonally shifted
            MF = RFLUAMD.lu(A, Val(_p))
            RFLUAMD.available() && @test RFLUAMD.last_path() in (1, 3, 4)
            testlu(A, MF, baselu(A, _p ? RowMaximum() : NoPivot()), _p)
            At = permutedims(A)
            testlu(At, parent(RFLUAMD.lu(At', Val(_p))), baselu(At, _p ? RowMaximum() : NoPivot()), _p)
        end
    end
    A = rand(300, 300); A[:, 17] .= 0
    @test RFLUAMD.lu(A; check = false).info == baselu(A; check = false).info
    ipiv = fill(typemax(Int64) - 7, 300)
    F = RFLUAMD.lu!(rand(300, 300) + 10I, ipiv, Val(false), Val(false))
    @test ipiv == 1:300
end
@testset "RFLUAMD ldiv! with the adjoint / transposed factorization" begin
    RFLUAMD.GPU_MIN_N[] = 64
    for _p in (true, false), T in (Float64, Float32), n in (64, 65, 300, 1000)
        A = rand(T, n, n) + T(10) * I
        F = RFLUAMD.lu(A, Val(_p))
        b = rand(T, n); B = rand(T, n, 3)
        for Ft in (F', transpose(F))
            x = RFLUAMD.ldiv!(Ft, copy(b))
            @test norm(A' * x - b) < 1000n * eps(T)          # the reference's bound for ldiv!, test/runtests.jl:126-128
            X = RFLUAMD.ldiv!(Ft, copy(B))
            @test norm(A' * X - B) < 1000n * eps(T)
        end
    end
end
@testset "RFLUAMD ldiv! with the adjoint / transposed COMPLEX factorization (two different solves)" begin
    RFLUAMD.GPU_MIN_N[] = 64
    for _p in (true, false), T in (ComplexF64, ComplexF32), n in (64, 65, 300, 1000)
        A = rand(T, n, n) + T(10) * I
        F = RFLUAMD.lu(A, Val(_p))
        b = rand(T, n); B = rand(T, n, 9)                     # a vector (few-right-hand-side path) and 9 columns (GEMM path)
        for (Ft, opA) in ((F', A'), (transpose(F), transpose(A)))
            x = RFLUAMD.ldiv!(Ft, copy(b))
            @test norm(opA * x - b) < 1000n * eps(real(T))
            X = RFLUAMD.ldiv!(Ft, copy(B))
            @test norm(opA * X - B) < 1000n * eps(real(T))
        end
    end
end
@testset "RFLUAMD inv! / det / logabsdet from the factors" begin
    RFLUAMD.GPU_MIN_N[] = 64
    for _p in (true, false), T in (Float64, Float32), n in (64, 65, 300, 1000)
        A = rand(T, n, n) + T(10) * I
        F = RFLUAMD.lu(A, Val(_p))
        la, sg = RFLUAMD.logabsdet(F)
        la0, sg0 = logabsdet(Float64.(A))
        @test sg == sg0 && abs(la - la0) <= 8n * eps(T)
        @test RFLUAMD.det(F) ≈ det(F)
        X = RFLUAMD.inv!(F)                                   # F is invalid from here on
        @test opnorm(A * X - I, 1) <= n * eps(T) * opnorm(A, 1) * opnorm(X, 1)
        @test opnorm(X * A - I, 1) <= n * eps(T) * opnorm(A, 1) * opnorm(X, 1)
    end
    S = rand(100, 100); S[:, 40] .= 0
    @test_throws SingularException RFLUAMD.inv!(RFLUAMD.lu(S; check = false))
end
@testset "RFLUAMD complex inv! / det / logabsdet from the factors" begin
    RFLUAMD.GPU_MIN_N[] = 64
    for _p in (true, false), T in (ComplexF64, ComplexF32), n in (64, 65, 300, 1000)
        R = real(T)
        A = rand(T, n, n) .- T(0.5 + 0.5im) + T(n) * I
        F = RFLUAMD.lu(A, Val(_p))
        la, sg = RFLUAMD.logabsdet(F)
        la0, sg0 = logabsdet(ComplexF64.(A))
        @test abs(sg - sg0) <= 16n * eps(R) && abs(la - la0) <= 8n * eps(R)
        @test RFLUAMD.det(F) ≈ det(F)
        X = RFLUAMD.inv!(F)                                   # F is invalid from here on
        @test opnorm(A * X - I, 1) <= n * eps(R) * opnorm(A, 1) * opnorm(X, 1)
        @test opnorm(X * A - I, 1) <= n * eps(R) * opnorm(A, 1) * opnorm(X, 1)
    end
    S = rand(ComplexF64, 130, 130); S[:, 70] .= 0
    @test_throws SingularException RFLUAMD.inv!(RFLUAMD.lu(S; check = false))
end
# The batched entries take DEVICE pointers, so this block needs AMDGPU.jl for the buffers (not a dependency of the package: skipped
# when it is not installed).  4096 systems of order 32, packed column-major: pivots and info against LAPACK, the reference's solve bound.
if Base.find_package("AMDGPU") !== nothing
    @eval using AMDGPU
    @testset "RFLUAMD batched getrf / getrs ($T)" for T in (Float64, Float32)
        n, batch = 32, 4096
        A = rand(T, n, n, batch); A[:, 5, 7] .= 0              # matrix 7 is singular: info 5, alone
        b = rand(T, n, batch)
        dA, dB = ROCArray(A), ROCArray(b)
        dipiv, dinfo = ROCArray(zeros(Int64, n, batch)), ROCArray(fill(Int64(-1), batch))
        GC.@preserve dA dB dipiv dinfo begin
            RFLUAMD.getrf_batched_dev!(Ptr{T}(UInt(pointer(dA))), batch, n, n, n, n * n, false, Ptr{Int64}(UInt(pointer(dipiv))), n, true,
                                       Ptr{Int64}(UInt(pointer(dinfo))))
            @test RFLUAMD.last_path() == 5
            RFLUAMD.getrs_batched_dev!(Ptr{T}(UInt(pointer(dA))), batch, n, 1, n, n * n, false, Ptr{Int64}(UInt(pointer(dipiv))), n,
                                       Ptr{T}(UInt(pointer(dB))), n, n, false)
        end
        ipiv, info, x = Array(dipiv), Array(dinfo), Array(dB)
        @test info[7] == 5 && count(!iszero, info) == 1
        for k in (1, 2, 1000, batch)
            @test ipiv[:, k] == baselu(A[:, :, k]).ipiv
            @test norm(A[:, :, k] * x[:, k] - b[:, k]) < 1000n * eps(T) * norm(A[:, :, k]) * norm(x[:, k])
        end
    end
    # complex batches: info of a singular matrix stays its own; 'N', 'T' and 'C' each solve their own operator
    @testset "RFLUAMD complex batched getrf / getrs ($T)" for T in (ComplexF64, ComplexF32)
        n, batch = 32, 1024
        A = rand(T, n, n, batch); A[:, 5, 7] .= 0
        b = rand(T, n, batch)
        dA = ROCArray(A)
        dipiv, dinfo = ROCArray(zeros(Int64, n, batch)), ROCArray(fill(Int64(-1), batch))
        GC.@preserve dA dipiv dinfo begin
            RFLUAMD.getrf_batched_dev!(Ptr{T}(UInt(pointer(dA))), batch, n, n, n, n * n, false, Ptr{Int64}(UInt(pointer(dipiv))), n, true,
                                       Ptr{Int64}(UInt(pointer(dinfo))))
            @test RFLUAMD.last_path() == 5
        end
        info = Array(dinfo)
        @test info[7] == 5 && count(!iszero, info) == 1
        for (trans, op) in (('N', identity), ('T', transpose), ('C', adjoint))
            dB = ROCArray(b)
            GC.@preserve dA dB dipiv begin
                RFLUAMD.getrs_batched_dev!(Ptr{T}(UInt(pointer(dA))), batch, n, 1, n, n * n, false, Ptr{Int64}(UInt(pointer(dipiv))), n,
                                           Ptr{T}(UInt(pointer(dB))), n, n, trans)
            end
            x = Array(dB)
            for k in (1, 2, 1000, batch)
                M = op(A[:, :, k])
                @test norm(M * x[:, k] - b[:, k]) < 1000n * eps(real(T)) * norm(M) * norm(x[:, k])
            end
        end
    end
    # complex batched inverse: one launch, the three letters, a singular matrix alone with its info
    @testset "RFLUAMD complex batched getri ($T)" for T in (ComplexF64, ComplexF32)
        n, batch = 32, 1024
        A = rand(T, n, n, batch); A[:, 5, 7] .= 0
        dA, dX = ROCArray(A), ROCArray(zeros(T, n, n, batch))
        dipiv, dinfo = ROCArray(zeros(Int64, n, batch)), ROCArray(fill(Int64(-1), batch))
        GC.@preserve dA dipiv dinfo begin
            RFLUAMD.getrf_batched_dev!(Ptr{T}(UInt(pointer(dA))), batch, n, n, n, n * n, false, Ptr{Int64}(UInt(pointer(dipiv))), n, true,
                                       Ptr{Int64}(UInt(pointer(dinfo))))
        end
        F = Array(dA)
        for (trans, op) in (('N', identity), ('T', transpose), ('C', adjoint))
            GC.@preserve dA dX dipiv dinfo begin
                RFLUAMD.getri_batched_dev!(Ptr{T}(UInt(pointer(dX))), n, n * n, Ptr{T}(UInt(pointer(dA))), batch, n, n, n * n, false,
                                           Ptr{Int64}(UInt(pointer(dipiv))), n, Ptr{Int64}(UInt(pointer(dinfo))), trans)
                @test RFLUAMD.last_path() == 5
            end
            X, info = Array(dX), Array(dinfo)
            @test info[7] == 5 && count(!iszero, info) == 1
            @test !all(isfinite, X[:, :, 7])
            @test Array(dA) == F                                   # the factors are only read
            for k in (1, 2, 1000, batch)
                M = op(A[:, :, k])
                @test all(isfinite, X[:, :, k])
                @test opnorm(M * X[:, :, k] - I, 1) < 1000n * eps(real(T)) * opnorm(M, 1) * opnorm(X[:, :, k], 1)
            end
        end
    end
    # mixed precision: Float32 factors, Float64 refinement; A and b untouched, dsgesv's rule met, the residual kernel alone
    @testset "RFLUAMD mixed-precision solve" begin
        n, nrhs = 1000, 9
        A, B = rand(n, n), rand(n, nrhs)
        dA, dB, dX, dR = ROCArray(A), ROCArray(B), ROCArray(zeros(n, nrhs)), ROCArray(zeros(n, nrhs))
        dF, dipiv = ROCArray(zeros(Float32, n, n)), ROCArray(zeros(Int64, n))
        p(x::ROCArray{T}) where {T} = Ptr{T}(UInt(pointer(x)))
        GC.@preserve dA dB dX dR dF dipiv begin
            F = RFLUAMD.lu_mixed(p(dA), n, n, p(dF), n, p(dipiv))
            @test F.info == 0 && F.anorm == maximum(sum(abs, A; dims = 2))
            @test RFLUAMD.ldiv_mixed!(p(dX), n, F, p(dB), n, nrhs) && 1 <= F.iters <= 10
            RFLUAMD.residual_dev!(p(dR), n, p(dA), n, nrhs, n, p(dX), n, p(dB), n)
        end
        X, R = Array(dX), Array(dR)
        @test Array(dA) == A && Array(dB) == B
        for k in 1:nrhs
            @test norm(B[:, k] - A * X[:, k], Inf) <= norm(X[:, k], Inf) * opnorm(A, Inf) * eps() * sqrt(n)
        end
        @test maximum(abs, R - (B - A * X)) <= (n + 2) * eps() * maximum(abs.(A) * abs.(X) + abs.(B))
    end
end
