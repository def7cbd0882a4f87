// complex.hpp -- the ComplexF64 / ComplexF32 path of librflu.so: what complex_gemm.hip, complex.hip, driver.cpp
// (the C ABI) and host_entry.cpp (the host-pointer entries) need from each other.
//
// A complex array crosses every boundary as R* (R = double / float) pointing at interleaved (re, im) pairs -- the storage of Julia's
// Complex{R} and numpy's complex128 / complex64 -- and every leading dimension counts COMPLEX elements.  Inside, the matrix lives in the
// library's row-major layout like the real types do: element (i, j) at R[2 * (i * ld + j)], ld a multiple of 8 complex elements.
// Everything here is an in-order launch on the handle's stream: no kernel of this path waits for another workgroup.
#pragma once
#include "rflu_internal.hpp"

namespace rflu {

constexpr int CLEAF = 32;   // leaf width of the complex recursion (columns per leaf panel, rows of a base triangle)

// the argument rules of the getrf / getrs entries, one copy for the device entries (complex.hip) and the host entries (host_entry.cpp)
inline int cgetrf_check_args(int64_t m, int64_t n, const void* A, int64_t lda, const int64_t* ipiv, int pivot, const int64_t* info)
{
    if (m < 0 || n < 0 || lda < (m > 1 ? m : 1) || info == nullptr || (m > 0 && n > 0 && A == nullptr)) {
        set_error("complex getrf: bad arguments m=%lld n=%lld lda=%lld (or a null pointer)", (long long)m, (long long)n, (long long)lda);
        return RFLU_ERR_ARG;
    }
    if (pivot && ipiv == nullptr && m > 0 && n > 0) {
        set_error("complex getrf: ipiv may be NULL only with pivot == 0 (NotIPIV)");
        return RFLU_ERR_ARG;
    }
    return RFLU_OK;
}
inline int cgetrs_check_args(int64_t n, int64_t nrhs, const void* F, int64_t lda, const void* B, int64_t ldb)
{
    const int64_t n1 = n > 1 ? n : 1;
    if (n < 0 || nrhs < 0 || lda < n1 || ldb < n1 || (n > 0 && nrhs > 0 && (F == nullptr || B == nullptr))) {
        set_error("complex getrs: bad arguments n=%lld nrhs=%lld lda=%lld ldb=%lld (or a null pointer)", (long long)n, (long long)nrhs,
                  (long long)lda, (long long)ldb);
        return RFLU_ERR_ARG;
    }
    return RFLU_OK;
}

// complex_gemm.hip: C <- C - A * B, all row-major complex; A is M x K (lda), B is K x N (ldb), C is M x N (ldc)
template <typename R>
int launch_cgemm(Handle* h, int64_t M, int64_t N, int64_t K, const R* A, int64_t lda, const R* B, int64_t ldb, R* C, int64_t ldc);

// complex.hip: the device entries (column-major, as LinearAlgebra.LU holds them) and the stand-alone GEMM of the C ABI
template <typename R>
int cgetrf_cm_dev(Handle* h, int64_t m, int64_t n, R* A, int64_t lda, int64_t* ipiv, int pivot, int64_t* info);
template <typename R>
int cgetrs_cm_dev(Handle* h, int64_t n, int64_t nrhs, const R* F, int64_t lda, const int64_t* ipiv, R* B, int64_t ldb);
template <typename R>
int cgemm_public(Handle* h, int64_t M, int64_t N, int64_t K, const R* A, int64_t lda, const R* B, int64_t ldb, R* C, int64_t ldc);

// host_entry.cpp: caller-owned column-major host arrays; copied back only on success
template <typename R>
int cgetrf_host(Handle* h, int64_t m, int64_t n, R* A, int64_t lda, int64_t* ipiv, int pivot, int64_t* info);
template <typename R>
int cgetrs_host(Handle* h, int64_t n, int64_t nrhs, const R* F, int64_t lda, const int64_t* ipiv, R* B, int64_t ldb);

}  // namespace rflu
