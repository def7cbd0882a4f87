// complex.hpp -- the ComplexF64 / ComplexF32 path of librflu.so (DESIGN.md sections 4.5, 4.6): what complex_gemm.hip, complex.hip,
// complex_solve.hip, driver.cpp (the C ABI) and host_entry.cpp (the host-pointer entries) need from each other.
//
// A complex array crosses every boundary as R* (R = double / float) pointing at interleaved (re, im) pairs -- the storage of Julia's
// Complex{R} and numpy's complex128 / complex64 -- and every leading dimension counts COMPLEX elements.  Inside, the matrix lives in the
// library's row-major layout like the real types do: element (i, j) at R[2 * (i * ld + j)], ld a multiple of 8 complex elements.
// Everything here is an in-order launch on the handle's stream: no kernel of this path waits for another workgroup.
#pragma once
#include "rflu_internal.hpp"

namespace rflu {

constexpr int CLEAF = 32;   // leaf width of the complex recursion (columns per leaf panel, rows of a base triangle)
// The transposed / adjoint solve (complex_solve.hip).  Neither value is tuned and nobody has measured either: they are structural
// starting values.  8 is the pass width of the real path's solves, 256 rows keep the launch count near n / 64.
constexpr int CNARROW = 8;   // up to this many right-hand sides the solve works on B's columns in place (the few-right-hand-side path)
constexpr int CNB = 256;     // rows of a diagonal block of that path: one streaming launch and one one-workgroup launch per block

inline int64_t cworkspace_ld(int64_t n) { return (n + 7) / 8 * 8; }   // rows start on 64- / 128-byte boundaries

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
// the transposed solves: conj = 0 is LAPACK's 'T', conj = 1 its 'C'; everything else as the forward solve, in its words
inline int cgetrs_trans_check_args(int64_t n, int64_t nrhs, const void* F, int64_t lda, const void* B, int64_t ldb, int conj)
{
    if (conj != 0 && conj != 1) {
        set_error("complex getrs_trans: conj must be 0 (transpose) or 1 (adjoint), got %d", conj);
        return RFLU_ERR_ARG;
    }
    return cgetrs_check_args(n, nrhs, F, lda, B, ldb);
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

// complex.hip, for complex_solve.hip: the layout change out[r][c] = in[c][r] (conjugated when `conj`), and the recursive triangular
// solves B <- T^-1 B on row-major operands with the triangle's diagonal stored (`unit` false) or taken as 1 (`unit` true)
template <typename R>
int launch_ctranspose(Handle* h, int64_t rows_out, int64_t cols_out, const R* in, int64_t ld_in, R* out, int64_t ld_out, bool conj = false);
template <typename R>
int ctri_lower_rec(Handle* h, int64_t n, int64_t nrhs, const R* T, int64_t ldt, R* B, int64_t ldb, bool unit);
template <typename R>
int ctri_upper_rec(Handle* h, int64_t n, int64_t nrhs, const R* T, int64_t ldt, R* B, int64_t ldb, bool unit);

// complex_solve.hip: ldiv!(transpose(F), B) (conj = 0) and ldiv!(F', B) (conj = 1) on column-major device arrays; F is only read
template <typename R>
int cgetrs_trans_cm_dev(Handle* h, int64_t n, int64_t nrhs, const R* F, int64_t lda, const int64_t* ipiv, R* B, int64_t ldb, int conj);

// complex_solve.hip, for inverse.hip: x = P^T z, the interchanges of rows [0, rows) undone last first; element (k, c) at
// A[2 * (k * rs + c * cs)]
template <typename R>
int launch_claswp_rev(Handle* h, R* A, int64_t rs, int64_t cs, int64_t rows, int64_t ncols, const int64_t* ipiv);

// ---- complex mixed precision: ComplexF32 factors in the ROW-MAJOR layout, ComplexF64 refinement ----------------
// complex.hip: factor the n x n row-major F in place (cgetrf_rm with the info word zeroed before and copied back after; waits for the
// stream).  Pivot and zero-pivot rules are cgetrf_cm_dev's.
template <typename R>
int cgetrf_rm_dev(Handle* h, int64_t n, R* F, int64_t ldf, int64_t* ipiv, int pivot, int64_t* info);
// complex_solve.hip: B <- U^-1 L^-1 P B with W the row-major packed factors, no n x n copy.  csolve_fwd_narrow works on the columns of a
// column-major B (nrhs <= CNARROW), csolve_fwd_image on a row-major n x nrhs image X; neither waits for the stream.  cgetrs_fwd_rm_dev
// is the checked entry on a column-major B (any nrhs; wider blocks go through the image in Handle::rhs_work) and waits.
template <typename R>
int csolve_fwd_narrow(Handle* h, int64_t n, int nrhs, const R* W, int64_t ldw, const int64_t* ipiv, R* B, int64_t ldb);
template <typename R>
int csolve_fwd_image(Handle* h, int64_t n, int64_t nrhs, const R* W, int64_t ldw, const int64_t* ipiv, R* X, int64_t ldx);
template <typename R>
int cgetrs_fwd_rm_dev(Handle* h, int64_t n, int64_t nrhs, const R* W, int64_t ldw, const int64_t* ipiv, R* B, int64_t ldb);
// (the kernels of the refinement, real and complex: mixed.hip, declared in rflu_internal.hpp)

// the complex condition estimate (the norms and the vector kernels are condest.hip, declared in rflu_internal.hpp)
// batched_complex.hip: the whole estimator on a matrix held in LDS, one launch for n <= CBATCHED_MAX_DIM_CF64 / _CF32
template <typename R>
int launch_cgecon_batched(Handle* h, int norm, int64_t batch, int64_t n, const R* F, int64_t lda, int64_t strideF, int row_major,
                          const double* anorm, double* rcond);
// driver.cpp: rcond of column-major complex factors (rflu.h: COMPLEX NORMS, CONDITION); host_entry.cpp: the same from host factors
template <typename R>
int cgecon_dev(Handle* h, int norm, int64_t n, const R* F, int64_t lda, double anorm, double* rcond);
template <typename R>
int cgecon_host(Handle* h, int norm, int64_t n, const R* F, int64_t lda, double anorm, double* rcond);

// host_entry.cpp: caller-owned column-major host arrays; copied back only on success
template <typename R>
int cgetrf_host(Handle* h, int64_t m, int64_t n, R* A, int64_t lda, int64_t* ipiv, int pivot, int64_t* info);
template <typename R>
int cgetrs_host(Handle* h, int64_t n, int64_t nrhs, const R* F, int64_t lda, const int64_t* ipiv, R* B, int64_t ldb);
template <typename R>
int cgetrs_trans_host(Handle* h, int64_t n, int64_t nrhs, const R* F, int64_t lda, const int64_t* ipiv, R* B, int64_t ldb, int conj);

}  // namespace rflu
