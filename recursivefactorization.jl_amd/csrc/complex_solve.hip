// complex_solve.hip -- ldiv!(transpose(F), B) and ldiv!(F', B) for ComplexF64 / ComplexF32 factors:
// B <- P^T L^-T U^-T B (LAPACK getrs 'T') and B <- P^T L^-H U^-H B ('C').  F is column-major and only read, in place: a column-major F
// read as a row-major array with ld = lda IS V = F^T, whose lower triangle with the diagonal is U^T and whose strict upper triangle is
// L^T (unit diagonal).  So: a forward solve with the lower, stored-diagonal triangle of V, a backward solve with its upper, unit one,
// then the interchanges undone last first.  Two paths:
//   nrhs <= CNARROW: B is not copied, a right-hand side is a contiguous column of it.  A left-looking loop over diagonal blocks of CNB
//                    rows, per block one streaming launch (cgemv_sub_kernel) and one one-workgroup launch (ctrsv_block_kernel).
//                    The adjoint conjugates V as it is loaded (CONJ).
//   nrhs >  CNARROW: the structure of the forward solve without its n x n copy: the row-major image of B, the two recursions of
//                    complex.hip on V with the complex GEMM in between, the layout change back.  The GEMM has no conjugation flag,
//                    so the adjoint conjugates B on its way in and out instead: A^H x = b  <=>  A^T conj(x) = conj(b).
// Every kernel is an ordinary in-order launch on the handle's stream; none waits for another workgroup.
#include <algorithm>
#include <cstdint>
#include <cstdlib>

#include "complex_dev.hpp"

namespace rflu {

template <typename R>
__device__ __forceinline__ Cx<R> cload(const R* p) { return Cx<R>{p[0], p[1]}; }

// ---- Y[i, r] -= sum over k in [k0, k1) of V[i, k] * X[k, r], for the rows i0 + blockIdx.x and r < nrhs <= CNARROW ------------------------
// V row-major (ld): row i is column i of F, contiguous.  X and Y are columns of B (column-major, ldb): X[k, r] = B[k + r * ldb].
// One workgroup of four waves per row.  The k range is cut into chunks of 64 * EPL elements (EPL = elements per 16 bytes); chunk c goes
// to wave c mod 4, lane l of it takes the EPL consecutive elements from l * EPL on, so consecutive lanes sit on consecutive k and every
// element of the band is read once.  A lane adds its products in ascending k into up to CNARROW running sums; a wave folds its 64 lanes
// with a shuffle tree, the four waves' sums are added in wave order by one thread per right-hand side, which is also the only writer of
// Y[i, r].  Which lane sums which k is fixed by the chunking alone: the 16-byte load (taken when the row's first element sits on a
// 16-byte boundary) and the element-by-element load feed the same registers, so the result does not depend on the alignment of F or
// on lda, and there is no atomic and no shared word that two threads modify.
constexpr int CGEMV_WAVES = 4;

template <typename R, bool CONJ>
__global__ void __launch_bounds__(64 * CGEMV_WAVES) cgemv_sub_kernel(const R* __restrict__ V, int64_t ld, int64_t i0, int64_t k0, int64_t k1,
                                                                      int nrhs, R* B, int64_t ldb)
{
    constexpr int EPL = 16 / (2 * (int)sizeof(R));
    constexpr int CHUNK = 64 * EPL;
    __shared__ R red[CGEMV_WAVES][CNARROW][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t i = i0 + blockIdx.x;
    const R* row = V + 2 * (i * ld);
    const bool vec = (reinterpret_cast<uintptr_t>(row + 2 * k0) & 15) == 0;
    Cx<R> acc[CNARROW];
#pragma unroll
    for (int r = 0; r < CNARROW; ++r) acc[r] = Cx<R>{R(0), R(0)};
    for (int64_t c = k0 + (int64_t)wave * CHUNK; c < k1; c += (int64_t)CGEMV_WAVES * CHUNK) {
        const int64_t k = c + (int64_t)lane * EPL;
        const int64_t left = k1 - k;
        R w[2 * EPL];
        if (left >= EPL && vec) {
            if constexpr (sizeof(R) == 8) {
                const double2 t = *reinterpret_cast<const double2*>(row + 2 * k);
                w[0] = t.x; w[1] = t.y;
            } else {
                const float4 t = *reinterpret_cast<const float4*>(row + 2 * k);
                w[0] = t.x; w[1] = t.y; w[2] = t.z; w[3] = t.w;
            }
        } else {
#pragma unroll
            for (int e = 0; e < EPL; ++e) {
                const bool in = e < left;
                w[2 * e] = in ? row[2 * (k + e)] : R(0);
                w[2 * e + 1] = in ? row[2 * (k + e) + 1] : R(0);
            }
        }
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
            if (e < left) {
                const Cx<R> v{w[2 * e], CONJ ? -w[2 * e + 1] : w[2 * e + 1]};
#pragma unroll
                for (int r = 0; r < CNARROW; ++r)
                    if (r < nrhs) acc[r] = cfma(v, cload(B + 2 * ((int64_t)r * ldb + k + e)), acc[r]);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < CNARROW; ++r) {
        if (r < nrhs) {   // (uniform over the workgroup)
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                acc[r].re += __shfl_down(acc[r].re, off);
                acc[r].im += __shfl_down(acc[r].im, off);
            }
            if (lane == 0) { red[wave][r][0] = acc[r].re; red[wave][r][1] = acc[r].im; }
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < nrhs) {
        const int r = threadIdx.x;
        R sre = red[0][r][0], sim = red[0][r][1];
#pragma unroll
        for (int q = 1; q < CGEMV_WAVES; ++q) { sre += red[q][r][0]; sim += red[q][r][1]; }
        R* y = B + 2 * ((int64_t)r * ldb + i);
        y[0] -= sre;
        y[1] -= sim;
    }
}

// ---- one diagonal block: Y <- T^-1 Y, T the nb x nb (nb <= CNB) triangle of V at `T`, Y the nb rows of B from `Y` on, ONE workgroup --------
// In steps of 32 rows (ascending for the lower triangle, descending for the upper one):
//   1. the step's 32 x 32 triangle goes from global memory (L2 after the first touch) into LDS, 32 consecutive lanes on one row;
//   2. thread (l, r) = (tid % 32, tid / 32) owns row l of right-hand side r: for each column j in turn the owner of row j divides by the
//      diagonal (not UNIT), the solved component is broadcast over the 32 lanes and the others subtract their multiple of it;
//   3. the block's other rows that still wait for these 32 components take Y[i, r] -= sum_j T[i, j] x[j, r]: 64 rows at a time go through
//      LDS (consecutive lanes on consecutive k of a row again), thread (a, q) = (tid % 64, tid / 64) then owns row a for the right-hand
//      sides q and q + 4, summing j in ascending order.
// Only __syncthreads() orders the steps; Y lives in global memory and every element has one writer per phase.  A zero u_ii gives
// Inf / NaN.  CONJ conjugates T as it is loaded.
constexpr int CTRSV_THREADS = 256;
static_assert(CNARROW * 32 == CTRSV_THREADS && CNARROW == 8, "phase 2 gives each right-hand side 32 lanes, phase 3 pairs r with r + 4");

template <typename R, bool UPPER, bool UNIT, bool CONJ>
__global__ void __launch_bounds__(CTRSV_THREADS) ctrsv_block_kernel(const R* __restrict__ T, int64_t ld, int nb, int nrhs, R* Y, int64_t ldb)
{
    __shared__ R Tp[32][33][2];
    __shared__ R Pp[64][33][2];
    __shared__ R xs[32][CNARROW][2];
    const int tid = threadIdx.x;
    const int nsteps = (nb + 31) / 32;
    for (int q = 0; q < nsteps; ++q) {
        const int s = 32 * (UPPER ? nsteps - 1 - q : q);
        const int jn = nb - s < 32 ? nb - s : 32;
        for (int e = tid; e < 32 * 32; e += CTRSV_THREADS) {
            const int a = e >> 5, b = e & 31;
            if (a < jn && b < jn) {
                const R* p = T + 2 * ((int64_t)(s + a) * ld + s + b);
                Tp[a][b][0] = p[0];
                Tp[a][b][1] = CONJ ? -p[1] : p[1];
            }
        }
        __syncthreads();
        {
            const int l = tid & 31, r = tid >> 5;
            const bool active = r < nrhs && l < jn;
            R* yp = Y + 2 * ((int64_t)r * ldb + s + l);
            Cx<R> y = active ? cload(yp) : Cx<R>{R(0), R(0)};
            for (int jj = 0; jj < jn; ++jj) {
                const int j = UPPER ? jn - 1 - jj : jj;
                if (!UNIT && l == j) y = cdiv(y, Cx<R>{Tp[j][j][0], Tp[j][j][1]});
                const Cx<R> xj{__shfl(y.re, j, 32), __shfl(y.im, j, 32)};
                if ((UPPER ? l < j : l > j) && l < jn) y = cfma(Cx<R>{-Tp[l][j][0], -Tp[l][j][1]}, xj, y);
            }
            if (active) {
                yp[0] = y.re;
                yp[1] = y.im;
                xs[l][r][0] = y.re;
                xs[l][r][1] = y.im;
            }
        }
        __syncthreads();
        const int u0 = UPPER ? 0 : s + 32, u1 = UPPER ? s : nb;
        for (int g = u0; g < u1; g += 64) {
            for (int e = tid; e < 64 * 32; e += CTRSV_THREADS) {
                const int a = e >> 5, b = e & 31;
                if (g + a < u1 && b < jn) {
                    const R* p = T + 2 * ((int64_t)(g + a) * ld + s + b);
                    Pp[a][b][0] = p[0];
                    Pp[a][b][1] = CONJ ? -p[1] : p[1];
                }
            }
            __syncthreads();
            const int a = tid & 63, i = g + a;
            if (i < u1) {
#pragma unroll
                for (int half = 0; half < 2; ++half) {
                    const int r = (tid >> 6) + 4 * half;
                    if (r < nrhs) {
                        Cx<R> acc{R(0), R(0)};
                        for (int j = 0; j < jn; ++j) acc = cfma(Cx<R>{Pp[a][j][0], Pp[a][j][1]}, Cx<R>{xs[j][r][0], xs[j][r][1]}, acc);
                        R* yp = Y + 2 * ((int64_t)r * ldb + i);
                        yp[0] -= acc.re;
                        yp[1] -= acc.im;
                    }
                }
            }
            __syncthreads();
        }
    }
}

// ---- x = P^T z: the interchanges k <-> ipiv[k] - 1 undone last first, k = k1 - 1 ... k0 (ipiv repeats targets, so the order matters) -----
// One thread per column; element (k, c) sits at A[2 * (k * rs + c * cs)]: (ld, 1) walks a row-major image of B, (1, ldb) B itself.
template <typename R>
__global__ void __launch_bounds__(256) claswp_rev_kernel(R* __restrict__ A, int64_t rs, int64_t cs, int64_t rows, int64_t ncols,
                                                          const int64_t* __restrict__ ipiv, int64_t k0, int64_t k1)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= ncols) return;
    R* col = A + 2 * (c * cs);
    for (int64_t k = k1 - 1; k >= k0; --k) {
        const int64_t p = ipiv[k] - 1;
        if (p != k && p >= 0 && p < rows) {   // (a caller's ipiv outside the matrix is not followed)
            R* a = col + 2 * k * rs;
            R* b = col + 2 * p * rs;
            const R ar = a[0], ai = a[1], br = b[0], bi = b[1];
            a[0] = br; a[1] = bi;
            b[0] = ar; b[1] = ai;
        }
    }
}

template <typename R>
int launch_claswp_rev(Handle* h, R* A, int64_t rs, int64_t cs, int64_t rows, int64_t ncols, const int64_t* ipiv)
{
    ProfScope ps(h, RFLU_K_LASWP, 8.0 * sizeof(R) * (double)ncols * (double)rows);
    hipLaunchKernelGGL(claswp_rev_kernel<R>, dim3((unsigned)((ncols + 255) / 256)), dim3(256), 0, h->stream, A, rs, cs, rows, ncols, ipiv,
                       (int64_t)0, rows);
    RFLU_HIP(hipGetLastError());
    return RFLU_OK;
}

template <typename R>
static int launch_cgemv_sub(Handle* h, const R* V, int64_t ld, int64_t i0, int64_t rows, int64_t k0, int64_t k1, int nrhs, R* B, int64_t ldb,
                            bool conj)
{
    if (rows <= 0 || k1 <= k0) return RFLU_OK;
    ProfScope ps(h, RFLU_K_TRSM, 8.0 * (double)rows * (double)(k1 - k0) * nrhs);
    const dim3 grid((unsigned)rows), block(64 * CGEMV_WAVES);
    if (conj) hipLaunchKernelGGL((cgemv_sub_kernel<R, true>), grid, block, 0, h->stream, V, ld, i0, k0, k1, nrhs, B, ldb);
    else hipLaunchKernelGGL((cgemv_sub_kernel<R, false>), grid, block, 0, h->stream, V, ld, i0, k0, k1, nrhs, B, ldb);
    RFLU_HIP(hipGetLastError());
    return RFLU_OK;
}

// lower with the stored diagonal (U^T, forward) or upper with a unit one (L^T, backward): the two kinds this solve needs
template <typename R, bool UPPER>
static int launch_ctrsv_block(Handle* h, const R* T, int64_t ld, int64_t nb, int nrhs, R* Y, int64_t ldb, bool conj)
{
    ProfScope ps(h, RFLU_K_TRSM, 4.0 * (double)nb * nb * nrhs);
    const dim3 grid(1), block(CTRSV_THREADS);
    if (conj) hipLaunchKernelGGL((ctrsv_block_kernel<R, UPPER, UPPER, true>), grid, block, 0, h->stream, T, ld, (int)nb, nrhs, Y, ldb);
    else hipLaunchKernelGGL((ctrsv_block_kernel<R, UPPER, UPPER, false>), grid, block, 0, h->stream, T, ld, (int)nb, nrhs, Y, ldb);
    RFLU_HIP(hipGetLastError());
    return RFLU_OK;
}

// the two thresholds; an experiments build (RFLU_EXPERIMENTS) reads them from the environment at every call so that
// scripts/microbench_complex_solve.py can sweep them -- the default build has the constants and nothing else
static int64_t narrow_limit()
{
#ifdef RFLU_EXPERIMENTS
    if (const char* e = std::getenv("RFLU_CNARROW")) return std::min<int64_t>(std::max<int64_t>(std::atoll(e), 0), CNARROW);
#endif
    return CNARROW;
}
static int64_t block_rows()
{
#ifdef RFLU_EXPERIMENTS
    if (const char* e = std::getenv("RFLU_CNB")) return std::min<int64_t>(std::max<int64_t>(std::atoll(e) / 32 * 32, 32), CNB);
#endif
    return CNB;
}

template <typename R>
static int csolve_narrow(Handle* h, int64_t n, int nrhs, const R* V, int64_t ld, const int64_t* ipiv, R* B, int64_t ldb, bool conj)
{
    const int64_t cnb = block_rows();
    for (int64_t j0 = 0; j0 < n; j0 += cnb) {   // U^T y = b, top down; the band left of the block holds what is already solved
        const int64_t nb = std::min(cnb, n - j0);
        RFLU_TRY(launch_cgemv_sub<R>(h, V, ld, j0, nb, 0, j0, nrhs, B, ldb, conj));
        RFLU_TRY((launch_ctrsv_block<R, false>(h, V + 2 * (j0 * ld + j0), ld, nb, nrhs, B + 2 * j0, ldb, conj)));
    }
    for (int64_t j0 = (n - 1) / cnb * cnb; j0 >= 0; j0 -= cnb) {   // L^T z = y, bottom up; the band right of the block
        const int64_t nb = std::min(cnb, n - j0);
        RFLU_TRY(launch_cgemv_sub<R>(h, V, ld, j0, nb, j0 + nb, n, nrhs, B, ldb, conj));
        RFLU_TRY((launch_ctrsv_block<R, true>(h, V + 2 * (j0 * ld + j0), ld, nb, nrhs, B + 2 * j0, ldb, conj)));
    }
    if (ipiv) RFLU_TRY(launch_claswp_rev<R>(h, B, 1, ldb, n, nrhs, ipiv));
    return RFLU_OK;
}

template <typename R>
static int csolve_wide(Handle* h, int64_t n, int64_t nrhs, const R* V, int64_t ld, const int64_t* ipiv, R* B, int64_t ldb, bool conj)
{
    const int64_t ldx = cworkspace_ld(nrhs);
    RFLU_TRY(ensure_buffer(&h->rhs_work, &h->rhs_work_bytes, (size_t)n * (size_t)ldx * 2 * sizeof(R)));
    R* X = static_cast<R*>(h->rhs_work);
    RFLU_TRY(launch_ctranspose<R>(h, n, nrhs, B, ldb, X, ldx, conj));
    RFLU_TRY(ctri_lower_rec<R>(h, n, nrhs, V, ld, X, ldx, false));
    RFLU_TRY(ctri_upper_rec<R>(h, n, nrhs, V, ld, X, ldx, true));
    if (ipiv) RFLU_TRY(launch_claswp_rev<R>(h, X, ldx, 1, n, nrhs, ipiv));
    return launch_ctranspose<R>(h, nrhs, n, X, ldx, B, ldb, conj);
}

template <typename R>
int cgetrs_trans_cm_dev(Handle* h, int64_t n, int64_t nrhs, const R* F, int64_t lda, const int64_t* ipiv, R* B, int64_t ldb, int conj)
{
    RFLU_TRY(cgetrs_trans_check_args(n, nrhs, F, lda, B, ldb, conj));
    if (n == 0 || nrhs == 0) return RFLU_OK;
    if (nrhs <= narrow_limit()) RFLU_TRY(csolve_narrow<R>(h, n, (int)nrhs, F, lda, ipiv, B, ldb, conj != 0));
    else RFLU_TRY(csolve_wide<R>(h, n, nrhs, F, lda, ipiv, B, ldb, conj != 0));
    RFLU_HIP(hipStreamSynchronize(h->stream));
    return RFLU_OK;
}

// ---- the forward solve on ROW-MAJOR factors: B <- U^-1 L^-1 P B, W = the packed L\U as cgetrf_rm leaves it ------
// The same two paths with the other two triangle kinds: the lower triangle of W is L (unit), its upper one U (stored diagonal), and a row
// of W is contiguous like a row of V above.  Nothing is conjugated.  The interchanges come first and ascend.

// x = P b: the interchanges k <-> ipiv[k] - 1 applied first first, k = k0 ... k1 - 1; claswp_rev_kernel's addressing, claswp_kernel's order
template <typename R>
__global__ void __launch_bounds__(256) claswp_fwd_kernel(R* __restrict__ A, int64_t rs, int64_t cs, int64_t rows, int64_t ncols,
                                                          const int64_t* __restrict__ ipiv, int64_t k0, int64_t k1)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= ncols) return;
    R* col = A + 2 * (c * cs);
    for (int64_t k = k0; k < k1; ++k) {
        const int64_t p = ipiv[k] - 1;
        if (p != k && p >= 0 && p < rows) {   // (a caller's ipiv outside the matrix is not followed)
            R* a = col + 2 * k * rs;
            R* b = col + 2 * p * rs;
            const R ar = a[0], ai = a[1], br = b[0], bi = b[1];
            a[0] = br; a[1] = bi;
            b[0] = ar; b[1] = ai;
        }
    }
}

template <typename R>
static int launch_claswp_fwd(Handle* h, R* A, int64_t rs, int64_t cs, int64_t rows, int64_t ncols, const int64_t* ipiv)
{
    ProfScope ps(h, RFLU_K_LASWP, 8.0 * sizeof(R) * (double)ncols * (double)rows);
    hipLaunchKernelGGL(claswp_fwd_kernel<R>, dim3((unsigned)((ncols + 255) / 256)), dim3(256), 0, h->stream, A, rs, cs, rows, ncols, ipiv,
                       (int64_t)0, rows);
    RFLU_HIP(hipGetLastError());
    return RFLU_OK;
}

// lower with a unit diagonal (L, forward) or upper with the stored one (U, backward)
template <typename R, bool UPPER>
static int launch_ctrsv_block_fwd(Handle* h, const R* T, int64_t ld, int64_t nb, int nrhs, R* Y, int64_t ldb)
{
    ProfScope ps(h, RFLU_K_TRSM, 4.0 * (double)nb * nb * nrhs);
    hipLaunchKernelGGL((ctrsv_block_kernel<R, UPPER, !UPPER, false>), dim3(1), dim3(CTRSV_THREADS), 0, h->stream, T, ld, (int)nb, nrhs, Y, ldb);
    RFLU_HIP(hipGetLastError());
    return RFLU_OK;
}

template <typename R>
int csolve_fwd_narrow(Handle* h, int64_t n, int nrhs, const R* W, int64_t ldw, const int64_t* ipiv, R* B, int64_t ldb)
{
    if (n <= 0 || nrhs <= 0) return RFLU_OK;
    const int64_t cnb = block_rows();
    if (ipiv) RFLU_TRY(launch_claswp_fwd<R>(h, B, 1, ldb, n, nrhs, ipiv));
    for (int64_t j0 = 0; j0 < n; j0 += cnb) {   // L y = P b, top down; the band left of the block holds what is already solved
        const int64_t nb = std::min(cnb, n - j0);
        RFLU_TRY(launch_cgemv_sub<R>(h, W, ldw, j0, nb, 0, j0, nrhs, B, ldb, false));
        RFLU_TRY((launch_ctrsv_block_fwd<R, false>(h, W + 2 * (j0 * ldw + j0), ldw, nb, nrhs, B + 2 * j0, ldb)));
    }
    for (int64_t j0 = (n - 1) / cnb * cnb; j0 >= 0; j0 -= cnb) {   // U x = y, bottom up; the band right of the block
        const int64_t nb = std::min(cnb, n - j0);
        RFLU_TRY(launch_cgemv_sub<R>(h, W, ldw, j0, nb, j0 + nb, n, nrhs, B, ldb, false));
        RFLU_TRY((launch_ctrsv_block_fwd<R, true>(h, W + 2 * (j0 * ldw + j0), ldw, nb, nrhs, B + 2 * j0, ldb)));
    }
    return RFLU_OK;
}

template <typename R>
int csolve_fwd_image(Handle* h, int64_t n, int64_t nrhs, const R* W, int64_t ldw, const int64_t* ipiv, R* X, int64_t ldx)
{
    if (n <= 0 || nrhs <= 0) return RFLU_OK;
    if (ipiv) RFLU_TRY(launch_claswp_fwd<R>(h, X, ldx, 1, n, nrhs, ipiv));
    RFLU_TRY(ctri_lower_rec<R>(h, n, nrhs, W, ldw, X, ldx, true));
    return ctri_upper_rec<R>(h, n, nrhs, W, ldw, X, ldx, false);
}

template <typename R>
int cgetrs_fwd_rm_dev(Handle* h, int64_t n, int64_t nrhs, const R* W, int64_t ldw, const int64_t* ipiv, R* B, int64_t ldb)
{
    RFLU_TRY(cgetrs_check_args(n, nrhs, W, ldw, B, ldb));
    if (n > INT32_MAX || nrhs > INT32_MAX) { set_error("complex mixed solve: n or nrhs beyond 2^31 - 1"); return RFLU_ERR_ARG; }
    if (n == 0 || nrhs == 0) return RFLU_OK;
    if (nrhs <= narrow_limit()) {
        RFLU_TRY(csolve_fwd_narrow<R>(h, n, (int)nrhs, W, ldw, ipiv, B, ldb));
    } else {
        const int64_t ldx = cworkspace_ld(nrhs);
        RFLU_TRY(ensure_buffer(&h->rhs_work, &h->rhs_work_bytes, (size_t)n * (size_t)ldx * 2 * sizeof(R)));
        R* X = static_cast<R*>(h->rhs_work);
        RFLU_TRY(launch_ctranspose<R>(h, n, nrhs, B, ldb, X, ldx, false));
        RFLU_TRY(csolve_fwd_image<R>(h, n, nrhs, W, ldw, ipiv, X, ldx));
        RFLU_TRY(launch_ctranspose<R>(h, nrhs, n, X, ldx, B, ldb, false));
    }
    RFLU_HIP(hipStreamSynchronize(h->stream));
    return RFLU_OK;
}

template int csolve_fwd_narrow<float>(Handle*, int64_t, int, const float*, int64_t, const int64_t*, float*, int64_t);
template int csolve_fwd_image<float>(Handle*, int64_t, int64_t, const float*, int64_t, const int64_t*, float*, int64_t);
template int cgetrs_fwd_rm_dev<float>(Handle*, int64_t, int64_t, const float*, int64_t, const int64_t*, float*, int64_t);
template int cgetrs_trans_cm_dev<double>(Handle*, int64_t, int64_t, const double*, int64_t, const int64_t*, double*, int64_t, int);
template int cgetrs_trans_cm_dev<float>(Handle*, int64_t, int64_t, const float*, int64_t, const int64_t*, float*, int64_t, int);
template int launch_claswp_rev<double>(Handle*, double*, int64_t, int64_t, int64_t, int64_t, const int64_t*);
template int launch_claswp_rev<float>(Handle*, float*, int64_t, int64_t, int64_t, int64_t, const int64_t*);
// the forward narrow solve on ComplexF64 row-major factors: M x of the condition estimate (cgecon_dev, driver.cpp)
template int csolve_fwd_narrow<double>(Handle*, int64_t, int, const double*, int64_t, const int64_t*, double*, int64_t);

}  // namespace rflu
