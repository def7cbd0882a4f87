// mixed.hip -- the kernels of the mixed-precision solve for real and complex elements: Float32 factors with Float64 iterative refinement
// (LAPACK dsgesv's scheme) and ComplexF32 factors with ComplexF64 refinement (zcgesv's; section 4.10).  E is the
// element trait of rflu_internal.hpp: RealElem<double> is one Float64 word, CplxElem<double> an interleaved (re, im) pair; every array
// crosses as double* / float* and every leading dimension counts elements.
//
//   demote_relayout   column-major A -> row-major F32 of the narrow type (the layout getrf_rm<float> / cgetrf_rm<float> factor in place)
//                     in ONE pass through LDS tiles, 8 n^2 bytes read + 4 n^2 written per part, and the row sums of |a_ij| of every tile
//                     on the way: ||A||_inf = the largest row sum, in Float64 (complex: of the moduli hypot(re, im), LAPACK zlange('I')).
//   residual_few      R = B - A X in the wide type for up to RESIDUAL_PASS right-hand sides: A (column-major) is read in place exactly
//                     once, rows are the coalesced direction, the columns are split over workgroups.
//   the small ones    wide <-> narrow conversion fused with the column-major <-> row-major change of the right-hand sides (complex, few
//                     right-hand sides: element-wise, the narrow solve works on columns), with the update X += d on the way back, and the
//                     per-column norms ||r_k||_inf, ||x_k||_inf (complex: largest modulus) of the convergence rule.
//
// What is stated once, as a template on E: the second stage of ||A||_inf, the combine of the residual's partial sums, the column norms,
// the transposing conversion and every host launcher (buffer sizes, the split, the refusals, the timers' figures, the dispatch on the
// number of right-hand sides and on alignment).  What stays two bodies side by side: demote_relayout_kernel / cdemote_relayout_kernel and
// residual_slice / cresidual_slice with their *_few_kernel wrappers.  Their thread-to-data maps differ -- a real lane owns two rows
// (one 16-byte load), a complex lane one element; tiles of 128 x 64 against 64 x 64 -- and tests/mixed_cases.py restates the real one
// index by index; folded, most of their lines would carry a switch on PARTS and the order of the row sums would be at risk.
//
// Everything here is a plain in-order launch on the handle's stream, reproducible bit for bit from run to run: no kernel waits for
// another workgroup and there are no floating-point atomics.  Sums that cross workgroups go through a workspace of partial sums
// (Handle::mixed_part) and are combined in a fixed order by a second kernel; the split depends on n alone.  The vector (16-byte) and the
// element-wise forms of a kernel add the same numbers in the same order.
// Roofline: HBM for the two matrix passes (algorithmic bytes 12 n^2 and 8 n^2 per part); the small kernels are latency.
#include <algorithm>

#include "complex_dev.hpp"

namespace rflu {

typedef RealElem<double> MixedReal;
typedef CplxElem<double> MixedCplx;

// max that keeps a NaN once it has seen one (fmax drops it): a NaN or Inf anywhere must reach the host's convergence test
__device__ __forceinline__ double nanmax(double m, double v) { return (v > m || v != v) ? v : m; }

// all 256 threads of the workgroup call it; thread 0 holds the result (fixed tree: the same order every run)
__device__ __forceinline__ double block_nanmax(double v, double* sh)
{
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] = nanmax(sh[threadIdx.x], sh[threadIdx.x + s]);
        __syncthreads();
    }
    return sh[0];
}

// 16-byte accesses.  Real: a load is two adjacent rows of a column of A, so every column has to start on a boundary (lda even), and a
// store is four adjacent columns of a row of F32 (ldf a multiple of 4).
static bool aligned_in(MixedReal, const double* A, int64_t lda) { return reinterpret_cast<uintptr_t>(A) % 16 == 0 && lda % 2 == 0; }
static bool aligned_out(MixedReal, const float* F, int64_t ldf) { return reinterpret_cast<uintptr_t>(F) % 16 == 0 && ldf % 4 == 0; }
// Complex: an element of A is 16 bytes, so every element sits on a boundary exactly when A does, whatever lda; a store is two adjacent
// elements of a row of F32 (ldf even).
static bool aligned_in(MixedCplx, const double* A, int64_t) { return reinterpret_cast<uintptr_t>(A) % 16 == 0; }
static bool aligned_out(MixedCplx, const float* F, int64_t ldf) { return reinterpret_cast<uintptr_t>(F) % 16 == 0 && ldf % 2 == 0; }

// ---- demote_relayout -------------------------------------------------------------------------------------------------------------
// One workgroup = one tile of DM_TI rows x DM_TJ columns of A.  Load: a lane owns two rows (VIN: the adjacent rows 2l, 2l+1 as one
// 16-byte load, a wave reads 1 KiB of one column; otherwise rows l and l + 64), the four waves take the columns c = w, w+4, ...
// Store: 64 consecutive columns of a row of F32 = 256 contiguous bytes (VOUT: 16 lanes x float4).  Row sums of |a|: every lane adds
// its columns in ascending order, the four waves' sums are added in wave order -> part[tile column][row].
constexpr int DM_TI = 128, DM_TJ = 64, DM_P = 65;   // 65: the column-direction LDS writes of the load phase spread over the banks

template <bool VIN, bool VOUT>
__global__ void __launch_bounds__(256) demote_relayout_kernel(int n, const double* __restrict__ A, int64_t lda, float* __restrict__ F,
                                                              int64_t ldf, double* __restrict__ part)
{
    __shared__ float tile[DM_TI * DM_P];
    __shared__ double rsum[4][DM_TI];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    // diagonal tile order (as transpose_kernel, laswp.hip): with a power-of-two ldf the tiles of one tile column start 2^k bytes apart
    const int tj = (int)((blockIdx.y + blockIdx.x) % gridDim.y);
    const int64_t i0 = (int64_t)blockIdx.x * DM_TI, j0 = (int64_t)tj * DM_TJ;
    const int ra = VIN ? 2 * lane : lane, rb = VIN ? 2 * lane + 1 : lane + 64;
    const bool oka = i0 + ra < n, okb = i0 + rb < n;
    double sa = 0.0, sb = 0.0;
#pragma unroll 4
    for (int c = w; c < DM_TJ; c += 4) {
        const int64_t j = j0 + c;
        double va = 0.0, vb = 0.0;
        if (j < n) {
            const double* col = A + j * lda + i0;
            if (VIN && okb) {
                const double2 v = *reinterpret_cast<const double2*>(col + ra);
                va = v.x;
                vb = v.y;
            } else {
                if (oka) va = col[ra];
                if (okb) vb = col[rb];
            }
        }
        sa += fabs(va);
        sb += fabs(vb);
        tile[ra * DM_P + c] = (float)va;
        tile[rb * DM_P + c] = (float)vb;
    }
    rsum[w][ra] = sa;
    rsum[w][rb] = sb;
    __syncthreads();
    if (threadIdx.x < DM_TI && i0 + threadIdx.x < n) {
        const int r = threadIdx.x;
        part[(int64_t)tj * n + i0 + r] = ((rsum[0][r] + rsum[1][r]) + rsum[2][r]) + rsum[3][r];
    }
    if (VOUT) {
        const int q = threadIdx.x & 15, rr = threadIdx.x >> 4;
        for (int r = rr; r < DM_TI; r += 16) {
            const int64_t i = i0 + r, j = j0 + 4 * q;
            if (i >= n) break;
            const float* t = tile + r * DM_P + 4 * q;
            if (j + 3 < n) {
                *reinterpret_cast<float4*>(F + i * ldf + j) = make_float4(t[0], t[1], t[2], t[3]);
            } else {
                for (int k = 0; k < 4; ++k)
                    if (j + k < n) F[i * ldf + j + k] = t[k];
            }
        }
    } else {
        for (int r = w; r < DM_TI; r += 4) {
            const int64_t i = i0 + r, j = j0 + lane;
            if (i < n && j < n) F[i * ldf + j] = tile[r * DM_P + lane];
        }
    }
}

// The complex tile is CDM_T rows x CDM_T columns.  Load: lane l owns row l (VIN: one 16-byte load per element, a wave reads 1 KiB of
// one column), the four waves take the columns c = w, w + 4, ...  Store: 64 consecutive columns of a row of F32 = 512 contiguous bytes
// (VOUT: 32 lanes x float4 = two elements each).  Row sums of the moduli, taken as plain hypot: the order of the real kernel.  A
// 128-row tile of 8-byte elements (the real shape) is 66560 B, more than a workgroup's static LDS; 64 x 65 x 8 B = 33280 B.
constexpr int CDM_T = 64, CDM_P = 65;   // 65: the column-direction 8-byte LDS writes of the load phase spread over the banks

template <bool VIN, bool VOUT>
__global__ void __launch_bounds__(256) cdemote_relayout_kernel(int n, const double* __restrict__ A, int64_t lda, float* __restrict__ F,
                                                               int64_t ldf, double* __restrict__ part)
{
    __shared__ float2 tile[CDM_T * CDM_P];
    __shared__ double rsum[4][CDM_T];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    // diagonal tile order (as demote_relayout_kernel): with a power-of-two ldf the tiles of one tile column start 2^k bytes apart
    const int tj = (int)((blockIdx.y + blockIdx.x) % gridDim.y);
    const int64_t i0 = (int64_t)blockIdx.x * CDM_T, j0 = (int64_t)tj * CDM_T;
    const bool ok = i0 + lane < n;
    double s = 0.0;
#pragma unroll 4
    for (int c = w; c < CDM_T; c += 4) {
        const int64_t j = j0 + c;
        double re = 0.0, im = 0.0;
        if (ok && j < n) {
            const double* p = A + 2 * (j * lda + i0 + lane);
            if (VIN) {
                const double2 v = *reinterpret_cast<const double2*>(p);
                re = v.x;
                im = v.y;
            } else {
                re = p[0];
                im = p[1];
            }
        }
        s += hypot(re, im);
        tile[lane * CDM_P + c] = make_float2((float)re, (float)im);
    }
    rsum[w][lane] = s;
    __syncthreads();
    if (threadIdx.x < CDM_T && i0 + threadIdx.x < n) {
        const int r = threadIdx.x;
        part[(int64_t)tj * n + i0 + r] = ((rsum[0][r] + rsum[1][r]) + rsum[2][r]) + rsum[3][r];
    }
    if (VOUT) {
        const int q = threadIdx.x & 31, rr = threadIdx.x >> 5;
        for (int r = rr; r < CDM_T; r += 8) {
            const int64_t i = i0 + r, j = j0 + 2 * q;
            if (i >= n) break;
            const float2 t0 = tile[r * CDM_P + 2 * q], t1 = tile[r * CDM_P + 2 * q + 1];
            float* out = F + 2 * (i * ldf + j);
            if (j + 1 < n) {
                *reinterpret_cast<float4*>(out) = make_float4(t0.x, t0.y, t1.x, t1.y);
            } else if (j < n) {
                out[0] = t0.x;
                out[1] = t0.y;
            }
        }
    } else {
        for (int r = w; r < CDM_T; r += 4) {
            const int64_t i = i0 + r, j = j0 + lane;
            if (i < n && j < n) {
                const float2 t = tile[r * CDM_P + lane];
                float* out = F + 2 * (i * ldf + j);
                out[0] = t.x;
                out[1] = t.y;
            }
        }
    }
}

// the kernel family of an element type: the two bodies have one signature
template <typename E, bool VIN, bool VOUT>
constexpr auto demote_kernel = E::PARTS == 1 ? demote_relayout_kernel<VIN, VOUT> : cdemote_relayout_kernel<VIN, VOUT>;

// second stage: row i's sum = its tiles' sums in tile order; the largest of a workgroup's 256 rows -> blockmax
__global__ void __launch_bounds__(256) rowsum_max_kernel(int n, int ntj, const double* __restrict__ part, double* __restrict__ blockmax)
{
    __shared__ double sh[256];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double s = 0.0;
    if (i < n) {
#pragma unroll 16   // the loads of 16 tiles in flight; the additions stay in tile order
        for (int t = 0; t < ntj; ++t) s += part[(int64_t)t * n + i];
    }
    const double m = block_nanmax(s, sh);
    if (threadIdx.x == 0) blockmax[blockIdx.x] = m;
}

__global__ void __launch_bounds__(256) final_max_kernel(int nb, const double* __restrict__ blockmax, double* __restrict__ out)
{
    __shared__ double sh[256];
    double m = 0.0;
    for (int b = threadIdx.x; b < nb; b += 256) m = nanmax(m, blockmax[b]);
    m = block_nanmax(m, sh);
    if (threadIdx.x == 0) out[0] = m;
}

// *out (device) <- the largest over rows i < n of part[0 * n + i] + part[1 * n + i] + ... (ntj terms, in that order); blockmax:
// ceil(n / 256) doubles of workspace
static int launch_rowsum_max(Handle* h, int64_t n, int64_t ntj, const double* part, double* blockmax, double* out)
{
    const int64_t nb = (n + 255) / 256;
    hipLaunchKernelGGL(rowsum_max_kernel, dim3((unsigned)nb), dim3(256), 0, h->stream, (int)n, (int)ntj, part, blockmax);
    RFLU_HIP(hipGetLastError());
    hipLaunchKernelGGL(final_max_kernel, dim3(1), dim3(256), 0, h->stream, (int)nb, blockmax, out);
    RFLU_HIP(hipGetLastError());
    return RFLU_OK;
}

template <typename E>
int launch_demote_relayout(Handle* h, int64_t n, const double* A, int64_t lda, float* F, int64_t ldf, double* anorm_dev)
{
    constexpr int P = E::PARTS;
    if (n <= 0) return RFLU_OK;
    const int64_t nti = (n + DM_TI / P - 1) / (DM_TI / P), ntj = (n + DM_TJ - 1) / DM_TJ, nb = (n + 255) / 256;
    if (ntj > 65535) { set_error("%sdemote_relayout: n = %lld is too large", E::WHO, (long long)n); return RFLU_ERR_ARG; }
    RFLU_TRY(ensure_buffer(&h->mixed_part, &h->mixed_part_bytes, (size_t)(ntj * n + nb) * sizeof(double)));
    double* part = static_cast<double*>(h->mixed_part);
    double* blockmax = part + ntj * n;
    const bool vin = aligned_in(E(), A, lda), vout = aligned_out(E(), F, ldf);
    const dim3 grid((unsigned)nti, (unsigned)ntj);
    {
        ProfScope ps(h, RFLU_K_TRANSPOSE, 12.0 * P * (double)n * (double)n);
        if (vin && vout) hipLaunchKernelGGL((demote_kernel<E, true, true>), grid, dim3(256), 0, h->stream, (int)n, A, lda, F, ldf, part);
        else if (vin)    hipLaunchKernelGGL((demote_kernel<E, true, false>), grid, dim3(256), 0, h->stream, (int)n, A, lda, F, ldf, part);
        else if (vout)   hipLaunchKernelGGL((demote_kernel<E, false, true>), grid, dim3(256), 0, h->stream, (int)n, A, lda, F, ldf, part);
        else             hipLaunchKernelGGL((demote_kernel<E, false, false>), grid, dim3(256), 0, h->stream, (int)n, A, lda, F, ldf, part);
        RFLU_HIP(hipGetLastError());
    }
    return launch_rowsum_max(h, n, ntj, part, blockmax, anorm_dev);
}

// ---- residual_few ----------------------------------------------------------------------------------------------------------------
// Workgroup (bx, by): rows [512 bx, 512 bx + 512) x columns [cj by, cj by + cj).  A thread owns two rows (VEC: adjacent, one 16-byte
// load per column; otherwise rows t and t + 256) and NR right-hand sides: 2 NR accumulators, one fma per element and right-hand side,
// the columns in ascending order.  X[j, k] has the same address in every lane (scalar loads).  Nothing is shared between threads: no
// LDS, no barrier; several columns' loads are in flight per thread.  part[(by * NR + k) * n + i] = the slice's share of (A X)[i, k].
constexpr int RF_ROWS = 512, RF_MIN_CJ = 32, RF_TARGET_WGS = 2048;   // rows per workgroup: 256 threads x 16 bytes = RF_ROWS / PARTS elements

template <int NR, bool VEC, bool FULL>
__device__ __forceinline__ void residual_slice(int n, int64_t ia, int64_t ib, int64_t jbeg, int64_t jend, const double* __restrict__ A,
                                               int64_t lda, const double* __restrict__ X, int64_t ldx, double (&acca)[NR], double (&accb)[NR])
{
    const bool oka = FULL || ia < n, okb = FULL || ib < n;
    // columns in flight per thread: 8, or 4 where 8 columns' X values (2 NR scalar registers each) no longer fit the scalar file
#pragma unroll(NR <= 4 ? 8 : 4)
    for (int64_t j = jbeg; j < jend; ++j) {
        const double* col = A + j * lda;
        double va = 0.0, vb = 0.0;
        if (VEC && okb) {
            const double2 v = *reinterpret_cast<const double2*>(col + ia);
            va = v.x;
            vb = v.y;
        } else {
            if (oka) va = col[ia];
            if (okb) vb = col[ib];
        }
#pragma unroll
        for (int k = 0; k < NR; ++k) {
            const double x = X[j + k * ldx];
            acca[k] = fma(va, x, acca[k]);
            accb[k] = fma(vb, x, accb[k]);
        }
    }
}

template <int NR, bool VEC>
__global__ void __launch_bounds__(256) residual_few_kernel(int n, int cj, const double* __restrict__ A, int64_t lda,
                                                           const double* __restrict__ X, int64_t ldx, double* __restrict__ part)
{
    const int t = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * RF_ROWS;
    const int64_t ia = i0 + (VEC ? 2 * t : t), ib = i0 + (VEC ? 2 * t + 1 : t + 256);
    const int64_t jbeg = (int64_t)blockIdx.y * cj, jend = jbeg + cj < n ? jbeg + cj : n;
    double acca[NR], accb[NR];
#pragma unroll
    for (int k = 0; k < NR; ++k) acca[k] = accb[k] = 0.0;
    if (i0 + RF_ROWS <= n) residual_slice<NR, VEC, true>(n, ia, ib, jbeg, jend, A, lda, X, ldx, acca, accb);
    else                   residual_slice<NR, VEC, false>(n, ia, ib, jbeg, jend, A, lda, X, ldx, acca, accb);
    double* p = part + (int64_t)blockIdx.y * NR * n;
#pragma unroll
    for (int k = 0; k < NR; ++k) {
        if (ia < n) p[(int64_t)k * n + ia] = acca[k];
        if (ib < n) p[(int64_t)k * n + ib] = accb[k];
    }
}

// The complex workgroup (bx, by): rows [256 bx, 256 bx + 256) x the same columns.  A thread owns one row (VEC: one 16-byte load per
// element; otherwise its two words) and NR right-hand sides: NR complex accumulators, one cfma (four fused multiply-adds) per element
// and right-hand side, the columns in ascending order.  part[2 * ((by * NR + k) * n + i)] = the slice's share of (A X)[i, k].
constexpr int CRF_ROWS = RF_ROWS / 2;

template <int NR, bool VEC, bool FULL>
__device__ __forceinline__ void cresidual_slice(int n, int64_t i, int64_t jbeg, int64_t jend, const double* __restrict__ A, int64_t lda,
                                                const double* __restrict__ X, int64_t ldx, Cx<double> (&acc)[NR])
{
    const bool ok = FULL || i < n;
    // columns in flight per thread: 4, or 2 where 4 columns' X values (4 NR scalar registers each) no longer fit the scalar file
#pragma unroll(NR <= 4 ? 4 : 2)
    for (int64_t j = jbeg; j < jend; ++j) {
        const double* p = A + 2 * (j * lda + i);
        Cx<double> v{0.0, 0.0};
        if (ok) {
            if (VEC) {
                const double2 t = *reinterpret_cast<const double2*>(p);
                v = Cx<double>{t.x, t.y};
            } else {
                v = Cx<double>{p[0], p[1]};
            }
        }
#pragma unroll
        for (int k = 0; k < NR; ++k) {
            const double* x = X + 2 * (j + k * ldx);
            acc[k] = cfma(v, Cx<double>{x[0], x[1]}, acc[k]);
        }
    }
}

template <int NR, bool VEC>
__global__ void __launch_bounds__(256) cresidual_few_kernel(int n, int cj, const double* __restrict__ A, int64_t lda,
                                                            const double* __restrict__ X, int64_t ldx, double* __restrict__ part)
{
    const int64_t i0 = (int64_t)blockIdx.x * CRF_ROWS, i = i0 + threadIdx.x;
    const int64_t jbeg = (int64_t)blockIdx.y * cj, jend = jbeg + cj < n ? jbeg + cj : n;
    Cx<double> acc[NR];
#pragma unroll
    for (int k = 0; k < NR; ++k) acc[k] = Cx<double>{0.0, 0.0};
    if (i0 + CRF_ROWS <= n) cresidual_slice<NR, VEC, true>(n, i, jbeg, jend, A, lda, X, ldx, acc);
    else                    cresidual_slice<NR, VEC, false>(n, i, jbeg, jend, A, lda, X, ldx, acc);
    if (i < n) {
        double* p = part + 2 * ((int64_t)blockIdx.y * NR * n + i);
#pragma unroll
        for (int k = 0; k < NR; ++k) *reinterpret_cast<double2*>(p + 2 * ((int64_t)k * n)) = make_double2(acc[k].re, acc[k].im);
    }
}

template <typename E, int NR, bool VEC>
constexpr auto residual_kernel = E::PARTS == 1 ? residual_few_kernel<NR, VEC> : cresidual_few_kernel<NR, VEC>;

// R[i, k] = B[i, k] - (the slices' shares in slice order), every part on its own; 16 bytes per slice in flight
template <typename E>
__global__ void __launch_bounds__(256) residual_combine_kernel(int n, int nr, int splits, const double* __restrict__ part,
                                                               const double* __restrict__ B, int64_t ldb, double* __restrict__ R, int64_t ldr)
{
    constexpr int P = E::PARTS;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int k = blockIdx.y;
    if (i >= n) return;
    double s[P];
#pragma unroll
    for (int q = 0; q < P; ++q) s[q] = 0.0;
#pragma unroll(16 / P)
    for (int sp = 0; sp < splits; ++sp) {
        const double* t = static_cast<const double*>(__builtin_assume_aligned(part + P * (((int64_t)sp * nr + k) * n + i), 8 * P));
#pragma unroll
        for (int q = 0; q < P; ++q) s[q] += t[q];
    }
#pragma unroll
    for (int q = 0; q < P; ++q) R[P * (i + k * ldr) + q] = B[P * (i + k * ldb) + q] - s[q];
}

template <typename E, int NR>
static void launch_residual_nr(hipStream_t st, dim3 grid, bool vec, int n, int cj, const double* A, int64_t lda, const double* X, int64_t ldx,
                               double* part)
{
    if (vec) hipLaunchKernelGGL((residual_kernel<E, NR, true>), grid, dim3(256), 0, st, n, cj, A, lda, X, ldx, part);
    else     hipLaunchKernelGGL((residual_kernel<E, NR, false>), grid, dim3(256), 0, st, n, cj, A, lda, X, ldx, part);
}

template <typename E>
int launch_residual_few(Handle* h, int64_t n, int64_t nrhs, const double* A, int64_t lda, const double* X, int64_t ldx, const double* B,
                        int64_t ldb, double* R, int64_t ldr)
{
    constexpr int P = E::PARTS;
    if (n <= 0 || nrhs <= 0) return RFLU_OK;
    if (nrhs > RESIDUAL_PASS) { set_error("%sresidual_few: at most %d right-hand sides per pass", E::WHO, RESIDUAL_PASS); return RFLU_ERR_ARG; }
    // the split is a function of n alone (the results do not depend on the device or on what else runs)
    const int64_t rb = (n + RF_ROWS / P - 1) / (RF_ROWS / P);
    int64_t splits = std::max<int64_t>(1, std::min<int64_t>((n + RF_MIN_CJ - 1) / RF_MIN_CJ, (RF_TARGET_WGS + rb - 1) / rb));
    const int64_t cj = ((n + splits - 1) / splits + 7) / 8 * 8;
    splits = (n + cj - 1) / cj;
    if (splits > 65535) { set_error("%sresidual_few: n = %lld is too large", E::WHO, (long long)n); return RFLU_ERR_ARG; }
    RFLU_TRY(ensure_buffer(&h->mixed_part, &h->mixed_part_bytes, (size_t)(splits * nrhs * n) * P * sizeof(double)));
    double* part = static_cast<double*>(h->mixed_part);
    const bool vec = aligned_in(E(), A, lda);
    const dim3 grid((unsigned)rb, (unsigned)splits);
    {
        ProfScope ps(h, RFLU_K_MISC, 2.0 * P * P * (double)n * (double)n * (double)nrhs, 8.0 * P * (double)n * (double)n);
        switch (nrhs) {
            case 1: launch_residual_nr<E, 1>(h->stream, grid, vec, (int)n, (int)cj, A, lda, X, ldx, part); break;
            case 2: launch_residual_nr<E, 2>(h->stream, grid, vec, (int)n, (int)cj, A, lda, X, ldx, part); break;
            case 3: launch_residual_nr<E, 3>(h->stream, grid, vec, (int)n, (int)cj, A, lda, X, ldx, part); break;
            case 4: launch_residual_nr<E, 4>(h->stream, grid, vec, (int)n, (int)cj, A, lda, X, ldx, part); break;
            case 5: launch_residual_nr<E, 5>(h->stream, grid, vec, (int)n, (int)cj, A, lda, X, ldx, part); break;
            case 6: launch_residual_nr<E, 6>(h->stream, grid, vec, (int)n, (int)cj, A, lda, X, ldx, part); break;
            case 7: launch_residual_nr<E, 7>(h->stream, grid, vec, (int)n, (int)cj, A, lda, X, ldx, part); break;
            default: launch_residual_nr<E, 8>(h->stream, grid, vec, (int)n, (int)cj, A, lda, X, ldx, part); break;
        }
        RFLU_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(residual_combine_kernel<E>, dim3((unsigned)((n + 255) / 256), (unsigned)nrhs), dim3(256), 0, h->stream, (int)n,
                       (int)nrhs, (int)splits, part, B, ldb, R, ldr);
    RFLU_HIP(hipGetLastError());
    return RFLU_OK;
}

// ---- the small kernels -------------------------------------------------------------------------------------------------------------
// out[i, k] (+)= (TO) in[i, k], both column-major n x nrhs complex: the few-right-hand-side complex solve works on columns, so the
// ComplexF32 right-hand sides keep the layout of B and X and only the element type changes
template <typename TI, typename TO, bool ADD>
__global__ void __launch_bounds__(256) cconvert_kernel(int64_t n, const TI* __restrict__ in, int64_t ld_in, TO* __restrict__ out, int64_t ld_out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
    if (i >= n) return;
    const TI* p = in + 2 * (i + k * ld_in);
    TO* q = out + 2 * (i + k * ld_out);
    if (ADD) {
        q[0] += (TO)p[0];
        q[1] += (TO)p[1];
    } else {
        q[0] = (TO)p[0];
        q[1] = (TO)p[1];
    }
}

template <typename TI, typename TO>
int launch_cconvert(Handle* h, int64_t n, int64_t nrhs, const TI* in, int64_t ld_in, TO* out, int64_t ld_out, bool add)
{
    if (n <= 0 || nrhs <= 0) return RFLU_OK;
    if (nrhs > 65535) { set_error("right-hand side conversion: %lld columns are too many for the column form", (long long)nrhs); return RFLU_ERR_ARG; }
    const dim3 grid((unsigned)((n + 255) / 256), (unsigned)nrhs);
    if (add) hipLaunchKernelGGL((cconvert_kernel<TI, TO, true>), grid, dim3(256), 0, h->stream, n, in, ld_in, out, ld_out);
    else     hipLaunchKernelGGL((cconvert_kernel<TI, TO, false>), grid, dim3(256), 0, h->stream, n, in, ld_in, out, ld_out);
    RFLU_HIP(hipGetLastError());
    return RFLU_OK;
}
template int launch_cconvert<double, float>(Handle*, int64_t, int64_t, const double*, int64_t, float*, int64_t, bool);
template int launch_cconvert<float, double>(Handle*, int64_t, int64_t, const float*, int64_t, double*, int64_t, bool);

// out[r][c] (+)= (TO) in[c][r] on elements of PARTS words: transpose_kernel / ctranspose_kernel (laswp.hip, complex.hip) with a change
// of element type and, ADD, an update instead of a store.  The tile is 64 / PARTS elements square (64 x 65 words, 32 x 33 x 2: the same
// LDS bytes), the tiles are numbered along blockIdx.x alone.  A column-major n x nrhs block IS a row-major nrhs x n one, so this is
// demote(R) -> row-major narrow workspace one way and X (+)= promote(d) the other way.
template <int PARTS, typename TI, typename TO, bool ADD>
__global__ void __launch_bounds__(256) convert_transpose_kernel(int64_t rows_out, int64_t cols_out, const TI* __restrict__ in, int64_t ld_in,
                                                                TO* __restrict__ out, int64_t ld_out, unsigned tiles_x)
{
    constexpr int T = 64 / PARTS, STEP = 256 / T;
    __shared__ TO tile[T][T + 1][PARTS];
    const int tx = threadIdx.x % T, ty = threadIdx.x / T;
    const int64_t r0 = (int64_t)(blockIdx.x / tiles_x) * T, c0 = (int64_t)(blockIdx.x % tiles_x) * T;
    for (int i = ty; i < T; i += STEP) {
        const int64_t ir = c0 + i, ic = r0 + tx;
        const bool ok = ir < cols_out && ic < rows_out;
#pragma unroll
        for (int q = 0; q < PARTS; ++q) tile[i][tx][q] = ok ? (TO)in[PARTS * (ir * ld_in + ic) + q] : TO(0);
    }
    __syncthreads();
    for (int i = ty; i < T; i += STEP) {
        const int64_t orow = r0 + i, ocol = c0 + tx;
        if (orow < rows_out && ocol < cols_out) {
            TO* o = out + PARTS * (orow * ld_out + ocol);
#pragma unroll
            for (int q = 0; q < PARTS; ++q) {
                if (ADD) o[q] += tile[tx][i][q];
                else o[q] = tile[tx][i][q];
            }
        }
    }
}

template <typename E, typename TI, typename TO>
int launch_convert_transpose(Handle* h, int64_t rows_out, int64_t cols_out, const TI* in, int64_t ld_in, TO* out, int64_t ld_out, bool add)
{
    constexpr int P = E::PARTS, T = 64 / P;
    if (rows_out <= 0 || cols_out <= 0) return RFLU_OK;
    const int64_t gx = (cols_out + T - 1) / T, gy = (rows_out + T - 1) / T;
    if (gx > INT32_MAX || gy > INT32_MAX || gx * gy > INT32_MAX) {
        set_error("%sright-hand side conversion: %lld x %lld is beyond one launch", E::WHO, (long long)rows_out, (long long)cols_out);
        return RFLU_ERR_ARG;
    }
    const dim3 grid((unsigned)(gx * gy));
    if (add) hipLaunchKernelGGL((convert_transpose_kernel<P, TI, TO, true>), grid, dim3(256), 0, h->stream, rows_out, cols_out, in, ld_in, out, ld_out, (unsigned)gx);
    else     hipLaunchKernelGGL((convert_transpose_kernel<P, TI, TO, false>), grid, dim3(256), 0, h->stream, rows_out, cols_out, in, ld_in, out, ld_out, (unsigned)gx);
    RFLU_HIP(hipGetLastError());
    return RFLU_OK;
}

// norms[2k] = ||r_k||_inf, norms[2k + 1] = ||x_k||_inf (complex: the largest modulus, plain hypot); one workgroup per column
template <typename E>
__global__ void __launch_bounds__(256) colnorms_kernel(int64_t n, const double* __restrict__ R, int64_t ldr, const double* __restrict__ X,
                                                       int64_t ldx, double* __restrict__ norms)
{
    constexpr int P = E::PARTS;
    __shared__ double sh[256];
    const int64_t k = blockIdx.x;
    double rn = 0.0, xn = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        rn = nanmax(rn, E::modulus(R + P * (i + k * ldr)));
        xn = nanmax(xn, E::modulus(X + P * (i + k * ldx)));
    }
    rn = block_nanmax(rn, sh);
    __syncthreads();
    xn = block_nanmax(xn, sh);
    if (threadIdx.x == 0) {
        norms[2 * k] = rn;
        norms[2 * k + 1] = xn;
    }
}

template <typename E>
int launch_colnorms(Handle* h, int64_t n, int64_t nrhs, const double* R, int64_t ldr, const double* X, int64_t ldx, double* norms)
{
    if (n <= 0 || nrhs <= 0) return RFLU_OK;
    hipLaunchKernelGGL(colnorms_kernel<E>, dim3((unsigned)nrhs), dim3(256), 0, h->stream, n, R, ldr, X, ldx, norms);
    RFLU_HIP(hipGetLastError());
    return RFLU_OK;
}

#define RFLU_INSTANTIATE_MIXED(E)                                                                                                           \
    template int launch_demote_relayout<E>(Handle*, int64_t, const double*, int64_t, float*, int64_t, double*);                            \
    template int launch_residual_few<E>(Handle*, int64_t, int64_t, const double*, int64_t, const double*, int64_t, const double*, int64_t, \
                                        double*, int64_t);                                                                                  \
    template int launch_convert_transpose<E, double, float>(Handle*, int64_t, int64_t, const double*, int64_t, float*, int64_t, bool);     \
    template int launch_convert_transpose<E, float, double>(Handle*, int64_t, int64_t, const float*, int64_t, double*, int64_t, bool);     \
    template int launch_colnorms<E>(Handle*, int64_t, int64_t, const double*, int64_t, const double*, int64_t, double*);
RFLU_INSTANTIATE_MIXED(MixedReal)
RFLU_INSTANTIATE_MIXED(MixedCplx)

}  // namespace rflu
