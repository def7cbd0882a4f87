// mixed.hip -- the kernels of the mixed-precision solve (Float32 factors, Float64 iterative refinement; LAPACK dsgesv's scheme).
//
//   demote_relayout   Float64 column-major A  ->  Float32 row-major F32 (the layout getrf_rm<float> factors in place) in ONE pass
//                     through LDS tiles, 8 n^2 bytes read + 4 n^2 written, and the row sums of |a_ij| of every tile on the way:
//                     ||A||_inf = the largest row sum, in Float64.
//   residual_few      R = B - A X in Float64 for up to RESIDUAL_PASS right-hand sides: A (column-major) is read in place exactly once,
//                     rows are the coalesced direction, the columns are split over workgroups.
//   the small ones    Float64 <-> Float32 conversion fused with the column-major <-> row-major change of the right-hand sides (with
//                     the update X += d on the way back), and the per-column norms ||r_k||_inf, ||x_k||_inf of the convergence rule.
//
// Everything here is reproducible bit for bit from run to run: no floating-point atomics anywhere.  Sums that cross workgroups go
// through a workspace of partial sums (Handle::mixed_part) and are combined in a fixed order by a second kernel; the split depends on
// n alone.  The vector (16-byte) and the element-wise forms of a kernel add the same numbers in the same order.
// Roofline: HBM for the two matrix passes (algorithmic bytes 12 n^2 and 8 n^2); the small kernels are latency.
#include "mixed_dev.hpp"

namespace rflu {

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

int launch_rowsum_max(Handle* h, int64_t n, int64_t ntj, const double* part, double* blockmax, double* out)
{
    const int64_t nb = (n + 255) / 256;
    hipLaunchKernelGGL(rowsum_max_kernel, dim3((unsigned)nb), dim3(256), 0, h->stream, (int)n, (int)ntj, part, blockmax);
    RFLU_HIP(hipGetLastError());
    hipLaunchKernelGGL(final_max_kernel, dim3(1), dim3(256), 0, h->stream, (int)nb, blockmax, out);
    RFLU_HIP(hipGetLastError());
    return RFLU_OK;
}

int launch_demote_relayout(Handle* h, int64_t n, const double* A, int64_t lda, float* F, int64_t ldf, double* anorm_dev)
{
    if (n <= 0) return RFLU_OK;
    const int64_t nti = (n + DM_TI - 1) / DM_TI, ntj = (n + DM_TJ - 1) / DM_TJ, nb = (n + 255) / 256;
    if (ntj > 65535) { set_error("demote_relayout: n = %lld is too large", (long long)n); return RFLU_ERR_ARG; }
    RFLU_TRY(ensure_buffer(&h->mixed_part, &h->mixed_part_bytes, (size_t)(ntj * n + nb) * sizeof(double)));
    double* part = static_cast<double*>(h->mixed_part);
    double* blockmax = part + ntj * n;
    const bool vin = reinterpret_cast<uintptr_t>(A) % 16 == 0 && lda % 2 == 0;
    const bool vout = reinterpret_cast<uintptr_t>(F) % 16 == 0 && ldf % 4 == 0;
    const dim3 grid((unsigned)nti, (unsigned)ntj);
    {
        ProfScope ps(h, RFLU_K_TRANSPOSE, 12.0 * (double)n * (double)n);
        if (vin && vout) hipLaunchKernelGGL((demote_relayout_kernel<true, true>), grid, dim3(256), 0, h->stream, (int)n, A, lda, F, ldf, part);
        else if (vin)    hipLaunchKernelGGL((demote_relayout_kernel<true, false>), grid, dim3(256), 0, h->stream, (int)n, A, lda, F, ldf, part);
        else if (vout)   hipLaunchKernelGGL((demote_relayout_kernel<false, true>), grid, dim3(256), 0, h->stream, (int)n, A, lda, F, ldf, part);
        else             hipLaunchKernelGGL((demote_relayout_kernel<false, false>), grid, dim3(256), 0, h->stream, (int)n, A, lda, F, ldf, part);
        RFLU_HIP(hipGetLastError());
    }
    return launch_rowsum_max(h, n, ntj, part, blockmax, anorm_dev);
}

// ---- residual_few ----------------------------------------------------------------------------------------------------------------
// Workgroup (bx, by): rows [512 bx, 512 bx + 512) x columns [cj by, cj by + cj).  A thread owns two rows (VEC: adjacent, one 16-byte
// load per column; otherwise rows t and t + 256) and NR right-hand sides: 2 NR accumulators, one fma per element and right-hand side,
// the columns in ascending order.  X[j, k] has the same address in every lane (scalar loads).  Nothing is shared between threads: no
// LDS, no barrier; several columns' loads are in flight per thread.  part[(by * NR + k) * n + i] = the slice's share of (A X)[i, k].
constexpr int RF_ROWS = 512, RF_MIN_CJ = 32, RF_TARGET_WGS = 2048;

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

// R[i, k] = B[i, k] - (the slices' shares in slice order)
__global__ void __launch_bounds__(256) residual_combine_kernel(int n, int nr, int splits, const double* __restrict__ part,
                                                               const double* __restrict__ B, int64_t ldb, double* __restrict__ R, int64_t ldr)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int k = blockIdx.y;
    if (i >= n) return;
    double s = 0.0;
#pragma unroll 16
    for (int sp = 0; sp < splits; ++sp) s += part[((int64_t)sp * nr + k) * n + i];
    R[i + k * ldr] = B[i + k * ldb] - s;
}

template <int NR>
static void launch_residual_nr(hipStream_t st, dim3 grid, bool vec, int n, int cj, const double* A, int64_t lda, const double* X, int64_t ldx,
                               double* part)
{
    if (vec) hipLaunchKernelGGL((residual_few_kernel<NR, true>), grid, dim3(256), 0, st, n, cj, A, lda, X, ldx, part);
    else     hipLaunchKernelGGL((residual_few_kernel<NR, false>), grid, dim3(256), 0, st, n, cj, A, lda, X, ldx, part);
}

int launch_residual_few(Handle* h, int64_t n, int64_t nrhs, const double* A, int64_t lda, const double* X, int64_t ldx, const double* B,
                        int64_t ldb, double* R, int64_t ldr)
{
    if (n <= 0 || nrhs <= 0) return RFLU_OK;
    if (nrhs > RESIDUAL_PASS) { set_error("residual_few: at most %d right-hand sides per pass", RESIDUAL_PASS); return RFLU_ERR_ARG; }
    // the split is a function of n alone (the results do not depend on the device or on what else runs)
    const int64_t rb = (n + RF_ROWS - 1) / RF_ROWS;
    int64_t splits = std::max<int64_t>(1, std::min<int64_t>((n + RF_MIN_CJ - 1) / RF_MIN_CJ, (RF_TARGET_WGS + rb - 1) / rb));
    const int64_t cj = ((n + splits - 1) / splits + 7) / 8 * 8;
    splits = (n + cj - 1) / cj;
    if (splits > 65535) { set_error("residual_few: n = %lld is too large", (long long)n); return RFLU_ERR_ARG; }
    RFLU_TRY(ensure_buffer(&h->mixed_part, &h->mixed_part_bytes, (size_t)(splits * nrhs * n) * sizeof(double)));
    double* part = static_cast<double*>(h->mixed_part);
    const bool vec = reinterpret_cast<uintptr_t>(A) % 16 == 0 && lda % 2 == 0;
    const dim3 grid((unsigned)rb, (unsigned)splits);
    {
        ProfScope ps(h, RFLU_K_MISC, 2.0 * (double)n * (double)n * (double)nrhs, 8.0 * (double)n * (double)n);
        switch (nrhs) {
            case 1: launch_residual_nr<1>(h->stream, grid, vec, (int)n, (int)cj, A, lda, X, ldx, part); break;
            case 2: launch_residual_nr<2>(h->stream, grid, vec, (int)n, (int)cj, A, lda, X, ldx, part); break;
            case 3: launch_residual_nr<3>(h->stream, grid, vec, (int)n, (int)cj, A, lda, X, ldx, part); break;
            case 4: launch_residual_nr<4>(h->stream, grid, vec, (int)n, (int)cj, A, lda, X, ldx, part); break;
            case 5: launch_residual_nr<5>(h->stream, grid, vec, (int)n, (int)cj, A, lda, X, ldx, part); break;
            case 6: launch_residual_nr<6>(h->stream, grid, vec, (int)n, (int)cj, A, lda, X, ldx, part); break;
            case 7: launch_residual_nr<7>(h->stream, grid, vec, (int)n, (int)cj, A, lda, X, ldx, part); break;
            default: launch_residual_nr<8>(h->stream, grid, vec, (int)n, (int)cj, A, lda, X, ldx, part); break;
        }
        RFLU_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(residual_combine_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)nrhs), dim3(256), 0, h->stream, (int)n, (int)nrhs,
                       (int)splits, part, B, ldb, R, ldr);
    RFLU_HIP(hipGetLastError());
    return RFLU_OK;
}

// ---- the small kernels -------------------------------------------------------------------------------------------------------------
// out[r][c] (+)= (TO) in[c][r]: transpose_kernel (laswp.hip) with a change of element type and, ADD, an update instead of a store.
// A column-major n x nrhs block IS a row-major nrhs x n one, so this is demote(R) -> row-major Float32 workspace one way and
// X (+)= promote(d) the other way.
template <typename TI, typename TO, bool ADD>
__global__ void __launch_bounds__(256) convert_transpose_kernel(int64_t rows_out, int64_t cols_out, const TI* __restrict__ in, int64_t ld_in,
                                                                TO* __restrict__ out, int64_t ld_out)
{
    __shared__ TO tile[64][65];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int64_t r0 = (int64_t)blockIdx.y * 64, c0 = (int64_t)blockIdx.x * 64;
    for (int i = ty; i < 64; i += 4) {
        const int64_t ir = c0 + i, ic = r0 + tx;
        tile[i][tx] = (ir < cols_out && ic < rows_out) ? (TO)in[ir * ld_in + ic] : TO(0);
    }
    __syncthreads();
    for (int i = ty; i < 64; i += 4) {
        const int64_t orow = r0 + i, ocol = c0 + tx;
        if (orow < rows_out && ocol < cols_out) {
            if (ADD) out[orow * ld_out + ocol] += tile[tx][i];
            else out[orow * ld_out + ocol] = tile[tx][i];
        }
    }
}

template <typename TI, typename TO>
int launch_convert_transpose(Handle* h, int64_t rows_out, int64_t cols_out, const TI* in, int64_t ld_in, TO* out, int64_t ld_out, bool add)
{
    if (rows_out <= 0 || cols_out <= 0) return RFLU_OK;
    const int64_t gx = (cols_out + 63) / 64, gy = (rows_out + 63) / 64;
    if (gy > 65535) { set_error("right-hand side conversion: %lld rows are too many", (long long)rows_out); return RFLU_ERR_ARG; }
    const dim3 grid((unsigned)gx, (unsigned)gy);
    if (add) hipLaunchKernelGGL((convert_transpose_kernel<TI, TO, true>), grid, dim3(256), 0, h->stream, rows_out, cols_out, in, ld_in, out, ld_out);
    else     hipLaunchKernelGGL((convert_transpose_kernel<TI, TO, false>), grid, dim3(256), 0, h->stream, rows_out, cols_out, in, ld_in, out, ld_out);
    RFLU_HIP(hipGetLastError());
    return RFLU_OK;
}
template int launch_convert_transpose<double, float>(Handle*, int64_t, int64_t, const double*, int64_t, float*, int64_t, bool);
template int launch_convert_transpose<float, double>(Handle*, int64_t, int64_t, const float*, int64_t, double*, int64_t, bool);

// norms[2k] = ||r_k||_inf, norms[2k + 1] = ||x_k||_inf; one workgroup per column
__global__ void __launch_bounds__(256) colnorms_kernel(int64_t n, const double* __restrict__ R, int64_t ldr, const double* __restrict__ X,
                                                       int64_t ldx, double* __restrict__ norms)
{
    __shared__ double sh[256];
    const int64_t k = blockIdx.x;
    double rn = 0.0, xn = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        rn = nanmax(rn, fabs(R[i + k * ldr]));
        xn = nanmax(xn, fabs(X[i + k * ldx]));
    }
    rn = block_nanmax(rn, sh);
    __syncthreads();
    xn = block_nanmax(xn, sh);
    if (threadIdx.x == 0) {
        norms[2 * k] = rn;
        norms[2 * k + 1] = xn;
    }
}

int launch_colnorms(Handle* h, int64_t n, int64_t nrhs, const double* R, int64_t ldr, const double* X, int64_t ldx, double* norms)
{
    if (n <= 0 || nrhs <= 0) return RFLU_OK;
    hipLaunchKernelGGL(colnorms_kernel, dim3((unsigned)nrhs), dim3(256), 0, h->stream, n, R, ldr, X, ldx, norms);
    RFLU_HIP(hipGetLastError());
    return RFLU_OK;
}

}  // namespace rflu
