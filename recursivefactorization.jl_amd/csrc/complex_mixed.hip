// complex_mixed.hip -- the kernels of the complex mixed-precision solve (ComplexF32 factors, ComplexF64 iterative refinement; LAPACK
// zcgesv's scheme).  The complex counterparts of mixed.hip:
//
//   cdemote_relayout  ComplexF64 column-major A -> ComplexF32 row-major F32 (the layout cgetrf_rm<float> factors in place) in ONE pass
//                     through LDS tiles, 16 n^2 bytes read + 8 n^2 written, and the row sums of the MODULI hypot(re, im) of every tile
//                     on the way: ||A||_inf = the largest row sum, in Float64 (LAPACK zlange('I')).
//   cresidual_few     R = B - A X in ComplexF64 for up to RESIDUAL_PASS right-hand sides: A (column-major) is read in place exactly
//                     once, rows are the coalesced direction, the columns are split over workgroups.
//   the small ones    ComplexF64 <-> ComplexF32 conversion of the right-hand sides (element-wise for the few-right-hand-side solve, which
//                     works on column-major columns; through a row-major image for more), with the update X += d on the way back, and
//                     the per-column norms ||r_k||_inf, ||x_k||_inf (largest modulus) of the convergence rule.
//
// Everything here is a plain in-order launch on the handle's stream, reproducible bit for bit from run to run: no kernel waits for
// another workgroup and there are no floating-point atomics.  Sums that cross threads go through a workspace of partial sums
// (Handle::mixed_part) and are combined in a fixed order by a second kernel; the split depends on n alone.  The 16-byte and the
// element-wise forms of a kernel add the same numbers in the same order.
// Roofline: HBM for the two matrix passes (algorithmic bytes 24 n^2 and 16 n^2); the small kernels are latency.
#include <algorithm>

#include "complex_dev.hpp"
#include "mixed_dev.hpp"

namespace rflu {

// ---- cdemote_relayout ------------------------------------------------------------------------------------------------------------
// One workgroup = one tile of CDM_T rows x CDM_T columns of A.  Load: lane l owns row l (VIN: one 16-byte load per element, a wave
// reads 1 KiB of one column), the four waves take the columns c = w, w + 4, ...  Store: 64 consecutive columns of a row of F32 = 512
// contiguous bytes (VOUT: 32 lanes x float4 = two elements each).  Row sums of the moduli: every lane adds its columns in ascending
// order, the four waves' sums are added in wave order -> part[tile column][row].  A 128-row tile of 8-byte elements (mixed.hip's shape)
// is 66560 B, more than a workgroup's static LDS; 64 x 65 x 8 B = 33280 B.
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

int launch_cdemote_relayout(Handle* h, int64_t n, const double* A, int64_t lda, float* F, int64_t ldf, double* anorm_dev)
{
    if (n <= 0) return RFLU_OK;
    const int64_t nt = (n + CDM_T - 1) / CDM_T, nb = (n + 255) / 256;
    if (nt > 65535) { set_error("cdemote_relayout: n = %lld is too large", (long long)n); return RFLU_ERR_ARG; }
    RFLU_TRY(ensure_buffer(&h->mixed_part, &h->mixed_part_bytes, (size_t)(nt * n + nb) * sizeof(double)));
    double* part = static_cast<double*>(h->mixed_part);
    double* blockmax = part + nt * n;
    // a complex element is 16 bytes, so every element of A sits on a 16-byte boundary exactly when A does, whatever lda
    const bool vin = reinterpret_cast<uintptr_t>(A) % 16 == 0;
    const bool vout = reinterpret_cast<uintptr_t>(F) % 16 == 0 && ldf % 2 == 0;
    const dim3 grid((unsigned)nt, (unsigned)nt);
    {
        ProfScope ps(h, RFLU_K_TRANSPOSE, 24.0 * (double)n * (double)n);
        if (vin && vout) hipLaunchKernelGGL((cdemote_relayout_kernel<true, true>), grid, dim3(256), 0, h->stream, (int)n, A, lda, F, ldf, part);
        else if (vin)    hipLaunchKernelGGL((cdemote_relayout_kernel<true, false>), grid, dim3(256), 0, h->stream, (int)n, A, lda, F, ldf, part);
        else if (vout)   hipLaunchKernelGGL((cdemote_relayout_kernel<false, true>), grid, dim3(256), 0, h->stream, (int)n, A, lda, F, ldf, part);
        else             hipLaunchKernelGGL((cdemote_relayout_kernel<false, false>), grid, dim3(256), 0, h->stream, (int)n, A, lda, F, ldf, part);
        RFLU_HIP(hipGetLastError());
    }
    return launch_rowsum_max(h, n, nt, part, blockmax, anorm_dev);
}

// ---- cresidual_few ---------------------------------------------------------------------------------------------------------------
// Workgroup (bx, by): rows [256 bx, 256 bx + 256) x columns [cj by, cj by + cj).  A thread owns one row (VEC: one 16-byte load per
// element; otherwise its two words) and NR right-hand sides: NR complex accumulators, one cfma (four fused multiply-adds) per element
// and right-hand side, the columns in ascending order.  X[j, k] has the same address in every lane (scalar loads).  Nothing is shared
// between threads: no LDS, no barrier; several columns' loads are in flight per thread.
// part[2 * ((by * NR + k) * n + i)] = the slice's share of (A X)[i, k].
constexpr int CRF_ROWS = 256, CRF_MIN_CJ = 32, CRF_TARGET_WGS = 2048;

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

// R[i, k] = B[i, k] - (the slices' shares in slice order), the two parts on their own
__global__ void __launch_bounds__(256) cresidual_combine_kernel(int n, int nr, int splits, const double* __restrict__ part,
                                                                const double* __restrict__ B, int64_t ldb, double* __restrict__ R, int64_t ldr)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int k = blockIdx.y;
    if (i >= n) return;
    double sre = 0.0, sim = 0.0;
#pragma unroll 8
    for (int sp = 0; sp < splits; ++sp) {
        const double2 t = *reinterpret_cast<const double2*>(part + 2 * (((int64_t)sp * nr + k) * n + i));
        sre += t.x;
        sim += t.y;
    }
    const double* b = B + 2 * (i + k * ldb);
    double* r = R + 2 * (i + k * ldr);
    r[0] = b[0] - sre;
    r[1] = b[1] - sim;
}

template <int NR>
static void launch_cresidual_nr(hipStream_t st, dim3 grid, bool vec, int n, int cj, const double* A, int64_t lda, const double* X, int64_t ldx,
                                double* part)
{
    if (vec) hipLaunchKernelGGL((cresidual_few_kernel<NR, true>), grid, dim3(256), 0, st, n, cj, A, lda, X, ldx, part);
    else     hipLaunchKernelGGL((cresidual_few_kernel<NR, false>), grid, dim3(256), 0, st, n, cj, A, lda, X, ldx, part);
}

int launch_cresidual_few(Handle* h, int64_t n, int64_t nrhs, const double* A, int64_t lda, const double* X, int64_t ldx, const double* B,
                         int64_t ldb, double* R, int64_t ldr)
{
    if (n <= 0 || nrhs <= 0) return RFLU_OK;
    if (nrhs > RESIDUAL_PASS) { set_error("cresidual_few: at most %d right-hand sides per pass", RESIDUAL_PASS); return RFLU_ERR_ARG; }
    // the split is a function of n alone (the results do not depend on the device or on what else runs)
    const int64_t rb = (n + CRF_ROWS - 1) / CRF_ROWS;
    int64_t splits = std::max<int64_t>(1, std::min<int64_t>((n + CRF_MIN_CJ - 1) / CRF_MIN_CJ, (CRF_TARGET_WGS + rb - 1) / rb));
    const int64_t cj = ((n + splits - 1) / splits + 7) / 8 * 8;
    splits = (n + cj - 1) / cj;
    if (splits > 65535) { set_error("cresidual_few: n = %lld is too large", (long long)n); return RFLU_ERR_ARG; }
    RFLU_TRY(ensure_buffer(&h->mixed_part, &h->mixed_part_bytes, (size_t)(splits * nrhs * n) * 2 * sizeof(double)));
    double* part = static_cast<double*>(h->mixed_part);
    const bool vec = reinterpret_cast<uintptr_t>(A) % 16 == 0;
    const dim3 grid((unsigned)rb, (unsigned)splits);
    {
        ProfScope ps(h, RFLU_K_MISC, 8.0 * (double)n * (double)n * (double)nrhs, 16.0 * (double)n * (double)n);
        switch (nrhs) {
            case 1: launch_cresidual_nr<1>(h->stream, grid, vec, (int)n, (int)cj, A, lda, X, ldx, part); break;
            case 2: launch_cresidual_nr<2>(h->stream, grid, vec, (int)n, (int)cj, A, lda, X, ldx, part); break;
            case 3: launch_cresidual_nr<3>(h->stream, grid, vec, (int)n, (int)cj, A, lda, X, ldx, part); break;
            case 4: launch_cresidual_nr<4>(h->stream, grid, vec, (int)n, (int)cj, A, lda, X, ldx, part); break;
            case 5: launch_cresidual_nr<5>(h->stream, grid, vec, (int)n, (int)cj, A, lda, X, ldx, part); break;
            case 6: launch_cresidual_nr<6>(h->stream, grid, vec, (int)n, (int)cj, A, lda, X, ldx, part); break;
            case 7: launch_cresidual_nr<7>(h->stream, grid, vec, (int)n, (int)cj, A, lda, X, ldx, part); break;
            default: launch_cresidual_nr<8>(h->stream, grid, vec, (int)n, (int)cj, A, lda, X, ldx, part); break;
        }
        RFLU_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(cresidual_combine_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)nrhs), dim3(256), 0, h->stream, (int)n, (int)nrhs,
                       (int)splits, part, B, ldb, R, ldr);
    RFLU_HIP(hipGetLastError());
    return RFLU_OK;
}

// ---- the small kernels -------------------------------------------------------------------------------------------------------------
// out[i, k] (+)= (TO) in[i, k], both column-major n x nrhs complex: the few-right-hand-side solve works on columns, so the Float32
// right-hand sides keep the layout of B and X and only the element type changes
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

// out[r][c] (+)= (TO) in[c][r] on complex elements: convert_transpose_kernel (mixed.hip) with the 32 x 33 tile of ctranspose_kernel and
// its numbering of the tiles along blockIdx.x alone.  A column-major n x nrhs block IS a row-major nrhs x n one.
template <typename TI, typename TO, bool ADD>
__global__ void __launch_bounds__(256) cconvert_transpose_kernel(int64_t rows_out, int64_t cols_out, const TI* __restrict__ in, int64_t ld_in,
                                                                 TO* __restrict__ out, int64_t ld_out, unsigned tiles_x)
{
    __shared__ TO tile[32][33][2];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int64_t r0 = (int64_t)(blockIdx.x / tiles_x) * 32, c0 = (int64_t)(blockIdx.x % tiles_x) * 32;
    for (int i = ty; i < 32; i += 8) {
        const int64_t ir = c0 + i, ic = r0 + tx;
        const bool ok = ir < cols_out && ic < rows_out;
        tile[i][tx][0] = ok ? (TO)in[2 * (ir * ld_in + ic)] : TO(0);
        tile[i][tx][1] = ok ? (TO)in[2 * (ir * ld_in + ic) + 1] : TO(0);
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        const int64_t orow = r0 + i, ocol = c0 + tx;
        if (orow < rows_out && ocol < cols_out) {
            TO* q = out + 2 * (orow * ld_out + ocol);
            if (ADD) {
                q[0] += tile[tx][i][0];
                q[1] += tile[tx][i][1];
            } else {
                q[0] = tile[tx][i][0];
                q[1] = tile[tx][i][1];
            }
        }
    }
}

template <typename TI, typename TO>
int launch_cconvert_transpose(Handle* h, int64_t rows_out, int64_t cols_out, const TI* in, int64_t ld_in, TO* out, int64_t ld_out, bool add)
{
    if (rows_out <= 0 || cols_out <= 0) return RFLU_OK;
    const int64_t gx = (cols_out + 31) / 32, gy = (rows_out + 31) / 32;
    if (gx > INT32_MAX || gy > INT32_MAX || gx * gy > INT32_MAX) {
        set_error("complex right-hand side conversion: %lld x %lld is beyond one launch", (long long)rows_out, (long long)cols_out);
        return RFLU_ERR_ARG;
    }
    const dim3 grid((unsigned)(gx * gy));
    if (add) hipLaunchKernelGGL((cconvert_transpose_kernel<TI, TO, true>), grid, dim3(256), 0, h->stream, rows_out, cols_out, in, ld_in, out, ld_out, (unsigned)gx);
    else     hipLaunchKernelGGL((cconvert_transpose_kernel<TI, TO, false>), grid, dim3(256), 0, h->stream, rows_out, cols_out, in, ld_in, out, ld_out, (unsigned)gx);
    RFLU_HIP(hipGetLastError());
    return RFLU_OK;
}
template int launch_cconvert_transpose<double, float>(Handle*, int64_t, int64_t, const double*, int64_t, float*, int64_t, bool);
template int launch_cconvert_transpose<float, double>(Handle*, int64_t, int64_t, const float*, int64_t, double*, int64_t, bool);

// norms[2k] = ||r_k||_inf, norms[2k + 1] = ||x_k||_inf as the largest modulus; one workgroup per column
__global__ void __launch_bounds__(256) ccolnorms_kernel(int64_t n, const double* __restrict__ R, int64_t ldr, const double* __restrict__ X,
                                                        int64_t ldx, double* __restrict__ norms)
{
    __shared__ double sh[256];
    const int64_t k = blockIdx.x;
    double rn = 0.0, xn = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        const double* r = R + 2 * (i + k * ldr);
        const double* x = X + 2 * (i + k * ldx);
        rn = nanmax(rn, cmodulus(Cx<double>{r[0], r[1]}));
        xn = nanmax(xn, cmodulus(Cx<double>{x[0], x[1]}));
    }
    rn = block_nanmax(rn, sh);
    __syncthreads();
    xn = block_nanmax(xn, sh);
    if (threadIdx.x == 0) {
        norms[2 * k] = rn;
        norms[2 * k + 1] = xn;
    }
}

int launch_ccolnorms(Handle* h, int64_t n, int64_t nrhs, const double* R, int64_t ldr, const double* X, int64_t ldx, double* norms)
{
    if (n <= 0 || nrhs <= 0) return RFLU_OK;
    hipLaunchKernelGGL(ccolnorms_kernel, dim3((unsigned)nrhs), dim3(256), 0, h->stream, n, R, ldr, X, ldx, norms);
    RFLU_HIP(hipGetLastError());
    return RFLU_OK;
}

}  // namespace rflu
