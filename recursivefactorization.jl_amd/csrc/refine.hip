// refine.hip -- the kernels of iterative refinement with error bounds (LAPACK xGERFS, trans = 'N'; rflu_gerfs_* / rflu_berr_*, the loop
// is gerfs_dev in driver.cpp) for Float64 and Float32 elements.
//
//   absresidual_few   for up to REFINE_PASS right-hand sides BOTH sums of a refinement step in ONE pass over A (column-major, read in
//                     place exactly once): acc = sum a_ij x_j and accw = sum |a_ij| |x_j|, in Float64 for both element types, one fused
//                     multiply-add per term and sum.  The geometry is residual_few's (mixed.hip): 512-row workgroups x column slices,
//                     rows the coalesced direction, the split a function of n alone.
//   absresidual_combine  the slices' shares in slice order -> r = b - A x and w = |b| + |A| |x| (Float64, n x REFINE_PASS) and (T) r as
//                     the row-major n x REFINE_PASS block the cooperative solve takes: no transpose kernel per step.
//   berr_reduce       per column the NaN-keeping maximum of |r_i| / w_i and of |x_i| by a fixed tree.
//   the small ones    the masked update X[:, k] += d[:, k] from the row-major block, the weights wt = (T)(|r| + (n + 1) u w) of the
//                     forward error bound, x o= wt.
//
// Everything is a plain in-order launch on the handle's stream: no kernel waits for another workgroup, there are no floating-point
// atomics, and every sum has a fixed order, so results repeat bit for bit.  The 16-byte and the element-wise form of absresidual_few add
// the same numbers in the same order: the results do not depend on alignment or on the leading dimensions.
// Roofline: HBM for the matrix pass (sizeof(T) n^2 bytes per pass against 4 n^2 nr flops); the small kernels are latency.
#include <algorithm>

#include "rflu_internal.hpp"

namespace rflu {

namespace {

// max that keeps a NaN once it has seen one (fmax drops it)
__device__ __forceinline__ double keepmax(double m, double v) { return (v > m || v != v) ? v : m; }

// all 256 threads of the workgroup call it; thread 0 holds the result (fixed tree: the same order every run)
__device__ __forceinline__ double block_keepmax(double v, double* sh)
{
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] = keepmax(sh[threadIdx.x], sh[threadIdx.x + s]);
        __syncthreads();
    }
    return sh[0];
}

// ---- absresidual_few ---------------------------------------------------------------------------------------------------------------
// Workgroup (bx, by): rows [512 bx, 512 bx + 512) x columns [cj by, cj by + cj).  A thread owns RPT = 16 / sizeof(T) rows (VEC: adjacent,
// one 16-byte load per column; otherwise rows t, t + TH, ...) and NR right-hand sides, so a workgroup is TH = 512 / RPT threads: 256 for
// Float64 as residual_few, 128 for Float32, whose loads stay 16 bytes (four rows).  Per thread 2 RPT NR Float64 accumulators (NR = 8: 32
// for Float64, 64 for Float32), two fma per element and right-hand side, the columns in ascending order; |a| and |x| are source
// modifiers of the second fma.  X[j, k] has the same address in every lane (scalar loads).  No LDS, no barrier.
// part[((by * 2 + s) * NR + k) * n + i] = the slice's share of (A X)[i, k] (s = 0) and of (|A| |X|)[i, k] (s = 1).
constexpr int AR_ROWS = 512, AR_MIN_CJ = 32, AR_TARGET_WGS = 2048;   // residual_few's RF_ROWS, RF_MIN_CJ, RF_TARGET_WGS

template <typename T> struct Vec16;
template <> struct Vec16<double> { typedef double2 type; };
template <> struct Vec16<float> { typedef float4 type; };

template <typename T, int NR, bool VEC, bool FULL>
__device__ __forceinline__ void absresidual_slice(int n, const int64_t (&row)[16 / sizeof(T)], int64_t jbeg, int64_t jend,
                                                  const T* __restrict__ A, int64_t lda, const T* __restrict__ X, int64_t ldx,
                                                  double (&acc)[16 / sizeof(T)][NR], double (&accw)[16 / sizeof(T)][NR])
{
    constexpr int RPT = 16 / sizeof(T);
    bool ok[RPT];
#pragma unroll
    for (int q = 0; q < RPT; ++q) ok[q] = FULL || row[q] < n;
    // columns in flight per thread: as residual_few, 8, or 4 where 8 columns' X values no longer fit the scalar file
#pragma unroll(NR <= 4 ? 8 : 4)
    for (int64_t j = jbeg; j < jend; ++j) {
        const T* col = A + j * lda;
        double v[RPT];
        if (VEC && ok[RPT - 1]) {
            const typename Vec16<T>::type t = *reinterpret_cast<const typename Vec16<T>::type*>(col + row[0]);
            const T* e = reinterpret_cast<const T*>(&t);
#pragma unroll
            for (int q = 0; q < RPT; ++q) v[q] = (double)e[q];
        } else {
#pragma unroll
            for (int q = 0; q < RPT; ++q) v[q] = ok[q] ? (double)col[row[q]] : 0.0;
        }
#pragma unroll
        for (int k = 0; k < NR; ++k) {
            const double x = (double)X[j + k * ldx];
#pragma unroll
            for (int q = 0; q < RPT; ++q) {
                acc[q][k] = fma(v[q], x, acc[q][k]);
                accw[q][k] = fma(__builtin_fabs(v[q]), __builtin_fabs(x), accw[q][k]);
            }
        }
    }
}

template <typename T, int NR, bool VEC>
__global__ void __launch_bounds__(AR_ROWS / (16 / sizeof(T))) absresidual_few_kernel(int n, int cj, const T* __restrict__ A, int64_t lda,
                                                                                     const T* __restrict__ X, int64_t ldx,
                                                                                     double* __restrict__ part)
{
    constexpr int RPT = 16 / sizeof(T), TH = AR_ROWS / RPT;
    const int t = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * AR_ROWS;
    int64_t row[RPT];
#pragma unroll
    for (int q = 0; q < RPT; ++q) row[q] = i0 + (VEC ? RPT * t + q : t + q * TH);
    const int64_t jbeg = (int64_t)blockIdx.y * cj, jend = jbeg + cj < n ? jbeg + cj : n;
    double acc[RPT][NR], accw[RPT][NR];
#pragma unroll
    for (int q = 0; q < RPT; ++q)
#pragma unroll
        for (int k = 0; k < NR; ++k) acc[q][k] = accw[q][k] = 0.0;
    if (i0 + AR_ROWS <= n) absresidual_slice<T, NR, VEC, true>(n, row, jbeg, jend, A, lda, X, ldx, acc, accw);
    else                   absresidual_slice<T, NR, VEC, false>(n, row, jbeg, jend, A, lda, X, ldx, acc, accw);
    double* p = part + (int64_t)blockIdx.y * 2 * NR * n;
#pragma unroll
    for (int k = 0; k < NR; ++k)
#pragma unroll
        for (int q = 0; q < RPT; ++q)
            if (row[q] < n) {
                p[(int64_t)k * n + row[q]] = acc[q][k];
                p[(int64_t)(NR + k) * n + row[q]] = accw[q][k];
            }
}

// column k of the pass (blockIdx.y < REFINE_PASS): k < nr: the slices' shares in slice order, then r, w and the solve's block; the
// columns behind the last right-hand side of a short pass are zeros in the block (the solve always takes REFINE_PASS columns)
template <typename T>
__global__ void __launch_bounds__(256) absresidual_combine_kernel(int n, int nr, int splits, const double* __restrict__ part,
                                                                  const T* __restrict__ B, int64_t ldb, double* __restrict__ R,
                                                                  double* __restrict__ Wt, T* __restrict__ D)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int k = blockIdx.y;
    if (i >= n) return;
    if (k >= nr) {
        if (D) D[i * REFINE_LDD + k] = T(0);
        return;
    }
    double s = 0.0, sw = 0.0;
#pragma unroll 8
    for (int sp = 0; sp < splits; ++sp) {
        const double* t = part + ((int64_t)sp * 2 * nr + k) * n + i;
        s += t[0];
        sw += t[(int64_t)nr * n];
    }
    const double b = (double)B[i + k * ldb];
    const double r = b - s;
    R[i + (int64_t)k * n] = r;
    Wt[i + (int64_t)k * n] = __builtin_fabs(b) + sw;
    if (D) D[i * REFINE_LDD + k] = (T)r;
}

// one workgroup per column: thread t takes rows t, t + 256, ... in ascending order, then the tree
template <typename T>
__global__ void __launch_bounds__(256) berr_reduce_kernel(int64_t n, const double* __restrict__ R, const double* __restrict__ Wt,
                                                          const T* __restrict__ X, int64_t ldx, double* __restrict__ out)
{
    __shared__ double sh[256];
    const int64_t k = blockIdx.x;
    double be = 0.0, xm = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        const double r = R[i + k * n], w = Wt[i + k * n];
        be = keepmax(be, w == 0.0 ? 0.0 : __builtin_fabs(r) / w);   // w == 0: every term of the row is zero, and so is r
        xm = keepmax(xm, __builtin_fabs((double)X[i + k * ldx]));
    }
    be = block_keepmax(be, sh);
    __syncthreads();
    xm = block_keepmax(xm, sh);
    if (threadIdx.x == 0) {
        out[2 * k] = be;
        out[2 * k + 1] = xm;
    }
}

template <typename T>
__global__ void __launch_bounds__(256) refine_update_kernel(int64_t n, unsigned mask, const T* __restrict__ D, T* __restrict__ X, int64_t ldx)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int k = blockIdx.y;
    if (i >= n || !((mask >> k) & 1u)) return;
    X[i + k * ldx] += D[i * REFINE_LDD + k];
}

template <typename T>
__global__ void __launch_bounds__(256) refine_weights_kernel(int64_t n, double nu, const double* __restrict__ r, const double* __restrict__ w,
                                                             T* __restrict__ wt)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) wt[i] = (T)(__builtin_fabs(r[i]) + nu * w[i]);
}

template <typename T>
__global__ void __launch_bounds__(256) refine_scale_kernel(int64_t n, const T* __restrict__ wt, T* __restrict__ x)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) x[i] *= wt[i];
}

template <typename T, int NR>
void launch_absresidual_nr(hipStream_t st, dim3 grid, bool vec, int n, int cj, const T* A, int64_t lda, const T* X, int64_t ldx, double* part)
{
    constexpr int TH = AR_ROWS / (16 / sizeof(T));
    if (vec) hipLaunchKernelGGL((absresidual_few_kernel<T, NR, true>), grid, dim3(TH), 0, st, n, cj, A, lda, X, ldx, part);
    else     hipLaunchKernelGGL((absresidual_few_kernel<T, NR, false>), grid, dim3(TH), 0, st, n, cj, A, lda, X, ldx, part);
}

}  // namespace

template <typename T>
int launch_absresidual(Handle* h, int64_t n, int64_t nr, const T* A, int64_t lda, const T* X, int64_t ldx, const T* B, int64_t ldb,
                       double* R, double* Wt, T* D)
{
    if (n <= 0 || nr <= 0) return RFLU_OK;
    if (nr > REFINE_PASS) { set_error("absresidual: at most %d right-hand sides per pass", REFINE_PASS); return RFLU_ERR_ARG; }
    if (n > INT32_MAX) { set_error("absresidual: n = %lld is too large", (long long)n); return RFLU_ERR_ARG; }
    // the split of launch_residual_few (mixed.hip): a function of n alone
    const int64_t rb = (n + AR_ROWS - 1) / AR_ROWS;
    int64_t splits = std::max<int64_t>(1, std::min<int64_t>((n + AR_MIN_CJ - 1) / AR_MIN_CJ, (AR_TARGET_WGS + rb - 1) / rb));
    const int64_t cj = ((n + splits - 1) / splits + 7) / 8 * 8;
    splits = (n + cj - 1) / cj;
    if (splits > 65535) { set_error("absresidual: n = %lld is too large", (long long)n); return RFLU_ERR_ARG; }
    RFLU_TRY(ensure_buffer(&h->mixed_part, &h->mixed_part_bytes, (size_t)(splits * 2 * nr * n) * sizeof(double)));
    double* part = static_cast<double*>(h->mixed_part);
    const bool vec = reinterpret_cast<uintptr_t>(A) % 16 == 0 && (lda * sizeof(T)) % 16 == 0;
    const dim3 grid((unsigned)rb, (unsigned)splits);
    {
        ProfScope ps(h, RFLU_K_MISC, 4.0 * (double)n * (double)n * (double)nr, (double)sizeof(T) * (double)n * (double)n);
        switch (nr) {
            case 1: launch_absresidual_nr<T, 1>(h->stream, grid, vec, (int)n, (int)cj, A, lda, X, ldx, part); break;
            case 2: launch_absresidual_nr<T, 2>(h->stream, grid, vec, (int)n, (int)cj, A, lda, X, ldx, part); break;
            case 3: launch_absresidual_nr<T, 3>(h->stream, grid, vec, (int)n, (int)cj, A, lda, X, ldx, part); break;
            case 4: launch_absresidual_nr<T, 4>(h->stream, grid, vec, (int)n, (int)cj, A, lda, X, ldx, part); break;
            case 5: launch_absresidual_nr<T, 5>(h->stream, grid, vec, (int)n, (int)cj, A, lda, X, ldx, part); break;
            case 6: launch_absresidual_nr<T, 6>(h->stream, grid, vec, (int)n, (int)cj, A, lda, X, ldx, part); break;
            case 7: launch_absresidual_nr<T, 7>(h->stream, grid, vec, (int)n, (int)cj, A, lda, X, ldx, part); break;
            default: launch_absresidual_nr<T, 8>(h->stream, grid, vec, (int)n, (int)cj, A, lda, X, ldx, part); break;
        }
        RFLU_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(absresidual_combine_kernel<T>, dim3((unsigned)((n + 255) / 256), (unsigned)(D ? REFINE_PASS : nr)), dim3(256), 0,
                       h->stream, (int)n, (int)nr, (int)splits, part, B, ldb, R, Wt, D);
    RFLU_HIP(hipGetLastError());
    return RFLU_OK;
}

template <typename T>
int launch_berr_reduce(Handle* h, int64_t n, int64_t nr, const double* R, const double* Wt, const T* X, int64_t ldx, double* out)
{
    if (n <= 0 || nr <= 0) return RFLU_OK;
    hipLaunchKernelGGL(berr_reduce_kernel<T>, dim3((unsigned)nr), dim3(256), 0, h->stream, n, R, Wt, X, ldx, out);
    RFLU_HIP(hipGetLastError());
    return RFLU_OK;
}

template <typename T>
int launch_refine_update(Handle* h, int64_t n, int64_t nr, unsigned mask, const T* D, T* X, int64_t ldx)
{
    if (n <= 0 || nr <= 0 || mask == 0) return RFLU_OK;
    hipLaunchKernelGGL(refine_update_kernel<T>, dim3((unsigned)((n + 255) / 256), (unsigned)nr), dim3(256), 0, h->stream, n, mask, D, X, ldx);
    RFLU_HIP(hipGetLastError());
    return RFLU_OK;
}

template <typename T>
int launch_refine_weights(Handle* h, int64_t n, const double* r, const double* w, T* wt)
{
    if (n <= 0) return RFLU_OK;
    const double u = sizeof(T) == 8 ? 0x1p-53 : 0x1p-24;
    hipLaunchKernelGGL(refine_weights_kernel<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, n, (double)(n + 1) * u, r, w, wt);
    RFLU_HIP(hipGetLastError());
    return RFLU_OK;
}

template <typename T>
int launch_refine_scale(Handle* h, int64_t n, const T* wt, T* x)
{
    if (n <= 0) return RFLU_OK;
    hipLaunchKernelGGL(refine_scale_kernel<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, n, wt, x);
    RFLU_HIP(hipGetLastError());
    return RFLU_OK;
}

#define RFLU_INSTANTIATE_REFINE(T)                                                                                                          \
    template int launch_absresidual<T>(Handle*, int64_t, int64_t, const T*, int64_t, const T*, int64_t, const T*, int64_t, double*, double*, T*); \
    template int launch_berr_reduce<T>(Handle*, int64_t, int64_t, const double*, const double*, const T*, int64_t, double*);                \
    template int launch_refine_update<T>(Handle*, int64_t, int64_t, unsigned, const T*, T*, int64_t);                                       \
    template int launch_refine_weights<T>(Handle*, int64_t, const double*, const double*, T*);                                              \
    template int launch_refine_scale<T>(Handle*, int64_t, const T*, T*);
RFLU_INSTANTIATE_REFINE(double)
RFLU_INSTANTIATE_REFINE(float)

}  // namespace rflu
