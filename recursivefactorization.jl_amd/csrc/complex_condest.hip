// complex_condest.hip -- operator norms (LAPACK zlange / clange, 1 and Inf) of ComplexF64 / ComplexF32 matrices and the vector kernels of
// the complex condition estimate (LAPACK zgecon / cgecon; the driver loop is cgecon_dev in driver.cpp, the batched estimator
// cgecon_batched_kernel in batched_complex.hip).  DESIGN.md section 4.12.  condest.hip with "element" read as COMPLEX element: a matrix is
// R* (R = double / float) at interleaved (re, im) pairs, every ld counts complex elements, a pointer aligned to R is enough.
//
// |a| = hypot(re, im) in Float64 (ComplexF32 parts are converted first), except that a NaN in EITHER part gives NaN: C's hypot(Inf, NaN)
// is Inf, so the parts are tested, not the modulus.  Every sum is Float64 in the ONE order of condest.hip:
//   * along  (column-major 1-norm, row-major Inf-norm): a workgroup per line, the line in chunks of 1024 elements, thread t of 256 owns
//     elements 4t .. 4t+3 of the chunk and adds their moduli in index order, the 64 lanes of a wave add by the tree t += t + s
//     (s = 32 .. 1), the four wave sums in order, the chunk sums in index order;
//   * across (column-major Inf-norm, row-major 1-norm): lanes along the line, a thread owns 16 bytes of positions (one ComplexF64, two
//     ComplexF32), the lines in groups of 256 added in index order, the group sums in index order by the second kernel.
// 16-byte loads where the pointer allows (ComplexF64: A on a 16-byte boundary, then every element is; ComplexF32: also every line start,
// i.e. an even lda), element loads otherwise -- the same additions either way.  Padding (ld > len) is never read.  Then the largest sum,
// a NaN kept.  The batched entry runs one workgroup per matrix for max(m, n) <= 128 with the additions of the kernels above (the lanes
// without data add +0.0), so the results agree bit for bit.
//
// Estimator vectors (x: n contiguous complex elements): ccond_stats gives sum|x_i| in the chunking of cond_stats (chunks of 1024, thread
// t of 256 takes t, t + 256, t + 512, t + 768 in that order, an LDS tree t += t + s for s = 128 .. 1, chunks in index order), a
// non-finite flag, the FIRST index of the largest modulus and |x[jq]|, and can leave the phase vector x_i / |x_i| (1 + 0i for a zero) in
// x; ccond_fill makes the ones vector, e_j and the alternating vector (-1)^i (n - 1 + i).  No kernel here waits for another workgroup.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "complex_dev.hpp"

namespace rflu {

namespace {

constexpr int CLN_THREADS = 256;
constexpr int CLN_CHUNK = 1024;   // complex elements of a line per workgroup pass: four per thread
constexpr int CLN_GROUP = 256;    // lines per partial sum of the across kernel
constexpr int64_t CLN_MAX_GRID = 1 << 22;

__device__ __forceinline__ double cnan_max(double a, double b)
{
    return (a != a) ? a : ((b != b) ? b : (a > b ? a : b));
}

// the modulus the norms and the estimator add: Float64 hypot, NaN when either part is one
template <typename R>
__device__ __forceinline__ double cabs64(R re, R im)
{
    const double x = (double)re, y = (double)im;
    if (x != x || y != y) return __builtin_nan("");
    return hypot(x, y);
}

// complex elements [e0, e0 + 4) of a line below len, moduli added in index order to 0.0; `line` points at element 0 of the line
template <typename R>
__device__ __forceinline__ double cline_quad(const R* __restrict__ line, int64_t e0, int64_t len, bool vec)
{
    double s = 0.0;
    if (vec && e0 + 4 <= len) {
        if (sizeof(R) == 4) {
            const float4 a = *reinterpret_cast<const float4*>(line + 2 * e0);
            const float4 b = *reinterpret_cast<const float4*>(line + 2 * e0 + 4);
            s += cabs64(a.x, a.y); s += cabs64(a.z, a.w); s += cabs64(b.x, b.y); s += cabs64(b.z, b.w);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double2 a = *reinterpret_cast<const double2*>(line + 2 * (e0 + e));
                s += cabs64(a.x, a.y);
            }
        }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e0 + e < len) s += cabs64(line[2 * (e0 + e)], line[2 * (e0 + e) + 1]);
    }
    return s;
}

template <int WIDTH>
__device__ __forceinline__ double cwave_tree(double v)
{
#pragma unroll
    for (int s = WIDTH / 2; s > 0; s >>= 1) v += __shfl_down(v, s, WIDTH);
    return v;
}

// sums[q] = sum of |a| over line q (lines at A + 2*q*ld); a workgroup takes every gridDim.x-th line
template <typename R>
__global__ void __launch_bounds__(CLN_THREADS) clange_along_kernel(const R* __restrict__ A, int64_t ld, int64_t len, int64_t cnt, int vec,
                                                                   double* __restrict__ sums)
{
    __shared__ double sW[2][CLN_THREADS / 64];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    int par = 0;
    for (int64_t q = blockIdx.x; q < cnt; q += gridDim.x) {
        const R* line = A + 2 * (q * ld);
        double acc = 0.0;
        for (int64_t c0 = 0; c0 < len; c0 += CLN_CHUNK, par ^= 1) {
            const double v = cwave_tree<64>(cline_quad<R>(line, c0 + 4 * t, len, vec != 0));
            if (lane == 0) sW[par][w] = v;
            __syncthreads();   // one barrier per chunk: the other half of sW is written next
            if (t == 0) {
                const double cs = ((sW[par][0] + sW[par][1]) + sW[par][2]) + sW[par][3];
                acc = (c0 == 0) ? cs : acc + cs;
            }
        }
        if (t == 0) sums[q] = acc;
    }
}

// part[g * len + p] = sum over the lines q of group g (CLN_GROUP lines, in index order) of |a[p + q*ld]|
template <typename R>
__global__ void __launch_bounds__(CLN_THREADS) clange_across_kernel(const R* __restrict__ A, int64_t ld, int64_t len, int64_t cnt, int vec,
                                                                    double* __restrict__ part)
{
    constexpr int V = 16 / (2 * (int)sizeof(R));   // complex elements per 16 bytes
    const int64_t p0 = ((int64_t)blockIdx.x * CLN_THREADS + threadIdx.x) * V;
    if (p0 >= len) return;
    const int64_t ngroups = (cnt + CLN_GROUP - 1) / CLN_GROUP;
    for (int64_t g = blockIdx.y; g < ngroups; g += gridDim.y) {
        const int64_t q0 = g * CLN_GROUP, q1 = q0 + CLN_GROUP < cnt ? q0 + CLN_GROUP : cnt;
        double s[V];
#pragma unroll
        for (int e = 0; e < V; ++e) s[e] = 0.0;
        if (vec && p0 + V <= len) {
            for (int64_t q = q0; q < q1; ++q) {
                const R* p = A + 2 * (q * ld + p0);
                if (sizeof(R) == 4) {
                    const float4 v = *reinterpret_cast<const float4*>(p);
                    s[0] += cabs64(v.x, v.y);
                    s[V - 1] += cabs64(v.z, v.w);   // V == 2 here
                } else {
                    const double2 v = *reinterpret_cast<const double2*>(p);
                    s[0] += cabs64(v.x, v.y);
                }
            }
        } else {
            for (int64_t q = q0; q < q1; ++q) {
#pragma unroll
                for (int e = 0; e < V; ++e)
                    if (p0 + e < len) {
                        const R* p = A + 2 * (q * ld + p0 + e);
                        s[e] += cabs64(p[0], p[1]);
                    }
            }
        }
#pragma unroll
        for (int e = 0; e < V; ++e)
            if (p0 + e < len) part[g * len + p0 + e] = s[e];
    }
}

// bmax[block] = max over the block's 256 positions p of (part[p] + part[len + p] + ... in group order); a NaN is kept
__global__ void __launch_bounds__(CLN_THREADS) clange_max_kernel(const double* __restrict__ part, int64_t ngroups, int64_t len,
                                                                 double* __restrict__ bmax)
{
    __shared__ double sM[CLN_THREADS];
    const int t = threadIdx.x;
    const int64_t p = (int64_t)blockIdx.x * CLN_THREADS + t;
    double v = 0.0;
    if (p < len) {
        v = part[p];
        for (int64_t g = 1; g < ngroups; ++g) v += part[g * len + p];
    }
    sM[t] = v;
    __syncthreads();
    for (int s = CLN_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) sM[t] = cnan_max(sM[t], sM[t + s]);
        __syncthreads();
    }
    if (t == 0) bmax[blockIdx.x] = sM[0];
}

__global__ void __launch_bounds__(CLN_THREADS) clange_final_kernel(const double* __restrict__ bmax, int64_t nblocks, double* __restrict__ out)
{
    __shared__ double sM[CLN_THREADS];
    const int t = threadIdx.x;
    double v = 0.0;
    for (int64_t i = t; i < nblocks; i += CLN_THREADS) v = cnan_max(v, bmax[i]);
    sM[t] = v;
    __syncthreads();
    for (int s = CLN_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) sM[t] = cnan_max(sM[t], sM[t + s]);
        __syncthreads();
    }
    if (t == 0) out[0] = sM[0];
}

// one workgroup per matrix, len <= 128 and cnt <= 128: the additions of the kernels above (see the head of the file)
template <typename R>
__global__ void __launch_bounds__(CLN_THREADS) clange_small_batched_kernel(const R* __restrict__ A, int64_t ld, int64_t strideA, int len,
                                                                           int cnt, int along, double* __restrict__ out)
{
    __shared__ double sM[CLN_THREADS];
    const int t = threadIdx.x;
    const R* Ab = A + 2 * ((int64_t)blockIdx.x * strideA);
    double best = 0.0;
    if (along) {
        const int l32 = t & 31, half = t >> 5;   // a half-wave per line, eight lines per pass
        for (int q0 = 0; q0 < cnt; q0 += CLN_THREADS / 32) {
            const int q = q0 + half;
            double v = 0.0;
            if (q < cnt) v = cline_quad<R>(Ab + 2 * ((int64_t)q * ld), 4 * l32, len, false);
            v = cwave_tree<32>(v);
            if (q < cnt && l32 == 0) best = cnan_max(best, v);
        }
    } else if (t < len) {
        double s = 0.0;
        for (int q = 0; q < cnt; ++q) {
            const R* p = Ab + 2 * ((int64_t)q * ld + t);
            s += cabs64(p[0], p[1]);
        }
        best = s;
    }
    sM[t] = best;
    __syncthreads();
    for (int s = CLN_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) sM[t] = cnan_max(sM[t], sM[t + s]);
        __syncthreads();
    }
    if (t == 0) out[blockIdx.x] = sM[0];
}

// ---- the estimator's vectors ------------------------------------------------------------------------------------------------------
constexpr int CCS_THREADS = 256;
constexpr int CCS_CHUNK = 1024;

struct CcsPart {
    double sum;
    double maxabs;     // -1: no comparable entry yet
    long long argmax;
    int nonfinite;
    int pad;
};

__device__ __forceinline__ void ccs_take(double& m, long long& a, double om, long long oa)
{
    if (om > m || (om == m && oa < a)) { m = om; a = oa; }
}

template <typename R>
__global__ void __launch_bounds__(CCS_THREADS) ccond_stats_kernel(R* __restrict__ x, int64_t n, int write_phase, CcsPart* __restrict__ part)
{
    __shared__ double sSum[CCS_THREADS];
    __shared__ double sMax[CCS_THREADS];
    __shared__ long long sArg[CCS_THREADS];
    __shared__ int sNf[CCS_THREADS];
    const int t = threadIdx.x;
    double sum = 0.0, mx = -1.0;
    long long am = (long long)n;
    int nf = 0;
#pragma unroll
    for (int k = 0; k < CCS_CHUNK / CCS_THREADS; ++k) {
        const int64_t i = (int64_t)blockIdx.x * CCS_CHUNK + k * CCS_THREADS + t;
        if (i < n) {
            const R re = x[2 * i], im = x[2 * i + 1];
            const double a = cabs64(re, im);
            sum += a;
            if (!(a < __builtin_inf())) nf = 1;
            if (a > mx) { mx = a; am = i; }
            if (write_phase) {   // x_i / |x_i|: two Float64 quotients rounded to the element type; 1 + 0i for a zero
                const bool z = re == R(0) && im == R(0);
                x[2 * i] = z ? R(1) : (R)((double)re / a);
                x[2 * i + 1] = z ? R(0) : (R)((double)im / a);
            }
        }
    }
    sSum[t] = sum; sMax[t] = mx; sArg[t] = am; sNf[t] = nf;
    __syncthreads();
    for (int s = CCS_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) {
            sSum[t] += sSum[t + s];
            ccs_take(sMax[t], sArg[t], sMax[t + s], sArg[t + s]);
            sNf[t] |= sNf[t + s];
        }
        __syncthreads();
    }
    if (t == 0) {
        CcsPart p;
        p.sum = sSum[0]; p.maxabs = sMax[0]; p.argmax = sArg[0]; p.nonfinite = sNf[0]; p.pad = 0;
        part[blockIdx.x] = p;
    }
}

// xj_abs: |x[jq]| as it stood BEFORE the statistics kernel (which may have replaced x by its phases), captured here first
template <typename R>
__global__ void __launch_bounds__(64) ccond_peek_kernel(const R* __restrict__ x, int64_t jq, double* __restrict__ xj_abs)
{
    if (threadIdx.x == 0) xj_abs[0] = jq >= 0 ? cabs64(x[2 * jq], x[2 * jq + 1]) : 0.0;
}

__global__ void __launch_bounds__(64) ccond_final_kernel(const CcsPart* __restrict__ part, int64_t nchunks, const double* __restrict__ xj_abs,
                                                         CondStats* __restrict__ res)
{
    if (threadIdx.x != 0) return;
    CcsPart acc = part[0];
    for (int64_t c = 1; c < nchunks; ++c) {
        const CcsPart p = part[c];
        acc.sum += p.sum;
        ccs_take(acc.maxabs, acc.argmax, p.maxabs, p.argmax);
        acc.nonfinite |= p.nonfinite;
    }
    CondStats r;
    r.sum = acc.sum; r.maxabs = acc.maxabs; r.xj_abs = xj_abs[0]; r.argmax = acc.argmax; r.differs = 0; r.nonfinite = acc.nonfinite;
    res[0] = r;
}

template <typename R>
__global__ void __launch_bounds__(256) ccond_fill_kernel(R* __restrict__ x, int64_t n, int mode, int64_t j)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    R v;
    if (mode == COND_FILL_ONES) v = R(1);
    else if (mode == COND_FILL_UNIT) v = (i == j) ? R(1) : R(0);
    else {
        const R a = (R)(double)(n - 1 + i);   // exact in Float32 below 2^24
        v = (i & 1) ? -a : a;
    }
    x[2 * i] = v;
    x[2 * i + 1] = R(0);
}

inline size_t cup16(size_t v) { return (v + 15) & ~(size_t)15; }

}  // namespace

template <typename R>
int launch_clange(Handle* h, int norm, int64_t m, int64_t n, const R* A, int64_t lda, int row_major, double* out)
{
    *out = 0.0;
    if (m == 0 || n == 0) return RFLU_OK;
    const int64_t len = row_major ? n : m, cnt = row_major ? m : n;
    const bool along = (norm == RFLU_NORM_ONE) != (row_major != 0);
    if (cnt > 0x7fffffffLL || len > 0x7fffffffLL) {   // the second kernel runs one thread per sum: 2^31 of them at most
        set_error("complex lange: %lld x %lld has more than 2^31 - 1 rows or columns", (long long)m, (long long)n);
        return RFLU_ERR_ARG;
    }
    // ComplexF64: an element is 16 bytes, an aligned A aligns them all; ComplexF32: every line has to start on a 16-byte boundary too
    const int vec = (reinterpret_cast<uintptr_t>(A) % 16 == 0 && (lda * 2 * sizeof(R)) % 16 == 0) ? 1 : 0;
    const int64_t ngroups = along ? 1 : (cnt + CLN_GROUP - 1) / CLN_GROUP;
    const int64_t nsums = along ? cnt : len;
    const int64_t nblocks = (nsums + CLN_THREADS - 1) / CLN_THREADS;
    const size_t part_bytes = cup16((size_t)ngroups * (size_t)nsums * sizeof(double));
    const size_t bmax_bytes = cup16((size_t)nblocks * sizeof(double));
    RFLU_TRY(ensure_buffer(&h->cond_work, &h->cond_work_bytes, part_bytes + bmax_bytes + 16));
    char* base = static_cast<char*>(h->cond_work);
    double* part = reinterpret_cast<double*>(base);
    double* bmax = reinterpret_cast<double*>(base + part_bytes);
    double* res = reinterpret_cast<double*>(base + part_bytes + bmax_bytes);
    {
        ProfScope ps(h, RFLU_K_MISC, (double)m * (double)n, (double)m * (double)n * 2 * sizeof(R));
        if (along) {
            hipLaunchKernelGGL(clange_along_kernel<R>, dim3((unsigned)std::min<int64_t>(cnt, CLN_MAX_GRID)), dim3(CLN_THREADS), 0, h->stream, A, lda,
                               len, cnt, vec, part);
        } else {
            const int64_t per_block = (int64_t)CLN_THREADS * (16 / (2 * (int)sizeof(R)));
            hipLaunchKernelGGL(clange_across_kernel<R>, dim3((unsigned)((len + per_block - 1) / per_block), (unsigned)std::min<int64_t>(ngroups, 65535)),
                               dim3(CLN_THREADS), 0, h->stream, A, lda, len, cnt, vec, part);
        }
        hipLaunchKernelGGL(clange_max_kernel, dim3((unsigned)nblocks), dim3(CLN_THREADS), 0, h->stream, part, ngroups, nsums, bmax);
        hipLaunchKernelGGL(clange_final_kernel, dim3(1), dim3(CLN_THREADS), 0, h->stream, bmax, nblocks, res);
        RFLU_HIP(hipGetLastError());
    }
    RFLU_HIP(hipMemcpyAsync(out, res, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    RFLU_HIP(hipStreamSynchronize(h->stream));
    return RFLU_OK;
}

template <typename R>
int launch_clange_batched(Handle* h, int norm, int64_t batch, int64_t m, int64_t n, const R* A, int64_t lda, int64_t strideA, int row_major,
                          double* out_dev)
{
    const int64_t len = row_major ? n : m, cnt = row_major ? m : n;
    const bool along = (norm == RFLU_NORM_ONE) != (row_major != 0);
    if (std::max(m, n) <= BATCHED_MAX_DIM) {
        ProfScope ps(h, RFLU_K_MISC, (double)batch * (double)m * (double)n, (double)batch * (double)m * (double)n * 2 * sizeof(R));
        hipLaunchKernelGGL(clange_small_batched_kernel<R>, dim3((unsigned)batch), dim3(CLN_THREADS), 0, h->stream, A, lda, strideA, (int)len,
                           (int)cnt, along ? 1 : 0, out_dev);
        RFLU_HIP(hipGetLastError());
        return RFLU_OK;
    }
    for (int64_t b = 0; b < batch; ++b) {   // the single entry's kernels, matrix by matrix: the same bits
        double v = 0.0;
        RFLU_TRY(launch_clange<R>(h, norm, m, n, A + 2 * b * strideA, lda, row_major, &v));
        RFLU_HIP(hipMemcpyAsync(out_dev + b, &v, sizeof(double), hipMemcpyHostToDevice, h->stream));
        RFLU_HIP(hipStreamSynchronize(h->stream));   // `v` is pageable and reused
    }
    return RFLU_OK;
}

template <typename R>
int launch_ccond_fill(Handle* h, int64_t n, R* x, int mode, int64_t j)
{
    ProfScope ps(h, RFLU_K_MISC, (double)n, (double)n * 2 * sizeof(R));
    hipLaunchKernelGGL(ccond_fill_kernel<R>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, x, n, mode, j);
    RFLU_HIP(hipGetLastError());
    return RFLU_OK;
}

template <typename R>
int launch_ccond_stats(Handle* h, int64_t n, R* x, int64_t jq, int write_phase, CondStats* out)
{
    const int64_t nchunks = (n + CCS_CHUNK - 1) / CCS_CHUNK;
    const size_t part_bytes = cup16((size_t)nchunks * sizeof(CcsPart));
    RFLU_TRY(ensure_buffer(&h->inv_part, &h->inv_part_bytes, part_bytes + 16 + sizeof(CondStats)));
    CcsPart* part = static_cast<CcsPart*>(h->inv_part);
    double* xj = reinterpret_cast<double*>(static_cast<char*>(h->inv_part) + part_bytes);
    CondStats* res = reinterpret_cast<CondStats*>(static_cast<char*>(h->inv_part) + part_bytes + 16);
    {
        ProfScope ps(h, RFLU_K_MISC, (double)n, 4.0 * (double)n * sizeof(R));
        hipLaunchKernelGGL(ccond_peek_kernel<R>, dim3(1), dim3(64), 0, h->stream, x, jq, xj);
        hipLaunchKernelGGL(ccond_stats_kernel<R>, dim3((unsigned)nchunks), dim3(CCS_THREADS), 0, h->stream, x, n, write_phase, part);
        hipLaunchKernelGGL(ccond_final_kernel, dim3(1), dim3(64), 0, h->stream, part, nchunks, xj, res);
        RFLU_HIP(hipGetLastError());
    }
    RFLU_HIP(hipMemcpyAsync(out, res, sizeof(CondStats), hipMemcpyDeviceToHost, h->stream));
    RFLU_HIP(hipStreamSynchronize(h->stream));
    return RFLU_OK;
}

template int launch_clange<double>(Handle*, int, int64_t, int64_t, const double*, int64_t, int, double*);
template int launch_clange<float>(Handle*, int, int64_t, int64_t, const float*, int64_t, int, double*);
template int launch_clange_batched<double>(Handle*, int, int64_t, int64_t, int64_t, const double*, int64_t, int64_t, int, double*);
template int launch_clange_batched<float>(Handle*, int, int64_t, int64_t, int64_t, const float*, int64_t, int64_t, int, double*);
template int launch_ccond_fill<double>(Handle*, int64_t, double*, int, int64_t);
template int launch_ccond_fill<float>(Handle*, int64_t, float*, int, int64_t);
template int launch_ccond_stats<double>(Handle*, int64_t, double*, int64_t, int, CondStats*);
template int launch_ccond_stats<float>(Handle*, int64_t, float*, int64_t, int, CondStats*);

}  // namespace rflu
