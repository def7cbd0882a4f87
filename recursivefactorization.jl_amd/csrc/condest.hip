// condest.hip -- operator norms (LAPACK lange, 1 and Inf) and the vector kernels of the condition estimate (LAPACK gecon; the driver
// loops are gecon_dev / cgecon_dev in driver.cpp, the batched estimators gecon_batched_kernel in batched.hip and cgecon_batched_kernel
// in batched_complex.hip) for Float64, Float32, ComplexF64 and ComplexF32.  DESIGN.md sections 4.11 and 4.12.
//
// ELEMENT means what the element trait E (rflu_internal.hpp) says: for a real matrix one R (R = double / float), for a complex matrix
// one interleaved (re, im) pair of R -- the matrix is R*, every ld, len, stride and index counts complex elements, a pointer aligned to
// R is enough, and |a| = hypot(re, im) in Float64 (ComplexF32 parts are converted first) except that a NaN in EITHER part gives NaN.
//
// Every sum is Float64 for all four element types and is formed in ONE order, whatever the pointer's alignment and the launch geometry:
// no floating-point read-modify-write on memory another workgroup touches, so every run repeats the last one bit for bit, and no kernel
// here waits for another workgroup.
//
// Norms.  Call the contiguous dimension of the matrix a LINE (a column of a column-major matrix, a row of a row-major one): `len`
// elements, `cnt` lines, `ld` apart.  Two kernels serve the four (norm, layout) pairs:
//   * along  (column-major 1-norm, row-major Inf-norm): the sum of |a| over each line.  A workgroup per line (beyond 2^22 lines it takes
//     every 2^22-th); the line in chunks of LN_CHUNK = 1024; thread t of 256 owns elements 4t .. 4t+3 of the chunk and adds them in
//     index order, the 64 lanes of a wave add by the fixed tree t += t + s (s = 32 .. 1), the four wave sums are added in order, the
//     chunk sums in index order;
//   * across (column-major Inf-norm, row-major 1-norm): for each position p of a line the sum over the lines.  Lanes along the line
//     (coalesced), a thread owns 16 bytes of positions (2 Float64, 4 Float32, 1 ComplexF64, 2 ComplexF32); the lines in groups of
//     LN_GROUP = 256, a thread adds a group's lines in index order; the group sums are added in index order by the second kernel.
// 16-byte loads where every line starts on a 16-byte boundary (A aligned to 16 bytes and ld elements a multiple of 16 bytes: for
// ComplexF64 an aligned A is enough, for ComplexF32 an even ld too), element loads otherwise -- the same additions either way.
// Then the largest sum, with a NaN kept (max must not drop it).  Both are one streaming pass over A: HBM bound, (len * cnt) elements
// read once, the partial sums (cnt, or len * cnt / 256 doubles) are noise.  Padding (ld > len) is never read.
// The batched entry runs one workgroup per matrix for max(m, n) <= 128: there a line is one chunk in which only lanes 0 .. 31 of the
// first wave hold data and there is one group of lines, so a 32-lane tree / a plain loop over the lines performs the additions of the
// kernels above (the others add +0.0), and the results agree bit for bit.
//
// Estimator vectors (x and sgn: n contiguous elements): cond_stats gives sum|x_i| (the chunking of logabsdet in inverse.hip: chunks of
// 1024, thread t of 256 takes t, t + 256, t + 512, t + 768 in that order, an LDS tree t += t + s for s = 128 .. 1, chunks in index
// order), a non-finite flag, the FIRST index of max|x_i| and |x[jq]|.  Real elements: also the number of sign changes against sgn, and it
// can leave sign(x) in x and sgn.  Complex elements: there is no sgn, and it can leave the phase vector x_i / |x_i| (1 + 0i for a zero)
// in x.  cond_fill makes the ones vector, e_j and the alternating vector (-1)^i (n - 1 + i).  n elements each: latency, not traffic.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "rflu_internal.hpp"

namespace rflu {

namespace {

constexpr int LN_THREADS = 256;
constexpr int LN_CHUNK = 1024;   // elements of a line per workgroup pass: four per thread
constexpr int LN_GROUP = 256;    // lines per partial sum of the across kernel
constexpr int64_t LN_MAX_GRID = 1 << 22;   // workgroups of the along kernel: 2^30 threads, a launch holds fewer than 2^32

template <typename R> struct Vec16;
template <> struct Vec16<double> { typedef double2 type; };
template <> struct Vec16<float> { typedef float4 type; };

__device__ __forceinline__ double nan_max(double a, double b)
{
    return (a != a) ? a : ((b != b) ? b : (a > b ? a : b));
}

// NE elements at p (on a 16-byte boundary) through 16-byte loads, |.| of element e added to s[e * STEP] in index order (STEP 0: one sum)
template <typename E, int NE, int STEP>
__device__ __forceinline__ void add_abs16(const typename E::real* __restrict__ p, double* s)
{
    typedef typename E::real R;
    typedef typename Vec16<R>::type V;
    constexpr int NR = NE * E::PARTS, PER = 16 / (int)sizeof(R);
    alignas(16) R v[NR];
#pragma unroll
    for (int k = 0; k < NR / PER; ++k) reinterpret_cast<V*>(v)[k] = reinterpret_cast<const V*>(p)[k];
#pragma unroll
    for (int e = 0; e < NE; ++e) s[e * STEP] += E::abs(v + E::PARTS * e);
}

// elements [e0, e0 + 4) of a line below len, |.| added in index order to 0.0; `line` points at element 0 of the line
template <typename E>
__device__ __forceinline__ double line_quad(const typename E::real* __restrict__ line, int64_t e0, int64_t len, bool vec)
{
    double s = 0.0;
    if (vec && e0 + 4 <= len) {
        add_abs16<E, 4, 0>(line + E::PARTS * e0, &s);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e0 + e < len) s += E::abs(line + E::PARTS * (e0 + e));
    }
    return s;
}

// the fixed tree of a wave: lane t += lane t + s, s = 32 .. 1 (lane 0 holds the sum); `width` 32 leaves out the first step
template <int WIDTH>
__device__ __forceinline__ double wave_tree(double v)
{
#pragma unroll
    for (int s = WIDTH / 2; s > 0; s >>= 1) v += __shfl_down(v, s, WIDTH);
    return v;
}

// sums[q] = sum of |a| over line q (lines ld elements apart); a workgroup takes every gridDim.x-th line (the grid is capped: a launch
// holds fewer than 2^32 threads)
template <typename E>
__global__ void __launch_bounds__(LN_THREADS) lange_along_kernel(const typename E::real* __restrict__ A, int64_t ld, int64_t len,
                                                                 int64_t cnt, int vec, double* __restrict__ sums)
{
    __shared__ double sW[2][LN_THREADS / 64];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    int par = 0;
    for (int64_t q = blockIdx.x; q < cnt; q += gridDim.x) {
        const typename E::real* line = A + E::PARTS * (q * ld);
        double acc = 0.0;
        for (int64_t c0 = 0; c0 < len; c0 += LN_CHUNK, par ^= 1) {
            const double v = wave_tree<64>(line_quad<E>(line, c0 + 4 * t, len, vec != 0));
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

// part[g * len + p] = sum over the lines q of group g (LN_GROUP lines, in index order) of |a[p + q*ld]|
template <typename E>
__global__ void __launch_bounds__(LN_THREADS) lange_across_kernel(const typename E::real* __restrict__ A, int64_t ld, int64_t len,
                                                                  int64_t cnt, int vec, double* __restrict__ part)
{
    constexpr int P = E::PARTS, V = 16 / (P * (int)sizeof(typename E::real));   // elements per 16 bytes
    const int64_t p0 = ((int64_t)blockIdx.x * LN_THREADS + threadIdx.x) * V;
    if (p0 >= len) return;
    const int64_t ngroups = (cnt + LN_GROUP - 1) / LN_GROUP;
    for (int64_t g = blockIdx.y; g < ngroups; g += gridDim.y) {   // gridDim.y is capped at 65535: a workgroup takes every gridDim.y-th group
        const int64_t q0 = g * LN_GROUP, q1 = q0 + LN_GROUP < cnt ? q0 + LN_GROUP : cnt;
        double s[V];
#pragma unroll
        for (int e = 0; e < V; ++e) s[e] = 0.0;
        if (vec && p0 + V <= len) {
            for (int64_t q = q0; q < q1; ++q) add_abs16<E, V, 1>(A + P * (q * ld + p0), s);
        } else {
            for (int64_t q = q0; q < q1; ++q) {
#pragma unroll
                for (int e = 0; e < V; ++e)
                    if (p0 + e < len) s[e] += E::abs(A + P * (q * ld + p0 + e));
            }
        }
#pragma unroll
        for (int e = 0; e < V; ++e)
            if (p0 + e < len) part[g * len + p0 + e] = s[e];
    }
}

// bmax[block] = max over the block's 256 positions p of (part[p] + part[len + p] + ... in group order); a NaN is kept
__global__ void __launch_bounds__(LN_THREADS) lange_max_kernel(const double* __restrict__ part, int64_t ngroups, int64_t len,
                                                               double* __restrict__ bmax)
{
    __shared__ double sM[LN_THREADS];
    const int t = threadIdx.x;
    const int64_t p = (int64_t)blockIdx.x * LN_THREADS + t;
    double v = 0.0;
    if (p < len) {
        v = part[p];
        for (int64_t g = 1; g < ngroups; ++g) v += part[g * len + p];
    }
    sM[t] = v;
    __syncthreads();
    for (int s = LN_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) sM[t] = nan_max(sM[t], sM[t + s]);
        __syncthreads();
    }
    if (t == 0) bmax[blockIdx.x] = sM[0];
}

__global__ void __launch_bounds__(LN_THREADS) lange_final_kernel(const double* __restrict__ bmax, int64_t nblocks, double* __restrict__ out)
{
    __shared__ double sM[LN_THREADS];
    const int t = threadIdx.x;
    double v = 0.0;
    for (int64_t i = t; i < nblocks; i += LN_THREADS) v = nan_max(v, bmax[i]);
    sM[t] = v;
    __syncthreads();
    for (int s = LN_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) sM[t] = nan_max(sM[t], sM[t + s]);
        __syncthreads();
    }
    if (t == 0) out[0] = sM[0];
}

// one workgroup per matrix, len <= 128 and cnt <= 128: the additions of the kernels above (see the head of the file)
template <typename E>
__global__ void __launch_bounds__(LN_THREADS) lange_small_batched_kernel(const typename E::real* __restrict__ A, int64_t ld,
                                                                         int64_t strideA, int len, int cnt, int along,
                                                                         double* __restrict__ out)
{
    constexpr int P = E::PARTS;
    __shared__ double sM[LN_THREADS];
    const int t = threadIdx.x;
    const typename E::real* Ab = A + P * ((int64_t)blockIdx.x * strideA);
    double best = 0.0;
    if (along) {
        const int l32 = t & 31, half = t >> 5;   // a half-wave per line, eight lines per pass
        for (int q0 = 0; q0 < cnt; q0 += LN_THREADS / 32) {
            const int q = q0 + half;
            double v = 0.0;
            if (q < cnt) v = line_quad<E>(Ab + P * ((int64_t)q * ld), 4 * l32, len, false);
            v = wave_tree<32>(v);
            if (q < cnt && l32 == 0) best = nan_max(best, v);
        }
    } else if (t < len) {
        double s = 0.0;
        for (int q = 0; q < cnt; ++q) s += E::abs(Ab + P * ((int64_t)q * ld + t));
        best = s;
    }
    sM[t] = best;
    __syncthreads();
    for (int s = LN_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) sM[t] = nan_max(sM[t], sM[t + s]);
        __syncthreads();
    }
    if (t == 0) out[blockIdx.x] = sM[0];
}

// ---- the estimator's vectors ------------------------------------------------------------------------------------------------------
constexpr int CS_THREADS = 256;
constexpr int CS_CHUNK = 1024;

struct CsPart {
    double sum;
    double maxabs;     // -1: no finite-comparable entry yet
    long long argmax;
    int differs;       // complex elements: 0
    int nonfinite;
};

__device__ __forceinline__ void cs_take(double& m, long long& a, double om, long long oa)
{
    if (om > m || (om == m && oa < a)) { m = om; a = oa; }
}

// `write`: x (and, real, sgn) <- sign(x) / the phases of x; only the real instantiations read or write sgn and count `differs`
template <typename E>
__global__ void __launch_bounds__(CS_THREADS) cond_stats_kernel(typename E::real* __restrict__ x, typename E::real* __restrict__ sgn,
                                                                int64_t n, int write, CsPart* __restrict__ part)
{
    typedef typename E::real R;
    constexpr bool REAL = E::PARTS == 1;
    __shared__ double sSum[CS_THREADS];
    __shared__ double sMax[CS_THREADS];
    __shared__ long long sArg[CS_THREADS];
    __shared__ int sDif[REAL ? CS_THREADS : 1];   // never touched, so never allocated, for complex elements
    __shared__ int sNf[CS_THREADS];
    const int t = threadIdx.x;
    double sum = 0.0, mx = -1.0;
    long long am = (long long)n;
    int dif = 0, nf = 0;
#pragma unroll
    for (int k = 0; k < CS_CHUNK / CS_THREADS; ++k) {
        const int64_t i = (int64_t)blockIdx.x * CS_CHUNK + k * CS_THREADS + t;
        if (i < n) {
            R* xi = x + E::PARTS * i;
            const R re = xi[0];
            const double a = E::abs(xi);
            sum += a;
            if (!(a < __builtin_inf())) nf = 1;
            if (a > mx) { mx = a; am = i; }
            if constexpr (REAL) {
                const R sv = re >= R(0) ? R(1) : R(-1);
                if (sv != sgn[i]) ++dif;
                if (write) { xi[0] = sv; sgn[i] = sv; }
            } else if (write) {   // x_i / |x_i|: two Float64 quotients rounded to the element type; 1 + 0i for a zero
                const R im = xi[1];
                const bool z = re == R(0) && im == R(0);
                xi[0] = z ? R(1) : (R)((double)re / a);
                xi[1] = z ? R(0) : (R)((double)im / a);
            }
        }
    }
    sSum[t] = sum; sMax[t] = mx; sArg[t] = am;
    if constexpr (REAL) sDif[t] = dif;
    sNf[t] = nf;
    __syncthreads();
    for (int s = CS_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) {
            sSum[t] += sSum[t + s];
            cs_take(sMax[t], sArg[t], sMax[t + s], sArg[t + s]);
            if constexpr (REAL) sDif[t] += sDif[t + s];
            sNf[t] |= sNf[t + s];
        }
        __syncthreads();
    }
    if (t == 0) {
        CsPart p;
        p.sum = sSum[0]; p.maxabs = sMax[0]; p.argmax = sArg[0];
        if constexpr (REAL) p.differs = sDif[0];
        else p.differs = 0;
        p.nonfinite = sNf[0];
        part[blockIdx.x] = p;
    }
}

// xj_abs: |x[jq]| as it stood BEFORE the statistics kernel (which may have replaced x by its signs / phases), captured here first
template <typename E>
__global__ void __launch_bounds__(64) cond_peek_kernel(const typename E::real* __restrict__ x, int64_t jq, double* __restrict__ xj_abs)
{
    if (threadIdx.x == 0) xj_abs[0] = jq >= 0 ? E::abs(x + E::PARTS * jq) : 0.0;
}

__global__ void __launch_bounds__(64) cond_final_kernel(const CsPart* __restrict__ part, int64_t nchunks, const double* __restrict__ xj_abs,
                                                        CondStats* __restrict__ res)
{
    if (threadIdx.x != 0) return;
    CsPart acc = part[0];
    for (int64_t c = 1; c < nchunks; ++c) {
        const CsPart p = part[c];
        acc.sum += p.sum;
        cs_take(acc.maxabs, acc.argmax, p.maxabs, p.argmax);
        acc.differs += p.differs;
        acc.nonfinite |= p.nonfinite;
    }
    CondStats r;
    r.sum = acc.sum; r.maxabs = acc.maxabs; r.xj_abs = xj_abs[0]; r.argmax = acc.argmax; r.differs = acc.differs; r.nonfinite = acc.nonfinite;
    res[0] = r;
}

template <typename E>
__global__ void __launch_bounds__(256) cond_fill_kernel(typename E::real* __restrict__ x, int64_t n, int mode, int64_t j)
{
    typedef typename E::real R;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    R v;
    if (mode == COND_FILL_ONES) v = R(1);
    else if (mode == COND_FILL_UNIT) v = (i == j) ? R(1) : R(0);
    else {
        const R a = (R)(double)(n - 1 + i);   // below 2^24 for every n the estimator serves: exact in Float32
        v = (i & 1) ? -a : a;
    }
    x[E::PARTS * i] = v;
    if constexpr (E::PARTS == 2) x[2 * i + 1] = R(0);
}

inline size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

}  // namespace

template <typename E>
int launch_lange(Handle* h, int norm, int64_t m, int64_t n, const typename E::real* A, int64_t lda, int row_major, double* out)
{
    constexpr size_t ES = E::PARTS * sizeof(typename E::real);   // bytes of an element
    *out = 0.0;
    if (m == 0 || n == 0) return RFLU_OK;
    const int64_t len = row_major ? n : m, cnt = row_major ? m : n;
    const bool along = (norm == RFLU_NORM_ONE) != (row_major != 0);
    if (cnt > 0x7fffffffLL || len > 0x7fffffffLL) {   // the second kernel runs one thread per sum: 2^31 of them at most
        set_error("%slange: %lld x %lld has more than 2^31 - 1 rows or columns", E::WHO, (long long)m, (long long)n);
        return RFLU_ERR_ARG;
    }
    const int vec = (reinterpret_cast<uintptr_t>(A) % 16 == 0 && (lda * ES) % 16 == 0) ? 1 : 0;
    // along: cnt line sums; across: ngroups x len partial sums; then one maximum per 256 of them, then the result
    const int64_t ngroups = along ? 1 : (cnt + LN_GROUP - 1) / LN_GROUP;
    const int64_t nsums = along ? cnt : len;
    const int64_t nblocks = (nsums + LN_THREADS - 1) / LN_THREADS;
    const size_t part_bytes = up16((size_t)ngroups * (size_t)nsums * sizeof(double));
    const size_t bmax_bytes = up16((size_t)nblocks * sizeof(double));
    RFLU_TRY(ensure_buffer(&h->cond_work, &h->cond_work_bytes, part_bytes + bmax_bytes + 16));
    double* part = static_cast<double*>(h->cond_work);
    double* bmax = reinterpret_cast<double*>(static_cast<char*>(h->cond_work) + part_bytes);
    double* res = reinterpret_cast<double*>(static_cast<char*>(h->cond_work) + part_bytes + bmax_bytes);
    {
        ProfScope ps(h, RFLU_K_MISC, (double)m * (double)n, (double)m * (double)n * ES);
        if (along) {
            hipLaunchKernelGGL(lange_along_kernel<E>, dim3((unsigned)std::min<int64_t>(cnt, LN_MAX_GRID)), dim3(LN_THREADS), 0, h->stream, A, lda, len, cnt,
                               vec, part);
        } else {
            const int64_t per_block = (int64_t)LN_THREADS * (16 / ES);
            hipLaunchKernelGGL(lange_across_kernel<E>, dim3((unsigned)((len + per_block - 1) / per_block), (unsigned)std::min<int64_t>(ngroups, 65535)), dim3(LN_THREADS), 0,
                               h->stream, A, lda, len, cnt, vec, part);
        }
        hipLaunchKernelGGL(lange_max_kernel, dim3((unsigned)nblocks), dim3(LN_THREADS), 0, h->stream, part, ngroups, nsums, bmax);
        hipLaunchKernelGGL(lange_final_kernel, dim3(1), dim3(LN_THREADS), 0, h->stream, bmax, nblocks, res);
        RFLU_HIP(hipGetLastError());
    }
    RFLU_HIP(hipMemcpyAsync(out, res, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    RFLU_HIP(hipStreamSynchronize(h->stream));
    return RFLU_OK;
}

template <typename E>
int launch_lange_batched(Handle* h, int norm, int64_t batch, int64_t m, int64_t n, const typename E::real* A, int64_t lda, int64_t strideA,
                         int row_major, double* out_dev)
{
    const int64_t len = row_major ? n : m, cnt = row_major ? m : n;
    const bool along = (norm == RFLU_NORM_ONE) != (row_major != 0);
    if (std::max(m, n) <= BATCHED_MAX_DIM) {
        ProfScope ps(h, RFLU_K_MISC, (double)batch * (double)m * (double)n,
                     (double)batch * (double)m * (double)n * E::PARTS * sizeof(typename E::real));
        hipLaunchKernelGGL(lange_small_batched_kernel<E>, dim3((unsigned)batch), dim3(LN_THREADS), 0, h->stream, A, lda, strideA, (int)len,
                           (int)cnt, along ? 1 : 0, out_dev);
        RFLU_HIP(hipGetLastError());
        return RFLU_OK;
    }
    for (int64_t b = 0; b < batch; ++b) {   // the single entry's kernels, matrix by matrix: the same bits
        double v = 0.0;
        RFLU_TRY(launch_lange<E>(h, norm, m, n, A + E::PARTS * b * strideA, lda, row_major, &v));
        RFLU_HIP(hipMemcpyAsync(out_dev + b, &v, sizeof(double), hipMemcpyHostToDevice, h->stream));
        RFLU_HIP(hipStreamSynchronize(h->stream));   // `v` is pageable and reused
    }
    return RFLU_OK;
}

template <typename E>
int launch_cond_fill(Handle* h, int64_t n, typename E::real* x, int mode, int64_t j)
{
    ProfScope ps(h, RFLU_K_MISC, (double)n, (double)n * E::PARTS * sizeof(typename E::real));
    hipLaunchKernelGGL(cond_fill_kernel<E>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, x, n, mode, j);
    RFLU_HIP(hipGetLastError());
    return RFLU_OK;
}

template <typename E>
int launch_cond_stats(Handle* h, int64_t n, typename E::real* x, typename E::real* sgn, int64_t jq, int write, CondStats* out)
{
    const int64_t nchunks = (n + CS_CHUNK - 1) / CS_CHUNK;
    const size_t part_bytes = up16((size_t)nchunks * sizeof(CsPart));
    RFLU_TRY(ensure_buffer(&h->inv_part, &h->inv_part_bytes, part_bytes + 16 + sizeof(CondStats)));
    CsPart* part = static_cast<CsPart*>(h->inv_part);
    double* xj = reinterpret_cast<double*>(static_cast<char*>(h->inv_part) + part_bytes);
    CondStats* res = reinterpret_cast<CondStats*>(static_cast<char*>(h->inv_part) + part_bytes + 16);
    {
        ProfScope ps(h, RFLU_K_MISC, (double)n, 2.0 * (double)n * E::PARTS * sizeof(typename E::real));
        hipLaunchKernelGGL(cond_peek_kernel<E>, dim3(1), dim3(64), 0, h->stream, x, jq, xj);
        hipLaunchKernelGGL(cond_stats_kernel<E>, dim3((unsigned)nchunks), dim3(CS_THREADS), 0, h->stream, x, sgn, n, write, part);
        hipLaunchKernelGGL(cond_final_kernel, dim3(1), dim3(64), 0, h->stream, part, nchunks, xj, res);
        RFLU_HIP(hipGetLastError());
    }
    RFLU_HIP(hipMemcpyAsync(out, res, sizeof(CondStats), hipMemcpyDeviceToHost, h->stream));
    RFLU_HIP(hipStreamSynchronize(h->stream));
    return RFLU_OK;
}

#define RFLU_CONDEST_FOR(E)                                                                                                             \
    template int launch_lange<E>(Handle*, int, int64_t, int64_t, const E::real*, int64_t, int, double*);                                \
    template int launch_lange_batched<E>(Handle*, int, int64_t, int64_t, int64_t, const E::real*, int64_t, int64_t, int, double*);      \
    template int launch_cond_fill<E>(Handle*, int64_t, E::real*, int, int64_t);                                                         \
    template int launch_cond_stats<E>(Handle*, int64_t, E::real*, E::real*, int64_t, int, CondStats*);
RFLU_CONDEST_FOR(RealElem<double>)
RFLU_CONDEST_FOR(RealElem<float>)
RFLU_CONDEST_FOR(CplxElem<double>)
RFLU_CONDEST_FOR(CplxElem<float>)
#undef RFLU_CONDEST_FOR

}  // namespace rflu
