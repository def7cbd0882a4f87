// inverse.hip -- what LinearAlgebra offers on the object lu! returns besides the solve: logabsdet / det and the in-place inverse
// (LAPACK getri) from the packed factors.  DESIGN.md section 4.4.
//
// logabsdet: (sum of log|u_ii|, product of sign(u_ii) times the parity of the interchanges), Float64 arithmetic for both element types.
// The diagonal is cut into chunks of LD_CHUNK = 1024 entries; a 256-thread workgroup sums a chunk (four entries per thread in index
// order, then a fixed LDS tree), the chunk sums are added in index order.  The single-matrix entry runs one workgroup per chunk and a
// second launch that walks the partial sums; the batched entry runs one workgroup per matrix that walks its chunks itself -- the same
// additions in the same order, so the two agree bit for bit, and every run repeats the last one (no floating-point read-modify-write
// on memory another workgroup touches).
//
// getri: on the transposed view V (a column-major F read row-major with ld = lda is F^T) the lower triangle with the diagonal is
// G = U^T and the strict upper triangle is H = L^T (unit); A^-T = P^T H^-1 G^-1, and A^-1 column-major IS A^-T row-major.
//   1. the diagonal is scanned for an exact zero (the reduction above): on a hit nothing is written;
//   2. G <- G^-1 in place, block columns of width GETRI_W right to left (LAPACK trtri): the 64x64 diagonal inverses come from
//      tri_inv_trans_kernel (trsv.hip) and are put in place first; a wider diagonal block is the same sweep with width 64; the panel
//      below becomes  -G22^-1 * (panel * Gjj^-1):  Q = panel * Gjj^-1 as ONE GEMM against a dense negated copy of the inverted diagonal
//      block (zeros above its diagonal, so H never reaches the GEMM), then  panel = 0 - tri(G22^-1) * Q  with rectangles that lie wholly
//      below the 64-row diagonal blocks through the GEMM and the diagonal blocks through the masked kernel below;
//   3. Z = H^-1 G^-1 in place, block rows bottom-up: H's part of the block row moves to the workspace and its place is zeroed, the rows
//      below are taken out by one GEMM (M = W, N = n), and the unit upper block on the diagonal by 64-row steps: GEMM, then the
//      pre-inverted 64x64 block times the strip, in place;
//   4. rows <- P^T (launch_perm_build + launch_laswp_rev).
// Everything is an in-order launch on the handle's stream: no kernel here waits for another workgroup, none uses a read-modify-write
// on shared memory words, so results repeat bit for bit.
// Rooflines: ld_*: n strided 4/8-byte reads (latency); blk64_kernel: 2*64*64*N flops per 64-row block against 64*N*2 elements of
// traffic -- LDS/FMA bound at ~1/8 of the vector rate, O(n^2 * 64) flops per inverse in all; tril_place / neg_tril / h_save_zero:
// element-wise, HBM bound (h_save_zero moves n^2/2 elements over the whole sweep).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "rflu_internal.hpp"

namespace rflu {

namespace {

constexpr int LD_THREADS = 256;
constexpr int LD_CHUNK = 1024;   // diagonal entries per workgroup pass: four per thread

struct LdPart {
    double sum;
    long long zero1;   // 1-based index of the first exactly-zero entry, 0 = none
    unsigned flags;    // bit 0: parity of (negative entries + interchanges), bit 1: a NaN was seen
    unsigned pad;
};

__device__ __forceinline__ long long ld_minpos(long long a, long long b)
{
    return a == 0 ? b : (b == 0 ? a : (a < b ? a : b));
}

// chunk c of the diagonal F[i * dstride], i in [c * LD_CHUNK, ...) below n: valid in thread 0
template <typename T>
__device__ __forceinline__ LdPart ld_chunk(const T* __restrict__ F, int64_t dstride, const int64_t* __restrict__ ipiv, int64_t n,
                                           int64_t c, double* sSum, long long* sZero, unsigned* sFlg)
{
    const int t = threadIdx.x;
    double sum = 0.0;
    long long zero1 = 0;
    unsigned flg = 0;
#pragma unroll
    for (int k = 0; k < LD_CHUNK / LD_THREADS; ++k) {
        const int64_t i = c * LD_CHUNK + k * LD_THREADS + t;
        if (i < n) {
            const double v = (double)F[i * dstride];
            sum += log(__builtin_fabs(v));
            if (v != v) flg |= 2u;
            if (v < 0.0) flg ^= 1u;
            if (v == 0.0 && zero1 == 0) zero1 = i + 1;
            if (ipiv && ipiv[i] != i + 1) flg ^= 1u;
        }
    }
    __syncthreads();   // the previous chunk's tree has been read
    sSum[t] = sum;
    sZero[t] = zero1;
    sFlg[t] = flg;
    __syncthreads();
    for (int s = LD_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) {
            sSum[t] += sSum[t + s];
            sZero[t] = ld_minpos(sZero[t], sZero[t + s]);
            sFlg[t] = ((sFlg[t] ^ sFlg[t + s]) & 1u) | ((sFlg[t] | sFlg[t + s]) & 2u);
        }
        __syncthreads();
    }
    LdPart p;
    p.sum = sSum[0];
    p.zero1 = sZero[0];
    p.flags = sFlg[0];
    p.pad = 0;
    return p;
}

__device__ __forceinline__ void ld_combine(LdPart& acc, const LdPart& p, bool first)
{
    if (first) { acc = p; return; }
    acc.sum += p.sum;
    acc.zero1 = ld_minpos(acc.zero1, p.zero1);
    acc.flags = ((acc.flags ^ p.flags) & 1u) | ((acc.flags | p.flags) & 2u);
}

__device__ __forceinline__ double ld_sign(const LdPart& p)
{
    if (p.flags & 2u) return __builtin_nan("");
    if (p.zero1 != 0) return 0.0;
    return (p.flags & 1u) ? -1.0 : 1.0;
}

template <typename T>
__global__ void __launch_bounds__(LD_THREADS) ld_partial_kernel(const T* __restrict__ F, int64_t dstride, const int64_t* __restrict__ ipiv,
                                                                int64_t n, LdPart* __restrict__ part)
{
    __shared__ double sSum[LD_THREADS];
    __shared__ long long sZero[LD_THREADS];
    __shared__ unsigned sFlg[LD_THREADS];
    const LdPart p = ld_chunk<T>(F, dstride, ipiv, n, (int64_t)blockIdx.x, sSum, sZero, sFlg);
    if (threadIdx.x == 0) part[blockIdx.x] = p;
}

// res[0] = logabs, res[1] = sign, res[2] = bits of the first zero's 1-based index
__global__ void __launch_bounds__(64) ld_final_kernel(const LdPart* __restrict__ part, int64_t nchunks, double* __restrict__ res)
{
    if (threadIdx.x != 0) return;
    LdPart acc = {0.0, 0, 0u, 0u};
    for (int64_t c = 0; c < nchunks; ++c) ld_combine(acc, part[c], c == 0);
    res[0] = acc.sum;
    res[1] = ld_sign(acc);
    reinterpret_cast<long long*>(res)[2] = acc.zero1;
}

template <typename T>
__global__ void __launch_bounds__(LD_THREADS) ld_batched_kernel(const T* __restrict__ F, int64_t dstride, int64_t strideF,
                                                                const int64_t* __restrict__ ipiv, int64_t stride_ipiv, int64_t n,
                                                                double* __restrict__ logabs, double* __restrict__ sign)
{
    __shared__ double sSum[LD_THREADS];
    __shared__ long long sZero[LD_THREADS];
    __shared__ unsigned sFlg[LD_THREADS];
    const int64_t b = blockIdx.x;
    const T* Fb = F + b * strideF;
    const int64_t* ip = ipiv ? ipiv + b * stride_ipiv : nullptr;
    const int64_t nchunks = (n + LD_CHUNK - 1) / LD_CHUNK;
    LdPart acc = {0.0, 0, 0u, 0u};
    for (int64_t c = 0; c < nchunks; ++c) {
        const LdPart p = ld_chunk<T>(Fb, dstride, ip, n, c, sSum, sZero, sFlg);
        ld_combine(acc, p, c == 0);
    }
    if (threadIdx.x == 0) {
        logabs[b] = acc.sum;
        sign[b] = ld_sign(acc);
    }
}

// ---- the 64-row block products of getri -------------------------------------------------------------------------------------------
// Block b (rows [64 b, 64 b + 64) below rows_total) and a tile of 32 columns per workgroup; thread (r = tid & 63, q = tid >> 6) owns
// row r, columns [8 q, 8 q + 8) of the tile.
//   MODE 0:  C_b -= tril(M_b) * B_b   M_b = M + b * mstride inside a matrix with leading dimension ldm: only entries on and below its
//                                     diagonal are loaded (what lies above belongs to the other triangle)
//   MODE 1:  C_b  = M_b * C_b         M_b dense 64x64 (ldm = 64, identity padding beyond the matrix); in place: the tile is in LDS
//                                     before the first store, and no other workgroup touches it
template <typename T, int MODE>
__global__ void __launch_bounds__(256) blk64_kernel(int rows_total, int ncols, const T* __restrict__ M, int64_t ldm, int64_t mstride,
                                                    const T* B, int64_t ldb, T* C, int64_t ldc)
{
    __shared__ T sM[64 * 65];
    __shared__ T sB[64 * 33];
    const int tid = threadIdx.x, b = blockIdx.y, c0 = blockIdx.x * 32;
    const int nb = min(64, rows_total - b * 64), nc = min(32, ncols - c0);
    const T* Mb = M + (int64_t)b * mstride;
    const T* Bb = B + (int64_t)b * 64 * ldb + c0;
    T* Cb = C + (int64_t)b * 64 * ldc + c0;
    {
        const int k = tid & 63;
        for (int i = tid >> 6; i < 64; i += 4) {
            T v = T(0);
            if (MODE == 0) {
                if (i < nb && k <= i) v = Mb[(int64_t)i * ldm + k];
            } else {
                v = Mb[i * 64 + k];
            }
            sM[i * 65 + k] = v;
        }
    }
    {
        const int c = tid & 31;
        for (int k = tid >> 5; k < 64; k += 8) sB[k * 33 + c] = (k < nb && c < nc) ? Bb[(int64_t)k * ldb + c] : T(0);
    }
    __syncthreads();
    const int r = tid & 63, q = tid >> 6;
    T acc[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[c] = T(0);
#pragma unroll 4
    for (int k = 0; k < 64; ++k) {
        const T m = sM[r * 65 + k];
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[c] += m * sB[k * 33 + q * 8 + c];
    }
    if (r < nb) {
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int col = q * 8 + c;
            if (col < nc) {
                T* p = Cb + (int64_t)r * ldc + col;
                *p = (MODE == 0) ? *p - acc[c] : acc[c];
            }
        }
    }
}

// the lower triangle (diagonal included) of every 64x64 diagonal block of V <- the block's inverse (dense 64x64 in Ginv)
template <typename T>
__global__ void __launch_bounds__(256) tril_place_kernel(int n, T* __restrict__ V, int64_t ld, const T* __restrict__ Ginv)
{
    const int b = blockIdx.x, k = threadIdx.x & 63;
    const int nb = min(64, n - b * 64);
    T* Vb = V + (int64_t)b * 64 * ld + b * 64;
    const T* src = Ginv + (size_t)b * 64 * 64;
    for (int i = threadIdx.x >> 6; i < nb; i += 4)
        if (k <= i) Vb[(int64_t)i * ld + k] = src[i * 64 + k];
}

// D (w x w, leading dimension ldd) <- -tril(Vjj), zeros above the diagonal
template <typename T>
__global__ void __launch_bounds__(256) neg_tril_kernel(int w, const T* __restrict__ Vjj, int64_t ld, T* __restrict__ D, int64_t ldd)
{
    const int k = blockIdx.x * 64 + (threadIdx.x & 63);
    const int i = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (i < w && k < w) D[(int64_t)i * ldd + k] = (k <= i) ? -Vjj[(int64_t)i * ld + k] : T(0);
}

// rows [i0, i0 + w) of V: what lies right of the diagonal (H's share of the block row) moves to Hs (row r of the block at Hs + r * ldh,
// same column index) and its place is zeroed
template <typename T>
__global__ void __launch_bounds__(256) h_save_zero_kernel(int64_t n, int64_t i0, int w, T* __restrict__ V, int64_t ld, T* __restrict__ Hs,
                                                          int64_t ldh)
{
    const int64_t c = i0 + (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int r = blockIdx.y;
    if (r < w && c < n && c > i0 + r) {
        T* p = V + (i0 + r) * ld + c;
        Hs[(int64_t)r * ldh + c] = *p;
        *p = T(0);
    }
}

template <typename T, int MODE>
int launch_blk64(Handle* h, int64_t rows_total, int64_t ncols, const T* M, int64_t ldm, int64_t mstride, const T* B, int64_t ldb, T* C,
                 int64_t ldc)
{
    if (rows_total <= 0 || ncols <= 0) return RFLU_OK;
    const int64_t nb = (rows_total + 63) / 64;
    ProfScope ps(h, RFLU_K_TRSM, 2.0 * 64.0 * (double)rows_total * (double)ncols, 3.0 * sizeof(T) * (double)rows_total * (double)ncols);
    hipLaunchKernelGGL((blk64_kernel<T, MODE>), dim3((unsigned)((ncols + 31) / 32), (unsigned)nb), dim3(256), 0, h->stream, (int)rows_total,
                       (int)ncols, M, ldm, mstride, B, ldb, C, ldc);
    RFLU_HIP(hipGetLastError());
    return RFLU_OK;
}

// C -= L21-type rectangles of tril(L) * B: every rectangle lies wholly below the 64-row diagonal blocks (those are launch_blk64's)
template <typename T>
int trmm_rect_rec(Handle* h, int64_t m, int64_t N, const T* L, int64_t ldl, const T* B, int64_t ldb, T* C, int64_t ldc)
{
    if (m <= NB) return RFLU_OK;
    const int64_t leaves = (m + NB - 1) / NB;
    const int64_t n1 = ((leaves + 1) / 2) * NB;
    RFLU_TRY(launch_gemm<T>(h, m - n1, N, n1, L + n1 * ldl, ldl, B, ldb, C + n1 * ldc, ldc));
    RFLU_TRY(trmm_rect_rec<T>(h, n1, N, L, ldl, B, ldb, C, ldc));
    return trmm_rect_rec<T>(h, m - n1, N, L + n1 * ldl + n1, ldl, B + n1 * ldb, ldb, C + n1 * ldc, ldc);
}

// G <- G^-1 for the lower triangle of the n x n block V whose 64x64 diagonal blocks already hold their inverses; block columns of width
// W, right to left.  ws: W * W elements for the negated diagonal block, then (n - W) * W for Q.
template <typename T>
int trtri_sweep(Handle* h, int64_t n, T* V, int64_t ld, int64_t W, T* ws)
{
    const int64_t nblk = (n + W - 1) / W;
    for (int64_t jb = nblk - 1; jb >= 0; --jb) {
        const int64_t j0 = jb * W, w = std::min(W, n - j0), m = n - j0 - w;
        T* Vjj = V + j0 * ld + j0;
        if (W > NB && w > NB) RFLU_TRY(trtri_sweep<T>(h, w, Vjj, ld, NB, ws));
        if (m <= 0) continue;
        T* D = ws;
        T* Q = ws + W * W;
        T* P = V + (j0 + w) * ld + j0;
        {
            ProfScope ps(h, RFLU_K_MISC, 0.0, 2.0 * sizeof(T) * (double)w * (double)w);
            hipLaunchKernelGGL(neg_tril_kernel<T>, dim3((unsigned)((w + 63) / 64), (unsigned)((w + 3) / 4)), dim3(256), 0, h->stream, (int)w,
                               Vjj, ld, D, W);
            RFLU_HIP(hipGetLastError());
        }
        RFLU_HIP(hipMemsetAsync(Q, 0, (size_t)m * (size_t)W * sizeof(T), h->stream));
        RFLU_TRY(launch_gemm<T>(h, m, w, w, P, ld, D, W, Q, W));                        // Q = panel * Gjj^-1
        RFLU_HIP(hipMemset2DAsync(P, (size_t)ld * sizeof(T), 0, (size_t)w * sizeof(T), (size_t)m, h->stream));
        const T* G22 = V + (j0 + w) * ld + (j0 + w);
        RFLU_TRY((launch_blk64<T, 0>(h, m, w, G22, ld, (int64_t)NB * ld + NB, Q, W, P, ld)));   // panel = -tri(G22^-1) * Q
        RFLU_TRY(trmm_rect_rec<T>(h, m, w, G22, ld, Q, W, P, ld));
    }
    return RFLU_OK;
}

}  // namespace

int64_t getri_width(int64_t n) { return std::min<int64_t>(GETRI_W, (n + NB - 1) / NB * NB); }

template <typename T>
int launch_logabsdet(Handle* h, int64_t n, const T* F, int64_t dstride, const int64_t* ipiv, double* logabs, double* sign, int64_t* zero1)
{
    const int64_t nchunks = (n + LD_CHUNK - 1) / LD_CHUNK;
    const size_t res_off = ((size_t)nchunks * sizeof(LdPart) + 15) & ~(size_t)15;
    RFLU_TRY(ensure_buffer(&h->inv_part, &h->inv_part_bytes, res_off + 3 * sizeof(double)));
    LdPart* part = static_cast<LdPart*>(h->inv_part);
    double* res = reinterpret_cast<double*>(static_cast<char*>(h->inv_part) + res_off);
    {
        ProfScope ps(h, RFLU_K_MISC, (double)n, (double)n * (sizeof(T) + (ipiv ? 8.0 : 0.0)));
        hipLaunchKernelGGL(ld_partial_kernel<T>, dim3((unsigned)nchunks), dim3(LD_THREADS), 0, h->stream, F, dstride, ipiv, n, part);
        hipLaunchKernelGGL(ld_final_kernel, dim3(1), dim3(64), 0, h->stream, part, nchunks, res);
        RFLU_HIP(hipGetLastError());
    }
    double host[3];
    RFLU_HIP(hipMemcpyAsync(host, res, sizeof(host), hipMemcpyDeviceToHost, h->stream));
    RFLU_HIP(hipStreamSynchronize(h->stream));
    if (logabs) *logabs = host[0];
    if (sign) *sign = host[1];
    if (zero1) {
        long long z;
        memcpy(&z, &host[2], sizeof(z));
        *zero1 = (int64_t)z;
    }
    return RFLU_OK;
}

template <typename T>
int launch_logabsdet_batched(Handle* h, int64_t batch, int64_t n, const T* F, int64_t dstride, int64_t strideF, const int64_t* ipiv,
                             int64_t stride_ipiv, double* logabs, double* sign)
{
    ProfScope ps(h, RFLU_K_MISC, (double)batch * (double)n, (double)batch * (double)n * (sizeof(T) + (ipiv ? 8.0 : 0.0)));
    hipLaunchKernelGGL(ld_batched_kernel<T>, dim3((unsigned)batch), dim3(LD_THREADS), 0, h->stream, F, dstride, strideF, ipiv, stride_ipiv, n,
                       logabs, sign);
    RFLU_HIP(hipGetLastError());
    return RFLU_OK;
}

// V (n x n, row-major, ld): the transposed view of the packed factors -> A^-T.  *info: first exactly-zero u_ii (then V is untouched).
template <typename T>
int getri_view(Handle* h, int64_t n, T* V, int64_t ld, const int64_t* ipiv, int64_t* info)
{
    *info = 0;
    if (n <= 0) return RFLU_OK;
    RFLU_TRY(launch_logabsdet<T>(h, n, V, ld + 1, nullptr, nullptr, nullptr, info));
    if (*info != 0) return RFLU_OK;
    const int64_t nb = (n + NB - 1) / NB, W = getri_width(n), ldh = (n + 15) / 16 * 16;
    const size_t inv_bytes = (size_t)nb * NB * NB * sizeof(T);
    RFLU_TRY(ensure_buffer(&h->linv_tmp, &h->linv_tmp_bytes, 2 * inv_bytes));
    h->trsv_area = nullptr;   // the cooperative solve's exchange area shares this buffer: have it wiped before its next use
    RFLU_TRY(ensure_buffer(&h->inv_work, &h->inv_work_bytes, (size_t)W * (size_t)std::max(nb * NB, ldh) * sizeof(T)));
    RFLU_TRY(ensure_bookkeeping(h, n));
    T* Ginv = static_cast<T*>(h->linv_tmp);
    T* Hinv = Ginv + (size_t)nb * NB * NB;
    T* ws = static_cast<T*>(h->inv_work);
    RFLU_TRY(launch_tri_inv_trans<T>(h, n, V, ld, Ginv, Hinv));
    {
        ProfScope ps(h, RFLU_K_MISC, 0.0, sizeof(T) * (double)n * NB);
        hipLaunchKernelGGL(tril_place_kernel<T>, dim3((unsigned)nb), dim3(256), 0, h->stream, (int)n, V, ld, Ginv);
        RFLU_HIP(hipGetLastError());
    }
    RFLU_TRY(trtri_sweep<T>(h, n, V, ld, W, ws));
    // Z = H^-1 G^-1, block rows bottom-up
    T* Hs = ws;
    for (int64_t ib = (n + W - 1) / W - 1; ib >= 0; --ib) {
        const int64_t i0 = ib * W, w = std::min(W, n - i0), below = n - i0 - w;
        {
            ProfScope ps(h, RFLU_K_MISC, 0.0, 3.0 * sizeof(T) * (double)w * (double)(n - i0));
            hipLaunchKernelGGL(h_save_zero_kernel<T>, dim3((unsigned)((n - i0 + 255) / 256), (unsigned)w), dim3(256), 0, h->stream, n, i0, (int)w,
                               V, ld, Hs, ldh);
            RFLU_HIP(hipGetLastError());
        }
        T* Zi = V + i0 * ld;
        if (below > 0) RFLU_TRY(launch_gemm<T>(h, w, n, below, Hs + i0 + w, ldh, V + (i0 + w) * ld, ld, Zi, ld));
        const int64_t subs = (w + NB - 1) / NB;
        for (int64_t sb = subs - 1; sb >= 0; --sb) {
            const int64_t s = sb * NB, rows = std::min<int64_t>(NB, w - s), ks = s + NB;
            if (ks < w) RFLU_TRY(launch_gemm<T>(h, rows, n, w - ks, Hs + s * ldh + i0 + ks, ldh, V + (i0 + ks) * ld, ld, Zi + s * ld, ld));
            RFLU_TRY((launch_blk64<T, 1>(h, rows, n, Hinv + (size_t)((i0 + s) / NB) * NB * NB, NB, 0, Zi + s * ld, ld, Zi + s * ld, ld)));
        }
    }
    if (ipiv) {
        RFLU_TRY(launch_perm_build(h, ipiv, 0, n, n));
        RFLU_TRY(launch_laswp_rev<T>(h, V, ld, n, 0, nb));
    }
    RFLU_HIP(hipStreamSynchronize(h->stream));
    return RFLU_OK;
}

template int launch_logabsdet<double>(Handle*, int64_t, const double*, int64_t, const int64_t*, double*, double*, int64_t*);
template int launch_logabsdet<float>(Handle*, int64_t, const float*, int64_t, const int64_t*, double*, double*, int64_t*);
template int launch_logabsdet_batched<double>(Handle*, int64_t, int64_t, const double*, int64_t, int64_t, const int64_t*, int64_t, double*,
                                              double*);
template int launch_logabsdet_batched<float>(Handle*, int64_t, int64_t, const float*, int64_t, int64_t, const int64_t*, int64_t, double*,
                                             double*);
template int getri_view<double>(Handle*, int64_t, double*, int64_t, const int64_t*, int64_t*);
template int getri_view<float>(Handle*, int64_t, float*, int64_t, const int64_t*, int64_t*);

}  // namespace rflu
