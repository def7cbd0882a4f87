// complex_inverse.hip -- inv / det / logabsdet from ComplexF64 / ComplexF32 LU factors: inverse.hip's two
// sweeps and its diagonal reduction with the element of complex.hip.  The real file is not touched and shares no kernel with this one.
//
// logabsdet: (sum of log|u_ii|, product of u_ii / |u_ii| times the parity of the interchanges), Float64 arithmetic for both element
// types; |u| = hypot(re, im).  The order is inverse.hip's: chunks of LD_CHUNK = 1024 diagonal entries, a 256-thread workgroup takes
// four entries per thread in index order and folds them with a fixed LDS tree, the chunk results are combined in index order -- the
// logs by addition, the unit phases by complex multiplication (spelled with fma / __dmul_rn so that every copy of it rounds alike).
// The parity and ONE renormalisation to modulus 1 come last.  The single-matrix entry runs one workgroup per chunk and a second launch
// that walks the partial results; the batched entry runs one workgroup per matrix that walks its chunks itself: the same operations in
// the same order, so the two agree bit for bit and every run repeats the last.  A diagonal entry with both parts zero: (-Inf, 0 + 0i)
// and its 1-based index (getri's pre-check); a NaN part: NaN in all three outputs.
//
// getri: on the transposed view V (a column-major F read row-major with ld = lda is F^T -- the plain transpose, nothing is ever
// conjugated) the lower triangle with the diagonal is G = U^T and the strict upper triangle is H = L^T (unit); A^-T = P^T H^-1 G^-1, and
// A^-1 column-major IS A^-T row-major.
//   1. the diagonal is scanned for an exact zero (the reduction above): on a hit nothing is written;
//   2. G <- G^-1 in place, block columns of width GETRI_W right to left: the 64x64 diagonal inverses of both triangles come from
//      ctri_inv64_kernel and the lower ones are put in place first; a wider diagonal block is the same sweep with width 64; the panel
//      below becomes  -G22^-1 * (panel * Gjj^-1):  Q = panel * Gjj^-1 as ONE launch_cgemm against a dense negated copy of the inverted
//      diagonal block (zeros above its diagonal, so H never reaches the GEMM), then  panel = 0 - tri(G22^-1) * Q  with the rectangles
//      below the 64-row diagonal blocks through launch_cgemm (bisection on 64-row boundaries) and the diagonal triangles through
//      cblk64_kernel<MODE 0>;
//   3. Z = H^-1 G^-1 in place, block rows bottom-up: H's share of the block row moves to the workspace and its place is zeroed, the rows
//      below are taken out by one launch_cgemm (M = W, N = n), the unit upper block on the diagonal by 64-row steps: launch_cgemm, then
//      the pre-inverted 64x64 block times the strip, in place (cblk64_kernel<MODE 1>);
//   4. rows <- P^T: launch_claswp_rev (complex_solve.hip), row stride ld, column stride 1.  Skipped for NotIPIV.
// About 4n^3/3 complex multiply-adds' worth of GEMM (n^3/3 for G^-1, n^3 for the sweep with H) against 2n^3 for a solve on an explicit
// identity; workspace GETRI_W x n elements and the 2 * ceil(n / 64) diagonal inverses, nothing of size n x n.
// Everything is an in-order launch on the handle's stream: no kernel here waits for another workgroup, none forms a value by
// read-modify-write on words another workgroup touches, so results repeat bit for bit.
//
// LDS.  One 64 x 65 image of ComplexF64 is 66560 B, above what a static __shared__ array may hold, so
//   * ctri_inv64_kernel inverts IN PLACE in one 64 x 65 image in dynamic LDS (ComplexF64 asks for the opt-in once per handle);
//   * cblk64_kernel takes K in two halves of 32 and a tile of 16 columns: M image 64 x 33, B / C image 64 x 17, 51200 B (ComplexF64) /
//     25600 B (ComplexF32) of static LDS, three workgroups per CU instead of the one that 64 x 65 + 64 x 33 (100 KB) would leave.
// Both images have an odd leading dimension counted in 16- / 8-byte elements (the rule in batched_complex.hip's header): lane r reads
// row r at a fixed column -- 33 * 16 B = 132 dwords apart, 16 lanes of one ds_read_b128 on 16 different groups of four banks -- and the
// B image is read as a broadcast; the loads into LDS run along rows.
// Rooflines: cld_*: n strided 8/16-byte reads (latency); ctri_inv64_kernel: one wave per block, 64 dependent steps (latency, as
// tri_inv_trans_kernel); cblk64_kernel: 8 * 64 * 64 * N flops per 64-row block against 64 * N * 2 elements of traffic -- LDS/FMA bound,
// O(n^2 * 64) flops per inverse in all; ctril_place / cneg_tril / ch_save_zero: element-wise, HBM bound.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "complex_dev.hpp"

namespace rflu {

namespace {

constexpr int CLD_THREADS = 256;
constexpr int CLD_CHUNK = 1024;   // diagonal entries per workgroup pass: four per thread

struct CLdPart {
    double sum;        // sum of log|u_ii|
    double pre, pim;   // product of u_ii / |u_ii| (exact zeros left out)
    long long zero1;   // 1-based index of the first entry with both parts zero, 0 = none
    unsigned flags;    // bit 0: parity of the interchanges, bit 1: a NaN was seen
    unsigned pad;
};

__device__ __forceinline__ long long cld_minpos(long long a, long long b)
{
    return a == 0 ? b : (b == 0 ? a : (a < b ? a : b));
}

// a * b in Float64 with the roundings pinned: two products rounded on their own, two fused
__device__ __forceinline__ void cld_mul(double& are, double& aim, double bre, double bim)
{
    const double re = fma(are, bre, -__dmul_rn(aim, bim));
    const double im = fma(are, bim, __dmul_rn(aim, bre));
    are = re;
    aim = im;
}

// chunk c of the diagonal F[i * dstride] (complex elements), i in [c * CLD_CHUNK, ...) below n: valid in thread 0
template <typename R>
__device__ __forceinline__ CLdPart cld_chunk(const Cx<R>* __restrict__ F, int64_t dstride, const int64_t* __restrict__ ipiv, int64_t n,
                                             int64_t c, double* sSum, double* sRe, double* sIm, long long* sZero, unsigned* sFlg)
{
    const int t = threadIdx.x;
    double sum = 0.0, pre = 1.0, pim = 0.0;
    long long zero1 = 0;
    unsigned flg = 0;
#pragma unroll
    for (int k = 0; k < CLD_CHUNK / CLD_THREADS; ++k) {
        const int64_t i = c * CLD_CHUNK + k * CLD_THREADS + t;
        if (i < n) {
            const Cx<R> z = F[i * dstride];
            const double re = (double)z.re, im = (double)z.im;
            const double mod = hypot(re, im);
            sum += log(mod);
            if (re != re || im != im) flg |= 2u;
            if (re == 0.0 && im == 0.0) {
                if (zero1 == 0) zero1 = i + 1;
            } else {
                cld_mul(pre, pim, re / mod, im / mod);
            }
            if (ipiv && ipiv[i] != i + 1) flg ^= 1u;
        }
    }
    __syncthreads();   // the previous chunk's tree has been read
    sSum[t] = sum;
    sRe[t] = pre;
    sIm[t] = pim;
    sZero[t] = zero1;
    sFlg[t] = flg;
    __syncthreads();
    for (int s = CLD_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) {
            sSum[t] += sSum[t + s];
            double a = sRe[t], b = sIm[t];
            cld_mul(a, b, sRe[t + s], sIm[t + s]);
            sRe[t] = a;
            sIm[t] = b;
            sZero[t] = cld_minpos(sZero[t], sZero[t + s]);
            sFlg[t] = ((sFlg[t] ^ sFlg[t + s]) & 1u) | ((sFlg[t] | sFlg[t + s]) & 2u);
        }
        __syncthreads();
    }
    CLdPart p;
    p.sum = sSum[0];
    p.pre = sRe[0];
    p.pim = sIm[0];
    p.zero1 = sZero[0];
    p.flags = sFlg[0];
    p.pad = 0;
    return p;
}

__device__ __forceinline__ void cld_combine(CLdPart& acc, const CLdPart& p, bool first)
{
    if (first) { acc = p; return; }
    acc.sum += p.sum;
    cld_mul(acc.pre, acc.pim, p.pre, p.pim);
    acc.zero1 = cld_minpos(acc.zero1, p.zero1);
    acc.flags = ((acc.flags ^ p.flags) & 1u) | ((acc.flags | p.flags) & 2u);
}

// out[0] = logabs, out[1] + i out[2] = the phase: parity applied, renormalised once
__device__ __forceinline__ void cld_finish(const CLdPart& p, double* logabs, double* sre, double* sim)
{
    if (p.flags & 2u) {
        *logabs = *sre = *sim = __builtin_nan("");
        return;
    }
    *logabs = p.sum;
    if (p.zero1 != 0) {
        *sre = 0.0;
        *sim = 0.0;
        return;
    }
    const double sgn = (p.flags & 1u) ? -1.0 : 1.0;
    const double re = sgn * p.pre, im = sgn * p.pim, mod = hypot(re, im);
    *sre = re / mod;
    *sim = im / mod;
}

#define RFLU_CLD_SHARED                             \
    __shared__ double sSum[CLD_THREADS];            \
    __shared__ double sRe[CLD_THREADS];             \
    __shared__ double sIm[CLD_THREADS];             \
    __shared__ long long sZero[CLD_THREADS];        \
    __shared__ unsigned sFlg[CLD_THREADS]

template <typename R>
__global__ void __launch_bounds__(CLD_THREADS) cld_partial_kernel(const Cx<R>* __restrict__ F, int64_t dstride,
                                                                  const int64_t* __restrict__ ipiv, int64_t n, CLdPart* __restrict__ part)
{
    RFLU_CLD_SHARED;
    const CLdPart p = cld_chunk<R>(F, dstride, ipiv, n, (int64_t)blockIdx.x, sSum, sRe, sIm, sZero, sFlg);
    if (threadIdx.x == 0) part[blockIdx.x] = p;
}

// res[0] = logabs, res[1] = Re sign, res[2] = Im sign, res[3] = bits of the first zero's 1-based index
__global__ void __launch_bounds__(64) cld_final_kernel(const CLdPart* __restrict__ part, int64_t nchunks, double* __restrict__ res)
{
    if (threadIdx.x != 0) return;
    CLdPart acc = {0.0, 1.0, 0.0, 0, 0u, 0u};
    for (int64_t c = 0; c < nchunks; ++c) cld_combine(acc, part[c], c == 0);
    cld_finish(acc, &res[0], &res[1], &res[2]);
    reinterpret_cast<long long*>(res)[3] = acc.zero1;
}

template <typename R>
__global__ void __launch_bounds__(CLD_THREADS) cld_batched_kernel(const Cx<R>* __restrict__ F, int64_t dstride, int64_t strideF,
                                                                  const int64_t* __restrict__ ipiv, int64_t stride_ipiv, int64_t n,
                                                                  double* __restrict__ logabs, double* __restrict__ sign)
{
    RFLU_CLD_SHARED;
    const int64_t b = blockIdx.x;
    const Cx<R>* Fb = F + b * strideF;
    const int64_t* ip = ipiv ? ipiv + b * stride_ipiv : nullptr;
    const int64_t nchunks = (n + CLD_CHUNK - 1) / CLD_CHUNK;
    CLdPart acc = {0.0, 1.0, 0.0, 0, 0u, 0u};
    for (int64_t c = 0; c < nchunks; ++c) {
        const CLdPart p = cld_chunk<R>(Fb, dstride, ip, n, c, sSum, sRe, sIm, sZero, sFlg);
        cld_combine(acc, p, c == 0);
    }
    if (threadIdx.x == 0) cld_finish(acc, &logabs[b], &sign[2 * b], &sign[2 * b + 1]);
}

// ---- the element in LDS: one 16- / 8-byte vector, so that an element is one ds_read / ds_write ---------------------------------------
template <typename R>
struct CLds {
    typedef R type __attribute__((ext_vector_type(2)));
    static __device__ __forceinline__ Cx<R> get(const type* s, int i) { const type v = s[i]; return Cx<R>{v.x, v.y}; }
    static __device__ __forceinline__ void put(type* s, int i, Cx<R> z) { type v; v.x = z.re; v.y = z.im; s[i] = v; }
};

// *p where `ok`, zero elsewhere (part by part: a choice between a global element and a private zero would go through scratch)
template <typename R>
__device__ __forceinline__ Cx<R> cload_if(bool ok, const Cx<R>* p)
{
    R re = R(0), im = R(0);
    if (ok) {
        re = p->re;
        im = p->im;
    }
    return Cx<R>{re, im};
}

// acc + a * b, four fused multiply-adds in a fixed order
template <typename R>
__device__ __forceinline__ Cx<R> cmac(Cx<R> a, Cx<R> b, Cx<R> acc)
{
    return Cx<R>{fma(-a.im, b.im, fma(a.re, b.re, acc.re)), fma(a.im, b.re, fma(a.re, b.im, acc.im))};
}

// ---- the 64x64 inverses of the diagonal blocks of V ------------------------------------------------------------------------------
// UPPER = false: the lower triangle with its diagonal (G's block, non-unit); UPPER = true: the strict upper triangle with a unit
// diagonal (H's block; the stored diagonal belongs to G and is never read).  Output: block b -> dense row-major 64x64 at out + 4096 b,
// identity padding beyond the matrix.  One workgroup (one wave) per block; lane = row.  The block is inverted IN PLACE in one LDS image,
// column by column (LAPACK trti2): with the columns right of j done,  x_jj = 1 / a_jj  (ONE reciprocal per column, then multiplies, as
// the complex leaf scales)  and  x_ij = -(sum_{k = j+1..i} x_ik a_kj) x_jj  for i > j; the unit upper kind runs left to right with
// x_ij = -(a_ij + sum_{k = i+1..j-1} x_ik a_kj).  Every lane forms its sum from the old column before anyone overwrites it (barrier).
constexpr int CINV_LD = NB + 1;

template <typename R, bool UPPER>
__global__ void __launch_bounds__(64) ctri_inv64_kernel(int n, const Cx<R>* __restrict__ V, int64_t ld, Cx<R>* __restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char cinv_lds[];
    typedef typename CLds<R>::type vec_t;
    vec_t* S = reinterpret_cast<vec_t*>(cinv_lds);
    const int t = threadIdx.x, b = blockIdx.x;
    const int nbk = min(NB, n - b * NB);
    const Cx<R>* Vb = V + (int64_t)b * NB * ld + b * NB;
    for (int i = 0; i < NB; ++i) {   // lane = column here: a row of the block is contiguous
        const bool in_tri = UPPER ? t > i : t <= i;
        Cx<R> v = cload_if(i < nbk && t < nbk && in_tri, Vb + (int64_t)i * ld + t);
        if (i == t && (UPPER || i >= nbk)) v = Cx<R>{R(1), R(0)};
        CLds<R>::put(S, i * CINV_LD + t, v);
    }
    __syncthreads();
    if (!UPPER) {
#pragma unroll 1
        for (int j = NB - 1; j >= 0; --j) {
            const Cx<R> rinv = cdiv(Cx<R>{R(1), R(0)}, CLds<R>::get(S, j * CINV_LD + j));   // (uniform over the wave)
            Cx<R> acc{R(0), R(0)};
            for (int k = j + 1; k <= t; ++k) acc = cmac(CLds<R>::get(S, t * CINV_LD + k), CLds<R>::get(S, k * CINV_LD + j), acc);
            __syncthreads();
            if (t > j) {
                const Cx<R> x = cmul(acc, rinv);
                CLds<R>::put(S, t * CINV_LD + j, Cx<R>{-x.re, -x.im});
            } else if (t == j) {
                CLds<R>::put(S, j * CINV_LD + j, rinv);
            }
            __syncthreads();
        }
    } else {
#pragma unroll 1
        for (int j = 1; j < NB; ++j) {
            Cx<R> acc{R(0), R(0)};
            if (t < j) {
                acc = CLds<R>::get(S, t * CINV_LD + j);
                for (int k = t + 1; k < j; ++k) acc = cmac(CLds<R>::get(S, t * CINV_LD + k), CLds<R>::get(S, k * CINV_LD + j), acc);
            }
            __syncthreads();
            if (t < j) CLds<R>::put(S, t * CINV_LD + j, Cx<R>{-acc.re, -acc.im});
            __syncthreads();
        }
    }
    Cx<R>* o = out + (size_t)b * NB * NB;
    for (int i = 0; i < NB; ++i) o[i * NB + t] = CLds<R>::get(S, i * CINV_LD + t);
}

// ---- the 64-row block products of getri -------------------------------------------------------------------------------------------
// Block b (rows [64 b, 64 b + 64) below rows_total) and a tile of CB_TC = 16 columns per workgroup; thread (r = tid & 63, q = tid >> 6)
// owns row r, columns [4 q, 4 q + 4) of the tile.  K runs in two halves of CB_KH = 32 so that the images fit static LDS.
//   MODE 0:  C_b -= tril(M_b) * B_b   M_b = M + b * mstride inside a matrix with leading dimension ldm: only entries on and below its
//                                     diagonal are loaded (what lies above belongs to the other triangle)
//   MODE 1:  C_b  = M_b * C_b         M_b dense 64x64 (ldm = 64, identity padding beyond the matrix); in place: the tile is wholly in
//                                     LDS before the first store, and no other workgroup touches it
constexpr int CB_TC = 16, CB_KH = 32;
constexpr int CB_LDM = CB_KH + 1, CB_LDB = CB_TC + 1;

template <typename R, int MODE>
__global__ void __launch_bounds__(256) cblk64_kernel(int rows_total, int ncols, const Cx<R>* __restrict__ M, int64_t ldm, int64_t mstride,
                                                     const Cx<R>* B, int64_t ldb, Cx<R>* C, int64_t ldc)
{
    typedef typename CLds<R>::type vec_t;
    __shared__ vec_t sM[NB * CB_LDM];
    __shared__ vec_t sB[NB * CB_LDB];
    const int tid = threadIdx.x, b = blockIdx.y, c0 = blockIdx.x * CB_TC;
    const int nb = min(NB, rows_total - b * NB), nc = min(CB_TC, ncols - c0);
    const Cx<R>* Mb = M + (int64_t)b * mstride;
    const Cx<R>* Bb = B + (int64_t)b * NB * ldb + c0;
    Cx<R>* Cb = C + (int64_t)b * NB * ldc + c0;
    {
        const int c = tid & (CB_TC - 1);
        for (int k = tid / CB_TC; k < NB; k += 256 / CB_TC)
            CLds<R>::put(sB, k * CB_LDB + c, cload_if(k < nb && c < nc, Bb + (int64_t)k * ldb + c));
    }
    const int r = tid & 63, q = tid >> 6;
    R accr[4], acci[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) accr[c] = acci[c] = R(0);
#pragma unroll 1
    for (int kh = 0; kh < NB / CB_KH; ++kh) {
        if (kh) __syncthreads();   // the previous half of M has been read
        {
            const int k = tid & (CB_KH - 1), kk = kh * CB_KH + k;
            for (int i = tid / CB_KH; i < NB; i += 256 / CB_KH) {
                const Cx<R> v = (MODE == 0) ? cload_if(i < nb && kk <= i, Mb + (int64_t)i * ldm + kk) : cload_if(true, Mb + i * NB + kk);
                CLds<R>::put(sM, i * CB_LDM + k, v);
            }
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < CB_KH; ++k) {
            const Cx<R> m = CLds<R>::get(sM, r * CB_LDM + k);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const Cx<R> x = cmac(m, CLds<R>::get(sB, (kh * CB_KH + k) * CB_LDB + q * 4 + c), Cx<R>{accr[c], acci[c]});
                accr[c] = x.re;
                acci[c] = x.im;
            }
        }
    }
    if (r < nb) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int col = q * 4 + c;
            if (col < nc) {
                Cx<R>* p = Cb + (int64_t)r * ldc + col;
                const Cx<R> a{accr[c], acci[c]};
                *p = (MODE == 0) ? csub(*p, a) : a;
            }
        }
    }
}

// the lower triangle (diagonal included) of every 64x64 diagonal block of V <- the block's inverse (dense 64x64 in Ginv)
template <typename R>
__global__ void __launch_bounds__(256) ctril_place_kernel(int n, Cx<R>* __restrict__ V, int64_t ld, const Cx<R>* __restrict__ Ginv)
{
    const int b = blockIdx.x, k = threadIdx.x & 63;
    const int nb = min(NB, n - b * NB);
    Cx<R>* Vb = V + (int64_t)b * NB * ld + b * NB;
    const Cx<R>* src = Ginv + (size_t)b * NB * NB;
    for (int i = threadIdx.x >> 6; i < nb; i += 4)
        if (k <= i) Vb[(int64_t)i * ld + k] = src[i * NB + k];
}

// D (w x w, leading dimension ldd) <- -tril(Vjj), zeros above the diagonal
template <typename R>
__global__ void __launch_bounds__(256) cneg_tril_kernel(int w, const Cx<R>* __restrict__ Vjj, int64_t ld, Cx<R>* __restrict__ D, int64_t ldd)
{
    const int k = blockIdx.x * 64 + (threadIdx.x & 63);
    const int i = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (i < w && k < w) {
        const Cx<R> g = cload_if(k <= i, Vjj + (int64_t)i * ld + k);
        D[(int64_t)i * ldd + k] = Cx<R>{-g.re, -g.im};
    }
}

// rows [i0, i0 + w) of V: what lies right of the diagonal (H's share of the block row) moves to Hs (row r of the block at Hs + r * ldh,
// same column index), as it is -- the plain transpose's L^T, no conjugation -- and its place is zeroed
template <typename R>
__global__ void __launch_bounds__(256) ch_save_zero_kernel(int64_t n, int64_t i0, int w, Cx<R>* __restrict__ V, int64_t ld,
                                                           Cx<R>* __restrict__ Hs, int64_t ldh)
{
    const int64_t c = i0 + (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int r = blockIdx.y;
    if (r < w && c < n && c > i0 + r) {
        Cx<R>* p = V + (i0 + r) * ld + c;
        Hs[(int64_t)r * ldh + c] = *p;
        *p = Cx<R>{R(0), R(0)};
    }
}

template <typename R>
R* flat(Cx<R>* p) { return reinterpret_cast<R*>(p); }
template <typename R>
const R* flat(const Cx<R>* p) { return reinterpret_cast<const R*>(p); }

template <typename R>
int launch_ctri_inv64(Handle* h, int64_t n, const Cx<R>* V, int64_t ld, Cx<R>* Ginv, Cx<R>* Hinv)
{
    const int64_t nb = (n + NB - 1) / NB;
    const size_t lds = (size_t)NB * CINV_LD * sizeof(Cx<R>);
    bool* done = &h->cinv_attr_set[sizeof(R) == 8 ? 0 : 1];
    if (lds > 64 * 1024 && !*done) {   // above the default limit a kernel has to ask once (160 KiB per CU on gfx950)
        RFLU_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(ctri_inv64_kernel<R, false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)lds));
        RFLU_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(ctri_inv64_kernel<R, true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)lds));
        *done = true;
    }
    ProfScope ps(h, RFLU_K_TRSM, 2.0 * 4.0 * (double)nb * NB * NB * NB / 3.0, 4.0 * sizeof(Cx<R>) * (double)nb * NB * NB);
    hipLaunchKernelGGL((ctri_inv64_kernel<R, false>), dim3((unsigned)nb), dim3(64), lds, h->stream, (int)n, V, ld, Ginv);
    hipLaunchKernelGGL((ctri_inv64_kernel<R, true>), dim3((unsigned)nb), dim3(64), lds, h->stream, (int)n, V, ld, Hinv);
    RFLU_HIP(hipGetLastError());
    return RFLU_OK;
}

template <typename R, int MODE>
int launch_cblk64(Handle* h, int64_t rows_total, int64_t ncols, const Cx<R>* M, int64_t ldm, int64_t mstride, const Cx<R>* B, int64_t ldb,
                  Cx<R>* C, int64_t ldc)
{
    if (rows_total <= 0 || ncols <= 0) return RFLU_OK;
    const int64_t nb = (rows_total + NB - 1) / NB;
    ProfScope ps(h, RFLU_K_TRSM, 8.0 * NB * (double)rows_total * (double)ncols, 3.0 * sizeof(Cx<R>) * (double)rows_total * (double)ncols);
    hipLaunchKernelGGL((cblk64_kernel<R, MODE>), dim3((unsigned)((ncols + CB_TC - 1) / CB_TC), (unsigned)nb), dim3(256), 0, h->stream,
                       (int)rows_total, (int)ncols, M, ldm, mstride, B, ldb, C, ldc);
    RFLU_HIP(hipGetLastError());
    return RFLU_OK;
}

// C -= L21-type rectangles of tril(L) * B: every rectangle lies wholly below the 64-row diagonal blocks (those are launch_cblk64's)
template <typename R>
int ctrmm_rect_rec(Handle* h, int64_t m, int64_t N, const Cx<R>* L, int64_t ldl, const Cx<R>* B, int64_t ldb, Cx<R>* C, int64_t ldc)
{
    if (m <= NB) return RFLU_OK;
    const int64_t leaves = (m + NB - 1) / NB;
    const int64_t n1 = ((leaves + 1) / 2) * NB;
    RFLU_TRY(launch_cgemm<R>(h, m - n1, N, n1, flat(L + n1 * ldl), ldl, flat(B), ldb, flat(C + n1 * ldc), ldc));
    RFLU_TRY(ctrmm_rect_rec<R>(h, n1, N, L, ldl, B, ldb, C, ldc));
    return ctrmm_rect_rec<R>(h, m - n1, N, L + n1 * ldl + n1, ldl, B + n1 * ldb, ldb, C + n1 * ldc, ldc);
}

// G <- G^-1 for the lower triangle of the n x n block V whose 64x64 diagonal blocks already hold their inverses; block columns of width
// W, right to left.  ws: W * W elements for the negated diagonal block, then (n - W) * W for Q.
template <typename R>
int ctrtri_sweep(Handle* h, int64_t n, Cx<R>* V, int64_t ld, int64_t W, Cx<R>* ws)
{
    const int64_t nblk = (n + W - 1) / W;
    for (int64_t jb = nblk - 1; jb >= 0; --jb) {
        const int64_t j0 = jb * W, w = std::min(W, n - j0), m = n - j0 - w;
        Cx<R>* Vjj = V + j0 * ld + j0;
        if (W > NB && w > NB) RFLU_TRY(ctrtri_sweep<R>(h, w, Vjj, ld, NB, ws));
        if (m <= 0) continue;
        Cx<R>* D = ws;
        Cx<R>* Q = ws + W * W;
        Cx<R>* P = V + (j0 + w) * ld + j0;
        {
            ProfScope ps(h, RFLU_K_MISC, 0.0, 2.0 * sizeof(Cx<R>) * (double)w * (double)w);
            hipLaunchKernelGGL(cneg_tril_kernel<R>, dim3((unsigned)((w + 63) / 64), (unsigned)((w + 3) / 4)), dim3(256), 0, h->stream, (int)w,
                               Vjj, ld, D, W);
            RFLU_HIP(hipGetLastError());
        }
        RFLU_HIP(hipMemsetAsync(Q, 0, (size_t)m * (size_t)W * sizeof(Cx<R>), h->stream));
        RFLU_TRY(launch_cgemm<R>(h, m, w, w, flat(P), ld, flat(D), W, flat(Q), W));                // Q = panel * Gjj^-1
        RFLU_HIP(hipMemset2DAsync(P, (size_t)ld * sizeof(Cx<R>), 0, (size_t)w * sizeof(Cx<R>), (size_t)m, h->stream));
        const Cx<R>* G22 = V + (j0 + w) * ld + (j0 + w);
        RFLU_TRY((launch_cblk64<R, 0>(h, m, w, G22, ld, (int64_t)NB * ld + NB, Q, W, P, ld)));     // panel = -tri(G22^-1) * Q
        RFLU_TRY(ctrmm_rect_rec<R>(h, m, w, G22, ld, Q, W, P, ld));
    }
    return RFLU_OK;
}

}  // namespace

template <typename R>
int launch_clogabsdet(Handle* h, int64_t n, const R* F, int64_t dstride, const int64_t* ipiv, double* logabs, double* sign_re,
                      double* sign_im, int64_t* zero1)
{
    const int64_t nchunks = (n + CLD_CHUNK - 1) / CLD_CHUNK;
    const size_t res_off = ((size_t)nchunks * sizeof(CLdPart) + 15) & ~(size_t)15;
    RFLU_TRY(ensure_buffer(&h->inv_part, &h->inv_part_bytes, res_off + 4 * sizeof(double)));
    CLdPart* part = static_cast<CLdPart*>(h->inv_part);
    double* res = reinterpret_cast<double*>(static_cast<char*>(h->inv_part) + res_off);
    {
        ProfScope ps(h, RFLU_K_MISC, (double)n, (double)n * (2 * sizeof(R) + (ipiv ? 8.0 : 0.0)));
        hipLaunchKernelGGL(cld_partial_kernel<R>, dim3((unsigned)nchunks), dim3(CLD_THREADS), 0, h->stream, reinterpret_cast<const Cx<R>*>(F),
                           dstride, ipiv, n, part);
        hipLaunchKernelGGL(cld_final_kernel, dim3(1), dim3(64), 0, h->stream, part, nchunks, res);
        RFLU_HIP(hipGetLastError());
    }
    double host[4];
    RFLU_HIP(hipMemcpyAsync(host, res, sizeof(host), hipMemcpyDeviceToHost, h->stream));
    RFLU_HIP(hipStreamSynchronize(h->stream));
    if (logabs) *logabs = host[0];
    if (sign_re) *sign_re = host[1];
    if (sign_im) *sign_im = host[2];
    if (zero1) {
        long long z;
        memcpy(&z, &host[3], sizeof(z));
        *zero1 = (int64_t)z;
    }
    return RFLU_OK;
}

template <typename R>
int launch_clogabsdet_batched(Handle* h, int64_t batch, int64_t n, const R* F, int64_t dstride, int64_t strideF, const int64_t* ipiv,
                              int64_t stride_ipiv, double* logabs, double* sign)
{
    ProfScope ps(h, RFLU_K_MISC, (double)batch * (double)n, (double)batch * (double)n * (2 * sizeof(R) + (ipiv ? 8.0 : 0.0)));
    hipLaunchKernelGGL(cld_batched_kernel<R>, dim3((unsigned)batch), dim3(CLD_THREADS), 0, h->stream, reinterpret_cast<const Cx<R>*>(F),
                       dstride, strideF, ipiv, stride_ipiv, n, logabs, sign);
    RFLU_HIP(hipGetLastError());
    return RFLU_OK;
}

// V (n x n complex, row-major, ld): the transposed view of the packed factors -> A^-T.  *info: first u_ii with both parts zero (then V
// is untouched).
template <typename R>
int cgetri_view(Handle* h, int64_t n, R* Vr, int64_t ld, const int64_t* ipiv, int64_t* info)
{
    *info = 0;
    if (n <= 0) return RFLU_OK;
    RFLU_TRY(launch_clogabsdet<R>(h, n, Vr, ld + 1, nullptr, nullptr, nullptr, nullptr, info));
    if (*info != 0) return RFLU_OK;
    Cx<R>* V = reinterpret_cast<Cx<R>*>(Vr);
    const int64_t nb = (n + NB - 1) / NB, W = getri_width(n), ldh = (n + 15) / 16 * 16;
    const size_t inv_bytes = (size_t)nb * NB * NB * sizeof(Cx<R>);
    RFLU_TRY(ensure_buffer(&h->linv_tmp, &h->linv_tmp_bytes, 2 * inv_bytes));
    h->trsv_area = nullptr;   // the cooperative solve's exchange area shares this buffer: have it wiped before its next use
    RFLU_TRY(ensure_buffer(&h->inv_work, &h->inv_work_bytes, (size_t)W * (size_t)std::max(nb * NB, ldh) * sizeof(Cx<R>)));
    Cx<R>* Ginv = static_cast<Cx<R>*>(h->linv_tmp);
    Cx<R>* Hinv = Ginv + (size_t)nb * NB * NB;
    Cx<R>* ws = static_cast<Cx<R>*>(h->inv_work);
    RFLU_TRY(launch_ctri_inv64<R>(h, n, V, ld, Ginv, Hinv));
    {
        ProfScope ps(h, RFLU_K_MISC, 0.0, sizeof(Cx<R>) * (double)n * NB);
        hipLaunchKernelGGL(ctril_place_kernel<R>, dim3((unsigned)nb), dim3(256), 0, h->stream, (int)n, V, ld, Ginv);
        RFLU_HIP(hipGetLastError());
    }
    RFLU_TRY(ctrtri_sweep<R>(h, n, V, ld, W, ws));
    // Z = H^-1 G^-1, block rows bottom-up
    Cx<R>* Hs = ws;
    for (int64_t ib = (n + W - 1) / W - 1; ib >= 0; --ib) {
        const int64_t i0 = ib * W, w = std::min(W, n - i0), below = n - i0 - w;
        {
            ProfScope ps(h, RFLU_K_MISC, 0.0, 3.0 * sizeof(Cx<R>) * (double)w * (double)(n - i0));
            hipLaunchKernelGGL(ch_save_zero_kernel<R>, dim3((unsigned)((n - i0 + 255) / 256), (unsigned)w), dim3(256), 0, h->stream, n, i0,
                               (int)w, V, ld, Hs, ldh);
            RFLU_HIP(hipGetLastError());
        }
        Cx<R>* Zi = V + i0 * ld;
        if (below > 0) RFLU_TRY(launch_cgemm<R>(h, w, n, below, flat(Hs + i0 + w), ldh, flat(V + (i0 + w) * ld), ld, flat(Zi), ld));
        const int64_t subs = (w + NB - 1) / NB;
        for (int64_t sb = subs - 1; sb >= 0; --sb) {
            const int64_t s = sb * NB, rows = std::min<int64_t>(NB, w - s), ks = s + NB;
            if (ks < w)
                RFLU_TRY(launch_cgemm<R>(h, rows, n, w - ks, flat(Hs + s * ldh + i0 + ks), ldh, flat(V + (i0 + ks) * ld), ld, flat(Zi + s * ld),
                                         ld));
            RFLU_TRY((launch_cblk64<R, 1>(h, rows, n, Hinv + (size_t)((i0 + s) / NB) * NB * NB, NB, 0, Zi + s * ld, ld, Zi + s * ld, ld)));
        }
    }
    if (ipiv) RFLU_TRY(launch_claswp_rev<R>(h, Vr, ld, 1, n, n, ipiv));
    RFLU_HIP(hipStreamSynchronize(h->stream));
    return RFLU_OK;
}

// ---- the device entries (column-major, as LinearAlgebra.LU holds the factors) --------------------------------------------------------
// F read as a row-major array with ld = lda IS the transposed view, and A^-1 column-major IS A^-T row-major: no layout change, whatever
// lda and the pointer's alignment (misaligned: the GEMM's element-wise loads, same arithmetic)
template <typename R>
int cgetri_cm_dev(Handle* h, int64_t n, R* F, int64_t lda, const int64_t* ipiv, int64_t* info)
{
    RFLU_TRY(cgetri_check_args(n, F, lda, info));
    *info = 0;
    if (n == 0) return RFLU_OK;
    return cgetri_view<R>(h, n, F, lda, ipiv, info);
}

template <typename R>
int clogabsdet_dev(Handle* h, int64_t n, const R* F, int64_t ld, const int64_t* ipiv, double* logabs, double* sign_re, double* sign_im)
{
    RFLU_TRY(clogabsdet_check_args(n, F, ld, logabs, sign_re, sign_im));
    *logabs = 0.0;
    *sign_re = 1.0;
    *sign_im = 0.0;
    if (n == 0) return RFLU_OK;
    return launch_clogabsdet<R>(h, n, F, ld + 1, ipiv, logabs, sign_re, sign_im, nullptr);
}

template <typename R>
int clogabsdet_batched_dev(Handle* h, int64_t batch, int64_t n, const R* F, int64_t lda, int64_t strideF, const int64_t* ipiv,
                           int64_t stride_ipiv, double* logabs_dev, double* sign_dev)
{
    if (batch < 0 || n < 0) {
        set_error("complex logabsdet_batched: negative size batch=%lld n=%lld", (long long)batch, (long long)n);
        return RFLU_ERR_ARG;
    }
    if (batch == 0) return RFLU_OK;
    if (logabs_dev == nullptr || sign_dev == nullptr || (n > 0 && F == nullptr)) {
        set_error("complex logabsdet_batched: null pointer");
        return RFLU_ERR_ARG;
    }
    if (n > 0 && (lda < n || (batch > 1 && strideF < (n - 1) * lda + n))) {
        set_error("complex logabsdet_batched: lda=%lld strideF=%lld too small for n=%lld", (long long)lda, (long long)strideF, (long long)n);
        return RFLU_ERR_ARG;
    }
    if (ipiv && batch > 1 && stride_ipiv < n) {
        set_error("complex logabsdet_batched: stride_ipiv=%lld < n", (long long)stride_ipiv);
        return RFLU_ERR_ARG;
    }
    if (n == 0) {   // the empty product: (0, 1 + 0i) for every matrix
        std::vector<double> z((size_t)batch, 0.0), o(2 * (size_t)batch, 0.0);
        for (int64_t b = 0; b < batch; ++b) o[2 * (size_t)b] = 1.0;
        RFLU_HIP(hipMemcpyAsync(logabs_dev, z.data(), z.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
        RFLU_HIP(hipMemcpyAsync(sign_dev, o.data(), o.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
        RFLU_HIP(hipStreamSynchronize(h->stream));
        return RFLU_OK;
    }
    RFLU_TRY(launch_clogabsdet_batched<R>(h, batch, n, F, lda + 1, strideF, ipiv, stride_ipiv, logabs_dev, sign_dev));
    RFLU_HIP(hipStreamSynchronize(h->stream));
    return RFLU_OK;
}

#define RFLU_INSTANTIATE_CINV(R)                                                                                                     \
    template int launch_clogabsdet<R>(Handle*, int64_t, const R*, int64_t, const int64_t*, double*, double*, double*, int64_t*);      \
    template int cgetri_cm_dev<R>(Handle*, int64_t, R*, int64_t, const int64_t*, int64_t*);                                           \
    template int clogabsdet_dev<R>(Handle*, int64_t, const R*, int64_t, const int64_t*, double*, double*, double*);                   \
    template int clogabsdet_batched_dev<R>(Handle*, int64_t, int64_t, const R*, int64_t, int64_t, const int64_t*, int64_t, double*,   \
                                           double*);
RFLU_INSTANTIATE_CINV(double)
RFLU_INSTANTIATE_CINV(float)

}  // namespace rflu
