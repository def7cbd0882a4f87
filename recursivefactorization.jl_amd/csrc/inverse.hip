// inverse.hip -- what LinearAlgebra offers on the object lu! returns besides the solve: logabsdet / det and the in-place inverse
// (LAPACK getri) from the packed factors, for Float64, Float32, ComplexF64 and ComplexF32.  DESIGN.md sections 4.4 and 4.8.
//
// ELEMENT means what the element trait E (rflu_internal.hpp) says: for a real matrix one R (R = double / float), for a complex matrix
// one interleaved (re, im) pair of R -- the matrix crosses as R*, every ld, stride and index counts elements, and inside the stored
// element is Stored<E>::type = R or Cx<R>.  Nothing is ever conjugated: the view below is the plain transpose.  One host path and one
// set of element-wise and reduction kernels serve the four element types; FOUR points differ per element, each behind a pair of
// overloads on the stored element and nothing wider:
//   * the GEMM                          gemm_sub:       launch_gemm<R> / launch_cgemm<R>;
//   * the 64x64 diagonal inverses       tri_inv64:      tri_inv_trans_kernel (trsv.hip: substitution with divisions) / ctri_inv64_kernel
//                                                       (below: in-place trti2, one reciprocal per column);
//   * the 64-row block products         launch_blk64:   blk64_kernel / cblk64_kernel (below: the complex tile is narrower so that the
//                                                       images fit static LDS);
//   * the last step, rows <- P^T        rows_unpivot:   launch_perm_build + launch_laswp_rev / launch_claswp_rev.
//
// logabsdet: (sum of log|u_ii|, the sign / phase of the product times the parity of the interchanges), Float64 arithmetic for the four
// element types; complex |u| = hypot(re, im).  The diagonal is cut into chunks of LD_CHUNK = 1024 entries; a 256-thread workgroup
// takes a chunk (four entries per thread in index order, then a fixed LDS tree), the chunk results are combined in index order -- the
// logs by addition.  The sign of a real product is bit 0 of `flags`, into which the negative entries go with the interchanges; the
// phase of a complex product is (pre, pim), the product of u_ii / |u_ii| by complex multiplication (spelled with fma / __dmul_rn so
// that every copy of it rounds alike), with the parity and ONE renormalisation to modulus 1 last.  The single-matrix entry runs one
// workgroup per chunk and a second launch that walks the partial results; the batched entry runs one workgroup per matrix that walks
// its chunks itself -- the same operations in the same order, so the two agree bit for bit, and every run repeats the last one (no
// floating-point read-modify-write on memory another workgroup touches).  An exactly zero entry (complex: both parts zero): -Inf, sign
// 0 (0 + 0i) and its 1-based index (getri's pre-check); a NaN (complex: in either part): NaN in every output.
//
// getri: on the transposed view V (a column-major F read row-major with ld = lda is F^T) the lower triangle with the diagonal is
// G = U^T and the strict upper triangle is H = L^T (unit); A^-T = P^T H^-1 G^-1, and A^-1 column-major IS A^-T row-major.
//   1. the diagonal is scanned for an exact zero (the reduction above): on a hit nothing is written;
//   2. G <- G^-1 in place, block columns of width GETRI_W right to left (LAPACK trtri): the 64x64 diagonal inverses of both triangles
//      come from tri_inv64 and the lower ones are put in place first; a wider diagonal block is the same sweep with width 64; the panel
//      below becomes  -G22^-1 * (panel * Gjj^-1):  Q = panel * Gjj^-1 as ONE GEMM against a dense negated copy of the inverted diagonal
//      block (zeros above its diagonal, so H never reaches the GEMM), then  panel = 0 - tri(G22^-1) * Q  with rectangles that lie wholly
//      below the 64-row diagonal blocks through the GEMM and the diagonal blocks through the masked block product (MODE 0);
//   3. Z = H^-1 G^-1 in place, block rows bottom-up: H's part of the block row moves to the workspace and its place is zeroed, the rows
//      below are taken out by one GEMM (M = W, N = n), and the unit upper block on the diagonal by 64-row steps: GEMM, then the
//      pre-inverted 64x64 block times the strip, in place (MODE 1);
//   4. rows <- P^T (rows_unpivot).  Skipped for NotIPIV.
// Workspace GETRI_W x n elements and the 2 * ceil(n / 64) diagonal inverses, nothing of size n x n.
// Everything is an in-order launch on the handle's stream: no kernel here waits for another workgroup, none uses a read-modify-write
// on shared memory words, so results repeat bit for bit.
// Rooflines: ld_*: n strided element reads (latency); ctri_inv64_kernel: one wave per block, 64 dependent steps (latency, as
// tri_inv_trans_kernel); blk64_kernel / cblk64_kernel: 2 (8 complex) * 64 * 64 * N flops per 64-row block against 64 * N * 2 elements
// of traffic -- LDS/FMA bound at ~1/8 of the vector rate, O(n^2 * 64) flops per inverse in all; tril_place / neg_tril / h_save_zero:
// element-wise, HBM bound (h_save_zero moves n^2/2 elements over the whole sweep).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "complex_dev.hpp"

namespace rflu {

namespace {

template <typename E> struct Stored { typedef typename E::real type; };
template <typename R> struct Stored<CplxElem<R>> { typedef Cx<R> type; };

template <typename R>
R* flat(Cx<R>* p) { return reinterpret_cast<R*>(p); }
template <typename R>
const R* flat(const Cx<R>* p) { return reinterpret_cast<const R*>(p); }

constexpr int LD_THREADS = 256;
constexpr int LD_CHUNK = 1024;   // diagonal entries per workgroup pass: four per thread

template <int PARTS> struct LdPart;
template <> struct LdPart<1> {
    double sum;
    long long zero1;   // 1-based index of the first exactly-zero entry, 0 = none
    unsigned flags;    // bit 0: parity of (negative entries + interchanges), bit 1: a NaN was seen
    unsigned pad;
};
template <> struct LdPart<2> {
    double sum;        // sum of log|u_ii|
    double pre, pim;   // product of u_ii / |u_ii| (exact zeros left out)
    long long zero1;   // 1-based index of the first entry with both parts zero, 0 = none
    unsigned flags;    // bit 0: parity of the interchanges, bit 1: a NaN was seen
    unsigned pad;
};

__device__ __forceinline__ long long ld_minpos(long long a, long long b)
{
    return a == 0 ? b : (b == 0 ? a : (a < b ? a : b));
}

// a * b in Float64 with the roundings pinned: two products rounded on their own, two fused
__device__ __forceinline__ void ld_mul(double& are, double& aim, double bre, double bim)
{
    const double re = fma(are, bre, -__dmul_rn(aim, bim));
    const double im = fma(are, bim, __dmul_rn(aim, bre));
    are = re;
    aim = im;
}

// the LDS of a chunk's tree; the phase arrays are never touched, so never allocated, for real elements
#define RFLU_LD_SHARED(E)                                        \
    __shared__ double sSum[LD_THREADS];                          \
    __shared__ double sRe[E::PARTS == 2 ? LD_THREADS : 1];       \
    __shared__ double sIm[E::PARTS == 2 ? LD_THREADS : 1];       \
    __shared__ long long sZero[LD_THREADS];                      \
    __shared__ unsigned sFlg[LD_THREADS]

// chunk c of the diagonal F[i * dstride], i in [c * LD_CHUNK, ...) below n: valid in thread 0
template <typename E>
__device__ __forceinline__ LdPart<E::PARTS> ld_chunk(const typename Stored<E>::type* __restrict__ F, int64_t dstride,
                                                     const int64_t* __restrict__ ipiv, int64_t n, int64_t c, double* sSum, double* sRe,
                                                     double* sIm, long long* sZero, unsigned* sFlg)
{
    constexpr bool CPLX = E::PARTS == 2;
    const int t = threadIdx.x;
    double sum = 0.0, pre = 1.0, pim = 0.0;
    long long zero1 = 0;
    unsigned flg = 0;
#pragma unroll
    for (int k = 0; k < LD_CHUNK / LD_THREADS; ++k) {
        const int64_t i = c * LD_CHUNK + k * LD_THREADS + t;
        if (i < n) {
            if constexpr (CPLX) {
                const typename Stored<E>::type z = F[i * dstride];
                const double re = (double)z.re, im = (double)z.im;
                const double mod = hypot(re, im);
                sum += log(mod);
                if (re != re || im != im) flg |= 2u;
                if (re == 0.0 && im == 0.0) {
                    if (zero1 == 0) zero1 = i + 1;
                } else {
                    ld_mul(pre, pim, re / mod, im / mod);
                }
            } else {
                const double v = (double)F[i * dstride];
                sum += log(__builtin_fabs(v));
                if (v != v) flg |= 2u;
                if (v < 0.0) flg ^= 1u;
                if (v == 0.0 && zero1 == 0) zero1 = i + 1;
            }
            if (ipiv && ipiv[i] != i + 1) flg ^= 1u;
        }
    }
    __syncthreads();   // the previous chunk's tree has been read
    sSum[t] = sum;
    if constexpr (CPLX) {
        sRe[t] = pre;
        sIm[t] = pim;
    }
    sZero[t] = zero1;
    sFlg[t] = flg;
    __syncthreads();
    for (int s = LD_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) {
            sSum[t] += sSum[t + s];
            if constexpr (CPLX) {
                double a = sRe[t], b = sIm[t];
                ld_mul(a, b, sRe[t + s], sIm[t + s]);
                sRe[t] = a;
                sIm[t] = b;
            }
            sZero[t] = ld_minpos(sZero[t], sZero[t + s]);
            sFlg[t] = ((sFlg[t] ^ sFlg[t + s]) & 1u) | ((sFlg[t] | sFlg[t + s]) & 2u);
        }
        __syncthreads();
    }
    LdPart<E::PARTS> p;
    p.sum = sSum[0];
    if constexpr (CPLX) {
        p.pre = sRe[0];
        p.pim = sIm[0];
    }
    p.zero1 = sZero[0];
    p.flags = sFlg[0];
    p.pad = 0;
    return p;
}

template <int PARTS>
__device__ __forceinline__ LdPart<PARTS> ld_start()
{
    if constexpr (PARTS == 2) return {0.0, 1.0, 0.0, 0, 0u, 0u};
    else return {0.0, 0, 0u, 0u};
}

template <int PARTS>
__device__ __forceinline__ void ld_combine(LdPart<PARTS>& acc, const LdPart<PARTS>& p, bool first)
{
    if (first) { acc = p; return; }
    acc.sum += p.sum;
    if constexpr (PARTS == 2) ld_mul(acc.pre, acc.pim, p.pre, p.pim);
    acc.zero1 = ld_minpos(acc.zero1, p.zero1);
    acc.flags = ((acc.flags ^ p.flags) & 1u) | ((acc.flags | p.flags) & 2u);
}

__device__ __forceinline__ double ld_sign(const LdPart<1>& p)
{
    if (p.flags & 2u) return __builtin_nan("");
    if (p.zero1 != 0) return 0.0;
    return (p.flags & 1u) ? -1.0 : 1.0;
}

// *logabs and the sign
__device__ __forceinline__ void ld_finish(const LdPart<1>& p, double* logabs, double* sign)
{
    *logabs = p.sum;
    sign[0] = ld_sign(p);
}
// *logabs and sign[0] + i sign[1], the phase: parity applied, renormalised once
__device__ __forceinline__ void ld_finish(const LdPart<2>& p, double* logabs, double* sign)
{
    if (p.flags & 2u) {
        *logabs = sign[0] = sign[1] = __builtin_nan("");
        return;
    }
    *logabs = p.sum;
    if (p.zero1 != 0) {
        sign[0] = 0.0;
        sign[1] = 0.0;
        return;
    }
    const double sgn = (p.flags & 1u) ? -1.0 : 1.0;
    const double re = sgn * p.pre, im = sgn * p.pim, mod = hypot(re, im);
    sign[0] = re / mod;
    sign[1] = im / mod;
}

template <typename E>
__global__ void __launch_bounds__(LD_THREADS) ld_partial_kernel(const typename Stored<E>::type* __restrict__ F, int64_t dstride,
                                                                const int64_t* __restrict__ ipiv, int64_t n,
                                                                LdPart<E::PARTS>* __restrict__ part)
{
    RFLU_LD_SHARED(E);
    const LdPart<E::PARTS> p = ld_chunk<E>(F, dstride, ipiv, n, (int64_t)blockIdx.x, sSum, sRe, sIm, sZero, sFlg);
    if (threadIdx.x == 0) part[blockIdx.x] = p;
}

// res[0] = logabs, res[1 .. PARTS] = sign, res[1 + PARTS] = bits of the first zero's 1-based index
template <int PARTS>
__global__ void __launch_bounds__(64) ld_final_kernel(const LdPart<PARTS>* __restrict__ part, int64_t nchunks, double* __restrict__ res)
{
    if (threadIdx.x != 0) return;
    LdPart<PARTS> acc = ld_start<PARTS>();
    for (int64_t c = 0; c < nchunks; ++c) ld_combine(acc, part[c], c == 0);
    ld_finish(acc, &res[0], &res[1]);
    reinterpret_cast<long long*>(res)[1 + PARTS] = acc.zero1;
}

template <typename E>
__global__ void __launch_bounds__(LD_THREADS) ld_batched_kernel(const typename Stored<E>::type* __restrict__ F, int64_t dstride,
                                                                int64_t strideF, const int64_t* __restrict__ ipiv, int64_t stride_ipiv,
                                                                int64_t n, double* __restrict__ logabs, double* __restrict__ sign)
{
    RFLU_LD_SHARED(E);
    const int64_t b = blockIdx.x;
    const typename Stored<E>::type* Fb = F + b * strideF;
    const int64_t* ip = ipiv ? ipiv + b * stride_ipiv : nullptr;
    const int64_t nchunks = (n + LD_CHUNK - 1) / LD_CHUNK;
    LdPart<E::PARTS> acc = ld_start<E::PARTS>();
    for (int64_t c = 0; c < nchunks; ++c) {
        const LdPart<E::PARTS> p = ld_chunk<E>(Fb, dstride, ip, n, c, sSum, sRe, sIm, sZero, sFlg);
        ld_combine(acc, p, c == 0);
    }
    if (threadIdx.x == 0) ld_finish(acc, &logabs[b], &sign[E::PARTS * b]);
}

// ---- the complex element in LDS: one 16- / 8-byte vector, so that an element is one ds_read / ds_write -------------------------------
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

// ---- the 64x64 inverses of the diagonal blocks of a complex V --------------------------------------------------------------------
// UPPER = false: the lower triangle with its diagonal (G's block, non-unit); UPPER = true: the strict upper triangle with a unit
// diagonal (H's block; the stored diagonal belongs to G and is never read).  Output: block b -> dense row-major 64x64 at out + 4096 b,
// identity padding beyond the matrix.  One workgroup (one wave) per block; lane = row.  The block is inverted IN PLACE in one LDS image,
// column by column (LAPACK trti2): with the columns right of j done,  x_jj = 1 / a_jj  (ONE reciprocal per column, then multiplies, as
// the complex leaf scales)  and  x_ij = -(sum_{k = j+1..i} x_ik a_kj) x_jj  for i > j; the unit upper kind runs left to right with
// x_ij = -(a_ij + sum_{k = i+1..j-1} x_ik a_kj).  Every lane forms its sum from the old column before anyone overwrites it (barrier).
// One 64 x 65 image of ComplexF64 is 66560 B, above what a static __shared__ array may hold: dynamic LDS, and ComplexF64 asks for the
// opt-in once per handle (DESIGN.md section 4.8 has the LDS budget of this kernel and of cblk64_kernel).
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
            for (int k = j + 1; k <= t; ++k) acc = cfma(CLds<R>::get(S, t * CINV_LD + k), CLds<R>::get(S, k * CINV_LD + j), acc);
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
                for (int k = t + 1; k < j; ++k) acc = cfma(CLds<R>::get(S, t * CINV_LD + k), CLds<R>::get(S, k * CINV_LD + j), acc);
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
// Block b (rows [64 b, 64 b + 64) below rows_total) and a tile of columns per workgroup; thread (r = tid & 63, q = tid >> 6) owns row r
// and a quarter of the tile's columns.
//   MODE 0:  C_b -= tril(M_b) * B_b   M_b = M + b * mstride inside a matrix with leading dimension ldm: only entries on and below its
//                                     diagonal are loaded (what lies above belongs to the other triangle)
//   MODE 1:  C_b  = M_b * C_b         M_b dense 64x64 (ldm = 64, identity padding beyond the matrix); in place: the tile is wholly in
//                                     LDS before the first store, and no other workgroup touches it
// Real elements: a tile of 32 columns, K = 64 in one go.
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

// Complex elements: K runs in two halves of CB_KH = 32 and the tile has CB_TC = 16 columns, so that the images (M 64 x 33, B / C
// 64 x 17: 51200 B ComplexF64, 25600 B ComplexF32) fit static LDS.  Both images have an odd leading dimension counted in 16- / 8-byte
// elements (the rule in batched_complex.hip's header).
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
                const Cx<R> x = cfma(m, CLds<R>::get(sB, (kh * CB_KH + k) * CB_LDB + q * 4 + c), Cx<R>{accr[c], acci[c]});
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

// ---- the element-wise kernels, T the stored element ----------------------------------------------------------------------------
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

// -*p where `lower`, zero elsewhere.  The complex spelling goes part by part (cload_if) and negates the zero with the rest: the zeros
// of D meet the GEMM as factors only, where their sign does not reach a sum
template <typename R>
__device__ __forceinline__ R neg_if(bool lower, const R* p) { return lower ? -*p : R(0); }
template <typename R>
__device__ __forceinline__ Cx<R> neg_if(bool lower, const Cx<R>* p)
{
    const Cx<R> g = cload_if(lower, p);
    return Cx<R>{-g.re, -g.im};
}

// D (w x w, leading dimension ldd) <- -tril(Vjj), zeros above the diagonal
template <typename T>
__global__ void __launch_bounds__(256) neg_tril_kernel(int w, const T* __restrict__ Vjj, int64_t ld, T* __restrict__ D, int64_t ldd)
{
    const int k = blockIdx.x * 64 + (threadIdx.x & 63);
    const int i = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (i < w && k < w) D[(int64_t)i * ldd + k] = neg_if(k <= i, Vjj + (int64_t)i * ld + k);
}

// rows [i0, i0 + w) of V: what lies right of the diagonal (H's share of the block row) moves to Hs (row r of the block at Hs + r * ldh,
// same column index), as it is, and its place is zeroed
template <typename T>
__global__ void __launch_bounds__(256) h_save_zero_kernel(int64_t n, int64_t i0, int w, T* __restrict__ V, int64_t ld, T* __restrict__ Hs,
                                                          int64_t ldh)
{
    const int64_t c = i0 + (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int r = blockIdx.y;
    if (r < w && c < n && c > i0 + r) {
        T* p = V + (i0 + r) * ld + c;
        Hs[(int64_t)r * ldh + c] = *p;
        *p = T{};
    }
}

// ---- the four points that differ per element: overloads on the stored element ----------------------------------------------------------
// C <- C - A * B, row-major
template <typename R>
int gemm_sub(Handle* h, int64_t M, int64_t N, int64_t K, const R* A, int64_t lda, const R* B, int64_t ldb, R* C, int64_t ldc)
{
    return launch_gemm<R>(h, M, N, K, A, lda, B, ldb, C, ldc);
}
template <typename R>
int gemm_sub(Handle* h, int64_t M, int64_t N, int64_t K, const Cx<R>* A, int64_t lda, const Cx<R>* B, int64_t ldb, Cx<R>* C, int64_t ldc)
{
    return launch_cgemm<R>(h, M, N, K, flat(A), lda, flat(B), ldb, flat(C), ldc);
}

// the 64x64 diagonal inverses of both triangles of V: lower non-unit -> Ginv, unit upper -> Hinv
template <typename R>
int tri_inv64(Handle* h, int64_t n, const R* V, int64_t ld, R* Ginv, R* Hinv) { return launch_tri_inv_trans<R>(h, n, V, ld, Ginv, Hinv); }
template <typename R>
int tri_inv64(Handle* h, int64_t n, const Cx<R>* V, int64_t ld, Cx<R>* Ginv, Cx<R>* Hinv)
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

template <int MODE, typename R>
int launch_blk64(Handle* h, int64_t rows_total, int64_t ncols, const R* M, int64_t ldm, int64_t mstride, const R* B, int64_t ldb, R* C,
                 int64_t ldc)
{
    if (rows_total <= 0 || ncols <= 0) return RFLU_OK;
    const int64_t nb = (rows_total + 63) / 64;
    ProfScope ps(h, RFLU_K_TRSM, 2.0 * 64.0 * (double)rows_total * (double)ncols, 3.0 * sizeof(R) * (double)rows_total * (double)ncols);
    hipLaunchKernelGGL((blk64_kernel<R, MODE>), dim3((unsigned)((ncols + 31) / 32), (unsigned)nb), dim3(256), 0, h->stream, (int)rows_total,
                       (int)ncols, M, ldm, mstride, B, ldb, C, ldc);
    RFLU_HIP(hipGetLastError());
    return RFLU_OK;
}
template <int MODE, typename R>
int launch_blk64(Handle* h, int64_t rows_total, int64_t ncols, const Cx<R>* M, int64_t ldm, int64_t mstride, const Cx<R>* B, int64_t ldb,
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

// rows of V <- P^T: the interchanges undone, last first
template <typename R>
int rows_unpivot(Handle* h, int64_t n, R* V, int64_t ld, const int64_t* ipiv)
{
    RFLU_TRY(ensure_bookkeeping(h, n));
    RFLU_TRY(launch_perm_build(h, ipiv, 0, n, n));
    return launch_laswp_rev<R>(h, V, ld, n, 0, (n + NB - 1) / NB);
}
template <typename R>
int rows_unpivot(Handle* h, int64_t n, Cx<R>* V, int64_t ld, const int64_t* ipiv)
{
    return launch_claswp_rev<R>(h, flat(V), ld, 1, n, n, ipiv);
}

// ---- the two sweeps, once for every element ---------------------------------------------------------------------------------------------
// C -= L21-type rectangles of tril(L) * B: every rectangle lies wholly below the 64-row diagonal blocks (those are launch_blk64's)
template <typename E>
int trmm_rect_rec(Handle* h, int64_t m, int64_t N, const typename Stored<E>::type* L, int64_t ldl, const typename Stored<E>::type* B,
                  int64_t ldb, typename Stored<E>::type* C, int64_t ldc)
{
    if (m <= NB) return RFLU_OK;
    const int64_t leaves = (m + NB - 1) / NB;
    const int64_t n1 = ((leaves + 1) / 2) * NB;
    RFLU_TRY(gemm_sub(h, m - n1, N, n1, L + n1 * ldl, ldl, B, ldb, C + n1 * ldc, ldc));
    RFLU_TRY(trmm_rect_rec<E>(h, n1, N, L, ldl, B, ldb, C, ldc));
    return trmm_rect_rec<E>(h, m - n1, N, L + n1 * ldl + n1, ldl, B + n1 * ldb, ldb, C + n1 * ldc, ldc);
}

// G <- G^-1 for the lower triangle of the n x n block V whose 64x64 diagonal blocks already hold their inverses; block columns of width
// W, right to left.  ws: W * W elements for the negated diagonal block, then (n - W) * W for Q.
template <typename E>
int trtri_sweep(Handle* h, int64_t n, typename Stored<E>::type* V, int64_t ld, int64_t W, typename Stored<E>::type* ws)
{
    typedef typename Stored<E>::type T;
    const int64_t nblk = (n + W - 1) / W;
    for (int64_t jb = nblk - 1; jb >= 0; --jb) {
        const int64_t j0 = jb * W, w = std::min(W, n - j0), m = n - j0 - w;
        T* Vjj = V + j0 * ld + j0;
        if (W > NB && w > NB) RFLU_TRY(trtri_sweep<E>(h, w, Vjj, ld, NB, ws));
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
        RFLU_TRY(gemm_sub(h, m, w, w, P, ld, D, W, Q, W));                                  // Q = panel * Gjj^-1
        RFLU_HIP(hipMemset2DAsync(P, (size_t)ld * sizeof(T), 0, (size_t)w * sizeof(T), (size_t)m, h->stream));
        const T* G22 = V + (j0 + w) * ld + (j0 + w);
        RFLU_TRY(launch_blk64<0>(h, m, w, G22, ld, (int64_t)NB * ld + NB, Q, W, P, ld));    // panel = -tri(G22^-1) * Q
        RFLU_TRY(trmm_rect_rec<E>(h, m, w, G22, ld, Q, W, P, ld));
    }
    return RFLU_OK;
}

}  // namespace

int64_t getri_width(int64_t n) { return std::min<int64_t>(GETRI_W, (n + NB - 1) / NB * NB); }

template <typename E>
int launch_logabsdet(Handle* h, int64_t n, const typename E::real* F, int64_t dstride, const int64_t* ipiv, double* logabs,
                     double* sign_re, double* sign_im, int64_t* zero1)
{
    typedef typename Stored<E>::type T;
    typedef LdPart<E::PARTS> Part;
    constexpr int WORDS = 2 + E::PARTS;   // {logabs, sign[E::PARTS], zero1}
    const int64_t nchunks = (n + LD_CHUNK - 1) / LD_CHUNK;
    const size_t res_off = ((size_t)nchunks * sizeof(Part) + 15) & ~(size_t)15;
    RFLU_TRY(ensure_buffer(&h->inv_part, &h->inv_part_bytes, res_off + WORDS * sizeof(double)));
    Part* part = static_cast<Part*>(h->inv_part);
    double* res = reinterpret_cast<double*>(static_cast<char*>(h->inv_part) + res_off);
    {
        ProfScope ps(h, RFLU_K_MISC, (double)n, (double)n * (sizeof(T) + (ipiv ? 8.0 : 0.0)));
        hipLaunchKernelGGL(ld_partial_kernel<E>, dim3((unsigned)nchunks), dim3(LD_THREADS), 0, h->stream, reinterpret_cast<const T*>(F),
                           dstride, ipiv, n, part);
        hipLaunchKernelGGL(ld_final_kernel<E::PARTS>, dim3(1), dim3(64), 0, h->stream, part, nchunks, res);
        RFLU_HIP(hipGetLastError());
    }
    double host[WORDS];
    RFLU_HIP(hipMemcpyAsync(host, res, sizeof(host), hipMemcpyDeviceToHost, h->stream));
    RFLU_HIP(hipStreamSynchronize(h->stream));
    if (logabs) *logabs = host[0];
    if (sign_re) *sign_re = host[1];
    if (E::PARTS == 2 && sign_im) *sign_im = host[E::PARTS];
    if (zero1) {
        long long z;
        memcpy(&z, &host[1 + E::PARTS], sizeof(z));
        *zero1 = (int64_t)z;
    }
    return RFLU_OK;
}

template <typename E>
int launch_logabsdet_batched(Handle* h, int64_t batch, int64_t n, const typename E::real* F, int64_t dstride, int64_t strideF,
                             const int64_t* ipiv, int64_t stride_ipiv, double* logabs, double* sign)
{
    typedef typename Stored<E>::type T;
    ProfScope ps(h, RFLU_K_MISC, (double)batch * (double)n, (double)batch * (double)n * (sizeof(T) + (ipiv ? 8.0 : 0.0)));
    hipLaunchKernelGGL(ld_batched_kernel<E>, dim3((unsigned)batch), dim3(LD_THREADS), 0, h->stream, reinterpret_cast<const T*>(F), dstride,
                       strideF, ipiv, stride_ipiv, n, logabs, sign);
    RFLU_HIP(hipGetLastError());
    return RFLU_OK;
}

// V (n x n, row-major, ld): the transposed view of the packed factors -> A^-T.  *info: first exactly-zero u_ii (then V is untouched).
template <typename E>
int getri_view(Handle* h, int64_t n, typename E::real* Vr, int64_t ld, const int64_t* ipiv, int64_t* info)
{
    typedef typename Stored<E>::type T;
    *info = 0;
    if (n <= 0) return RFLU_OK;
    RFLU_TRY(launch_logabsdet<E>(h, n, Vr, ld + 1, nullptr, nullptr, nullptr, nullptr, info));
    if (*info != 0) return RFLU_OK;
    T* V = reinterpret_cast<T*>(Vr);
    const int64_t nb = (n + NB - 1) / NB, W = getri_width(n), ldh = (n + 15) / 16 * 16;
    const size_t inv_bytes = (size_t)nb * NB * NB * sizeof(T);
    RFLU_TRY(ensure_buffer(&h->linv_tmp, &h->linv_tmp_bytes, 2 * inv_bytes));
    h->trsv_area = nullptr;   // the cooperative solve's exchange area shares this buffer: have it wiped before its next use
    RFLU_TRY(ensure_buffer(&h->inv_work, &h->inv_work_bytes, (size_t)W * (size_t)std::max(nb * NB, ldh) * sizeof(T)));
    T* Ginv = static_cast<T*>(h->linv_tmp);
    T* Hinv = Ginv + (size_t)nb * NB * NB;
    T* ws = static_cast<T*>(h->inv_work);
    RFLU_TRY(tri_inv64(h, n, V, ld, Ginv, Hinv));
    {
        ProfScope ps(h, RFLU_K_MISC, 0.0, sizeof(T) * (double)n * NB);
        hipLaunchKernelGGL(tril_place_kernel<T>, dim3((unsigned)nb), dim3(256), 0, h->stream, (int)n, V, ld, Ginv);
        RFLU_HIP(hipGetLastError());
    }
    RFLU_TRY(trtri_sweep<E>(h, n, V, ld, W, ws));
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
        if (below > 0) RFLU_TRY(gemm_sub(h, w, n, below, Hs + i0 + w, ldh, V + (i0 + w) * ld, ld, Zi, ld));
        const int64_t subs = (w + NB - 1) / NB;
        for (int64_t sb = subs - 1; sb >= 0; --sb) {
            const int64_t s = sb * NB, rows = std::min<int64_t>(NB, w - s), ks = s + NB;
            if (ks < w) RFLU_TRY(gemm_sub(h, rows, n, w - ks, Hs + s * ldh + i0 + ks, ldh, V + (i0 + ks) * ld, ld, Zi + s * ld, ld));
            RFLU_TRY(launch_blk64<1>(h, rows, n, Hinv + (size_t)((i0 + s) / NB) * NB * NB, NB, 0, Zi + s * ld, ld, Zi + s * ld, ld));
        }
    }
    if (ipiv) RFLU_TRY(rows_unpivot(h, n, V, ld, ipiv));
    RFLU_HIP(hipStreamSynchronize(h->stream));
    return RFLU_OK;
}

#define RFLU_INVERSE_FOR(E)                                                                                                             \
    template int launch_logabsdet<E>(Handle*, int64_t, const E::real*, int64_t, const int64_t*, double*, double*, double*, int64_t*);   \
    template int launch_logabsdet_batched<E>(Handle*, int64_t, int64_t, const E::real*, int64_t, int64_t, const int64_t*, int64_t,      \
                                             double*, double*);                                                                        \
    template int getri_view<E>(Handle*, int64_t, E::real*, int64_t, const int64_t*, int64_t*);
RFLU_INVERSE_FOR(RealElem<double>)
RFLU_INVERSE_FOR(RealElem<float>)
RFLU_INVERSE_FOR(CplxElem<double>)
RFLU_INVERSE_FOR(CplxElem<float>)
#undef RFLU_INVERSE_FOR

}  // namespace rflu
