// batched_complex.hip -- LU and solve for a BATCH of small independent ComplexF64 / ComplexF32 matrices:
// batched.hip's two kernels with the element of complex.hip.  ComplexF32: max(m, n) <= CBATCHED_MAX_DIM_CF32 = 128 (the bytes of the
// Float64 real kernel), ComplexF64: max(m, n) <= CBATCHED_MAX_DIM_CF64 = 64 (65 x 64 x 16 B = 66.5 KB; two matrices and their passes of
// right-hand sides fit the 160 KiB of a CU).
//
// Shape of both kernels, as in batched.hip: a GROUP of 64 / 128 / 256 threads (max(m, n) <= 32 / 64 / 128) owns one matrix; a 256-thread
// workgroup holds 4 / 2 / 1 groups.  The matrix is read from HBM once into LDS, worked on there, and written once.  The matrices never
// talk to each other: no global-memory hand-off, no cooperative launch, nothing a workgroup could wait for -- one workgroup barrier per
// pivot column is all the synchronisation there is.  A group beyond the end of the batch works on zeros and stores nothing.
//
// LDS image: INTERLEAVED elements (re, im side by side, 16 / 8 bytes, moved as one double2 / float2), column-major with an ODD leading
// dimension counted in elements.  Chosen over separate re / im planes because it keeps the property the planes were offered for -- a
// column and a row are both bank-conflict free -- at half the LDS instructions: a column is contiguous; along a row consecutive lanes
// are ld * 16 bytes apart, i.e. 4 * ld dwords, and with ld odd the 16 lanes that one ds_read_b128 services together land on 16
// different groups of 4 banks (ComplexF32: ds_read_b64, 2 * ld dwords apart, 32 lanes on 32 different bank pairs).  One element is one
// LDS instruction instead of two, and the image of a caller's element is a plain copy.
//
// Factorization, per matrix the semantics of _generic_lufact! (the reference's src/lu.jl:290-338) for a complex element exactly as
// cleaf_kernel (complex.hip) states them: the pivot of column k is the row of largest modulus cmodulus(z) = hypot(re, im), strict '>'
// from 0 with the lowest current row on ties (a NaN modulus never wins, an all-zero column keeps row k); a pivot whose two parts are
// zero sets info once and the elimination carries on unscaled; otherwise inv = cdiv({1, 0}, piv) once per column, one cmul per row,
// and the rank-1 update csub(a, cmul(l, u)).  NoPivot takes row k.  The mechanics are batched.hip's:
//   * thread (r, c) of a group owns row r and every CT-th column; rows are never moved in LDS: a row carries its current POSITION
//     (interchange by renaming) and goes to that position in the one store at the end;
//   * every wave of the group finds the pivot of column k redundantly (two rows per lane, one 64-bit DPP max over the bits of the
//     modulus -- a non-negative real, so its bits order like its value; 0 for zero and NaN; the low-position tie-break only when two
//     lanes hold the same maximum), so no wave waits for another one's search;
//   * l_ik is written back one step late by the row's first thread.  One barrier per column.
// Solve: factors and 8 right-hand sides in LDS; the interchanges composed into one permutation in registers by the group's first wave
// while the factors arrive; two column-oriented substitutions with one barrier per column.  trans = 0: B <- U^-1 L^-1 P B; trans = 1
// (LAPACK 'T'): B <- P^T L^-T U^-T B; trans = 2 ('C'): B <- P^T L^-H U^-H B -- both read the same LDS image by rows, 'C' conjugates the
// element as it is read.  Diagonal: ONE reciprocal cdiv({1, 0}, d_kk) per column, formed once per matrix into LDS, then multiplies:
// a complex division per right-hand side and thread would cost more than the whole rank-1 step it feeds, and the extra rounding
// (a few eps per element) is far inside the 20 n eps backward-error bar of the tests.  A zero on the diagonal gives Inf / NaN in that
// matrix's own right-hand sides only.
// Inverse (cgetri_batched_kernel, at the end of the file): the forward solve on the columns of P * I made in LDS;
// inv(transpose(A)) and inv(A') come from the store alone.
// Geometry, the DPP maximum and the launch are shared with batched.hip: batched_kernels.hpp.
#include "complex_dev.hpp"
#include "batched_kernels.hpp"

namespace rflu {

using namespace batched;

namespace {

template <typename R> struct CVec;
template <> struct CVec<double> { typedef double2 type; };
template <> struct CVec<float> { typedef float2 type; };

// the LDS image of one matrix (or of a pass of right-hand sides): element (i, j) at s[i + j * ld], one vector load / store each
template <typename R>
struct CImage {
    typename CVec<R>::type* s;
    int ld;
    __device__ __forceinline__ Cx<R> get(int i, int j) const { const typename CVec<R>::type v = s[i + j * ld]; return Cx<R>{v.x, v.y}; }
    __device__ __forceinline__ void put(int i, int j, Cx<R> z) const { typename CVec<R>::type v; v.x = z.re; v.y = z.im; s[i + j * ld] = v; }
};

// the modulus as an integer that orders like it; 0 for zeros and NaN (neither ever beats a candidate: `absi > amax`, lu.jl:301)
__device__ __forceinline__ bu64 ckey(double v) { return (v > 0.0) ? (bu64)__double_as_longlong(v) : 0ull; }
__device__ __forceinline__ bu64 ckey(float v) { return (v > 0.0f) ? (bu64)__float_as_uint(v) : 0ull; }

// ---- the one load ----------------------------------------------------------------------------------------------------------------
// element (i, j) of the caller's matrix: G[i + j*lda] (column-major) or G[i*lda + j] (row-major), lda in complex elements; in LDS
// always (i, j) of the image.  Column-major: lanes along a column (thread grid RT x TPM/RT); row-major: lanes along a row (CT x TPM/CT).
// `valid` = false (a group beyond the end of the batch): zeros.
template <typename R>
__device__ __forceinline__ void cbload_matrix(const CImage<R>& S, const Cx<R>* G, int64_t lda, int row_major, int m, int n, const BGeo& g,
                                              int t, bool valid)
{
    const Cx<R> zero{R(0), R(0)};
    if (!row_major) {
        const int r = t & ((1 << g.rt_log) - 1), c0 = t >> g.rt_log, cs = g.tpm >> g.rt_log;
        if (r < m)
            for (int j = c0; j < n; j += cs) S.put(r, j, valid ? G[r + (int64_t)j * lda] : zero);
    } else {
        const int c = t & ((1 << g.ct_log) - 1), r0 = t >> g.ct_log, rs = g.tpm >> g.ct_log;
        if (c < n)
            for (int i = r0; i < m; i += rs) S.put(i, c, valid ? G[(int64_t)i * lda + c] : zero);
    }
}

template <typename R>
struct CFactorArgs {
    Cx<R>* A;
    int64_t* ipiv;
    int64_t* info;
    int64_t lda, strideA, stride_ipiv, batch;
    int m, n, row_major, pivot;
    BGeo g;
};

template <typename R>
__global__ void __launch_bounds__(BT) cgetrf_batched_kernel(CFactorArgs<R> a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char cbsmem[];
    const BGeo g = a.g;
    const int m = a.m, n = a.n, mn = m < n ? m : n;
    const int grp = (int)threadIdx.x >> g.tpm_log, t = (int)threadIdx.x & (g.tpm - 1), lane = t & 63;
    const int64_t b = (int64_t)blockIdx.x * (BT >> g.tpm_log) + grp;
    const bool valid = b < a.batch;
    unsigned char* base = cbsmem + (size_t)grp * g.group_bytes;
    const CImage<R> S{reinterpret_cast<typename CVec<R>::type*>(base), g.ld};
    unsigned* spiv = reinterpret_cast<unsigned*>(base + g.off_b);   // [mn] position the pivot of step k came from
    unsigned* spos = spiv + mn;                                        // [m]  final position of every row
    Cx<R>* G = a.A + (valid ? b : 0) * a.strideA;

    cbload_matrix<R>(S, G, a.lda, a.row_major, m, n, g, t, valid);

    // the row this thread updates, and the rows this lane looks at in the pivot search (every wave searches all rows)
    const int r = t & ((1 << g.rt_log) - 1), c = t >> g.rt_log, cs = g.tpm >> g.rt_log;
    bool act = r < m;
    unsigned mypos = act ? (unsigned)r : BPOS_NONE;
    unsigned pos0 = lane < m ? (unsigned)lane : BPOS_NONE, pos1 = lane + 64 < m ? (unsigned)(lane + 64) : BPOS_NONE;
    Cx<R> lprev{R(0), R(0)};
    bool updprev = false;
    int info = 0;

    for (int k = 0; k < mn; ++k) {
        __syncthreads();   // elimination k-1 is in LDS (k == 0: the matrix)
        if (updprev && c == 0) S.put(r, k - 1, lprev);   // nobody reads column k-1 any more
        int q = k;                   // row (as loaded) that becomes the pivot row
        unsigned gp = (unsigned)k;   // its current position
        if (a.pivot) {
            bu64 key = 0;
            unsigned pos = BPOS_NONE;
            int phys = 0;
            if (pos0 != BPOS_NONE) {
                key = ckey(cmodulus(S.get(lane, k)));
                pos = pos0;
                phys = lane;
            }
            if (pos1 != BPOS_NONE) {
                const bu64 k1 = ckey(cmodulus(S.get(lane + 64, k)));
                if (pos == BPOS_NONE || k1 > key || (k1 == key && pos1 < pos)) {
                    key = k1;
                    pos = pos1;
                    phys = lane + 64;
                }
            }
            const bu64 mx = bwave_max(key);
            const bool hit = pos != BPOS_NONE && key == mx;
            bu64 mask = __ballot(hit);
            if (__popcll(mask) > 1) {   // exact ties (and columns of zeros / NaN): the lowest position
                const unsigned pm = ~(unsigned)bwave_max(hit ? (bu64)(~pos) : 0ull);
                mask = __ballot(hit && pos == pm);
            }
            // position k is always among the candidates, so mask != 0
            const int wl = __builtin_amdgcn_readfirstlane(__ffsll((long long)mask) - 1) & 63;
            gp = (unsigned)__builtin_amdgcn_readlane((int)pos, wl);
            q = __builtin_amdgcn_readlane(phys, wl);
            if (pos0 != BPOS_NONE) pos0 = (lane == q) ? BPOS_NONE : (pos0 == (unsigned)k ? gp : pos0);
            if (pos1 != BPOS_NONE) pos1 = (lane + 64 == q) ? BPOS_NONE : (pos1 == (unsigned)k ? gp : pos1);
        }
        const Cx<R> piv = S.get(q, k);
        const bool zero = piv.re == R(0) && piv.im == R(0);   // iszero: both parts
        const Cx<R> inv = zero ? Cx<R>{R(1), R(0)} : cdiv(Cx<R>{R(1), R(0)}, piv);
        if (t == 0) {
            spiv[k] = gp;
            if (zero && info == 0) info = k + 1;
        }
        updprev = false;
        if (act) {
            if (r == q) {
                act = false;
                mypos = (unsigned)k;
            } else {
                if (mypos == (unsigned)k) mypos = gp;
                const Cx<R> aik = S.get(r, k);
                const Cx<R> l = zero ? aik : cmul(aik, inv);   // a zero pivot: the column stays as it is
#pragma unroll 4
                for (int j = k + 1 + c; j < n; j += cs) S.put(r, j, csub(S.get(r, j), cmul(l, S.get(q, j))));
                lprev = l;
                updprev = true;
            }
        }
    }
    __syncthreads();
    if (updprev && c == 0) S.put(r, mn - 1, lprev);
    if (c == 0 && r < m) spos[r] = mypos;
    __syncthreads();

    if (!valid) return;
    if (!a.row_major) {
        if (r < m)
            for (int j = c; j < n; j += cs) G[(int64_t)mypos + (int64_t)j * a.lda] = S.get(r, j);
    } else {
        const int cc = t & ((1 << g.ct_log) - 1), r0 = t >> g.ct_log, rs = g.tpm >> g.ct_log;
        if (cc < n)
            for (int i = r0; i < m; i += rs) G[(int64_t)spos[i] * a.lda + cc] = S.get(i, cc);
    }
    if (a.ipiv) {
        int64_t* ip = a.ipiv + b * a.stride_ipiv;
        for (int k = t; k < mn; k += g.tpm) ip[k] = (int64_t)spiv[k] + 1;
    }
    if (t == 0) a.info[b] = (int64_t)info;
}

template <typename R>
struct CSolveArgs {
    const Cx<R>* F;
    const int64_t* ipiv;
    Cx<R>* B;
    int64_t lda, strideF, stride_ipiv, ldb, strideB, batch, nrhs;
    int n, row_major, trans;
    BGeo g;
};

// F(i, k) of the triangle being solved.  MODE 0: the LDS image by columns; 1 ('T'): by rows; 2 ('C'): by rows, conjugated as it is read
template <typename R, int MODE>
__device__ __forceinline__ Cx<R> cbf(const CImage<R>& S, int i, int k)
{
    Cx<R> z = MODE ? S.get(k, i) : S.get(i, k);
    if (MODE == 2) z.im = -z.im;
    return z;
}

// x <- op(F)^-1 x on the group's pass of right-hand sides: a unit or non-unit LOWER triangle forward, then the other one backward.
// Column-oriented: after the barrier of step k every thread reads x_k (for the non-unit triangle it scales by 1 / f_kk for itself; the
// stored x_k stays unscaled until the triangle is done, so nobody reads a value that is being replaced), then takes it out of its own
// row.  D[k] = 1 / op(F)(k, k).
template <typename R, int MODE>
__device__ __forceinline__ void cbsubstitute(const CImage<R>& S, const CImage<R>& X, const CImage<R>& D, int n, int nr, int r, int c, int cs)
{
    constexpr bool UNIT_LOWER = MODE == 0;   // L (unit) forward and U backward; transposed: U^T forward and L^T (unit) backward
    for (int k = 0; k < n; ++k) {
        if (r > k && r < n) {
            const Cx<R> f = cbf<R, MODE>(S, r, k);
            const Cx<R> d = D.get(k, 0);
            for (int j = c; j < nr; j += cs) {
                const Cx<R> xk = UNIT_LOWER ? X.get(k, j) : cmul(X.get(k, j), d);
                X.put(r, j, csub(X.get(r, j), cmul(f, xk)));
            }
        }
        __syncthreads();
    }
    if (!UNIT_LOWER) {
        if (r < n) {
            const Cx<R> d = D.get(r, 0);
            for (int j = c; j < nr; j += cs) X.put(r, j, cmul(X.get(r, j), d));
        }
        __syncthreads();
    }
    for (int k = n - 1; k >= 0; --k) {
        if (r < k) {
            const Cx<R> f = cbf<R, MODE>(S, r, k);
            const Cx<R> d = D.get(k, 0);
            for (int j = c; j < nr; j += cs) {
                const Cx<R> xk = UNIT_LOWER ? cmul(X.get(k, j), d) : X.get(k, j);
                X.put(r, j, csub(X.get(r, j), cmul(f, xk)));
            }
        }
        __syncthreads();
    }
    if (UNIT_LOWER) {
        if (r < n) {
            const Cx<R> d = D.get(r, 0);
            for (int j = c; j < nr; j += cs) X.put(r, j, cmul(X.get(r, j), d));
        }
        __syncthreads();
    }
}

template <typename R>
__global__ void __launch_bounds__(BT) cgetrs_batched_kernel(CSolveArgs<R> a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char cbsmem[];
    const BGeo g = a.g;
    const int n = a.n;
    const int grp = (int)threadIdx.x >> g.tpm_log, t = (int)threadIdx.x & (g.tpm - 1), lane = t & 63;
    const int64_t b = (int64_t)blockIdx.x * (BT >> g.tpm_log) + grp;
    const bool valid = b < a.batch;
    unsigned char* base = cbsmem + (size_t)grp * g.group_bytes;
    const CImage<R> S{reinterpret_cast<typename CVec<R>::type*>(base), g.ld};
    const CImage<R> X{reinterpret_cast<typename CVec<R>::type*>(base + g.off_x), g.ld};
    const CImage<R> D{reinterpret_cast<typename CVec<R>::type*>(base + g.off_a), 0};   // [n]: reciprocal of the diagonal
    int* sperm = reinterpret_cast<int*>(base + g.off_b);   // [n]: row i of P*B is row sperm[i] of B
    const int64_t bb = valid ? b : 0;
    const Cx<R>* F = a.F + bb * a.strideF;
    Cx<R>* B = a.B + bb * a.strideB;

    cbload_matrix<R>(S, F, a.lda, a.row_major, n, n, g, t, valid);
    if (t < 64) {
        // the interchanges k <-> ipiv[k]-1, k = 0 .. n-1, composed into one permutation: two entries per lane, 2 n readlanes
        int p0 = lane, p1 = lane + 64, i0 = lane, i1 = lane + 64;
        if (a.ipiv && valid) {
            const int64_t* ip = a.ipiv + b * a.stride_ipiv;
            if (lane < n) i0 = (int)(ip[lane] - 1);
            if (lane + 64 < n) i1 = (int)(ip[lane + 64] - 1);
        }
        if (a.ipiv) {
            for (int k = 0; k < n; ++k) {
                const int ku = __builtin_amdgcn_readfirstlane(k);
                int p = ku < 64 ? __builtin_amdgcn_readlane(i0, ku) : __builtin_amdgcn_readlane(i1, ku - 64);
                if (p <= ku || p >= n) continue;   // nothing to exchange (or not an interchange getrf could have written)
                const int vk = ku < 64 ? __builtin_amdgcn_readlane(p0, ku) : __builtin_amdgcn_readlane(p1, ku - 64);
                const int vp = p < 64 ? __builtin_amdgcn_readlane(p0, p) : __builtin_amdgcn_readlane(p1, p - 64);
                if (lane == (ku & 63)) { if (ku < 64) p0 = vp; else p1 = vp; }
                if (lane == (p & 63)) { if (p < 64) p0 = vk; else p1 = vk; }
            }
        }
        if (lane < n) sperm[lane] = p0;
        if (lane + 64 < n) sperm[lane + 64] = p1;
    }
    __syncthreads();
    if (t < n) {   // one reciprocal per column for the whole solve; conj(1 / d) = 1 / conj(d) term by term in cdiv
        Cx<R> d = S.get(t, t);
        if (a.trans == 2) d.im = -d.im;
        D.put(t, 0, cdiv(Cx<R>{R(1), R(0)}, d));
    }
    __syncthreads();

    const Cx<R> zero{R(0), R(0)};
    const int r = t & ((1 << g.rt_log) - 1), c = t >> g.rt_log, cs = g.tpm >> g.rt_log;
    const int rr = t & (BNR - 1), ri0 = t >> 3, ris = g.tpm >> 3;   // row-major right-hand sides: lanes along a row of B
    for (int64_t j0 = 0; j0 < a.nrhs; j0 += BNR) {
        const int nr = (int)(a.nrhs - j0 < BNR ? a.nrhs - j0 : BNR);
        // row i of the pass: from row perm[i] of B (forward solve: P B), or row i (transposed: the interchanges come last)
        if (!a.row_major) {
            if (r < n) {
                const int src = a.trans ? r : sperm[r];
                for (int j = c; j < nr; j += cs) X.put(r, j, valid ? B[src + (j0 + j) * a.ldb] : zero);
            }
        } else if (rr < nr) {
            for (int i = ri0; i < n; i += ris) {
                const int src = a.trans ? i : sperm[i];
                X.put(i, rr, valid ? B[(int64_t)src * a.ldb + j0 + rr] : zero);
            }
        }
        __syncthreads();
        if (a.trans == 0) cbsubstitute<R, 0>(S, X, D, n, nr, r, c, cs);
        else if (a.trans == 1) cbsubstitute<R, 1>(S, X, D, n, nr, r, c, cs);
        else cbsubstitute<R, 2>(S, X, D, n, nr, r, c, cs);
        if (valid) {
            if (!a.row_major) {
                if (r < n) {
                    const int dst = a.trans ? sperm[r] : r;
                    for (int j = c; j < nr; j += cs) B[dst + (j0 + j) * a.ldb] = X.get(r, j);
                }
            } else if (rr < nr) {
                for (int i = ri0; i < n; i += ris) {
                    const int dst = a.trans ? sperm[i] : i;
                    B[(int64_t)dst * a.ldb + j0 + rr] = X.get(i, rr);
                }
            }
        }
        __syncthreads();   // the pass has left LDS before the next one arrives
    }
}

}  // namespace

template <typename R>
bool cbatched_fits(int64_t m, int64_t n)
{
    return std::max(m, n) <= (sizeof(R) == 8 ? CBATCHED_MAX_DIM_CF64 : CBATCHED_MAX_DIM_CF32);
}

template <typename R>
int launch_cgetrf_batched(Handle* h, int64_t batch, int64_t m, int64_t n, R* A, int64_t lda, int64_t strideA, int row_major,
                          int64_t* ipiv, int64_t stride_ipiv, int pivot, int64_t* info)
{
    CFactorArgs<R> a;
    a.A = reinterpret_cast<Cx<R>*>(A); a.ipiv = ipiv; a.info = info;
    a.lda = lda; a.strideA = strideA; a.stride_ipiv = stride_ipiv; a.batch = batch;
    a.m = (int)m; a.n = (int)n; a.row_major = row_major; a.pivot = pivot;
    a.g = batched_geo(m, n, sizeof(Cx<R>), false, true);
    return launch_batched(h, 0, 2 + (sizeof(R) == 4), &cgetrf_batched_kernel<R>, a, batch, RFLU_K_PANEL, 4.0 * (double)batch * (double)m * (double)n * (double)std::min(m, n),
                          2.0 * (double)batch * (double)m * (double)n * sizeof(Cx<R>));
}

template <typename R>
int launch_cgetrs_batched(Handle* h, int64_t batch, int64_t n, int64_t nrhs, const R* F, int64_t lda, int64_t strideF, int row_major,
                          const int64_t* ipiv, int64_t stride_ipiv, R* B, int64_t ldb, int64_t strideB, int trans)
{
    CSolveArgs<R> a;
    a.F = reinterpret_cast<const Cx<R>*>(F); a.ipiv = ipiv; a.B = reinterpret_cast<Cx<R>*>(B);
    a.lda = lda; a.strideF = strideF; a.stride_ipiv = stride_ipiv; a.ldb = ldb; a.strideB = strideB; a.batch = batch; a.nrhs = nrhs;
    a.n = (int)n; a.row_major = row_major; a.trans = trans;
    a.g = batched_geo(n, n, sizeof(Cx<R>), true, true);
    return launch_batched(h, 1, 2 + (sizeof(R) == 4), &cgetrs_batched_kernel<R>, a, batch, RFLU_K_TRSM, 8.0 * (double)batch * (double)n * (double)n * (double)nrhs,
                          (double)batch * ((double)n * (double)n + 2.0 * (double)n * (double)nrhs) * sizeof(Cx<R>));
}

template bool cbatched_fits<double>(int64_t, int64_t);
template bool cbatched_fits<float>(int64_t, int64_t);
template int launch_cgetrf_batched<double>(Handle*, int64_t, int64_t, int64_t, double*, int64_t, int64_t, int, int64_t*, int64_t, int, int64_t*);
template int launch_cgetrf_batched<float>(Handle*, int64_t, int64_t, int64_t, float*, int64_t, int64_t, int, int64_t*, int64_t, int, int64_t*);
template int launch_cgetrs_batched<double>(Handle*, int64_t, int64_t, int64_t, const double*, int64_t, int64_t, int, const int64_t*, int64_t,
                                           double*, int64_t, int64_t, int);
template int launch_cgetrs_batched<float>(Handle*, int64_t, int64_t, int64_t, const float*, int64_t, int64_t, int, const int64_t*, int64_t,
                                          float*, int64_t, int64_t, int);

// ---- the batched inverse.  It stands behind everything above on purpose: the two kernels above keep their
// place in the code object, and moved code alone has cost them up to 2.5 % before (profiles/batched_unified_ab.txt).
namespace {

template <typename R>
struct CInvArgs {
    const Cx<R>* F;
    const int64_t* ipiv;
    Cx<R>* Ainv;
    int64_t* info;
    int64_t lda, strideF, stride_ipiv, ldi, strideI, batch;
    int n, row_major, trans;
    BGeo g;
};

// cgetrs_batched_kernel's forward solve (cbsubstitute<R, 0>, unchanged) on the columns of P * I, which are made in LDS -- row i of a
// pass is {1, 0} in column sperm[i] -- and never read from HBM; info from the diagonal held in LDS.  Ainv holds inv(op(A)) in the
// orientation of the factors, and op costs nothing: inv(A^T) = (A^-1)^T, and a transposed column-major store has the addresses of a
// plain row-major one, so 'T' (trans = 1) takes the OTHER of the two store branches and 'C' (trans = 2) also negates the imaginary
// part as the element leaves LDS.  The lanes run along the contiguous direction of the output in all six combinations.
template <typename R>
__global__ void __launch_bounds__(BT) cgetri_batched_kernel(CInvArgs<R> a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char cbsmem[];
    const BGeo g = a.g;
    const int n = a.n;
    const int grp = (int)threadIdx.x >> g.tpm_log, t = (int)threadIdx.x & (g.tpm - 1), lane = t & 63;
    const int64_t b = (int64_t)blockIdx.x * (BT >> g.tpm_log) + grp;
    const bool valid = b < a.batch;
    unsigned char* base = cbsmem + (size_t)grp * g.group_bytes;
    const CImage<R> S{reinterpret_cast<typename CVec<R>::type*>(base), g.ld};
    const CImage<R> X{reinterpret_cast<typename CVec<R>::type*>(base + g.off_x), g.ld};
    const CImage<R> D{reinterpret_cast<typename CVec<R>::type*>(base + g.off_a), 0};   // [n]: reciprocal of the diagonal
    int* sperm = reinterpret_cast<int*>(base + g.off_b);   // [n]: row i of P*I is row sperm[i] of I
    const int64_t bb = valid ? b : 0;
    const Cx<R>* F = a.F + bb * a.strideF;
    Cx<R>* Y = a.Ainv + bb * a.strideI;

    cbload_matrix<R>(S, F, a.lda, a.row_major, n, n, g, t, valid);
    if (t < 64) {
        // the interchanges composed into one permutation, as in cgetrs_batched_kernel
        int p0 = lane, p1 = lane + 64, i0 = lane, i1 = lane + 64;
        if (a.ipiv && valid) {
            const int64_t* ip = a.ipiv + b * a.stride_ipiv;
            if (lane < n) i0 = (int)(ip[lane] - 1);
            if (lane + 64 < n) i1 = (int)(ip[lane + 64] - 1);
        }
        if (a.ipiv) {
            for (int k = 0; k < n; ++k) {
                const int ku = __builtin_amdgcn_readfirstlane(k);
                int p = ku < 64 ? __builtin_amdgcn_readlane(i0, ku) : __builtin_amdgcn_readlane(i1, ku - 64);
                if (p <= ku || p >= n) continue;
                const int vk = ku < 64 ? __builtin_amdgcn_readlane(p0, ku) : __builtin_amdgcn_readlane(p1, ku - 64);
                const int vp = p < 64 ? __builtin_amdgcn_readlane(p0, p) : __builtin_amdgcn_readlane(p1, p - 64);
                if (lane == (ku & 63)) { if (ku < 64) p0 = vp; else p1 = vp; }
                if (lane == (p & 63)) { if (p < 64) p0 = vk; else p1 = vk; }
            }
        }
        if (lane < n) sperm[lane] = p0;
        if (lane + 64 < n) sperm[lane + 64] = p1;
    }
    __syncthreads();
    if (t < 64 && valid) {   // first u_ii of this matrix with BOTH parts zero
        bool z0 = false, z1 = false;
        if (lane < n) { const Cx<R> d = S.get(lane, lane); z0 = d.re == R(0) && d.im == R(0); }
        if (lane + 64 < n) { const Cx<R> d = S.get(lane + 64, lane + 64); z1 = d.re == R(0) && d.im == R(0); }
        const bu64 m0 = __ballot(z0), m1 = __ballot(z1);
        if (lane == 0) a.info[b] = m0 ? (int64_t)__ffsll((long long)m0) : (m1 ? (int64_t)(64 + __ffsll((long long)m1)) : (int64_t)0);
    }
    if (t < n) D.put(t, 0, cdiv(Cx<R>{R(1), R(0)}, S.get(t, t)));   // one reciprocal per column for the whole inverse
    __syncthreads();

    const Cx<R> zero{R(0), R(0)}, one{R(1), R(0)};
    const int r = t & ((1 << g.rt_log) - 1), c = t >> g.rt_log, cs = g.tpm >> g.rt_log;
    const int rr = t & (BNR - 1), ri0 = t >> 3, ris = g.tpm >> 3;   // lanes along a row of the pass
    const bool by_columns = (a.row_major != 0) == (a.trans != 0);   // the store with the lanes along a column of the pass
    const bool conj = a.trans == 2;
    for (int j0 = 0; j0 < n; j0 += BNR) {
        const int nr = n - j0 < BNR ? n - j0 : BNR;
        if (r < n) {
            const int hot = sperm[r] - j0;
            for (int j = c; j < nr; j += cs) X.put(r, j, (j == hot) ? one : zero);
        }
        __syncthreads();
        cbsubstitute<R, 0>(S, X, D, n, nr, r, c, cs);
        if (valid) {
            if (by_columns) {
                if (r < n)
                    for (int j = c; j < nr; j += cs) {
                        Cx<R> z = X.get(r, j);
                        if (conj) z.im = -z.im;
                        Y[r + (int64_t)(j0 + j) * a.ldi] = z;
                    }
            } else if (rr < nr) {
                for (int i = ri0; i < n; i += ris) {
                    Cx<R> z = X.get(i, rr);
                    if (conj) z.im = -z.im;
                    Y[(int64_t)i * a.ldi + j0 + rr] = z;
                }
            }
        }
        __syncthreads();   // the pass has left LDS before the next one is made
    }
}

}  // namespace

template <typename R>
int launch_cgetri_batched(Handle* h, int64_t batch, int64_t n, const R* F, int64_t lda, int64_t strideF, int row_major, const int64_t* ipiv,
                          int64_t stride_ipiv, R* Ainv, int64_t ldi, int64_t strideI, int trans, int64_t* info)
{
    CInvArgs<R> a;
    a.F = reinterpret_cast<const Cx<R>*>(F); a.ipiv = ipiv; a.Ainv = reinterpret_cast<Cx<R>*>(Ainv); a.info = info;
    a.lda = lda; a.strideF = strideF; a.stride_ipiv = stride_ipiv; a.ldi = ldi; a.strideI = strideI; a.batch = batch;
    a.n = (int)n; a.row_major = row_major; a.trans = trans;
    a.g = batched_geo(n, n, sizeof(Cx<R>), true, true);
    return launch_batched(h, 2, 2 + (sizeof(R) == 4), &cgetri_batched_kernel<R>, a, batch, RFLU_K_TRSM, 8.0 * (double)batch * (double)n * (double)n * (double)n,
                          2.0 * (double)batch * (double)n * (double)n * sizeof(Cx<R>));
}

template int launch_cgetri_batched<double>(Handle*, int64_t, int64_t, const double*, int64_t, int64_t, int, const int64_t*, int64_t, double*,
                                           int64_t, int64_t, int, int64_t*);
template int launch_cgetri_batched<float>(Handle*, int64_t, int64_t, const float*, int64_t, int64_t, int, const int64_t*, int64_t, float*,
                                          int64_t, int64_t, int, int64_t*);

// ---- the batched condition estimate, behind everything above for the reason given at the inverse.
namespace {

template <typename R>
struct CCondArgs {
    const Cx<R>* F;
    const double* anorm;
    double* rcond;
    int64_t lda, strideF, batch;
    int n, row_major, norm;
    BGeo g;
};

struct CBStat {
    double sum, maxabs, xj;
    int argmax, nonfinite;
};

// the modulus the estimator adds: Float64 hypot, NaN when either part is one (CplxElem::abs of rflu_internal.hpp)
template <typename R>
__device__ __forceinline__ double cbabs64(Cx<R> z)
{
    const double x = (double)z.re, y = (double)z.im;
    if (x != x || y != y) return __builtin_nan("");
    return hypot(x, y);
}

// The statistics of the group's work vector X(0 .. n, 0), the same in every thread of the group: bstats of batched.hip on moduli and
// without the sign test.  Thread t < n holds x_t.  sum|x_t| is added by the tree t += t + s, s = 64 .. 1 -- the tree of
// cond_stats_kernel (condest.hip) on one chunk, whose steps s = 128 and, for n <= 64, s = 64 add +0.0 --; the first index of the
// largest modulus and the flag do not depend on an order.  sc: the group's scratch (3 doubles, 131 for n > 64).
// Barriers: two (three for n > 64), under no condition but n, which the whole workgroup shares.
template <typename R>
__device__ __forceinline__ CBStat cbstats(const CImage<R>& X, double* sc, int n, int t, int jq)
{
    const int lane = t & 63, w = t >> 6;
    int* si = reinterpret_cast<int*>(sc + 1);
    double v = 0.0, av = -1.0;
    int ai = lane, nf = 0;
    if (t < n) {
        v = cbabs64<R>(X.get(t, 0));
        av = v;
        ai = t;
        nf = !(v < __builtin_inf());
    }
    bu64 bn = __ballot(nf);
    if (n > 64) {
        if (w == 1) {
            sc[3 + lane] = v;
            sc[67 + lane] = av;
            if (lane == 0) si[1] = bn != 0;
        }
        __syncthreads();
        if (w == 0) {
            v += sc[3 + lane];
            const double a1 = sc[67 + lane];
            if (a1 > av) { av = a1; ai = 64 + lane; }
            if (si[1]) bn = 1;
        }
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        v += __shfl_down(v, s, 64);
        const double oa = __shfl_xor(av, s, 64);
        const int oi = __shfl_xor(ai, s, 64);
        if (oa > av || (oa == av && oi < ai)) { av = oa; ai = oi; }
    }
    if (w == 0 && lane == 0) {
        sc[0] = v;
        sc[2] = av;
        si[0] = ai;
        si[1] = bn != 0 ? 1 : 0;
    }
    __syncthreads();
    CBStat r;
    r.sum = sc[0];
    r.maxabs = sc[2];
    r.argmax = si[0];
    r.nonfinite = si[1];
    r.xj = cbabs64<R>(X.get(jq, 0));
    __syncthreads();   // everybody has read the scratch before its next writer comes
    return r;
}

// Higham's estimator (LAPACK zlacn2 with the integer start and closing vectors of rflu.h) on M = U^-1 L^-1, wholly inside the kernel: the
// factors go into LDS once (cbload_matrix), cbsubstitute<R, 0> on one right-hand side is M x and cbsubstitute<R, 2> is M^H x; the work
// vector (column 0), the reciprocals of the conjugated diagonal (column 1) and the scratch of cbstats (from column 2 on) live in the
// 8-column x region of the solve's geometry.  No previous-sign vector: zlacn2 has no such test.
//
// WHY NO GROUP CAN LEAVE ANOTHER ONE AT A BARRIER.  cbsubstitute's barriers are workgroup-wide, a workgroup holds 4 / 2 / 1 matrices, and
// the matrices need different numbers of estimator rounds.  So the code below has NO barrier under a condition that depends on a group's
// state: every barrier stands in straight-line code of the round, inside cbsubstitute / cbstats (whose barrier counts depend on n alone,
// and n is a kernel argument), or in loops whose trip count is n or the round counter.  The round loop is left through ONE test,
// __syncthreads_or(act), whose result is the same in every thread of the workgroup; it runs at most 5 times.  What differs between
// groups is only data: a finished group, a singular one and a group beyond the end of the batch (valid == false) run the same code with
// nr = 0 right-hand sides (cbsubstitute then touches nothing) and ignore the statistics, their estimate frozen.
template <typename R>
__global__ void __launch_bounds__(BT) cgecon_batched_kernel(CCondArgs<R> a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char cbsmem[];
    const BGeo g = a.g;
    const int n = a.n, ld = g.ld;
    const int grp = (int)threadIdx.x >> g.tpm_log, t = (int)threadIdx.x & (g.tpm - 1);
    const int64_t b = (int64_t)blockIdx.x * (BT >> g.tpm_log) + grp;
    const bool valid = b < a.batch;
    unsigned char* base = cbsmem + (size_t)grp * g.group_bytes;
    typedef typename CVec<R>::type V2;
    const CImage<R> S{reinterpret_cast<V2*>(base), ld};
    const CImage<R> X{reinterpret_cast<V2*>(base + g.off_x), ld};              // column 0: the work vector
    const CImage<R> D{reinterpret_cast<V2*>(base + g.off_a), 0};               // [n]: 1 / u_kk
    const CImage<R> DC{reinterpret_cast<V2*>(base + g.off_x) + ld, 0};         // [n]: 1 / conj(u_kk), column 1 of the x region
    double* sc = reinterpret_cast<double*>(reinterpret_cast<V2*>(base + g.off_x) + 2 * ld);   // 8-byte aligned: off_x and a V2 are
    int* si = reinterpret_cast<int*>(sc + 1);
    const Cx<R>* F = a.F + (valid ? b : 0) * a.strideF;

    cbload_matrix<R>(S, F, a.lda, a.row_major, n, n, g, t, valid);
    if (t == 0) { si[0] = 0; si[1] = 0; }
    const int r = t & ((1 << g.rt_log) - 1), c = t >> g.rt_log, cs = g.tpm >> g.rt_log;
    const bool own = c == 0 && r < n;   // this thread holds x_r (then r == t)
    __syncthreads();
    {   // a NaN in either part of any factor entry (bit 0), a u_ii with both parts zero (bit 1): plain stores of the same value
        int f = 0;
        if (r < n)
            for (int j = c; j < n; j += cs) {
                const Cx<R> v = S.get(r, j);
                if (v.re != v.re || v.im != v.im) f |= 1;
                if (j == r && v.re == R(0) && v.im == R(0)) f |= 2;
            }
        if (f & 1) si[0] = 1;
        if (f & 2) si[1] = 1;
    }
    if (t < n) {   // one reciprocal per column and operator for the whole estimate, formed as cgetrs_batched_kernel forms them
        Cx<R> d = S.get(t, t);
        D.put(t, 0, cdiv(Cx<R>{R(1), R(0)}, d));
        d.im = -d.im;
        DC.put(t, 0, cdiv(Cx<R>{R(1), R(0)}, d));
    }
    __syncthreads();
    const int scan = (si[0] ? 1 : 0) | (si[1] ? 2 : 0);
    __syncthreads();

    const bool inf_norm = a.norm == RFLU_NORM_INF;   // ||M||_inf = ||M^H||_1: M and M^H swap roles
    const Cx<R> one{R(1), R(0)}, zero{R(0), R(0)};
    bool act = valid && scan == 0, closing = false, bad = false;
    double est = 0.0;
    int j = 0;
    for (int round = 0; round < 5; ++round) {
        if (act && own) X.put(r, 0, (round == 0 || r == j) ? one : zero);
        __syncthreads();
        if (inf_norm) cbsubstitute<R, 2>(S, X, DC, n, act ? 1 : 0, r, c, cs);
        else cbsubstitute<R, 0>(S, X, D, n, act ? 1 : 0, r, c, cs);
        const CBStat s1 = cbstats<R>(X, sc, n, t, j);
        if (act) {
            if (s1.nonfinite) { bad = true; act = false; }
            else if (round == 0) {
                est = s1.sum / (double)n;
                if (n == 1) act = false;
            } else {
                const double est_old = est;
                est = s1.sum;
                if (est <= est_old) { act = false; closing = true; }
            }
        }
        if (act && own) {   // the phase vector: two Float64 quotients rounded to the element type, 1 + 0i for a zero
            const Cx<R> v = X.get(r, 0);
            const double m = cbabs64<R>(v);
            const bool z = v.re == R(0) && v.im == R(0);
            X.put(r, 0, z ? one : Cx<R>{(R)((double)v.re / m), (R)((double)v.im / m)});
        }
        __syncthreads();
        if (inf_norm) cbsubstitute<R, 0>(S, X, D, n, act ? 1 : 0, r, c, cs);
        else cbsubstitute<R, 2>(S, X, DC, n, act ? 1 : 0, r, c, cs);
        const CBStat s2 = cbstats<R>(X, sc, n, t, j);
        if (act) {
            if (s2.nonfinite) { bad = true; act = false; }
            else {
                j = s2.argmax;
                if ((round > 0 && s2.xj == s2.maxabs) || round == 4) { act = false; closing = true; }
            }
        }
        if (!__syncthreads_or(act ? 1 : 0)) break;
    }
    // the alternating vector's bound: every group runs the solve, those that do not need it with no right-hand side
    if (closing && own) {
        const R av = (R)(double)(n - 1 + r);
        X.put(r, 0, Cx<R>{(r & 1) ? -av : av, R(0)});
    }
    __syncthreads();
    if (inf_norm) cbsubstitute<R, 2>(S, X, DC, n, closing ? 1 : 0, r, c, cs);
    else cbsubstitute<R, 0>(S, X, D, n, closing ? 1 : 0, r, c, cs);
    const CBStat s3 = cbstats<R>(X, sc, n, t, 0);
    if (closing) {
        if (s3.nonfinite) bad = true;
        else {
            const double alt = 2.0 * s3.sum / (3.0 * (double)n * (double)(n - 1));
            if (alt > est) est = alt;
        }
    }
    if (valid && t == 0) {
        const double an = a.anorm[b];
        double rc;
        if (an != an || an < 0.0) rc = __builtin_nan("");
        else if (an == 0.0) rc = 0.0;
        else if (scan & 2) rc = 0.0;
        else if (scan & 1) rc = __builtin_nan("");
        else if (bad || est == 0.0) rc = 0.0;
        else rc = 1.0 / (an * est);
        a.rcond[b] = rc;
    }
}

}  // namespace

template <typename R>
int launch_cgecon_batched(Handle* h, int norm, int64_t batch, int64_t n, const R* F, int64_t lda, int64_t strideF, int row_major,
                          const double* anorm, double* rcond)
{
    CCondArgs<R> a;
    a.F = reinterpret_cast<const Cx<R>*>(F); a.anorm = anorm; a.rcond = rcond;
    a.lda = lda; a.strideF = strideF; a.batch = batch;
    a.n = (int)n; a.row_major = row_major; a.norm = norm;
    a.g = batched_geo(n, n, sizeof(Cx<R>), true, true);
    // launch_batched's bookkeeping (Handle::batched_attr_set) has no row for a fourth kernel: the same launch with a flag of its own.
    // The kernel also holds static LDS (the word behind __syncthreads_or), so asking for all 160 KiB as dynamic memory is refused: ask
    // once for what the largest launch needs, the same value from every handle.
    const int groups = BT / a.g.tpm;
    const size_t lds = (size_t)groups * a.g.group_bytes;
    const int64_t nmax = sizeof(R) == 8 ? CBATCHED_MAX_DIM_CF64 : CBATCHED_MAX_DIM_CF32;
    const BGeo gmax = batched_geo(nmax, nmax, sizeof(Cx<R>), true, true);
    const size_t lds_max = std::max(lds, (size_t)(BT / gmax.tpm) * gmax.group_bytes);
    size_t* asked = &h->cgecon_lds_asked[sizeof(R) == 4 ? 1 : 0];
    if (lds > 64 * 1024 && *asked == 0) {
        RFLU_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&cgecon_batched_kernel<R>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max));
        *asked = lds_max;
    }
    const int64_t wgs = (batch + groups - 1) / groups;
    ProfScope ps(h, RFLU_K_TRSM, 88.0 * (double)batch * (double)n * (double)n, (double)batch * (double)n * (double)n * sizeof(Cx<R>));
    hipLaunchKernelGGL(cgecon_batched_kernel<R>, dim3((unsigned)wgs), dim3(BT), lds, h->stream, a);
    RFLU_HIP(hipGetLastError());
    return RFLU_OK;
}

template int launch_cgecon_batched<double>(Handle*, int, int64_t, int64_t, const double*, int64_t, int64_t, int, const double*, double*);
template int launch_cgecon_batched<float>(Handle*, int, int64_t, int64_t, const float*, int64_t, int64_t, int, const double*, double*);

}  // namespace rflu
