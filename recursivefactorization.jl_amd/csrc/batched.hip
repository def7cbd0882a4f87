// batched.hip -- LU and solve for a BATCH of small independent matrices (max(m, n) <= BATCHED_MAX_DIM = 128): the sizes the reference
// was written for (threshold 40, the reference's src/lu.jl:90; tests up to 300 columns), where one matrix cannot fill a GPU.
//
// Shape of both kernels: a GROUP of 64 / 128 / 256 threads (max(m, n) <= 32 / 64 / 128) owns one matrix; a 256-thread workgroup holds
// 4 / 2 / 1 groups.  The matrix is read from HBM once into LDS (column-major, odd leading dimension: a column AND a row are
// bank-conflict free), worked on there, and written once.  The matrices never talk to each other: no global-memory hand-off, no
// cooperative launch, nothing a workgroup could wait for -- one workgroup barrier per pivot column is all the synchronisation there is.
//
// Factorization, per matrix the semantics of _generic_lufact! (the reference's src/lu.jl:290-338), as panel_single.hip states them:
// argmax |a_ik| with strict '>' from 0 and the lowest row on ties (:298-305; a NaN never wins), reciprocal-multiply scaling (:317-320),
// a zero pivot sets info once and the elimination carries on unscaled (:321-334), NoPivot takes row k.
//   * thread (r, c) of a group owns row r and every CT-th column; rows are never moved in LDS: a row carries its current POSITION
//     (interchange by renaming, as in the leaf kernels) and goes to that position in the one store at the end;
//   * every wave of the group finds the pivot of column k redundantly (two rows per lane, one 64-bit DPP max; the low-position
//     tie-break only when two lanes hold the same maximum), so no wave waits for another one's search;
//   * l_ik is written back one step late by the row's first thread: nobody reads column k-1 any more then, and the other threads of
//     the row still read a_ik while step k runs.  One barrier per column.
// Solve: factors and 8 right-hand sides in LDS; interchanges as one gather through the composed permutation (built in registers by
// the group's first wave while the factors arrive), then two column-oriented substitutions with one barrier per column; the
// transposed solve reads the same LDS image by rows (U^T forward, L^T backward) and scatters through the permutation.
// Roofline: n dependent steps of {barrier, pivot search, LDS rank-1 update}; only for n <= 16 the one load and one store matter.
// Geometry, the DPP maximum and the launch are shared with batched_complex.hip: batched_kernels.hpp.
#include "batched_kernels.hpp"

namespace rflu {

using namespace batched;

namespace {

// |v| as an integer that orders like the magnitude; 0 for zeros and NaN (neither ever beats a candidate: `absi > amax`, lu.jl:301)
__device__ __forceinline__ bu64 bkey(double v)
{
    return (__builtin_fabs(v) > 0.0) ? ((bu64)__double_as_longlong(v) & 0x7fffffffffffffffull) : 0ull;
}
__device__ __forceinline__ bu64 bkey(float v)
{
    return (__builtin_fabsf(v) > 0.0f) ? (bu64)(__float_as_uint(v) & 0x7fffffffu) : 0ull;
}

// ---- the one load and the one store ---------------------------------------------------------------------------------------------
// element (i, j) of the caller's matrix: G[i + j*lda] (column-major) or G[i*lda + j] (row-major); in LDS always s[i + j*ld].
// Column-major: lanes along a column (thread grid RT x TPM/RT); row-major: lanes along a row (CT x TPM/CT).  A power-of-two grid:
// no integer division.  `valid` = false (a group beyond the end of the batch): zeros.
template <typename T>
__device__ __forceinline__ void bload_matrix(T* s, int ld, const T* G, int64_t lda, int row_major, int m, int n, const BGeo& g,
                                             int t, bool valid)
{
    if (!row_major) {
        const int r = t & ((1 << g.rt_log) - 1), c0 = t >> g.rt_log, cs = g.tpm >> g.rt_log;
        if (r < m)
            for (int j = c0; j < n; j += cs) s[r + j * ld] = valid ? G[r + (int64_t)j * lda] : T(0);
    } else {
        const int c = t & ((1 << g.ct_log) - 1), r0 = t >> g.ct_log, rs = g.tpm >> g.ct_log;
        if (c < n)
            for (int i = r0; i < m; i += rs) s[i + c * ld] = valid ? G[(int64_t)i * lda + c] : T(0);
    }
}

template <typename T>
struct BFactorArgs {
    T* A;
    int64_t* ipiv;
    int64_t* info;
    int64_t lda, strideA, stride_ipiv, batch;
    int m, n, row_major, pivot;
    BGeo g;
};

template <typename T>
__global__ void __launch_bounds__(BT) getrf_batched_kernel(BFactorArgs<T> a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char bsmem[];
    const BGeo g = a.g;
    const int m = a.m, n = a.n, mn = m < n ? m : n, ld = g.ld;
    const int grp = (int)threadIdx.x >> g.tpm_log, t = (int)threadIdx.x & (g.tpm - 1), lane = t & 63;
    const int64_t b = (int64_t)blockIdx.x * (BT >> g.tpm_log) + grp;
    const bool valid = b < a.batch;
    unsigned char* base = bsmem + (size_t)grp * g.group_bytes;
    T* s = reinterpret_cast<T*>(base);
    unsigned* spiv = reinterpret_cast<unsigned*>(base + g.off_a);   // [mn] position the pivot of step k came from
    unsigned* spos = spiv + mn;                                        // [m]  final position of every row
    T* G = a.A + (valid ? b : 0) * a.strideA;

    bload_matrix<T>(s, ld, G, a.lda, a.row_major, m, n, g, t, valid);

    // the row this thread updates, and the rows this lane looks at in the pivot search (every wave searches all rows)
    const int r = t & ((1 << g.rt_log) - 1), c = t >> g.rt_log, cs = g.tpm >> g.rt_log;
    bool act = r < m;
    unsigned mypos = act ? (unsigned)r : BPOS_NONE;
    unsigned pos0 = lane < m ? (unsigned)lane : BPOS_NONE, pos1 = lane + 64 < m ? (unsigned)(lane + 64) : BPOS_NONE;
    T lprev = T(0);
    bool updprev = false;
    int info = 0;

    for (int k = 0; k < mn; ++k) {
        __syncthreads();   // elimination k-1 is in LDS (k == 0: the matrix)
        if (updprev && c == 0) s[r + (k - 1) * ld] = lprev;   // nobody reads column k-1 any more
        int q = k;             // row (as loaded) that becomes the pivot row
        unsigned gp = (unsigned)k;   // its current position
        if (a.pivot) {
            bu64 key = 0;
            unsigned pos = BPOS_NONE;
            int phys = 0;
            if (pos0 != BPOS_NONE) {
                key = bkey(s[lane + k * ld]);
                pos = pos0;
                phys = lane;
            }
            if (pos1 != BPOS_NONE) {
                const bu64 k1 = bkey(s[lane + 64 + k * ld]);
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
        const T piv = s[q + k * ld];
        const T sc = (piv != T(0)) ? T(1) / piv : T(1);
        if (t == 0) {
            spiv[k] = gp;
            if (piv == T(0) && info == 0) info = k + 1;
        }
        updprev = false;
        if (act) {
            if (r == q) {
                act = false;
                mypos = (unsigned)k;
            } else {
                if (mypos == (unsigned)k) mypos = gp;
                const T l = s[r + k * ld] * sc;
#pragma unroll 4
                for (int j = k + 1 + c; j < n; j += cs) s[r + j * ld] -= l * s[q + j * ld];
                lprev = l;
                updprev = true;
            }
        }
    }
    __syncthreads();
    if (updprev && c == 0) s[r + (mn - 1) * ld] = lprev;
    if (c == 0 && r < m) spos[r] = mypos;
    __syncthreads();

    if (!valid) return;
    if (!a.row_major) {
        if (r < m)
            for (int j = c; j < n; j += cs) G[(int64_t)mypos + (int64_t)j * a.lda] = s[r + j * ld];
    } else {
        const int cc = t & ((1 << g.ct_log) - 1), r0 = t >> g.ct_log, rs = g.tpm >> g.ct_log;
        if (cc < n)
            for (int i = r0; i < m; i += rs) G[(int64_t)spos[i] * a.lda + cc] = s[i + cc * ld];
    }
    if (a.ipiv) {
        int64_t* ip = a.ipiv + b * a.stride_ipiv;
        for (int k = t; k < mn; k += g.tpm) ip[k] = (int64_t)spiv[k] + 1;
    }
    if (t == 0) a.info[b] = (int64_t)info;
}

template <typename T>
struct BSolveArgs {
    const T* F;
    const int64_t* ipiv;
    T* B;
    int64_t lda, strideF, stride_ipiv, ldb, strideB, batch, nrhs;
    int n, row_major, trans;
    BGeo g;
};

// F(i, k) of the triangle being solved: the LDS image by columns, or by rows for the transposed solve
template <typename T, bool TRANS>
__device__ __forceinline__ T bf(const T* s, int ld, int i, int k)
{
    return TRANS ? s[k + i * ld] : s[i + k * ld];
}

// x <- op(F)^-1 x on the group's pass of right-hand sides: a unit or non-unit LOWER triangle forward, then the other one backward.
// Column-oriented: after the barrier of step k every thread reads x_k (for the non-unit triangle it divides for itself; the stored
// x_k stays undivided until the triangle is done, so nobody reads a value that is being replaced), then takes it out of its own row.
template <typename T, bool TRANS>
__device__ __forceinline__ void bsubstitute(const T* s, T* x, int ld, int n, int nr, int r, int c, int cs)
{
    constexpr bool UNIT_LOWER = !TRANS;   // L (unit) forward and U backward; transposed: U^T forward and L^T (unit) backward
    for (int k = 0; k < n; ++k) {
        if (r > k && r < n) {
            const T f = bf<T, TRANS>(s, ld, r, k);
            const T d = UNIT_LOWER ? T(1) : bf<T, TRANS>(s, ld, k, k);
            for (int j = c; j < nr; j += cs) {
                const T xk = UNIT_LOWER ? x[k + j * ld] : x[k + j * ld] / d;
                x[r + j * ld] -= f * xk;
            }
        }
        __syncthreads();
    }
    if (!UNIT_LOWER) {
        if (r < n) {
            const T d = bf<T, TRANS>(s, ld, r, r);
            for (int j = c; j < nr; j += cs) x[r + j * ld] /= d;
        }
        __syncthreads();
    }
    for (int k = n - 1; k >= 0; --k) {
        if (r < k) {
            const T f = bf<T, TRANS>(s, ld, r, k);
            const T d = UNIT_LOWER ? bf<T, TRANS>(s, ld, k, k) : T(1);
            for (int j = c; j < nr; j += cs) {
                const T xk = UNIT_LOWER ? x[k + j * ld] / d : x[k + j * ld];
                x[r + j * ld] -= f * xk;
            }
        }
        __syncthreads();
    }
    if (UNIT_LOWER) {
        if (r < n) {
            const T d = bf<T, TRANS>(s, ld, r, r);
            for (int j = c; j < nr; j += cs) x[r + j * ld] /= d;
        }
        __syncthreads();
    }
}

template <typename T>
__global__ void __launch_bounds__(BT) getrs_batched_kernel(BSolveArgs<T> a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char bsmem[];
    const BGeo g = a.g;
    const int n = a.n, ld = g.ld;
    const int grp = (int)threadIdx.x >> g.tpm_log, t = (int)threadIdx.x & (g.tpm - 1), lane = t & 63;
    const int64_t b = (int64_t)blockIdx.x * (BT >> g.tpm_log) + grp;
    const bool valid = b < a.batch;
    unsigned char* base = bsmem + (size_t)grp * g.group_bytes;
    T* s = reinterpret_cast<T*>(base);
    T* x = reinterpret_cast<T*>(base + g.off_x);
    int* sperm = reinterpret_cast<int*>(base + g.off_a);   // [n]: row i of P*B is row sperm[i] of B
    const int64_t bb = valid ? b : 0;
    const T* F = a.F + bb * a.strideF;
    T* B = a.B + bb * a.strideB;

    bload_matrix<T>(s, ld, F, a.lda, a.row_major, n, n, g, t, valid);
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

    const int r = t & ((1 << g.rt_log) - 1), c = t >> g.rt_log, cs = g.tpm >> g.rt_log;
    const int rr = t & (BNR - 1), ri0 = t >> 3, ris = g.tpm >> 3;   // row-major right-hand sides: lanes along a row of B
    for (int64_t j0 = 0; j0 < a.nrhs; j0 += BNR) {
        const int nr = (int)(a.nrhs - j0 < BNR ? a.nrhs - j0 : BNR);
        // row i of the pass: from row perm[i] of B (forward solve: P B), or row i (transposed: the interchanges come last)
        if (!a.row_major) {
            if (r < n) {
                const int src = a.trans ? r : sperm[r];
                for (int j = c; j < nr; j += cs) x[r + j * ld] = valid ? B[src + (j0 + j) * a.ldb] : T(0);
            }
        } else if (rr < nr) {
            for (int i = ri0; i < n; i += ris) {
                const int src = a.trans ? i : sperm[i];
                x[i + rr * ld] = valid ? B[(int64_t)src * a.ldb + j0 + rr] : T(0);
            }
        }
        __syncthreads();
        if (a.trans) bsubstitute<T, true>(s, x, ld, n, nr, r, c, cs);
        else bsubstitute<T, false>(s, x, ld, n, nr, r, c, cs);
        if (valid) {
            if (!a.row_major) {
                if (r < n) {
                    const int dst = a.trans ? sperm[r] : r;
                    for (int j = c; j < nr; j += cs) B[dst + (j0 + j) * a.ldb] = x[r + j * ld];
                }
            } else if (rr < nr) {
                for (int i = ri0; i < n; i += ris) {
                    const int dst = a.trans ? sperm[i] : i;
                    B[(int64_t)dst * a.ldb + j0 + rr] = x[i + rr * ld];
                }
            }
        }
        __syncthreads();   // the pass has left LDS before the next one arrives
    }
}

template <typename T>
struct BInvArgs {
    const T* F;
    const int64_t* ipiv;
    T* Ainv;
    int64_t* info;
    int64_t lda, strideF, stride_ipiv, ldi, strideI, batch;
    int n, row_major;
    BGeo g;
};

// the batched inverse: getrs_batched_kernel's forward solve (bsubstitute<T, false>, unchanged) on the columns of P * I, which are made
// in LDS -- row i of a pass is 1 in column sperm[i] -- and never read from HBM; info from the diagonal held in LDS
template <typename T>
__global__ void __launch_bounds__(BT) getri_batched_kernel(BInvArgs<T> a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char bsmem[];
    const BGeo g = a.g;
    const int n = a.n, ld = g.ld;
    const int grp = (int)threadIdx.x >> g.tpm_log, t = (int)threadIdx.x & (g.tpm - 1), lane = t & 63;
    const int64_t b = (int64_t)blockIdx.x * (BT >> g.tpm_log) + grp;
    const bool valid = b < a.batch;
    unsigned char* base = bsmem + (size_t)grp * g.group_bytes;
    T* s = reinterpret_cast<T*>(base);
    T* x = reinterpret_cast<T*>(base + g.off_x);
    int* sperm = reinterpret_cast<int*>(base + g.off_a);   // [n]: row i of P*I is row sperm[i] of I
    const int64_t bb = valid ? b : 0;
    const T* F = a.F + bb * a.strideF;
    T* X = a.Ainv + bb * a.strideI;

    bload_matrix<T>(s, ld, F, a.lda, a.row_major, n, n, g, t, valid);
    if (t < 64) {
        // the interchanges composed into one permutation, as in getrs_batched_kernel
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
    if (t < 64 && valid) {   // first exactly-zero u_ii of this matrix
        const bool z0 = lane < n && s[lane + lane * ld] == T(0), z1 = lane + 64 < n && s[lane + 64 + (lane + 64) * ld] == T(0);
        const bu64 m0 = __ballot(z0), m1 = __ballot(z1);
        if (lane == 0) a.info[b] = m0 ? (int64_t)__ffsll((long long)m0) : (m1 ? (int64_t)(64 + __ffsll((long long)m1)) : (int64_t)0);
    }

    const int r = t & ((1 << g.rt_log) - 1), c = t >> g.rt_log, cs = g.tpm >> g.rt_log;
    const int rr = t & (BNR - 1), ri0 = t >> 3, ris = g.tpm >> 3;   // row-major output: lanes along a row
    for (int j0 = 0; j0 < n; j0 += BNR) {
        const int nr = n - j0 < BNR ? n - j0 : BNR;
        if (r < n) {
            const int one = sperm[r] - j0;
            for (int j = c; j < nr; j += cs) x[r + j * ld] = (j == one) ? T(1) : T(0);
        }
        __syncthreads();
        bsubstitute<T, false>(s, x, ld, n, nr, r, c, cs);
        if (valid) {
            if (!a.row_major) {
                if (r < n)
                    for (int j = c; j < nr; j += cs) X[r + (int64_t)(j0 + j) * a.ldi] = x[r + j * ld];
            } else if (rr < nr) {
                for (int i = ri0; i < n; i += ris) X[(int64_t)i * a.ldi + j0 + rr] = x[i + rr * ld];
            }
        }
        __syncthreads();   // the pass has left LDS before the next one is made
    }
}

// ---- the batched condition estimate (rflu_gecon_batched_*) ------------------------------------------------------
template <typename T>
struct BCondArgs {
    const T* F;
    const double* anorm;
    double* rcond;
    int64_t lda, strideF, batch;
    int n, row_major, norm;
    BGeo g;
};

struct BStat {
    double sum, maxabs, xj;
    int argmax, differs, nonfinite;
};

// The statistics of the group's work vector xs[0 .. n), the same in every thread of the group.  Thread t < n holds x_t (these are the
// threads with column slice 0, in the group's first wave, or its first two for n > 64).  sum|x_t| is added by the tree t += t + s,
// s = 64 .. 1 -- the tree of cond_stats_kernel (condest.hip) on one chunk, whose steps s = 128 and, for n <= 64, s = 64 add +0.0 --; the
// first index of max|x_t| and the two flags do not depend on an order.  sc: the group's scratch (3 doubles, 131 for n > 64).
// Barriers: two (three for n > 64), under no condition but n, which the whole workgroup shares.
template <typename T>
__device__ __forceinline__ BStat bstats(const T* xs, const T* sg, double* sc, int n, int t, int jq)
{
    const int lane = t & 63, w = t >> 6;
    int* si = reinterpret_cast<int*>(sc + 1);
    double v = 0.0, av = -1.0;
    int ai = lane, df = 0, nf = 0;
    if (t < n) {
        const T xv = xs[t];
        v = __builtin_fabs((double)xv);
        av = v;
        ai = t;
        nf = !(v < __builtin_inf());
        df = (xv >= T(0) ? T(1) : T(-1)) != sg[t];
    }
    bu64 bd = __ballot(df), bn = __ballot(nf);
    if (n > 64) {
        if (w == 1) {
            sc[3 + lane] = v;
            sc[67 + lane] = av;
            if (lane == 0) { si[0] = bd != 0; si[1] = bn != 0; }
        }
        __syncthreads();
        if (w == 0) {
            v += sc[3 + lane];
            const double a1 = sc[67 + lane];
            if (a1 > av) { av = a1; ai = 64 + lane; }
            if (si[0]) bd = 1;
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
        si[1] = (bd != 0 ? 1 : 0) | (bn != 0 ? 2 : 0);
    }
    __syncthreads();
    BStat r;
    r.sum = sc[0];
    r.maxabs = sc[2];
    r.argmax = si[0];
    r.differs = si[1] & 1;
    r.nonfinite = (si[1] >> 1) & 1;
    r.xj = __builtin_fabs((double)xs[jq]);
    __syncthreads();   // everybody has read the scratch before its next writer comes
    return r;
}

// Higham's estimator (LAPACK xLACN2 with the integer start and closing vectors of rflu.h) on M = U^-1 L^-1, wholly inside the kernel: the
// factors go into LDS once (bload_matrix), bsubstitute<T, false> on one right-hand side is M x and bsubstitute<T, true> is M^T x; the
// work vector, the previous sign vector and the scratch of bstats live in the 8-column x region of the solve's geometry.
//
// WHY NO GROUP CAN LEAVE ANOTHER ONE AT A BARRIER.  bsubstitute's barriers are workgroup-wide, a workgroup holds 4 / 2 / 1 matrices, and
// the matrices need different numbers of estimator rounds.  So the code below has NO barrier under a condition that depends on a group's
// state: every barrier stands in straight-line code of the round, inside bsubstitute / bstats (whose barrier counts depend on n alone,
// and n is a kernel argument), or in loops whose trip count is n or the round counter.  The round loop is left through ONE test,
// __syncthreads_or(act), whose result is the same in every thread of the workgroup; it runs at most 5 times.  What differs between
// groups is only data: a finished group, a singular one and a group beyond the end of the batch (valid == false) run the same code with
// nr = 0 right-hand sides (bsubstitute then touches nothing) and ignore the statistics, their estimate frozen.
template <typename T>
__global__ void __launch_bounds__(BT) gecon_batched_kernel(BCondArgs<T> a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char bsmem[];
    const BGeo g = a.g;
    const int n = a.n, ld = g.ld;
    const int grp = (int)threadIdx.x >> g.tpm_log, t = (int)threadIdx.x & (g.tpm - 1);
    const int64_t b = (int64_t)blockIdx.x * (BT >> g.tpm_log) + grp;
    const bool valid = b < a.batch;
    unsigned char* base = bsmem + (size_t)grp * g.group_bytes;
    T* s = reinterpret_cast<T*>(base);
    T* xs = reinterpret_cast<T*>(base + g.off_x);       // the work vector ...
    T* sg = xs + ld;                                     // ... the previous sign vector ...
    double* sc = reinterpret_cast<double*>(xs + 2 * ld);   // ... and the scratch of bstats, 8-byte aligned: off_x is, and so is 2 * ld * sizeof(T)
    int* si = reinterpret_cast<int*>(sc + 1);
    const T* F = a.F + (valid ? b : 0) * a.strideF;

    bload_matrix<T>(s, ld, F, a.lda, a.row_major, n, n, g, t, valid);
    if (t == 0) { si[0] = 0; si[1] = 0; }
    const int r = t & ((1 << g.rt_log) - 1), c = t >> g.rt_log, cs = g.tpm >> g.rt_log;
    const bool own = c == 0 && r < n;   // this thread holds x_r (then r == t)
    if (own) sg[r] = T(0);
    __syncthreads();
    {   // a NaN anywhere in the factors (bit 0), an exactly zero u_ii (bit 1): plain stores of the same value, whoever comes last
        int f = 0;
        if (r < n)
            for (int j = c; j < n; j += cs) {
                const T v = s[r + j * ld];
                if (v != v) f |= 1;
                if (j == r && v == T(0)) f |= 2;
            }
        if (f & 1) si[0] = 1;
        if (f & 2) si[1] = 1;
    }
    __syncthreads();
    const int scan = (si[0] ? 1 : 0) | (si[1] ? 2 : 0);
    __syncthreads();

    const bool inf_norm = a.norm == RFLU_NORM_INF;   // ||M||_inf = ||M^T||_1: M and M^T swap roles
    bool act = valid && scan == 0, closing = false, bad = false;
    double est = 0.0;
    int j = 0;
    for (int round = 0; round < 5; ++round) {
        if (act && own) xs[r] = (round == 0 || r == j) ? T(1) : T(0);
        __syncthreads();
        if (inf_norm) bsubstitute<T, true>(s, xs, ld, n, act ? 1 : 0, r, c, cs);
        else bsubstitute<T, false>(s, xs, ld, n, act ? 1 : 0, r, c, cs);
        const BStat s1 = bstats<T>(xs, sg, sc, n, t, j);
        if (act) {
            if (s1.nonfinite) { bad = true; act = false; }
            else if (round == 0) {
                est = s1.sum / (double)n;
                if (n == 1) act = false;
            } else {
                const double est_old = est;
                est = s1.sum;
                if (!s1.differs || est <= est_old) { act = false; closing = true; }
            }
        }
        if (act && own) {
            const T sv = xs[r] >= T(0) ? T(1) : T(-1);
            sg[r] = sv;
            xs[r] = sv;
        }
        __syncthreads();
        if (inf_norm) bsubstitute<T, false>(s, xs, ld, n, act ? 1 : 0, r, c, cs);
        else bsubstitute<T, true>(s, xs, ld, n, act ? 1 : 0, r, c, cs);
        const BStat s2 = bstats<T>(xs, sg, sc, n, t, j);
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
        const T av = (T)(double)(n - 1 + r);
        xs[r] = (r & 1) ? -av : av;
    }
    __syncthreads();
    if (inf_norm) bsubstitute<T, true>(s, xs, ld, n, closing ? 1 : 0, r, c, cs);
    else bsubstitute<T, false>(s, xs, ld, n, closing ? 1 : 0, r, c, cs);
    const BStat s3 = bstats<T>(xs, sg, sc, n, t, 0);
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

bool batched_fits(int64_t m, int64_t n) { return std::max(m, n) <= BATCHED_MAX_DIM; }

template <typename T>
int launch_gecon_batched(Handle* h, int norm, int64_t batch, int64_t n, const T* F, int64_t lda, int64_t strideF, int row_major,
                         const double* anorm, double* rcond)
{
    BCondArgs<T> a;
    a.F = F; a.anorm = anorm; a.rcond = rcond;
    a.lda = lda; a.strideF = strideF; a.batch = batch;
    a.n = (int)n; a.row_major = row_major; a.norm = norm;
    a.g = batched_geo(n, n, sizeof(T), true, false);
    // launch_batched's bookkeeping (Handle::batched_attr_set) has no row for a fourth kernel: the same launch with a flag of its own
    const int groups = BT / a.g.tpm;
    const size_t lds = (size_t)groups * a.g.group_bytes;
    // The kernel also holds 256 bytes of static LDS (the word behind __syncthreads_or), so asking for all 160 KiB as dynamic memory is
    // refused: ask once for what the largest launch needs (n = 128, one group: 138 KiB in Float64), the same value from every handle.
    const BGeo gmax = batched_geo(BATCHED_MAX_DIM, BATCHED_MAX_DIM, sizeof(T), true, false);
    const size_t lds_max = std::max(lds, (size_t)(BT / gmax.tpm) * gmax.group_bytes);
    size_t* asked = &h->gecon_lds_asked[sizeof(T) == 4 ? 1 : 0];
    if (lds > 64 * 1024 && *asked == 0) {
        RFLU_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&gecon_batched_kernel<T>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max));
        *asked = lds_max;
    }
    const int64_t wgs = (batch + groups - 1) / groups;
    ProfScope ps(h, RFLU_K_TRSM, 22.0 * (double)batch * (double)n * (double)n, (double)batch * (double)n * (double)n * sizeof(T));
    hipLaunchKernelGGL(gecon_batched_kernel<T>, dim3((unsigned)wgs), dim3(BT), lds, h->stream, a);
    RFLU_HIP(hipGetLastError());
    return RFLU_OK;
}

template int launch_gecon_batched<double>(Handle*, int, int64_t, int64_t, const double*, int64_t, int64_t, int, const double*, double*);
template int launch_gecon_batched<float>(Handle*, int, int64_t, int64_t, const float*, int64_t, int64_t, int, const double*, double*);

template <typename T>
int launch_getrf_batched(Handle* h, int64_t batch, int64_t m, int64_t n, T* A, int64_t lda, int64_t strideA, int row_major,
                         int64_t* ipiv, int64_t stride_ipiv, int pivot, int64_t* info)
{
    BFactorArgs<T> a;
    a.A = A; a.ipiv = ipiv; a.info = info;
    a.lda = lda; a.strideA = strideA; a.stride_ipiv = stride_ipiv; a.batch = batch;
    a.m = (int)m; a.n = (int)n; a.row_major = row_major; a.pivot = pivot;
    a.g = batched_geo(m, n, sizeof(T), false, false);
    return launch_batched(h, 0, sizeof(T) == 4, &getrf_batched_kernel<T>, a, batch, RFLU_K_PANEL, (double)batch * (double)m * (double)n * (double)std::min(m, n),
                          2.0 * (double)batch * (double)m * (double)n * sizeof(T));
}

template <typename T>
int launch_getrs_batched(Handle* h, int64_t batch, int64_t n, int64_t nrhs, const T* F, int64_t lda, int64_t strideF, int row_major,
                         const int64_t* ipiv, int64_t stride_ipiv, T* B, int64_t ldb, int64_t strideB, int trans)
{
    BSolveArgs<T> a;
    a.F = F; a.ipiv = ipiv; a.B = B;
    a.lda = lda; a.strideF = strideF; a.stride_ipiv = stride_ipiv; a.ldb = ldb; a.strideB = strideB; a.batch = batch; a.nrhs = nrhs;
    a.n = (int)n; a.row_major = row_major; a.trans = trans;
    a.g = batched_geo(n, n, sizeof(T), true, false);
    return launch_batched(h, 1, sizeof(T) == 4, &getrs_batched_kernel<T>, a, batch, RFLU_K_TRSM, 2.0 * (double)batch * (double)n * (double)n * (double)nrhs,
                          (double)batch * ((double)n * (double)n + 2.0 * (double)n * (double)nrhs) * sizeof(T));
}

template <typename T>
int launch_getri_batched(Handle* h, int64_t batch, int64_t n, const T* F, int64_t lda, int64_t strideF, int row_major, const int64_t* ipiv,
                         int64_t stride_ipiv, T* Ainv, int64_t ldi, int64_t strideI, int64_t* info)
{
    BInvArgs<T> a;
    a.F = F; a.ipiv = ipiv; a.Ainv = Ainv; a.info = info;
    a.lda = lda; a.strideF = strideF; a.stride_ipiv = stride_ipiv; a.ldi = ldi; a.strideI = strideI; a.batch = batch;
    a.n = (int)n; a.row_major = row_major;
    a.g = batched_geo(n, n, sizeof(T), true, false);
    return launch_batched(h, 2, sizeof(T) == 4, &getri_batched_kernel<T>, a, batch, RFLU_K_TRSM, 2.0 * (double)batch * (double)n * (double)n * (double)n,
                          2.0 * (double)batch * (double)n * (double)n * sizeof(T));
}

template int launch_getri_batched<double>(Handle*, int64_t, int64_t, const double*, int64_t, int64_t, int, const int64_t*, int64_t, double*,
                                          int64_t, int64_t, int64_t*);
template int launch_getri_batched<float>(Handle*, int64_t, int64_t, const float*, int64_t, int64_t, int, const int64_t*, int64_t, float*,
                                         int64_t, int64_t, int64_t*);

template int launch_getrf_batched<double>(Handle*, int64_t, int64_t, int64_t, double*, int64_t, int64_t, int, int64_t*, int64_t, int, int64_t*);
template int launch_getrf_batched<float>(Handle*, int64_t, int64_t, int64_t, float*, int64_t, int64_t, int, int64_t*, int64_t, int, int64_t*);
template int launch_getrs_batched<double>(Handle*, int64_t, int64_t, int64_t, const double*, int64_t, int64_t, int, const int64_t*, int64_t,
                                          double*, int64_t, int64_t, int);
template int launch_getrs_batched<float>(Handle*, int64_t, int64_t, int64_t, const float*, int64_t, int64_t, int, const int64_t*, int64_t,
                                         float*, int64_t, int64_t, int);

}  // namespace rflu
