// complex.hip -- LU with partial pivoting and the solve that follows it for ComplexF64 / ComplexF32:
// /root/reference/src/lu.jl:97-130 (lu!), :189-263 (the recursion), :290-338 (_generic_lufact!) with a complex element type.
// The kernels besides the GEMM (complex_gemm.hip) and the host side of the recursion.  Element (i, j) of a row-major complex matrix
// sits at R[2 * (i * ld + j)] (re) and the word after it (im).  Every kernel here is an ordinary in-order launch: none waits for
// another workgroup, so there is no residency requirement, no flag to spin on and no timeout status on this path.
#include <algorithm>

#include "complex_dev.hpp"

namespace rflu {

// ---- leaf panel: _generic_lufact! on rows [j0, m) x columns [j0, j0 + w), w <= CLEAF, ONE workgroup ------------------------------------
// Per column k: the modulus argmax over the rows below (strict '>' from 0, the lowest row on ties, a NaN modulus never wins), the
// interchange inside the leaf, inv(pivot) once and one multiply per row, the rank-1 update of the columns right of k.  The first
// CLEAF_LDS_ROWS rows of the leaf live in LDS between one load and one store; rows beyond stream from global memory at every step (they
// stay in L2), so any m is served.  PIVOT = false is NoPivot: the same kernel without search and interchange.
constexpr int CLEAF_THREADS = 256;
constexpr int CLEAF_LDS_ROWS = 96;   // 96 x 32 x 16 B = 48 KiB (Float64)

template <typename R>
struct LeafView {
    R* G;         // global: element (0, 0) of the leaf
    int64_t ld;   // complex elements
    R* S;         // LDS image of the first CLEAF_LDS_ROWS rows, CLEAF complex per row
    __device__ __forceinline__ R* at(int64_t i, int j) const { return i < CLEAF_LDS_ROWS ? S + 2 * (i * CLEAF + j) : G + 2 * (i * ld + j); }
    __device__ __forceinline__ Cx<R> get(int64_t i, int j) const { const R* p = at(i, j); return Cx<R>{p[0], p[1]}; }
    __device__ __forceinline__ void put(int64_t i, int j, Cx<R> z) const { R* p = at(i, j); p[0] = z.re; p[1] = z.im; }
};

template <typename R, bool PIVOT>
__global__ void __launch_bounds__(CLEAF_THREADS) cleaf_kernel(R* __restrict__ A, int64_t ld, int64_t m, int64_t j0, int w,
                                                              int64_t* __restrict__ ipiv, int64_t* __restrict__ info)
{
    __shared__ __attribute__((aligned(16))) R S[2 * CLEAF_LDS_ROWS * CLEAF];
    __shared__ R red_val[CLEAF_THREADS / 64];
    __shared__ int64_t red_row[CLEAF_THREADS / 64];
    __shared__ int64_t piv_row;
    const int tid = threadIdx.x;
    const int64_t mr = m - j0;   // rows of the leaf (>= w: the recursion only sees tall or square blocks)
    const LeafView<R> V{A + 2 * (j0 * ld + j0), ld, S};
    const int64_t lrows = mr < CLEAF_LDS_ROWS ? mr : CLEAF_LDS_ROWS;
    for (int64_t e = tid; e < lrows * w; e += CLEAF_THREADS) {
        const int64_t i = e / w;
        const int j = (int)(e % w);
        const R* p = V.G + 2 * (i * ld + j);
        S[2 * (i * CLEAF + j)] = p[0];
        S[2 * (i * CLEAF + j) + 1] = p[1];
    }
    __syncthreads();
    const int steps = (int)(mr < w ? mr : w);
    for (int k = 0; k < steps; ++k) {
        if (PIVOT) {
            // src/lu.jl:298-307: amax = 0, kp = k; absi > amax moves kp.  Rows ascend per thread, so '>' keeps a thread's lowest row
            R best = R(0);
            int64_t brow = k;
            for (int64_t i = k + tid; i < mr; i += CLEAF_THREADS) {
                const R v = cmodulus(V.get(i, k));
                if (v > best) { best = v; brow = i; }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const R ov = __shfl_down(best, off);
                const int64_t orow = __shfl_down(brow, off);
                if (ov > best || (ov == best && orow < brow)) { best = ov; brow = orow; }
            }
            if ((tid & 63) == 0) { red_val[tid >> 6] = best; red_row[tid >> 6] = brow; }
            __syncthreads();
            if (tid == 0) {
                for (int q = 1; q < CLEAF_THREADS / 64; ++q)
                    if (red_val[q] > best || (red_val[q] == best && red_row[q] < brow)) { best = red_val[q]; brow = red_row[q]; }
                piv_row = brow;
                ipiv[j0 + k] = j0 + brow + 1;
            }
            __syncthreads();
            const int64_t p = piv_row;
            if (p != k && tid < w) {   // src/lu.jl:312-317, on the leaf's own columns (the driver applies it to the others)
                const Cx<R> x = V.get(k, tid), y = V.get(p, tid);
                V.put(k, tid, y);
                V.put(p, tid, x);
            }
            __syncthreads();
        }
        const Cx<R> piv = V.get(k, k);   // (row k < CLEAF <= CLEAF_LDS_ROWS: always in LDS)
        if (piv.re == R(0) && piv.im == R(0)) {   // iszero: both parts; info once, elimination carries on (src/lu.jl:321-334)
            if (tid == 0 && *info == 0) *info = j0 + k + 1;
        } else {
            const Cx<R> inv = cdiv(Cx<R>{R(1), R(0)}, piv);   // src/lu.jl:309-311: one reciprocal, then one multiply per row
            for (int64_t i = k + 1 + tid; i < mr; i += CLEAF_THREADS) V.put(i, k, cmul(V.get(i, k), inv));
        }
        __syncthreads();
        // rank-1 update of columns (k, w): 32 consecutive lanes walk one row
        const int j = k + 1 + (tid & 31);
        if (j < w) {
            const Cx<R> u = V.get(k, j);
            for (int64_t i = k + 1 + (tid >> 5); i < mr; i += CLEAF_THREADS / 32) V.put(i, j, csub(V.get(i, j), cmul(V.get(i, k), u)));
        }
        __syncthreads();
    }
    for (int64_t e = tid; e < lrows * w; e += CLEAF_THREADS) {
        const int64_t i = e / w;
        const int j = (int)(e % w);
        R* p = V.G + 2 * (i * ld + j);
        p[0] = S[2 * (i * CLEAF + j)];
        p[1] = S[2 * (i * CLEAF + j) + 1];
    }
}

template <typename R>
static int launch_cleaf(Handle* h, R* A, int64_t ld, int64_t m, int64_t j0, int64_t w, int64_t* ipiv, int pivot)
{
    const int64_t mr = m - j0;
    ProfScope ps(h, RFLU_K_PANEL, 8.0 * ((double)mr * w * w / 2.0));
    if (pivot) hipLaunchKernelGGL((cleaf_kernel<R, true>), dim3(1), dim3(CLEAF_THREADS), 0, h->stream, A, ld, m, j0, (int)w, ipiv, h->info_dev);
    else hipLaunchKernelGGL((cleaf_kernel<R, false>), dim3(1), dim3(CLEAF_THREADS), 0, h->stream, A, ld, m, j0, (int)w, ipiv, h->info_dev);
    RFLU_HIP(hipGetLastError());
    return RFLU_OK;
}

// ---- base solves on one leaf-sized triangle (n <= CLEAF), one thread per right-hand side, the solution in registers ---------------------
// UPPER = false, UNIT = true: B <- L^-1 B, L unit lower (ldiv!(UnitLowerTriangular(A11), A12), src/lu.jl:235); UPPER = true, UNIT = false:
// B <- U^-1 B, a zero on U's diagonal gives Inf / NaN.  The other two kinds serve the transposed solves (complex_solve.hip): lower with
// the stored diagonal is U^T, upper with a unit diagonal is L^T.  T is n x n row-major (ldt), B is n x nrhs row-major (ldb).
template <typename R, bool UPPER, bool UNIT>
__global__ void __launch_bounds__(128) ctri_base_kernel(int n, int64_t nrhs, const R* __restrict__ T, int64_t ldt, R* __restrict__ B, int64_t ldb)
{
    __shared__ R Ts[2 * CLEAF * CLEAF];
    for (int e = threadIdx.x; e < n * n; e += 128) {
        const int i = e / n, j = e % n;
        Ts[2 * (i * CLEAF + j)] = T[2 * (i * ldt + j)];
        Ts[2 * (i * CLEAF + j) + 1] = T[2 * (i * ldt + j) + 1];
    }
    __syncthreads();
    const int64_t c = (int64_t)blockIdx.x * 128 + threadIdx.x;
    if (c >= nrhs) return;
    Cx<R> x[CLEAF];
#pragma unroll
    for (int s = 0; s < CLEAF; ++s) {
        const int i = UPPER ? CLEAF - 1 - s : s;
        if (i < n) {
            Cx<R> acc{B[2 * (i * ldb + c)], B[2 * (i * ldb + c) + 1]};
#pragma unroll
            for (int t = 0; t < CLEAF; ++t) {
                const bool use = UPPER ? (t > i && t < n) : (t < i);
                if (use) acc = csub(acc, cmul(Cx<R>{Ts[2 * (i * CLEAF + t)], Ts[2 * (i * CLEAF + t) + 1]}, x[t]));
            }
            if (!UNIT) acc = cdiv(acc, Cx<R>{Ts[2 * (i * CLEAF + i)], Ts[2 * (i * CLEAF + i) + 1]});
            x[i] = acc;
            B[2 * (i * ldb + c)] = acc.re;
            B[2 * (i * ldb + c) + 1] = acc.im;
        }
    }
}

template <typename R, bool UPPER, bool UNIT>
static int launch_ctri_base(Handle* h, int64_t n, int64_t nrhs, const R* T, int64_t ldt, R* B, int64_t ldb)
{
    if (n <= 0 || nrhs <= 0) return RFLU_OK;
    ProfScope ps(h, RFLU_K_TRSM, 4.0 * (double)n * n * nrhs);
    hipLaunchKernelGGL((ctri_base_kernel<R, UPPER, UNIT>), dim3((unsigned)((nrhs + 127) / 128)), dim3(128), 0, h->stream, (int)n, nrhs, T, ldt, B, ldb);
    RFLU_HIP(hipGetLastError());
    return RFLU_OK;
}

// above the base size: the recursive splitting of trsm_rec / triu_solve_rec (driver.cpp) on CLEAF boundaries, the complex GEMM in between
template <typename R, bool UNIT = true>
static int ctrsm_rec(Handle* h, int64_t n, int64_t nrhs, const R* L, int64_t ldl, R* B, int64_t ldb)
{
    if (n <= 0 || nrhs <= 0) return RFLU_OK;
    if (n <= CLEAF) return launch_ctri_base<R, false, UNIT>(h, n, nrhs, L, ldl, B, ldb);
    const int64_t n1 = ((n + CLEAF - 1) / CLEAF + 1) / 2 * CLEAF;
    RFLU_TRY((ctrsm_rec<R, UNIT>(h, n1, nrhs, L, ldl, B, ldb)));
    RFLU_TRY(launch_cgemm<R>(h, n - n1, nrhs, n1, L + 2 * (n1 * ldl), ldl, B, ldb, B + 2 * (n1 * ldb), ldb));
    return ctrsm_rec<R, UNIT>(h, n - n1, nrhs, L + 2 * (n1 * ldl + n1), ldl, B + 2 * (n1 * ldb), ldb);
}

template <typename R, bool UNIT = false>
static int ctriu_rec(Handle* h, int64_t n, int64_t nrhs, const R* U, int64_t ldu, R* B, int64_t ldb)
{
    if (n <= 0 || nrhs <= 0) return RFLU_OK;
    if (n <= CLEAF) return launch_ctri_base<R, true, UNIT>(h, n, nrhs, U, ldu, B, ldb);
    const int64_t n1 = ((n + CLEAF - 1) / CLEAF + 1) / 2 * CLEAF;   // rows of the top block
    RFLU_TRY((ctriu_rec<R, UNIT>(h, n - n1, nrhs, U + 2 * (n1 * ldu + n1), ldu, B + 2 * (n1 * ldb), ldb)));
    RFLU_TRY(launch_cgemm<R>(h, n1, nrhs, n - n1, U + 2 * n1, ldu, B + 2 * (n1 * ldb), ldb, B, ldb));
    return ctriu_rec<R, UNIT>(h, n1, nrhs, U, ldu, B, ldb);
}

// the two recursions with the diagonal kind chosen at run time, for complex_solve.hip
template <typename R>
int ctri_lower_rec(Handle* h, int64_t n, int64_t nrhs, const R* T, int64_t ldt, R* B, int64_t ldb, bool unit)
{
    return unit ? ctrsm_rec<R, true>(h, n, nrhs, T, ldt, B, ldb) : ctrsm_rec<R, false>(h, n, nrhs, T, ldt, B, ldb);
}
template <typename R>
int ctri_upper_rec(Handle* h, int64_t n, int64_t nrhs, const R* T, int64_t ldt, R* B, int64_t ldb, bool unit)
{
    return unit ? ctriu_rec<R, true>(h, n, nrhs, T, ldt, B, ldb) : ctriu_rec<R, false>(h, n, nrhs, T, ldt, B, ldb);
}

// ---- interchanges: rows k <-> ipiv[k] - 1 for k in [k0, k1), in order, on columns [c0, c0 + ncols); one thread per column -------------
// (laswp_kernel of laswp.hip works from move lists folded per 64 pivots and vector widths of the real types; this is the plain form)
template <typename R>
__global__ void __launch_bounds__(256) claswp_kernel(R* __restrict__ A, int64_t ld, int64_t rows, int64_t c0, int64_t ncols,
                                                      const int64_t* __restrict__ ipiv, int64_t k0, int64_t k1)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= ncols) return;
    R* col = A + 2 * (c0 + c);
    for (int64_t k = k0; k < k1; ++k) {
        const int64_t p = ipiv[k] - 1;
        if (p != k && p >= 0 && p < rows) {   // (a caller's ipiv outside the matrix is not followed)
            R* a = col + 2 * k * ld;
            R* b = col + 2 * p * ld;
            const R ar = a[0], ai = a[1], br = b[0], bi = b[1];
            a[0] = br; a[1] = bi;
            b[0] = ar; b[1] = ai;
        }
    }
}

template <typename R>
static int launch_claswp(Handle* h, R* A, int64_t ld, int64_t rows, int64_t c0, int64_t ncols, const int64_t* ipiv, int64_t k0, int64_t k1)
{
    if (ncols <= 0 || k1 <= k0) return RFLU_OK;
    ProfScope ps(h, RFLU_K_LASWP, 8.0 * sizeof(R) * (double)ncols * (double)(k1 - k0));
    hipLaunchKernelGGL(claswp_kernel<R>, dim3((unsigned)((ncols + 255) / 256)), dim3(256), 0, h->stream, A, ld, rows, c0, ncols, ipiv, k0, k1);
    RFLU_HIP(hipGetLastError());
    return RFLU_OK;
}

// ---- layout change: out[r][c] = in[c][r], `out` is rows_out x cols_out row-major (a column-major m x n matrix with lda IS a row-major
// n x m matrix with ld = lda).  transpose_kernel of laswp.hip holds a 64 x 65 tile: 66560 B of a 16-byte element, more than a
// workgroup's static LDS, so this is a 32 x 33 one.  The tiles are numbered along blockIdx.x alone (2^31 tiles of 1024 elements are
// beyond any memory), so neither dimension meets a grid limit.  CONJ conjugates on the way (the adjoint solve of complex_solve.hip).
template <typename R, bool CONJ>
__global__ void __launch_bounds__(256) ctranspose_kernel(int64_t rows_out, int64_t cols_out, const R* __restrict__ in, int64_t ld_in,
                                                          R* __restrict__ out, int64_t ld_out, unsigned tiles_x)
{
    __shared__ R tile[32][33][2];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int64_t r0 = (int64_t)(blockIdx.x / tiles_x) * 32, c0 = (int64_t)(blockIdx.x % tiles_x) * 32;
    for (int i = ty; i < 32; i += 8) {
        const int64_t ir = c0 + i, ic = r0 + tx;
        const bool ok = ir < cols_out && ic < rows_out;
        tile[i][tx][0] = ok ? in[2 * (ir * ld_in + ic)] : R(0);
        tile[i][tx][1] = ok ? (CONJ ? -in[2 * (ir * ld_in + ic) + 1] : in[2 * (ir * ld_in + ic) + 1]) : R(0);
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        const int64_t orow = r0 + i, ocol = c0 + tx;
        if (orow < rows_out && ocol < cols_out) {
            out[2 * (orow * ld_out + ocol)] = tile[tx][i][0];
            out[2 * (orow * ld_out + ocol) + 1] = tile[tx][i][1];
        }
    }
}

template <typename R>
int launch_ctranspose(Handle* h, int64_t rows_out, int64_t cols_out, const R* in, int64_t ld_in, R* out, int64_t ld_out, bool conj)
{
    if (rows_out <= 0 || cols_out <= 0) return RFLU_OK;
    const int64_t gx = (cols_out + 31) / 32, gy = (rows_out + 31) / 32;
    if (gx > INT32_MAX || gy > INT32_MAX || gx * gy > INT32_MAX) {   // (more than 2^41 elements: no device holds them)
        set_error("complex layout change: %lld x %lld is beyond one launch", (long long)rows_out, (long long)cols_out);
        return RFLU_ERR_ARG;
    }
    ProfScope ps(h, RFLU_K_TRANSPOSE, 4.0 * sizeof(R) * (double)rows_out * (double)cols_out);
    if (conj) hipLaunchKernelGGL((ctranspose_kernel<R, true>), dim3((unsigned)(gx * gy)), dim3(256), 0, h->stream, rows_out, cols_out, in, ld_in, out,
                                 ld_out, (unsigned)gx);
    else hipLaunchKernelGGL((ctranspose_kernel<R, false>), dim3((unsigned)(gx * gy)), dim3(256), 0, h->stream, rows_out, cols_out, in, ld_in, out,
                            ld_out, (unsigned)gx);
    RFLU_HIP(hipGetLastError());
    return RFLU_OK;
}

// ---- the recursion (Fact<T>::rec of schedule.cpp, src/lu.jl:189-263): columns [j0, j1), rows [j0, m), the diagonal at (j0, j0) ------------
// On return the interchanges ipiv[j0 .. j1) have been applied to columns [j0, j1); the caller applies them to the others.
template <typename R>
struct CFact {
    Handle* h;
    R* A;
    int64_t ld, m;
    int64_t* ipiv;
    int pivot;
    R* at(int64_t i, int64_t j) const { return A + 2 * (i * ld + j); }
    int rec(int64_t j0, int64_t j1) const
    {
        const int64_t w = j1 - j0;
        if (w <= CLEAF) return launch_cleaf<R>(h, A, ld, m, j0, w, ipiv, pivot);
        const int64_t n1 = ((w + CLEAF - 1) / CLEAF + 1) / 2 * CLEAF, jm = j0 + n1;   // split on a leaf boundary
        RFLU_TRY(rec(j0, jm));                                                                                        // src/lu.jl:222
        if (pivot) RFLU_TRY(launch_claswp<R>(h, A, ld, m, jm, j1 - jm, ipiv, j0, jm));                                   // :229-231
        RFLU_TRY(ctrsm_rec<R>(h, n1, j1 - jm, at(j0, j0), ld, at(j0, jm), ld));                                       // :235
        RFLU_TRY(launch_cgemm<R>(h, m - jm, j1 - jm, n1, at(jm, j0), ld, at(j0, jm), ld, at(jm, jm), ld));            // :238 schur_complement!
        RFLU_TRY(rec(jm, j1));                                                                                        // :245
        if (pivot) RFLU_TRY(launch_claswp<R>(h, A, ld, m, j0, n1, ipiv, jm, j1));                                        // :256-260
        return RFLU_OK;
    }
};

// row-major m x n in place; ipiv / info_dev as the leaves write them (info_dev[0] zeroed by the caller)
template <typename R>
static int cgetrf_rm(Handle* h, int64_t m, int64_t n, R* A, int64_t ld, int64_t* ipiv, int pivot)
{
    const int64_t mn = std::min(m, n);
    if (!pivot && ipiv) RFLU_TRY(launch_iota_ipiv(h, ipiv, 0, mn));   // src/lu.jl:111-113
    const CFact<R> f{h, A, ld, m, ipiv, pivot};
    RFLU_TRY(f.rec(0, mn));
    if (n > mn) {   // the fat tail, src/lu.jl:148-154: interchanges, then the unit-lower solve, on the columns right of the square part
        if (pivot) RFLU_TRY(launch_claswp<R>(h, A, ld, m, mn, n - mn, ipiv, 0, mn));
        RFLU_TRY(ctrsm_rec<R>(h, mn, n - mn, A, ld, A + 2 * mn, ld));
    }
    return RFLU_OK;
}

template <typename R>
int cgetrf_cm_dev(Handle* h, int64_t m, int64_t n, R* A, int64_t lda, int64_t* ipiv, int pivot, int64_t* info)
{
    RFLU_TRY(cgetrf_check_args(m, n, A, lda, ipiv, pivot, info));
    *info = 0;
    if (m == 0 || n == 0) return RFLU_OK;
    const int64_t ldw = cworkspace_ld(n);
    RFLU_TRY(ensure_buffer(&h->work, &h->work_bytes, (size_t)m * (size_t)ldw * 2 * sizeof(R)));
    R* W = static_cast<R*>(h->work);
    RFLU_HIP(hipMemsetAsync(h->info_dev, 0, 2 * sizeof(int64_t), h->stream));
    RFLU_TRY(launch_ctranspose<R>(h, m, n, A, lda, W, ldw));
    RFLU_TRY(cgetrf_rm<R>(h, m, n, W, ldw, ipiv, pivot));
    RFLU_TRY(launch_ctranspose<R>(h, n, m, W, ldw, A, lda));
    RFLU_HIP(hipMemcpyAsync(h->info_pinned, h->info_dev, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    RFLU_HIP(hipStreamSynchronize(h->stream));
    *info = h->info_pinned[0];
    h->last_path = RFLU_PATH_HIP_RECURSIVE;
    return RFLU_OK;
}

// the factorization on the caller's row-major n x n array, for the mixed-precision driver (arguments checked there)
template <typename R>
int cgetrf_rm_dev(Handle* h, int64_t n, R* F, int64_t ldf, int64_t* ipiv, int pivot, int64_t* info)
{
    *info = 0;
    if (n == 0) return RFLU_OK;
    RFLU_HIP(hipMemsetAsync(h->info_dev, 0, 2 * sizeof(int64_t), h->stream));
    RFLU_TRY(cgetrf_rm<R>(h, n, n, F, ldf, ipiv, pivot));
    RFLU_HIP(hipMemcpyAsync(h->info_pinned, h->info_dev, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    RFLU_HIP(hipStreamSynchronize(h->stream));
    *info = h->info_pinned[0];
    h->last_path = RFLU_PATH_HIP_RECURSIVE;
    return RFLU_OK;
}

// ldiv!(F, B): B <- U^-1 L^-1 P B; F (n x n, lda) and B (n x nrhs, ldb) column-major, ipiv NULL = NotIPIV
template <typename R>
int cgetrs_cm_dev(Handle* h, int64_t n, int64_t nrhs, const R* F, int64_t lda, const int64_t* ipiv, R* B, int64_t ldb)
{
    RFLU_TRY(cgetrs_check_args(n, nrhs, F, lda, B, ldb));
    if (n == 0 || nrhs == 0) return RFLU_OK;
    const int64_t ldw = cworkspace_ld(n), ldx = cworkspace_ld(nrhs);
    RFLU_TRY(ensure_buffer(&h->work, &h->work_bytes, (size_t)n * (size_t)ldw * 2 * sizeof(R)));
    RFLU_TRY(ensure_buffer(&h->rhs_work, &h->rhs_work_bytes, (size_t)n * (size_t)ldx * 2 * sizeof(R)));
    R* W = static_cast<R*>(h->work);
    R* X = static_cast<R*>(h->rhs_work);
    RFLU_TRY(launch_ctranspose<R>(h, n, n, F, lda, W, ldw));
    RFLU_TRY(launch_ctranspose<R>(h, n, nrhs, B, ldb, X, ldx));
    if (ipiv) RFLU_TRY(launch_claswp<R>(h, X, ldx, n, 0, nrhs, ipiv, 0, n));
    RFLU_TRY(ctrsm_rec<R>(h, n, nrhs, W, ldw, X, ldx));
    RFLU_TRY(ctriu_rec<R>(h, n, nrhs, W, ldw, X, ldx));
    RFLU_TRY(launch_ctranspose<R>(h, nrhs, n, X, ldx, B, ldb));
    RFLU_HIP(hipStreamSynchronize(h->stream));
    return RFLU_OK;
}

template <typename R>
int cgemm_public(Handle* h, int64_t M, int64_t N, int64_t K, const R* A, int64_t lda, const R* B, int64_t ldb, R* C, int64_t ldc)
{
    if (M < 0 || N < 0 || K < 0 || lda < std::max<int64_t>(K, 1) || ldb < std::max<int64_t>(N, 1) || ldc < std::max<int64_t>(N, 1) ||
        (M > 0 && N > 0 && K > 0 && (A == nullptr || B == nullptr || C == nullptr))) {
        set_error("complex gemm: bad arguments M=%lld N=%lld K=%lld lda=%lld ldb=%lld ldc=%lld (or a null pointer)", (long long)M, (long long)N,
                  (long long)K, (long long)lda, (long long)ldb, (long long)ldc);
        return RFLU_ERR_ARG;
    }
    RFLU_TRY(launch_cgemm<R>(h, M, N, K, A, lda, B, ldb, C, ldc));
    RFLU_HIP(hipStreamSynchronize(h->stream));
    return RFLU_OK;
}

#define RFLU_INSTANTIATE_COMPLEX(R)                                                                                                  \
    template int cgetrf_cm_dev<R>(Handle*, int64_t, int64_t, R*, int64_t, int64_t*, int, int64_t*);                                  \
    template int cgetrf_rm_dev<R>(Handle*, int64_t, R*, int64_t, int64_t*, int, int64_t*);                                           \
    template int cgetrs_cm_dev<R>(Handle*, int64_t, int64_t, const R*, int64_t, const int64_t*, R*, int64_t);                        \
    template int cgemm_public<R>(Handle*, int64_t, int64_t, int64_t, const R*, int64_t, const R*, int64_t, R*, int64_t);                \
    template int launch_ctranspose<R>(Handle*, int64_t, int64_t, const R*, int64_t, R*, int64_t, bool);                                 \
    template int ctri_lower_rec<R>(Handle*, int64_t, int64_t, const R*, int64_t, R*, int64_t, bool);                                    \
    template int ctri_upper_rec<R>(Handle*, int64_t, int64_t, const R*, int64_t, R*, int64_t, bool);
RFLU_INSTANTIATE_COMPLEX(double)
RFLU_INSTANTIATE_COMPLEX(float)

}  // namespace rflu
