/*
 * rflu.h -- C ABI of librflu.so: MI355X-native (gfx950, hand-written HIP) recursive LU with partial pivoting.
 *
 * Drop-in boundary for RecursiveFactorization.jl's hot path (citations into /root/reference/):
 *   lu!(A, ipiv, pivot, thread; check, blocksize, threshold) -> LU(A, ipiv, info)     src/lu.jl:97-130
 *   recurse!/_recurse!/reckernel! and their four kernels                              src/lu.jl:132-338
 * The reference is pure Julia and has no FFI today; these entry points are what a `ccall` from its `lu!` method
 * binds (see INTEGRATION.md for the Julia stub).  Conventions follow what LinearAlgebra.LU / LAPACK getrf expect:
 *   - matrices are column-major with leading dimension lda >= m; factors overwrite A (strict lower = L with an
 *     implicit unit diagonal, upper = U);
 *   - ipiv is int64 (Julia BlasInt on ILP64), 1-based, sequential row interchanges, GLOBAL indices
 *     (the reference makes them global through `P2 .+= n1`, src/lu.jl:256-260);
 *   - *info = 0 or the 1-based index of the first exactly-zero pivot, POSITIVE convention; the factorization
 *     continues past it (src/lu.jl:321-334).  The Julia>=1.11 sign flip for NoPivot (src/lu.jl:25,250,324) and
 *     `check` -> SingularException (src/lu.jl:128) are applied by the host glue, not here;
 *   - pivot != 0 is Val(true)/RowMaximum(), pivot == 0 is Val(false)/NoPivot(); with pivot == 0 a non-NULL ipiv is
 *     filled with the identity 1..min(m,n) (src/lu.jl:111-113), NULL plays the role of NotIPIV (src/lu.jl:27-40).
 * Return value of every function: 0 on success, non-zero rflu_status on a runtime (HIP / argument) failure --
 * never a numerical condition.  rflu_last_error() returns a thread-local description of the last failure.
 * A handle owns one device, one stream and its workspaces; one handle is not thread-safe, distinct handles are.
 * No function falls back to a CPU implementation.
 */
#ifndef RFLU_H
#define RFLU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rflu_handle_s* rflu_handle_t;

enum rflu_status {
    RFLU_OK = 0,
    RFLU_ERR_ARG = 1,      /* bad argument (negative size, lda < m, NULL pointer, unsupported size) */
    RFLU_ERR_HIP = 2,      /* a HIP runtime call failed */
    RFLU_ERR_TIMEOUT = 3,  /* the cooperative panel kernel gave up waiting for a peer workgroup */
    RFLU_ERR_NODEVICE = 4, /* no usable gfx950 device */
    RFLU_ERR_PLACEMENT = 5 /* a workgroup of the XCD-local panel kernel ran on an unexpected XCD (results discarded) */
};

/* rflu_last_path values: which implementation served the last getrf call on this handle.  The analogue of the
 * reference's dispatch-routing tests (test/runtests.jl:86-114,162-192): tests assert the HIP path really ran. */
enum rflu_path {
    RFLU_PATH_NONE = 0,
    RFLU_PATH_HIP_RECURSIVE = 1, /* pure Toledo recursion on one stream */
    RFLU_PATH_HIP_BLOCKED = 2,   /* right-looking block columns on one stream (profiling modes, devices without 256 CUs) */
    RFLU_PATH_HIP_LOOKAHEAD = 3, /* block-column lookahead / leaf-wise schedules on CU-masked streams */
    RFLU_PATH_HIP_ENGINE = 4,    /* the leaf-wise chain with every trailing update pulled by the persistent update engine (csrc/engine.hip) */
    RFLU_PATH_HIP_BATCHED = 5    /* rflu_get{rf,rs}_batched_*: one launch of the batched kernels, one group of threads per matrix (csrc/batched.hip, csrc/batched_complex.hip) */
};

/* kernel classes for the built-in per-kernel timers (rflu_profile_*) */
enum rflu_kclass {
    RFLU_K_GEMM = 0,      /* schur_complement!  C -= A*B      (src/lu.jl:265-284), MFMA */
    RFLU_K_TRSM = 1,      /* ldiv!(UnitLowerTriangular(A11), A12) base blocks (src/lu.jl:235) */
    RFLU_K_LASWP = 2,     /* apply_permutation! (src/lu.jl:164-188) */
    RFLU_K_PANEL = 3,     /* _generic_lufact!   (src/lu.jl:290-338) cooperative leaf panel */
    RFLU_K_TRANSPOSE = 4, /* column-major <-> internal row-major layout change at the boundary */
    RFLU_K_MISC = 5,      /* pivot bookkeeping, fills */
    RFLU_K_GEMM_SMALL = 6, /* the same update for K < 256: per-leaf updates and small merges (latency / HBM bound) */
    RFLU_K_LASWP_WIDE = 7, /* apply_permutation! launches that move >= 32 MiB (trailing-update / finished-columns interchanges:
                              the bandwidth-bound share; the per-leaf launches stay in RFLU_K_LASWP and are latency-bound) */
    RFLU_K_COUNT = 8
};

/* ---- lifetime ---- */
int rflu_create(rflu_handle_t* handle, int device);
int rflu_destroy(rflu_handle_t handle);
/* The library's RFLU_* tuning / debugging variables (INTEGRATION.md lists them) are read from the environment once, by
 * rflu_create; this reads them again for an existing handle (a host that changes them between calls: the test-suite). */
int rflu_reload_tuning(rflu_handle_t handle);
const char* rflu_last_error(void);
int rflu_version(void);
/* Use an existing HIP stream (hipStream_t passed as void*); NULL restores the handle's own stream. */
int rflu_set_stream(rflu_handle_t handle, void* hip_stream);
int rflu_synchronize(rflu_handle_t handle);
int rflu_last_path(rflu_handle_t handle);
/* The handle's second stream (hipStream_t as void*): restricted by a CU mask to 224 of the 256 CUs so that cooperative
 * panel kernels issued on another stream always find 32 free CUs.  Used by the lookahead drivers (single- and
 * multi-GPU) for the bulk trailing updates. */
int rflu_update_stream(rflu_handle_t handle, void** hip_stream_out);
/* Measurement aid (scripts/microbench_*.py): about `usec` microseconds of register-only MFMA load, launched asynchronously on
 * the CU-masked update stream.  Not part of the reference interface. */
int rflu_debug_heat(rflu_handle_t handle, double usec);
/* Measurement aid (scripts/gate_trace.py): with RFLU_GATE_TRACE=1 in the environment the leaf-wise schedule stamps the wall
 * clock (100 MHz ticks) when each stream passes each leaf; copies the 3 x 4096 stamps to `out` (host). */
int rflu_debug_gate_stamps(rflu_handle_t handle, long long* out);
/* RFLU_ENGINE_TRACE=1 (measurement): workgroup-time accumulators of the last launch of the persistent update engine on this handle, in
 * 100 MHz ticks summed over its workgroups: out8[0] block-column tiles, [1] leaf-window tiles, [2] interchange strips + block-row solves,
 * [3] deferred interchanges on finished columns, [4] everything between two units, [5] (part of 4) asleep, [6] (part of 4) publications */
int rflu_debug_engine_acct(rflu_handle_t handle, long long* out8);

/* ---- the boundary: lu!(A, ipiv, pivot; blocksize) on HOST buffers (caller-owned, column-major) ----
 * Replaces src/lu.jl:114-126 (recursive path + unblocked fallback) for Float64 / Float32.
 * blocksize: < 0 = pure Toledo recursion on the whole matrix, one stream (the reference's structure, src/lu.jl:189-263);
 *            > 0 = width of the outer right-looking block column (`blocksize` re-read as the GPU panel
 *                  width, BASELINE config 2 sweeps 64/128/256; rounded up to a multiple of 64).  Tall, update-bound block
 *                  columns: factored by the same recursion with one block column of lookahead (the next block column is
 *                  updated and factored while the rest of the trailing update still runs on a second stream); from the first
 *                  panel of at most 8192 rows (Float32: 16384) on, for widths 128..512: leaf by leaf, right-looking, with only
 *                  the next leaf's 64 columns on the critical path;
 *            = 0 = library default, measured on MI355X: pure recursion below 1024 columns, then block columns of
 *                  256 (<= 11264 columns), 512 (<= 16384: pivoted, not fat and at most 16384 rows these go through the persistent
 *                  update engine, RFLU_PATH_HIP_ENGINE), 1024 (<= 24576), 2048 above. */
int rflu_getrf_f64(rflu_handle_t handle, int64_t m, int64_t n, double* A_host, int64_t lda, int64_t* ipiv_host,
                   int pivot, int64_t blocksize, int64_t* info);
int rflu_getrf_f32(rflu_handle_t handle, int64_t m, int64_t n, float* A_host, int64_t lda, int64_t* ipiv_host,
                   int pivot, int64_t blocksize, int64_t* info);

/* ---- same, DEVICE-resident (A_dev, ipiv_dev are device pointers on the handle's device; info is a host pointer).
 * Column-major in, column-major out; asynchronous work is completed before return. */
int rflu_getrf_f64_dev(rflu_handle_t handle, int64_t m, int64_t n, double* A_dev, int64_t lda, int64_t* ipiv_dev,
                       int pivot, int64_t blocksize, int64_t* info);
int rflu_getrf_f32_dev(rflu_handle_t handle, int64_t m, int64_t n, float* A_dev, int64_t lda, int64_t* ipiv_dev,
                       int pivot, int64_t blocksize, int64_t* info);

/* ---- the solve step that follows the path in every caller: ldiv!(F::LU, B), i.e. B <- U^-1 L^-1 P B ----
 * Reference: stdlib ldiv!(::LU) on the object lu! returns (LinearSolve's solve!), and the package's own ldiv! for
 * NotIPIV factors (src/lu.jl:60-64).  F/ipiv exactly as rflu_getrf_* left them (column-major packed L\U, 1-based
 * ipiv; ipiv == NULL plays NotIPIV); B is n x nrhs column-major, overwritten with the solution.  A singular U
 * (info != 0) yields Inf/NaN like LAPACK getrs; the host glue checks info first. */
int rflu_getrs_f64(rflu_handle_t handle, int64_t n, int64_t nrhs, const double* F_host, int64_t lda,
                   const int64_t* ipiv_host, double* B_host, int64_t ldb);
int rflu_getrs_f32(rflu_handle_t handle, int64_t n, int64_t nrhs, const float* F_host, int64_t lda,
                   const int64_t* ipiv_host, float* B_host, int64_t ldb);
int rflu_getrs_f64_dev(rflu_handle_t handle, int64_t n, int64_t nrhs, const double* F_dev, int64_t lda,
                       const int64_t* ipiv_dev, double* B_dev, int64_t ldb);
int rflu_getrs_f32_dev(rflu_handle_t handle, int64_t n, int64_t nrhs, const float* F_dev, int64_t lda,
                       const int64_t* ipiv_dev, float* B_dev, int64_t ldb);
/* same on row-major device data (F as left by rflu_getrf_rm_*; B is n x nrhs row-major with leading dimension ldb) */
int rflu_getrs_rm_f64_dev(rflu_handle_t handle, int64_t n, int64_t nrhs, const double* R_dev, int64_t ld,
                          const int64_t* ipiv_dev, double* B_dev, int64_t ldb);
int rflu_getrs_rm_f32_dev(rflu_handle_t handle, int64_t n, int64_t nrhs, const float* R_dev, int64_t ld,
                          const int64_t* ipiv_dev, float* B_dev, int64_t ldb);

/* ---- the TRANSPOSED solve: ldiv!(F', B) / ldiv!(transpose(F), B), i.e. B <- P^T L^-T U^-T B = A^-T B ----
 * LAPACK getrs with trans = 'T' (real element types only, so adjoint and transpose coincide).  Arguments, argument checks, stream
 * use and the synchronisation before return exactly as the rflu_getrs_* entry of the same shape; ipiv == NULL plays NotIPIV;
 * a singular U (info != 0) yields Inf/NaN like LAPACK, the host glue checks info first.
 *   - The column-major entries read F IN PLACE: a column-major F read as a row-major array with ld = lda is F^T (lower triangle
 *     with the diagonal = U^T, strict upper triangle = L^T), so no n x n layout change happens.  Any lda >= n and any pointer
 *     aligned to the element size are accepted; with lda * sizeof(T) and the pointer multiples of 16 bytes the blocks arrive as
 *     16-byte loads, otherwise element by element (same arithmetic, same results).
 *   - The row-major entries (F as left by rflu_getrf_rm_*) pay one layout change of R into the handle's workspace first: there the
 *     transposed view is not free.
 *   - Served by the cooperative chain kernels for ANY nrhs (passes of 8 right-hand sides up to 32, passes of 64 beyond); they cover
 *     n <= 65536.  A larger n returns RFLU_ERR_ARG with a message: there is no recursive form of this solve and no CPU fallback. */
int rflu_getrs_trans_f64(rflu_handle_t handle, int64_t n, int64_t nrhs, const double* F_host, int64_t lda,
                         const int64_t* ipiv_host, double* B_host, int64_t ldb);
int rflu_getrs_trans_f32(rflu_handle_t handle, int64_t n, int64_t nrhs, const float* F_host, int64_t lda,
                         const int64_t* ipiv_host, float* B_host, int64_t ldb);
int rflu_getrs_trans_f64_dev(rflu_handle_t handle, int64_t n, int64_t nrhs, const double* F_dev, int64_t lda,
                             const int64_t* ipiv_dev, double* B_dev, int64_t ldb);
int rflu_getrs_trans_f32_dev(rflu_handle_t handle, int64_t n, int64_t nrhs, const float* F_dev, int64_t lda,
                             const int64_t* ipiv_dev, float* B_dev, int64_t ldb);
int rflu_getrs_trans_rm_f64_dev(rflu_handle_t handle, int64_t n, int64_t nrhs, const double* R_dev, int64_t ld,
                                const int64_t* ipiv_dev, double* B_dev, int64_t ldb);
int rflu_getrs_trans_rm_f32_dev(rflu_handle_t handle, int64_t n, int64_t nrhs, const float* R_dev, int64_t ld,
                                const int64_t* ipiv_dev, float* B_dev, int64_t ldb);

/* ---- BATCHED: `batch` independent small systems in one call (getrfBatched / getrsBatched; the sizes the reference was written
 * for -- recursion threshold 40, src/lu.jl:90 -- where one matrix cannot occupy a GPU).  Strided, not arrays of pointers:
 *   - matrix b starts at A_dev + b*strideA; row_major = 0: element (i,j) at [i + j*lda] (lda >= m), row_major = 1: at [i*lda + j]
 *     (lda >= n); the matrices of a batch must not overlap;
 *   - ipiv of matrix b at ipiv_dev + b*stride_ipiv (stride_ipiv >= min(m,n)), 1-based and sequential as everywhere in this header;
 *     ipiv_dev == NULL only with pivot == 0 (NotIPIV); a non-NULL ipiv with pivot == 0 is filled with the identity (src/lu.jl:111-113);
 *   - info_dev: DEVICE array of `batch` entries, required: 0 or the index of the first exactly-zero pivot of that matrix, positive
 *     convention.  Per matrix the semantics of _generic_lufact! (src/lu.jl:290-338): strict-'>' argmax from 0 with the lowest row on
 *     ties, reciprocal-multiply scaling, a zero pivot sets info once and the factorization carries on; pivot == 0 is NoPivot;
 *   - rflu_getrs_batched_*: F / ipiv as the factorization left them, B (n x nrhs per matrix, matrix b at B_dev + b*strideB) in the
 *     ORIENTATION OF F: row_major = 0: (i,r) at [i + r*ldb], row_major = 1: at [i*ldb + r]; trans != 0 solves A^T x = b (U^T, L^T, then
 *     the interchanges undone).  Any nrhs.  A singular matrix yields Inf/NaN in its own right-hand sides only;
 *   - max(m, n) <= 128 (both element types): ONE launch, a group of 64..256 threads per matrix, the matrix in LDS between its one load
 *     and its one store; rflu_last_path reports RFLU_PATH_HIP_BATCHED.  Larger matrices: a loop over the single-matrix device path on
 *     the handle's stream -- there so that the interface has no size cliff; it is correct, NOT fast (a launch chain and a
 *     synchronisation per matrix), and rflu_last_path reports what the last single factorization reports;
 *   - batch == 0, m == 0 or n == 0 (nrhs == 0): success, nothing launched.  Negative sizes, lda / strides too small, NULL pointers:
 *     RFLU_ERR_ARG with a message.  Work goes on the handle's stream and is complete on return. */
int rflu_getrf_batched_f64_dev(rflu_handle_t handle, int64_t batch, int64_t m, int64_t n, double* A_dev, int64_t lda, int64_t strideA,
                               int row_major, int64_t* ipiv_dev, int64_t stride_ipiv, int pivot, int64_t* info_dev);
int rflu_getrf_batched_f32_dev(rflu_handle_t handle, int64_t batch, int64_t m, int64_t n, float* A_dev, int64_t lda, int64_t strideA,
                               int row_major, int64_t* ipiv_dev, int64_t stride_ipiv, int pivot, int64_t* info_dev);
int rflu_getrs_batched_f64_dev(rflu_handle_t handle, int64_t batch, int64_t n, int64_t nrhs, const double* F_dev, int64_t lda,
                               int64_t strideF, int row_major, const int64_t* ipiv_dev, int64_t stride_ipiv, double* B_dev, int64_t ldb,
                               int64_t strideB, int trans);
int rflu_getrs_batched_f32_dev(rflu_handle_t handle, int64_t batch, int64_t n, int64_t nrhs, const float* F_dev, int64_t lda,
                               int64_t strideF, int row_major, const int64_t* ipiv_dev, int64_t stride_ipiv, float* B_dev, int64_t ldb,
                               int64_t strideB, int trans);

/* ---- INVERSE, DETERMINANT: what LinearAlgebra offers on the object lu! returns besides the solve (inv / inv!, det, logabsdet,
 * logdet on an LU), from the packed factors alone.  Kernels and the two sweeps: csrc/inverse.hip, DESIGN.md section 4.4.
 * Everything is an in-order launch on the handle's stream -- no kernel of these entries waits for another workgroup -- and no sum is
 * formed by read-modify-write on shared words: results are bit-identical from run to run.  Work is complete on return.
 *
 * (log|det A|, sign det A) from the factors.  The diagonal sits at F[i*(ld+1)] in BOTH layouts, so one entry serves column- and
 * row-major factors.  ipiv NULL = NotIPIV.  *logabs_out, *sign_out: host, required.  Julia's logabsdet(::LU): sum of log|u_ii|;
 * sign = product of sign(u_ii) times (-1)^#{k : ipiv[k] != k+1}.  Float64 arithmetic for both element types; chunks of 1024 diagonal
 * entries are summed by a fixed tree, the chunk sums in index order.  A zero u_ii gives (-Inf, 0); a NaN u_ii gives (NaN, NaN).
 * n == 0: (0, 1).  The host entry copies the diagonal and ipiv only. */
int rflu_logabsdet_f64_dev(rflu_handle_t handle, int64_t n, const double* F_dev, int64_t ld, const int64_t* ipiv_dev,
                           double* logabs_out, double* sign_out);
int rflu_logabsdet_f32_dev(rflu_handle_t handle, int64_t n, const float* F_dev, int64_t ld, const int64_t* ipiv_dev,
                           double* logabs_out, double* sign_out);
int rflu_logabsdet_f64(rflu_handle_t handle, int64_t n, const double* F_host, int64_t ld, const int64_t* ipiv_host,
                       double* logabs_out, double* sign_out);
int rflu_logabsdet_f32(rflu_handle_t handle, int64_t n, const float* F_host, int64_t ld, const int64_t* ipiv_host,
                       double* logabs_out, double* sign_out);
/* the same for every matrix of a batch (matrix b at F_dev + b*strideF, ipiv at ipiv_dev + b*stride_ipiv as in the BATCHED entries
 * below); logabs_dev / sign_dev: DEVICE arrays of `batch` doubles.  One launch, one workgroup per matrix, any n (only diagonals are
 * read: no size cliff); bit-identical to the single-matrix entry on the same factors. */
int rflu_logabsdet_batched_f64_dev(rflu_handle_t handle, int64_t batch, int64_t n, const double* F_dev, int64_t lda, int64_t strideF,
                                   const int64_t* ipiv_dev, int64_t stride_ipiv, double* logabs_dev, double* sign_dev);
int rflu_logabsdet_batched_f32_dev(rflu_handle_t handle, int64_t batch, int64_t n, const float* F_dev, int64_t lda, int64_t strideF,
                                   const int64_t* ipiv_dev, int64_t stride_ipiv, double* logabs_dev, double* sign_dev);
/* LAPACK getri: F (packed L\U exactly as rflu_getrf_* left it) is overwritten by A^-1 -- the factors are gone afterwards.  ipiv NULL =
 * NotIPIV.  *info (host, required): 0, or the 1-based index of the first exactly-zero u_ii -- then F is left UNTOUCHED and the return
 * value is still RFLU_OK (a numerical condition, like everywhere in this header).  n == 0: success, nothing launched.
 *   - About 4n^3/3 flops (n^3/3 for U^-1 in place, n^3 for the sweep with L), all of it through the MFMA GEMM; against 2n^3 and four
 *     n x n arrays for rflu_getrs_* on an explicit identity.  Workspace beyond F, owned by the handle: one buffer of 512 x n elements
 *     and the 64x64 diagonal inverses of both triangles (2 * ceil(n/64) * 4096 elements); nothing of size n x n.
 *   - The column-major entries work IN PLACE on F read as a row-major array with ld = lda (that is F^T, and A^-1 column-major is
 *     A^-T row-major): no layout change.  Any lda >= n and any pointer aligned to the element size are accepted; where lda *
 *     sizeof(T) or the pointer is no multiple of 16 bytes the GEMM loads element by element (slower, same arithmetic; h->work is
 *     not used).  Entries of F beyond the n x n matrix (rows n .. lda-1 of a column) are never written.
 *   - The row-major entry pays one layout change of R into the handle's workspace and one back (the trade of rflu_getrs_trans_rm_*).
 *   - The host entry: H2D, the device entry, D2H (not at all when info != 0). */
int rflu_getri_f64_dev(rflu_handle_t handle, int64_t n, double* F_dev, int64_t lda, const int64_t* ipiv_dev, int64_t* info);
int rflu_getri_f32_dev(rflu_handle_t handle, int64_t n, float* F_dev, int64_t lda, const int64_t* ipiv_dev, int64_t* info);
int rflu_getri_rm_f64_dev(rflu_handle_t handle, int64_t n, double* R_dev, int64_t ld, const int64_t* ipiv_dev, int64_t* info);
int rflu_getri_rm_f32_dev(rflu_handle_t handle, int64_t n, float* R_dev, int64_t ld, const int64_t* ipiv_dev, int64_t* info);
int rflu_getri_f64(rflu_handle_t handle, int64_t n, double* F_host, int64_t lda, const int64_t* ipiv_host, int64_t* info);
int rflu_getri_f32(rflu_handle_t handle, int64_t n, float* F_host, int64_t lda, const int64_t* ipiv_host, int64_t* info);
/* Ainv_b <- A_b^-1 from batched factors (getriBatched); out of place (Ainv must not overlap F), Ainv in the ORIENTATION OF F with its
 * own ldi / strideI.  info_dev (device, batch entries, required): 0 or the first zero u_ii of that matrix, whose output is then
 * Inf/NaN in its own matrix only.  n <= 128: ONE launch, the factors in LDS once, the identity right-hand sides made in LDS.  Larger
 * matrices: a loop over a device copy and the single-matrix getri -- correct, NOT fast, no size cliff.  Argument rules and the
 * batch == 0 / n == 0 cases as rflu_getrs_batched_*. */
int rflu_getri_batched_f64_dev(rflu_handle_t handle, int64_t batch, int64_t n, const double* F_dev, int64_t lda, int64_t strideF,
                               int row_major, const int64_t* ipiv_dev, int64_t stride_ipiv, double* Ainv_dev, int64_t ldi,
                               int64_t strideI, int64_t* info_dev);
int rflu_getri_batched_f32_dev(rflu_handle_t handle, int64_t batch, int64_t n, const float* F_dev, int64_t lda, int64_t strideF,
                               int row_major, const int64_t* ipiv_dev, int64_t stride_ipiv, float* Ainv_dev, int64_t ldi,
                               int64_t strideI, int64_t* info_dev);

/* ---- NORMS, CONDITION: what LAPACK pairs with getrf (lange + gecon) and Julia's cond(A, 1) / cond(A, Inf) is made of: the operator
 * norm of A BEFORE the factorization overwrites it, then an estimate of rcond = 1 / (||A|| ||A^-1||) from the packed factors alone.
 * Float64 / Float32 here; the complex form is the block COMPLEX NORMS, CONDITION below.  Kernels: csrc/condest.hip and
 * gecon_batched_kernel in csrc/batched.hip; DESIGN.md section 4.11.
 * Every sum is formed in Float64 for both element types, in a fixed order -- no read-modify-write on shared words, partial sums per
 * chunk, the chunks combined in index order -- so results are bit-identical from run to run.  Work goes on the handle's stream and is
 * complete on return (the batched lange entry included).
 *
 * rflu_lange_*: norm = RFLU_NORM_ONE (largest column sum of |a_ij|) or RFLU_NORM_INF (largest row sum); any other value is
 * RFLU_ERR_ARG.  A is m x n, element (i, j) at [i + j*lda] (row_major = 0, lda >= m) or [i*lda + j] (row_major = 1, lda >= n); it is
 * read once, lanes along the contiguous dimension, in 16-byte loads where the pointer and lda allow and element by element otherwise --
 * the same sums either way.  Padding behind a column / row is never read.  A NaN anywhere gives NaN (LAPACK lange), an Inf gives Inf;
 * m == 0 or n == 0 gives 0.  *out: host, required.  The batched entry (matrix b at A_dev + b*strideA; out_dev: DEVICE array of `batch`
 * doubles) runs one workgroup per matrix up to max(m, n) <= 128 and the single entry's kernels per matrix above, and agrees with the
 * single entry on the same matrix bit for bit. */
enum rflu_norm { RFLU_NORM_ONE = 1, RFLU_NORM_INF = 2 };
int rflu_lange_f64_dev(rflu_handle_t handle, int norm, int64_t m, int64_t n, const double* A_dev, int64_t lda, int row_major,
                       double* out);
int rflu_lange_f32_dev(rflu_handle_t handle, int norm, int64_t m, int64_t n, const float* A_dev, int64_t lda, int row_major,
                       double* out);
int rflu_lange_batched_f64_dev(rflu_handle_t handle, int norm, int64_t batch, int64_t m, int64_t n, const double* A_dev, int64_t lda,
                               int64_t strideA, int row_major, double* out_dev);
int rflu_lange_batched_f32_dev(rflu_handle_t handle, int norm, int64_t batch, int64_t m, int64_t n, const float* A_dev, int64_t lda,
                               int64_t strideA, int row_major, double* out_dev);
/* rflu_gecon_*: *rcond_out (host, required) = 1 / (anorm * est), est an estimate (a lower bound up to rounding) of ||A^-1|| in the norm
 * `norm`; anorm = that norm of A, from rflu_lange_* before the factorization.  There is no ipiv argument, as in LAPACK: with A = P^T L U,
 * ||A^-1||_1 = ||U^-1 L^-1 P||_1 = ||U^-1 L^-1||_1, and the same holds for the Inf norm.  F is ONLY READ (packed L\U as rflu_getrf_* /
 * rflu_getrf_rm_* left it; the host entry: H2D, then the device entry).
 *   - The estimator is Higham's (LAPACK xLACN2, at most 5 iterations) on M = U^-1 L^-1, with TWO DELIBERATE DIFFERENCES from LAPACK that
 *     make every vector entering a solve a vector of small integers: (1) the start vector is all ones and the first estimate is
 *     sum|v_i| / n (LAPACK starts from 1/n); (2) the closing alternating vector is x_i = (-1)^i (n - 1 + i), i = 0 .. n-1, and its bound
 *     2 sum|v_i| / (3 n (n - 1)) (LAPACK: 1 + i/(n-1) and 2 sum / (3n)).  n = 1: the estimate is |v_0| of the first solve.  The control
 *     flow is xLACN2's: sign(v) = v >= 0 ? +1 : -1; stop on a repeated sign vector; stop when est <= est_old; j = the FIRST index of
 *     max|x_i|; stop when |x_jlast| == |x_j|; the result is the larger of the iteration's estimate and the alternating-vector bound.
 *     For RFLU_NORM_INF, M and M^T swap roles.  At most 11 solves with one right-hand side, 2n^2 flops each.
 *   - One layout change per call: the row-major image of column-major factors (the transposed image of row-major ones) is made once in
 *     the handle's workspace; every M x runs on the row-major image and every M^T x on the transposed view through the cooperative chain
 *     kernels of rflu_getrs_* / rflu_getrs_trans_* with ipiv = NULL.  Between two solves: fixed-order vector kernels (chunks of 1024, a
 *     fixed tree, chunks in index order) and one read of a few scalars by the host.
 *   - No scaling as in xLATRS: a non-finite estimate (overflow in the substitution) gives rcond = 0.
 *   - n == 0: 1.  anorm NaN: NaN.  anorm == 0: 0.  An exactly zero u_ii: 0, before any solve is launched.  A NaN in the factors: NaN.
 *     Where several apply the first in this order decides: factors with an exactly zero u_ii AND a NaN give 0, not NaN (single and
 *     batched entries alike).
 *     anorm < 0, norm not 1 / 2, lda < n, NULL pointers: RFLU_ERR_ARG.  n > 65536 (the transposed chain's limit): RFLU_ERR_ARG with a
 *     message.
 *   - The handle's workspaces are shared with the other entries and refilled by each of them: a solve, an inverse or a factorization
 *     after rflu_gecon_* on the same handle is bit-identical to one on a fresh handle.
 * rflu_gecon_batched_*: the same for every matrix of a batch (matrix b at F_dev + b*strideF in either orientation; anorm_dev, rcond_dev:
 * DEVICE arrays of `batch` doubles).  n <= 128: ONE launch, the factors in LDS once, the whole estimator inside the kernel (the
 * batched substitutions of rflu_getrs_batched_* on one right-hand side), every group of a workgroup running the same number of rounds.
 * Larger n: a loop over the single entry -- correct, NOT fast, no size cliff.  Special values per member as above, except that a
 * member's anorm < 0 gives NaN in its own output; one member's NaN or singularity touches its own output only.  batch == 0: success;
 * n == 0: every rcond is 1. */
int rflu_gecon_f64_dev(rflu_handle_t handle, int norm, int64_t n, const double* F_dev, int64_t lda, double anorm, double* rcond_out);
int rflu_gecon_f32_dev(rflu_handle_t handle, int norm, int64_t n, const float* F_dev, int64_t lda, double anorm, double* rcond_out);
int rflu_gecon_rm_f64_dev(rflu_handle_t handle, int norm, int64_t n, const double* R_dev, int64_t ld, double anorm, double* rcond_out);
int rflu_gecon_rm_f32_dev(rflu_handle_t handle, int norm, int64_t n, const float* R_dev, int64_t ld, double anorm, double* rcond_out);
int rflu_gecon_f64(rflu_handle_t handle, int norm, int64_t n, const double* F_host, int64_t lda, double anorm, double* rcond_out);
int rflu_gecon_f32(rflu_handle_t handle, int norm, int64_t n, const float* F_host, int64_t lda, double anorm, double* rcond_out);
int rflu_gecon_batched_f64_dev(rflu_handle_t handle, int norm, int64_t batch, int64_t n, const double* F_dev, int64_t lda,
                               int64_t strideF, int row_major, const double* anorm_dev, double* rcond_dev);
int rflu_gecon_batched_f32_dev(rflu_handle_t handle, int norm, int64_t batch, int64_t n, const float* F_dev, int64_t lda,
                               int64_t strideF, int row_major, const double* anorm_dev, double* rcond_dev);

/* ---- COMPLEX: lu! / ldiv! for ComplexF64 / ComplexF32 (suffixes _cf64 / _cf32; csrc/complex.hip, csrc/complex_gemm.hip,
 * csrc/complex_solve.hip, DESIGN.md sections 4.5 and 4.6).  The reference's lu! with a complex element type (src/lu.jl:97-130, :189-263, :290-338; test/runtests.jl:33-84).
 * A complex array crosses the boundary as double* / float* pointing at INTERLEAVED (re, im) pairs, the storage of Julia's Complex{T}
 * and numpy's complex128 / complex64; every lda / ldb / ldc counts COMPLEX elements.  A pointer aligned to the real type is enough.
 *   - pivot of column k: the row with the largest MODULUS abs(z) = hypot(re, im) in the element's real precision, strict '>' from 0, so
 *     the lowest row wins a tie and a NaN modulus never wins.  This is the reference's rule, NOT LAPACK's |re| + |im|: LAPACK's ipiv is
 *     no comparator for these entries;
 *   - a pivot is zero when both parts are: *info is set once (positive, 1-based) and the elimination carries on; the host glue applies
 *     the NoPivot sign flip and `check`.  Scaling multiplies by inv(pivot), formed once per column;
 *   - ipiv, pivot, NULL = NotIPIV (with pivot == 0 only; a non-NULL ipiv is then filled with 1..min(m,n)) as for rflu_getrf_f64_dev;
 *     any m, n >= 0, fat matrices get the reference's tail (src/lu.jl:148-154); m == 0 or n == 0: success, nothing launched.  There is
 *     no blocksize: one schedule, the Toledo recursion on the handle's stream down to leaves of 32 columns, all of its n^3 work in the
 *     complex MFMA GEMM; rflu_last_path reports RFLU_PATH_HIP_RECURSIVE.  No size cliff, no CPU fallback;
 *   - every kernel is an in-order launch on the handle's stream and NONE waits for another workgroup: no cooperative launch, no flag,
 *     no RFLU_ERR_TIMEOUT from these entries.  Work is complete on return;
 *   - rflu_getrs_*: ldiv!(F, B) for any nrhs, F / ipiv as the factorization left them; a singular U yields Inf/NaN, no error status.
 *     The batched form is rflu_get{rf,rs}_batched_cf64_dev / _cf32_dev below, inv! / det / logabsdet from these factors are
 *     rflu_getri_c* / rflu_logabsdet_c* further below, the mixed-precision form is rflu_mixed_get{rf,rs}_cf64_dev;
 *   - rflu_getrs_trans_*: ldiv!(transpose(F), B) and ldiv!(F', B), which differ for these element types, so the entries take `conj`:
 *     conj = 0 solves transpose(A) x = b (LAPACK 'T', B <- P^T L^-T U^-T B), conj = 1 solves A' x = b (LAPACK 'C', B <- P^T L^-H U^-H B),
 *     any other value is RFLU_ERR_ARG.  Everything else is as rflu_getrs_*: storage, lda / ldb, NULL ipiv = NotIPIV, alignment, any
 *     lda >= n, Inf/NaN and RFLU_OK for a singular U, n == 0 or nrhs == 0 succeed with nothing launched, the same argument checks.
 *     F is ONLY READ, IN PLACE (a column-major F read row-major is its transpose): no n x n copy, no workspace that grows as n^2.
 *     Up to 8 right-hand sides are solved in B's own columns (csrc/complex_solve.hip), more go through a
 *     row-major image of B and the complex GEMM.  Results are bit-identical from run to run and whatever the alignment of F and lda;
 *   - the host entries: H2D, the device entry, D2H -- only on success, so a failed call leaves the caller's arrays as they were. */
int rflu_getrf_cf64(rflu_handle_t handle, int64_t m, int64_t n, double* A_host, int64_t lda, int64_t* ipiv_host, int pivot,
                    int64_t* info);
int rflu_getrf_cf32(rflu_handle_t handle, int64_t m, int64_t n, float* A_host, int64_t lda, int64_t* ipiv_host, int pivot,
                    int64_t* info);
int rflu_getrf_cf64_dev(rflu_handle_t handle, int64_t m, int64_t n, double* A_dev, int64_t lda, int64_t* ipiv_dev, int pivot,
                        int64_t* info);
int rflu_getrf_cf32_dev(rflu_handle_t handle, int64_t m, int64_t n, float* A_dev, int64_t lda, int64_t* ipiv_dev, int pivot,
                        int64_t* info);
int rflu_getrs_cf64(rflu_handle_t handle, int64_t n, int64_t nrhs, const double* F_host, int64_t lda, const int64_t* ipiv_host,
                    double* B_host, int64_t ldb);
int rflu_getrs_cf32(rflu_handle_t handle, int64_t n, int64_t nrhs, const float* F_host, int64_t lda, const int64_t* ipiv_host,
                    float* B_host, int64_t ldb);
int rflu_getrs_cf64_dev(rflu_handle_t handle, int64_t n, int64_t nrhs, const double* F_dev, int64_t lda, const int64_t* ipiv_dev,
                        double* B_dev, int64_t ldb);
int rflu_getrs_cf32_dev(rflu_handle_t handle, int64_t n, int64_t nrhs, const float* F_dev, int64_t lda, const int64_t* ipiv_dev,
                        float* B_dev, int64_t ldb);
int rflu_getrs_trans_cf64(rflu_handle_t handle, int64_t n, int64_t nrhs, const double* F_host, int64_t lda, const int64_t* ipiv_host,
                          double* B_host, int64_t ldb, int conj);
int rflu_getrs_trans_cf32(rflu_handle_t handle, int64_t n, int64_t nrhs, const float* F_host, int64_t lda, const int64_t* ipiv_host,
                          float* B_host, int64_t ldb, int conj);
int rflu_getrs_trans_cf64_dev(rflu_handle_t handle, int64_t n, int64_t nrhs, const double* F_dev, int64_t lda, const int64_t* ipiv_dev,
                              double* B_dev, int64_t ldb, int conj);
int rflu_getrs_trans_cf32_dev(rflu_handle_t handle, int64_t n, int64_t nrhs, const float* F_dev, int64_t lda, const int64_t* ipiv_dev,
                              float* B_dev, int64_t ldb, int conj);
/* COMPLEX INVERSE, DETERMINANT: inv! / inv, det, logabsdet, logdet on a ComplexF64 / ComplexF32 LU (csrc/inverse.hip, DESIGN.md
 * section 4.8).  Storage as in the other complex entries: double* / float* to interleaved (re, im) pairs; lda / ld / strideF count
 * COMPLEX elements; a pointer aligned to the real type is enough.  The contract is that of rflu_getri_* and rflu_logabsdet_* in the
 * INVERSE, DETERMINANT block above, word for word: ipiv NULL = NotIPIV; in-order launches on the handle's stream, no kernel waits for
 * another workgroup, no value is formed by read-modify-write on shared words, so results are bit-identical from run to run; n == 0
 * succeeds with nothing launched; negative sizes, lda < n and NULL pointers give RFLU_ERR_ARG with a message; work is complete on return.
 * There is no row-major entry: the single-matrix complex path is column-major only.
 *   - rflu_getri_c*: F (packed L\U exactly as rflu_getrf_c* left it) is overwritten by A^-1.  *info (host, required): 0, or the 1-based
 *     index of the first u_ii with BOTH parts zero -- then F is left UNTOUCHED and the return value is still RFLU_OK.  The sweeps of
 *     DESIGN.md section 4.4 IN PLACE on F read as a row-major array with ld = lda, which is transpose(F) -- the plain transpose, nothing
 *     is ever conjugated.  About 4n^3/3 complex multiply-adds through the complex MFMA GEMM against 2n^3 for rflu_getrs_c* on an explicit
 *     identity; workspace owned by the handle: one buffer of 512 x n complex elements and 2 * ceil(n/64) * 4096 for the 64x64 diagonal
 *     inverses, nothing of size n x n.  Any lda >= n; where the pointer is no multiple of 16 bytes (_cf32: or lda is odd) the GEMM loads
 *     element by element, same arithmetic, same bits.  Entries of F beyond the n x n matrix are never written.  The host entry: H2D, the
 *     device entry, D2H (not at all when info != 0);
 *   - rflu_logabsdet_c*: *logabs_out = sum of log|u_ii| with |u| = hypot(re, im); (*sign_re_out, *sign_im_out) = det A / |det A| = the
 *     product of u_ii / |u_ii| times (-1)^#{k : ipiv[k] != k+1}, renormalised to modulus 1 once at the end.  All three are host
 *     pointers, required.  Float64 arithmetic for both element types, in the fixed order of rflu_logabsdet_*: chunks of 1024 entries,
 *     four per thread in index order, a fixed tree, chunk results in index order (sums for the logs, products for the phases).  A u_ii
 *     with both parts zero gives (-Inf, 0 + 0i), a NaN in either part gives NaN in all three, n == 0 gives (0, 1 + 0i).  The diagonal
 *     sits at F[i*(ld+1)]; the host entry copies the diagonal and ipiv only;
 *   - rflu_logabsdet_batched_c*: the same for every matrix of a batch (matrix b at F_dev + b*strideF complex elements, ipiv at ipiv_dev +
 *     b*stride_ipiv); logabs_dev: DEVICE array of `batch` doubles, sign_dev: DEVICE array of `batch` interleaved (re, im) pairs.  One
 *     launch, one workgroup per matrix, any n (only diagonals are read, so it serves both orientations of rflu_getrf_batched_c*'s
 *     factors); bit-identical to the single-matrix entry on the same factors.
 * The batched inverse is rflu_getri_batched_c*_dev in the BATCHED COMPLEX block below.  Not here: row-major complex factors of a
 * single matrix. */
int rflu_getri_cf64_dev(rflu_handle_t handle, int64_t n, double* F_dev, int64_t lda, const int64_t* ipiv_dev, int64_t* info);
int rflu_getri_cf32_dev(rflu_handle_t handle, int64_t n, float* F_dev, int64_t lda, const int64_t* ipiv_dev, int64_t* info);
int rflu_getri_cf64(rflu_handle_t handle, int64_t n, double* F_host, int64_t lda, const int64_t* ipiv_host, int64_t* info);
int rflu_getri_cf32(rflu_handle_t handle, int64_t n, float* F_host, int64_t lda, const int64_t* ipiv_host, int64_t* info);
int rflu_logabsdet_cf64_dev(rflu_handle_t handle, int64_t n, const double* F_dev, int64_t ld, const int64_t* ipiv_dev,
                            double* logabs_out, double* sign_re_out, double* sign_im_out);
int rflu_logabsdet_cf32_dev(rflu_handle_t handle, int64_t n, const float* F_dev, int64_t ld, const int64_t* ipiv_dev,
                            double* logabs_out, double* sign_re_out, double* sign_im_out);
int rflu_logabsdet_cf64(rflu_handle_t handle, int64_t n, const double* F_host, int64_t ld, const int64_t* ipiv_host,
                        double* logabs_out, double* sign_re_out, double* sign_im_out);
int rflu_logabsdet_cf32(rflu_handle_t handle, int64_t n, const float* F_host, int64_t ld, const int64_t* ipiv_host,
                        double* logabs_out, double* sign_re_out, double* sign_im_out);
int rflu_logabsdet_batched_cf64_dev(rflu_handle_t handle, int64_t batch, int64_t n, const double* F_dev, int64_t lda, int64_t strideF,
                                    const int64_t* ipiv_dev, int64_t stride_ipiv, double* logabs_dev, double* sign_dev);
int rflu_logabsdet_batched_cf32_dev(rflu_handle_t handle, int64_t batch, int64_t n, const float* F_dev, int64_t lda, int64_t strideF,
                                    const int64_t* ipiv_dev, int64_t stride_ipiv, double* logabs_dev, double* sign_dev);
/* BATCHED COMPLEX: `batch` independent small ComplexF64 / ComplexF32 systems in one call (csrc/batched_complex.hip, DESIGN.md section
 * 4.7).  Storage as in the other complex entries: double* / float* to interleaved (re, im) pairs; lda, ldb, strideA / strideF / strideB
 * count COMPLEX elements.  Everything else is the contract of the BATCHED entries above, word for word: strided matrices (matrix b at
 * A_dev + b*strideA complex elements), row_major = 0 / 1 with lda >= m / n, ipiv at ipiv_dev + b*stride_ipiv (1-based; NULL only with
 * pivot == 0; a non-NULL ipiv with pivot == 0 is filled with the identity), info_dev a required DEVICE array of `batch` entries,
 * B in the orientation of F; batch == 0, m == 0, n == 0 or nrhs == 0 succeed with nothing launched; negative sizes, too-small lda /
 * strides and NULL pointers give RFLU_ERR_ARG with a message; work goes on the handle's stream and is complete on return.
 *   - per matrix the semantics of the COMPLEX entries: pivot = the row of largest modulus hypot(re, im), strict '>' from 0, the lowest
 *     row on ties, a NaN modulus never wins; a pivot with BOTH parts zero sets info once (1-based) and the elimination carries on
 *     unscaled; inv(pivot) once per column and one multiply per row; pivot == 0 is NoPivot;
 *   - rflu_getrs_batched_c*: trans = 0: B <- U^-1 L^-1 P B; trans = 1 (LAPACK 'T'): B <- P^T L^-T U^-T B, solves transpose(A) x = b;
 *     trans = 2 (LAPACK 'C'): B <- P^T L^-H U^-H B, solves A' x = b.  The two differ for these element types; any other value is
 *     RFLU_ERR_ARG.  Any nrhs.  A singular matrix yields Inf/NaN in its own right-hand sides only;
 *   - ONE launch up to max(m, n) <= 128 (ComplexF32) and max(m, n) <= 64 (ComplexF64; 65 x 64 x 16 B of LDS per matrix): a group of
 *     64..256 threads per matrix, the matrix in LDS between its one load and its one store, no kernel waits for another workgroup;
 *     rflu_last_path reports RFLU_PATH_HIP_BATCHED;
 *   - above that limit a COLUMN-MAJOR batch is looped over the single-matrix complex device path (rflu_getrf_c*_dev, rflu_getrs_c*_dev /
 *     rflu_getrs_trans_c*_dev), each matrix's info written into info_dev: correct, NOT fast, no size cliff, and rflu_last_path reports
 *     what that path reports.  A ROW-MAJOR batch above the limit is RFLU_ERR_ARG with a message that says so: the single-matrix
 *     complex path is column-major only;
 *   - rflu_getri_batched_c*: Ainv_b <- inv(op(A_b)) from the factors, op by trans = 0 (A), 1 (transpose(A), LAPACK 'T') or 2 (A', LAPACK
 *     'C'); any other value is RFLU_ERR_ARG.  The contract is that of rflu_getri_batched_f64_dev: out of place (Ainv must not overlap F;
 *     F and ipiv are only read), Ainv in the ORIENTATION OF F with its own ldi >= n / strideI in complex elements, ipiv NULL = NotIPIV,
 *     info_dev (device, batch entries, required): 0 or the 1-based index of the first u_ii with BOTH parts zero (one zero part is not
 *     singular), whose output is then Inf/NaN in its own matrix only; batch == 0 or n == 0 succeed with nothing launched.  ONE launch
 *     up to n <= 64 (ComplexF64) / n <= 128 (ComplexF32): the factors in LDS once, the columns of P * I made in LDS and never read
 *     from HBM, one reciprocal per u_ii and then multiplies; since inv(transpose(A)) = transpose(inv(A)), the three values of trans
 *     share every flop and differ only in how the result is stored (and 'C' in the sign of the imaginary part), so the 'T' result IS
 *     the transposed 'N' result bit for bit.  Above the limit a COLUMN-MAJOR batch is looped: a device copy of F_b into Ainv_b, the
 *     single-matrix rflu_getri_c*_dev in place, a singular matrix's output filled with NaN, and for trans != 0 one layout change of the
 *     result through an n x n buffer of the handle -- correct, NOT fast; a ROW-MAJOR batch above the limit is RFLU_ERR_ARG (the
 *     single-matrix complex path is column-major only). */
int rflu_getri_batched_cf64_dev(rflu_handle_t handle, int64_t batch, int64_t n, const double* F_dev, int64_t lda, int64_t strideF,
                                int row_major, const int64_t* ipiv_dev, int64_t stride_ipiv, double* Ainv_dev, int64_t ldi,
                                int64_t strideI, int trans, int64_t* info_dev);
int rflu_getri_batched_cf32_dev(rflu_handle_t handle, int64_t batch, int64_t n, const float* F_dev, int64_t lda, int64_t strideF,
                                int row_major, const int64_t* ipiv_dev, int64_t stride_ipiv, float* Ainv_dev, int64_t ldi,
                                int64_t strideI, int trans, int64_t* info_dev);
int rflu_getrf_batched_cf64_dev(rflu_handle_t handle, int64_t batch, int64_t m, int64_t n, double* A_dev, int64_t lda, int64_t strideA,
                                int row_major, int64_t* ipiv_dev, int64_t stride_ipiv, int pivot, int64_t* info_dev);
int rflu_getrf_batched_cf32_dev(rflu_handle_t handle, int64_t batch, int64_t m, int64_t n, float* A_dev, int64_t lda, int64_t strideA,
                                int row_major, int64_t* ipiv_dev, int64_t stride_ipiv, int pivot, int64_t* info_dev);
int rflu_getrs_batched_cf64_dev(rflu_handle_t handle, int64_t batch, int64_t n, int64_t nrhs, const double* F_dev, int64_t lda,
                                int64_t strideF, int row_major, const int64_t* ipiv_dev, int64_t stride_ipiv, double* B_dev, int64_t ldb,
                                int64_t strideB, int trans);
int rflu_getrs_batched_cf32_dev(rflu_handle_t handle, int64_t batch, int64_t n, int64_t nrhs, const float* F_dev, int64_t lda,
                                int64_t strideF, int row_major, const int64_t* ipiv_dev, int64_t stride_ipiv, float* B_dev, int64_t ldb,
                                int64_t strideB, int trans);
/* building block: C <- C - A*B, all row-major complex: A is M x K (lda), B is K x N (ldb), C is M x N (ldc).  Four real MFMA products
 * per K step; 16-byte loads where the pointers (and, for _cf32, even lda / ldb) allow, element by element otherwise -- same arithmetic. */
int rflu_gemm_rm_cf64_dev(rflu_handle_t handle, int64_t M, int64_t N, int64_t K, const double* A_dev, int64_t lda,
                          const double* B_dev, int64_t ldb, double* C_dev, int64_t ldc);
int rflu_gemm_rm_cf32_dev(rflu_handle_t handle, int64_t M, int64_t N, int64_t K, const float* A_dev, int64_t lda,
                          const float* B_dev, int64_t ldb, float* C_dev, int64_t ldc);

/* ---- COMPLEX NORMS, CONDITION: the NORMS, CONDITION block above for ComplexF64 / ComplexF32 (LAPACK zlange / clange + zgecon / cgecon).
 * Kernels: csrc/condest.hip and cgecon_batched_kernel in csrc/batched_complex.hip; DESIGN.md section 4.12.  The contract is that
 * of the real block with the storage rules of the other complex entries: a matrix crosses as double* / float* at interleaved (re, im)
 * pairs, every lda / strideA / strideF counts COMPLEX elements, a pointer aligned to the real type is enough.  Argument lists are those
 * of the _f64 / _f32 entries of the same name.  There is NO rflu_gecon_rm_c*: the single-matrix complex path is column-major only.
 * rflu_lange_c* keeps row_major (it only reads); rflu_gecon_batched_c* keeps row_major (the complex batched factors exist in both
 * orientations).  Work goes on the handle's stream and is complete on return.
 *
 * rflu_lange_c*: |a| = hypot(re, im) in Float64 (ComplexF32 parts are converted first).  The sums are Float64 in the fixed order of the
 * real entries with "element" read as complex element: chunks of 1024 elements of a line, thread t owns elements 4t .. 4t+3 in index
 * order, the same wave tree, the four wave sums in order, the chunks in index order; groups of 256 lines for the sum across lines, the
 * groups in index order.  Results are bit-identical from run to run, whatever the alignment and lda, and between the single and batched
 * entries.  16-byte loads where the pointer allows (for _cf32 also the start of every line, i.e. an even lda), element loads otherwise:
 * the same additions either way.  Padding is never read.  A NaN in EITHER part of any element gives NaN -- also when the other part is
 * Inf (the parts are tested, not the modulus: C's hypot(Inf, NaN) is Inf); otherwise an Inf gives Inf; m == 0 or n == 0 gives 0.  The
 * batched entry is one workgroup per matrix up to max(m, n) <= 128 for both element types and runs the single entry's kernels per
 * matrix above that, with the same bits. */
int rflu_lange_cf64_dev(rflu_handle_t handle, int norm, int64_t m, int64_t n, const double* A_dev, int64_t lda, int row_major,
                        double* out);
int rflu_lange_cf32_dev(rflu_handle_t handle, int norm, int64_t m, int64_t n, const float* A_dev, int64_t lda, int row_major,
                        double* out);
int rflu_lange_batched_cf64_dev(rflu_handle_t handle, int norm, int64_t batch, int64_t m, int64_t n, const double* A_dev, int64_t lda,
                                int64_t strideA, int row_major, double* out_dev);
int rflu_lange_batched_cf32_dev(rflu_handle_t handle, int norm, int64_t batch, int64_t m, int64_t n, const float* A_dev, int64_t lda,
                                int64_t strideA, int row_major, double* out_dev);
/* rflu_gecon_c*: *rcond_out = 1 / (anorm * est), est an estimate of ||U^-1 L^-1|| = ||A^-1|| in the norm `norm`; no ipiv argument; F
 * (column-major packed L\U as rflu_getrf_c* left it) is ONLY READ; the host entry is H2D, then the device entry.
 *   - The method is LAPACK zlacn2 (at most 5 iterations) on M = U^-1 L^-1 with the real entry's two stated changes carried over: the
 *     all-ones start vector with first estimate sum|v_i| / n, and the closing vector x_i = (-1)^i (n - 1 + i) with the bound
 *     2 sum|v_i| / (3 n (n - 1)).  n = 1: the estimate is |v_0| of the first solve.
 *   - The pair of operators is M and M^H (the ADJOINT, not M^T).  For RFLU_NORM_INF the two swap roles (||M||_inf = ||M^H||_1).
 *   - After a solve with M the next iterate is the phase vector x_i = v_i / |v_i|: |v_i| is hypot in Float64, the two quotients are
 *     formed in Float64 and rounded to the element type; x_i = 1 + 0i where both parts of v_i are zero.
 *   - There is NO repeated-sign-vector test (zlacn2 has none).  The stops are: est <= est_old; |x_jlast| == |x_j| with j the FIRST index
 *     of the largest modulus; 5 iterations.  The result is the larger of the iteration's estimate and the closing vector's bound.
 *     At most 11 solves with one right-hand side, 8n^2 real flops each.
 *   - One layout change per call: the row-major image W of F is made once in the handle's workspace; every M x is the few-right-hand-side
 *     forward solve of rflu_mixed_solve_cf32_dev (here also for ComplexF64) on W, every M^H x the few-right-hand-side path of
 *     rflu_getrs_trans_c*_dev with conj = 1 on F in place, both with ipiv = NULL.  Between two solves: fixed-order vector kernels and one
 *     read of a few scalars by the host.  No kernel of this path waits for another workgroup.  Neither solve path states a size limit,
 *     so there is NO size limit on n here (beyond memory).
 *   - Special values, the first in this order deciding: n == 0: 1.  anorm NaN: NaN.  anorm == 0: 0.  A u_ii with BOTH parts zero: 0,
 *     before any solve is launched (u_ii = 0 + 1i is not singular).  A NaN in either part of any factor entry: NaN.  A non-finite vector
 *     out of a solve (no xLATRS scaling): 0.
 *   - anorm < 0, norm not 1 / 2, lda < n, NULL pointers: RFLU_ERR_ARG with a message.
 *   - A solve, an inverse or a factorization after rflu_gecon_c* on the same handle is bit-identical to one on a fresh handle.
 * rflu_gecon_batched_c*: the same for every matrix of a batch (matrix b at F_dev + b*strideF complex elements in either orientation;
 * anorm_dev, rcond_dev: DEVICE arrays of `batch` doubles).  n <= 64 (ComplexF64) / n <= 128 (ComplexF32): ONE launch, the factors in LDS
 * once, the whole estimator inside the kernel (the batched substitutions of rflu_getrs_batched_c*, trans = 0 and trans = 2, on one
 * right-hand side; they multiply by one reciprocal of u_kk per column where the single entry divides), every group of a workgroup
 * running the same number of rounds.  Larger n: a column-major batch is looped over the single entry -- correct, NOT fast; a row-major
 * one is RFLU_ERR_ARG (the single-matrix complex path is column-major only).  Special values per member as above, except that a
 * member's anorm < 0 gives NaN in its own output; one member's NaN or singularity touches its own output only.  batch == 0: success;
 * n == 0: every rcond is 1. */
int rflu_gecon_cf64_dev(rflu_handle_t handle, int norm, int64_t n, const double* F_dev, int64_t lda, double anorm, double* rcond_out);
int rflu_gecon_cf32_dev(rflu_handle_t handle, int norm, int64_t n, const float* F_dev, int64_t lda, double anorm, double* rcond_out);
int rflu_gecon_cf64(rflu_handle_t handle, int norm, int64_t n, const double* F_host, int64_t lda, double anorm, double* rcond_out);
int rflu_gecon_cf32(rflu_handle_t handle, int norm, int64_t n, const float* F_host, int64_t lda, double anorm, double* rcond_out);
int rflu_gecon_batched_cf64_dev(rflu_handle_t handle, int norm, int64_t batch, int64_t n, const double* F_dev, int64_t lda,
                                int64_t strideF, int row_major, const double* anorm_dev, double* rcond_dev);
int rflu_gecon_batched_cf32_dev(rflu_handle_t handle, int norm, int64_t batch, int64_t n, const float* F_dev, int64_t lda,
                                int64_t strideF, int row_major, const double* anorm_dev, double* rcond_dev);

/* ---- MIXED PRECISION: Float32 factors of a Float64 matrix, Float64 iterative refinement (LAPACK dsgesv's scheme) ----
 * The Float32 factorization is the faster one; refinement with Float64 residuals r = b - A x brings the solution to Float64 backward
 * error when A is not too ill-conditioned for its Float32 factors (kappa well below 1 / eps32), and says so when it does not.
 * Float32 factors of a Float64 matrix.  A (column-major, lda >= n) is only read.  F32_dev: caller-owned n x n ROW-MAJOR
 * (ldf >= n, the layout and rules of rflu_getrf_rm_f32_dev), receives L\U.  ipiv / pivot / blocksize / info as in
 * rflu_getrf_rm_f32_dev (info = first exactly-zero pivot OF THE FLOAT32 FACTORIZATION).  *anorm_out (host, required) = ||A||_inf,
 * bit-identical from run to run.  The Float32 image that is factored is the IEEE conversion of every entry of A: round to nearest, ties
 * to even; an entry beyond FLT_MAX + half an ulp becomes +-Inf, a NaN stays a NaN, and underflow is GRADUAL: an entry in the Float32
 * subnormal range becomes the nearest subnormal, nothing is flushed to zero (an entry of magnitude 2^-150 or less becomes a zero, and
 * as a pivot sets info).  The image, ||A||_inf and the factors do not depend on the alignment of A / F32 or on lda / ldf.  The complex
 * entry below converts both parts of every element in the same way. */
int rflu_mixed_getrf_f64_dev(rflu_handle_t handle, int64_t n, const double* A_dev, int64_t lda, float* F32_dev, int64_t ldf,
                             int64_t* ipiv_dev, int pivot, int64_t blocksize, double* anorm_out, int64_t* info);
/* X <- A^-1 B to Float64 backward error by iterative refinement.  A, B are only read; X (n x nrhs, ldx) is written.
 * Converged when for every column k  ||r_k||_inf <= ||x_k||_inf * anorm * eps64 * sqrt(n)  (a NaN or Inf anywhere is NOT convergence).
 * *iters (host, required): >= 0 = refinement steps taken, converged; < 0 = -(steps taken + 1), NOT converged within max_iter
 * (<= 0 means 30), X is then the last iterate and must not be used.  Return value is RFLU_OK in both cases: the library has no
 * Float64 fallback inside, the host glue decides.  n == 0 or nrhs == 0: success, *iters = 0, nothing launched.  The Float32 factors
 * are used as they lie (no n x n layout change per solve); the residual of up to RFLU_MIXED_GEMV_MAX_RHS right-hand sides streams A
 * once per 8 of them, more go through the Float64 GEMM.  Work goes on the handle's stream and is complete on return. */
int rflu_mixed_getrs_f64_dev(rflu_handle_t handle, int64_t n, int64_t nrhs, const double* A_dev, int64_t lda, const float* F32_dev,
                             int64_t ldf, const int64_t* ipiv_dev, double anorm, const double* B_dev, int64_t ldb, double* X_dev,
                             int64_t ldx, int max_iter, int* iters);
/* building block: R <- B - A X, all column-major Float64, A n x n (R must not overlap A, X or B).  Bit-identical from run to run. */
int rflu_residual_f64_dev(rflu_handle_t handle, int64_t n, int64_t nrhs, const double* A_dev, int64_t lda, const double* X_dev,
                          int64_t ldx, const double* B_dev, int64_t ldb, double* R_dev, int64_t ldr);

/* ---- COMPLEX MIXED PRECISION: ComplexF32 factors of a ComplexF64 matrix, ComplexF64 iterative refinement (LAPACK zcgesv's scheme;
 * csrc/mixed.hip) ----
 * A ComplexF64 factorization costs four times the real flops, so this is the element type where the Float32 rate matters most.  The
 * contracts are those of rflu_mixed_getrf_f64_dev / rflu_mixed_getrs_f64_dev / rflu_residual_f64_dev above, word for word, except:
 *   - storage and leading dimensions follow the other complex entries: double* / float* to interleaved (re, im) pairs, lda / ldf / ldb /
 *     ldx / ldr count COMPLEX elements, a pointer aligned to the real type is enough;
 *   - there is no blocksize; the pivot rule (largest modulus hypot(re, im), strict '>' from 0, lowest row on ties, a NaN modulus never
 *     wins) and the zero-pivot rule (BOTH parts zero sets info once, the elimination carries on) are those of rflu_getrf_cf32_dev, and
 *     info is that of the ComplexF32 factorization;
 *   - F32_dev: caller-owned n x n ROW-MAJOR ComplexF32 (ldf >= n), receives L\U as the complex recursion leaves it;
 *   - *anorm_out = ||A||_inf = the largest row sum of MODULI hypot(re, im) (LAPACK zlange('I')), summed in a fixed order in Float64;
 *     the norms of the convergence rule are largest moduli.
 * Carried over unchanged: A and B are only read; converged when for every column k ||r_k||_inf <= ||x_k||_inf * anorm * eps64 * sqrt(n),
 * tested so that a NaN or Inf is never convergence; *iters >= 0 = steps taken, converged, < 0 = -(steps + 1), not converged within
 * max_iter (<= 0 means 30); RFLU_OK in both cases, the library never falls back; an entry of A that overflows Float32 is no special case: it
 * becomes Inf in F32, where the elimination turns it into NaN (Inf - Inf, 0 * Inf) the solve ends as non-convergence, and where it is
 * taken as a pivot (multipliers 0, no NaN) convergence is still only reported when the rule, which then scales with ||A||_inf >= 1e38,
 * is met; n == 0 or nrhs == 0 succeed with nothing launched; the argument checks; the handle's buffers.  Results are
 * bit-identical from run to run and whatever the alignment of A / F32 and the values of lda / ldf.  The residual of up to
 * RFLU_MIXED_GEMV_MAX_RHS right-hand sides streams A once per 8 of them, more go through the ComplexF64 GEMM on the transposed views
 * (that crossover is the real path's value: a structural starting value here).  Every solve of the loop works on the row-major factors
 * as they lie: no n x n copy, no workspace of size n^2. */
int rflu_mixed_getrf_cf64_dev(rflu_handle_t handle, int64_t n, const double* A_dev, int64_t lda, float* F32_dev, int64_t ldf,
                              int64_t* ipiv_dev, int pivot, double* anorm_out, int64_t* info);
int rflu_mixed_getrs_cf64_dev(rflu_handle_t handle, int64_t n, int64_t nrhs, const double* A_dev, int64_t lda, const float* F32_dev,
                              int64_t ldf, const int64_t* ipiv_dev, double anorm, const double* B_dev, int64_t ldb, double* X_dev,
                              int64_t ldx, int max_iter, int* iters);
/* building block: R <- B - A X, all column-major ComplexF64, A n x n (R must not overlap A, X or B).  Bit-identical from run to run. */
int rflu_residual_cf64_dev(rflu_handle_t handle, int64_t n, int64_t nrhs, const double* A_dev, int64_t lda, const double* X_dev,
                           int64_t ldx, const double* B_dev, int64_t ldb, double* R_dev, int64_t ldr);
/* building block: B <- U^-1 L^-1 P B with F32_dev the ROW-MAJOR packed ComplexF32 factors (as rflu_mixed_getrf_cf64_dev leaves them)
 * and B column-major (ldb >= n); ipiv NULL = NotIPIV.  F32 is only read, in place.  Up to 8 right-hand sides are solved in B's own
 * columns, more go through a row-major image of B and the complex GEMM.  A zero u_ii gives Inf/NaN, no error status.  Argument checks
 * and empty problems as rflu_getrs_cf32_dev.  Bit-identical from run to run and whatever the alignment of F32 and ldf. */
int rflu_mixed_solve_cf32_dev(rflu_handle_t handle, int64_t n, int64_t nrhs, const float* F32_dev, int64_t ldf,
                              const int64_t* ipiv_dev, float* B_dev, int64_t ldb);

/* ---- REFINEMENT AND ERROR BOUNDS: LAPACK xGERFS with trans = 'N' (what gesvx runs behind getrf / getrs): iterative refinement of a
 * computed solution in the WORKING precision, the componentwise backward error berr and the forward error bound ferr of every
 * right-hand side.  Float64 / Float32.  Kernels: csrc/refine.hip; driver: gerfs_dev in csrc/driver.cpp; DESIGN.md section 4.13.
 * rflu_gecon_* says how bad A can be for ANY right-hand side; berr and ferr say how good THIS X is for THIS B.
 *
 * rflu_gerfs_*: all matrices are column-major DEVICE memory.  A (n x n, lda) is the original matrix, F (ldf) and ipiv what
 * rflu_getrf_*_dev left (ipiv == NULL: NotIPIV), B (n x nrhs, ldb) the right-hand sides: A, F and B are ONLY READ.  X (n x nrhs, ldx)
 * holds a computed solution and is refined IN PLACE; X overlapping A, F or B is undefined.  ferr (may be NULL), berr (required) and
 * steps (may be NULL) are HOST arrays of nrhs entries; *info: host, required.
 *   - Per column k, with u the unit roundoff of the element type (2^-53 / 2^-24, LAPACK's eps):  r = b - A x,  w = |b| + |A| |x|,
 *     berr = max_i |r_i| / w_i.  While berr > u and 2 berr <= lstres (which starts at 3) and fewer than max_iter steps were taken
 *     (max_iter <= 0 means 5, LAPACK's ITMAX): solve A d = r with the factors, x += d, lstres = berr, recompute.  The last iterate
 *     stays even when it is the worse one, as in LAPACK.  steps[k] = the corrections applied to column k; berr[k] belongs to the X
 *     that is returned.
 *   - ferr[k] is LAPACK's bound: with wt_i = |r_i| + (n + 1) u w_i, ferr[k] = est(||A^-1 diag(wt)||_inf) / max_i |x_i| (no division
 *     when that maximum is 0).  est is the estimator of rflu_gecon_* on M = diag(wt) A^-T (||A^-1 diag(wt)||_inf = ||M||_1): M x is
 *     the transposed solve (P^T L^-T U^-T, with ipiv) followed by x o= wt, M^T x is x o= wt followed by the forward solve.  At most 11
 *     solves with one right-hand side per column, 2n^2 flops each: for many right-hand sides ferr is the expensive part.
 *     ferr == NULL skips the estimator entirely; berr, X and steps then come out bit for bit as with it.
 *   - FOUR DELIBERATE DIFFERENCES from LAPACK: (1) there are no safe1 / safe2 guards: a row with w_i == 0 (then r_i == 0 too)
 *     contributes 0 to berr, where LAPACK gives 1.  (2) r and w are accumulated in FLOAT64 FOR BOTH ELEMENT TYPES, one fused
 *     multiply-add per term, the columns of A in ascending order inside a column slice and the slices combined in slice order: a fixed
 *     order, no read-modify-write on shared words, the split a function of n alone.  The results are bit-identical from run to run and
 *     whatever the alignment of A and the values of lda / ldb / ldx.  The Float32 entry therefore refines with an extra-precise
 *     residual (its correction is the Float32 rounding of that residual), and its bound stays valid.  (3) The estimator's all-ones
 *     start vector and integer closing vector are those of rflu_gecon_* (see there).  (4) Up to 8 columns advance in lock step: one
 *     pass over A and one solve on an n x 8 block per step; a column that has stopped is solved again but NOT updated.  A column's
 *     results do not depend on its neighbours or on nrhs, bit for bit.
 *   - One layout change per call: the row-major image of F is made once in the handle's workspace; every correction runs on it and
 *     every transposed solve of the estimator on F in place.  No n x n copy per step or per right-hand side.  One host read of a few
 *     scalars per step.  Work goes on the handle's stream and is complete on return.
 *   - n == 0 or nrhs == 0: success, nothing launched, berr / ferr / steps of the nrhs columns are 0, *info = 0.  An exactly zero u_ii:
 *     *info = i (1-based), found before any solve as in rflu_getri_*; X, berr, ferr and steps are then untouched.  Otherwise *info = 0.
 *     A NaN in a column's r or w: berr[k] = NaN, no step for that column, ferr[k] = NaN; a NaN confined to one column of X or B touches
 *     that column's outputs only.  A non-finite vector inside the estimator while berr is no NaN: ferr[k] = +Inf.  A column with b = 0
 *     and x = 0: berr = ferr = 0.
 *   - RFLU_ERR_ARG with a message: negative n or nrhs, a leading dimension below max(n, 1), berr == NULL, info == NULL, NULL data
 *     pointers with n, nrhs > 0, n > 65536 when ferr is requested (the transposed chain's limit).
 *   - The handle's workspaces are shared with the other entries and refilled by each of them: a solve, an inverse, a factorization, a
 *     condition estimate or a mixed-precision solve after rflu_gerfs_* on the same handle is bit-identical to one on a fresh handle.
 * rflu_berr_*: the first half alone -- the Oettli-Prager componentwise backward error max_i |b - A x|_i / (|b| + |A| |x|)_i of ANY X,
 * by the same kernels and with the same rules (zero rows, NaN, empty problems, argument checks).  It needs no factors and writes
 * nothing on the device that the caller sees. */
int rflu_gerfs_f64_dev(rflu_handle_t handle, int64_t n, int64_t nrhs, const double* A_dev, int64_t lda, const double* F_dev,
                       int64_t ldf, const int64_t* ipiv_dev, const double* B_dev, int64_t ldb, double* X_dev, int64_t ldx,
                       double* ferr, double* berr, int max_iter, int* steps, int64_t* info);
int rflu_gerfs_f32_dev(rflu_handle_t handle, int64_t n, int64_t nrhs, const float* A_dev, int64_t lda, const float* F_dev,
                       int64_t ldf, const int64_t* ipiv_dev, const float* B_dev, int64_t ldb, float* X_dev, int64_t ldx,
                       double* ferr, double* berr, int max_iter, int* steps, int64_t* info);
int rflu_berr_f64_dev(rflu_handle_t handle, int64_t n, int64_t nrhs, const double* A_dev, int64_t lda, const double* X_dev,
                      int64_t ldx, const double* B_dev, int64_t ldb, double* berr);
int rflu_berr_f32_dev(rflu_handle_t handle, int64_t n, int64_t nrhs, const float* A_dev, int64_t lda, const float* X_dev,
                      int64_t ldx, const float* B_dev, int64_t ldb, double* berr);

/* ---- building blocks on the INTERNAL row-major layout: element (i,j) at R[i*ld + j] (device pointers).
 * These are the four kernels of the path plus the bookkeeping the multi-GPU block-column driver and the parity
 * tests need.  Pivot rows are GLOBAL 0-based row positions r0.. of the slab; ipiv entries are 1-based rows.
 * rflu_getrf_rm_*: factor the m x n row-major matrix in place (diagonal at (0,0)); ipiv_dev length min(m,n). */
int rflu_getrf_rm_f64_dev(rflu_handle_t handle, int64_t m, int64_t n, double* R_dev, int64_t ld, int64_t* ipiv_dev,
                          int pivot, int64_t blocksize, int64_t* info);
int rflu_getrf_rm_f32_dev(rflu_handle_t handle, int64_t m, int64_t n, float* R_dev, int64_t ld, int64_t* ipiv_dev,
                          int pivot, int64_t blocksize, int64_t* info);
/* Factor the tall panel rows [r0, m) x columns [c0, c0+w) whose diagonal block starts at (r0, c0); writes
 * ipiv_dev[r0 .. r0+w) (1-based global rows) and the row-interchange bookkeeping used by rflu_laswp_rm_*.
 * r0 must be a multiple of 64.  *info (host) gets 0 or r0 + k + 1 of the first zero pivot. */
int rflu_panel_rm_f64_dev(rflu_handle_t handle, int64_t m, int64_t r0, int64_t c0, int64_t w, double* R_dev,
                          int64_t ld, int64_t* ipiv_dev, int pivot, int64_t* info);
int rflu_panel_rm_f32_dev(rflu_handle_t handle, int64_t m, int64_t r0, int64_t c0, int64_t w, float* R_dev,
                          int64_t ld, int64_t* ipiv_dev, int pivot, int64_t* info);
/* apply_permutation!: apply the interchanges ipiv_dev[k0 .. k1) (row k <-> ipiv[k]-1, in order) to columns
 * [c0, c0+ncols) of R.  k0 must be a multiple of 64.  m = number of rows of R (bounds for the bookkeeping). */
int rflu_laswp_rm_f64_dev(rflu_handle_t handle, double* R_dev, int64_t ld, int64_t m, int64_t c0, int64_t ncols,
                          const int64_t* ipiv_dev, int64_t k0, int64_t k1);
int rflu_laswp_rm_f32_dev(rflu_handle_t handle, float* R_dev, int64_t ld, int64_t m, int64_t c0, int64_t ncols,
                          const int64_t* ipiv_dev, int64_t k0, int64_t k1);
/* B <- L^-1 B, L = unit lower triangle of the n x n block L_dev (row-major, ldl); B is n x nrhs (row-major, ldb). */
int rflu_trsm_rm_f64_dev(rflu_handle_t handle, int64_t n, int64_t nrhs, const double* L_dev, int64_t ldl,
                         double* B_dev, int64_t ldb);
int rflu_trsm_rm_f32_dev(rflu_handle_t handle, int64_t n, int64_t nrhs, const float* L_dev, int64_t ldl, float* B_dev,
                         int64_t ldb);
/* C <- C - A*B, all row-major: A is M x K (lda), B is K x N (ldb), C is M x N (ldc). */
int rflu_gemm_rm_f64_dev(rflu_handle_t handle, int64_t M, int64_t N, int64_t K, const double* A_dev, int64_t lda,
                         const double* B_dev, int64_t ldb, double* C_dev, int64_t ldc);
int rflu_gemm_rm_f32_dev(rflu_handle_t handle, int64_t M, int64_t N, int64_t K, const float* A_dev, int64_t lda,
                         const float* B_dev, int64_t ldb, float* C_dev, int64_t ldc);
/* Layout change: column-major (m x n, lda) <-> row-major (m x n, ldr). */
int rflu_cm_to_rm_f64_dev(rflu_handle_t handle, int64_t m, int64_t n, const double* A_cm, int64_t lda, double* R_rm,
                          int64_t ldr);
int rflu_rm_to_cm_f64_dev(rflu_handle_t handle, int64_t m, int64_t n, const double* R_rm, int64_t ldr, double* A_cm,
                          int64_t lda);
int rflu_cm_to_rm_f32_dev(rflu_handle_t handle, int64_t m, int64_t n, const float* A_cm, int64_t lda, float* R_rm,
                          int64_t ldr);
int rflu_rm_to_cm_f32_dev(rflu_handle_t handle, int64_t m, int64_t n, const float* R_rm, int64_t ldr, float* A_cm,
                          int64_t lda);

/* ---- randomized butterfly pre-transform (the reference's 🦋 solver, src/butterflylu.jl) ----
 * rflu_butterfly_mul_*: A <- U' A V in place (🦋mul!, src/butterflylu.jl:90-113), A column-major n x n on the device, n % 4
 * == 0 (pad! first, :180-197), uv = the 4n random diagonal entries in the reference's layout (:93-108).  One streaming
 * pass applies both butterfly levels.  After it a NoPivot factorization (rflu_getrf_*_dev with pivot = 0) is safe.
 * rflu_butterfly_vec_*: X <- U' X (transpose_u != 0) or X <- V X (transpose_u == 0) for nrhs column vectors -- the two
 * products around ldiv! in 🦋solve! (:50-52), applied as butterflies instead of dense matrices. */
int rflu_butterfly_mul_f64_dev(rflu_handle_t handle, int64_t n, double* A_dev, int64_t lda, const double* uv_dev);
int rflu_butterfly_mul_f32_dev(rflu_handle_t handle, int64_t n, float* A_dev, int64_t lda, const float* uv_dev);
int rflu_butterfly_vec_f64_dev(rflu_handle_t handle, int64_t n, int64_t nrhs, double* X_dev, int64_t ldx,
                               const double* uv_dev, int transpose_u);
int rflu_butterfly_vec_f32_dev(rflu_handle_t handle, int64_t n, int64_t nrhs, float* X_dev, int64_t ldx,
                               const float* uv_dev, int transpose_u);

/* ---- synthetic input on device (bench / tests; not part of the reference's surface) ----
 * Fill the m x n sub-block starting at global (i0, j0) of an M_global-row uniform[0,1) matrix:
 * element (i,j) = u01(seed, (j0+j)*M_global + (i0+i)) -- bit-identical to oracle/rflu_oracle.c:rfo_uniform01.
 * row_major = 0: A[i + j*ld]; row_major = 1: A[i*ld + j].  diag_add is added to global diagonal entries. */
int rflu_fill_uniform_f64_dev(rflu_handle_t handle, double* A_dev, int64_t m, int64_t n, int64_t ld, int row_major,
                              uint64_t seed, int64_t M_global, int64_t i0, int64_t j0, double diag_add);
int rflu_fill_uniform_f32_dev(rflu_handle_t handle, float* A_dev, int64_t m, int64_t n, int64_t ld, int row_major,
                              uint64_t seed, int64_t M_global, int64_t i0, int64_t j0, double diag_add);
/* ---- multi-GPU: 1-D block-column layout over the GPUs of one node, ONE process (BASELINE configs 3-4).
 * The reference has no distributed path; this is the partition the north star specifies.  Block column b (width `block`, a
 * multiple of 64) lives on logical device (b / run) % ndev inside that device's ROW-MAJOR slab (n rows x its local
 * columns, element (i, jl) at slab[i*ld + jl]); per block column the owner factors the panel with the single-GPU
 * recursion and ONE ncclBroadcast (RCCL, enqueued on the library's panel streams -- no host synchronisation per block
 * column) carries {L\U panel, pivot segment} to the other devices, which then apply laswp / TRSM / GEMM to their slabs;
 * one block column of lookahead.  devs[] may name ONE physical device several times ("fake multi-GPU"): the broadcast
 * then is a device-to-device copy, so the whole partition logic runs -- and is tested -- on a single GPU.
 * ipiv_host (length n, HOST memory, global 1-based rows) and *info as for rflu_getrf_*; ipiv_host may be NULL iff pivot == 0. */
typedef struct rflu_mgpu_s* rflu_mgpu_t;
int rflu_mgpu_create(rflu_mgpu_t* out, int ndev, const int* devs);
int rflu_mgpu_destroy(rflu_mgpu_t mgpu);
int rflu_mgpu_ndev(rflu_mgpu_t mgpu);
int rflu_mgpu_is_fake(rflu_mgpu_t mgpu);
/* number of ncclBroadcast calls this object has enqueued so far (0 in fake mode and with one device, unless
 * RFLU_MGPU_FORCE_RCCL=1 made a one-device object build a one-rank communicator and broadcast to itself: the way the
 * collective's code path is executed on a box with a single GPU) */
int64_t rflu_mgpu_collectives(rflu_mgpu_t mgpu);
/* The RFLU_* tuning variables are read ONCE per handle (rflu_create / rflu_mgpu_create).  A host that changes them between
 * calls asks for another read: rflu_reload_tuning for a single-GPU handle, this one for the per-device handles of a multi-GPU
 * object. */
int rflu_mgpu_reload_tuning(rflu_mgpu_t mgpu);
/* number of local columns of logical device d for an n-column matrix (-1 on bad arguments) */
int64_t rflu_mgpu_local_cols(int64_t n, int64_t block, int ndev, int64_t run, int d);
int rflu_getrf_f64_mgpu(rflu_mgpu_t mgpu, int64_t n, double* const* slabs_dev, const int64_t* lds, int64_t* ipiv_host,
                        int pivot, int64_t block, int64_t run, int64_t* info);
int rflu_getrf_f32_mgpu(rflu_mgpu_t mgpu, int64_t n, float* const* slabs_dev, const int64_t* lds, int64_t* ipiv_host,
                        int pivot, int64_t block, int64_t run, int64_t* info);
/* synthetic input (bench / tests): every slab receives its block columns of the n x n uniform[0,1) matrix of
 * rflu_fill_uniform_* (same seed -> the same matrix as on one GPU) */
int rflu_mgpu_fill_uniform_f64(rflu_mgpu_t mgpu, int64_t n, double* const* slabs_dev, const int64_t* lds, int64_t block,
                               int64_t run, uint64_t seed, double diag_add);
int rflu_mgpu_fill_uniform_f32(rflu_mgpu_t mgpu, int64_t n, float* const* slabs_dev, const int64_t* lds, int64_t block,
                               int64_t run, uint64_t seed, double diag_add);

/* ---- built-in per-kernel timers (hipEvents on the launch stream around every launch of a class) ----
 * enable = 1: synchronous mode -- every launch is bracketed and waited for; the factorization then runs the one-stream
 *             blocked schedule (each kernel alone on the GPU: the kernel's own roofline);
 * enable = 2: in-schedule mode -- event pairs are recorded on whatever stream a launch goes to and resolved when the
 *             timers are read; the default two-stream lookahead schedule is left untouched (what a kernel achieves next
 *             to the other stream's work);
 * enable = 3: the single-stream blocked schedule of mode 1 with the event pairs of mode 2: nothing is waited for between the
 *             launches, so the GPU does not go idle (and its power management does not lower the clock) behind every kernel --
 *             each kernel alone on the GPU at the clock of a busy GPU (bench.py's roofline pass);
 * enable = 0: off.  Enabling resets the timers.  rflu_profile_get returns accumulated milliseconds, launch count and the
 * algorithmic work (flops for GEMM/TRSM/PANEL, bytes for LASWP/TRANSPOSE) of class k since enabling. */
int rflu_profile_enable(rflu_handle_t handle, int enable);
int rflu_profile_get(rflu_handle_t handle, int kclass, double* ms, int64_t* launches, double* work);
/* algorithmic (minimum) HBM bytes of the launches of class k since enabling (GEMM: A and B once, C in and out) */
int rflu_profile_get_bytes(rflu_handle_t handle, int kclass, double* bytes);

#ifdef __cplusplus
}
#endif
#endif /* RFLU_H */
