// driver.cpp -- host side of librflu.so: the handle and its environment, buffers, the solve / batched / inverse / mixed-precision drivers, the
// profile entries and the C ABI of include/rflu.h.  The factorization schedules are in schedule.cpp, their streams in streams.cpp, the
// multi-GPU path in mgpu.cpp and the host-pointer entries in host_entry.cpp (driver.hpp: what they share).
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <new>

#include "complex.hpp"
#include "driver.hpp"

namespace rflu {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

static int64_t round_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }

// ---- the environment, read in ONE place (Tune::load_env / load_handle_env: at rflu_create and on rflu_reload_tuning) -----------
const char* env_str(const char* name) { return getenv(name); }
static void env_get(const char* name, int& v) { if (const char* e = env_str(name)) v = atoi(e); }
static void env_get(const char* name, int64_t& v) { if (const char* e = env_str(name)) v = atoll(e); }
static void env_get(const char* name, double& v) { if (const char* e = env_str(name)) v = atof(e); }
static void env_flag(const char* name, int& v) { if (env_str(name)) v = 1; }   // set = on, whatever the value

void Tune::load_env()
{
    *this = Tune();
    // ---- the shipped library's surface: schedule selection, the knobs the tests and the measurement scripts
    // switch, tracing.  Everything below the #ifdef is tuning that was measured once and settled: read by the
    // experiments build only (RFLU_EXPERIMENTS=1 at BUILD time -> librflu_exp.so), compiled-in defaults otherwise.
    env_get("RFLU_PANEL_LOCAL_ROWS", panel_local_rows);
    env_get("RFLU_GEMM_MASKED", gemm_masked);
    env_get("RFLU_TRSV_MAX_RHS", trsv_max_rhs);
    env_get("RFLU_TRSM_CHAIN_MAX_RHS", trsm_chain_max_rhs);
    env_get("RFLU_MIXED_GEMV_MAX_RHS", mixed_gemv_max_rhs);
    env_get("RFLU_QUEUE_CHECK", queue_check);
    env_flag("RFLU_QUEUE_TRACE", queue_trace);
    env_flag("RFLU_SPLIT_ALL", split_all);
    env_get("RFLU_SPLIT_SCALE", split_scale);
    env_get("RFLU_LEAFWISE", leafwise);
    env_get("RFLU_LEAFWISE_ROWS", leafwise_rows);
    env_flag("RFLU_GATE_TRACE", gate_trace);
    if (const char* e = env_str("RFLU_SCHEDULE")) schedule_events = strcmp(e, "events") == 0;
    // rocprofv3 --pmc exports this into the profiled process and runs one kernel at a time: a device-side gate would only ever
    // see its timeout, so a counter-collection run takes the event schedule by itself (RFLU_SCHEDULE=gates overrides)
    else if (env_str("ROCPROF_COUNTER_COLLECTION")) schedule_events = 1;
    env_get("RFLU_LEAF_FUSE", leaf_fuse);
    env_get("RFLU_HOST_EARLY_OUT", host_early_out);
    env_flag("RFLU_HOST_TRACE", host_trace);
    env_get("RFLU_HOST_THREADS", host_threads);
    env_get("RFLU_MGPU_BIG_RESERVE", mgpu_big_reserve);
    env_get("RFLU_DEBUG_GHOST_LEAF", debug_ghost_leaf);
    env_get("RFLU_ENGINE", engine);
    env_get("RFLU_ENGINE_ROWS", engine_rows);
    env_get("RFLU_ENGINE_HOST", engine_host);
    env_get("RFLU_ENGINE_REPLAY", engine_replay);
    env_get("RFLU_ENGINE_RETIRE", engine_retire);
    env_get("RFLU_ENGINE_AHEAD", engine_ahead);
#ifdef RFLU_EXPERIMENTS
    env_get("RFLU_PANEL_PW", panel_pw);
    env_get("RFLU_PANEL_MAXG", panel_maxg);
    env_get("RFLU_PANEL_RPW", panel_rpw);
    if (panel_rpw != 64 && panel_rpw != 128 && panel_rpw != 256 && panel_rpw != 384 && panel_rpw != 512) panel_rpw = 0;   // the kernels that exist
    env_get("RFLU_PANEL_SPARE", panel_spare);
    env_get("RFLU_PANEL_SPARE_MIN", panel_spare_min);
    env_get("RFLU_PANEL_BALLAST", panel_ballast);
    env_get("RFLU_PANEL_LOCAL_MIN", panel_local_min);
    env_get("RFLU_PANEL_LOCAL_PW8_ROWS", panel_local_pw8_rows);
    env_get("RFLU_POLL_DELAY", poll_delay);
    env_get("RFLU_POLL_ADAPT", poll_adapt);
    env_get("RFLU_LASWP_LPR", laswp_lpr);
    env_get("RFLU_GEMM_FLAGS", gemm_flags);
    env_get("RFLU_SKINNY_MAXK", skinny_max_k);
    env_get("RFLU_SKINNY_WIDE", skinny_wide);
    env_get("RFLU_GEMM_CFIRST_BELOW", gemm_cfirst_below);
    env_get("RFLU_LD_PAD", ld_pad);
    ld_pad = (ld_pad / 16) * 16;
    env_get("RFLU_TRSM_CHAIN_SPLIT", trsm_chain_split);
    env_get("RFLU_TRSM_CHAIN_CACHED", trsm_chain_cached);
    env_get("RFLU_SPLIT_SHARE", split_share);
    env_get("RFLU_MAX_RESERVE", max_reserve);
    env_get("RFLU_WIDE_NARROW", wide_narrow);
    env_get("RFLU_NARROW_COLS", narrow_cols);
    env_get("RFLU_RESERVE_CUS", min_reserve);
    env_get("RFLU_CONFINE_ROWS", confine_rows);
    env_get("RFLU_MERGE_ROWS", merge_rows);
    env_get("RFLU_SWAP_SU", swap_su);
    env_get("RFLU_SWAP_LATE", swap_late);
    env_get("RFLU_SWAP_ROWS", swap_rows);
    env_get("RFLU_GATE_FOLD", gate_fold);
    env_flag("RFLU_TIME_ENQUEUE", time_enqueue);
    env_get("RFLU_TAIL_OVERLAP", tail_overlap);
    env_get("RFLU_MGPU_TALL_ROWS", mgpu_tall_rows);
    env_get("RFLU_MGPU_SYNC", mgpu_sync);
    env_get("RFLU_ENGINE_POLICY", engine_policy);
    env_get("RFLU_ENGINE_WGS", engine_wgs);
    env_get("RFLU_ENGINE_WC", engine_wc);
    env_get("RFLU_ENGINE_WRITE_THROUGH", engine_write_through);
    env_get("RFLU_ENGINE_LEAF_XCDS", engine_leaf_xcds);
    env_get("RFLU_ENGINE_LEAF_WGS", engine_leaf_wgs);
    env_get("RFLU_ENGINE_HOST_LAG", engine_host_lag);
    env_get("RFLU_ENGINE_SOLVE_RL", engine_solve_rl);
#endif
}

// the handle's own switches (kernel routing) + its Tune
void load_handle_env(Handle* h)
{
    h->tune.load_env();
    h->coop_launch = false;
    h->panel_local = 2;
    h->panel_single = 1;
    h->panel_blocked = 0;
    h->panel_local_maxg = 64;
    int v = 0;
    env_get("RFLU_COOP_LAUNCH", v);
    h->coop_launch = v != 0;
    env_get("RFLU_PANEL_LOCAL", h->panel_local);
    env_get("RFLU_PANEL_SINGLE", h->panel_single);
    env_get("RFLU_PANEL_BLOCKED", h->panel_blocked);
    if (h->panel_local == 1) h->panel_local_maxg = 32;   // one XCD has 32 CUs
#ifdef RFLU_EXPERIMENTS
    env_get("RFLU_PANEL_LOCAL_MAXG", h->panel_local_maxg);
#endif
}

// Leading dimension of the row-major workspace for n columns: a multiple of 16 elements (rows start on 128-byte lines).
// RFLU_LD_PAD=<elements> adds a padding when that is a multiple of 512 elements (a power-of-two row pitch): measured on MI355X
// (round 3, N=16384: 82.7 ms / laswp 3.11 TB/s without, 82.3-82.9 ms / 3.0-3.17 TB/s with 16..272 elements) it changes nothing --
// the HBM address hash already spreads equal columns of consecutive rows over the channels -- so the default is none.
int64_t workspace_ld(const Handle* h, int64_t n)
{
    const int64_t pad = h->tune.ld_pad;
    int64_t ld = round_up(std::max<int64_t>(n, 1), 16);
    if (pad > 0 && ld % 512 == 0) ld += pad;
    return ld;
}

int ensure_buffer(void** ptr, size_t* cap, size_t need)
{
    if (*cap >= need) return RFLU_OK;
    if (*ptr) RFLU_HIP(hipFree(*ptr));
    *ptr = nullptr;
    *cap = 0;
    RFLU_HIP(hipMalloc(ptr, need));
    *cap = need;
    return RFLU_OK;
}

int ensure_bookkeeping(Handle* h, int64_t rows)
{
    const int64_t chunks = (rows + NB - 1) / NB + 1;
    if (chunks <= h->pm_chunks) return RFLU_OK;
    if (h->pm_cnt) RFLU_HIP(hipFree(h->pm_cnt));
    if (h->pm_dst) RFLU_HIP(hipFree(h->pm_dst));
    if (h->pm_src) RFLU_HIP(hipFree(h->pm_src));
    if (h->linv) RFLU_HIP(hipFree(h->linv));
    h->linv = nullptr;
    h->pm_cnt = h->pm_dst = h->pm_src = nullptr;
    h->pm_chunks = 0;
    RFLU_HIP(hipMalloc((void**)&h->pm_cnt, (size_t)chunks * sizeof(int)));
    RFLU_HIP(hipMalloc((void**)&h->pm_dst, (size_t)chunks * 2 * NB * sizeof(int)));
    RFLU_HIP(hipMalloc((void**)&h->pm_src, (size_t)chunks * 2 * NB * sizeof(int)));
    RFLU_HIP(hipMalloc(&h->linv, (size_t)chunks * NB * NB * sizeof(double)));
    RFLU_HIP(hipMemset(h->pm_cnt, 0, (size_t)chunks * sizeof(int)));
    h->pm_chunks = chunks;
    return RFLU_OK;
}

// ---- B <- L^-1 B by recursive splitting on 64-row boundaries (off-diagonal work = MFMA GEMM) -----------------------
// linv: inverses of L's 64x64 diagonal blocks (one 64x64 dense block per 64 rows), or nullptr.  With them, triangles of
// up to 256 rows are solved by ONE fused strip kernel instead of 7 dependent launches.
constexpr int64_t TRSM_FUSED_MAX = 256;

template <typename T>
int trsm_rec(Handle* h, int64_t n, int64_t nrhs, const T* L, int64_t ldl, T* B, int64_t ldb, const T* linv)
{
    if (n <= 0 || nrhs <= 0) return RFLU_OK;
    if (linv && n <= TRSM_FUSED_MAX) return launch_trsm_fused<T>(h, n, nrhs, L, ldl, linv, B, ldb);
    if (n <= NB) return launch_trsm_base<T>(h, n, nrhs, L, ldl, B, ldb);
    const int64_t leaves = (n + NB - 1) / NB;
    const int64_t n1 = ((leaves + 1) / 2) * NB;
    RFLU_TRY(trsm_rec<T>(h, n1, nrhs, L, ldl, B, ldb, linv));
    RFLU_TRY(launch_gemm<T>(h, n - n1, nrhs, n1, L + n1 * ldl, ldl, B, ldb, B + n1 * ldb, ldb));
    return trsm_rec<T>(h, n - n1, nrhs, L + n1 * ldl + n1, ldl, B + n1 * ldb, ldb,
                       linv ? linv + (n1 / NB) * NB * NB : nullptr);
}

// stand-alone TRSM (C ABI building block): invert the diagonal blocks first, then the fused path
template <typename T>
int trsm_public(Handle* h, int64_t n, int64_t nrhs, const T* L, int64_t ldl, T* B, int64_t ldb)
{
    if (n <= 0 || nrhs <= 0) return RFLU_OK;
    const size_t need = (size_t)((n + NB - 1) / NB) * NB * NB * sizeof(T);
    RFLU_TRY(ensure_buffer(&h->linv_tmp, &h->linv_tmp_bytes, need));
    h->trsv_area = nullptr;  // the cooperative solve's exchange area shares this buffer: have it wiped before its next use
    T* li = static_cast<T*>(h->linv_tmp);
    RFLU_TRY(launch_diag_inv<T>(h, n, L, ldl, li));
    return trsm_rec<T>(h, n, nrhs, L, ldl, B, ldb, li);
}

// ---- B <- U^-1 B (upper, non-unit) by recursive splitting on 64-row boundaries: bottom block, GEMM, top block ------
template <typename T>
static int triu_solve_rec(Handle* h, int64_t n, int64_t nrhs, const T* U, int64_t ldu, T* B, int64_t ldb)
{
    if (n <= 0 || nrhs <= 0) return RFLU_OK;
    if (n <= NB) return launch_triu_base<T>(h, n, nrhs, U, ldu, B, ldb);
    const int64_t leaves = (n + NB - 1) / NB;
    const int64_t n1 = ((leaves + 1) / 2) * NB;  // rows of the top block; the (possibly partial) rest is the bottom
    RFLU_TRY(triu_solve_rec<T>(h, n - n1, nrhs, U + n1 * ldu + n1, ldu, B + n1 * ldb, ldb));
    RFLU_TRY(launch_gemm<T>(h, n1, nrhs, n - n1, U + n1, ldu, B + n1 * ldb, ldb, B, ldb));
    return triu_solve_rec<T>(h, n1, nrhs, U, ldu, B, ldb);
}

// ldiv!(F::LU, B): B <- U^-1 L^-1 P B on row-major device data (F as left by getrf_rm; B is n x nrhs, row-major).
template <typename T>
static int getrs_rm(Handle* h, int64_t n, int64_t nrhs, const T* R, int64_t ld, const int64_t* ipiv, T* B, int64_t ldb)
{
    if (n <= 0 || nrhs <= 0) return RFLU_OK;
    RFLU_TRY(ensure_bookkeeping(h, n));
    if (ipiv) {  // rows of B follow the factorization's interchanges (NULL = NotIPIV: nothing to apply)
        RFLU_TRY(launch_perm_build(h, ipiv, 0, n, n));
        RFLU_TRY(launch_laswp<T>(h, B, ldb, 0, nrhs, 0, (n + NB - 1) / NB));
    }
    // few right-hand sides (<= 32: measured crossover): one cooperative launch per triangle and pass of 8 (trsv.hip)
    // instead of ~n/32 dependent launches; many:
    // the recursive splitting, whose GEMMs then carry the work.  RFLU_TRSV_MAX_RHS moves the crossover (0 = never).
    const int64_t trsv_max = h->tune.trsv_max_rhs;
    // a block of right-hand sides (33 .. trsm_chain_max_rhs): the same cooperative chain in passes of 64 columns on the MFMA units
    // (trsv.hip: trsm_chain_kernel; n = 16384, 64 right-hand sides: 28.8 ms with the recursive splitting below)
    const bool wide = nrhs > trsv_max && nrhs <= h->tune.trsm_chain_max_rhs;
    if ((nrhs <= trsv_max || wide) && n <= (int64_t)NB * 256 * 4) {
        RFLU_HIP(hipMemsetAsync(h->info_dev, 0, 2 * sizeof(int64_t), h->stream));
        RFLU_TRY(launch_trsv_coop<T>(h, n, nrhs, R, ld, B, ldb, wide));
        RFLU_HIP(hipMemcpyAsync(h->info_pinned, h->info_dev, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
        RFLU_HIP(hipStreamSynchronize(h->stream));
        if (h->info_pinned[1] != 0) {
            set_error("cooperative solve kernel timed out waiting for a peer workgroup");
            return RFLU_ERR_TIMEOUT;
        }
        return RFLU_OK;
    }
    RFLU_TRY(trsm_public<T>(h, n, nrhs, R, ld, B, ldb));
    return triu_solve_rec<T>(h, n, nrhs, R, ld, B, ldb);
}

// column-major device entry: F (n x n, lda) and B (n x nrhs, ldb) as LinearAlgebra.LU / LAPACK getrs hold them
template <typename T>
int getrs_cm_dev(Handle* h, int64_t n, int64_t nrhs, const T* F, int64_t lda, const int64_t* ipiv, T* B,
                        int64_t ldb)
{
    if (n < 0 || nrhs < 0 || lda < std::max<int64_t>(n, 1) || ldb < std::max<int64_t>(n, 1)) {
        set_error("getrs: bad arguments n=%lld nrhs=%lld lda=%lld ldb=%lld", (long long)n, (long long)nrhs,
                  (long long)lda, (long long)ldb);
        return RFLU_ERR_ARG;
    }
    if (n == 0 || nrhs == 0) return RFLU_OK;
    const int64_t ldr = workspace_ld(h, n), ldx = round_up(nrhs, 16);
    RFLU_TRY(ensure_buffer(&h->work, &h->work_bytes, (size_t)n * (size_t)ldr * sizeof(T)));
    RFLU_TRY(ensure_buffer(&h->rhs_work, &h->rhs_work_bytes, (size_t)n * (size_t)ldx * sizeof(T)));
    T* R = static_cast<T*>(h->work);
    T* X = static_cast<T*>(h->rhs_work);
    RFLU_TRY(launch_transpose<T>(h, n, n, F, lda, R, ldr));
    RFLU_TRY(launch_transpose<T>(h, n, nrhs, B, ldb, X, ldx));
    RFLU_TRY(getrs_rm<T>(h, n, nrhs, R, ldr, ipiv, X, ldx));
    RFLU_TRY(launch_transpose<T>(h, nrhs, n, X, ldx, B, ldb));
    RFLU_HIP(hipStreamSynchronize(h->stream));
    return RFLU_OK;
}

// ---- ldiv!(F', B): B <- P^T L^-T U^-T B, LAPACK getrs with trans = 'T' (real types: adjoint == transpose) ----------------------------
// V is the row-major image of F^T, B the row-major n x nrhs block.  The cooperative chain only (trsv.hip): passes of 8 columns up to
// trsv_max_rhs right-hand sides, passes of 64 on the MFMA units beyond, for any nrhs -- there is no recursive form of this solve.
template <typename T>
static int getrs_trans_view(Handle* h, int64_t n, int64_t nrhs, const T* V, int64_t ldv, const int64_t* ipiv, T* B, int64_t ldb)
{
    if (n <= 0 || nrhs <= 0) return RFLU_OK;
    if (n > (int64_t)NB * 256 * 4) {
        set_error("getrs_trans: n = %lld exceeds the %d rows the cooperative solve covers", (long long)n, NB * 256 * 4);
        return RFLU_ERR_ARG;
    }
    RFLU_TRY(ensure_bookkeeping(h, n));
    RFLU_HIP(hipMemsetAsync(h->info_dev, 0, 2 * sizeof(int64_t), h->stream));
    RFLU_TRY(launch_trsv_coop<T>(h, n, nrhs, V, ldv, B, ldb, nrhs > h->tune.trsv_max_rhs, true));
    if (ipiv) {  // the factorization's interchanges, undone last to first (NULL = NotIPIV: nothing to apply)
        RFLU_TRY(launch_perm_build(h, ipiv, 0, n, n));
        RFLU_TRY(launch_laswp_rev<T>(h, B, ldb, nrhs, 0, (n + NB - 1) / NB));
    }
    RFLU_HIP(hipMemcpyAsync(h->info_pinned, h->info_dev, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    RFLU_HIP(hipStreamSynchronize(h->stream));
    if (h->info_pinned[1] != 0) {
        set_error("cooperative solve kernel timed out waiting for a peer workgroup");
        return RFLU_ERR_TIMEOUT;
    }
    return RFLU_OK;
}

// column-major device entry.  A column-major F read as a row-major array with ld = lda IS F^T: the factors are read in place, whatever
// lda and the pointer's alignment (the chain kernels fall back to element loads where a 16-byte load would be misaligned); only the
// right-hand sides change layout.
template <typename T>
int getrs_trans_cm_dev(Handle* h, int64_t n, int64_t nrhs, const T* F, int64_t lda, const int64_t* ipiv, T* B,
                              int64_t ldb)
{
    if (n < 0 || nrhs < 0 || lda < std::max<int64_t>(n, 1) || ldb < std::max<int64_t>(n, 1)) {
        set_error("getrs_trans: bad arguments n=%lld nrhs=%lld lda=%lld ldb=%lld", (long long)n, (long long)nrhs,
                  (long long)lda, (long long)ldb);
        return RFLU_ERR_ARG;
    }
    if (n == 0 || nrhs == 0) return RFLU_OK;
    const int64_t ldx = round_up(nrhs, 16);
    RFLU_TRY(ensure_buffer(&h->rhs_work, &h->rhs_work_bytes, (size_t)n * (size_t)ldx * sizeof(T)));
    T* X = static_cast<T*>(h->rhs_work);
    RFLU_TRY(launch_transpose<T>(h, n, nrhs, B, ldb, X, ldx));
    RFLU_TRY(getrs_trans_view<T>(h, n, nrhs, F, lda, ipiv, X, ldx));
    RFLU_TRY(launch_transpose<T>(h, nrhs, n, X, ldx, B, ldb));
    RFLU_HIP(hipStreamSynchronize(h->stream));
    return RFLU_OK;
}

// row-major factors (getrf_rm): here the transposed view is not free -- one layout change of R into the handle's workspace, then the
// same path
template <typename T>
static int getrs_trans_rm(Handle* h, int64_t n, int64_t nrhs, const T* R, int64_t ld, const int64_t* ipiv, T* B, int64_t ldb)
{
    if (n < 0 || nrhs < 0 || ld < std::max<int64_t>(n, 1) || ldb < std::max<int64_t>(nrhs, 1)) {
        set_error("getrs_trans_rm: bad arguments n=%lld nrhs=%lld ld=%lld ldb=%lld", (long long)n, (long long)nrhs,
                  (long long)ld, (long long)ldb);
        return RFLU_ERR_ARG;
    }
    if (n == 0 || nrhs == 0) return RFLU_OK;
    const int64_t ldv = workspace_ld(h, n);
    RFLU_TRY(ensure_buffer(&h->work, &h->work_bytes, (size_t)n * (size_t)ldv * sizeof(T)));
    T* V = static_cast<T*>(h->work);
    RFLU_TRY(launch_transpose<T>(h, n, n, R, ld, V, ldv));
    return getrs_trans_view<T>(h, n, nrhs, V, ldv, ipiv, B, ldb);
}

// C-ABI GEMM.  RFLU_GEMM_MASKED=<reserve> (measurement only): run it on the CU-masked update stream of the lookahead
// schedule and wait for it, so that scripts/microbench_gemm_k.py can time the kernel on 256 - reserve CUs.
template <typename T>
static int gemm_public(Handle* h, int64_t M, int64_t N, int64_t K, const T* A, int64_t lda, const T* B, int64_t ldb, T* C,
                       int64_t ldc)
{
    if (h->tune.gemm_masked < 0) return launch_gemm<T>(h, M, N, K, A, lda, B, ldb, C, ldc);
    hipStream_t U;
    RFLU_TRY(get_ustream(h, h->tune.gemm_masked, &U));
    RFLU_HIP(hipStreamSynchronize(h->stream));
    {
        OnStream on(h, U);
        RFLU_TRY(launch_gemm<T>(h, M, N, K, A, lda, B, ldb, C, ldc));
    }
    RFLU_HIP(hipStreamSynchronize(U));
    return RFLU_OK;
}

// ---- batched entries (include/rflu.h): `batch` independent matrices, strided.  max(m, n) <= BATCHED_MAX_DIM: one launch of the
// batched kernels (batched.hip); larger: a loop over the single-matrix device path on the same stream -- correct, not fast, no size cliff.
// The argument rules are the same for real and complex elements (`who` = the entry's name in the error text; lda / ldb / strides in
// elements).  true: there is work to do; false: return *rc -- RFLU_ERR_ARG, or RFLU_OK for an empty batch, whose pointers nobody checks.
static bool check_batched_factor_args(const char* who, int64_t batch, int64_t m, int64_t n, const void* A, int64_t lda, int64_t strideA,
                                     int row_major, const int64_t* ipiv, int64_t stride_ipiv, int pivot, const int64_t* info_dev, int* rc)
{
    *rc = RFLU_ERR_ARG;
    if (batch < 0 || m < 0 || n < 0) {
        set_error("%s: negative size batch=%lld m=%lld n=%lld", who, (long long)batch, (long long)m, (long long)n);
        return false;
    }
    if (batch == 0 || m == 0 || n == 0) { *rc = RFLU_OK; return false; }
    const int64_t mn = std::min(m, n), rows = row_major ? n : m, cols = row_major ? m : n;   // rows = the contiguous dimension
    if (A == nullptr || info_dev == nullptr) { set_error("%s: null matrix or info pointer", who); return false; }
    if (pivot && ipiv == nullptr) { set_error("%s: pivot != 0 needs an ipiv buffer", who); return false; }
    if (lda < rows || (batch > 1 && strideA < (cols - 1) * lda + rows)) {
        set_error("%s: lda=%lld strideA=%lld too small for %lld x %lld (%s)", who, (long long)lda, (long long)strideA, (long long)m,
                  (long long)n, row_major ? "row-major" : "column-major");
        return false;
    }
    if (ipiv && batch > 1 && stride_ipiv < mn) { set_error("%s: stride_ipiv=%lld < min(m, n)", who, (long long)stride_ipiv); return false; }
    return true;
}

// trans3: trans has to be 0, 1 or 2 (the complex entries; the real ones read any non-zero value as "transposed")
static bool check_batched_solve_args(const char* who, int64_t batch, int64_t n, int64_t nrhs, const void* F, int64_t lda, int64_t strideF,
                                    int row_major, const int64_t* ipiv, int64_t stride_ipiv, const void* B, int64_t ldb, int64_t strideB,
                                    int trans, bool trans3, int* rc)
{
    *rc = RFLU_ERR_ARG;
    if (batch < 0 || n < 0 || nrhs < 0) {
        set_error("%s: negative size batch=%lld n=%lld nrhs=%lld", who, (long long)batch, (long long)n, (long long)nrhs);
        return false;
    }
    if (trans3 && (trans < 0 || trans > 2)) {
        set_error("%s: trans must be 0 (A), 1 (transpose) or 2 (adjoint), got %d", who, trans);
        return false;
    }
    if (batch == 0 || n == 0 || nrhs == 0) { *rc = RFLU_OK; return false; }
    if (F == nullptr || B == nullptr) { set_error("%s: null pointer", who); return false; }
    const int64_t brows = row_major ? nrhs : n, bcols = row_major ? n : nrhs;   // brows = the contiguous dimension of B
    if (lda < n || ldb < brows || (batch > 1 && (strideF < (n - 1) * lda + n || strideB < (bcols - 1) * ldb + brows))) {
        set_error("%s: lda=%lld strideF=%lld ldb=%lld strideB=%lld too small for n=%lld nrhs=%lld (%s)", who, (long long)lda,
                  (long long)strideF, (long long)ldb, (long long)strideB, (long long)n, (long long)nrhs, row_major ? "row-major" : "column-major");
        return false;
    }
    if (ipiv && batch > 1 && stride_ipiv < n) { set_error("%s: stride_ipiv=%lld < n", who, (long long)stride_ipiv); return false; }
    return true;
}

template <typename T>
static int getrf_batched(Handle* h, int64_t batch, int64_t m, int64_t n, T* A, int64_t lda, int64_t strideA, int row_major,
                         int64_t* ipiv, int64_t stride_ipiv, int pivot, int64_t* info_dev)
{
    int rc;
    if (!check_batched_factor_args("getrf_batched", batch, m, n, A, lda, strideA, row_major, ipiv, stride_ipiv, pivot, info_dev, &rc)) return rc;
    if (batched_fits(m, n)) {
        RFLU_TRY(launch_getrf_batched<T>(h, batch, m, n, A, lda, strideA, row_major, ipiv, stride_ipiv, pivot, info_dev));
        RFLU_HIP(hipStreamSynchronize(h->stream));
        h->last_path = RFLU_PATH_HIP_BATCHED;
        return RFLU_OK;
    }
    std::vector<int64_t> infos((size_t)batch, 0);
    for (int64_t b = 0; b < batch; ++b) {
        T* Ab = A + b * strideA;
        int64_t* ip = ipiv ? ipiv + b * stride_ipiv : nullptr;
        if (row_major) RFLU_TRY(getrf_rm<T>(h, m, n, Ab, lda, ip, pivot, 0, &infos[(size_t)b]));
        else RFLU_TRY(getrf_cm_dev<T>(h, m, n, Ab, lda, ip, pivot, 0, &infos[(size_t)b]));
    }
    RFLU_HIP(hipMemcpyAsync(info_dev, infos.data(), (size_t)batch * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
    RFLU_HIP(hipStreamSynchronize(h->stream));
    return RFLU_OK;
}

template <typename T>
static int getrs_batched(Handle* h, int64_t batch, int64_t n, int64_t nrhs, const T* F, int64_t lda, int64_t strideF, int row_major,
                         const int64_t* ipiv, int64_t stride_ipiv, T* B, int64_t ldb, int64_t strideB, int trans)
{
    int rc;
    if (!check_batched_solve_args("getrs_batched", batch, n, nrhs, F, lda, strideF, row_major, ipiv, stride_ipiv, B, ldb, strideB, trans, false, &rc)) return rc;
    if (batched_fits(n, n)) {
        RFLU_TRY(launch_getrs_batched<T>(h, batch, n, nrhs, F, lda, strideF, row_major, ipiv, stride_ipiv, B, ldb, strideB, trans ? 1 : 0));
        RFLU_HIP(hipStreamSynchronize(h->stream));
        h->last_path = RFLU_PATH_HIP_BATCHED;
        return RFLU_OK;
    }
    for (int64_t b = 0; b < batch; ++b) {
        const T* Fb = F + b * strideF;
        const int64_t* ip = ipiv ? ipiv + b * stride_ipiv : nullptr;
        T* Bb = B + b * strideB;
        if (row_major) RFLU_TRY(trans ? getrs_trans_rm<T>(h, n, nrhs, Fb, lda, ip, Bb, ldb) : getrs_rm<T>(h, n, nrhs, Fb, lda, ip, Bb, ldb));
        else RFLU_TRY(trans ? getrs_trans_cm_dev<T>(h, n, nrhs, Fb, lda, ip, Bb, ldb) : getrs_cm_dev<T>(h, n, nrhs, Fb, lda, ip, Bb, ldb));
    }
    RFLU_HIP(hipStreamSynchronize(h->stream));
    return RFLU_OK;
}

// ---- complex batched entries (include/rflu.h; kernels: batched_complex.hip).  Above the one-launch limit:
// column-major batches loop over the single-matrix complex device path; row-major ones are refused, because that path is column-major only.
template <typename R>
static int refuse_large_row_major(const char* who)
{
    const int lim = sizeof(R) == 8 ? (int)CBATCHED_MAX_DIM_CF64 : (int)CBATCHED_MAX_DIM_CF32;
    set_error("%s: row-major matrices larger than %d x %d are not served (the single-matrix complex path that "
              "larger batches loop over is column-major only)", who, lim, lim);
    return RFLU_ERR_ARG;
}

template <typename R>
static int cgetrf_batched(Handle* h, int64_t batch, int64_t m, int64_t n, R* A, int64_t lda, int64_t strideA, int row_major,
                          int64_t* ipiv, int64_t stride_ipiv, int pivot, int64_t* info_dev)
{
    int rc;
    if (!check_batched_factor_args("complex getrf_batched", batch, m, n, A, lda, strideA, row_major, ipiv, stride_ipiv, pivot, info_dev, &rc)) return rc;
    if (cbatched_fits<R>(m, n)) {
        RFLU_TRY(launch_cgetrf_batched<R>(h, batch, m, n, A, lda, strideA, row_major, ipiv, stride_ipiv, pivot, info_dev));
        RFLU_HIP(hipStreamSynchronize(h->stream));
        h->last_path = RFLU_PATH_HIP_BATCHED;
        return RFLU_OK;
    }
    if (row_major) return refuse_large_row_major<R>("complex getrf_batched");
    std::vector<int64_t> infos((size_t)batch, 0);
    for (int64_t b = 0; b < batch; ++b)
        RFLU_TRY(cgetrf_cm_dev<R>(h, m, n, A + 2 * b * strideA, lda, ipiv ? ipiv + b * stride_ipiv : nullptr, pivot, &infos[(size_t)b]));
    RFLU_HIP(hipMemcpyAsync(info_dev, infos.data(), (size_t)batch * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
    RFLU_HIP(hipStreamSynchronize(h->stream));
    return RFLU_OK;
}

template <typename R>
static int cgetrs_batched(Handle* h, int64_t batch, int64_t n, int64_t nrhs, const R* F, int64_t lda, int64_t strideF, int row_major,
                          const int64_t* ipiv, int64_t stride_ipiv, R* B, int64_t ldb, int64_t strideB, int trans)
{
    int rc;
    if (!check_batched_solve_args("complex getrs_batched", batch, n, nrhs, F, lda, strideF, row_major, ipiv, stride_ipiv, B, ldb, strideB, trans, true, &rc)) return rc;
    if (cbatched_fits<R>(n, n)) {
        RFLU_TRY(launch_cgetrs_batched<R>(h, batch, n, nrhs, F, lda, strideF, row_major, ipiv, stride_ipiv, B, ldb, strideB, trans));
        RFLU_HIP(hipStreamSynchronize(h->stream));
        h->last_path = RFLU_PATH_HIP_BATCHED;
        return RFLU_OK;
    }
    if (row_major) return refuse_large_row_major<R>("complex getrs_batched");
    for (int64_t b = 0; b < batch; ++b) {
        const R* Fb = F + 2 * b * strideF;
        const int64_t* ip = ipiv ? ipiv + b * stride_ipiv : nullptr;
        R* Bb = B + 2 * b * strideB;
        if (trans) RFLU_TRY(cgetrs_trans_cm_dev<R>(h, n, nrhs, Fb, lda, ip, Bb, ldb, trans == 2 ? 1 : 0));
        else RFLU_TRY(cgetrs_cm_dev<R>(h, n, nrhs, Fb, lda, ip, Bb, ldb));
    }
    RFLU_HIP(hipStreamSynchronize(h->stream));
    return RFLU_OK;
}

// ---- inv / det / logabsdet from the factors, real and complex (include/rflu.h; kernels and the two sweeps: inverse.hip, DESIGN.md
// sections 4.4, 4.8, 4.9).  E is the element trait of rflu_internal.hpp: sizes, leading dimensions and strides count elements, every
// message starts with E::WHO.  The sign is one word for real elements and (re, im) for complex ones: sign_im belongs to the latter only.
template <typename E>
static int logabsdet_dev(Handle* h, int64_t n, const typename E::real* F, int64_t ld, const int64_t* ipiv, double* logabs, double* sign_re,
                         double* sign_im)
{
    RFLU_TRY(logabsdet_check_args<E>(n, F, ld, logabs, sign_re, sign_im));   // ... and the empty product in the outputs
    if (n == 0) return RFLU_OK;
    return launch_logabsdet<E>(h, n, F, ld + 1, ipiv, logabs, sign_re, sign_im, nullptr);
}

// sign_dev: E::PARTS words per matrix
template <typename E>
static int logabsdet_batched(Handle* h, int64_t batch, int64_t n, const typename E::real* F, int64_t lda, int64_t strideF,
                             const int64_t* ipiv, int64_t stride_ipiv, double* logabs_dev, double* sign_dev)
{
    if (batch < 0 || n < 0) {
        set_error("%slogabsdet_batched: negative size batch=%lld n=%lld", E::WHO, (long long)batch, (long long)n);
        return RFLU_ERR_ARG;
    }
    if (batch == 0) return RFLU_OK;
    if (logabs_dev == nullptr || sign_dev == nullptr || (n > 0 && F == nullptr)) { set_error("%slogabsdet_batched: null pointer", E::WHO); return RFLU_ERR_ARG; }
    if (n > 0 && (lda < n || (batch > 1 && strideF < (n - 1) * lda + n))) {
        set_error("%slogabsdet_batched: lda=%lld strideF=%lld too small for n=%lld", E::WHO, (long long)lda, (long long)strideF, (long long)n);
        return RFLU_ERR_ARG;
    }
    if (ipiv && batch > 1 && stride_ipiv < n) { set_error("%slogabsdet_batched: stride_ipiv=%lld < n", E::WHO, (long long)stride_ipiv); return RFLU_ERR_ARG; }
    if (n == 0) {   // the empty product: (0, 1) or (0, 1 + 0i) for every matrix
        std::vector<double> z((size_t)batch, 0.0), o(E::PARTS * (size_t)batch, 0.0);
        for (int64_t b = 0; b < batch; ++b) o[E::PARTS * (size_t)b] = 1.0;
        RFLU_HIP(hipMemcpyAsync(logabs_dev, z.data(), z.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
        RFLU_HIP(hipMemcpyAsync(sign_dev, o.data(), o.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
        RFLU_HIP(hipStreamSynchronize(h->stream));
        return RFLU_OK;
    }
    RFLU_TRY(launch_logabsdet_batched<E>(h, batch, n, F, lda + 1, strideF, ipiv, stride_ipiv, logabs_dev, sign_dev));
    RFLU_HIP(hipStreamSynchronize(h->stream));
    return RFLU_OK;
}

// column-major device entry: F read as a row-major array with ld = lda IS the transposed view, and A^-1 column-major IS A^-T row-major:
// no layout change, whatever lda and the pointer's alignment (misaligned: the GEMM's element-wise loads, same arithmetic)
template <typename E>
int getri_cm_dev(Handle* h, int64_t n, typename E::real* F, int64_t lda, const int64_t* ipiv, int64_t* info)
{
    RFLU_TRY(getri_check_args<E>(n, F, lda, info));
    *info = 0;
    if (n == 0) return RFLU_OK;
    return getri_view<E>(h, n, F, lda, ipiv, info);
}

// row-major real factors: one layout change into the handle's workspace, the sweeps there, one layout change back
template <typename T>
static int getri_rm(Handle* h, int64_t n, T* R, int64_t ld, const int64_t* ipiv, int64_t* info)
{
    if (n < 0 || ld < std::max<int64_t>(n, 1) || info == nullptr || (n > 0 && R == nullptr)) {
        set_error("getri_rm: bad arguments n=%lld ld=%lld (or a null pointer)", (long long)n, (long long)ld);
        return RFLU_ERR_ARG;
    }
    *info = 0;
    if (n == 0) return RFLU_OK;
    const int64_t ldv = workspace_ld(h, n);
    RFLU_TRY(ensure_buffer(&h->work, &h->work_bytes, (size_t)n * (size_t)ldv * sizeof(T)));
    T* V = static_cast<T*>(h->work);
    RFLU_TRY(launch_transpose<T>(h, n, n, R, ld, V, ldv));
    RFLU_TRY(getri_view<RealElem<T>>(h, n, V, ldv, ipiv, info));
    if (*info != 0) return RFLU_OK;
    RFLU_TRY(launch_transpose<T>(h, n, n, V, ldv, R, ld));
    RFLU_HIP(hipStreamSynchronize(h->stream));
    return RFLU_OK;
}

// the batched inverse (kernels: batched.hip / batched_complex.hip), out of place.  Complex elements take `trans`:
// Ainv_b <- inv(op(A_b)), op = A / transpose(A) / A' by 0 / 1 / 2; real entries pass 0.  Above the one-launch limit a loop over the
// single-matrix getri on a copy: real row-major batches through getri_rm, complex ones are column-major only and 'T' / 'C' take one
// layout change of the result through the handle's workspace (conjugating for 'C') and a copy back -- correct, not fast.
template <typename E>
static int getri_batched(Handle* h, int64_t batch, int64_t n, const typename E::real* F, int64_t lda, int64_t strideF, int row_major,
                         const int64_t* ipiv, int64_t stride_ipiv, typename E::real* Ainv, int64_t ldi, int64_t strideI, int trans,
                         int64_t* info_dev)
{
    typedef typename E::real R;
    constexpr bool CPLX = E::PARTS == 2;
    constexpr size_t ES = E::PARTS * sizeof(R);   // bytes of an element
    if (batch < 0 || n < 0) {
        set_error("%sgetri_batched: negative size batch=%lld n=%lld", E::WHO, (long long)batch, (long long)n);
        return RFLU_ERR_ARG;
    }
    if (CPLX && (trans < 0 || trans > 2)) {
        set_error("%sgetri_batched: trans must be 0 (A), 1 (transpose) or 2 (adjoint), got %d", E::WHO, trans);
        return RFLU_ERR_ARG;
    }
    if (batch == 0 || n == 0) return RFLU_OK;
    if (F == nullptr || Ainv == nullptr || info_dev == nullptr) { set_error("%sgetri_batched: null pointer", E::WHO); return RFLU_ERR_ARG; }
    if (lda < n || ldi < n || (batch > 1 && (strideF < (n - 1) * lda + n || strideI < (n - 1) * ldi + n))) {
        set_error("%sgetri_batched: lda=%lld strideF=%lld ldi=%lld strideI=%lld too small for n=%lld", E::WHO, (long long)lda,
                  (long long)strideF, (long long)ldi, (long long)strideI, (long long)n);
        return RFLU_ERR_ARG;
    }
    if (ipiv && batch > 1 && stride_ipiv < n) { set_error("%sgetri_batched: stride_ipiv=%lld < n", E::WHO, (long long)stride_ipiv); return RFLU_ERR_ARG; }
    if (CPLX ? cbatched_fits<R>(n, n) : batched_fits(n, n)) {
        if constexpr (CPLX) RFLU_TRY(launch_cgetri_batched<R>(h, batch, n, F, lda, strideF, row_major, ipiv, stride_ipiv, Ainv, ldi, strideI, trans, info_dev));
        else RFLU_TRY(launch_getri_batched<R>(h, batch, n, F, lda, strideF, row_major, ipiv, stride_ipiv, Ainv, ldi, strideI, info_dev));
        RFLU_HIP(hipStreamSynchronize(h->stream));
        h->last_path = RFLU_PATH_HIP_BATCHED;
        return RFLU_OK;
    }
    if (CPLX && row_major) return refuse_large_row_major<R>("complex getri_batched");
    std::vector<int64_t> infos((size_t)batch, 0);
    for (int64_t b = 0; b < batch; ++b) {
        const int64_t* ip = ipiv ? ipiv + b * stride_ipiv : nullptr;
        R* Xb = Ainv + E::PARTS * b * strideI;
        RFLU_HIP(hipMemcpy2DAsync(Xb, (size_t)ldi * ES, F + E::PARTS * b * strideF, (size_t)lda * ES, (size_t)n * ES, (size_t)n,
                                  hipMemcpyDeviceToDevice, h->stream));
        int rc;
        if constexpr (CPLX) rc = getri_cm_dev<E>(h, n, Xb, ldi, ip, &infos[(size_t)b]);   // (row-major batches were refused above)
        else rc = row_major ? getri_rm<R>(h, n, Xb, ldi, ip, &infos[(size_t)b]) : getri_cm_dev<E>(h, n, Xb, ldi, ip, &infos[(size_t)b]);
        RFLU_TRY(rc);
        if (infos[(size_t)b] != 0) {   // a singular matrix: its output is NaN, as the one-launch path's division by zero leaves it non-finite
            RFLU_HIP(hipMemset2DAsync(Xb, (size_t)ldi * ES, 0xff, (size_t)n * ES, (size_t)n, h->stream));
        } else if constexpr (CPLX) {
            if (trans) {
                const int64_t ldw = cworkspace_ld(n);
                RFLU_TRY(ensure_buffer(&h->work, &h->work_bytes, (size_t)n * (size_t)ldw * ES));
                R* W = static_cast<R*>(h->work);
                RFLU_TRY(launch_ctranspose<R>(h, n, n, Xb, ldi, W, ldw, trans == 2));
                RFLU_HIP(hipMemcpy2DAsync(Xb, (size_t)ldi * ES, W, (size_t)ldw * ES, (size_t)n * ES, (size_t)n, hipMemcpyDeviceToDevice, h->stream));
            }
        }
    }
    RFLU_HIP(hipMemcpyAsync(info_dev, infos.data(), (size_t)batch * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
    RFLU_HIP(hipStreamSynchronize(h->stream));
    return RFLU_OK;
}

// ---- operator norms and the condition estimate, real and complex (include/rflu.h: NORMS, COMPLEX NORMS, CONDITION; kernels: condest.hip
// and the batched estimators of batched.hip / batched_complex.hip, DESIGN.md sections 4.11, 4.12).  E is the element trait of
// rflu_internal.hpp: sizes, leading dimensions and strides count elements, every message starts with E::WHO.
static bool norm_ok(const char* pre, const char* who, int norm)
{
    if (norm == RFLU_NORM_ONE || norm == RFLU_NORM_INF) return true;
    set_error("%s%s: norm must be RFLU_NORM_ONE (1) or RFLU_NORM_INF (2), got %d", pre, who, norm);
    return false;
}

template <typename E>
static int lange_dev(Handle* h, int norm, int64_t m, int64_t n, const typename E::real* A, int64_t lda, int row_major, double* out)
{
    if (!norm_ok(E::WHO, "lange", norm)) return RFLU_ERR_ARG;
    if (m < 0 || n < 0 || out == nullptr || lda < std::max<int64_t>(row_major ? n : m, 1) || (m > 0 && n > 0 && A == nullptr)) {
        set_error("%slange: bad arguments m=%lld n=%lld lda=%lld (or a null pointer)", E::WHO, (long long)m, (long long)n, (long long)lda);
        return RFLU_ERR_ARG;
    }
    return launch_lange<E>(h, norm, m, n, A, lda, row_major, out);
}

template <typename E>
static int lange_batched(Handle* h, int norm, int64_t batch, int64_t m, int64_t n, const typename E::real* A, int64_t lda, int64_t strideA,
                         int row_major, double* out_dev)
{
    if (!norm_ok(E::WHO, "lange_batched", norm)) return RFLU_ERR_ARG;
    if (batch < 0 || m < 0 || n < 0) {
        set_error("%slange_batched: negative size batch=%lld m=%lld n=%lld", E::WHO, (long long)batch, (long long)m, (long long)n);
        return RFLU_ERR_ARG;
    }
    if (batch == 0) return RFLU_OK;
    if (out_dev == nullptr || (m > 0 && n > 0 && A == nullptr)) { set_error("%slange_batched: null pointer", E::WHO); return RFLU_ERR_ARG; }
    if (m == 0 || n == 0) {
        RFLU_HIP(hipMemsetAsync(out_dev, 0, (size_t)batch * sizeof(double), h->stream));
        RFLU_HIP(hipStreamSynchronize(h->stream));
        return RFLU_OK;
    }
    const int64_t len = row_major ? n : m, cnt = row_major ? m : n;
    if (lda < len || (batch > 1 && strideA < (cnt - 1) * lda + len)) {
        set_error("%slange_batched: lda=%lld strideA=%lld too small for %lld x %lld (%s)", E::WHO, (long long)lda, (long long)strideA,
                  (long long)m, (long long)n, row_major ? "row-major" : "column-major");
        return RFLU_ERR_ARG;
    }
    RFLU_TRY(launch_lange_batched<E>(h, norm, batch, m, n, A, lda, strideA, row_major, out_dev));
    RFLU_HIP(hipStreamSynchronize(h->stream));
    return RFLU_OK;
}

// Higham's estimate of ||M||_1 (LAPACK xLACN2 with the integer start and closing vectors stated in rflu.h) on the caller's work vector
// x: fill(mode, j) makes a start vector, apply(false) is x <- M x and apply(true) x <- M^T x (complex: M^H x), stats(jq, write, &st) the
// statistics of x, after which x holds its signs (phases) when `write`.  sign_ends: an unchanged sign vector ends the iteration (real
// elements; complex phases are never compared).  *bad: a NaN or Inf turned up in x, *est then says nothing.
template <typename Fill, typename Apply, typename Stats>
static int higham_estimate(int64_t n, bool sign_ends, Fill fill, Apply apply, Stats stats, double* est_out, bool* bad_out)
{
    CondStats st;
    double est = 0.0;
    bool bad = false, closing = false;
    int64_t j = 0;
    for (int round = 0; round < 5; ++round) {
        RFLU_TRY(fill(round == 0 ? COND_FILL_ONES : COND_FILL_UNIT, j));
        RFLU_TRY(apply(false));
        RFLU_TRY(stats(-1, 1, &st));
        if (st.nonfinite) { bad = true; break; }
        if (round == 0) {
            est = st.sum / (double)n;
            if (n == 1) break;
        } else {
            const double est_old = est;
            est = st.sum;
            if ((sign_ends && st.differs == 0) || est <= est_old) { closing = true; break; }
        }
        RFLU_TRY(apply(true));
        RFLU_TRY(stats(j, 0, &st));
        if (st.nonfinite) { bad = true; break; }
        j = (int64_t)st.argmax;
        if ((round > 0 && st.xj_abs == st.maxabs) || round == 4) { closing = true; break; }
    }
    if (closing) {
        RFLU_TRY(fill(COND_FILL_ALT, 0));
        RFLU_TRY(apply(false));
        RFLU_TRY(stats(-1, 0, &st));
        if (st.nonfinite) bad = true;
        else {
            const double alt = 2.0 * st.sum / (3.0 * (double)n * (double)(n - 1));
            if (alt > est) est = alt;
        }
    }
    *est_out = est;
    *bad_out = bad;
    return RFLU_OK;
}

// the estimate on the n elements at x (and, real elements, their signs at sgn) with the caller's two solves, then rcond
template <typename E, typename Apply>
static int gecon_estimate(Handle* h, int64_t n, const typename E::real* F, int64_t ld, typename E::real* x, typename E::real* sgn,
                          double anorm, Apply apply, double* rcond)
{
    double est = 0.0;
    bool bad = false;
    RFLU_TRY(higham_estimate(
        n, E::PARTS == 1, [&](int mode, int64_t j) { return launch_cond_fill<E>(h, n, x, mode, j); }, apply,
        [&](int64_t jq, int write, CondStats* st) { return launch_cond_stats<E>(h, n, x, sgn, jq, write, st); }, &est, &bad));
    if (bad) {   // overflow in the substitution gives 0; a NaN in the factors (a norm keeps it) gives NaN
        double fnorm = 0.0;
        RFLU_TRY(launch_lange<E>(h, RFLU_NORM_ONE, n, n, F, ld, 0, &fnorm));
        *rcond = (fnorm != fnorm) ? fnorm : 0.0;
        return RFLU_OK;
    }
    *rcond = est == 0.0 ? 0.0 : 1.0 / (anorm * est);
    return RFLU_OK;
}

// rcond = 1 / (anorm * est) with Higham's estimator on M = U^-1 L^-1.  ONE layout change per call: W = the transposed image of F in
// h->work.  Column-major factors: W is their row-major image, every M x is getrs_rm on W and every M^T x is getrs_trans_view on F in
// place; row-major factors: M x is getrs_rm on F in place and M^T x is getrs_trans_view on W.  The work vector stays in the row-major
// n x 1 form the chain kernels take (ldb = 1).
template <typename T>
int gecon_dev(Handle* h, int norm, int64_t n, const T* F, int64_t ld, int row_major, double anorm, double* rcond)
{
    if (!norm_ok("", "gecon", norm)) return RFLU_ERR_ARG;
    if (n < 0 || ld < std::max<int64_t>(n, 1) || rcond == nullptr || (n > 0 && F == nullptr)) {
        set_error("gecon: bad arguments n=%lld ld=%lld (or a null pointer)", (long long)n, (long long)ld);
        return RFLU_ERR_ARG;
    }
    if (anorm < 0.0) { set_error("gecon: anorm = %g is negative", anorm); return RFLU_ERR_ARG; }
    if (n > (int64_t)NB * 256 * 4) {
        set_error("gecon: n = %lld exceeds the %d rows the cooperative transposed solve covers", (long long)n, NB * 256 * 4);
        return RFLU_ERR_ARG;
    }
    *rcond = 0.0;
    if (n == 0) { *rcond = 1.0; return RFLU_OK; }
    if (anorm != anorm) { *rcond = anorm; return RFLU_OK; }
    if (anorm == 0.0) return RFLU_OK;
    int64_t zero1 = 0;
    RFLU_TRY(launch_logabsdet<RealElem<T>>(h, n, F, ld + 1, nullptr, nullptr, nullptr, nullptr, &zero1));
    if (zero1 != 0) return RFLU_OK;   // an exactly zero u_ii: rcond = 0 before any solve is launched

    const int64_t ldw = workspace_ld(h, n);
    RFLU_TRY(ensure_buffer(&h->work, &h->work_bytes, (size_t)n * (size_t)ldw * sizeof(T)));
    RFLU_TRY(ensure_buffer(&h->cond_work, &h->cond_work_bytes, 2 * (size_t)n * sizeof(T)));
    T* W = static_cast<T*>(h->work);
    T* x = static_cast<T*>(h->cond_work);
    T* sgn = x + n;
    RFLU_TRY(launch_transpose<T>(h, n, n, F, ld, W, ldw));
    RFLU_HIP(hipMemsetAsync(sgn, 0, (size_t)n * sizeof(T), h->stream));
    const T* RM = row_major ? F : W;
    const T* V = row_major ? W : F;
    const int64_t ldrm = row_major ? ld : ldw, ldv = row_major ? ldw : ld;
    // ||M||_inf = ||M^T||_1: for the Inf norm M and M^T swap roles
    auto apply = [&](bool transposed) -> int {
        if (transposed != (norm == RFLU_NORM_INF)) return getrs_trans_view<T>(h, n, 1, V, ldv, nullptr, x, 1);
        return getrs_rm<T>(h, n, 1, RM, ldrm, nullptr, x, 1);
    };
    return gecon_estimate<RealElem<T>>(h, n, F, ld, x, sgn, anorm, apply, rcond);
}

// The same on M = U^-1 L^-1 of column-major complex factors.  ONE layout change per call: W = the row-major image of F in h->work.
// Every M x is csolve_fwd_narrow on W, every M^H x the narrow path of cgetrs_trans_cm_dev (conj = 1) on F in place, both with
// ipiv = NULL and one right-hand side, the n contiguous elements of x.  Neither narrow path states a size limit, so there is none here.
template <typename R>
int cgecon_dev(Handle* h, int norm, int64_t n, const R* F, int64_t lda, double anorm, double* rcond)
{
    if (!norm_ok("complex ", "gecon", norm)) return RFLU_ERR_ARG;
    if (n < 0 || lda < std::max<int64_t>(n, 1) || rcond == nullptr || (n > 0 && F == nullptr)) {
        set_error("complex gecon: bad arguments n=%lld lda=%lld (or a null pointer)", (long long)n, (long long)lda);
        return RFLU_ERR_ARG;
    }
    if (anorm < 0.0) { set_error("complex gecon: anorm = %g is negative", anorm); return RFLU_ERR_ARG; }
    *rcond = 0.0;
    if (n == 0) { *rcond = 1.0; return RFLU_OK; }
    if (anorm != anorm) { *rcond = anorm; return RFLU_OK; }
    if (anorm == 0.0) return RFLU_OK;
    int64_t zero1 = 0;
    RFLU_TRY(launch_logabsdet<CplxElem<R>>(h, n, F, lda + 1, nullptr, nullptr, nullptr, nullptr, &zero1));
    if (zero1 != 0) return RFLU_OK;   // a u_ii with both parts zero: rcond = 0 before any solve is launched

    const int64_t ldw = cworkspace_ld(n);
    RFLU_TRY(ensure_buffer(&h->work, &h->work_bytes, (size_t)n * (size_t)ldw * 2 * sizeof(R)));
    RFLU_TRY(ensure_buffer(&h->cond_work, &h->cond_work_bytes, (size_t)n * 2 * sizeof(R)));
    R* W = static_cast<R*>(h->work);
    R* x = static_cast<R*>(h->cond_work);
    RFLU_TRY(launch_ctranspose<R>(h, n, n, F, lda, W, ldw));
    // ||M||_inf = ||M^H||_1: for the Inf norm M and M^H swap roles
    auto apply = [&](bool adjoint) -> int {
        if (adjoint != (norm == RFLU_NORM_INF)) return cgetrs_trans_cm_dev<R>(h, n, 1, F, lda, nullptr, x, n, 1);
        return csolve_fwd_narrow<R>(h, n, 1, W, ldw, nullptr, x, n);
    };
    return gecon_estimate<CplxElem<R>>(h, n, F, lda, x, nullptr, anorm, apply, rcond);
}
template int cgecon_dev<double>(Handle*, int, int64_t, const double*, int64_t, double, double*);
template int cgecon_dev<float>(Handle*, int, int64_t, const float*, int64_t, double, double*);

// One launch where the matrix fits a workgroup's LDS; above that a loop over the single-matrix estimate, which for complex elements is
// column-major only.
template <typename E>
static int gecon_batched(Handle* h, int norm, int64_t batch, int64_t n, const typename E::real* F, int64_t lda, int64_t strideF,
                         int row_major, const double* anorm_dev, double* rcond_dev)
{
    typedef typename E::real R;
    constexpr bool CPLX = E::PARTS == 2;
    if (!norm_ok(E::WHO, "gecon_batched", norm)) return RFLU_ERR_ARG;
    if (batch < 0 || n < 0) {
        set_error("%sgecon_batched: negative size batch=%lld n=%lld", E::WHO, (long long)batch, (long long)n);
        return RFLU_ERR_ARG;
    }
    if (batch == 0) return RFLU_OK;
    if (rcond_dev == nullptr || (n > 0 && (F == nullptr || anorm_dev == nullptr))) { set_error("%sgecon_batched: null pointer", E::WHO); return RFLU_ERR_ARG; }
    if (n > 0 && (lda < n || (batch > 1 && strideF < (n - 1) * lda + n))) {
        set_error("%sgecon_batched: lda=%lld strideF=%lld too small for n=%lld", E::WHO, (long long)lda, (long long)strideF, (long long)n);
        return RFLU_ERR_ARG;
    }
    std::vector<double> host((size_t)batch, 1.0);
    if (n == 0) {   // the empty matrix: rcond = 1
        RFLU_HIP(hipMemcpyAsync(rcond_dev, host.data(), (size_t)batch * sizeof(double), hipMemcpyHostToDevice, h->stream));
        RFLU_HIP(hipStreamSynchronize(h->stream));
        return RFLU_OK;
    }
    if (CPLX ? cbatched_fits<R>(n, n) : batched_fits(n, n)) {
        RFLU_TRY(CPLX ? launch_cgecon_batched<R>(h, norm, batch, n, F, lda, strideF, row_major, anorm_dev, rcond_dev)
                      : launch_gecon_batched<R>(h, norm, batch, n, F, lda, strideF, row_major, anorm_dev, rcond_dev));
        RFLU_HIP(hipStreamSynchronize(h->stream));
        return RFLU_OK;
    }
    if (CPLX && row_major) return refuse_large_row_major<R>("complex gecon_batched");
    RFLU_HIP(hipMemcpyAsync(host.data(), anorm_dev, (size_t)batch * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    RFLU_HIP(hipStreamSynchronize(h->stream));
    for (int64_t b = 0; b < batch; ++b) {
        const double an = host[(size_t)b];
        if (an < 0.0) { host[(size_t)b] = std::nan(""); continue; }   // a member's bad anorm spoils its own output only
        const R* Fb = F + E::PARTS * b * strideF;
        RFLU_TRY(CPLX ? cgecon_dev<R>(h, norm, n, Fb, lda, an, &host[(size_t)b]) : gecon_dev<R>(h, norm, n, Fb, lda, row_major, an, &host[(size_t)b]));
    }
    RFLU_HIP(hipMemcpyAsync(rcond_dev, host.data(), (size_t)batch * sizeof(double), hipMemcpyHostToDevice, h->stream));
    RFLU_HIP(hipStreamSynchronize(h->stream));
    return RFLU_OK;
}

// ---- mixed precision: Float32 / ComplexF32 factors of a Float64 / ComplexF64 matrix, iterative refinement in the wide type (LAPACK
// dsgesv's and zcgesv's scheme; kernels: mixed.hip; DESIGN.md sections 4.3, 4.10) ---------------------------------------------------------
// One host path for both families, E = RealElem<double> / CplxElem<double>: leading dimensions count elements, a pointer steps by
// E::PARTS words per element, norms are absolute values or moduli.  The narrow factors stay in the row-major layout their factorization
// leaves them in and every solve of the loop works on them: no n x n layout change after the first.  What differs -- the factorization
// and the narrow solve with the shape of its workspace -- is the entry's lambda.
static int ensure_mixed_norms(Handle* h, int64_t count)
{
    const size_t need = (size_t)std::max<int64_t>(count, 2) * sizeof(double);
    RFLU_TRY(ensure_buffer(&h->mixed_norms, &h->mixed_norms_bytes, need));
    if (h->mixed_norms_host_bytes < need) {
        if (h->mixed_norms_host) RFLU_HIP(hipHostFree(h->mixed_norms_host));
        h->mixed_norms_host = nullptr;
        h->mixed_norms_host_bytes = 0;
        RFLU_HIP(hipHostMalloc(&h->mixed_norms_host, need));
        h->mixed_norms_host_bytes = need;
    }
    return RFLU_OK;
}

// F <- narrow(A) with ||A||_inf on the way, then factor(info) on F: getrf_rm<float> or cgetrf_rm_dev<float>, which wait for the stream
template <typename E, typename Factor>
static int mixed_getrf(Handle* h, int64_t n, const double* A, int64_t lda, float* F, int64_t ldf, const int64_t* ipiv, int pivot,
                       double* anorm_out, int64_t* info, Factor factor)
{
    if (n < 0 || n > INT32_MAX || lda < std::max<int64_t>(n, 1) || ldf < std::max<int64_t>(n, 1)) {
        set_error("%smixed_getrf: bad arguments n=%lld lda=%lld ldf=%lld", E::WHO, (long long)n, (long long)lda, (long long)ldf);
        return RFLU_ERR_ARG;
    }
    if (anorm_out == nullptr || info == nullptr) { set_error("%smixed_getrf: null anorm_out or info pointer", E::WHO); return RFLU_ERR_ARG; }
    if (n > 0 && (A == nullptr || F == nullptr)) { set_error("%smixed_getrf: null matrix pointer", E::WHO); return RFLU_ERR_ARG; }
    if (pivot && ipiv == nullptr && n > 0) { set_error("%smixed_getrf: pivot != 0 needs an ipiv buffer", E::WHO); return RFLU_ERR_ARG; }
    *anorm_out = 0.0;
    *info = 0;
    if (n == 0) return RFLU_OK;
    RFLU_TRY(ensure_mixed_norms(h, 2));
    RFLU_TRY(launch_demote_relayout<E>(h, n, A, lda, F, ldf, static_cast<double*>(h->mixed_norms)));
    RFLU_HIP(hipMemcpyAsync(h->mixed_norms_host, h->mixed_norms, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    RFLU_TRY(factor(info));   // waits for the stream: the norm has arrived
    *anorm_out = static_cast<const double*>(h->mixed_norms_host)[0];
    return RFLU_OK;
}

// C <- C - A B on row-major operands of the family
static int mixed_gemm(RealElem<double>, Handle* h, int64_t M, int64_t N, int64_t K, const double* A, int64_t lda, const double* B, int64_t ldb,
                      double* C, int64_t ldc) { return gemm_public<double>(h, M, N, K, A, lda, B, ldb, C, ldc); }
static int mixed_gemm(CplxElem<double>, Handle* h, int64_t M, int64_t N, int64_t K, const double* A, int64_t lda, const double* B, int64_t ldb,
                      double* C, int64_t ldc) { return launch_cgemm<double>(h, M, N, K, A, lda, B, ldb, C, ldc); }

// R <- B - A X.  Few right-hand sides: residual_few in passes of RESIDUAL_PASS (A streamed once per pass).  Many: read as row-major, a
// column-major matrix is its transpose, so after R <- B the row-major GEMM C -= A B with C = R^T (nrhs x n), A = X^T, B = A^T is
// R^T -= X^T A^T (plain transposes, nothing conjugated), in place on the column-major buffers.
// The crossover is tune.mixed_gemv_max_rhs, chosen for real elements: a structural starting value for complex, not measured.
template <typename E>
static int mixed_residual(Handle* h, int64_t n, int64_t nrhs, const double* A, int64_t lda, const double* X, int64_t ldx, const double* B,
                          int64_t ldb, double* R, int64_t ldr)
{
    constexpr int P = E::PARTS;
    if (n <= 0 || nrhs <= 0) return RFLU_OK;
    if (nrhs <= h->tune.mixed_gemv_max_rhs) {
        for (int64_t k0 = 0; k0 < nrhs; k0 += RESIDUAL_PASS)
            RFLU_TRY(launch_residual_few<E>(h, n, std::min<int64_t>(RESIDUAL_PASS, nrhs - k0), A, lda, X + P * k0 * ldx, ldx, B + P * k0 * ldb,
                                            ldb, R + P * k0 * ldr, ldr));
        return RFLU_OK;
    }
    RFLU_HIP(hipMemcpy2DAsync(R, (size_t)ldr * P * sizeof(double), B, (size_t)ldb * P * sizeof(double), (size_t)n * P * sizeof(double),
                              (size_t)nrhs, hipMemcpyDeviceToDevice, h->stream));
    return mixed_gemm(E(), h, nrhs, n, n, X, ldx, A, lda, R, ldr);
}

template <typename E>
static int residual_public(Handle* h, int64_t n, int64_t nrhs, const double* A, int64_t lda, const double* X, int64_t ldx, const double* B,
                           int64_t ldb, double* R, int64_t ldr)
{
    const int64_t n1 = std::max<int64_t>(n, 1);
    if (n < 0 || nrhs < 0 || n > INT32_MAX || nrhs > INT32_MAX || lda < n1 || ldx < n1 || ldb < n1 || ldr < n1) {
        set_error("%sresidual: bad arguments n=%lld nrhs=%lld lda=%lld ldx=%lld ldb=%lld ldr=%lld", E::WHO, (long long)n, (long long)nrhs,
                  (long long)lda, (long long)ldx, (long long)ldb, (long long)ldr);
        return RFLU_ERR_ARG;
    }
    if (n == 0 || nrhs == 0) return RFLU_OK;
    if (A == nullptr || X == nullptr || B == nullptr || R == nullptr) { set_error("%sresidual: null pointer", E::WHO); return RFLU_ERR_ARG; }
    RFLU_TRY(mixed_residual<E>(h, n, nrhs, A, lda, X, ldx, B, ldb, R, ldr));
    RFLU_HIP(hipStreamSynchronize(h->stream));
    return RFLU_OK;
}

// X <- A^-1 B: x_0 = F32^-1 narrow(B); then r = B - A x in the wide type, the norms, the decision (dsgesv's rule: converged when for
// every column ||r_k||_inf <= ||x_k||_inf * anorm * eps * sqrt(n); written so that a NaN or Inf anywhere is NOT convergence), and while
// it is not met x += F32^-1 narrow(r).  One host read per step: the 2 nrhs norms.  *iters: the steps taken, or -(steps + 1) when the
// rule is still not met after max_iter of them.
// correct(S, lds, add): X (+)= F32^-1 narrow(S) through the entry's workspace, the first w_bytes of Handle::mixed_rhs.
template <typename E, typename Correct>
static int mixed_refine(Handle* h, int64_t n, int64_t nrhs, const double* A, int64_t lda, const float* F, int64_t ldf, double anorm,
                        const double* B, int64_t ldb, double* X, int64_t ldx, int max_iter, int* iters, size_t w_bytes, Correct correct)
{
    const int64_t n1 = std::max<int64_t>(n, 1);
    if (n < 0 || nrhs < 0 || n > INT32_MAX || nrhs > INT32_MAX || lda < n1 || ldf < n1 || ldb < n1 || ldx < n1) {
        set_error("%smixed_getrs: bad arguments n=%lld nrhs=%lld lda=%lld ldf=%lld ldb=%lld ldx=%lld", E::WHO, (long long)n, (long long)nrhs,
                  (long long)lda, (long long)ldf, (long long)ldb, (long long)ldx);
        return RFLU_ERR_ARG;
    }
    if (iters == nullptr) { set_error("%smixed_getrs: null iters pointer", E::WHO); return RFLU_ERR_ARG; }
    *iters = 0;
    if (n == 0 || nrhs == 0) return RFLU_OK;
    if (A == nullptr || F == nullptr || B == nullptr || X == nullptr) { set_error("%smixed_getrs: null pointer", E::WHO); return RFLU_ERR_ARG; }
    if (max_iter <= 0) max_iter = 30;
    RFLU_TRY(ensure_buffer(&h->mixed_rhs, &h->mixed_rhs_bytes, w_bytes));
    RFLU_TRY(ensure_buffer(&h->mixed_r, &h->mixed_r_bytes, (size_t)n * (size_t)nrhs * E::PARTS * sizeof(double)));
    RFLU_TRY(ensure_mixed_norms(h, 2 * nrhs));
    double* R = static_cast<double*>(h->mixed_r);
    double* norms_dev = static_cast<double*>(h->mixed_norms);
    const double* norms = static_cast<const double*>(h->mixed_norms_host);
    const double scale = anorm * DBL_EPSILON * std::sqrt((double)n);

    RFLU_TRY(correct(B, ldb, false));
    for (int step = 0;; ++step) {
        RFLU_TRY(mixed_residual<E>(h, n, nrhs, A, lda, X, ldx, B, ldb, R, n));
        RFLU_TRY(launch_colnorms<E>(h, n, nrhs, R, n, X, ldx, norms_dev));
        RFLU_HIP(hipMemcpyAsync(h->mixed_norms_host, norms_dev, (size_t)(2 * nrhs) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        RFLU_HIP(hipStreamSynchronize(h->stream));
        bool converged = true;
        for (int64_t k = 0; k < nrhs && converged; ++k)
            if (!(norms[2 * k] <= norms[2 * k + 1] * scale)) converged = false;
        if (converged) { *iters = step; return RFLU_OK; }
        if (step >= max_iter) { *iters = -(step + 1); return RFLU_OK; }
        RFLU_TRY(correct(R, n, true));
    }
}

// Real: the Float32 right-hand sides are a row-major n x nrhs image (rows of round_up(nrhs, 16) floats), solved by getrs_rm<float>
static int mixed_getrs(Handle* h, int64_t n, int64_t nrhs, const double* A, int64_t lda, const float* F, int64_t ldf, const int64_t* ipiv,
                       double anorm, const double* B, int64_t ldb, double* X, int64_t ldx, int max_iter, int* iters)
{
    typedef RealElem<double> E;
    const int64_t ldw = round_up(nrhs, 16);
    auto correct = [&](const double* S, int64_t lds, bool add) -> int {
        float* W = static_cast<float*>(h->mixed_rhs);
        RFLU_TRY((launch_convert_transpose<E, double, float>(h, n, nrhs, S, lds, W, ldw, false)));
        RFLU_TRY(getrs_rm<float>(h, n, nrhs, F, ldf, ipiv, W, ldw));
        return launch_convert_transpose<E, float, double>(h, nrhs, n, W, ldw, X, ldx, add);
    };
    return mixed_refine<E>(h, n, nrhs, A, lda, F, ldf, anorm, B, ldb, X, ldx, max_iter, iters, (size_t)n * (size_t)ldw * sizeof(float), correct);
}

// Complex (the solve on the row-major factors: complex_solve.hip): up to CNARROW right-hand sides the ComplexF32 right-hand sides stay
// column-major (the narrow solve works on columns: an element-wise conversion, no transpose), more go through a row-major image.
static int cmixed_getrs(Handle* h, int64_t n, int64_t nrhs, const double* A, int64_t lda, const float* F, int64_t ldf, const int64_t* ipiv,
                        double anorm, const double* B, int64_t ldb, double* X, int64_t ldx, int max_iter, int* iters)
{
    typedef CplxElem<double> E;
    const bool narrow = nrhs <= CNARROW;
    const int64_t ldw = narrow ? cworkspace_ld(n) : cworkspace_ld(nrhs);
    auto correct = [&](const double* S, int64_t lds, bool add) -> int {
        float* W = static_cast<float*>(h->mixed_rhs);
        if (narrow) {
            RFLU_TRY((launch_cconvert<double, float>(h, n, nrhs, S, lds, W, ldw, false)));
            RFLU_TRY(csolve_fwd_narrow<float>(h, n, (int)nrhs, F, ldf, ipiv, W, ldw));
            return launch_cconvert<float, double>(h, n, nrhs, W, ldw, X, ldx, add);
        }
        RFLU_TRY((launch_convert_transpose<E, double, float>(h, n, nrhs, S, lds, W, ldw, false)));
        RFLU_TRY(csolve_fwd_image<float>(h, n, nrhs, F, ldf, ipiv, W, ldw));
        return launch_convert_transpose<E, float, double>(h, nrhs, n, W, ldw, X, ldx, add);
    };
    return mixed_refine<E>(h, n, nrhs, A, lda, F, ldf, anorm, B, ldb, X, ldx, max_iter, iters,
                           (size_t)(narrow ? nrhs : n) * (size_t)ldw * 2 * sizeof(float), correct);
}

// ---- iterative refinement with error bounds: LAPACK xGERFS, trans = 'N' (refine.hip) -----------------------------
// the argument rules the two entries share
template <typename T>
static int refine_args(const char* who, int64_t n, int64_t nrhs, const T* A, int64_t lda, const T* X, int64_t ldx, const T* B, int64_t ldb,
                       const double* berr)
{
    const int64_t n1 = std::max<int64_t>(n, 1);
    if (n < 0 || nrhs < 0 || n > INT32_MAX || nrhs > INT32_MAX || lda < n1 || ldx < n1 || ldb < n1) {
        set_error("%s: bad arguments n=%lld nrhs=%lld lda=%lld ldx=%lld ldb=%lld", who, (long long)n, (long long)nrhs, (long long)lda,
                  (long long)ldx, (long long)ldb);
        return RFLU_ERR_ARG;
    }
    if (berr == nullptr) { set_error("%s: null berr pointer", who); return RFLU_ERR_ARG; }
    if (n > 0 && nrhs > 0 && (A == nullptr || X == nullptr || B == nullptr)) { set_error("%s: null matrix pointer", who); return RFLU_ERR_ARG; }
    return RFLU_OK;
}

// r, w (-> R, Wt), the solve's block (-> D, may be NULL) and {berr, max|x|} of p <= REFINE_PASS columns; one host read, 2 p values
template <typename T>
static int refine_measure(Handle* h, int64_t n, int64_t p, const T* A, int64_t lda, const T* X, int64_t ldx, const T* B, int64_t ldb,
                          double* R, double* Wt, T* D)
{
    double* out_dev = static_cast<double*>(h->mixed_norms);
    RFLU_TRY(launch_absresidual<T>(h, n, p, A, lda, X, ldx, B, ldb, R, Wt, D));
    RFLU_TRY(launch_berr_reduce<T>(h, n, p, R, Wt, X, ldx, out_dev));
    RFLU_HIP(hipMemcpyAsync(h->mixed_norms_host, out_dev, (size_t)(2 * p) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    RFLU_HIP(hipStreamSynchronize(h->stream));
    return RFLU_OK;
}

template <typename T>
static int berr_dev(Handle* h, int64_t n, int64_t nrhs, const T* A, int64_t lda, const T* X, int64_t ldx, const T* B, int64_t ldb, double* berr)
{
    RFLU_TRY(refine_args<T>("berr", n, nrhs, A, lda, X, ldx, B, ldb, berr));
    for (int64_t k = 0; k < nrhs; ++k) berr[k] = 0.0;
    if (n == 0 || nrhs == 0) return RFLU_OK;
    RFLU_TRY(ensure_buffer(&h->mixed_r, &h->mixed_r_bytes, 2 * (size_t)n * REFINE_PASS * sizeof(double)));
    RFLU_TRY(ensure_mixed_norms(h, 2 * REFINE_PASS));
    double* R = static_cast<double*>(h->mixed_r);
    double* Wt = R + n * REFINE_PASS;
    const double* got = static_cast<const double*>(h->mixed_norms_host);
    for (int64_t k0 = 0; k0 < nrhs; k0 += REFINE_PASS) {
        const int64_t p = std::min<int64_t>(REFINE_PASS, nrhs - k0);
        RFLU_TRY(refine_measure<T>(h, n, p, A, lda, X + k0 * ldx, ldx, B + k0 * ldb, ldb, R, Wt, nullptr));
        for (int64_t k = 0; k < p; ++k) berr[k0 + k] = got[2 * k];
    }
    return RFLU_OK;
}

// The loop of xGERFS on passes of REFINE_PASS columns in lock step.  ONE layout change per call: W = the row-major image of F in h->work;
// every correction is getrs_rm(W, ipiv) on the n x REFINE_PASS row-major block the combine kernel wrote (always all REFINE_PASS columns, so
// that a column meets the same solve kernel whatever nrhs is), every transposed solve of the forward error bound getrs_trans_view on F in
// place.  Workspaces: mixed_part (the slices' shares), mixed_r (r and w), mixed_rhs (the block), cond_work (the estimator's x, sgn, wt).
template <typename T>
static int gerfs_dev(Handle* h, int64_t n, int64_t nrhs, const T* A, int64_t lda, const T* F, int64_t ldf, const int64_t* ipiv, const T* B,
                     int64_t ldb, T* X, int64_t ldx, double* ferr, double* berr, int max_iter, int* steps, int64_t* info)
{
    RFLU_TRY(refine_args<T>("gerfs", n, nrhs, A, lda, X, ldx, B, ldb, berr));
    if (ldf < std::max<int64_t>(n, 1)) { set_error("gerfs: ldf=%lld is below n=%lld", (long long)ldf, (long long)n); return RFLU_ERR_ARG; }
    if (info == nullptr) { set_error("gerfs: null info pointer"); return RFLU_ERR_ARG; }
    if (n > 0 && nrhs > 0 && F == nullptr) { set_error("gerfs: null factor pointer"); return RFLU_ERR_ARG; }
    if (ferr != nullptr && n > (int64_t)NB * 256 * 4) {
        set_error("gerfs: n = %lld exceeds the %d rows the cooperative transposed solve covers (ferr = NULL skips the bound)", (long long)n,
                  NB * 256 * 4);
        return RFLU_ERR_ARG;
    }
    *info = 0;
    if (n == 0 || nrhs == 0) {
        for (int64_t k = 0; k < nrhs; ++k) {
            berr[k] = 0.0;
            if (ferr) ferr[k] = 0.0;
            if (steps) steps[k] = 0;
        }
        return RFLU_OK;
    }
    int64_t zero1 = 0;
    RFLU_TRY(launch_logabsdet<RealElem<T>>(h, n, F, ldf + 1, nullptr, nullptr, nullptr, nullptr, &zero1));
    if (zero1 != 0) { *info = zero1; return RFLU_OK; }   // an exactly zero u_ii: before any solve, nothing written
    if (max_iter <= 0) max_iter = 5;
    const double u = sizeof(T) == 8 ? 0x1p-53 : 0x1p-24;

    const int64_t ldw = workspace_ld(h, n);
    RFLU_TRY(ensure_buffer(&h->work, &h->work_bytes, (size_t)n * (size_t)ldw * sizeof(T)));
    RFLU_TRY(ensure_buffer(&h->mixed_r, &h->mixed_r_bytes, 2 * (size_t)n * REFINE_PASS * sizeof(double)));
    RFLU_TRY(ensure_buffer(&h->mixed_rhs, &h->mixed_rhs_bytes, (size_t)n * REFINE_LDD * sizeof(T)));
    RFLU_TRY(ensure_buffer(&h->cond_work, &h->cond_work_bytes, 3 * (size_t)n * sizeof(T)));
    RFLU_TRY(ensure_mixed_norms(h, 2 * REFINE_PASS));
    T* W = static_cast<T*>(h->work);
    double* R = static_cast<double*>(h->mixed_r);
    double* Wt = R + n * REFINE_PASS;
    T* D = static_cast<T*>(h->mixed_rhs);
    T* x = static_cast<T*>(h->cond_work);
    T* sgn = x + n;
    T* wt = sgn + n;
    const double* got = static_cast<const double*>(h->mixed_norms_host);
    RFLU_TRY(launch_transpose<T>(h, n, n, F, ldf, W, ldw));
    // the block's padding columns REFINE_PASS .. REFINE_LDD - 1 are never read or written by the solve (nrhs = REFINE_PASS)

    for (int64_t k0 = 0; k0 < nrhs; k0 += REFINE_PASS) {
        const int64_t p = std::min<int64_t>(REFINE_PASS, nrhs - k0);
        const T* Bp = B + k0 * ldb;
        T* Xp = X + k0 * ldx;
        double lstres[REFINE_PASS], be[REFINE_PASS], xmax[REFINE_PASS];
        int taken[REFINE_PASS];
        unsigned active = (1u << p) - 1u;
        for (int k = 0; k < REFINE_PASS; ++k) { lstres[k] = 3.0; taken[k] = 0; be[k] = xmax[k] = 0.0; }
        for (;;) {
            RFLU_TRY(refine_measure<T>(h, n, p, A, lda, Xp, ldx, Bp, ldb, R, Wt, D));
            for (int k = 0; k < p; ++k) {
                be[k] = got[2 * k];
                xmax[k] = got[2 * k + 1];
                if (!((active >> k) & 1u)) continue;
                // xGERFS's test; written so that a NaN stops the column
                if (be[k] > u && 2.0 * be[k] <= lstres[k] && taken[k] < max_iter) lstres[k] = be[k];
                else active &= ~(1u << k);
            }
            if (active == 0) break;
            RFLU_TRY(getrs_rm<T>(h, n, REFINE_PASS, W, ldw, ipiv, D, REFINE_LDD));
            RFLU_TRY(launch_refine_update<T>(h, n, p, active, D, Xp, ldx));
            for (int k = 0; k < p; ++k)
                if ((active >> k) & 1u) ++taken[k];
        }
        for (int k = 0; k < p; ++k) {
            berr[k0 + k] = be[k];
            if (steps) steps[k0 + k] = taken[k];
        }
        if (ferr == nullptr) continue;
        // r and w of the pass's final X are still in R and Wt: the estimator's buffers are others
        for (int k = 0; k < p; ++k) {
            if (be[k] != be[k]) { ferr[k0 + k] = be[k]; continue; }
            RFLU_TRY(launch_refine_weights<T>(h, n, R + (int64_t)k * n, Wt + (int64_t)k * n, wt));
            RFLU_HIP(hipMemsetAsync(sgn, 0, (size_t)n * sizeof(T), h->stream));
            // M = diag(wt) A^-T: ||A^-1 diag(wt)||_inf = ||M||_1
            auto apply = [&](bool transposed) -> int {
                if (transposed) {
                    RFLU_TRY(launch_refine_scale<T>(h, n, wt, x));
                    return getrs_rm<T>(h, n, 1, W, ldw, ipiv, x, 1);
                }
                RFLU_TRY(getrs_trans_view<T>(h, n, 1, F, ldf, ipiv, x, 1));
                return launch_refine_scale<T>(h, n, wt, x);
            };
            double est = 0.0;
            bool bad = false;
            typedef RealElem<T> E;
            RFLU_TRY(higham_estimate(
                n, true, [&](int mode, int64_t j) { return launch_cond_fill<E>(h, n, x, mode, j); }, apply,
                [&](int64_t jq, int write, CondStats* st) { return launch_cond_stats<E>(h, n, x, sgn, jq, write, st); }, &est, &bad));
            if (bad) ferr[k0 + k] = HUGE_VAL;
            else ferr[k0 + k] = xmax[k] != 0.0 ? est / xmax[k] : est;
        }
    }
    RFLU_HIP(hipStreamSynchronize(h->stream));
    return RFLU_OK;
}

// ---- what the other host sources call (driver.hpp) -------------------------------------------------------------------------------------
#define RFLU_INSTANTIATE_DRIVER(T)                                                                                                   \
    template int trsm_rec<T>(Handle*, int64_t, int64_t, const T*, int64_t, T*, int64_t, const T*);                                    \
    template int trsm_public<T>(Handle*, int64_t, int64_t, const T*, int64_t, T*, int64_t);                                           \
    template int getrs_cm_dev<T>(Handle*, int64_t, int64_t, const T*, int64_t, const int64_t*, T*, int64_t);                          \
    template int getrs_trans_cm_dev<T>(Handle*, int64_t, int64_t, const T*, int64_t, const int64_t*, T*, int64_t);                    \
    template int getri_cm_dev<RealElem<T>>(Handle*, int64_t, T*, int64_t, const int64_t*, int64_t*);                                  \
    template int getri_cm_dev<CplxElem<T>>(Handle*, int64_t, T*, int64_t, const int64_t*, int64_t*);                                  \
    template int gecon_dev<T>(Handle*, int, int64_t, const T*, int64_t, int, double, double*);
RFLU_INSTANTIATE_DRIVER(double)
RFLU_INSTANTIATE_DRIVER(float)

}  // namespace rflu

using namespace rflu;

static Handle* H(rflu_handle_t h) { return reinterpret_cast<Handle*>(h); }

// CHECK_HANDLE declares the guard object in the enclosing scope: it must be the FIRST statement of a function body (not the
// body of an unbraced if / else, not twice in one scope).
#define CHECK_HANDLE(h)                                  \
    if ((h) == nullptr) {                                \
        set_error("null handle");                        \
        return RFLU_ERR_ARG;                             \
    }                                                    \
    DeviceGuard device_guard__(H(h)->device);            \
    RFLU_HIP(device_guard__.err)

extern "C" {

int rflu_version(void) { return 111; }

const char* rflu_last_error(void) { return g_err; }

int rflu_create(rflu_handle_t* handle, int device)
{
    if (handle == nullptr) { set_error("null handle pointer"); return RFLU_ERR_ARG; }
    *handle = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        set_error("no HIP device visible (this library has no CPU fallback)");
        return RFLU_ERR_NODEVICE;
    }
    if (device < 0 || device >= ndev) { set_error("device %d out of range (0..%d)", device, ndev - 1); return RFLU_ERR_ARG; }
    DeviceGuard device_guard__(device);
    RFLU_HIP(device_guard__.err);
    hipDeviceProp_t prop;
    RFLU_HIP(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_error("device %d is %s; librflu is built for gfx950 (MI355X) only", device, prop.gcnArchName);
        return RFLU_ERR_NODEVICE;
    }
    Handle* h = new (std::nothrow) Handle();
    if (!h) { set_error("out of host memory"); return RFLU_ERR_ARG; }
    h->device = device;
    h->num_cus = prop.multiProcessorCount;
    // a BLOCKING stream: it orders itself against the legacy default stream, so buffers produced by a framework on
    // stream 0 (PyTorch's default) need no extra synchronisation before/after a call
    {
        // highest priority: in the lookahead driver this stream carries the critical path (panels + next block column)
        // and competes for CUs with the bulk trailing update on the second stream
        int lo = 0, hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
#ifdef RFLU_EXPERIMENTS
        if (env_str("RFLU_NO_PRIORITY")) hi = 0;
#endif
        RFLU_HIP(hipStreamCreateWithPriority(&h->own_stream, hipStreamDefault, hi));
    }
    h->stream = h->own_stream;
    RFLU_HIP(hipMalloc((void**)&h->info_dev, 2 * sizeof(int64_t)));
    if (const char* e = env_str("RFLU_DUMMY_QUEUES")) {
        // measurement / test hook (scripts/queue_collision.py, tests/test_gpu_queues.py): k extra streams created AND USED here,
        // before the update / side streams exist, so that those get other queue indices -- and with them other hardware pipes -- than
        // in a fresh process.  Without validate_queues (RFLU_QUEUE_CHECK=0): N=16384 80 ms or 108-113 ms depending on k.
        for (int i = 0; i < atoi(e); ++i) {
            hipStream_t d;
            RFLU_HIP(hipStreamCreateWithFlags(&d, hipStreamNonBlocking));
            RFLU_HIP(hipMemsetAsync(h->info_dev, 0, 8, d));
            RFLU_HIP(hipStreamSynchronize(d));
        }
    }
    RFLU_HIP(hipMalloc((void**)&h->gates, 8 * sizeof(unsigned long long)));
    RFLU_HIP(hipMemset(h->gates, 0, 8 * sizeof(unsigned long long)));
    for (int i = 0; i < 3; ++i) h->gate_ptr[i] = h->gates + i;
    RFLU_HIP(hipHostMalloc((void**)&h->info_pinned, 2 * sizeof(int64_t)));
    h->pscratch_bytes = panel_scratch_bytes();
    RFLU_HIP(hipMalloc((void**)&h->pscratch, h->pscratch_bytes));
    RFLU_HIP(hipMemset(h->pscratch, 0, h->pscratch_bytes));
    RFLU_HIP(hipEventCreate(&h->ev0));
    RFLU_HIP(hipEventCreate(&h->ev1));
    // the cooperative kernels spin on peer workgroups: all of a launch's workgroups must be resident at once.  Ask the
    // runtime how many fit (one 512/576-thread workgroup per CU with these register counts) instead of assuming it.
    h->panel_max_wgs = panel_resident_limit(h->num_cus);
    if (h->panel_max_wgs <= 0) { set_error("occupancy query for the cooperative panel kernels failed"); delete h; return RFLU_ERR_HIP; }
    load_handle_env(h);
    *handle = reinterpret_cast<rflu_handle_t>(h);
    return RFLU_OK;
}

int rflu_destroy(rflu_handle_t handle)
{
    if (!handle) return RFLU_OK;
    Handle* h = H(handle);
    DeviceGuard device_guard__(h->device);
    (void)hipStreamSynchronize(h->stream);
    if (h->work) (void)hipFree(h->work);
    if (h->ipiv_dev) (void)hipFree(h->ipiv_dev);
    if (h->hostA_dev) (void)hipFree(h->hostA_dev);
    if (h->out_stage) (void)hipFree(h->out_stage);
    if (h->rhs_work) (void)hipFree(h->rhs_work);
    if (h->hostB_dev) (void)hipFree(h->hostB_dev);
    if (h->mixed_rhs) (void)hipFree(h->mixed_rhs);
    if (h->mixed_r) (void)hipFree(h->mixed_r);
    if (h->mixed_part) (void)hipFree(h->mixed_part);
    if (h->mixed_norms) (void)hipFree(h->mixed_norms);
    if (h->mixed_norms_host) (void)hipHostFree(h->mixed_norms_host);
    if (h->inv_work) (void)hipFree(h->inv_work);
    if (h->inv_part) (void)hipFree(h->inv_part);
    if (h->cond_work) (void)hipFree(h->cond_work);
    if (h->pm_cnt) (void)hipFree(h->pm_cnt);
    if (h->pm_dst) (void)hipFree(h->pm_dst);
    if (h->pm_src) (void)hipFree(h->pm_src);
    if (h->linv) (void)hipFree(h->linv);
    if (h->linv_tmp) (void)hipFree(h->linv_tmp);
    if (h->pscratch) (void)hipFree(h->pscratch);
    if (h->info_dev) (void)hipFree(h->info_dev);
    if (h->gates) (void)hipFree(h->gates);
    if (h->tail_event_obj) (void)hipEventDestroy(h->tail_event_obj);
    if (h->tail_fork_obj) (void)hipEventDestroy(h->tail_fork_obj);
    if (h->gate_stamps) (void)hipFree(h->gate_stamps);
    if (h->eng_state) (void)hipFree(h->eng_state);
    if (h->eng_host) (void)hipHostFree(h->eng_host);
    if (h->eng_rows_final) (void)hipHostFree(h->eng_rows_final);
    if (h->eng_trace_buf) (void)hipFree(h->eng_trace_buf);
    if (h->info_pinned) (void)hipHostFree(h->info_pinned);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    for (hipEvent_t e : h->out_events) (void)hipEventDestroy(e);
    for (void* b : h->bounce) if (b) (void)hipHostFree(b);
    for (hipStream_t ps : h->parked_streams)
        if (ps) (void)hipStreamDestroy(ps);
    if (h->qprobe_slots) (void)hipFree(h->qprobe_slots);
    for (hipStream_t us : h->ustreams)
        if (us) (void)hipStreamDestroy(us);
    for (hipStream_t ps : h->pstreams)
        if (ps) (void)hipStreamDestroy(ps);
    for (hipEvent_t e : h->events) (void)hipEventDestroy(e);
    for (auto& r : h->async_recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    for (hipEvent_t e : h->async_pool) (void)hipEventDestroy(e);
    if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
    delete h;
    return RFLU_OK;
}

int rflu_set_stream(rflu_handle_t handle, void* hip_stream)
{
    CHECK_HANDLE(handle);
    H(handle)->stream = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : H(handle)->own_stream;
    return RFLU_OK;
}

int rflu_synchronize(rflu_handle_t handle)
{
    CHECK_HANDLE(handle);
    RFLU_HIP(hipStreamSynchronize(H(handle)->stream));
    return RFLU_OK;
}

int rflu_reload_tuning(rflu_handle_t handle)
{
    if (!handle) { set_error("null handle"); return RFLU_ERR_ARG; }
    load_handle_env(H(handle));
    return RFLU_OK;
}

int rflu_last_path(rflu_handle_t handle) { return handle ? H(handle)->last_path : RFLU_PATH_NONE; }

int rflu_update_stream(rflu_handle_t handle, void** hip_stream_out)
{
    CHECK_HANDLE(handle);
    if (hip_stream_out == nullptr) { set_error("null output pointer"); return RFLU_ERR_ARG; }
    hipStream_t us;
    RFLU_TRY(get_ustream(H(handle), 32, &us));
    *hip_stream_out = reinterpret_cast<void*>(us);
    return RFLU_OK;
}

// measurement only (scripts/microbench_*): `usec` of register-only MFMA load on the CU-masked update stream, asynchronously
// measurement only: copy the RFLU_GATE_TRACE stamps (3 x 4096 wall-clock ticks, 100 MHz) to the host
int rflu_debug_gate_stamps(rflu_handle_t handle, long long* out)
{
    CHECK_HANDLE(handle);
    if (!H(handle)->gate_stamps) { set_error("no gate trace (set RFLU_GATE_TRACE=1)"); return RFLU_ERR_ARG; }
    RFLU_HIP(hipMemcpy(out, H(handle)->gate_stamps, 3 * 4096 * sizeof(long long), hipMemcpyDeviceToHost));
    return RFLU_OK;
}

int rflu_debug_engine_acct(rflu_handle_t handle, long long* out8)
{
    // RFLU_ENGINE_TRACE: the workgroup-time accumulators of the LAST engine launch on this handle (100 MHz ticks, summed over the
    // workgroups): [0] block-column tiles, [1] leaf-window tiles, [2] strips + solves, [3] deferred interchanges, [4] between units,
    // [5] (of 4) asleep, [6] (of 4) publications, [7] unused
    if (!handle || !out8) return RFLU_ERR_ARG;
    Handle* h = H(handle);
    DeviceGuard device_guard__(h->device);
    for (int i = 0; i < 8; ++i) out8[i] = 0;
    if (!h->eng_trace_buf) return RFLU_OK;
    RFLU_HIP(hipStreamSynchronize(h->stream));
    RFLU_HIP(hipMemcpy(out8, h->eng_trace_buf + 4096 * 4, 8 * sizeof(long long), hipMemcpyDeviceToHost));   // (the finer split behind them: engine_trace_report, schedule.cpp)
    return RFLU_OK;
}

int rflu_debug_heat(rflu_handle_t handle, double usec)
{
    CHECK_HANDLE(handle);
    Handle* h = H(handle);
    hipStream_t us;
    RFLU_TRY(get_ustream(h, 32, &us));
    OnStream on(h, us);
    return launch_heat(h, 224, usec);
}

#define DEFINE_TYPED(SFX, T)                                                                                          \
    int rflu_getrf_##SFX(rflu_handle_t handle, int64_t m, int64_t n, T* A, int64_t lda, int64_t* ipiv, int pivot,     \
                         int64_t blocksize, int64_t* info)                                                            \
    {                                                                                                                 \
        CHECK_HANDLE(handle);                                                                                         \
        return getrf_host<T>(H(handle), m, n, A, lda, ipiv, pivot, blocksize, info);                                  \
    }                                                                                                                 \
    int rflu_getrf_##SFX##_dev(rflu_handle_t handle, int64_t m, int64_t n, T* A, int64_t lda, int64_t* ipiv,          \
                               int pivot, int64_t blocksize, int64_t* info)                                           \
    {                                                                                                                 \
        CHECK_HANDLE(handle);                                                                                         \
        return getrf_cm_dev<T>(H(handle), m, n, A, lda, ipiv, pivot, blocksize, info);                                \
    }                                                                                                                 \
    int rflu_getrf_rm_##SFX##_dev(rflu_handle_t handle, int64_t m, int64_t n, T* R, int64_t ld, int64_t* ipiv,        \
                                  int pivot, int64_t blocksize, int64_t* info)                                        \
    {                                                                                                                 \
        CHECK_HANDLE(handle);                                                                                         \
        if (info == nullptr) { set_error("null info"); return RFLU_ERR_ARG; }                                         \
        return getrf_rm<T>(H(handle), m, n, R, ld, ipiv, pivot, blocksize, info);                                     \
    }                                                                                                                 \
    int rflu_panel_rm_##SFX##_dev(rflu_handle_t handle, int64_t m, int64_t r0, int64_t c0, int64_t w, T* R,           \
                                  int64_t ld, int64_t* ipiv, int pivot, int64_t* info)                                \
    {                                                                                                                 \
        CHECK_HANDLE(handle);                                                                                         \
        return panel_rm<T>(H(handle), m, r0, c0, w, R, ld, ipiv, pivot, info);                                        \
    }                                                                                                                 \
    int rflu_laswp_rm_##SFX##_dev(rflu_handle_t handle, T* R, int64_t ld, int64_t m, int64_t c0, int64_t ncols,       \
                                  const int64_t* ipiv, int64_t k0, int64_t k1)                                        \
    {                                                                                                                 \
        CHECK_HANDLE(handle);                                                                                         \
        return laswp_rm<T>(H(handle), R, ld, m, c0, ncols, ipiv, k0, k1);                                             \
    }                                                                                                                 \
    int rflu_trsm_rm_##SFX##_dev(rflu_handle_t handle, int64_t n, int64_t nrhs, const T* L, int64_t ldl, T* B,        \
                                 int64_t ldb)                                                                         \
    {                                                                                                                 \
        CHECK_HANDLE(handle);                                                                                         \
        return trsm_public<T>(H(handle), n, nrhs, L, ldl, B, ldb);                                                       \
    }                                                                                                                 \
    int rflu_gemm_rm_##SFX##_dev(rflu_handle_t handle, int64_t M, int64_t N, int64_t K, const T* A, int64_t lda,      \
                                 const T* B, int64_t ldb, T* C, int64_t ldc)                                          \
    {                                                                                                                 \
        CHECK_HANDLE(handle);                                                                                         \
        return gemm_public<T>(H(handle), M, N, K, A, lda, B, ldb, C, ldc);                                            \
    }                                                                                                                 \
    int rflu_cm_to_rm_##SFX##_dev(rflu_handle_t handle, int64_t m, int64_t n, const T* A, int64_t lda, T* R,          \
                                  int64_t ldr)                                                                        \
    {                                                                                                                 \
        CHECK_HANDLE(handle);                                                                                         \
        return launch_transpose<T>(H(handle), m, n, A, lda, R, ldr);                                                  \
    }                                                                                                                 \
    int rflu_rm_to_cm_##SFX##_dev(rflu_handle_t handle, int64_t m, int64_t n, const T* R, int64_t ldr, T* A,          \
                                  int64_t lda)                                                                        \
    {                                                                                                                 \
        CHECK_HANDLE(handle);                                                                                         \
        return launch_transpose<T>(H(handle), n, m, R, ldr, A, lda);                                                  \
    }                                                                                                                 \
    int rflu_getrs_##SFX(rflu_handle_t handle, int64_t n, int64_t nrhs, const T* F, int64_t lda, const int64_t* ipiv,  \
                         T* B, int64_t ldb)                                                                           \
    {                                                                                                                 \
        CHECK_HANDLE(handle);                                                                                         \
        return getrs_host<T>(H(handle), n, nrhs, F, lda, ipiv, B, ldb, false);                                        \
    }                                                                                                                 \
    int rflu_getrs_##SFX##_dev(rflu_handle_t handle, int64_t n, int64_t nrhs, const T* F, int64_t lda,                \
                               const int64_t* ipiv, T* B, int64_t ldb)                                                \
    {                                                                                                                 \
        CHECK_HANDLE(handle);                                                                                         \
        return getrs_cm_dev<T>(H(handle), n, nrhs, F, lda, ipiv, B, ldb);                                             \
    }                                                                                                                 \
    int rflu_getrs_rm_##SFX##_dev(rflu_handle_t handle, int64_t n, int64_t nrhs, const T* R, int64_t ld,              \
                                  const int64_t* ipiv, T* B, int64_t ldb)                                             \
    {                                                                                                                 \
        CHECK_HANDLE(handle);                                                                                         \
        RFLU_TRY(getrs_rm<T>(H(handle), n, nrhs, R, ld, ipiv, B, ldb));                                               \
        RFLU_HIP(hipStreamSynchronize(H(handle)->stream));                                                            \
        return RFLU_OK;                                                                                               \
    }                                                                                                                 \
    int rflu_getrs_trans_##SFX(rflu_handle_t handle, int64_t n, int64_t nrhs, const T* F, int64_t lda,                \
                               const int64_t* ipiv, T* B, int64_t ldb)                                                \
    {                                                                                                                 \
        CHECK_HANDLE(handle);                                                                                         \
        return getrs_host<T>(H(handle), n, nrhs, F, lda, ipiv, B, ldb, true);                                         \
    }                                                                                                                 \
    int rflu_getrs_trans_##SFX##_dev(rflu_handle_t handle, int64_t n, int64_t nrhs, const T* F, int64_t lda,          \
                                     const int64_t* ipiv, T* B, int64_t ldb)                                          \
    {                                                                                                                 \
        CHECK_HANDLE(handle);                                                                                         \
        return getrs_trans_cm_dev<T>(H(handle), n, nrhs, F, lda, ipiv, B, ldb);                                       \
    }                                                                                                                 \
    int rflu_getrs_trans_rm_##SFX##_dev(rflu_handle_t handle, int64_t n, int64_t nrhs, const T* R, int64_t ld,        \
                                        const int64_t* ipiv, T* B, int64_t ldb)                                       \
    {                                                                                                                 \
        CHECK_HANDLE(handle);                                                                                         \
        return getrs_trans_rm<T>(H(handle), n, nrhs, R, ld, ipiv, B, ldb);                                            \
    }                                                                                                                 \
    int rflu_butterfly_mul_##SFX##_dev(rflu_handle_t handle, int64_t n, T* A, int64_t lda, const T* uv)               \
    {                                                                                                                 \
        CHECK_HANDLE(handle);                                                                                         \
        if (n > 0 && (A == nullptr || uv == nullptr)) { set_error("butterfly: null pointer"); return RFLU_ERR_ARG; }  \
        return launch_butterfly_mul<T>(H(handle), n, A, lda, uv);                                                     \
    }                                                                                                                 \
    int rflu_butterfly_vec_##SFX##_dev(rflu_handle_t handle, int64_t n, int64_t nrhs, T* X, int64_t ldx, const T* uv, \
                                       int transpose_u)                                                               \
    {                                                                                                                 \
        CHECK_HANDLE(handle);                                                                                         \
        if (n > 0 && nrhs > 0 && (X == nullptr || uv == nullptr)) { set_error("butterfly: null pointer"); return RFLU_ERR_ARG; } \
        return launch_butterfly_vec<T>(H(handle), n, nrhs, X, ldx, uv, transpose_u ? 0 : 1);                          \
    }                                                                                                                 \
    int rflu_getrf_batched_##SFX##_dev(rflu_handle_t handle, int64_t batch, int64_t m, int64_t n, T* A, int64_t lda,  \
                                       int64_t strideA, int row_major, int64_t* ipiv, int64_t stride_ipiv, int pivot,  \
                                       int64_t* info_dev)                                                              \
    {                                                                                                                 \
        CHECK_HANDLE(handle);                                                                                         \
        return getrf_batched<T>(H(handle), batch, m, n, A, lda, strideA, row_major, ipiv, stride_ipiv, pivot, info_dev); \
    }                                                                                                                 \
    int rflu_getrs_batched_##SFX##_dev(rflu_handle_t handle, int64_t batch, int64_t n, int64_t nrhs, const T* F,      \
                                       int64_t lda, int64_t strideF, int row_major, const int64_t* ipiv,              \
                                       int64_t stride_ipiv, T* B, int64_t ldb, int64_t strideB, int trans)            \
    {                                                                                                                 \
        CHECK_HANDLE(handle);                                                                                         \
        return getrs_batched<T>(H(handle), batch, n, nrhs, F, lda, strideF, row_major, ipiv, stride_ipiv, B, ldb,     \
                                strideB, trans);                                                                      \
    }                                                                                                                 \
    int rflu_logabsdet_##SFX##_dev(rflu_handle_t handle, int64_t n, const T* F, int64_t ld, const int64_t* ipiv,       \
                                   double* logabs_out, double* sign_out)                                              \
    {                                                                                                                 \
        CHECK_HANDLE(handle);                                                                                         \
        return logabsdet_dev<RealElem<T>>(H(handle), n, F, ld, ipiv, logabs_out, sign_out, nullptr);                  \
    }                                                                                                                 \
    int rflu_logabsdet_##SFX(rflu_handle_t handle, int64_t n, const T* F, int64_t ld, const int64_t* ipiv,             \
                             double* logabs_out, double* sign_out)                                                    \
    {                                                                                                                 \
        CHECK_HANDLE(handle);                                                                                         \
        return logabsdet_host<RealElem<T>>(H(handle), n, F, ld, ipiv, logabs_out, sign_out, nullptr);                 \
    }                                                                                                                 \
    int rflu_logabsdet_batched_##SFX##_dev(rflu_handle_t handle, int64_t batch, int64_t n, const T* F, int64_t lda,   \
                                           int64_t strideF, const int64_t* ipiv, int64_t stride_ipiv,                 \
                                           double* logabs_dev, double* sign_dev)                                      \
    {                                                                                                                 \
        CHECK_HANDLE(handle);                                                                                         \
        return logabsdet_batched<RealElem<T>>(H(handle), batch, n, F, lda, strideF, ipiv, stride_ipiv, logabs_dev,    \
                                              sign_dev);                                                          \
    }                                                                                                                 \
    int rflu_getri_##SFX##_dev(rflu_handle_t handle, int64_t n, T* F, int64_t lda, const int64_t* ipiv, int64_t* info) \
    {                                                                                                                 \
        CHECK_HANDLE(handle);                                                                                         \
        return getri_cm_dev<RealElem<T>>(H(handle), n, F, lda, ipiv, info);                                           \
    }                                                                                                                 \
    int rflu_getri_rm_##SFX##_dev(rflu_handle_t handle, int64_t n, T* R, int64_t ld, const int64_t* ipiv,             \
                                  int64_t* info)                                                                      \
    {                                                                                                                 \
        CHECK_HANDLE(handle);                                                                                         \
        return getri_rm<T>(H(handle), n, R, ld, ipiv, info);                                                          \
    }                                                                                                                 \
    int rflu_getri_##SFX(rflu_handle_t handle, int64_t n, T* F, int64_t lda, const int64_t* ipiv, int64_t* info)      \
    {                                                                                                                 \
        CHECK_HANDLE(handle);                                                                                         \
        return getri_host<RealElem<T>>(H(handle), n, F, lda, ipiv, info);                                             \
    }                                                                                                                 \
    int rflu_getri_batched_##SFX##_dev(rflu_handle_t handle, int64_t batch, int64_t n, const T* F, int64_t lda,       \
                                       int64_t strideF, int row_major, const int64_t* ipiv, int64_t stride_ipiv,      \
                                       T* Ainv, int64_t ldi, int64_t strideI, int64_t* info_dev)                      \
    {                                                                                                                 \
        CHECK_HANDLE(handle);                                                                                         \
        return getri_batched<RealElem<T>>(H(handle), batch, n, F, lda, strideF, row_major, ipiv, stride_ipiv, Ainv,   \
                                          ldi, strideI, 0, info_dev);                                                 \
    }                                                                                                                 \
    int rflu_lange_##SFX##_dev(rflu_handle_t handle, int norm, int64_t m, int64_t n, const T* A, int64_t lda,          \
                               int row_major, double* out)                                                            \
    {                                                                                                                 \
        CHECK_HANDLE(handle);                                                                                         \
        return lange_dev<RealElem<T>>(H(handle), norm, m, n, A, lda, row_major, out);                                 \
    }                                                                                                                 \
    int rflu_lange_batched_##SFX##_dev(rflu_handle_t handle, int norm, int64_t batch, int64_t m, int64_t n,           \
                                       const T* A, int64_t lda, int64_t strideA, int row_major, double* out_dev)      \
    {                                                                                                                 \
        CHECK_HANDLE(handle);                                                                                         \
        return lange_batched<RealElem<T>>(H(handle), norm, batch, m, n, A, lda, strideA, row_major, out_dev);         \
    }                                                                                                                 \
    int rflu_gecon_##SFX##_dev(rflu_handle_t handle, int norm, int64_t n, const T* F, int64_t lda, double anorm,      \
                               double* rcond_out)                                                                     \
    {                                                                                                                 \
        CHECK_HANDLE(handle);                                                                                         \
        return gecon_dev<T>(H(handle), norm, n, F, lda, 0, anorm, rcond_out);                                         \
    }                                                                                                                 \
    int rflu_gecon_rm_##SFX##_dev(rflu_handle_t handle, int norm, int64_t n, const T* R, int64_t ld, double anorm,    \
                                  double* rcond_out)                                                                  \
    {                                                                                                                 \
        CHECK_HANDLE(handle);                                                                                         \
        return gecon_dev<T>(H(handle), norm, n, R, ld, 1, anorm, rcond_out);                                          \
    }                                                                                                                 \
    int rflu_gecon_##SFX(rflu_handle_t handle, int norm, int64_t n, const T* F, int64_t lda, double anorm,            \
                         double* rcond_out)                                                                           \
    {                                                                                                                 \
        CHECK_HANDLE(handle);                                                                                         \
        return gecon_host<T>(H(handle), norm, n, F, lda, anorm, rcond_out);                                           \
    }                                                                                                                 \
    int rflu_gecon_batched_##SFX##_dev(rflu_handle_t handle, int norm, int64_t batch, int64_t n, const T* F,          \
                                       int64_t lda, int64_t strideF, int row_major, const double* anorm_dev,          \
                                       double* rcond_dev)                                                             \
    {                                                                                                                 \
        CHECK_HANDLE(handle);                                                                                         \
        return gecon_batched<RealElem<T>>(H(handle), norm, batch, n, F, lda, strideF, row_major, anorm_dev,           \
                                          rcond_dev);                                                                 \
    }                                                                                                                 \
    int rflu_gerfs_##SFX##_dev(rflu_handle_t handle, int64_t n, int64_t nrhs, const T* A, int64_t lda, const T* F,    \
                               int64_t ldf, const int64_t* ipiv, const T* B, int64_t ldb, T* X, int64_t ldx,          \
                               double* ferr, double* berr, int max_iter, int* steps, int64_t* info)                   \
    {                                                                                                                 \
        CHECK_HANDLE(handle);                                                                                         \
        return gerfs_dev<T>(H(handle), n, nrhs, A, lda, F, ldf, ipiv, B, ldb, X, ldx, ferr, berr, max_iter, steps,    \
                            info);                                                                                    \
    }                                                                                                                 \
    int rflu_berr_##SFX##_dev(rflu_handle_t handle, int64_t n, int64_t nrhs, const T* A, int64_t lda, const T* X,     \
                              int64_t ldx, const T* B, int64_t ldb, double* berr)                                     \
    {                                                                                                                 \
        CHECK_HANDLE(handle);                                                                                         \
        return berr_dev<T>(H(handle), n, nrhs, A, lda, X, ldx, B, ldb, berr);                                         \
    }                                                                                                                 \
    int rflu_fill_uniform_##SFX##_dev(rflu_handle_t handle, T* A, int64_t m, int64_t n, int64_t ld, int row_major,    \
                                      uint64_t seed, int64_t M_global, int64_t i0, int64_t j0, double diag_add)       \
    {                                                                                                                 \
        CHECK_HANDLE(handle);                                                                                         \
        return launch_fill_uniform<T>(H(handle), A, m, n, ld, row_major, seed, M_global, i0, j0, diag_add);           \
    }

DEFINE_TYPED(f64, double)
DEFINE_TYPED(f32, float)

int rflu_mixed_getrf_f64_dev(rflu_handle_t handle, int64_t n, const double* A_dev, int64_t lda, float* F32_dev, int64_t ldf,
                             int64_t* ipiv_dev, int pivot, int64_t blocksize, double* anorm_out, int64_t* info)
{
    CHECK_HANDLE(handle);
    Handle* h = H(handle);
    return mixed_getrf<RealElem<double>>(h, n, A_dev, lda, F32_dev, ldf, ipiv_dev, pivot, anorm_out, info, [&](int64_t* inf) {
        return getrf_rm<float>(h, n, n, F32_dev, ldf, ipiv_dev, pivot, blocksize, inf);
    });
}

int rflu_mixed_getrs_f64_dev(rflu_handle_t handle, int64_t n, int64_t nrhs, const double* A_dev, int64_t lda, const float* F32_dev,
                             int64_t ldf, const int64_t* ipiv_dev, double anorm, const double* B_dev, int64_t ldb, double* X_dev,
                             int64_t ldx, int max_iter, int* iters)
{
    CHECK_HANDLE(handle);
    return mixed_getrs(H(handle), n, nrhs, A_dev, lda, F32_dev, ldf, ipiv_dev, anorm, B_dev, ldb, X_dev, ldx, max_iter, iters);
}

int rflu_residual_f64_dev(rflu_handle_t handle, int64_t n, int64_t nrhs, const double* A_dev, int64_t lda, const double* X_dev,
                          int64_t ldx, const double* B_dev, int64_t ldb, double* R_dev, int64_t ldr)
{
    CHECK_HANDLE(handle);
    return residual_public<RealElem<double>>(H(handle), n, nrhs, A_dev, lda, X_dev, ldx, B_dev, ldb, R_dev, ldr);
}

/* experiment hook (not in rflu.h): a stream restricted to an arbitrary CU mask (8 x 32 bits); the caller owns it */
int rflu_debug_masked_stream(rflu_handle_t handle, const unsigned* mask8, void** stream_out)
{
    CHECK_HANDLE(handle);
    hipStream_t st = nullptr;
    RFLU_HIP(hipExtStreamCreateWithCUMask(&st, 8, mask8));
    *stream_out = reinterpret_cast<void*>(st);
    return RFLU_OK;
}

/* experiment hook (not in rflu.h): copy the RFLU_PANEL_TRACE clock stamps of the last panel launch to the host */
int rflu_debug_panel_trace(rflu_handle_t handle, long long* out512)
{
    CHECK_HANDLE(handle);
    Handle* h = H(handle);
    RFLU_HIP(hipStreamSynchronize(h->stream));
    RFLU_HIP(hipMemcpy(out512, (char*)h->pscratch + panel_trace_offset_bytes(), (8 * NB + 16) * sizeof(long long), hipMemcpyDeviceToHost));
    return RFLU_OK;
}

/* experiment hook (not in rflu.h): the all-workgroup wall-clock stamps of a -DRFLU_PANEL_TRACE_ALL build (0 words otherwise) */
int rflu_debug_panel_trace_all(rflu_handle_t handle, long long* out, long long max_words)
{
    CHECK_HANDLE(handle);
    Handle* h = H(handle);
    RFLU_HIP(hipStreamSynchronize(h->stream));
    const size_t nw = std::min<size_t>(panel_trace_all_words(), (size_t)std::max<long long>(max_words, 0));
    if (nw) RFLU_HIP(hipMemcpy(out, (char*)h->pscratch + panel_trace_all_offset_bytes(), nw * sizeof(long long), hipMemcpyDeviceToHost));
    return (int)nw;
}

// ComplexF64 / ComplexF32 (complex.hip, complex_gemm.hip): interleaved (re, im) pairs behind R*, leading dimensions in complex elements
#define DEFINE_COMPLEX(SFX, R)                                                                                        \
    int rflu_getrf_##SFX(rflu_handle_t handle, int64_t m, int64_t n, R* A, int64_t lda, int64_t* ipiv, int pivot,     \
                         int64_t* info)                                                                               \
    {                                                                                                                 \
        CHECK_HANDLE(handle);                                                                                         \
        return cgetrf_host<R>(H(handle), m, n, A, lda, ipiv, pivot, info);                                            \
    }                                                                                                                 \
    int rflu_getrf_##SFX##_dev(rflu_handle_t handle, int64_t m, int64_t n, R* A, int64_t lda, int64_t* ipiv,          \
                               int pivot, int64_t* info)                                                              \
    {                                                                                                                 \
        CHECK_HANDLE(handle);                                                                                         \
        return cgetrf_cm_dev<R>(H(handle), m, n, A, lda, ipiv, pivot, info);                                          \
    }                                                                                                                 \
    int rflu_getrs_##SFX(rflu_handle_t handle, int64_t n, int64_t nrhs, const R* F, int64_t lda, const int64_t* ipiv, \
                         R* B, int64_t ldb)                                                                           \
    {                                                                                                                 \
        CHECK_HANDLE(handle);                                                                                         \
        return cgetrs_host<R>(H(handle), n, nrhs, F, lda, ipiv, B, ldb);                                              \
    }                                                                                                                 \
    int rflu_getrs_##SFX##_dev(rflu_handle_t handle, int64_t n, int64_t nrhs, const R* F, int64_t lda,                \
                               const int64_t* ipiv, R* B, int64_t ldb)                                                \
    {                                                                                                                 \
        CHECK_HANDLE(handle);                                                                                         \
        return cgetrs_cm_dev<R>(H(handle), n, nrhs, F, lda, ipiv, B, ldb);                                            \
    }                                                                                                                 \
    int rflu_getrs_trans_##SFX(rflu_handle_t handle, int64_t n, int64_t nrhs, const R* F, int64_t lda,                \
                               const int64_t* ipiv, R* B, int64_t ldb, int conj)                                      \
    {                                                                                                                 \
        CHECK_HANDLE(handle);                                                                                         \
        return cgetrs_trans_host<R>(H(handle), n, nrhs, F, lda, ipiv, B, ldb, conj);                                  \
    }                                                                                                                 \
    int rflu_getrs_trans_##SFX##_dev(rflu_handle_t handle, int64_t n, int64_t nrhs, const R* F, int64_t lda,          \
                                     const int64_t* ipiv, R* B, int64_t ldb, int conj)                                \
    {                                                                                                                 \
        CHECK_HANDLE(handle);                                                                                         \
        return cgetrs_trans_cm_dev<R>(H(handle), n, nrhs, F, lda, ipiv, B, ldb, conj);                                \
    }                                                                                                                 \
    int rflu_gemm_rm_##SFX##_dev(rflu_handle_t handle, int64_t M, int64_t N, int64_t K, const R* A, int64_t lda,      \
                                 const R* B, int64_t ldb, R* C, int64_t ldc)                                          \
    {                                                                                                                 \
        CHECK_HANDLE(handle);                                                                                         \
        return cgemm_public<R>(H(handle), M, N, K, A, lda, B, ldb, C, ldc);                                           \
    }                                                                                                                 \
    int rflu_getrf_batched_##SFX##_dev(rflu_handle_t handle, int64_t batch, int64_t m, int64_t n, R* A, int64_t lda,  \
                                       int64_t strideA, int row_major, int64_t* ipiv, int64_t stride_ipiv, int pivot,  \
                                       int64_t* info_dev)                                                              \
    {                                                                                                                 \
        CHECK_HANDLE(handle);                                                                                         \
        return cgetrf_batched<R>(H(handle), batch, m, n, A, lda, strideA, row_major, ipiv, stride_ipiv, pivot, info_dev); \
    }                                                                                                                 \
    int rflu_getrs_batched_##SFX##_dev(rflu_handle_t handle, int64_t batch, int64_t n, int64_t nrhs, const R* F,      \
                                       int64_t lda, int64_t strideF, int row_major, const int64_t* ipiv,              \
                                       int64_t stride_ipiv, R* B, int64_t ldb, int64_t strideB, int trans)            \
    {                                                                                                                 \
        CHECK_HANDLE(handle);                                                                                         \
        return cgetrs_batched<R>(H(handle), batch, n, nrhs, F, lda, strideF, row_major, ipiv, stride_ipiv, B, ldb,    \
                                 strideB, trans);                                                                     \
    }                                                                                                                 \
    int rflu_getri_##SFX##_dev(rflu_handle_t handle, int64_t n, R* F, int64_t lda, const int64_t* ipiv, int64_t* info) \
    {                                                                                                                 \
        CHECK_HANDLE(handle);                                                                                         \
        return getri_cm_dev<CplxElem<R>>(H(handle), n, F, lda, ipiv, info);                                           \
    }                                                                                                                 \
    int rflu_getri_##SFX(rflu_handle_t handle, int64_t n, R* F, int64_t lda, const int64_t* ipiv, int64_t* info)      \
    {                                                                                                                 \
        CHECK_HANDLE(handle);                                                                                         \
        return getri_host<CplxElem<R>>(H(handle), n, F, lda, ipiv, info);                                             \
    }                                                                                                                 \
    int rflu_getri_batched_##SFX##_dev(rflu_handle_t handle, int64_t batch, int64_t n, const R* F, int64_t lda,       \
                                       int64_t strideF, int row_major, const int64_t* ipiv, int64_t stride_ipiv,      \
                                       R* Ainv, int64_t ldi, int64_t strideI, int trans, int64_t* info_dev)           \
    {                                                                                                                 \
        CHECK_HANDLE(handle);                                                                                         \
        return getri_batched<CplxElem<R>>(H(handle), batch, n, F, lda, strideF, row_major, ipiv, stride_ipiv, Ainv,   \
                                          ldi, strideI, trans, info_dev);                                             \
    }                                                                                                                 \
    int rflu_logabsdet_##SFX##_dev(rflu_handle_t handle, int64_t n, const R* F, int64_t ld, const int64_t* ipiv,      \
                                   double* logabs_out, double* sign_re_out, double* sign_im_out)                      \
    {                                                                                                                 \
        CHECK_HANDLE(handle);                                                                                         \
        return logabsdet_dev<CplxElem<R>>(H(handle), n, F, ld, ipiv, logabs_out, sign_re_out, sign_im_out);           \
    }                                                                                                                 \
    int rflu_logabsdet_##SFX(rflu_handle_t handle, int64_t n, const R* F, int64_t ld, const int64_t* ipiv,            \
                             double* logabs_out, double* sign_re_out, double* sign_im_out)                            \
    {                                                                                                                 \
        CHECK_HANDLE(handle);                                                                                         \
        return logabsdet_host<CplxElem<R>>(H(handle), n, F, ld, ipiv, logabs_out, sign_re_out, sign_im_out);          \
    }                                                                                                                 \
    int rflu_logabsdet_batched_##SFX##_dev(rflu_handle_t handle, int64_t batch, int64_t n, const R* F, int64_t lda,   \
                                           int64_t strideF, const int64_t* ipiv, int64_t stride_ipiv,                 \
                                           double* logabs_dev, double* sign_dev)                                      \
    {                                                                                                                 \
        CHECK_HANDLE(handle);                                                                                         \
        return logabsdet_batched<CplxElem<R>>(H(handle), batch, n, F, lda, strideF, ipiv, stride_ipiv, logabs_dev,    \
                                              sign_dev);                                                              \
    }                                                                                                                 \
    int rflu_lange_##SFX##_dev(rflu_handle_t handle, int norm, int64_t m, int64_t n, const R* A, int64_t lda,          \
                               int row_major, double* out)                                                            \
    {                                                                                                                 \
        CHECK_HANDLE(handle);                                                                                         \
        return lange_dev<CplxElem<R>>(H(handle), norm, m, n, A, lda, row_major, out);                                 \
    }                                                                                                                 \
    int rflu_lange_batched_##SFX##_dev(rflu_handle_t handle, int norm, int64_t batch, int64_t m, int64_t n,           \
                                       const R* A, int64_t lda, int64_t strideA, int row_major, double* out_dev)      \
    {                                                                                                                 \
        CHECK_HANDLE(handle);                                                                                         \
        return lange_batched<CplxElem<R>>(H(handle), norm, batch, m, n, A, lda, strideA, row_major, out_dev);         \
    }                                                                                                                 \
    int rflu_gecon_##SFX##_dev(rflu_handle_t handle, int norm, int64_t n, const R* F, int64_t lda, double anorm,      \
                               double* rcond_out)                                                                     \
    {                                                                                                                 \
        CHECK_HANDLE(handle);                                                                                         \
        return cgecon_dev<R>(H(handle), norm, n, F, lda, anorm, rcond_out);                                           \
    }                                                                                                                 \
    int rflu_gecon_##SFX(rflu_handle_t handle, int norm, int64_t n, const R* F, int64_t lda, double anorm,            \
                         double* rcond_out)                                                                           \
    {                                                                                                                 \
        CHECK_HANDLE(handle);                                                                                         \
        return cgecon_host<R>(H(handle), norm, n, F, lda, anorm, rcond_out);                                          \
    }                                                                                                                 \
    int rflu_gecon_batched_##SFX##_dev(rflu_handle_t handle, int norm, int64_t batch, int64_t n, const R* F,          \
                                       int64_t lda, int64_t strideF, int row_major, const double* anorm_dev,          \
                                       double* rcond_dev)                                                             \
    {                                                                                                                 \
        CHECK_HANDLE(handle);                                                                                         \
        return gecon_batched<CplxElem<R>>(H(handle), norm, batch, n, F, lda, strideF, row_major, anorm_dev,           \
                                          rcond_dev);                                                                 \
    }
DEFINE_COMPLEX(cf64, double)
DEFINE_COMPLEX(cf32, float)

int rflu_mixed_getrf_cf64_dev(rflu_handle_t handle, int64_t n, const double* A_dev, int64_t lda, float* F32_dev, int64_t ldf,
                              int64_t* ipiv_dev, int pivot, double* anorm_out, int64_t* info)
{
    CHECK_HANDLE(handle);
    Handle* h = H(handle);
    return mixed_getrf<CplxElem<double>>(h, n, A_dev, lda, F32_dev, ldf, ipiv_dev, pivot, anorm_out, info, [&](int64_t* inf) {
        return cgetrf_rm_dev<float>(h, n, F32_dev, ldf, ipiv_dev, pivot, inf);
    });
}

int rflu_mixed_getrs_cf64_dev(rflu_handle_t handle, int64_t n, int64_t nrhs, const double* A_dev, int64_t lda, const float* F32_dev,
                              int64_t ldf, const int64_t* ipiv_dev, double anorm, const double* B_dev, int64_t ldb, double* X_dev,
                              int64_t ldx, int max_iter, int* iters)
{
    CHECK_HANDLE(handle);
    return cmixed_getrs(H(handle), n, nrhs, A_dev, lda, F32_dev, ldf, ipiv_dev, anorm, B_dev, ldb, X_dev, ldx, max_iter, iters);
}

int rflu_residual_cf64_dev(rflu_handle_t handle, int64_t n, int64_t nrhs, const double* A_dev, int64_t lda, const double* X_dev,
                           int64_t ldx, const double* B_dev, int64_t ldb, double* R_dev, int64_t ldr)
{
    CHECK_HANDLE(handle);
    return residual_public<CplxElem<double>>(H(handle), n, nrhs, A_dev, lda, X_dev, ldx, B_dev, ldb, R_dev, ldr);
}

int rflu_mixed_solve_cf32_dev(rflu_handle_t handle, int64_t n, int64_t nrhs, const float* F32_dev, int64_t ldf,
                              const int64_t* ipiv_dev, float* B_dev, int64_t ldb)
{
    CHECK_HANDLE(handle);
    return cgetrs_fwd_rm_dev<float>(H(handle), n, nrhs, F32_dev, ldf, ipiv_dev, B_dev, ldb);
}

int rflu_profile_enable(rflu_handle_t handle, int enable)
{
    CHECK_HANDLE(handle);
    Handle* h = H(handle);
    h->prof = enable == 1;
    h->prof_async = enable == 2 || enable == 3;
    h->prof_one_stream = enable == 3;
    for (int k = 0; k < RFLU_K_COUNT; ++k) h->slots[k] = ProfSlot();
    for (auto& r : h->async_recs) { h->async_pool.push_back(r.a); h->async_pool.push_back(r.b); }
    h->async_recs.clear();
    return RFLU_OK;
}

// in-schedule mode: fold the pending event pairs into the per-class timers (waits for the recorded work)
static int profile_resolve(Handle* h)
{
    for (auto& r : h->async_recs) {
        RFLU_HIP(hipEventSynchronize(r.b));
        float ms = 0.f;
        RFLU_HIP(hipEventElapsedTime(&ms, r.a, r.b));
        h->slots[r.k].ms += ms;
        h->slots[r.k].launches += 1;
        h->slots[r.k].work += r.work;
        h->slots[r.k].bytes += r.bytes;
        h->async_pool.push_back(r.a);
        h->async_pool.push_back(r.b);
    }
    h->async_recs.clear();
    return RFLU_OK;
}

int rflu_profile_get(rflu_handle_t handle, int kclass, double* ms, int64_t* launches, double* work)
{
    CHECK_HANDLE(handle);
    if (kclass < 0 || kclass >= RFLU_K_COUNT) { set_error("bad kernel class %d", kclass); return RFLU_ERR_ARG; }
    RFLU_TRY(profile_resolve(H(handle)));
    const ProfSlot& s = H(handle)->slots[kclass];
    if (ms) *ms = s.ms;
    if (launches) *launches = s.launches;
    if (work) *work = s.work;
    return RFLU_OK;
}

int rflu_profile_get_bytes(rflu_handle_t handle, int kclass, double* bytes)
{
    CHECK_HANDLE(handle);
    if (kclass < 0 || kclass >= RFLU_K_COUNT || bytes == nullptr) { set_error("bad kernel class %d", kclass); return RFLU_ERR_ARG; }
    RFLU_TRY(profile_resolve(H(handle)));
    *bytes = H(handle)->slots[kclass].bytes;
    return RFLU_OK;
}

}  // extern "C"
