// rflu_internal.hpp -- shared declarations of librflu.so (MI355X / gfx950 only; no other targets, no CPU fallback).
//
// Internal data layout ("R layout"): the matrix lives ROW-major in HBM, element (i,j) at R[i*ld + j], ld a multiple
// of 16 elements so every row starts on a 128-byte line.  Why: the row interchanges of partial pivoting
// (apply_permutation!, /root/reference/src/lu.jl:164-188) then move contiguous row segments (perfectly coalesced,
// 32 B of traffic per pivot per column, no cache-line amplification), and a panel row is one contiguous 512-byte run.
// The column-major boundary (rflu_getrf_*_dev) converts with two tiled transposes.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <functional>
#include <vector>

#include "../../include/rflu.h"

namespace rflu {

constexpr int NB = 64;            // leaf panel width == pivot chunk size (columns per cooperative panel kernel)
constexpr int PANEL_THREADS = 512;  // 8 waves = 2 per SIMD: the second wave fills the issue gaps of a latency-bound step
constexpr int MAX_PANEL_WGS = 256;  // one workgroup per CU at most: all must be co-resident (they spin on each other)

// ---- error plumbing -------------------------------------------------------------------------------------------------
void set_error(const char* fmt, ...);
#define RFLU_HIP(call)                                                                         \
    do {                                                                                       \
        hipError_t e__ = (call);                                                               \
        if (e__ != hipSuccess) {                                                               \
            ::rflu::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), __FILE__, __LINE__); \
            return RFLU_ERR_HIP;                                                               \
        }                                                                                      \
    } while (0)
#define RFLU_TRY(expr)            \
    do {                          \
        int s__ = (expr);         \
        if (s__ != RFLU_OK) return s__; \
    } while (0)

// ---- per-kernel-class timers ------------------------------------------------------------------------------------------
struct ProfSlot {
    double ms = 0.0;
    int64_t launches = 0;
    double work = 0.0;
    double bytes = 0.0;  // algorithmic (minimum) HBM bytes of the launches
};

// ---- tuning and debugging variables -----------------------------------------------------------------------------------
// Every RFLU_* environment variable of the library lives here: read ONCE per handle (rflu_create -> Tune::load_env) -- no
// getenv on the factorization paths -- and again only when the host asks for it (rflu_reload_tuning; the tests switch
// variables between calls).  INTEGRATION.md lists them.
struct Tune {
    // leaf panel
    int panel_pw = 0;                  // RFLU_PANEL_PW: floor for the row waves per cooperative workgroup (1|2|4|8)
    int panel_rpw = 0;                 // RFLU_PANEL_RPW: rows per workgroup of the cooperative leaf, forced (64|128|256|384|512; experiments)
    int panel_spare = 1;               // RFLU_PANEL_SPARE: 384-row workgroups whose communication wave has a SIMD for itself, for panels of ...
    int64_t panel_spare_min = 8192;    // RFLU_PANEL_SPARE_MIN: ... more than this many rows (and at most 32 * 384)
    int panel_maxg = 32;               // RFLU_PANEL_MAXG: most workgroups of the short-workgroup leaves
    int panel_ballast = 96 * 1024;     // RFLU_PANEL_BALLAST: dynamic LDS asked for by the 64- / 128-row workgroups (keeps them off shared CUs)
    int64_t panel_local_min = 256;     // RFLU_PANEL_LOCAL_MIN
    int64_t panel_local_rows = -1;     // RFLU_PANEL_LOCAL_ROWS: tallest XCD-local panel (-1: 4096 Float64 / 8192 Float32)
    int64_t panel_local_pw8_rows = 0;  // RFLU_PANEL_LOCAL_PW8_ROWS: XCD-local panels taller than this use 512-row workgroups (0: never)
    int poll_delay = 700;              // RFLU_POLL_DELAY: clocks between a workgroup's header publish and its poll round
    int poll_adapt = 1;                // RFLU_POLL_ADAPT: adapt that delay step by step
    // kernels
    int laswp_lpr = 0;                 // RFLU_LASWP_LPR
    int gemm_flags = 1;                // RFLU_GEMM_FLAGS
    int skinny_max_k = 128;            // RFLU_SKINNY_MAXK
    int skinny_wide = 0;               // RFLU_SKINNY_WIDE
    int64_t gemm_cfirst_below = (int64_t)1 << 40;   // RFLU_GEMM_CFIRST_BELOW
    int gemm_masked = -1;              // RFLU_GEMM_MASKED: stand-alone rflu_gemm_* calls on the CU-masked stream leaving this many CUs free
    int64_t ld_pad = 0;                // RFLU_LD_PAD
    int64_t trsv_max_rhs = 32;         // RFLU_TRSV_MAX_RHS
    int64_t mixed_gemv_max_rhs = 16;   // RFLU_MIXED_GEMV_MAX_RHS: mixed-precision refinement: residuals of up to this many right-hand sides by residual_few
                                       // (mixed.hip, passes of 8), of more by the Float64 GEMM on the transposed views
    int64_t trsm_chain_max_rhs = 320;  // RFLU_TRSM_CHAIN_MAX_RHS: up to this many right-hand sides the cooperative solve in passes of 64 (MFMA)
    int trsm_chain_cached = 1;         // RFLU_TRSM_CHAIN_CACHED=0: every workgroup fetches x_d with cache-bypassing loads (trsv.hip)
    int trsm_chain_split = 2;          // RFLU_TRSM_CHAIN_SPLIT: a pass of 64 right-hand sides as 0 = one chain of 64 columns, 1 = four of 16 in runs of two blocks,
                                       // 2 = two chains of 32 side by side (trsv.hip; n = 16384, 64 columns: 5.55 / 5.41 / 4.81 ms)
    // streams and queues
    int queue_check = 1;               // RFLU_QUEUE_CHECK
    int queue_trace = 0;               // RFLU_QUEUE_TRACE
    // block-column lookahead schedule
    int split_all = 0;                 // RFLU_SPLIT_ALL
    double split_share = 0.5;          // RFLU_SPLIT_SHARE
    double split_scale = 1.0;          // RFLU_SPLIT_SCALE
    int max_reserve = 64;              // RFLU_MAX_RESERVE
    int wide_narrow = 1;               // RFLU_WIDE_NARROW: default block width of matrices of 20480 columns and more = wide, then 512 for the last ...
    int64_t narrow_cols = 16384;       // RFLU_NARROW_COLS: ... this many columns
    int min_reserve = 32;              // RFLU_RESERVE_CUS
    int64_t confine_rows = (int64_t)1 << 40;   // RFLU_CONFINE_ROWS
    int64_t merge_rows = -1;           // RFLU_MERGE_ROWS (-1: 8192 Float64, never Float32)
    // leaf-wise schedule
    int leafwise = 1;                  // RFLU_LEAFWISE
    int64_t leafwise_rows = -1;        // RFLU_LEAFWISE_ROWS (-1: 8192 Float64 / 16384 Float32)
    int swap_su = -1;                  // RFLU_SWAP_SU (-1: by size)
    int gate_fold = 1;                 // RFLU_GATE_FOLD
    int gate_trace = 0;                // RFLU_GATE_TRACE
    int schedule_events = 0;           // RFLU_SCHEDULE=events: cross-stream edges by hipEvents only, no device-side gates (what a
                                       // counter-collection run needs: rocprofv3 --pmc runs one kernel at a time)
    int time_enqueue = 0;              // RFLU_TIME_ENQUEUE
    int tail_overlap = 1;              // RFLU_TAIL_OVERLAP
    // host-pointer entry
    int64_t host_early_out = 512;      // RFLU_HOST_EARLY_OUT
    int host_trace = 0;                // RFLU_HOST_TRACE
    int swap_late = 1;                 // RFLU_SWAP_LATE: leaf-wise schedule: side stream on the 224-CU stream (updates on the 192-CU one) from the first panel of at most swap_rows rows on, also behind a lookahead part (0: round 3's assignment)
    int64_t swap_rows = 8192;          // RFLU_SWAP_ROWS
    int leaf_fuse = 1;                 // RFLU_LEAF_FUSE: leaf-wise schedule: interchanges + diagonal inverse + 64-row solve of the next leaf's columns in ONE launch (leaf_la_kernel)
    int host_threads = 8;              // RFLU_HOST_THREADS
    // multi-GPU
    int64_t mgpu_big_reserve = 128;    // RFLU_MGPU_BIG_RESERVE
    int64_t mgpu_tall_rows = -1;       // RFLU_MGPU_TALL_ROWS
    int mgpu_sync = 0;                 // RFLU_MGPU_SYNC
    // fault injection (tests): the cooperative leaf launch with this sequence number inside a factorization waits for a
    // participant that does not exist, runs into its bounded spin and raises the timeout flag (RFLU_ERR_TIMEOUT at the end)
    int debug_ghost_leaf = -1;         // RFLU_DEBUG_GHOST_LEAF
    // persistent update engine (engine.hip): the default schedule where it measures faster than the streams, and the host entry
    int engine = -1;                   // RFLU_ENGINE: 1 = the side / update streams' work is pulled by the resident engine wherever it can be, 0 = never,
                                       // -1 (default) = where it measures faster (schedule_plan.hpp: plan_schedule)
    int engine_policy = 0;             // RFLU_ENGINE_POLICY: 0 = leftmost column block first, 1 = oldest panel piece first
    int engine_wgs = 0;                // RFLU_ENGINE_WGS: resident workgroups (0: two per CU of the update mask)
    int64_t engine_rows = 0;           // RFLU_ENGINE_ROWS: block columns whose panels are taller than this go through the engine, the streams take over below (0: the engine
                                       // to the end -- a hand-over waits for the engine's backlog on the far right: N=16384 79.6 ms at 4096 against 75.3)
    int engine_wc = 512;               // RFLU_ENGINE_WC: width of the engine's column blocks (a multiple of 128 dividing the block-column width; N=16384: 128: 82.7 ms, 256: 80.5, 512: 79.6)
    int engine_retire = -1;            // RFLU_ENGINE_RETIRE: from the first panel of at most this many rows on the engine's workgroups on the chain's XCD are gone and the
                                       // leaves XCD-local (-1: 4096, 2048 for matrices of 16384 rows or more; 0: they stay to the end, every leaf any-placement)
    int engine_replay = 0;             // RFLU_ENGINE_REPLAY=1 (measurement): the engine ALONE on the image a previous factorization of the same shape left behind -- every
                                       // leaf counts as done from the start, no chain is launched (results are meaningless; this is what rocprofv3 --pmc, which runs
                                       // one kernel at a time, can collect the resident kernel's counters on: scripts/pmc_engine.sh)
    int engine_host = 1;               // RFLU_ENGINE_HOST: host-pointer entry (rflu_getrf_*) through the engine: the way in overlaps the factorization
    int engine_write_through = 1;      // RFLU_ENGINE_WRITE_THROUGH: Schur tiles stored write-through, no L2 write-back per tile (N=16384: 84 -> 79 ms; 0: release fence per tile)
    int engine_leaf_xcds = 1;          // RFLU_ENGINE_LEAF_XCDS / RFLU_ENGINE_LEAF_WGS: the workgroups with blockIdx % 8 in [1, xcds] and blockIdx / 8 < wgs serve the
    int engine_leaf_wgs = 16;          //   leaf windows (K = 64) only: what the chain waits for never queues behind 127-us tiles (N=16384: 97 -> 84 ms; xcds 0: none)
    int engine_ahead = 1;              // RFLU_ENGINE_AHEAD: a leaf is applied leaf by leaf (K = 64) to its own block column and to this many block columns right of it
                                       // (engine.hpp: EngGeo::ahead; 1 = the stream schedule's window: the chain then waits 0.4 .. 2.5 ms at the last leaf of every block column)
    int engine_solve_rl = 1;           // RFLU_ENGINE_SOLVE_RL (experiments build): the engine's block-row solves right-looking, the block row in registers (0: left-looking,
                                       // X read back from memory; same box, alternating: N=16384 72.0-72.3 vs 72.8-73.1 ms, bit-identical)
    int engine_host_lag = 5;           // RFLU_ENGINE_HOST_LAG: host entry: whole-block-column operations that lag the chain by this many block columns go first, so
                                       // that block rows become final -- and leave -- while the factorization runs (N=16384: 3: 123 ms, 5: 109-110, 8: 112, 0 = never: 118)
    void load_env();                   // driver.cpp
};

struct Handle {
    Tune tune;
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    // second stream for the lookahead driver: the deferred trailing updates run here, restricted by a CU mask to
    // 224 of the 256 CUs so that the cooperative panel kernels of the critical path always find 32 free CUs
    hipStream_t ustreams[8] = {};     // ustreams[r]: CU mask leaving 32*r CUs to the critical path (r = 1..7)
    bool mask_failed = false;         // a CU-masked stream could not be created: plain streams may share a hardware queue, so the
                                      // device-side gates (which need the streams to run concurrently) are not used
    // host-pointer entry (host_entry.cpp: getrf_host): finished block rows travel back while the rest is still being factored
    std::function<int(int64_t)> progress;      // called by the block-column schedules: every kernel that writes rows [0, r) is enqueued
    std::function<int()> before_sync;          // called by getrf_rm when the whole factorization is enqueued, before it waits for it
    bool out_done = false;                     // set by before_sync: the factors are already in the caller's buffer
    std::vector<hipEvent_t> out_events;        // event pool of that path
    void* bounce[2] = {};                      // pinned bounce buffers of that path (one chunk of rows each)
    void* out_stage = nullptr;                 // device staging of the outgoing chunks (two pieces), so that the input copy stays intact
    size_t out_stage_bytes = 0;
    size_t bounce_bytes = 0;
    std::vector<hipStream_t> parked_streams;   // masked streams that shared a pipe with a stream in use (validate_queues): kept idle
    long long* qprobe_slots = nullptr;         // device: 4 stamps of the pipe probe
    std::vector<hipStream_t> queues_ok_streams;   // validate_queues: caller streams the masked streams in use have been checked against
    int queues_ok_count = 0;                      // ... and how many masked streams existed then
    int queue_unresolved = 0;                     // validate_queues: checks that ended with a conflict it could not settle
    bool queue_giveup = false;                    // ... three of them: the placement is taken as it is from then on
    hipStream_t pstreams[8] = {};     // pstreams[r]: the complement -- exactly those 32*r CUs (critical path of the update-bound phase)
    bool panel_attr_set[2][2][2] = {};     // [any placement|XCD-local][Float64|Float32][64|128 rows]: dynamic-LDS attribute of the small-workgroup leaves
    hipEvent_t tail_event = nullptr;       // column-major entry: the columns right of the first block column are still being
                                           // transposed on the update stream; set = pending, consumed by getrf_rm
    hipEvent_t tail_event_obj = nullptr, tail_fork_obj = nullptr;
    unsigned long long* gates = nullptr;   // device: [0] critical path, [1] side stream 1, [2] side stream 2 (leaf counters)
    unsigned long long* gate_ptr[3] = {};  // the three counters
    unsigned long long gate_epoch = 0;     // counters only grow: leaf g of a factorization is gate_epoch + g + 1
    long long* gate_stamps = nullptr;      // RFLU_GATE_TRACE: wall-clock stamps of the signals, [3][4096] (scripts/gate_trace.py)
    std::vector<hipEvent_t> events;   // reusable, timing disabled
    int last_path = RFLU_PATH_NONE;
    int num_cus = 256;

    // workspaces (grown on demand, kept for reuse across calls -- LinearSolve-style cache reuse)
    void* work = nullptr;        // row-major copy of the matrix for the column-major entry points
    size_t work_bytes = 0;
    int64_t* ipiv_dev = nullptr; // device pivots for the host entry points
    size_t ipiv_cap = 0;
    void* hostA_dev = nullptr;   // device copy of the host matrix (host entry points)
    size_t hostA_bytes = 0;
    void* rhs_work = nullptr;    // row-major copy of the right-hand sides (getrs)
    size_t rhs_work_bytes = 0;
    void* hostB_dev = nullptr;   // device copy of host right-hand sides (getrs host entry)
    size_t hostB_bytes = 0;
    // mixed-precision solve (mixed.hip, driver.cpp: mixed_getrf / mixed_refine), real and complex
    void* mixed_rhs = nullptr;   // Float32 row-major right-hand sides / corrections
    size_t mixed_rhs_bytes = 0;
    void* mixed_r = nullptr;     // Float64 residual, column-major n x nrhs
    size_t mixed_r_bytes = 0;
    void* mixed_part = nullptr;  // partial sums: row sums of |A| per tile column, the column slices' shares of A X
    size_t mixed_part_bytes = 0;
    void* mixed_norms = nullptr; // device: ||A||_inf, or per column {||r_k||_inf, ||x_k||_inf} ...
    size_t mixed_norms_bytes = 0;
    void* mixed_norms_host = nullptr;   // ... and their pinned host image: the one host read of a refinement step
    size_t mixed_norms_host_bytes = 0;
    // inverse / logabsdet (inverse.hip)
    void* inv_work = nullptr;    // getri: W x n elements -- the negated diagonal block and Q of the G sweep, then the saved block row of H
    size_t inv_work_bytes = 0;
    void* inv_part = nullptr;    // logabsdet: per-chunk partial sums, then {logabs, sign, first zero}
    size_t inv_part_bytes = 0;
    // operator norms / condition estimate (condest.hip): the estimator's work vector and sign vector, per-chunk partial results
    void* cond_work = nullptr;
    size_t cond_work_bytes = 0;

    // pivot bookkeeping: for every chunk of NB pivots the list of (dst,src) row moves equivalent to its interchanges
    int* pm_cnt = nullptr;
    int* pm_dst = nullptr;
    int* pm_src = nullptr;
    int64_t pm_chunks = 0;
    void* linv = nullptr;        // inverses of the 64x64 diagonal blocks of L, one per leaf (pm_chunks x 64 x 64 elements)
    unsigned trsv_tag = 0;       // last tag used by the cooperative solve (trsv.hip) in its exchange area ...
    void* trsv_area = nullptr;   // ... which lives at this address inside linv_tmp
    void* linv_tmp = nullptr;    // same for stand-alone rflu_trsm_rm_* calls
    size_t linv_tmp_bytes = 0;

    // cooperative panel scratch: double-buffered granule records + status words
    unsigned long long* pscratch = nullptr;
    size_t pscratch_bytes = 0;
    unsigned epoch = 1;          // next unused granule tag
    int coop_leaf_seq = 0;       // cooperative leaf launches since the start of the current factorization (Tune::debug_ghost_leaf)
    int64_t* info_dev = nullptr; // [0] = info, [1] = panel error flags (bit0 timeout, bit1 XCD placement mismatch)
    // pipelined leaf kernel with a communication wave (panel_local.hip), RFLU_PANEL_LOCAL: 0 = off (the kernels of
    // panel.hip), 2 = on with sc1 records on any placement (default), 1 = all workgroups on XCD panel_xcc with plain-store
    // records through that XCD's L2 (needs that XCD free: experiments only)
    int panel_local = 2;
    int panel_single = 1;        // RFLU_PANEL_SINGLE: leaves of at most 512 rows in one workgroup, LDS only (panel_single.hip)
    int panel_blocked = 0;       // RFLU_PANEL_BLOCKED=1: full pivoted leaves by the sub-panel kernel with one chain wave per workgroup (panel_blocked.hip;
                                 // bit-identical, measured no faster than the default leaves: opt-in)
    int panel_local_maxg = 64;
    int panel_xcc = 0;
    int64_t local_rows_cap = -1; // set by the schedule: tallest XCD-local leaf while it runs (0 while the update engine is resident; -1: no cap)
    int trsv_max_wgs[2] = {0, 0};    // same for the cooperative solve kernels (asked on first use, per element type: [Float64, Float32])
    int trsm32_per_cu[2] = {0, 0};
    int trsm16_per_cu[2] = {0, 0};   // workgroups of the 16-column block solve a CU holds (trsv.hip: chains side by side)
    int panel_max_wgs = 0;       // how many workgroups of the cooperative panel kernels the device holds at once (occupancy query)
    bool coop_launch = false;    // RFLU_COOP_LAUNCH=1: hipLaunchCooperativeKernel (launch-time residency check, +15-19 us each)
    bool la_attr_set[2] = {false, false};     // dynamic-LDS opt-in of leaf_la_kernel (f64, f32)
    bool gemm_attr_set[2] = {false, false};   // dynamic-LDS opt-in of the GEMM kernels done on this handle's device (f64, f32)
    bool eng_attr_set[2] = {false, false};    // same for the persistent update engine (engine.hip)
    bool batched_attr_set[3][4] = {};         // same for the batched kernels (batched_kernels.hpp): [getrf|getrs|getri][f64, f32, cf64, cf32]
    bool cinv_attr_set[2] = {false, false};   // same for the 64x64 triangular inverses of the complex getri (inverse.hip): [cf64, cf32]
    size_t gecon_lds_asked[2] = {0, 0};       // dynamic LDS asked for the batched condition estimate so far (batched.hip: gecon_batched_kernel): [f64, f32]
    size_t cgecon_lds_asked[2] = {0, 0};      // the same for the complex estimate (batched_complex.hip: cgecon_batched_kernel): [cf64, cf32]
    void* eng_state = nullptr;                // device: EngState (engine.hpp)
    void* eng_host = nullptr;                 // pinned host image of its initial value
    long long* eng_trace_buf = nullptr;       // device: RFLU_ENGINE_TRACE stamps + workgroup-time accounting (measurement only)
    bool eng_active = false;                  // a factorization's engine is resident (factor_leafwise in engine mode .. the join with its stream)
    // host entry through the engine (host_entry.cpp: getrf_host_engine): the matrix arrives while it is being factored
    bool eng_host_mode = false;
    unsigned long long* eng_rows_final = nullptr;       // pinned host word (rows of the factors that are final), ...
    unsigned long long* eng_rows_final_dev = nullptr;   // ... its device address
    int64_t* info_pinned = nullptr;

    // timers
    bool prof = false;           // synchronous mode: every launch bracketed and waited for (switches to the one-stream schedule)
    bool prof_async = false;     // in-schedule mode: event pairs recorded on the launch streams, resolved by profile_get
    bool prof_one_stream = false;   // mode 3: the one-stream schedule of the synchronous mode with the event pairs of the in-schedule mode
                                    // (nothing waited for between launches: the GPU does not idle -- and drop its clock -- behind every kernel)
    ProfSlot slots[RFLU_K_COUNT];
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    struct AsyncRec { int k; hipEvent_t a, b; double work, bytes; };
    std::vector<AsyncRec> async_recs;      // pending event pairs of the in-schedule mode
    std::vector<hipEvent_t> async_pool;    // timing events kept for reuse
};

// tallest panel the XCD-local leaf serves: RFLU_PANEL_LOCAL_ROWS (default 4096 Float64 / 8192 Float32), at most `cap` (Handle::local_rows_cap)
inline int64_t local_leaf_rows(const Tune& t, size_t esize, int64_t cap = -1)
{
    const int64_t rows = t.panel_local_rows >= 0 ? t.panel_local_rows : (esize == 4 ? 8192 : 4096);
    return cap >= 0 && cap < rows ? cap : rows;
}

// run the launchers on `s` until the end of the scope; the handle's stream is put back on every way out
struct OnStream { Handle* h; hipStream_t saved; OnStream(Handle* h_, hipStream_t s) : h(h_), saved(h_->stream) { h->stream = s; } ~OnStream() { h->stream = saved; } OnStream(const OnStream&) = delete; OnStream& operator=(const OnStream&) = delete; };

struct ProfScope {
    Handle* h;
    int k;
    double work;
    double bytes;
    bool on;
    hipEvent_t ea = nullptr, eb = nullptr;
    static hipEvent_t take(Handle* h) {
        if (!h->async_pool.empty()) { hipEvent_t e = h->async_pool.back(); h->async_pool.pop_back(); return e; }
        hipEvent_t e = nullptr;
        (void)hipEventCreate(&e);
        return e;
    }
    ProfScope(Handle* h_, int k_, double work_, double bytes_ = 0.0) : h(h_), k(k_), work(work_), bytes(bytes_), on(h_->prof) {
        if (on) (void)hipEventRecord(h->ev0, h->stream);
        else if (h->prof_async) {   // no wait: the pair is resolved when the timers are read
            ea = take(h);
            eb = take(h);
            if (ea) (void)hipEventRecord(ea, h->stream);
        }
    }
    ~ProfScope() {
        if (ea && eb) {
            (void)hipEventRecord(eb, h->stream);
            h->async_recs.push_back({k, ea, eb, work, bytes});
        }
        if (on) {
            (void)hipEventRecord(h->ev1, h->stream);
            (void)hipEventSynchronize(h->ev1);
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, h->ev0, h->ev1);
            h->slots[k].ms += ms;
            h->slots[k].launches += 1;
            h->slots[k].work += work;
            h->slots[k].bytes += bytes;
        }
    }
};

int ensure_bookkeeping(Handle* h, int64_t rows);
int ensure_buffer(void** ptr, size_t* cap, size_t need);  // grow-only device buffer (hipFree + hipMalloc)

// ---- kernel launchers (each returns an rflu_status); all pointers are device pointers in R layout -----------------------
int panel_local_rows_per_wg(const Handle* h, int64_t rows, size_t esize);   // panel_local.hip: rows per workgroup of a pivoted leaf
// panel.hip: does a full pivoted leaf of `rows` rows go to the sub-panel kernel (panel_blocked.hip), and the workgroups the leaf
// kernel of launch_panel's choice takes (what a schedule has to keep free)
bool panel_use_blocked(const Handle* h, int64_t rows, size_t esize);
int64_t panel_plan_wgs(const Handle* h, int64_t rows, size_t esize, int pivot);
int launch_heat(Handle* h, int cus, double usec);   // gemm.hip: clock keeper
// optional early-completion signal of a GEMM launch: the tiles of the first `first_cols` columns of C are computed first and
// the last of them publishes `val` in *flag (a stream gate, see LaswpGate); cnt: zero-initialised wrapping counter
struct GemmSignal {
    int64_t first_cols = 0;
    unsigned long long* flag = nullptr;
    unsigned long long val = 0;
    unsigned* cnt = nullptr;
};
template <typename T>
int launch_gemm(Handle* h, int64_t M, int64_t N, int64_t K, const T* A, int64_t lda, const T* B, int64_t ldb, T* C,
                int64_t ldc, GemmSignal sig = GemmSignal{});
template <typename T>
int launch_trsm_base(Handle* h, int64_t nb, int64_t nrhs, const T* L, int64_t ldl, T* B, int64_t ldb);
// fused strip TRSM (n <= 256) on pre-inverted 64x64 diagonal blocks, and the batched inversion of those blocks
template <typename T>
int launch_trsm_fused(Handle* h, int64_t n, int64_t nrhs, const T* L, int64_t ldl, const T* Linv, T* B, int64_t ldb);
template <typename T>
int launch_triu_base(Handle* h, int64_t nb, int64_t nrhs, const T* U, int64_t ldu, T* B, int64_t ldb);
template <typename T>
int launch_diag_inv(Handle* h, int64_t n, const T* L, int64_t ldl, T* Linv);
template <typename T>
int launch_trsm_inv64(Handle* h, int64_t n, int64_t nrhs, const T* Linv, T* B, int64_t ldb);   // one block, LDS-free
// cooperative solve for few right-hand sides (trsv.hip): B <- U^-1 L^-1 B, interchanges already applied.  trans: R is the row-major
// image of F^T (a column-major F read with ld = lda) and B <- L^-T U^-T B; the interchanges come afterwards, backwards (launch_laswp_rev)
template <typename T>
int launch_trsv_coop(Handle* h, int64_t n, int64_t nrhs, const T* R, int64_t ld, T* B, int64_t ldb, bool wide = false, bool trans = false);
// stream gates folded into an interchange launch (laswp.hip; used by factor_leafwise): hold the launch until *wait_flag >=
// wait_val, and let its last workgroup publish signal_val (signal_cnt: a zero-initialised counter that wraps by itself)
struct LaswpGate {
    const unsigned long long* wait_flag = nullptr;
    unsigned long long wait_val = 0;
    unsigned long long* signal_flag = nullptr;
    unsigned long long signal_val = 0;
    unsigned* signal_cnt = nullptr;
    int64_t* info = nullptr;   // timeout flag (info[1] bit 0)
};
template <typename T>
int launch_laswp(Handle* h, T* R, int64_t ld, int64_t c0, int64_t ncols, int64_t chunk0, int64_t chunk1);
// apply chunks [chunk0, chunk1) to two column ranges at once: [c0, c0+ncolsA) and [c1, c1+ncolsB)
template <typename T>
int launch_laswp3(Handle* h, T* R, int64_t ld, int64_t c0, int64_t ncolsA, int64_t c1, int64_t ncolsB, int64_t c2,
                  int64_t ncolsC, int64_t chunk0, int64_t chunk1, int64_t inv_nb, int64_t inv_cnt, const T* inv_L,
                  T* inv_out, LaswpGate gate = LaswpGate{});
template <typename T>
int launch_laswp2(Handle* h, T* R, int64_t ld, int64_t c0, int64_t ncolsA, int64_t c1, int64_t ncolsB, int64_t chunk0,
                  int64_t chunk1, int64_t inv_nb = 0, const T* inv_L = nullptr, T* inv_out = nullptr,
                  LaswpGate gate = LaswpGate{});
// leaf-wise schedule, one launch behind a full leaf (rows / columns c0.., move list `chunk`): the leaf's interchanges on the next
// leaf's 64 columns [la0, la0 + 64), the inverse of its diagonal block (-> inv_out) and the solve of those columns' top 64 rows
template <typename T>
int launch_leaf_la(Handle* h, T* R, int64_t ld, int64_t la0, int64_t chunk, int64_t c0, const T* inv_L, T* inv_out, LaswpGate gate);
// fold the interchanges ipiv[k0..k1) (k0 a multiple of NB) into per-chunk row-move lists
int launch_perm_build(Handle* h, const int64_t* ipiv, int64_t k0, int64_t k1, int64_t m);
// the interchanges of chunks [chunk0, chunk1) UNDONE on columns [0, ncols) of the row-major block B: last chunk first, every chunk's
// move list (launch_perm_build) run backwards -- B <- P^T B, the last step of the transposed solve
template <typename T>
int launch_laswp_rev(Handle* h, T* B, int64_t ldb, int64_t ncols, int64_t chunk0, int64_t chunk1);
size_t panel_scratch_bytes();
int panel_resident_limit(int num_cus);   // min over the cooperative leaf kernels of (resident workgroups per CU) * num_cus
size_t panel_trace_offset_bytes();
size_t panel_trace_all_offset_bytes();
size_t panel_trace_all_words();
template <typename T>
int launch_panel(Handle* h, T* R, int64_t ld, int64_t m, int64_t r0, int64_t c0, int64_t w, int64_t* ipiv, int pivot);
template <typename T>
int launch_panel_pair(Handle* h, T* R, int64_t ld, int64_t m, int64_t r0, int64_t c0, int64_t* ipiv);
template <typename T>
int launch_transpose(Handle* h, int64_t rows_out, int64_t cols_out, const T* in, int64_t ld_in, T* out, int64_t ld_out);
// the same on an explicit stream, touching nothing of the handle (a second host thread feeds the matrix in: host_entry.cpp, getrf_host_engine)
template <typename T>
int launch_transpose_on(hipStream_t st, int64_t rows_out, int64_t cols_out, const T* in, int64_t ld_in, T* out, int64_t ld_out);
int launch_gate_signal_on(hipStream_t st, unsigned long long* flag, unsigned long long value);
template <typename T>
int launch_fill_uniform(Handle* h, T* A, int64_t m, int64_t n, int64_t ld, int row_major, uint64_t seed,
                        int64_t M_global, int64_t i0, int64_t j0, double diag_add);
int launch_iota_ipiv(Handle* h, int64_t* ipiv, int64_t k0, int64_t n);
int queue_probe(hipStream_t a, hipStream_t b, long long* slots, long long* host3, int* shared);   // laswp.hip: do two streams share a pipe?
int queue_probe_rate(hipStream_t a, hipStream_t b, int n, long long* slots, double* us_per_kernel);
int launch_gate_signal(Handle* h, unsigned long long* flag, unsigned long long value, long long* stamp = nullptr);   // laswp.hip: device-side stream gates
int launch_gate_wait(Handle* h, const unsigned long long* flag, unsigned long long value);
// butterfly.hip: A <- U' A V (column-major, in place) and x <- U' x (mode 0) / x <- V x (mode 1)
template <typename T>
int launch_butterfly_mul(Handle* h, int64_t n, T* A, int64_t lda, const T* uv);
template <typename T>
int launch_butterfly_vec(Handle* h, int64_t n, int64_t nrhs, T* X, int64_t ldx, const T* uv, int mode);
// batched.hip (geometry, wave maximum and launch: batched_kernels.hpp): `batch` independent matrices of max(m, n) <= BATCHED_MAX_DIM, one group of threads each, everything between the one
// load and the one store in LDS.  Matrix b at A + b*strideA, element (i, j) at [i + j*lda] or (row_major) [i*lda + j]; info: DEVICE
// array of `batch` entries.  The solve: B in the orientation of F, any nrhs in passes of 8, trans = B <- A^-T B.
constexpr int64_t BATCHED_MAX_DIM = 128;
constexpr int64_t CBATCHED_MAX_DIM_CF32 = 128;   // batched_complex.hip, ComplexF32: the bytes of the Float64 real kernel
constexpr int64_t CBATCHED_MAX_DIM_CF64 = 64;    // ComplexF64: 65 x 64 x 16 B = 66.5 KB per matrix, two groups and their right-hand sides per CU
bool batched_fits(int64_t m, int64_t n);
template <typename T>
int launch_getrf_batched(Handle* h, int64_t batch, int64_t m, int64_t n, T* A, int64_t lda, int64_t strideA, int row_major,
                         int64_t* ipiv, int64_t stride_ipiv, int pivot, int64_t* info);
template <typename T>
int launch_getrs_batched(Handle* h, int64_t batch, int64_t n, int64_t nrhs, const T* F, int64_t lda, int64_t strideF, int row_major,
                         const int64_t* ipiv, int64_t stride_ipiv, T* B, int64_t ldb, int64_t strideB, int trans);

// batched_complex.hip: the same two kernels for ComplexF64 / ComplexF32 (R = double / float behind interleaved (re, im) pairs; lda, ldb
// and the strides in complex elements), max(m, n) <= CBATCHED_MAX_DIM_CF64 / _CF32.  trans: 0 = A, 1 = transpose(A), 2 = A'.
template <typename R>
bool cbatched_fits(int64_t m, int64_t n);
template <typename R>
int launch_cgetrf_batched(Handle* h, int64_t batch, int64_t m, int64_t n, R* A, int64_t lda, int64_t strideA, int row_major,
                          int64_t* ipiv, int64_t stride_ipiv, int pivot, int64_t* info);
template <typename R>
int launch_cgetrs_batched(Handle* h, int64_t batch, int64_t n, int64_t nrhs, const R* F, int64_t lda, int64_t strideF, int row_major,
                          const int64_t* ipiv, int64_t stride_ipiv, R* B, int64_t ldb, int64_t strideB, int trans);
// the batched complex inverse: Ainv_b <- inv(op(A_b)) from the factors, out of place, Ainv in the orientation of F (op by `trans` as
// above: the three differ in the store only); info[b] = first u_ii with both parts zero, or 0
template <typename R>
int launch_cgetri_batched(Handle* h, int64_t batch, int64_t n, const R* F, int64_t lda, int64_t strideF, int row_major, const int64_t* ipiv,
                          int64_t stride_ipiv, R* Ainv, int64_t ldi, int64_t strideI, int trans, int64_t* info);

// the batched inverse: Ainv_b <- A_b^-1 from the factors, out of place, Ainv in the orientation of F; info[b] = first zero u_ii or 0
template <typename T>
int launch_getri_batched(Handle* h, int64_t batch, int64_t n, const T* F, int64_t lda, int64_t strideF, int row_major, const int64_t* ipiv,
                         int64_t stride_ipiv, T* Ainv, int64_t ldi, int64_t strideI, int64_t* info);

// trsv.hip: the 64x64 diagonal inverses of both triangles of the transposed view V (lower non-unit -> Ginv, unit upper -> Hinv; block b
// dense row-major at [b * 64 * 64], identity padding beyond the matrix)
template <typename T>
int launch_tri_inv_trans(Handle* h, int64_t n, const T* V, int64_t ld, T* Ginv, T* Hinv);

// The element trait of the sources that serve the four element types from one text (condest.hip, mixed.hip, inverse.hip).  An ELEMENT
// is what a leading dimension counts: RealElem<R> is one R, CplxElem<R> one interleaved (re, im) pair of R, and every array crosses as
// R* (R = double / float).
template <typename R>
struct RealElem {
    typedef R real;
    static constexpr int PARTS = 1;
    static constexpr const char* WHO = "";   // in front of the entry's name in every message
    static __device__ __forceinline__ double abs(const R* p) { return __builtin_fabs((double)p[0]); }
    static __device__ __forceinline__ double modulus(const R* p) { return abs(p); }
};
template <typename R>
struct CplxElem {
    typedef R real;
    static constexpr int PARTS = 2;
    static constexpr const char* WHO = "complex ";
    // Float64 hypot, except that a NaN in EITHER part gives NaN: C's hypot(Inf, NaN) is Inf, so the parts are tested, not the modulus
    static __device__ __forceinline__ double abs(const R* p)
    {
        const double x = (double)p[0], y = (double)p[1];
        if (x != x || y != y) return __builtin_nan("");
        return hypot(x, y);
    }
    // plain Float64 hypot, NOT abs: (Inf, NaN) gives Inf.  What the mixed-precision kernels (mixed.hip) take as the modulus
    static __device__ __forceinline__ double modulus(const R* p) { return hypot((double)p[0], (double)p[1]); }
};

// inverse.hip (DESIGN.md sections 4.4, 4.8), one source for the four element types.  The diagonal entry i is element i * dstride of F
// (dstride = ld + 1 in both layouts); results on the HOST, the stream is synchronised.  The sign is *sign_re for real elements (sign_im is
// not touched), the phase (*sign_re, *sign_im) for complex ones.  zero1: 1-based index of the first exactly-zero entry (complex: both parts zero), 0 = none.
constexpr int64_t GETRI_W = 512;   // block-column / block-row width of getri's two sweeps
int64_t getri_width(int64_t n);    // ... for an n x n matrix (smaller matrices: n rounded up to 64)
template <typename E>
int launch_logabsdet(Handle* h, int64_t n, const typename E::real* F, int64_t dstride, const int64_t* ipiv, double* logabs, double* sign_re,
                     double* sign_im, int64_t* zero1);
// logabs[b], sign[E::PARTS * b ...] (device) for matrix b, strideF elements after the one before.  Enqueued only.
template <typename E>
int launch_logabsdet_batched(Handle* h, int64_t batch, int64_t n, const typename E::real* F, int64_t dstride, int64_t strideF,
                             const int64_t* ipiv, int64_t stride_ipiv, double* logabs, double* sign);
// V: row-major n x n image of F^T (the plain transpose), overwritten by A^-T; *info (host): first exactly-zero u_ii, V then untouched.
// Complete on return.
template <typename E>
int getri_view(Handle* h, int64_t n, typename E::real* V, int64_t ld, const int64_t* ipiv, int64_t* info);

// condest.hip (DESIGN.md sections 4.11, 4.12): operator norms and the vector kernels of the condition estimate, one source for the four
// element types.  Every sum is Float64 in a fixed order (no read-modify-write on shared words): results repeat bit for bit.
// *out (host) = the 1- or Inf-norm of the m x n matrix A; element (i, j) at [i + j*lda] or (row_major) [i*lda + j].  Synchronises.
template <typename E>
int launch_lange(Handle* h, int norm, int64_t m, int64_t n, const typename E::real* A, int64_t lda, int row_major, double* out);
// out_dev[b] (device) = the same for matrix b, strideA elements after the one before; one workgroup per matrix up to 128 x 128, the
// single kernels matrix by matrix above; bit-identical to launch_lange on the same matrix.  Enqueued only.
template <typename E>
int launch_lange_batched(Handle* h, int norm, int64_t batch, int64_t m, int64_t n, const typename E::real* A, int64_t lda, int64_t strideA,
                         int row_major, double* out_dev);
// the estimator's vectors: x and sgn are n contiguous elements on the device
struct CondStats {
    double sum;        // sum of |x_i|, chunks of 1024 by a fixed tree, chunk sums in index order
    double maxabs;     // max |x_i| ...
    double xj_abs;     // |x[jq]| (0 when jq < 0)
    long long argmax;  // ... and the FIRST index that attains it
    int differs;       // real: number of i with sign(x_i) != sgn[i], sign(v) = v >= 0 ? +1 : -1; complex: 0
    int nonfinite;     // a NaN or Inf among the x_i
};
enum { COND_FILL_ONES = 0, COND_FILL_UNIT = 1, COND_FILL_ALT = 2 };   // ones; e_j; x_i = (-1)^i (n - 1 + i); imaginary parts zero
template <typename E>
int launch_cond_fill(Handle* h, int64_t n, typename E::real* x, int mode, int64_t j);
// the statistics of x (host, the stream is synchronised).  `write`, real: afterwards x and sgn hold sign(x); complex: sgn is never read
// (pass nullptr) and afterwards x holds the phases x_i / |x_i| (1 + 0i where both parts are zero)
template <typename E>
int launch_cond_stats(Handle* h, int64_t n, typename E::real* x, typename E::real* sgn, int64_t jq, int write, CondStats* out);
// batched.hip: the whole estimator on a matrix held in LDS, one launch for n <= BATCHED_MAX_DIM
template <typename T>
int launch_gecon_batched(Handle* h, int norm, int64_t batch, int64_t n, const T* F, int64_t lda, int64_t strideF, int row_major,
                         const double* anorm, double* rcond);

// mixed.hip: the kernels of the mixed-precision solve, E = RealElem<double> or CplxElem<double>.  A, X, B, R column-major Float64 /
// ComplexF64; F row-major Float32 / ComplexF32; every ld in elements.
constexpr int RESIDUAL_PASS = 8;   // right-hand sides per launch of residual_few
// F <- narrow(A) in row-major, *anorm_dev (device) <- ||A||_inf (complex: row sums of moduli); partial sums in Handle::mixed_part
template <typename E>
int launch_demote_relayout(Handle* h, int64_t n, const double* A, int64_t lda, float* F, int64_t ldf, double* anorm_dev);
// R <- B - A X for nrhs <= RESIDUAL_PASS; A is read once
template <typename E>
int launch_residual_few(Handle* h, int64_t n, int64_t nrhs, const double* A, int64_t lda, const double* X, int64_t ldx, const double* B,
                        int64_t ldb, double* R, int64_t ldr);
// out[r][c] = (TO) in[c][r], or += with add: element type and layout of the right-hand sides in one pass
template <typename E, typename TI, typename TO>
int launch_convert_transpose(Handle* h, int64_t rows_out, int64_t cols_out, const TI* in, int64_t ld_in, TO* out, int64_t ld_out, bool add);
// complex only: out (+)= (TO) in on column-major n x nrhs blocks, the element type alone
template <typename TI, typename TO>
int launch_cconvert(Handle* h, int64_t n, int64_t nrhs, const TI* in, int64_t ld_in, TO* out, int64_t ld_out, bool add);
// norms[2k] = ||r_k||_inf, norms[2k + 1] = ||x_k||_inf (complex: largest modulus; a NaN anywhere in a column is kept)
template <typename E>
int launch_colnorms(Handle* h, int64_t n, int64_t nrhs, const double* R, int64_t ldr, const double* X, int64_t ldx, double* norms);

// refine.hip: the kernels of rflu_gerfs_* / rflu_berr_*, T = double or float.  A, X, B column-major T; every
// sum Float64 in a fixed order.  Enqueued only.
constexpr int REFINE_PASS = 8;    // right-hand sides that advance in lock step: one pass over A, one solve on an n x REFINE_PASS block
constexpr int REFINE_LDD = 16;    // leading dimension of that row-major block (rows of 16 elements, as the other right-hand-side images)
// for nr <= REFINE_PASS columns: R[i + k n] = (b - A x)_i and Wt[i + k n] = (|b| + |A| |x|)_i in Float64 (both n x REFINE_PASS,
// column-major) and, D != NULL, D[i * REFINE_LDD + k] = (T) R[i, k] for k < nr, 0 for nr <= k < REFINE_PASS.  A is read once; the partial
// sums go through Handle::mixed_part
template <typename T>
int launch_absresidual(Handle* h, int64_t n, int64_t nr, const T* A, int64_t lda, const T* X, int64_t ldx, const T* B, int64_t ldb,
                       double* R, double* Wt, T* D);
// out[2k] = max_i |R[i, k]| / Wt[i, k] (a row with Wt == 0 gives 0; a NaN is kept), out[2k + 1] = max_i |X[i, k]|; one workgroup a column
template <typename T>
int launch_berr_reduce(Handle* h, int64_t n, int64_t nr, const double* R, const double* Wt, const T* X, int64_t ldx, double* out);
// X[i, k] += D[i * REFINE_LDD + k] for the columns k < nr whose bit is set in mask
template <typename T>
int launch_refine_update(Handle* h, int64_t n, int64_t nr, unsigned mask, const T* D, T* X, int64_t ldx);
// wt[i] = (T)(|r_i| + (n + 1) u w_i), u the unit roundoff of T; and x[i] *= wt[i] on n contiguous elements
template <typename T>
int launch_refine_weights(Handle* h, int64_t n, const double* r, const double* w, T* wt);
template <typename T>
int launch_refine_scale(Handle* h, int64_t n, const T* wt, T* x);

}  // namespace rflu
