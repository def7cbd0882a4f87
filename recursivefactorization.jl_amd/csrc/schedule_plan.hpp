// schedule_plan.hpp -- which schedule factors a matrix: ONE pure function (plan_schedule) of the call, the handle's tuning and the
// workspace, used by every entry of driver.cpp and host_entry.cpp and checked on the host by tests/schedule_plan_check.cpp.  No HIP calls, no side effects.
//
// Which schedule serves which call (blocksize = 0 unless stated; W = the block width, default_blocksize below; sections: DESIGN.md):
//
// | call                                                                 | schedule                                                    | rflu_last_path |
// |----------------------------------------------------------------------|-------------------------------------------------------------|----------------|
// | min(m, n) < 1024, or blocksize < 0, or blocksize >= min(m, n)        | the Toledo recursion on one stream (Fact::rec): reckernel!'s | hip-recursive  |
// |                                                                      | sequence (src/lu.jl:229-246) with 64-column leaves           |                |
// | block columns of width W (256 up to 11264 columns, 512 up to 16384,  | block-column lookahead on two CU-masked streams              | hip-lookahead  |
// | 1024 up to 24576, 2048 above; from 20480 columns on "wide, then 512  | (factor_lookahead, section 3.6); panels above 32768 rows     |                |
// | for the last 16384 columns") whose panels are taller than 8192 rows  | single-stream                                                |                |
// | (Float32: 16384)                                                     |                                                             |                |
// | ... from the first panel of at most 8192 (16384) rows on (b_switch)  | leaf-wise schedule (factor_leafwise, section 3.6): the chain | hip-lookahead  |
// |                                                                      | of leaves + one side stream + one update stream              |                |
// | pivoted, default W = 512: more than 11264 columns, at most 16384     | the chain of leaves (section 3.3) + the persistent update    | hip-engine     |
// | rows, m >= n, Float64 and Float32 -- the headline size -- and        | engine (engine.hip, section 3.5) for block columns           |                |
// | RFLU_ENGINE=1 wherever the engine can serve (engine_usable)          | [0, eng_end)                                                 |                |
// | host-pointer entry, pivoted, 8192 <= min(m, n), m <= 16384, m >= n,  | the same, with the matrix arriving while it is factored      | hip-engine     |
// | either element type                                                  | (host_engine, section 3.8)                                   |                |
// | profiling modes 1 / 3, devices without 256 CUs                       | right-looking block columns on one stream                    | hip-blocked    |
//
// The column-major entry changes the layout of the columns right of the first block column on the update stream while the first panel
// runs (tail_overlap); the host entry brings finished block rows home while the rest is still being factored (host_early) when it does
// not go through the engine.  While the engine is resident the XCD-local leaves are off (Handle::local_rows_cap); with the engine to
// the end its workgroups on the chain's XCD retire in front of eng_retire_leaf and the XCD-local leaves come back from there on.
#pragma once

#include <stdint.h>

#include <algorithm>

#include "rflu_internal.hpp"
#include "engine.hpp"

namespace rflu {

enum SchedEntry {
    ENTRY_RM = 0,           // row-major device matrix (rflu_getrf_*_rm), and getrf_rm under the column-major entry
    ENTRY_CM = 1,           // column-major device matrix (getrf_cm_dev): the layout change in front
    ENTRY_HOST = 2,         // host matrix (host_entry.cpp: getrf_host): through the engine, or staged through the column-major entry
    ENTRY_HOST_ENGINE = 3,  // getrf_rm under the host entry through the engine (Handle::eng_host_mode)
};

struct SchedIn {
    int64_t m = 0, n = 0;
    size_t esize = 8;
    int pivot = 1;
    int64_t blocksize = 0;      // the caller's (0: default_blocksize)
    int entry = ENTRY_RM;
    Tune tune;
    // the handle
    int num_cus = 256;
    bool prof = false;          // Handle::prof || Handle::prof_one_stream: the one-stream schedule
    bool mask_failed = false;   // a CU-masked stream could not be created (getrf_rm: as it is after the streams have been asked for)
    bool progress = false;      // the host entry's progress hook is set
    int panel_local = 2;
    bool coop_launch = false;
    // the workspace
    int64_t roff = 0;
    bool aligned16 = true;      // R 16-byte aligned
    int64_t ld = 0;
};

struct SchedPlan {
    int path = RFLU_PATH_NONE;
    bool two_stream = false;      // lookahead / engine: the schedules on CU-masked streams (getrf_rm asks for them first)
    int64_t Wb = 0;               // block width (a multiple of 64) of the lookahead, engine and blocked paths
    int64_t nblk = 0;             // block columns of width Wb
    int64_t W_wide = 0, wide_end = 0;   // lookahead: block columns [0, wide_end) W_wide wide
    int64_t b_switch = 0;         // lookahead: first block column of the leaf-wise part (nblk: none)
    int64_t eng_end = 0;          // engine: block columns [0, eng_end) through the engine
    int eng_wc = 0;               // engine: width of its column blocks
    int eng_ahead = 0;            // engine: block columns right of a leaf's own it applies the leaf to (EngGeo::ahead)
    int64_t eng_retire_leaf = -1; // engine: the leaf in front of which its workgroups on the chain's XCD are gone (-1: they stay)
    int64_t local_rows = 0;       // tallest XCD-local leaf (local_leaf_rows without the schedule's cap)
    bool tail_overlap = false;    // column-major entry: the layout change of the columns right of tail_w0 overlaps the first panel
    int64_t tail_w0 = 0;
    bool host_engine = false;     // host entry through the engine (getrf_host_engine)
    bool host_early = false;      // host entry: finished block rows travel back early (getrf_host)
};

// measured on MI355X (bench.py --blocksize sweep): the knee moves right with the matrix size
// (512 from 11265 columns on: where the update engine, which wants 512-wide block columns, starts to win -- N=11264 38.4 vs 38.6 ms at 256
// through the streams, N=12288 41.5 vs 43.5, N=10240 33.8 vs 32.9: round 6)
inline int64_t default_blocksize(int64_t mn)
{
    return mn < 1024 ? -1 : (mn <= 11264 ? 256 : (mn <= 16384 ? 512 : (mn <= 24576 ? 1024 : 2048)));
}

// The persistent update engine (engine.hip) can serve a factorization when the column blocks start on tile boundaries, the
// workspace allows 16-byte accesses and nothing else wants to follow the schedule from the host (the host entry's progress hook).
inline bool engine_usable(const SchedIn& in, int64_t W)
{
    const int64_t VW = 16 / (int64_t)in.esize;
    return W % 128 == 0 && in.roff == 0 && in.aligned16 && in.ld % VW == 0 &&
           in.m < (int64_t)1 << 30 && in.n < (int64_t)1 << 30 && (in.n + W - 1) / W <= ENG_MAX_CB && !in.progress && !in.mask_failed &&
           (!in.tune.schedule_events || in.tune.engine_replay) && in.num_cus == 256 &&
           (in.m >= in.n || in.m % W == 0);   // (a fat matrix whose last panel ends inside a column block: the columns right of it in that block)
}

inline SchedPlan plan_schedule(const SchedIn& in)
{
    const Tune& t = in.tune;
    const int64_t m = in.m, n = in.n, mn = std::min(m, n);
    SchedPlan p;
    if (mn <= 0) return p;
    const bool default_bs = in.blocksize == 0;
    const int64_t bs = default_bs ? default_blocksize(mn) : in.blocksize;
    if (in.entry == ENTRY_HOST) {
        // through the engine: the way in overlaps the factorization (pivoted only: an unpivoted factorization shows the engine's summation
        // order in visibly other digits and measures slower through it, N=16384: 68.9 vs 64.1 ms; its host entry stays bit-identical to the
        // device entry).  Every block column goes through the engine there: the caller feeds the matrix in behind the streams' back.
        SchedIn e = in;
        e.entry = ENTRY_HOST_ENGINE;
        e.progress = false;
        p = plan_schedule(e);
        p.host_engine = in.pivot && t.engine_host && !t.schedule_events && t.host_early_out >= 64 && mn >= 8192 && m >= n &&
                        p.path == RFLU_PATH_HIP_ENGINE;
        if (p.host_engine) return p;
        // otherwise staged through the column-major entry; finished block rows go home early (RFLU_HOST_EARLY_OUT=0: after everything)
        const bool early = t.host_early_out >= 64 && !in.prof && in.num_cus == 256 && mn >= 8192 && bs > 0 && bs < mn;
        SchedIn c = in;
        c.entry = ENTRY_CM;
        c.progress = early;
        p = plan_schedule(c);
        p.host_early = early;
        return p;
    }
    p.local_rows = local_leaf_rows(t, in.esize);
    if (in.entry == ENTRY_CM) {   // the first block column's layout change on the caller's stream, the rest on the update stream
        p.tail_w0 = bs > 0 ? (bs + NB - 1) / NB * NB : 0;
        p.tail_overlap = t.tail_overlap != 0 && !in.prof && in.num_cus == 256 && mn >= 12288 && p.tail_w0 > 0 && p.tail_w0 < mn &&
                         n - p.tail_w0 >= 4096;
    }
    if (bs < 0 || bs >= mn) {
        p.path = RFLU_PATH_HIP_RECURSIVE;
        return p;
    }
    p.Wb = (bs + NB - 1) / NB * NB;
    if (in.prof || in.num_cus != 256) {   // the CU reservation of the two-stream schedule is laid out for 8 x 32 CUs
        p.path = RFLU_PATH_HIP_BLOCKED;
        return p;
    }
    p.path = RFLU_PATH_HIP_LOOKAHEAD;
    p.two_stream = true;
    // tall block columns (update-bound): factor_lookahead; from the first panel of at most lw_rows rows on: factor_leafwise.
    // RFLU_LEAFWISE=0 keeps the lookahead schedule to the end.  rocprofv3 --pmc runs ONE kernel at a time across all queues: a gate
    // kernel waiting for another stream's kernel would never see it start, so a counter-collection run (RFLU_SCHEDULE=events) takes the
    // lookahead schedule, whose cross-stream edges are hipEvents, to the end.  The leaf-wise / engine schedules hand work between streams
    // through device-side gates: only with real CU-masked streams.
    const bool leafwise = t.leafwise && !(t.schedule_events && !t.engine_replay) && !in.mask_failed;
    // Large matrices with the default block width: WIDE block columns (1024 / 2048: the bulk GEMM at K >= 1024 runs at 0.88-0.91 of
    // the MFMA peak instead of 0.83) while the update is the bottleneck, i.e. up to the last `narrow_cols` columns; those are
    // factored the way a matrix of that size is -- 512-wide block columns, leaf-wise from 8192 rows on -- because there the
    // chain of panels sets the pace and a 2048-column recursion on the critical path is what costs.
    if (default_bs && t.wide_narrow && p.Wb > 512 && mn >= 20480) {
        const int64_t narrow_cols = std::max<int64_t>(t.narrow_cols, 2048);
        p.W_wide = p.Wb;
        p.Wb = 512;
        p.wide_end = std::max<int64_t>(mn - narrow_cols, 0) / p.W_wide * p.W_wide;
    }
    const int64_t Wb = p.Wb;
    p.nblk = (mn + Wb - 1) / Wb;
    p.b_switch = p.nblk;
    // (block columns wider than 512 make the side stream's per-leaf window -- up to 2 W columns at K = 64 -- too much work to
    //  finish within one leaf: N=32768 at W=2048 is 0.8 % (Float64) / 5 % (Float32) slower leaf-wise, so those stay as they were)
    if (leafwise && Wb >= 2 * NB && Wb <= 512) {
        // Float64: panels at most this tall are the bottleneck of their block column (N=16384: 84.8 ms at 7168-8192, 85.4 at
        // 9216, 88.3 for the whole matrix); Float32's faster GEMM leaves the panel the bottleneck everywhere (61.7 vs 64.5 ms)
        int64_t lw_rows = in.esize == 8 ? 8192 : 16384;   // 16384 rows = 32 workgroups: the most the 32 reserved CUs take
        if (t.leafwise_rows >= 0) lw_rows = t.leafwise_rows;
        lw_rows = std::min<int64_t>(lw_rows, 32 * (int64_t)PANEL_THREADS);
        p.b_switch = m <= lw_rows ? 0 : std::min(p.nblk, (m - lw_rows + Wb - 1) / Wb);
    }
    // the block column in front of the leaf-wise part has to be a narrow one (factor_leafwise finds its events by number)
    if (p.W_wide > 0 && p.b_switch < p.nblk)
        p.wide_end = std::min(p.wide_end, std::max<int64_t>(p.b_switch - 1, 0) * Wb / p.W_wide * p.W_wide);
    // The update engine serves the block columns whose panels are taller than engine_rows (the leaf-wise schedule from block column 0,
    // its side / update streams replaced by the engine); below that the streams and the XCD-local leaves take over.  Where asked for
    // (RFLU_ENGINE=1, the host entry) or, by default, where it measures faster than the streams: with pivoting at the default block
    // width of 512, i.e. more than 11264 columns (N=16384 Float64: 71.5 vs 75 ms, Float32 55.3 vs 58.8; N=12288: 41.5 vs 43.5 through
    // the streams at 256, Float32 36.9 vs 38.4; NoPivot at N=16384: 68.9 vs 64.1, the streams stay; below, at 256-wide block columns,
    // the streams win: N=10240 32.9 vs 33.8, N=8192 24.0 vs 24.9).  A Float32 pivot search may answer another summation order with
    // another (equally valid) pivot sequence from a near-tie on -- between the stream schedules too: tests hold
    // Float32 to the residual and a floor of equal leading pivots, not to the bits of another schedule.
    const bool host_mode = in.entry == ENTRY_HOST_ENGINE;
    const bool eng_wanted = host_mode || t.engine == 1 || t.engine_replay ||
                            (t.engine < 0 && in.pivot && default_bs && Wb == 512 && mn > 11264 && m >= n);
    if (eng_wanted && leafwise && Wb >= 2 * NB && Wb <= 512 && p.W_wide == 0 && m <= 32 * (int64_t)PANEL_THREADS && engine_usable(in, Wb)) {
        const int64_t er = host_mode ? 0 : std::max<int64_t>(t.engine_rows, 0);   // (host entry: every block column through the engine)
        p.eng_end = m <= er ? 0 : std::min(p.nblk, (m - er + Wb - 1) / Wb);
    }
    if (p.eng_end == 0) return p;
    p.path = RFLU_PATH_HIP_ENGINE;
    p.b_switch = p.nblk;
    p.eng_wc = (t.engine_wc >= 128 && t.engine_wc % 128 == 0 && Wb % t.engine_wc == 0) ? t.engine_wc : (int)Wb;
    if ((n + p.eng_wc - 1) / p.eng_wc > ENG_MAX_CB) p.eng_wc = (int)Wb;
    p.eng_ahead = std::max(1, std::min(t.engine_ahead, 4));
    // Engine to the end: from the first panel of at most `rows` rows on the chain wants its XCD-local leaves back (worth 1.2 ms at
    // N=16384), and the engine has little left to do: its workgroups on the chain's XCD retire two leaves earlier, the first such
    // leaf waits until they are gone (RFLU_ENGINE_RETIRE=0: they stay, every leaf any-placement).  RFLU_ENGINE_RETIRE = the panel height
    // from which on, at most what the XCD-local leaf is used for anyway; default 4096 rows, 2048 from 16384 rows on, where the end is bound
    // by the engine's throughput and its workgroups are worth more than the faster leaves for longer (N=16384 75.2-76.5 ms at 4096 /
    // 74.4-75.2 at 2048, N=12288 44.8 / 47.1, N=8192 25.8 / 27.7)
    const int64_t retire_rows = t.engine_retire >= 0 ? t.engine_retire : (m >= 16384 ? 2048 : 4096);
    const int64_t rows = std::min<int64_t>(p.local_rows, retire_rows);
    if (retire_rows > 0 && p.eng_end >= p.nblk && !host_mode && !t.engine_replay && in.pivot && in.panel_local == 2 && !in.coop_launch &&
        rows >= 1024 && m > rows + 4 * NB)
        p.eng_retire_leaf = (m - rows + NB - 1) / NB;   // first leaf whose panel has at most `rows` rows
    return p;
}

}  // namespace rflu
