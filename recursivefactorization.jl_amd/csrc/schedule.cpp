// schedule.cpp -- how one matrix is factored on one GPU: the Toledo recursion (Fact<T>), the lookahead and the leaf-wise stream schedules,
// the start-up of the persistent update engine (engine.hip), and the device entries getrf_rm / getrf_cm_dev that choose among them by
// the plan of schedule_plan.hpp.
//
// Host control flow restates the reference's src/lu.jl:
//   lu!(A, ipiv, pivot, thread; ...)  (:97-130)  -> rflu_getrf_* : NoPivot identity fill (:111-113), recursion, info
//   _recurse! fat-matrix tail         (:148-154) -> getrf_rm(): TRSM of the columns right of the square part
//   reckernel!                        (:189-263) -> rec(): factor left half, TRSM, Schur GEMM, factor right half
// MI355X-specific re-scheduling (results unchanged):
//   * leaves are 64 columns wide (one cooperative panel kernel, panel.hip) and the split is on 64-column boundaries
//     (the reference's nsplit, :158-162, rounds to 64 BYTES of column; SURVEY.md a2: "GPU picks its own split");
//   * the interchanges of a leaf are applied to ALL other columns right after the leaf (one full-width, perfectly
//     parallel laswp launch) instead of level by level (:233, :246) -- the same swaps in the same order on data that
//     nothing touches in between, hence identical results with log2(N/64) times fewer dependent launches;
//   * ipiv is written with global 1-based rows directly (the reference reaches the same values through P2 .+= n1,
//     :256-260) and info is the global index of the first zero pivot (the reference's offset fix-up :248-255).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>

#include "driver.hpp"
#include "engine.hpp"

namespace rflu {

// error flags raised by the cooperative kernels (info_dev[1], copied to info_pinned[1] by the caller)
int panel_flags_status(Handle* h)
{
    const int64_t f = h->info_pinned[1];
    if (f & 2) {
        set_error("a workgroup of the XCD-local panel kernel ran on an unexpected XCD; results discarded "
                  "(set RFLU_PANEL_LOCAL=0 to use the placement-independent kernel)");
        return RFLU_ERR_PLACEMENT;
    }
    if (f != 0 && h->eng_state && env_str("RFLU_ENGINE_DUMP")) {   // debugging: where the engine and the chain stood when somebody gave up
        EngState es;
        unsigned long long gate[3] = {0, 0, 0};
        (void)hipMemcpy(&es, h->eng_state, offsetof(EngState, cb) + 16 * sizeof(EngCB), hipMemcpyDeviceToHost);
        for (int i = 0; i < 3; ++i) (void)hipMemcpy(&gate[i], h->gate_ptr[i], 8, hipMemcpyDeviceToHost);
        fprintf(stderr, "[rflu] engine dump: flags 0x%llx gates %llu %llu %llu arrived %llu remaining %llu abort %llu epoch %llu\n", (unsigned long long)f, gate[0], gate[1], gate[2],
                es.arrived, es.remaining, es.abort, es.epoch);
        for (int c = 0; c < 16; ++c)
            fprintf(stderr, "   cb %2d: claim %llx done %llx lclaim %llx ldone %llu prog %llu leftdone %llx lprog %llu bigdone %llu\n", c, es.cb[c].claim, es.cb[c].done, es.cb[c].lclaim,
                    es.cb[c].ldone, es.cb[c].prog, es.cb[c].leftdone, es.cb[c].lprog, es.cb[c].bigdone);
    }
    if (f != 0) {
        set_error("cooperative panel kernel timed out waiting for a peer workgroup (flags 0x%llx: 1 = a leaf / gate, 16 = the engine idle, 32 = a wait for the engine, 64 = the XCD-local leaf)", (unsigned long long)f);
        return RFLU_ERR_TIMEOUT;
    }
    return RFLU_OK;
}

// the inputs of plan_schedule (schedule_plan.hpp) as the handle has them now
SchedIn sched_in(const Handle* h, int64_t m, int64_t n, size_t esize, int pivot, int64_t blocksize, int entry, bool aligned16, int64_t ld)
{
    SchedIn in;
    in.m = m; in.n = n; in.esize = esize; in.pivot = pivot; in.blocksize = blocksize; in.entry = entry;
    in.tune = h->tune;
    in.num_cus = h->num_cus; in.prof = h->prof || h->prof_one_stream; in.mask_failed = h->mask_failed; in.progress = (bool)h->progress;
    in.panel_local = h->panel_local; in.coop_launch = h->coop_launch;
    in.aligned16 = aligned16; in.ld = ld;
    return in;
}

template <typename T>
struct Fact {
    Handle* h;
    T* R;
    int64_t ld, m, n;  // full matrix: m rows, n columns
    int64_t* ipiv;
    int pivot;
    int64_t sw_lo = 0, sw_hi = -1;  // column range that receives a leaf's interchanges right away ([0, n) by default)
    int64_t roff = 0;               // row of the diagonal minus its column (non-zero for a block column of a slab)
    hipEvent_t tail = nullptr;      // columns right of the first block column become valid with this event (getrf_cm_dev)

    T* linv_at(int64_t row) const { return static_cast<T*>(h->linv) + (row / NB) * NB * NB; }

    // leaf: rows [c0+roff, m), columns [c0, c0+w): cooperative panel + the interchanges on every other column
    int leaf(int64_t c0, int64_t w)
    {
        const int64_t r0 = c0 + roff;
        RFLU_TRY(launch_panel<T>(h, R, ld, m, r0, c0, w, ipiv, pivot));
        const int64_t hi = sw_hi < 0 ? n : sw_hi;
        // one launch: the leaf's interchanges on the other columns + the inverse of its diagonal block (fused TRSMs)
        if (pivot) RFLU_TRY(launch_laswp2<T>(h, R, ld, sw_lo, c0 - sw_lo, c0 + w, hi - (c0 + w), r0 / NB, r0 / NB + 1, w,
                                             R + r0 * ld + c0, linv_at(r0)));
        // (NoPivot: launch_panel has already inverted the diagonal block into linv_at(r0), next to inv(U11) for its own rows)
        return RFLU_OK;
    }

    // reckernel! (src/lu.jl:189-263) on columns [c0, c1), rows [c0+roff, m)
    int rec(int64_t c0, int64_t c1)
    {
        const int64_t w = c1 - c0;
        if (w <= 0) return RFLU_OK;
        if (w <= NB) return leaf(c0, w);
        const int64_t leaves = (w + NB - 1) / NB;
        const int64_t n1 = ((leaves + 1) / 2) * NB;
        const int64_t cm = c0 + n1;
        RFLU_TRY(rec(c0, cm));
        T* A11 = R + (c0 + roff) * ld + c0;
        T* A12 = R + (c0 + roff) * ld + cm;
        T* A21 = R + (cm + roff) * ld + c0;
        T* A22 = R + (cm + roff) * ld + cm;
        RFLU_TRY(trsm_rec<T>(h, n1, c1 - cm, A11, ld, A12, ld, linv_at(c0 + roff)));              // src/lu.jl:235
        RFLU_TRY(launch_gemm<T>(h, m - (cm + roff), c1 - cm, n1, A21, ld, A12, ld, A22, ld));     // src/lu.jl:240
        return rec(cm, c1);
    }
};

// The recursion on columns [c0, c0 + w) of an m-row slab, diagonal at (r0, c0), interchanges confined to those columns (a block column
// of the multi-GPU path, and what rflu_panel_rm_* factors)
template <typename T>
int panel_rec(Handle* h, int64_t m, int64_t r0, int64_t c0, int64_t w, T* R, int64_t ld, int64_t* ipiv, int pivot)
{
    Fact<T> f{h, R, ld, m, c0 + w, ipiv, pivot};
    f.sw_lo = c0; f.sw_hi = c0 + w; f.roff = r0 - c0;
    return f.rec(c0, c0 + w);
}

// rflu_panel_rm_*_dev: wide panels are factored by the same Toledo recursion as the single-GPU path
template <typename T>
int panel_rm(Handle* h, int64_t m, int64_t r0, int64_t c0, int64_t w, T* R, int64_t ld, int64_t* ipiv, int pivot, int64_t* info)
{
    if (info == nullptr || w < 0 || r0 < 0 || c0 < 0 || m < r0 + w) { set_error("panel: bad arguments"); return RFLU_ERR_ARG; }
    RFLU_TRY(ensure_bookkeeping(h, m));
    RFLU_HIP(hipMemsetAsync(h->info_dev, 0, 2 * sizeof(int64_t), h->stream));
    if (!pivot && ipiv) RFLU_TRY(launch_iota_ipiv(h, ipiv, r0, w));
    RFLU_TRY(panel_rec<T>(h, m, r0, c0, w, R, ld, ipiv, pivot));
    RFLU_HIP(hipMemcpyAsync(h->info_pinned, h->info_dev, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    RFLU_HIP(hipStreamSynchronize(h->stream));
    RFLU_TRY(panel_flags_status(h));
    *info = h->info_pinned[0];
    return RFLU_OK;
}

// rflu_laswp_rm_*_dev: the interchanges ipiv[k0, k1) on columns [c0, c0 + ncols)
template <typename T>
int laswp_rm(Handle* h, T* R, int64_t ld, int64_t m, int64_t c0, int64_t ncols, const int64_t* ipiv, int64_t k0, int64_t k1)
{
    if (k0 % NB != 0 || k1 < k0) { set_error("laswp: k0 must be a multiple of 64"); return RFLU_ERR_ARG; }
    RFLU_TRY(ensure_bookkeeping(h, std::max(m, k1)));
    RFLU_TRY(launch_perm_build(h, ipiv, k0, k1, m));
    return launch_laswp<T>(h, R, ld, c0, ncols, k0 / NB, (k1 + NB - 1) / NB);
}
// ---- cost model of the lookahead schedule (microseconds; calibrated on MI355X) ----
static double model_panel_us(int64_t rows, int64_t W)
{
    const double G = double((rows + PANEL_THREADS - 1) / PANEL_THREADS);
    const double step = 2.6 + 0.025 * G;                      // one pivot step of the cooperative kernel
    return double(W) * step + double(W) / NB * 70.0           // + per-leaf interchanges / solves / launches
           + double(rows) * double(W) * double(W) / 30e6;     // + the recursion's own GEMMs (small K, ~30 TFLOP/s)
}
static double model_gemm_flops_per_us(int64_t K, int cus, size_t elem)
{
    const double tf = (K >= 2048 ? 64.0 : K >= 1024 ? 60.0 : K >= 512 ? 55.0 : 50.0) * (elem == 4 ? 1.6 : 1.0);
    return tf * 1e6 * double(cus) / 256.0;
}

// Right-looking over block columns of width W with one block column of lookahead (two streams).
//   P (h->stream, all CUs)      : panel_b -> restB_{b-1} -> evP[b] -> [wait evU1[b-1]] next_b (update of block column b+1)
//                                 -> panel_{b+1} ...
//   U (CU-masked update stream) : [wait evP[b]] left swaps_b -> rest_b.part1 (block column b+2) -> evU1[b] -> restA_b
// rest_b (the update of everything right of block column b+1) is split by columns: restA_b is sized by the cost model to
// take as long as P's next_b + panel_{b+1}, and runs next to them on the CUs the mask leaves it; what does not fit in
// that time (restB_b: the early, update-bound block columns and every tall panel) follows panel_{b+1} on P with the
// whole GPU.  The mask reserves ceil(panel workgroups / 32) * 32 CUs, chosen per block column.
// Every block column receives the same operations in the same order as in the recursion; only independent pieces
// overlap in time, so the factors are those of the one-stream path.
// b_end < number of block columns: stop after block column b_end-1 (its update issued, block column b_end brought up to date on
// P) and hand over to factor_leafwise; *U_last = the update stream of that block column.
template <typename T>
static int factor_lookahead(Fact<T>& f, int64_t W, int64_t b_end, hipStream_t* U_last, int64_t W_wide = 0, int64_t wide_end = 0)
{
    // Block columns: [0, wide_end) in pieces of W_wide (a multiple of W; the update-bound part of a large matrix, whose bulk GEMM
    // wants the deeper K), the rest in pieces of W.  A block column is numbered by its first column / W ("id"): events, gate
    // values and b_end use that number, so the narrow part -- and factor_leafwise behind it -- see the numbering they would
    // see without a wide part.
    Handle* h = f.h;
    // tuning knobs (Tune): split_share = how much of what is left after the modelled time stays on the update stream;
    // max_reserve: taller panels (> 64 workgroups) take too many CUs from the update: one stream instead; min_reserve: least number
    // of CUs kept away from the update stream; split_scale scales the modelled critical-path time (0 = no split)
    const int min_reserve = (h->tune.min_reserve >= 32 && h->tune.min_reserve <= 224 && h->tune.min_reserve % 32 == 0) ? h->tune.min_reserve : 32;
    const double split_scale = h->tune.split_scale, split_share = h->tune.split_share;
    const bool split_all = h->tune.split_all != 0;
    const int max_reserve = h->tune.max_reserve;
    hipStream_t P = h->stream;
    const int64_t m = f.m, n = f.n, ld = f.ld, mn = std::min(m, n);
    T* R = f.R;
    if (W_wide <= W || wide_end <= 0) { W_wide = W; wide_end = 0; }
    wide_end = std::min(wide_end / W_wide * W_wide, mn);
    std::vector<int64_t> bstart;
    for (int64_t c = 0; c < mn; c += (c < wide_end ? W_wide : W)) bstart.push_back(c);
    bstart.push_back(mn);
    const int64_t nblk = (int64_t)bstart.size() - 1;            // block columns
    const int64_t nid = (mn + W - 1) / W;                       // ids
    auto id_of = [&](int64_t b) { return b >= nblk ? nid : bstart[b] / W; };
    auto width_of = [&](int64_t b) { return b < nblk ? bstart[b + 1] - bstart[b] : W; };
    hipEvent_t ev;
    // The critical path moves between the caller's stream and a stream confined to the reserved CUs (get_pstream); h->stream
    // follows it, and is put back on every way out of this function.
    struct Restore { Handle* h; hipStream_t s; ~Restore() { h->stream = s; } } restore{h, h->stream};
    const hipStream_t userS = h->stream;
    // Confining the critical path to the reserved CUs while the update is the bottleneck: round 2 measured +1.3 ms in its favour,
    // round 3 -2.4 ms against it with all four streams on pipes of their own (validate_queues; without that a fourth stream may share
    // a pipe with one of the other three, which costs 25-60 %): off unless RFLU_CONFINE_ROWS asks for it.
    const int64_t confine_rows = h->tune.confine_rows;
    auto move_P = [&](hipStream_t to, int64_t b) -> int {
        if (to == P) return RFLU_OK;
        hipEvent_t e0;
        RFLU_TRY(get_event(h, 4 * id_of(b) + 0, &e0));
        RFLU_HIP(hipEventRecord(e0, P));
        RFLU_HIP(hipStreamWaitEvent(to, e0, 0));
        P = to;
        h->stream = to;   // lasting: the critical path has moved (restored by `restore`)
        return RFLU_OK;
    };

    auto update = [&](hipStream_t st, int64_t j0, int64_t jb, int64_t c0, int64_t c1, LaswpGate gate = LaswpGate{},
                      GemmSignal sig = GemmSignal{}) -> int {
        // apply block column [j0, j0+jb) to columns [c0, c1): interchanges, block-row solve, Schur update
        // gate: hold the first launch until another stream's counter is reached; sig: publish when the first columns are done
        if (c1 <= c0) return RFLU_OK;
        OnStream on(h, st);
        const int64_t je = j0 + jb;
        if (f.pivot) RFLU_TRY(launch_laswp2<T>(h, R, ld, c0, c1 - c0, 0, 0, j0 / NB, (je + NB - 1) / NB, 0, nullptr, nullptr, gate));
        else if (gate.wait_flag) RFLU_TRY(launch_gate_wait(h, gate.wait_flag, gate.wait_val));
        RFLU_TRY(trsm_rec<T>(h, jb, c1 - c0, R + j0 * ld + j0, ld, R + j0 * ld + c0, ld, f.linv_at(j0)));
        if (m > je) RFLU_TRY(launch_gemm<T>(h, m - je, c1 - c0, jb, R + je * ld + j0, ld, R + j0 * ld + c0, ld, R + je * ld + c0, ld, sig));
        return RFLU_OK;
    };
    // While the update stream is the bottleneck, block column b+2 is not updated by a launch sequence of its own (interchanges,
    // solves and a 496-tile GEMM that fills 1.1 rounds of the 448 workgroup slots: ~450 us per block column at N=16384) but as the
    // FIRST tile columns of the one bulk update; the GEMM publishes a gate when those tiles are done and the critical path waits
    // on that gate instead of an event.
    int64_t merge_rows = h->tune.merge_rows >= 0 ? h->tune.merge_rows : (sizeof(T) == 8 ? 8192 : (int64_t)1 << 40);
    if (h->tune.schedule_events) merge_rows = (int64_t)1 << 40;   // RFLU_SCHEDULE=events: no device-side gates (see getrf_rm)
    {   // the gate needs P and U to run concurrently: only with a real CU-masked update stream (create it now to find out)
        hipStream_t probe;
        RFLU_TRY(get_ustream(h, 32, &probe));
        if (h->mask_failed) merge_rows = (int64_t)1 << 40;
    }
    const unsigned long long ubase = h->gate_epoch;
    h->gate_epoch += (unsigned long long)nid + 2;
    auto uval = [&](int64_t b) { return ubase + (unsigned long long)id_of(b) + 1; };
    bool prev_merged = false;

    // events: 4b+1 = evP[b], 4b+2 = evU1[b], 4b+3 = evUend[b]
    hipStream_t Uprev = nullptr;      // update stream of the previous overlapped block column
    int64_t uend_prev = -1;           // its id (evUend recorded), -1: none
    bool prev_overlapped = false;
    struct { bool valid = false; int64_t j0 = 0, jb = 0, c0 = 0; int64_t need_uend = -1; } pend;  // restB of block b-1

    auto flush_pending = [&]() -> int {
        if (!pend.valid) return RFLU_OK;
        if (pend.need_uend >= 0) {  // its columns were last written by restA of the block column before
            hipEvent_t e2;
            RFLU_TRY(get_event(h, 4 * pend.need_uend + 3, &e2));
            RFLU_HIP(hipStreamWaitEvent(P, e2, 0));
        }
        pend.valid = false;
        return update(P, pend.j0, pend.jb, pend.c0, n);
    };

    for (int64_t b = 0; b < nblk && id_of(b) < b_end; ++b) {
        const int64_t j0 = bstart[b], jb = width_of(b), je = j0 + jb;
        const bool last_here = !(b + 1 < nblk && id_of(b + 1) < b_end);   // the next block column is somebody else's (or there is none)
        {
            const int64_t g_b = panel_plan_wgs(h, m - j0, sizeof(T), f.pivot);
            const int res_b = std::max<int>(min_reserve, int((std::max<int64_t>(g_b, 1) + 31) / 32 * 32));
            hipStream_t to = userS;
            if (b > 0 && prev_overlapped && m - j0 >= confine_rows && res_b == 32)   // taller panels: restB needs the whole GPU
                RFLU_TRY(get_pstream(h, res_b, &to));
            RFLU_TRY(move_P(to, b));
        }
        // ---- panel b on P: Toledo recursion on the block column, interchanges confined to its own columns ----
        f.sw_lo = j0;
        f.sw_hi = je;
        RFLU_TRY(f.rec(j0, je));
        if (b == 0 && f.tail) {   // everything after the first panel may touch the columns whose layout change ran next to it
            RFLU_HIP(hipStreamWaitEvent(P, f.tail, 0));
            f.tail = nullptr;
        }
        RFLU_TRY(flush_pending());                                   // restB_{b-1}: whole GPU, after the panel
        // the panel that will run next to this block column's update is panel b+1
        const int64_t rows_next = m - je;
        const int64_t g_next = panel_plan_wgs(h, rows_next, sizeof(T), f.pivot);
        int reserve = std::max<int>(min_reserve, int((std::max<int64_t>(g_next, 1) + 31) / 32 * 32));
        // RFLU_SWAP_LATE (default on): the last block column in front of a leaf-wise part that starts swapped sends its update to the
        // 192-CU stream, so that the 224-CU stream is free to be the side stream of the first leaf-wise block column (factor_leafwise)
        // (RFLU_SWAP_SU overrides factor_leafwise's stream assignment: only its "swapped behind a lookahead part" mode wants this move)
        const bool swapped_at_handover = h->tune.swap_su >= 0 ? h->tune.swap_su == 2 : h->tune.swap_late != 0;
        if (swapped_at_handover && reserve == 32 && last_here && b_end < nid && rows_next <= h->tune.swap_rows) reserve = 64;
        if (reserve > std::min(max_reserve, 224)) {
            // the next panel needs (almost) the whole GPU: run this block column on one stream
            if (uend_prev >= 0) {
                RFLU_TRY(get_event(h, 4 * uend_prev + 3, &ev));
                RFLU_HIP(hipStreamWaitEvent(P, ev, 0));
                uend_prev = -1;
            }
            if (f.pivot && j0 > 0) RFLU_TRY(launch_laswp<T>(h, R, ld, 0, j0, j0 / NB, (je + NB - 1) / NB));
            RFLU_TRY(update(P, j0, jb, je, n));
            prev_overlapped = false;
            prev_merged = false;
            Uprev = nullptr;
            continue;
        }
        hipStream_t U;
        RFLU_TRY(get_ustream(h, reserve, &U));
        RFLU_TRY(get_event(h, 4 * id_of(b) + 1, &ev));
        RFLU_HIP(hipEventRecord(ev, P));
        RFLU_HIP(hipStreamWaitEvent(U, ev, 0));
        if (Uprev && Uprev != U && uend_prev >= 0) {                 // a different mask: order the two update streams
            RFLU_TRY(get_event(h, 4 * uend_prev + 3, &ev));
            RFLU_HIP(hipStreamWaitEvent(U, ev, 0));
        }
        // ---- U: interchanges on the finished columns to the left ----
        if (f.pivot && j0 > 0) {
            OnStream on(h, U);
            RFLU_TRY(launch_laswp<T>(h, R, ld, 0, j0, j0 / NB, (je + NB - 1) / NB));
        }
        if (je >= n) {
            RFLU_TRY(get_event(h, 4 * id_of(b) + 3, &ev));
            RFLU_HIP(hipEventRecord(ev, U));
            uend_prev = id_of(b);
            Uprev = U;
            break;
        }
        const int64_t n1e = std::min(je + width_of(b + 1), n);                              // end of block column b+1
        const int64_t n2e = std::min(n1e + width_of(b + 2), n);                             // end of block column b+2
        // ---- P: next block column (needs rest_{b-1}.part1, which updated exactly these columns).  Handing all but its
        // first leaf to U (and gating P's second leaf on it) was measured slower: U's in-order queue is still busy with
        // rest_{b-1} in the early, update-bound block columns.
        LaswpGate pgate;
        if (b > 0 && prev_overlapped) {
            if (prev_merged) {
                pgate.wait_flag = h->gates + 3;
                pgate.wait_val = uval(b - 1);
                pgate.info = h->info_dev;
            } else {
                RFLU_TRY(get_event(h, 4 * id_of(b - 1) + 2, &ev));
                RFLU_HIP(hipStreamWaitEvent(P, ev, 0));
            }
        }
        RFLU_TRY(update(P, j0, jb, je, n1e, pgate));
        // ---- U: block column b+2 first (the next `next`), then as much of the rest as fits next to P's work ----
        const bool merged = m - je >= merge_rows && reserve == 32 && jb >= 256 && n2e > n1e && m > je &&
                            !(b_end < nid && last_here) && b + 1 < nblk;
        if (!merged) {
            RFLU_TRY(update(U, j0, jb, n1e, n2e));
            RFLU_TRY(get_event(h, 4 * id_of(b) + 2, &ev));
            RFLU_HIP(hipEventRecord(ev, U));
        }
        int64_t cA = n;                                                                      // restA = [n2e, cA)
        // With the minimal reservation the masked stream keeps 7/8 of the GPU and a split cannot win more than ~1 %
        // (measured: nothing); it pays for the tall panels, whose reservation takes a quarter to half of the CUs.
        if (split_scale > 0 && m > je && (reserve > 32 || split_all)) {
            const double rateU = model_gemm_flops_per_us(jb, 256 - reserve, sizeof(T));
            const double rateP = model_gemm_flops_per_us(jb, 256, sizeof(T));
            const double col_flops = 2.0 * double(m - je) * double(jb);                      // per trailing column
            const double tP = split_scale * ((je < mn ? model_panel_us(m - je, std::min(width_of(b + 1), mn - je)) : 0.0)
                                             + col_flops * double(n1e - je) / rateP);
            const double colsA = tP * rateU / col_flops;                                     // columns U finishes in tP
            const int64_t left = n - n1e;
            // what is left after tP is shared by both streams; below one GEMM tile column it is not worth a launch
            int64_t a = int64_t(colsA) / 128 * 128;
            a = std::max<int64_t>(a, n2e - n1e);
            if (left - a >= 512)
                cA = n1e + a + int64_t(split_share * double(left - a) * double(256 - reserve) / 512.0) / 128 * 128;
        }
        if (merged) {
            GemmSignal sig;
            sig.first_cols = n2e - n1e;
            sig.flag = h->gates + 3;
            sig.val = uval(b);
            sig.cnt = reinterpret_cast<unsigned*>(h->gates + 5);
            RFLU_TRY(update(U, j0, jb, n1e, cA, LaswpGate{}, sig));
        } else {
            RFLU_TRY(update(U, j0, jb, n2e, cA));
        }
        prev_merged = merged;
        RFLU_TRY(get_event(h, 4 * id_of(b) + 3, &ev));
        RFLU_HIP(hipEventRecord(ev, U));
        if (cA < n) {
            pend.valid = true;
            pend.j0 = j0;
            pend.jb = jb;
            pend.c0 = cA;
            pend.need_uend = uend_prev;   // restA_{b-1} may have written columns right of cA
        }
        uend_prev = id_of(b);
        Uprev = U;
        prev_overlapped = true;
        if (h->progress) RFLU_TRY(h->progress(j0));   // block column b-1's last piece (restB) went out after panel b: rows above j0 are settled
    }
    RFLU_TRY(flush_pending());
    if (h->progress) RFLU_TRY(h->progress(std::min(std::min(nid, b_end) * W, mn)));
    RFLU_TRY(move_P(userS, nblk));
    f.sw_lo = 0;
    f.sw_hi = -1;
    if (U_last) *U_last = Uprev;
    if (b_end < nid) return RFLU_OK;   // factor_leafwise goes on from here and joins at its end
    // join: P continues only after U has drained
    if (uend_prev >= 0) {
        RFLU_TRY(get_event(h, 4 * uend_prev + 3, &ev));
        RFLU_HIP(hipStreamWaitEvent(P, ev, 0));
    }
    return RFLU_OK;
}

// the engine's state block (device) and the pinned host image of its initial value: both or neither (a half-made pair would
// have the next call write its image through a null pointer); freed by rflu_destroy
int ensure_engine_state(Handle* h)
{
    if (h->eng_state && h->eng_host) return RFLU_OK;
    if (!h->eng_host) RFLU_HIP(hipHostMalloc(&h->eng_host, sizeof(EngState), hipHostMallocDefault));
    if (!h->eng_state) {
        if (hipMalloc(&h->eng_state, sizeof(EngState)) != hipSuccess) {
            (void)hipGetLastError();
            h->eng_state = nullptr;
            set_error("hipMalloc of the update engine's state failed");
            return RFLU_ERR_HIP;
        }
    }
    return RFLU_OK;
}

// ---- the persistent update engine (engine.hip): what factor_leafwise needs to start it ------------------------------------------------
static int wait_on(Handle* h, hipStream_t st, size_t idx)
{
    hipEvent_t e;
    RFLU_TRY(get_event(h, idx, &e));
    RFLU_HIP(hipStreamWaitEvent(st, e, 0));
    return RFLU_OK;
}
static int record_on(Handle* h, hipStream_t st, size_t idx)
{
    hipEvent_t e;
    RFLU_TRY(get_event(h, idx, &e));
    RFLU_HIP(hipEventRecord(e, st));
    return RFLU_OK;
}

// measurement only (RFLU_ENGINE_TRACE=1): the stamps the previous call's engine left in h->eng_trace_buf (leaf windows, workgroup time),
// on stderr.  The format is read by people and by scripts/.
static int engine_trace_report(Handle* h, int64_t nleaf, int64_t W)
{
    std::vector<long long> hs(4096 * 4 + 16);
    RFLU_HIP(hipMemcpy(hs.data(), h->eng_trace_buf, hs.size() * sizeof(long long), hipMemcpyDeviceToHost));
    double s01 = 0, s12 = 0, s23 = 0, sq = 0; int cnt = 0;
    for (int g = 1; g + 1 < (int)nleaf && g < 4095; ++g) {
        if (!hs[g * 4] || !hs[g * 4 + 3] || !hs[(g - 1) * 4 + 3]) continue;
        s01 += (hs[g * 4 + 1] - hs[g * 4]) / 100.0; s12 += (hs[g * 4 + 2] - hs[g * 4 + 1]) / 100.0; s23 += (hs[g * 4 + 3] - hs[g * 4 + 2]) / 100.0;
        sq += (hs[g * 4] - hs[(g - 1) * 4 + 3]) / 100.0; ++cnt;
    }
    if (cnt) fprintf(stderr, "[rflu] engine trace (previous call, %d leaf windows on their first column block): first claim -> stage 0 done %.1f us, -> first tile claimed %.1f, -> window complete %.1f; previous window complete -> first claim %.1f us\n", cnt, s01 / cnt, s12 / cnt, s23 / cnt, sq / cnt);
    {
        const long long* ac = hs.data() + 4096 * 4;
        const double tot = (double)(ac[0] + ac[1] + ac[2] + ac[3] + ac[4]);
        if (tot > 0)
            fprintf(stderr, "[rflu] engine workgroup time (previous call, %.1f workgroup-ms): block-column tiles %.1f %%, leaf-window tiles %.1f %%, strips + solves %.1f %%, deferred interchanges %.1f %%, between units %.1f %% (of which asleep with nothing eligible %.1f %%, count + publication behind a unit %.1f %%, scan / claim / acquire %.1f %%)\n",
                    tot / 1e5, 100.0 * ac[0] / tot, 100.0 * ac[1] / tot, 100.0 * ac[2] / tot, 100.0 * ac[3] / tot, 100.0 * ac[4] / tot, 100.0 * ac[5] / tot, 100.0 * ac[6] / tot, 100.0 * (ac[4] - ac[5] - ac[6]) / tot);
        if (tot > 0 && ac[15] > 0)   // the scan by itself, per call (= per unit), in microseconds
            fprintf(stderr, "[rflu] engine scan (previous call, %lld calls, %.2f sweeps per call), us per call: epoch / gate sample %.2f, exit words %.2f, claim words + choice %.2f, ticket %.2f, "
                            "scan of the deferred interchanges %.2f, acquire + hand-over %.2f; asleep %.2f\n",
                    ac[15], (double)ac[14] / ac[15], ac[8] / 100.0 / ac[15], ac[9] / 100.0 / ac[15], ac[10] / 100.0 / ac[15], ac[11] / 100.0 / ac[15], ac[12] / 100.0 / ac[15],
                    ac[13] / 100.0 / ac[15], ac[5] / 100.0 / ac[15]);
    }
    // leaf by leaf (RFLU_ENGINE_TRACE=first:count): when LEAF(g) was first claimed on the column block of its first columns (ms since LEAF(0)'s first
    // claim), its three phases, and how long that column block had been idle before (the engine waiting for the chain) -- for the LAST
    // leaf but one of a block column that column block is the NEXT block column's: the window the chain's last leaf waits for
    int tg0 = 40, tgn = 4;
    if (const char* e = env_str("RFLU_ENGINE_TRACE")) { if (strchr(e, ':')) sscanf(e, "%d:%d", &tg0, &tgn); }
    for (int g = std::max(tg0, 1); g < tg0 + tgn && g + 1 < (int)nleaf && g < 4095; ++g)
    {
        fprintf(stderr, "   leaf %d: first claim at %.3f ms | stage 0 %.1f us | to first tile %.1f | tiles %.1f | idle before %.1f", g, (hs[g * 4] - hs[0]) / 1e5,
                (hs[g * 4 + 1] - hs[g * 4]) / 100.0, (hs[g * 4 + 2] - hs[g * 4 + 1]) / 100.0, (hs[g * 4 + 3] - hs[g * 4 + 2]) / 100.0, (hs[g * 4] - hs[(g - 1) * 4 + 3]) / 100.0);
        const long long* n4 = hs.data() + (size_t)(2048 + g) * 4;   // the same leaf on the next block column's first column block
        if (g < 2048 && n4[0] && n4[3])
            fprintf(stderr, " || next block column: first claim at %.3f ms (%.1f us after the previous leaf's window there was complete) | stage 0 %.1f | to first tile %.1f | tiles %.1f",
                    (n4[0] - hs[0]) / 1e5, (n4[0] - n4[-1]) / 100.0, (n4[1] - n4[0]) / 100.0, (n4[2] - n4[1]) / 100.0, (n4[3] - n4[2]) / 100.0);
        fprintf(stderr, "\n");
        // behind the last leaf of a block column b: what stands between it and BIG(b) being complete on the column block the chain needs next
        const int LPBt = (int)(W / NB);
        if ((g + 1) % LPBt == 0 && g / LPBt < 512) {
            const int b = g / LPBt;
            const long long* bg = hs.data() + (size_t)(1024 + b) * 4;
            const long long* lf = hs.data() + (size_t)(1536 + b) * 4;
            const long long t0 = n4[0];   // LEAF(last leaf of b) first claimed on the next block column: the leaf has just been factored
            if (t0 && bg[0] && bg[3])
                fprintf(stderr, "   block column %d ends (its last leaf's window is claimed at +0): own deferred interchanges +%.0f .. +%.0f us | BIG(%d) on the first column block of block column %d: "
                                "stage 0 +%.0f .. +%.0f | tiles +%.0f .. +%.0f us\n",
                        b, (lf[0] - t0) / 100.0, (lf[1] - t0) / 100.0, b, b + 2, (bg[0] - t0) / 100.0, (bg[1] - t0) / 100.0, (bg[2] - t0) / 100.0, (bg[3] - t0) / 100.0);
        }
    }
    return RFLU_OK;
}

// measurement (rflu_profile_enable(2)): the engine kernel as ONE launch of the class the bulk GEMM reports under -- its flops are
// the Schur updates it performs (every operation's 2 M N K), its duration the whole residency, waiting included
// ... and its algorithmic bytes: per operation the panel pieces once (A: M x K, B: K x N), the Schur block in and out (2 M N), the
// solved block row in and out (2 K N), and the interchanges (two rows read + written per pivot and column: 4 per entry), the
// deferred ones on the finished columns to the left included
template <typename T>
static void engine_prof_counts(const EngGeo& geo, int64_t n, int64_t mn, int64_t W, int pivot, double* flops, double* bytes)
{
    double eng_flops = 0, eng_bytes = 0;
    for (int cb = 0; cb < geo.ncb; ++cb) {
        for (int k = 0; k < eng_nops(geo, cb); ++k) {
            const EngOp o = eng_op(geo, cb, k);
            if (o.nc <= 0) continue;
            const double M = (double)std::max(geo.m - (o.j0 + o.jb), 0), N = (double)o.nc, K = (double)o.jb;
            eng_flops += 2.0 * M * N * K;
            eng_bytes += sizeof(T) * (M * K + K * N + 2.0 * M * N + 2.0 * K * N + 0.5 * K * K + (pivot ? 4.0 * K * N : 0.0));
        }
        if (pivot && eng_pb(geo, cb) < geo.nbp) {   // left op 0 (on average half of the block column's pivots per strip) + the later block columns as a whole
            const double nc = (double)(std::min<int64_t>(n, (int64_t)(cb + 1) * geo.Wc) - (int64_t)cb * geo.Wc);
            const double later = (double)std::max<int64_t>(std::min<int64_t>((int64_t)geo.nbp * W, mn) - (int64_t)(eng_pb(geo, cb) + 1) * W, 0);
            eng_bytes += sizeof(T) * 4.0 * nc * (0.5 * (double)std::min<int64_t>(W, mn - (int64_t)eng_pb(geo, cb) * W) + later);
        }
    }
    *flops = eng_flops;
    *bytes = eng_bytes;
}

// Engine mode of factor_leafwise: the engine's initial state goes to the device on the caller's stream, the engine is launched on the
// 224-CU update stream *E behind it, and an event on *E marks its exit (evUend of its last block column).  gbase: the base of this
// factorization's leaf gate values.
template <typename T>
static int start_engine(Fact<T>& f, const SchedPlan& plan, unsigned long long gbase, hipStream_t* E_out, EngState** est_out, EngGeo* geo_out)
{
    Handle* h = f.h;
    const int64_t m = f.m, n = f.n, mn = std::min(m, n);
    const int64_t W = plan.Wb, eng_end = plan.eng_end;
    const int64_t nblk = (mn + W - 1) / W, nleaf = (mn + NB - 1) / NB;
    const size_t EX = 4 * (size_t)nblk + 8;   // (factor_leafwise: events of its own from here on)
    const hipStream_t P = h->stream;
    hipStream_t E;
    RFLU_TRY(get_ustream(h, 32, &E));
    RFLU_TRY(ensure_engine_state(h));
    EngState* est = static_cast<EngState*>(h->eng_state);
    EngState* img = static_cast<EngState*>(h->eng_host);
    EngGeo geo{};
    geo.m = (int)m; geo.n = (int)n; geo.mn = (int)mn; geo.W = (int)W; geo.nbp = (int)eng_end;
    geo.Wc = plan.eng_wc;
    geo.ncb = (int)((n + geo.Wc - 1) / geo.Wc);
    geo.pivot = f.pivot;
    geo.ahead = plan.eng_ahead;
    const size_t bytes = offsetof(EngState, cb) + (size_t)geo.ncb * sizeof(EngCB);
    const size_t skip = offsetof(EngState, remaining);   // (the arrival word in front belongs to the feeding stream: host_entry.cpp)
    eng_initial_state<T>(geo, img);
    if (h->tune.engine_replay) {   // measurement: every leaf counts as done before the engine starts (factor_leafwise skips the chain)
        if (eng_end < nblk) { set_error("RFLU_ENGINE_REPLAY needs the engine to the end"); return RFLU_ERR_ARG; }
        RFLU_TRY(launch_gate_signal(h, h->gate_ptr[0], gbase + (unsigned long long)nleaf));
        if (f.tail) { RFLU_HIP(hipStreamWaitEvent(P, f.tail, 0)); f.tail = nullptr; }
    }
    // the initial state travels on the caller's stream, in front of everything the engine is going to wait for
    RFLU_HIP(hipMemcpyAsync(reinterpret_cast<char*>(est) + skip, reinterpret_cast<char*>(img) + skip, bytes - skip, hipMemcpyHostToDevice, P));
    RFLU_TRY(record_on(h, P, EX + (size_t)nblk + 1));
    RFLU_TRY(wait_on(h, E, EX + (size_t)nblk + 1));
    EngArgs<T> a;
    a.R = f.R; a.ld = f.ld; a.g = geo; a.policy = h->tune.engine_policy;
    a.linv = static_cast<const T*>(h->linv); a.pm_cnt = h->pm_cnt; a.pm_dst = h->pm_dst; a.pm_src = h->pm_src;
    a.st = est; a.leaf_gate = h->gate_ptr[0]; a.gate_base = gbase; a.info = h->info_dev; a.gemm_flags = h->tune.gemm_flags;
    a.arrived = h->eng_host_mode ? &est->arrived : nullptr;
    a.rows_final = h->eng_host_mode ? h->eng_rows_final_dev : nullptr;
    a.write_through = h->tune.engine_write_through != 0;
    a.leaf_xcds = h->tune.engine_leaf_xcds;
    a.leaf_wgs = h->tune.engine_leaf_wgs;
    a.solve_rl = h->tune.engine_solve_rl != 0;
    // host entry: whole-block-column operations that lag the chain by this many block columns go first (engine.hip), so that
    // block rows become final -- and leave -- while the factorization runs
    a.host_lag = h->eng_host_mode ? h->tune.engine_host_lag : 0;
    // Engine to the end: its workgroups on the chain's XCD retire two leaves in front of the plan's retire leaf, which waits until they
    // are gone and takes the XCD-local leaves back from there on
    a.retire_xcc = -1; a.retire_leaf = 0;
    if (plan.eng_retire_leaf >= 0) {
        a.retire_xcc = h->panel_xcc;
        a.retire_leaf = (int)std::max<int64_t>(1, plan.eng_retire_leaf - 2);
    }
    a.trace = nullptr;
    if (env_str("RFLU_ENGINE_TRACE")) {   // measurement only: stamps of the leaf windows, printed at the next call
        if (!h->eng_trace_buf) RFLU_HIP(hipMalloc((void**)&h->eng_trace_buf, (4096 * 4 + 16) * sizeof(long long)));
        else RFLU_TRY(engine_trace_report(h, nleaf, W));
        RFLU_HIP(hipMemsetAsync(h->eng_trace_buf, 0, (4096 * 4 + 16) * sizeof(long long), P));
        a.trace = h->eng_trace_buf;
    }
    const int wgs = h->tune.engine_wgs > 0 ? h->tune.engine_wgs : 2 * (h->num_cus - 32);
    if (img->remaining > 0) {
        double eng_flops = 0, eng_bytes = 0;
        engine_prof_counts<T>(geo, n, mn, W, f.pivot, &eng_flops, &eng_bytes);
        OnStream on(h, E);
        ProfScope ps(h, RFLU_K_GEMM, eng_flops, eng_bytes);
        RFLU_TRY(launch_engine<T>(h, E, a, wgs));
    }
    RFLU_TRY(record_on(h, E, 4 * (size_t)(eng_end - 1) + 3));   // evUend: the engine leaves when every column block has received everything it owes
    h->eng_active = true;
    // While the engine is resident the only CUs with room are the 4 per XCD its mask leaves out: the any-placement leaves (at most
    // 32 workgroups, one per CU) fit there, the XCD-local ones (all participants on ONE XCD) would wait for CUs it never gives back
    h->local_rows_cap = 0;
    *E_out = E;
    *est_out = est;
    *geo_out = geo;
    return RFLU_OK;
}

// Leaf-wise schedule: the critical path is nothing but the chain of cooperative leaves.
//
// The recursion's merges (solve + Schur update of the right half) and the block-column lookahead put ~640 us of small
// dependent launches between the leaves of every 512-column block (scripts/trace_timeline.sh) -- as much as a third of the
// late, panel-bound phase.  Here every leaf g (64 columns) is applied right-looking, and only the 64 columns the NEXT leaf
// needs stay on the critical-path stream:
//   P  : leaf g -> [wait: leaf g-1 applied to LA = [c0+64, c0+128) by the side stream] {interchanges of leaf g on LA, inverse
//        of its diagonal block} (gate P >= g; both gates ride on this launch) -> solve + update of LA (K = 64) -> leaf g+1 ...
//   S  : [wait gate P >= g] leaf g applied to the rest of its own block column (gate S-in >= g) and to the next block column
//        (first leaf of a block: after evU1[b-1]) (gate S-all >= g)
//   U  : once per block column b, after its last leaf: [wait gate S-all] the deferred interchanges on the columns to the
//        left, then block column b (K = W) applied to everything right of block column b+1 -- block column b+2 first
//        (evU1[b]) -- exactly the update stream of factor_lookahead.
// Queues: the critical path stays on the caller's stream and there is ONE side stream (the next block column's part of the first
// leaf of a block waits for evU1 between two gates of its own).  An earlier version with two side streams and the critical path
// on a third, CU-confined stream ran at 115-118 ms for N=16384 instead of 88 -- two of its streams shared a hardware pipe, as round 3
// found out (validate_queues now places every stream; with four streams there is no pipe to spare).  hipEvent edges per leaf cost 40-50 us of
// bubble per record/wait on the hot stream, hipStreamWaitValue64/WriteValue64 were slower still: hence the device-side gates.
// Measured (Float64, ms): N=4096 13.6 -> 12.0, N=8192 29.7 -> 26.8, N=12288 51.6 -> 49.6; N=16384 whole matrix 88.3, from the
// first panel of <= 8192 rows on (after factor_lookahead) 84.8 vs 86.1.
// S and U share the CU mask that keeps the panel's CUs free.  Every column receives the same eliminations in the same order
// as in reckernel! (src/lu.jl:189-263); inside a block column the Schur complement is accumulated 64 pivots at a time instead
// of in the recursion's growing chunks, so factors agree with the one-stream path to rounding, pivots exactly.
// Engine mode (eng_end > 0, b_begin == 0): the side stream's and the update stream's work of block columns [0, eng_end) -- and the
// block-column updates every column right of them needs from those -- is pulled by the persistent update engine (engine.hip) from
// per-column-block counters instead of being enqueued on S and U; P is unchanged except that its lookahead launch waits for the
// engine's progress word of the lookahead strip's column block instead of a side-stream gate.  From block column eng_end on the
// streams take over again (short panels: the XCD-local leaves need CUs the resident engine does not give back).
// The block width, eng_end and the engine's geometry come from the plan (schedule_plan.hpp).
template <typename T>
static int factor_leafwise(Fact<T>& f, const SchedPlan& plan, int64_t b_begin, hipStream_t U_before)
{
    Handle* h = f.h;
    const int64_t m = f.m, n = f.n, ld = f.ld, mn = std::min(m, n);
    const int64_t W = plan.Wb, eng_end = plan.eng_end;
    T* R = f.R;
    const hipStream_t userS = h->stream;
    // (the cap on the XCD-local leaves is the engine's: gone with this schedule, however it ends)
    struct Restore { Handle* h; hipStream_t s; ~Restore() { h->stream = s; h->local_rows_cap = -1; } } restore{h, userS};
    hipStream_t P = userS;
    const int64_t nblk = (mn + W - 1) / W, nleaf = (mn + NB - 1) / NB;
    // events as in factor_lookahead: block b -> 4b+2 (evU1), 4b+3 (evUend); stream moves of this function from EX on
    const size_t EX = 4 * (size_t)nblk + 8;
    auto evU1 = [](int64_t b) { return 4 * (size_t)b + 2; };
    auto evUend = [](int64_t b) { return 4 * (size_t)b + 3; };
    // RFLU_CONFINE_ROWS: panels at least this tall run on the stream confined to the reserved CUs (default: never -- the
    // critical path stays on the caller's stream: three active queues in all, see the header comment)
    // Which of the two masked streams is which.  When the whole matrix is factored leaf-wise (no lookahead part before it) the
    // SIDE stream gets the 224-CU mask and the update stream the 192-CU one: 32 CUs the bulk GEMM never touches are then always
    // free for the side stream's per-leaf kernels, and the update has the slack to pay for it (N=4096 12.18 -> 12.03 ms, N=8192
    // 26.91 -> 26.49).  After a lookahead part the 224-CU stream is still busy with that part's last bulk update when the first
    // leaf needs the side stream (2.4 ms stall), and moving that update to the 192-CU stream costs what the swap wins (N=16384
    // 85.1 vs 85.3 ms, N=12288 49.0 vs 48.8): there the update keeps 224 CUs and the side stream takes the 192-CU stream.
    // (Float32 at N=16384 is leaf-wise from block column 0 as well, but there the update still needs its 224 CUs: 63.9 vs 62.1 ms.)
    // Round 4: swapped from the first panel of at most swap_rows (8192) rows on, wherever that is (swap_mode 2): from block column
    // bs on the side stream is the 224-CU stream, and from U(bs-1) on every update goes to the 192-CU one -- the last update in front
    // of the swap too (it is factor_lookahead's when bs is the first leaf-wise block column), so that the 224-CU stream is idle when
    // the side stream moves there.  N=16384 79.1 -> 77.75 ms (swapped one block column later, without moving that update: 78.0),
    // N=12288 45.9 -> 45.7.  What it is for (scripts/rocpd_timeline.py, scripts/gate_trace.py): a bulk GEMM that STARTS fills every
    // workgroup slot its mask allows at once, and its tiles then finish in rounds of ~130 us -- a side stream confined to the same
    // CUs gets its three small kernels per leaf placed one round boundary at a time (96 + 128 + 211 us instead of 6 + 12 + 30) and
    // the critical path stalls on gate 1 at the third / fourth leaf of every block column (200..500 us each, 3 ms in all).
    const int swap_mode = h->tune.swap_su >= 0 ? h->tune.swap_su : ((b_begin == 0 && m <= 8192) ? 1 : h->tune.swap_late ? 2 : 0);
    const int64_t bs = std::max<int64_t>(b_begin, (std::max<int64_t>(m - h->tune.swap_rows, 0) + W - 1) / W);   // first swapped block column
    auto swap_s = [&](int64_t b) { return swap_mode == 1 || (swap_mode == 2 && b >= bs); };       // side stream of block column b on the 224-CU stream
    auto swap_u = [&](int64_t b) { return swap_mode == 1 || (swap_mode == 2 && b + 1 >= bs); };   // U(b) on the 192-CU stream
    const bool fold = h->tune.gate_fold != 0 && !h->tune.gate_trace;
    const int64_t confine_rows = h->tune.confine_rows;
    auto reserve_for = [&](int64_t rows) {
        const int64_t g = panel_plan_wgs(h, rows, sizeof(T), f.pivot);
        return std::max<int>(32, int((g + 31) / 32 * 32));
    };
    // leaf (rows r0.., columns c0..c0+w) applied to columns [a, b): interchanges (optional), block-row solve, Schur update
    auto apply_leaf = [&](hipStream_t st, int64_t c0, int64_t w, int64_t a, int64_t b, bool swaps) -> int {
        if (b <= a) return RFLU_OK;
        OnStream on(h, st);
        if (swaps && f.pivot) RFLU_TRY(launch_laswp<T>(h, R, ld, a, b - a, c0 / NB, c0 / NB + 1));
        RFLU_TRY(launch_trsm_inv64<T>(h, w, b - a, f.linv_at(c0), R + c0 * ld + a, ld));
        if (m > c0 + w) RFLU_TRY(launch_gemm<T>(h, m - c0 - w, b - a, w, R + (c0 + w) * ld + c0, ld, R + c0 * ld + a, ld, R + (c0 + w) * ld + a, ld));
        return RFLU_OK;
    };
    auto update = [&](hipStream_t st, int64_t j0, int64_t jb, int64_t c0, int64_t c1) -> int {
        if (c1 <= c0) return RFLU_OK;
        OnStream on(h, st);
        const int64_t je = j0 + jb;
        if (f.pivot) RFLU_TRY(launch_laswp<T>(h, R, ld, c0, c1 - c0, j0 / NB, (je + NB - 1) / NB));
        RFLU_TRY(trsm_rec<T>(h, jb, c1 - c0, R + j0 * ld + j0, ld, R + j0 * ld + c0, ld, f.linv_at(j0)));
        if (m > je) RFLU_TRY(launch_gemm<T>(h, m - je, c1 - c0, jb, R + je * ld + j0, ld, R + j0 * ld + c0, ld, R + je * ld + c0, ld));
        return RFLU_OK;
    };
    hipStream_t Uprev = U_before, Sprev = nullptr;   // U_before: the update stream of block b_begin-1 (factor_lookahead)
    const unsigned long long gbase = h->gate_epoch;
    h->gate_epoch += (unsigned long long)nleaf + 2;
    auto val = [&](int64_t g) { return gbase + (unsigned long long)g + 1; };
    const int64_t gfirst = b_begin * W / NB;   // the leaves before it were factored (and applied everywhere) by factor_lookahead
    if (h->tune.gate_trace && !h->gate_stamps) {
        RFLU_HIP(hipMalloc((void**)&h->gate_stamps, 3 * 4096 * sizeof(long long)));
        RFLU_HIP(hipMemset(h->gate_stamps, 0, 3 * 4096 * sizeof(long long)));
    }
    auto stamp = [&](int which, int64_t g) -> long long* { return (h->gate_stamps && g < 4096) ? h->gate_stamps + which * 4096 + g : nullptr; };
    // ---- engine mode: the engine takes the side stream's and the update stream's work of block columns [0, eng_end) ----
    const int64_t LPB = W / NB;
    EngGeo geo{};
    EngState* est = nullptr;
    const int64_t eng_retire_leaf = plan.eng_retire_leaf;   // engine mode: the leaf in front of which the engine's workgroups on the chain's XCD are gone
    if (eng_end > 0) {
        if (b_begin != 0) { set_error("factor_leafwise: the engine starts at block column 0"); return RFLU_ERR_ARG; }
        hipStream_t E = nullptr;
        RFLU_TRY(start_engine<T>(f, plan, gbase, &E, &est, &geo));
        Uprev = E;
    }
    // the hand-over from the engine to the streams: hold the handle's stream until every column block of block column x has completed its sequence
    auto wait_engine_done_with = [&](int64_t x) -> int {
        for (int c = eng_first_cb(geo, (int)x); c < eng_first_cb(geo, (int)x) + eng_cbs_of_block(geo, (int)x); ++c)
            if (eng_nops(geo, c) > 0) RFLU_TRY(launch_eng_wait(h, &est->cb[c].prog, 2ull * (unsigned long long)eng_nops(geo, c)));
        return RFLU_OK;
    };
    for (int64_t b = b_begin; b < nblk; ++b) {
        const bool in_eng = b < eng_end;
        if (in_eng && h->tune.engine_replay) continue;   // (measurement: the engine alone)
        if (eng_end > 0 && b == eng_end) h->local_rows_cap = -1;   // the streams take over: the leaves are short enough for the XCD-local exchange again
        const int64_t j0 = b * W, jb = std::min(W, mn - j0), je = j0 + jb;
        const int64_t bend = std::min(j0 + W, n), wend = std::min(j0 + 2 * W, n);
        const int res = reserve_for(m - j0);
        // The side stream is the update stream of the 64-CU reservation: it keeps away from the panel's 32 CUs like U does,
        // and a taller matrix has already used it for its first block columns -- one queue less to place (validate_queues).
        if (res != 32) { set_error("factor_leafwise: panel of %lld rows needs more than 32 CUs", (long long)(m - j0)); return RFLU_ERR_ARG; }
        hipStream_t S = nullptr;
        if (!in_eng) RFLU_TRY(get_ustream(h, swap_s(b) ? 32 : 64, &S));
        if (!in_eng)
        {   // the critical path runs on the reserved CUs while the update stream is the bottleneck (see get_pstream)
            hipStream_t to = userS;
            if (m - j0 >= confine_rows && res == 32) RFLU_TRY(get_pstream(h, res, &to));
            if (to != P) {
                RFLU_TRY(record_on(h, P, EX + (size_t)b));
                RFLU_TRY(wait_on(h, to, EX + (size_t)b));
                P = to;
                h->stream = to;   // lasting: the critical path has moved (restored by `restore`)
            }
        }
        const int64_t g0 = j0 / NB, nl = (jb + NB - 1) / NB;
        if (in_eng && h->eng_host_mode)   // host entry: the block column (and the lookahead strip of its last leaf) has to be in place
            RFLU_TRY(launch_eng_wait(h, &est->arrived, (unsigned long long)std::min<int64_t>(n, je + NB)));
        for (int64_t i = 0; i < nl; ++i) {
            const int64_t g = g0 + i, c0 = j0 + i * NB, w = std::min<int64_t>(NB, je - c0);
            if (in_eng && g == eng_retire_leaf) {   // the chain's XCD is its own again: XCD-local leaves from here on
                RFLU_TRY(launch_eng_wait_retired(h, h->panel_xcc));
                h->local_rows_cap = -1;   // (every panel from here on is at most engine_retire rows tall)
            }
            RFLU_TRY(launch_panel<T>(h, R, ld, m, c0, c0, w, f.ipiv, f.pivot));
            const int64_t la0 = c0 + w, la1 = std::min(la0 + NB, n);
            const unsigned long long* wflag = nullptr;   // leaf g-1 reached LA through the side stream: in its own block's part, or the next block's
            unsigned long long wval = g > 0 ? val(g - 1) : 0;
            if (la1 > la0 && g > gfirst) {
                if (eng_end > 0 && (g - 1) / LPB < eng_end) {   // ... through the engine: LEAF(g - 1) is complete on the lookahead strip's column block
                    const int cb_la = (int)(la0 / geo.Wc);
                    wflag = &est->cb[cb_la].prog;
                    wval = 2ull * (unsigned long long)eng_leaf_op_index(geo, cb_la, (int)(g - 1)) + 1;   // (its first tile column: engine.hpp, prog)
                } else {
                    wflag = h->gate_ptr[la0 < std::min(((c0 - NB) / W + 1) * W, n) ? 1 : 2];
                }
            }
            if (eng_end > 0 && f.tail && la1 > W) {   // the first launch of the critical path that touches the columns whose layout change
                RFLU_HIP(hipStreamWaitEvent(P, f.tail, 0));   // ran on the engine's stream next to the first leaves
                f.tail = nullptr;
            }
            // one launch for {interchanges on LA, diagonal inverse, 64-row solve of LA}: full leaves with a full, 16-byte aligned LA
            const bool fuse = f.pivot && fold && h->tune.leaf_fuse && w == NB && la1 - la0 == NB && m - c0 > NB &&
                              reinterpret_cast<uintptr_t>(R) % 16 == 0 && ld % (16 / (int64_t)sizeof(T)) == 0;
            LaswpGate gt;   // both gates ride on the leaf's lookahead launch (fuse / fold)
            gt.wait_flag = wflag;
            gt.wait_val = wflag ? wval : 0;
            gt.signal_flag = h->gate_ptr[0];
            gt.signal_val = val(g);
            gt.signal_cnt = reinterpret_cast<unsigned*>(h->gates + 4);
            gt.info = h->info_dev;
            if (fuse) {
                RFLU_TRY(launch_leaf_la<T>(h, R, ld, la0, c0 / NB, c0, R + c0 * ld + c0, f.linv_at(c0), gt));
                RFLU_TRY(launch_gemm<T>(h, m - c0 - w, la1 - la0, w, R + (c0 + w) * ld + c0, ld, R + c0 * ld + la0, ld, R + (c0 + w) * ld + la0, ld));
            } else if (f.pivot && fold) {   // two launches less per leaf on this stream
                RFLU_TRY(launch_laswp2<T>(h, R, ld, la0, la1 - la0, 0, 0, c0 / NB, c0 / NB + 1, w, R + c0 * ld + c0, f.linv_at(c0), gt));
            } else {
                if (wflag) RFLU_TRY(launch_gate_wait(h, wflag, wval));
                if (f.pivot) RFLU_TRY(launch_laswp2<T>(h, R, ld, la0, la1 - la0, 0, 0, c0 / NB, c0 / NB + 1, w, R + c0 * ld + c0, f.linv_at(c0)));
                RFLU_TRY(launch_gate_signal(h, h->gate_ptr[0], val(g), stamp(0, g)));
            }
            if (!fuse) RFLU_TRY(apply_leaf(P, c0, w, la0, la1, false));
            if (in_eng) continue;   // (the engine applies the leaf to the rest of this block column and to the next one)
            // ---- side stream: leaf g on the rest of this block column and on the next one ----
            OnStream on(h, S);   // (to the end of this leaf's turn)
            RFLU_TRY(launch_gate_wait(h, h->gate_ptr[0], val(g)));
            if (i == 0 && S != Sprev && g > gfirst && !(eng_end > 0 && (g - 1) / LPB < eng_end))
                RFLU_TRY(launch_gate_wait(h, h->gate_ptr[2], val(g - 1)));
            if (i == 0 && b > 0) {
                // the next block column holds U(b-1)'s update only after evU1[b-1]; the critical path needs this block
                // column's part first, so the leaf is applied in two pieces with a gate of its own in between.
                // (Round 4 tried leaving the next block column's part of the first 1..6 leaves to a later leaf, so that the in-order
                // side stream does not sit on the event with the own parts of the next leaves queued behind it: no gain, N=16384
                // 78.2-78.9 vs 78.7-79.1 ms -- the event is not what the side stream waits for, see swap_mode above.)
                // Hand-over from the update engine (b == eng_end): the rest of THIS block column is the side stream's from here on, and the
                // engine may still be applying the previous block column's last leaves to it (the chain's wait covered the first tile column
                // of the lookahead strip's column block only); and the next block column is up to date when all its operations are complete
                const bool handover = eng_end > 0 && b == eng_end;
                if (handover) RFLU_TRY(wait_engine_done_with(b));
                RFLU_TRY(apply_leaf(S, c0, w, la1, bend, true));
                RFLU_TRY(launch_gate_signal(h, h->gate_ptr[1], val(g), stamp(1, g)));
                if (handover) RFLU_TRY(wait_engine_done_with(b + 1));
                else {
                    hipEvent_t e;
                    RFLU_TRY(get_event(h, evU1(b - 1), &e));
                    if (hipStreamWaitEvent(S, e, 0) != hipSuccess) { set_error("hipStreamWaitEvent failed"); return RFLU_ERR_HIP; }
                }
                RFLU_TRY(apply_leaf(S, c0, w, std::max(la1, bend), wend, true));
                RFLU_TRY(launch_gate_signal(h, h->gate_ptr[2], val(g), stamp(2, g)));
            } else {
                RFLU_TRY(apply_leaf(S, c0, w, la1, wend, true));
                RFLU_TRY(launch_gate_signal(h, h->gate_ptr[1], val(g), stamp(1, g)));
                RFLU_TRY(launch_gate_signal(h, h->gate_ptr[2], val(g), stamp(2, g)));
            }
        }
        if (in_eng) continue;
        Sprev = S;
        // ---- U(b): everything right of block column b+1, and the interchanges nobody needed until now ----
        hipStream_t U;
        RFLU_TRY(get_ustream(h, swap_u(b) ? 64 : reserve_for(m - je), &U));
        const int64_t glast = g0 + nl - 1;
        {
            OnStream on(h, U);
            RFLU_TRY(launch_gate_wait(h, h->gate_ptr[2], val(glast)));
        }
        if (Uprev && Uprev != U) RFLU_TRY(wait_on(h, U, evUend(b - 1)));
        if (f.pivot) {
            OnStream on(h, U);
            for (int64_t i = 0; i + 1 < nl; ++i)   // leaf i's columns: the later leaves' interchanges
                RFLU_TRY(launch_laswp<T>(h, R, ld, j0 + i * NB, NB, g0 + i + 1, g0 + nl));
            if (j0 > 0) RFLU_TRY(launch_laswp<T>(h, R, ld, 0, j0, g0, g0 + nl));
        }
        const int64_t p1e = std::min(wend + W, n);
        RFLU_TRY(update(U, j0, jb, wend, p1e));
        RFLU_TRY(record_on(h, U, evU1(b)));
        RFLU_TRY(update(U, j0, jb, p1e, n));
        RFLU_TRY(record_on(h, U, evUend(b)));
        Uprev = U;
        if (h->progress) RFLU_TRY(h->progress(je));
    }
    if (P != userS) {
        RFLU_TRY(record_on(h, P, EX + (size_t)nblk));
        RFLU_TRY(wait_on(h, userS, EX + (size_t)nblk));
        P = userS;
        h->stream = userS;   // lasting: the critical path is back on the caller's stream
    }
    RFLU_TRY(wait_on(h, userS, evUend(nblk - 1)));
    h->eng_active = false;
    return RFLU_OK;
}

// Factor the row-major m x n matrix R in place (see rflu.h for `blocksize`).
template <typename T>
int getrf_rm(Handle* h, int64_t m, int64_t n, T* R, int64_t ld, int64_t* ipiv, int pivot, int64_t blocksize,
                    int64_t* info)
{
    if (m < 0 || n < 0 || ld < std::max<int64_t>(n, 1) || (m > 0 && n > 0 && R == nullptr)) {
        set_error("getrf: bad arguments m=%lld n=%lld ld=%lld", (long long)m, (long long)n, (long long)ld);
        return RFLU_ERR_ARG;
    }
    if (pivot && ipiv == nullptr && std::min(m, n) > 0) {
        set_error("getrf: pivot != 0 needs an ipiv buffer");
        return RFLU_ERR_ARG;
    }
    *info = 0;
    const int64_t mn = std::min(m, n);
    h->last_path = RFLU_PATH_NONE;
    if (mn == 0) return RFLU_OK;
    RFLU_TRY(ensure_bookkeeping(h, m));
    h->coop_leaf_seq = 0;
    RFLU_HIP(hipMemsetAsync(h->info_dev, 0, 2 * sizeof(int64_t), h->stream));
    // the wrapping "last workgroup" counters of the folded gates: a factorization that timed out or was aborted may have left
    // them mid-count, and a stale count would publish the next factorization's gate early or never
    RFLU_HIP(hipMemsetAsync(h->gates + 4, 0, 2 * sizeof(unsigned long long), h->stream));
    if (!pivot && ipiv) RFLU_TRY(launch_iota_ipiv(h, ipiv, 0, mn));  // src/lu.jl:111-113

    Fact<T> f{h, R, ld, m, n, ipiv, pivot};
    // which schedule (schedule_plan.hpp).  The two-stream schedules ask for their CU-masked streams first: a mask that cannot be had
    // changes the plan (the leaf-wise / engine schedules hand work between streams through device-side gates: only with real masks)
    SchedIn in = sched_in(h, m, n, sizeof(T), pivot, blocksize, h->eng_host_mode ? ENTRY_HOST_ENGINE : ENTRY_RM,
                          reinterpret_cast<uintptr_t>(R) % 16 == 0, ld);
    SchedPlan p = plan_schedule(in);
    // column-major entry with the tail of the layout change still in flight (getrf_cm_dev): only factor_lookahead and the engine know
    // where the first access to those columns is; every other path waits for it here
    hipEvent_t tail = h->tail_event;
    h->tail_event = nullptr;
    if (p.two_stream) {
        hipStream_t probe;
        RFLU_TRY(get_ustream(h, 32, &probe));
        RFLU_TRY(get_ustream(h, 64, &probe));
        if (!h->mask_failed) RFLU_TRY(validate_queues(h));
        in.mask_failed = h->mask_failed;
        p = plan_schedule(in);
    }
    if (h->eng_host_mode && p.path != RFLU_PATH_HIP_ENGINE) {   // (getrf_host asked the same plan: tests/schedule_plan_check.cpp)
        set_error("getrf: host entry through the engine asked for a schedule the engine cannot serve");
        return RFLU_ERR_ARG;
    }
    if (tail && p.b_switch == 0 && p.eng_end == 0) {
        RFLU_HIP(hipStreamWaitEvent(h->stream, tail, 0));
        tail = nullptr;
    }
    f.tail = tail;
    h->last_path = p.path;
    const auto t_enq0 = std::chrono::steady_clock::now();
    if (p.path == RFLU_PATH_HIP_RECURSIVE) {
        RFLU_TRY(f.rec(0, mn));
    } else if (p.path == RFLU_PATH_HIP_BLOCKED) {
        const int64_t bs = p.Wb;
        for (int64_t j = 0; j < mn; j += bs) {
            const int64_t jb = std::min(bs, mn - j);
            RFLU_TRY(f.rec(j, j + jb));
            const int64_t je = j + jb;
            if (je < mn) {  // trailing update of the remaining square part
                RFLU_TRY(trsm_rec<T>(h, jb, mn - je, R + j * ld + j, ld, R + j * ld + je, ld, f.linv_at(j)));
                RFLU_TRY(launch_gemm<T>(h, m - je, mn - je, jb, R + je * ld + j, ld, R + j * ld + je, ld,
                                        R + je * ld + je, ld));
            }
        }
    } else {
        hipStream_t U_last = nullptr;
        if (p.path == RFLU_PATH_HIP_ENGINE) {
            RFLU_TRY(factor_leafwise<T>(f, p, 0, nullptr));
        } else {
            if (p.b_switch > 0) RFLU_TRY(factor_lookahead<T>(f, p.Wb, p.b_switch, &U_last, p.W_wide, p.wide_end));
            if (p.b_switch < p.nblk) RFLU_TRY(factor_leafwise<T>(f, p, p.b_switch, U_last));
        }
        if (h->tune.time_enqueue)
            fprintf(stderr, "[rflu] host enqueue time %.2f ms\n",
                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_enq0).count());
    }
    // fat matrix: AR <- L^-1 AR (src/lu.jl:148-154; interchanges already applied there) -- the two-stream schedules' block-column
    // updates have already reached the columns right of the square part
    if (m < n && !p.two_stream)
        RFLU_TRY(trsm_rec<T>(h, m, n - m, R, ld, R + m, ld, f.linv_at(0)));

    if (h->before_sync) RFLU_TRY(h->before_sync());
    RFLU_HIP(hipMemcpyAsync(h->info_pinned, h->info_dev, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    RFLU_HIP(hipStreamSynchronize(h->stream));
    RFLU_TRY(panel_flags_status(h));
    *info = h->info_pinned[0];
    return RFLU_OK;
}

// column-major device entry: R-layout workspace, transpose in, factor, transpose out
template <typename T>
int getrf_cm_dev(Handle* h, int64_t m, int64_t n, T* A, int64_t lda, int64_t* ipiv, int pivot,
                        int64_t blocksize, int64_t* info)
{
    if (m < 0 || n < 0 || lda < std::max<int64_t>(m, 1) || info == nullptr) {
        set_error("getrf: bad arguments m=%lld n=%lld lda=%lld", (long long)m, (long long)n, (long long)lda);
        return RFLU_ERR_ARG;
    }
    *info = 0;
    if (m == 0 || n == 0) return RFLU_OK;
    const int64_t ldr = workspace_ld(h, n);
    RFLU_TRY(ensure_buffer(&h->work, &h->work_bytes, (size_t)m * (size_t)ldr * sizeof(T)));
    T* R = static_cast<T*>(h->work);
    // Layout change in two pieces: the first block column on the caller's stream, the rest on the CU-masked update stream while
    // the first panel (2.3 ms on 32 CUs at N=16384, nothing else to do) already runs.
    const SchedPlan p = plan_schedule(sched_in(h, m, n, sizeof(T), pivot, blocksize, ENTRY_CM, reinterpret_cast<uintptr_t>(R) % 16 == 0, ldr));
    const int64_t W0 = p.tail_w0;
    if (p.tail_overlap) {
        if (!h->tail_event_obj) {
            RFLU_HIP(hipEventCreateWithFlags(&h->tail_event_obj, hipEventDisableTiming));
            RFLU_HIP(hipEventCreateWithFlags(&h->tail_fork_obj, hipEventDisableTiming));
        }
        hipStream_t U0, user = h->stream;
        RFLU_TRY(get_ustream(h, 32, &U0));
        {   // settle which streams the schedules will use BEFORE work goes onto one of them (validate_queues may replace a stream)
            hipStream_t s64;
            RFLU_TRY(get_ustream(h, 64, &s64));
            if (!h->mask_failed) RFLU_TRY(validate_queues(h));
            RFLU_TRY(get_ustream(h, 32, &U0));
        }
        RFLU_HIP(hipEventRecord(h->tail_fork_obj, user));            // whatever produced A on the caller's stream
        RFLU_HIP(hipStreamWaitEvent(U0, h->tail_fork_obj, 0));
        RFLU_TRY(launch_transpose<T>(h, m, W0, A, lda, R, ldr));
        {
            OnStream on(h, U0);
            RFLU_TRY(launch_transpose<T>(h, m, n - W0, A + W0 * lda, lda, R + W0, ldr));
        }
        RFLU_HIP(hipEventRecord(h->tail_event_obj, U0));
        h->tail_event = h->tail_event_obj;
    } else {
        RFLU_TRY(launch_transpose<T>(h, m, n, A, lda, R, ldr));
    }
    const int rc_f = getrf_rm<T>(h, m, n, R, ldr, ipiv, pivot, blocksize, info);
    if (h->tail_event_obj && rc_f != RFLU_OK) {
        // error before the tail event was consumed: the layout change may still be reading A / writing the workspace on the
        // update stream -- do not hand either back to the caller while it runs
        hipStream_t U0 = nullptr;
        if (get_ustream(h, 32, &U0) == RFLU_OK && U0) (void)hipStreamSynchronize(U0);
    }
    h->tail_event = nullptr;
    RFLU_TRY(rc_f);
    if (!h->out_done) RFLU_TRY(launch_transpose<T>(h, n, m, R, ldr, A, lda));   // (the host entry has taken the factors out piece by piece)
    RFLU_HIP(hipStreamSynchronize(h->stream));
    return RFLU_OK;
}

#define RFLU_INSTANTIATE_SCHEDULE(T)                                                                                                  \
    template int getrf_rm<T>(Handle*, int64_t, int64_t, T*, int64_t, int64_t*, int, int64_t, int64_t*);                               \
    template int getrf_cm_dev<T>(Handle*, int64_t, int64_t, T*, int64_t, int64_t*, int, int64_t, int64_t*);                           \
    template int panel_rec<T>(Handle*, int64_t, int64_t, int64_t, int64_t, T*, int64_t, int64_t*, int);                               \
    template int panel_rm<T>(Handle*, int64_t, int64_t, int64_t, int64_t, T*, int64_t, int64_t*, int, int64_t*);                      \
    template int laswp_rm<T>(Handle*, T*, int64_t, int64_t, int64_t, int64_t, const int64_t*, int64_t, int64_t);
RFLU_INSTANTIATE_SCHEDULE(double)
RFLU_INSTANTIATE_SCHEDULE(float)

}  // namespace rflu
