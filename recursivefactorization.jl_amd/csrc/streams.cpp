// streams.cpp -- the streams and events the schedules run on: the handle's numbered events (get_event), the CU-masked update streams and
// their complements (get_ustream / get_pstream), and the placement of those streams on hardware pipes of their own (validate_queues).
#include <stdio.h>

#include <algorithm>

#include "driver.hpp"

namespace rflu {

int get_event(Handle* h, size_t idx, hipEvent_t* ev)
{
    while (h->events.size() <= idx) {
        hipEvent_t e;
        RFLU_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        h->events.push_back(e);
    }
    *ev = h->events[idx];
    return RFLU_OK;
}

// ustreams[r] (complement = false) keeps away from the first 32 * r CUs of the mask's enumeration, pstreams[r] (complement = true) is
// confined to them.  Streams are created once per reservation and kept for the life of the handle.
static int get_masked_stream(Handle* h, int reserve, bool complement, hipStream_t* out)
{
    const int r = reserve / 32;
    if (reserve % 32 != 0 || r < 1 || r > 7) { set_error("CU reservation %d not in 32..224 step 32", reserve); return RFLU_ERR_ARG; }
    hipStream_t* slot = complement ? &h->pstreams[r] : &h->ustreams[r];
    if (!*slot) {
        // CU mask bits are enumerated round-robin over the 8 XCDs (scripts/probes/cumask.hip): bits 0..31 are 4 CUs of
        // every XCD, and so on.  A mask that empties an XCD is ignored by the runtime, so whole 32-bit words are cleared.
        // The mask covers the CUs the device actually reports (num_cus / 32 words); callers only ask for a reservation
        // on a full 256-CU device (factor_lookahead).
        uint32_t mask[8];
        const int words = std::min(8, (h->num_cus + 31) / 32);
        for (int i = 0; i < 8; ++i) mask[i] = (i < words && (i < r) == complement) ? 0xffffffffu : 0u;
        if (words <= r || hipExtStreamCreateWithCUMask(slot, (uint32_t)words, mask) != hipSuccess) {
            (void)hipGetLastError();
            if (!complement) h->mask_failed = true;   // (the schedules ask the update streams whether masks can be had)
            RFLU_HIP(hipStreamCreateWithFlags(slot, hipStreamNonBlocking));
        }
    }
    *out = *slot;
    return RFLU_OK;
}

// An update stream leaves `reserve` CUs (a multiple of 32, 32..224) to the critical-path stream so that the cooperative
// panel kernel (one 512-thread workgroup per CU) finds all its workgroups a home at once.
int get_ustream(Handle* h, int reserve, hipStream_t* out) { return get_masked_stream(h, reserve, false, out); }

// The complement of get_ustream's mask: a stream confined to the `reserve` CUs the update stream never touches.
// While the factorization is update-bound the critical path has time to spare, and the workgroups of ITS GEMMs that land on
// shared CUs delay the update (scripts/microbench_gemm_vs_rec.py: -2 % on the masked 15872 x 14848 x 512 GEMM) -- so in that
// phase the critical path is kept on its own CUs (N=16384: 88.1 -> 86.8 ms).
int get_pstream(Handle* h, int reserve, hipStream_t* out) { return get_masked_stream(h, reserve, true, out); }

// ---- the schedules' streams on different hardware pipes -------------------------------------------------------------------------
// Every stream with a CU mask is an HSA queue of its own, and queues are spread round-robin over the 4 pipes of the compute
// micro-engine in the order the PROCESS created them.  Two busy queues on one pipe cost every kernel of both ~25 us
// (queue_probe_rate: two backlogged streams drain their one-thread kernels at 1.7 us per kernel on different pipes, 3.1 us when they are
// one and the same stream, 28 us when they share a pipe; N=4096 12 -> 20 ms, N=16384 80 -> 108 ms when the update or the side stream
// lands on the critical path's pipe).  With more than four busy streams somebody has to share; the library uses at most four.  Which
// queue index a new stream gets depends on how many queues the host program created before -- so it is measured, not assumed: each of
// the library's masked streams is probed against the caller's stream and the ones already accepted, and replaced by a new one with
// the same mask (the next queue index) until it shares a pipe with none of them; the rejected streams stay parked, idle.
// Re-checked when the caller's stream changes (rflu_set_stream) or a new masked stream appears.  RFLU_QUEUE_CHECK=0 skips it.
int validate_queues(Handle* h)
{
    if (!h->tune.queue_check || h->queue_giveup) return RFLU_OK;
    int created = 0;
    for (int r = 1; r < 8; ++r) created += (h->ustreams[r] != nullptr) + (h->pstreams[r] != nullptr);
    const bool new_masked = h->queues_ok_count != created;   // a masked stream has appeared since the last check: everything is checked again
    if (!new_masked)
        for (hipStream_t ok : h->queues_ok_streams)
            if (ok == h->stream) return RFLU_OK;   // (a host program that alternates between a few streams is checked once per stream)
    if (!h->qprobe_slots) RFLU_HIP(hipMalloc((void**)&h->qprobe_slots, 8 * sizeof(long long)));
    const hipStream_t P = h->stream;
    constexpr int NPROBE = 128;   // the second half is timed (queue_probe_rate)
    constexpr size_t MAX_PARKED = 16;   // replaced streams stay parked (idle) for the life of the handle: bounded
    double base = 0;
    RFLU_TRY(queue_probe_rate(P, P, NPROBE, h->qprobe_slots, &base));
    RFLU_TRY(queue_probe_rate(P, P, NPROBE, h->qprobe_slots, &base));   // the first pass warms the launch path
    const double limit = std::min(std::max(2.0 * base, base + 5.0), 12.0);   // (a slow first reading of the base must not raise the bar to what a shared pipe reads)   // base = the caller's stream against itself (3.1 us); a shared pipe reads 28
    // a masked stream has to get along with the current caller stream and with the masked streams accepted before it.  (Not with the
    // caller streams it was accepted next to earlier: those are idle while this one is in use, and with two caller streams + three
    // masked streams there are more queues than pipes -- asking for that left the host entry's way-back stream on a shared pipe:
    // 120 -> 145 ms host to host.  A host that alternates between caller streams gets a new check when a stream had to be
    // replaced for the other one; the cap on parked streams and the give-up rule below bound what that can cost.)
    std::vector<hipStream_t> accepted{P};
    const bool verbose = h->tune.queue_trace != 0;
    bool unresolved = false;
    auto worst_next_to = [&](hipStream_t s, double* worst) -> int {
        *worst = 0;
        for (hipStream_t a : accepted) {
            double us = 0;
            RFLU_TRY(queue_probe_rate(a, s, NPROBE, h->qprobe_slots, &us));
            *worst = std::max(*worst, us);
        }
        return RFLU_OK;
    };
    auto settle = [&](hipStream_t* slot, int r, bool complement) -> int {
        for (int attempt = 0; attempt < 8; ++attempt) {
            double worst = 0;
            RFLU_TRY(worst_next_to(*slot, &worst));
            // wall-clock readings: a marginally slow one has to repeat before it counts; a clear one (a shared pipe reads ~28 us, nine
            // times the base) is taken at once -- the repeat of a clear reading was seen to come back low and leave the collision in place
            if (worst > limit && worst < 2.0 * limit) RFLU_TRY(worst_next_to(*slot, &worst));
            if (verbose)
                fprintf(stderr, "[rflu] queue check %s[%d] attempt %d: %.1f us per kernel next to the accepted streams (alone %.1f)\n",
                        complement ? "pstream" : "ustream", r, attempt, worst, base);
            if (worst <= limit) {
                // a good reading is confirmed once: a colliding pair was seen to read low now and then (the whole process then runs with two
                // queues on one pipe: N=8192 35 instead of 24 ms, N=16384 100 instead of 76 -- one process in a few dozen)
                double again = 0;
                RFLU_TRY(worst_next_to(*slot, &again));
                if (verbose && again > limit)
                    fprintf(stderr, "[rflu] queue check %s[%d] attempt %d: second reading %.1f us\n", complement ? "pstream" : "ustream", r, attempt, again);
                worst = std::max(worst, again);
            }
            if (worst <= limit) break;
            if (attempt == 7 || h->parked_streams.size() >= MAX_PARKED) {   // keep this one: never fail a factorization over placement
                unresolved = true;
                break;
            }
            h->parked_streams.push_back(*slot);
            h->queues_ok_streams.clear();   // what was accepted next to other caller streams is no longer what is in use
            *slot = nullptr;
            hipStream_t fresh;
            if (complement) RFLU_TRY(get_pstream(h, 32 * r, &fresh));
            else RFLU_TRY(get_ustream(h, 32 * r, &fresh));
            if (h->mask_failed) return RFLU_OK;
        }
        accepted.push_back(*slot);
        return RFLU_OK;
    };
    for (int r = 1; r < 8; ++r)
        if (h->ustreams[r]) RFLU_TRY(settle(&h->ustreams[r], r, false));
    for (int r = 1; r < 8; ++r)
        if (h->pstreams[r]) RFLU_TRY(settle(&h->pstreams[r], r, true));
    // more busy caller streams than there are pipes to spare (or a GPU shared with another process, whose load reads like a
    // conflict): after three checks that could not be settled the placement is taken as it is
    if (unresolved && ++h->queue_unresolved >= 3) {
        h->queue_giveup = true;
        if (verbose) fprintf(stderr, "[rflu] queue check: placement not settled after %d checks, %zu streams parked: no further checks on this handle\n",
                             h->queue_unresolved, h->parked_streams.size());
    }
    bool known = false;
    for (hipStream_t ok : h->queues_ok_streams) known = known || ok == P;
    if (!known) {
        if (h->queues_ok_streams.size() >= 8) h->queues_ok_streams.erase(h->queues_ok_streams.begin());
        h->queues_ok_streams.push_back(P);
    }
    h->queues_ok_count = 0;
    for (int r = 1; r < 8; ++r) h->queues_ok_count += (h->ustreams[r] != nullptr) + (h->pstreams[r] != nullptr);
    return RFLU_OK;
}

}  // namespace rflu
