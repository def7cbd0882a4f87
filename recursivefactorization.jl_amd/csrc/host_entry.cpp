// host_entry.cpp -- the host-pointer entries of librflu.so (rflu_getrf_*, rflu_getrs_*, rflu_getrs_trans_*, rflu_getri_*,
// rflu_logabsdet_* without _dev): caller-owned column-major host arrays (the reference's boundary, src/lu.jl:116-121), staged through
// device buffers the handle owns and handed to the device entries of driver.cpp.  For the factorization of large matrices the
// transfers overlap the work: the way back on both schedules (WayBack), the way in through the update engine (getrf_host_engine).
#include <stdio.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <thread>

#include "complex.hpp"
#include "driver.hpp"
#include "engine.hpp"
#include "host_wayback.hpp"

namespace rflu {

// ---- staging: one helper per pattern --------------------------------------------------------------------------------------------------
static int ensure_ipiv_dev(Handle* h, int64_t n)
{
    if ((size_t)n <= h->ipiv_cap) return RFLU_OK;
    if (h->ipiv_dev) RFLU_HIP(hipFree(h->ipiv_dev));
    h->ipiv_dev = nullptr;
    h->ipiv_cap = 0;
    RFLU_HIP(hipMalloc((void**)&h->ipiv_dev, (size_t)n * sizeof(int64_t)));
    h->ipiv_cap = (size_t)n;
    return RFLU_OK;
}

// the caller's pivots onto the device (on the handle's stream); *dev is what the device entry gets: nullptr for NULL (NotIPIV)
static int stage_ipiv(Handle* h, const int64_t* ipiv, int64_t n, const int64_t** dev)
{
    RFLU_TRY(ensure_ipiv_dev(h, n));
    if (ipiv) RFLU_HIP(hipMemcpyAsync(h->ipiv_dev, ipiv, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
    *dev = ipiv ? h->ipiv_dev : nullptr;
    return RFLU_OK;
}

// host column-major rows x cols (leading dimension ld) -> packed device copy (leading dimension rows), and back
template <typename T>
static int copy_in(T* dev, const T* host, int64_t ld, int64_t rows, int64_t cols, hipStream_t st)
{
    RFLU_HIP(hipMemcpy2DAsync(dev, rows * sizeof(T), host, ld * sizeof(T), rows * sizeof(T), (size_t)cols, hipMemcpyHostToDevice, st));
    return RFLU_OK;
}
template <typename T>
static int copy_out(T* host, int64_t ld, const T* dev, int64_t rows, int64_t cols, hipStream_t st)
{
    RFLU_HIP(hipMemcpy2DAsync(host, ld * sizeof(T), dev, rows * sizeof(T), rows * sizeof(T), (size_t)cols, hipMemcpyDeviceToHost, st));
    return RFLU_OK;
}

// the element as these helpers stage it: a complex array arrives as R* pointing at interleaved (re, im) pairs; HostElem<E> is the staged
// element of the element trait E (rflu_internal.hpp)
template <typename R>
struct HostCx { R re, im; };
template <typename E> struct HostElem { typedef typename E::real type; };
template <typename R> struct HostElem<CplxElem<R>> { typedef HostCx<R> type; };

// the two pinned bounce buffers of the way back, `bytes` each.  *available = false, no buffers kept: no pinned memory to be had (no error)
static int ensure_bounce(Handle* h, size_t bytes, bool* available)
{
    *available = true;
    if (h->bounce_bytes >= bytes) return RFLU_OK;
    for (int i = 0; i < 2; ++i) {
        if (h->bounce[i]) RFLU_HIP(hipHostFree(h->bounce[i]));
        h->bounce[i] = nullptr;
    }
    h->bounce_bytes = 0;
    for (int i = 0; i < 2 && *available; ++i) *available = hipHostMalloc(&h->bounce[i], bytes) == hipSuccess;
    if (*available) h->bounce_bytes = bytes;
    else (void)hipGetLastError();
    for (int i = 0; i < 2 && !*available; ++i) {
        if (h->bounce[i]) (void)hipHostFree(h->bounce[i]);
        h->bounce[i] = nullptr;
    }
    return RFLU_OK;
}

// ---- ldiv!(F, B) and ldiv!(F', B) ---------------------------------------------------------------------------------------------------
template <typename T>
int getrs_host(Handle* h, int64_t n, int64_t nrhs, const T* F, int64_t lda, const int64_t* ipiv, T* B, int64_t ldb, bool trans)
{
    if (n < 0 || nrhs < 0 || lda < std::max<int64_t>(n, 1) || ldb < std::max<int64_t>(n, 1) ||
        (n > 0 && nrhs > 0 && (F == nullptr || B == nullptr))) {
        set_error(trans ? "getrs_trans: bad arguments" : "getrs: bad arguments");
        return RFLU_ERR_ARG;
    }
    if (n == 0 || nrhs == 0) return RFLU_OK;
    RFLU_TRY(ensure_buffer(&h->hostA_dev, &h->hostA_bytes, (size_t)n * (size_t)n * sizeof(T)));
    RFLU_TRY(ensure_buffer(&h->hostB_dev, &h->hostB_bytes, (size_t)n * (size_t)nrhs * sizeof(T)));
    T* dF = static_cast<T*>(h->hostA_dev);
    T* dB = static_cast<T*>(h->hostB_dev);
    const int64_t* dipiv;
    RFLU_TRY(copy_in(dF, F, lda, n, n, h->stream));
    RFLU_TRY(copy_in(dB, B, ldb, n, nrhs, h->stream));
    RFLU_TRY(stage_ipiv(h, ipiv, n, &dipiv));
    RFLU_TRY(trans ? getrs_trans_cm_dev<T>(h, n, nrhs, dF, n, dipiv, dB, n) : getrs_cm_dev<T>(h, n, nrhs, dF, n, dipiv, dB, n));
    RFLU_TRY(copy_out(B, ldb, dB, n, nrhs, h->stream));
    RFLU_HIP(hipStreamSynchronize(h->stream));
    return RFLU_OK;
}

// ---- logabsdet (only the diagonal and ipiv travel) and inv from host factors, real and complex (E: the element trait) ----------------
template <typename E>
int logabsdet_host(Handle* h, int64_t n, const typename E::real* F, int64_t ld, const int64_t* ipiv, double* logabs, double* sign_re,
                   double* sign_im)
{
    typedef typename HostElem<E>::type Z;
    RFLU_TRY(logabsdet_check_args<E>(n, F, ld, logabs, sign_re, sign_im));   // ... and the empty product in the outputs
    if (n == 0) return RFLU_OK;
    const Z* Fz = reinterpret_cast<const Z*>(F);
    std::vector<Z> diag((size_t)n);
    for (int64_t i = 0; i < n; ++i) diag[(size_t)i] = Fz[i * (ld + 1)];
    RFLU_TRY(ensure_buffer(&h->hostB_dev, &h->hostB_bytes, (size_t)n * sizeof(Z)));
    const int64_t* dipiv;
    RFLU_HIP(hipMemcpyAsync(h->hostB_dev, diag.data(), (size_t)n * sizeof(Z), hipMemcpyHostToDevice, h->stream));
    RFLU_TRY(stage_ipiv(h, ipiv, n, &dipiv));
    RFLU_HIP(hipStreamSynchronize(h->stream));   // `diag` is pageable and leaves scope
    return launch_logabsdet<E>(h, n, static_cast<const typename E::real*>(h->hostB_dev), 1, dipiv, logabs, sign_re, sign_im, nullptr);
}

template <typename E>
int getri_host(Handle* h, int64_t n, typename E::real* F, int64_t lda, const int64_t* ipiv, int64_t* info)
{
    typedef typename HostElem<E>::type Z;
    RFLU_TRY(getri_check_args<E>(n, F, lda, info));
    *info = 0;
    if (n == 0) return RFLU_OK;
    RFLU_TRY(ensure_buffer(&h->hostA_dev, &h->hostA_bytes, (size_t)n * (size_t)n * sizeof(Z)));
    Z* dF = static_cast<Z*>(h->hostA_dev);
    const int64_t* dipiv;
    RFLU_TRY(copy_in(dF, reinterpret_cast<const Z*>(F), lda, n, n, h->stream));
    RFLU_TRY(stage_ipiv(h, ipiv, n, &dipiv));
    RFLU_TRY(getri_cm_dev<E>(h, n, reinterpret_cast<typename E::real*>(dF), n, dipiv, info));
    if (*info != 0) return RFLU_OK;   // F stays as it is
    RFLU_TRY(copy_out(reinterpret_cast<Z*>(F), lda, dF, n, n, h->stream));
    RFLU_HIP(hipStreamSynchronize(h->stream));
    return RFLU_OK;
}

// rcond from host factors: H2D, then the device entry (which checks norm and anorm and serves the special values)
template <typename T>
int gecon_host(Handle* h, int norm, int64_t n, const T* F, int64_t lda, double anorm, double* rcond)
{
    if (n < 0 || lda < std::max<int64_t>(n, 1) || rcond == nullptr || (n > 0 && F == nullptr)) {
        set_error("gecon: bad arguments n=%lld lda=%lld (or a null pointer)", (long long)n, (long long)lda);
        return RFLU_ERR_ARG;
    }
    if (n == 0) return gecon_dev<T>(h, norm, 0, F, 1, 0, anorm, rcond);
    RFLU_TRY(ensure_buffer(&h->hostA_dev, &h->hostA_bytes, (size_t)n * (size_t)n * sizeof(T)));
    T* dF = static_cast<T*>(h->hostA_dev);
    RFLU_TRY(copy_in(dF, F, lda, n, n, h->stream));
    RFLU_HIP(hipStreamSynchronize(h->stream));   // the special values return without another wait: the caller's array is free by then
    return gecon_dev<T>(h, norm, n, dF, n, 0, anorm, rcond);
}

// ---- the way back of the factors, overlapped with the factorization -------------------------------------------------------------------
// Rows [0, r) of the factors are final as soon as every block column left of r has been applied everywhere (later interchanges only
// touch rows below), and in the row-major workspace a block of rows is one contiguous piece.  Once the factorization is enqueued
// (Handle::before_sync: 7 ms into 80 ms at N=16384) the calling thread -- which would only wait now -- brings the pieces of a ChunkPlan
// home on a stream of its own: ready(k) makes piece k final with respect to that stream, the piece is transposed into one half of a
// column-major staging area, copied in one go into a pinned bounce buffer, and from there into the caller's columns with a few host
// threads while the next piece is on the link.  This needs (1) the out stream on a hardware pipe of its own (validate_queues; without:
// +26 ms instead of -30) and (2) bounce buffers of our own: a device-to-host copy into PAGEABLE memory issued next to the running
// factorization returns only when that has finished (scripts/probes/d2h_block.hip).  The device copy of the INPUT stays intact until the
// factorization has succeeded, so a failure known only at the end (a panel timeout) gives the caller's matrix back (give_back).
// The transposes go through launch_transpose_on on both paths, so the in-schedule profile (rflu_profile_enable(2)) does not count them;
// nothing profiles a host-entry call (SchedPlan::host_early is false under the synchronous modes, bench.py switches profiling off first).
template <typename T>
struct WayBack {
    Handle* h;
    T* A;   // the caller's matrix: m x n, column-major, leading dimension lda
    int64_t lda, m, n;
    const char* label;   // of the trace lines (RFLU_HOST_TRACE)
    std::chrono::steady_clock::time_point t_call = std::chrono::steady_clock::now();
    size_t ev_used = 0;       // of the handle's event pool (out_events), shared with the caller's own events
    bool scattered = false;   // finished rows have reached A

    double since_call() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count(); }
    int new_event(hipEvent_t* e)
    {
        if (ev_used == h->out_events.size()) {
            hipEvent_t x;
            RFLU_HIP(hipEventCreateWithFlags(&x, hipEventDisableTiming));
            h->out_events.push_back(x);
        }
        *e = h->out_events[ev_used++];
        return RFLU_OK;
    }

    // R, ldr: the row-major workspace the factors are in; sets Handle::out_done when everything is home
    template <typename Ready>
    int run(const T* R, int64_t ldr, hipStream_t out, const ChunkPlan& plan, Ready ready)
    {
        const size_t nchunks = plan.ends.size();
        const size_t piece_elems = (size_t)std::min(plan.chunk, m) * (size_t)n;
        const int nthreads = std::max(1, std::min(h->tune.host_threads, 64));
        std::vector<hipEvent_t> landed(nchunks);
        auto send = [&](size_t k) -> int {   // piece k: final -> transpose into its half of the staging area -> bounce buffer
            const int64_t r0 = plan.start(k), rows = plan.ends[k] - r0;
            RFLU_TRY(ready(k));
            T* piece = static_cast<T*>(h->out_stage) + (k & 1) * piece_elems;
            RFLU_TRY(launch_transpose_on<T>(out, n, rows, R + r0 * ldr, ldr, piece, rows));
            RFLU_HIP(hipMemcpyAsync(h->bounce[k & 1], piece, (size_t)rows * (size_t)n * sizeof(T), hipMemcpyDeviceToHost, out));
            RFLU_TRY(new_event(&landed[k]));
            RFLU_HIP(hipEventRecord(landed[k], out));
            return RFLU_OK;
        };
        for (size_t k = 0; k < std::min<size_t>(2, nchunks); ++k) RFLU_TRY(send(k));
        for (size_t k = 0; k < nchunks; ++k) {
            RFLU_HIP(hipEventSynchronize(landed[k]));
            const int64_t r0 = plan.start(k), rows = plan.ends[k] - r0;
            scattered = true;
            scatter_columns(A, lda, r0, static_cast<const T*>(h->bounce[k & 1]), rows, n, nthreads);
            if (h->tune.host_trace) fprintf(stderr, "[rflu] %s: rows [%lld, %lld) home at %.1f ms\n", label, (long long)r0, (long long)plan.ends[k], since_call());
            if (k + 2 < nchunks) RFLU_TRY(send(k + 2));   // its bounce buffer is free again
        }
        h->out_done = true;
        return RFLU_OK;
    }

    // a failed call: rows that went home early are overwritten with the input again (dA is only written after success); error text kept
    void give_back(const T* dA)
    {
        if (!scattered) return;
        (void)hipDeviceSynchronize();
        (void)hipMemcpy2D(A, (size_t)lda * sizeof(T), dA, (size_t)m * sizeof(T), (size_t)m * sizeof(T), (size_t)n, hipMemcpyDeviceToHost);
    }
};

// ---- host entry through the update engine: the way in overlaps the factorization (round 5) -----------------------------------------
// Round 3 overlapped the way BACK with the factorization; the way in (38 ms of PCIe for a 16384^2 Float64 matrix) still preceded
// everything, because the stream schedules' first update touches every column.  The engine's per-column-block dataflow does not: a
// column block's operations become eligible when its columns have arrived, so the matrix is fed in block column by block column (a
// second host thread: copies from pageable memory block their caller) -- copy, layout change, a word that says how many columns are in
// place -- while the critical-path stream, which waits on the same word, factors what is there; finished block rows leave as before,
// told by a host-visible word the engine keeps (EngArgs::rows_final) instead of events.  Every block column goes through the engine
// here (no hand-over to the streams).  Called where the plan says so (SchedPlan::host_engine).  *handled = false: no CU-masked streams
// or no pinned memory to be had (the caller falls back to getrf_host's sequence).
template <typename T>
static int getrf_host_engine(Handle* h, int64_t m, int64_t n, T* A, int64_t lda, int64_t* ipiv, int pivot, int64_t blocksize,
                             const SchedPlan& plan, int64_t* info, bool* handled)
{
    *handled = false;
    const int64_t mn = std::min(m, n);
    const int64_t chunk = h->tune.host_early_out;
    const int64_t ldr = workspace_ld(h, n);
    hipStream_t E, IN, OUT;
    RFLU_TRY(get_ustream(h, 32, &E));
    RFLU_TRY(get_ustream(h, 64, &E));    // (what getrf_rm creates before it settles the queues: nothing new appears afterwards)
    RFLU_TRY(get_pstream(h, 32, &IN));   // streams confined to the CUs the resident engine leaves free: anything else would wait for it
    RFLU_TRY(get_pstream(h, 64, &OUT));
    if (h->mask_failed) return RFLU_OK;
    RFLU_TRY(validate_queues(h));
    RFLU_TRY(get_pstream(h, 32, &IN));
    RFLU_TRY(get_pstream(h, 64, &OUT));
    // buffers: device copy of the input (kept intact for a failed call), row-major workspace, staging + pinned bounce buffers of the way back
    RFLU_TRY(ensure_buffer(&h->hostA_dev, &h->hostA_bytes, (size_t)m * (size_t)n * sizeof(T)));
    RFLU_TRY(ensure_buffer(&h->work, &h->work_bytes, (size_t)m * (size_t)ldr * sizeof(T)));
    RFLU_TRY(ensure_ipiv_dev(h, mn));
    const size_t bounce_bytes = (size_t)std::min(chunk, m) * (size_t)n * sizeof(T);
    RFLU_TRY(ensure_buffer(&h->out_stage, &h->out_stage_bytes, 2 * bounce_bytes));
    bool pinned;
    RFLU_TRY(ensure_bounce(h, bounce_bytes, &pinned));
    if (!pinned) return RFLU_OK;
    RFLU_TRY(ensure_engine_state(h));
    if (!h->eng_rows_final) {
        void* p = nullptr;
        if (hipHostMalloc(&p, 64, hipHostMallocMapped) != hipSuccess) { (void)hipGetLastError(); return RFLU_OK; }
        h->eng_rows_final = static_cast<unsigned long long*>(p);
        void* d = nullptr;
        RFLU_HIP(hipHostGetDevicePointer(&d, p, 0));
        h->eng_rows_final_dev = static_cast<unsigned long long*>(d);
    }
    *handled = true;
    *info = 0;
    EngState* est = static_cast<EngState*>(h->eng_state);
    T* dA = static_cast<T*>(h->hostA_dev);
    T* R = static_cast<T*>(h->work);
    const hipStream_t user = h->stream;
    WayBack<T> back{h, A, lda, m, n, "host entry (engine)"};
    __atomic_store_n(h->eng_rows_final, 0ull, __ATOMIC_RELEASE);
    RFLU_HIP(hipMemsetAsync(&est->arrived, 0, sizeof(unsigned long long), user));
    RFLU_HIP(hipStreamSynchronize(user));   // (whatever the caller had in flight on this stream is done, the arrival word reads 0)
    // ---- the way in: a thread of its own (a copy from pageable memory returns when the data has left the host)
    std::atomic<int> feed_status{RFLU_OK};
    std::atomic<bool> feed_stop{false};
    const int device = h->device;
    const int64_t in_cols = std::max<int64_t>(plan.Wb, 512);
    std::thread feeder([&, device]() {
        if (hipSetDevice(device) != hipSuccess) { feed_status = RFLU_ERR_HIP; return; }
        for (int64_t c0 = 0; c0 < n && !feed_stop.load(); c0 += in_cols) {
            const int64_t nc = std::min(in_cols, n - c0);
            if (copy_in(dA + c0 * m, A + c0 * lda, lda, m, nc, IN) != RFLU_OK ||
                launch_transpose_on<T>(IN, m, nc, dA + c0 * m, m, R + c0, ldr) != RFLU_OK ||
                launch_gate_signal_on(IN, &est->arrived, (unsigned long long)(c0 + nc)) != RFLU_OK) {
                feed_status = RFLU_ERR_HIP;
                return;
            }
        }
    });
    struct Join { std::thread& t; std::atomic<bool>& stop; ~Join() { stop = true; if (t.joinable()) t.join(); } } join{feeder, feed_stop};
    // ---- the way back: on this thread once the factorization is enqueued, chunk by chunk as the engine reports block rows final
    struct Reset { Handle* h; ~Reset() { h->before_sync = nullptr; h->out_done = false; h->eng_host_mode = false; } } reset{h};
    h->eng_host_mode = true;
    h->before_sync = [&]() -> int {
        hipEvent_t all_done;
        RFLU_TRY(back.new_event(&all_done));
        RFLU_HIP(hipEventRecord(all_done, user));   // the whole factorization (the critical-path stream joins the engine's at its end)
        if (h->tune.host_trace) fprintf(stderr, "[rflu] host entry (engine): enqueue done %.1f ms after the call\n", back.since_call());
        ChunkPlan pieces{m, chunk};
        pieces.complete();
        bool everything = false;
        auto ready = [&](size_t k) -> int {   // rows [0, ends[k]) final: the engine's word, or the end of everything
            const auto t0 = std::chrono::steady_clock::now();
            while (!everything && (int64_t)__atomic_load_n(h->eng_rows_final, __ATOMIC_ACQUIRE) < pieces.ends[k]) {
                const hipError_t q = hipEventQuery(all_done);
                if (q == hipSuccess) { everything = true; break; }
                if (q != hipErrorNotReady) { set_error("hipEventQuery failed: %s", hipGetErrorString(q)); return RFLU_ERR_HIP; }
                if (feed_status.load() != RFLU_OK) { set_error("host entry: feeding the matrix to the device failed"); return RFLU_ERR_HIP; }
                if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(20)) { set_error("host entry: no progress for 20 s"); return RFLU_ERR_TIMEOUT; }
                std::this_thread::sleep_for(std::chrono::microseconds(20));
            }
            return RFLU_OK;
        };
        return back.run(R, ldr, OUT, pieces, ready);
    };
    int rc = getrf_rm<T>(h, m, n, R, ldr, (pivot || ipiv) ? h->ipiv_dev : nullptr, pivot, blocksize, info);
    feed_stop = true;
    if (feeder.joinable()) feeder.join();
    if (rc == RFLU_OK && feed_status.load() != RFLU_OK) { set_error("host entry: feeding the matrix to the device failed"); rc = feed_status.load(); }
    if (rc != RFLU_OK) {
        (void)hipDeviceSynchronize();   // (the feeding stream and the engine included: the device copy of the input is never written by the factorization)
        back.give_back(dA);
        return rc;
    }
    if (!h->out_done) {   // (cannot happen: before_sync either brings everything home or fails)
        set_error("host entry: the factors did not travel back");
        return RFLU_ERR_ARG;
    }
    if (ipiv) RFLU_HIP(hipMemcpyAsync(ipiv, h->ipiv_dev, (size_t)mn * sizeof(int64_t), hipMemcpyDeviceToHost, user));
    RFLU_HIP(hipStreamSynchronize(user));
    RFLU_HIP(hipStreamSynchronize(IN));
    return RFLU_OK;
}

// ---- rflu_getrf_*: through the engine where the plan says so, else staged through the column-major device entry -----------------------
// The stream schedules report how far they have got while they enqueue (Handle::progress); per piece of rows the events of every
// stream are kept, and the way-back stream waits for them.  RFLU_HOST_EARLY_OUT=0: everything travels after the factorization.
template <typename T>
int getrf_host(Handle* h, int64_t m, int64_t n, T* A, int64_t lda, int64_t* ipiv, int pivot, int64_t blocksize, int64_t* info)
{
    if (m < 0 || n < 0 || lda < std::max<int64_t>(m, 1) || info == nullptr || (m > 0 && n > 0 && A == nullptr)) {
        set_error("getrf: bad arguments m=%lld n=%lld lda=%lld", (long long)m, (long long)n, (long long)lda);
        return RFLU_ERR_ARG;
    }
    *info = 0;
    const int64_t mn = std::min(m, n);
    if (mn == 0) return RFLU_OK;
    const SchedPlan p = plan_schedule(sched_in(h, m, n, sizeof(T), pivot, blocksize, ENTRY_HOST, true, workspace_ld(h, n)));   // (workspace: hipMalloc)
    if (p.host_engine) {   // the way in overlapped with the factorization (the update engine's dataflow waits for columns; the stream schedules cannot)
        bool handled = false;
        const int rc = getrf_host_engine<T>(h, m, n, A, lda, ipiv, pivot, blocksize, p, info, &handled);
        if (handled || rc != RFLU_OK) return rc;
    }
    RFLU_TRY(ensure_buffer(&h->hostA_dev, &h->hostA_bytes, (size_t)m * (size_t)n * sizeof(T)));
    RFLU_TRY(ensure_ipiv_dev(h, mn));
    T* dA = static_cast<T*>(h->hostA_dev);
    WayBack<T> back{h, A, lda, m, n, "host entry"};
    RFLU_TRY(copy_in(dA, A, lda, m, n, h->stream));
    const auto t_in = std::chrono::steady_clock::now();
    const int64_t chunk = h->tune.host_early_out;
    ChunkPlan pieces{m, chunk};
    std::vector<std::vector<hipEvent_t>> events;   // of piece k: what every stream had enqueued when the piece was reported final
    hipStream_t C = nullptr;
    struct Reset { Handle* h; ~Reset() { h->progress = nullptr; h->before_sync = nullptr; h->out_done = false; } } reset{h};
    if (p.host_early) {
        RFLU_TRY(get_ustream(h, 96, &C));   // a masked stream = a queue of its own that validate_queues can place
        if (h->mask_failed) C = nullptr;
    }
    if (C) {   // staging area and bounce buffers; without them the plain sequence
        const size_t bounce_bytes = (size_t)std::min(chunk, m) * (size_t)n * sizeof(T);
        bool pinned = false;
        if (ensure_buffer(&h->out_stage, &h->out_stage_bytes, 2 * bounce_bytes) == RFLU_OK) RFLU_TRY(ensure_bounce(h, bounce_bytes, &pinned));
        if (!pinned) C = nullptr;
    }
    if (C) {
        const hipStream_t user = h->stream;
        auto mark_all = [h, user, &back](std::vector<hipEvent_t>& out) -> int {
            auto rec = [&](hipStream_t st) -> int {
                hipEvent_t e;
                RFLU_TRY(back.new_event(&e));
                RFLU_HIP(hipEventRecord(e, st));
                out.push_back(e);
                return RFLU_OK;
            };
            RFLU_TRY(rec(user));
            if (h->stream != user) RFLU_TRY(rec(h->stream));
            for (int r = 1; r < 8; ++r) {
                if (r != 3 && h->ustreams[r]) RFLU_TRY(rec(h->ustreams[r]));
                if (h->pstreams[r] && h->pstreams[r] != h->stream) RFLU_TRY(rec(h->pstreams[r]));
            }
            return RFLU_OK;
        };
        h->progress = [&pieces, &events, mark_all](int64_t r) -> int {
            if (!pieces.report(r)) return RFLU_OK;
            events.emplace_back();
            return mark_all(events.back());
        };
        h->before_sync = [&, mark_all]() -> int {
            if (pieces.have() < m) {   // whatever is left is final when everything is
                std::vector<hipEvent_t> all;
                RFLU_TRY(mark_all(all));
                events.insert(events.end(), pieces.complete(), all);
            }
            // the way-back stream as it is NOW: validate_queues (run by the factorization, after C was first taken) may have parked the
            // stream of this mask and put a fresh one, on a pipe of its own, in its place
            RFLU_TRY(get_ustream(h, 96, &C));
            if (h->tune.host_trace)
                fprintf(stderr, "[rflu] host entry: enqueue done %.1f ms after the call (%.1f after the copy in), %zu chunks\n", back.since_call(),
                        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_in).count(), pieces.ends.size());
            auto ready = [&](size_t k) -> int {
                for (hipEvent_t e : events[k])
                    if (hipStreamWaitEvent(C, e, 0) != hipSuccess) { set_error("hipStreamWaitEvent failed"); return RFLU_ERR_HIP; }
                return RFLU_OK;
            };
            return back.run(static_cast<const T*>(h->work), workspace_ld(h, n), C, pieces, ready);
        };
    }
    const int rc = getrf_cm_dev<T>(h, m, n, dA, m, (pivot || ipiv) ? h->ipiv_dev : nullptr, pivot, blocksize, info);
    if (rc != RFLU_OK) {
        back.give_back(dA);
        return rc;
    }
    if (!h->out_done) RFLU_TRY(copy_out(A, lda, dA, m, n, h->stream));
    if (ipiv) RFLU_HIP(hipMemcpyAsync(ipiv, h->ipiv_dev, (size_t)mn * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    RFLU_HIP(hipStreamSynchronize(h->stream));
    return RFLU_OK;
}

// ---- ComplexF64 / ComplexF32 (complex.hip): H2D, the device entry, D2H -- the factors travel only after success, so a failed call
// leaves the caller's matrix as it was.  R* points at interleaved (re, im) pairs, lda / ldb count complex elements.
template <typename R>
int cgetrf_host(Handle* h, int64_t m, int64_t n, R* A, int64_t lda, int64_t* ipiv, int pivot, int64_t* info)
{
    typedef HostCx<R> Z;
    RFLU_TRY(cgetrf_check_args(m, n, A, lda, ipiv, pivot, info));
    *info = 0;
    const int64_t mn = std::min(m, n);
    if (mn == 0) return RFLU_OK;
    RFLU_TRY(ensure_buffer(&h->hostA_dev, &h->hostA_bytes, (size_t)m * (size_t)n * sizeof(Z)));
    RFLU_TRY(ensure_ipiv_dev(h, mn));
    Z* dA = static_cast<Z*>(h->hostA_dev);
    RFLU_TRY(copy_in(dA, reinterpret_cast<const Z*>(A), lda, m, n, h->stream));
    RFLU_TRY(cgetrf_cm_dev<R>(h, m, n, reinterpret_cast<R*>(dA), m, ipiv ? h->ipiv_dev : nullptr, pivot, info));
    RFLU_TRY(copy_out(reinterpret_cast<Z*>(A), lda, dA, m, n, h->stream));
    if (ipiv) RFLU_HIP(hipMemcpyAsync(ipiv, h->ipiv_dev, (size_t)mn * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    RFLU_HIP(hipStreamSynchronize(h->stream));
    return RFLU_OK;
}

template <typename R>
int cgetrs_host(Handle* h, int64_t n, int64_t nrhs, const R* F, int64_t lda, const int64_t* ipiv, R* B, int64_t ldb)
{
    typedef HostCx<R> Z;
    RFLU_TRY(cgetrs_check_args(n, nrhs, F, lda, B, ldb));
    if (n == 0 || nrhs == 0) return RFLU_OK;
    RFLU_TRY(ensure_buffer(&h->hostA_dev, &h->hostA_bytes, (size_t)n * (size_t)n * sizeof(Z)));
    RFLU_TRY(ensure_buffer(&h->hostB_dev, &h->hostB_bytes, (size_t)n * (size_t)nrhs * sizeof(Z)));
    Z* dF = static_cast<Z*>(h->hostA_dev);
    Z* dB = static_cast<Z*>(h->hostB_dev);
    const int64_t* dipiv;
    RFLU_TRY(copy_in(dF, reinterpret_cast<const Z*>(F), lda, n, n, h->stream));
    RFLU_TRY(copy_in(dB, reinterpret_cast<const Z*>(B), ldb, n, nrhs, h->stream));
    RFLU_TRY(stage_ipiv(h, ipiv, n, &dipiv));
    RFLU_TRY(cgetrs_cm_dev<R>(h, n, nrhs, reinterpret_cast<const R*>(dF), n, dipiv, reinterpret_cast<R*>(dB), n));
    RFLU_TRY(copy_out(reinterpret_cast<Z*>(B), ldb, dB, n, nrhs, h->stream));
    RFLU_HIP(hipStreamSynchronize(h->stream));
    return RFLU_OK;
}

// ldiv!(transpose(F), B) / ldiv!(F', B): the same staging, the transposed device entry in the middle
template <typename R>
int cgetrs_trans_host(Handle* h, int64_t n, int64_t nrhs, const R* F, int64_t lda, const int64_t* ipiv, R* B, int64_t ldb, int conj)
{
    typedef HostCx<R> Z;
    RFLU_TRY(cgetrs_trans_check_args(n, nrhs, F, lda, B, ldb, conj));
    if (n == 0 || nrhs == 0) return RFLU_OK;
    RFLU_TRY(ensure_buffer(&h->hostA_dev, &h->hostA_bytes, (size_t)n * (size_t)n * sizeof(Z)));
    RFLU_TRY(ensure_buffer(&h->hostB_dev, &h->hostB_bytes, (size_t)n * (size_t)nrhs * sizeof(Z)));
    Z* dF = static_cast<Z*>(h->hostA_dev);
    Z* dB = static_cast<Z*>(h->hostB_dev);
    const int64_t* dipiv;
    RFLU_TRY(copy_in(dF, reinterpret_cast<const Z*>(F), lda, n, n, h->stream));
    RFLU_TRY(copy_in(dB, reinterpret_cast<const Z*>(B), ldb, n, nrhs, h->stream));
    RFLU_TRY(stage_ipiv(h, ipiv, n, &dipiv));
    RFLU_TRY(cgetrs_trans_cm_dev<R>(h, n, nrhs, reinterpret_cast<const R*>(dF), n, dipiv, reinterpret_cast<R*>(dB), n, conj));
    RFLU_TRY(copy_out(reinterpret_cast<Z*>(B), ldb, dB, n, nrhs, h->stream));
    RFLU_HIP(hipStreamSynchronize(h->stream));
    return RFLU_OK;
}

// rcond from complex host factors: H2D, then the device entry (which checks norm and anorm and serves the special values)
template <typename R>
int cgecon_host(Handle* h, int norm, int64_t n, const R* F, int64_t lda, double anorm, double* rcond)
{
    typedef HostCx<R> Z;
    if (n < 0 || lda < std::max<int64_t>(n, 1) || rcond == nullptr || (n > 0 && F == nullptr)) {
        set_error("complex gecon: bad arguments n=%lld lda=%lld (or a null pointer)", (long long)n, (long long)lda);
        return RFLU_ERR_ARG;
    }
    if (n == 0) return cgecon_dev<R>(h, norm, 0, F, 1, anorm, rcond);
    RFLU_TRY(ensure_buffer(&h->hostA_dev, &h->hostA_bytes, (size_t)n * (size_t)n * sizeof(Z)));
    Z* dF = static_cast<Z*>(h->hostA_dev);
    RFLU_TRY(copy_in(dF, reinterpret_cast<const Z*>(F), lda, n, n, h->stream));
    RFLU_HIP(hipStreamSynchronize(h->stream));   // the special values return without another wait: the caller's array is free by then
    return cgecon_dev<R>(h, norm, n, reinterpret_cast<const R*>(dF), n, anorm, rcond);
}

#define RFLU_INSTANTIATE_HOST(T)                                                                                                      \
    template int getrf_host<T>(Handle*, int64_t, int64_t, T*, int64_t, int64_t*, int, int64_t, int64_t*);                             \
    template int getrs_host<T>(Handle*, int64_t, int64_t, const T*, int64_t, const int64_t*, T*, int64_t, bool);                      \
    template int getri_host<RealElem<T>>(Handle*, int64_t, T*, int64_t, const int64_t*, int64_t*);                                    \
    template int logabsdet_host<RealElem<T>>(Handle*, int64_t, const T*, int64_t, const int64_t*, double*, double*, double*);         \
    template int gecon_host<T>(Handle*, int, int64_t, const T*, int64_t, double, double*);
RFLU_INSTANTIATE_HOST(double)
RFLU_INSTANTIATE_HOST(float)
#define RFLU_INSTANTIATE_HOST_COMPLEX(R)                                                                                              \
    template int cgetrf_host<R>(Handle*, int64_t, int64_t, R*, int64_t, int64_t*, int, int64_t*);                                     \
    template int cgetrs_host<R>(Handle*, int64_t, int64_t, const R*, int64_t, const int64_t*, R*, int64_t);                           \
    template int cgetrs_trans_host<R>(Handle*, int64_t, int64_t, const R*, int64_t, const int64_t*, R*, int64_t, int);             \
    template int getri_host<CplxElem<R>>(Handle*, int64_t, R*, int64_t, const int64_t*, int64_t*);                                    \
    template int logabsdet_host<CplxElem<R>>(Handle*, int64_t, const R*, int64_t, const int64_t*, double*, double*, double*);         \
    template int cgecon_host<R>(Handle*, int, int64_t, const R*, int64_t, double, double*);
RFLU_INSTANTIATE_HOST_COMPLEX(double)
RFLU_INSTANTIATE_HOST_COMPLEX(float)

}  // namespace rflu
