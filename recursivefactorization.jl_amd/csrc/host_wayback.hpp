// host_wayback.hpp -- the two pieces of the host entry's way back (host_entry.cpp: WayBack) that are plain host arithmetic: which rows
// travel together, and how a landed chunk is copied into the caller's columns.  No HIP, no handle: tests/host_wayback_check.cpp checks
// both on the CPU.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

namespace rflu {

// ---- the chunk plan: rows [0, m) cut into pieces of at most `chunk` rows, in the order in which they become final -----------------
// The stream schedules report how far they have got (report(r): every kernel that writes rows [0, r) is enqueued).  Far from the end a
// piece is a whole chunk; within one chunk of the end every report makes a piece (one block column at a time), so that little is left
// when the last leaf finishes.  complete() cuts what no report covered (the rows below the square part of a tall matrix included) into
// chunk-sized pieces; without any report -- the engine path, whose rows are told final by a host word -- that is the whole plan.
// No piece exceeds min(chunk, m) rows: a piece has to fit a bounce buffer and its half of the staging area.
struct ChunkPlan {
    int64_t m = 0, chunk = 0;
    std::vector<int64_t> ends;   // r1 of every piece, increasing; piece k is [start(k), ends[k])
    int64_t have() const { return ends.empty() ? 0 : ends.back(); }
    int64_t start(size_t k) const { return k == 0 ? 0 : ends[k - 1]; }
    bool report(int64_t r)       // true: a piece was added (the caller records its events)
    {
        r = std::min(r, m);
        if (r <= have() || (r - have() < chunk && r + chunk < m)) return false;
        ends.push_back(std::min(r, have() + chunk));
        return true;
    }
    size_t complete()            // number of pieces added: all of them final when everything is
    {
        size_t added = 0;
        for (; have() < m; ++added) ends.push_back(std::min(m, have() + chunk));
        return added;
    }
};

// ---- the scatter: a landed chunk (rows [r0, r0 + rows) of all n columns, packed column-major in `src`) into the caller's columns -----
constexpr size_t SCATTER_SINGLE_BYTES = (size_t)8 << 20;   // below this one thread is as fast as several

// Columns are split evenly over nthreads; the calling thread takes the first share and whatever threads could not be started.
template <typename T>
void scatter_columns(T* A, int64_t lda, int64_t r0, const T* src, int64_t rows, int64_t n, int nthreads)
{
    auto scatter = [=](int64_t j0, int64_t j1) {
        for (int64_t j = j0; j < j1; ++j) memcpy(A + j * lda + r0, src + j * rows, (size_t)rows * sizeof(T));
    };
    if (nthreads <= 1 || (size_t)rows * (size_t)n * sizeof(T) < SCATTER_SINGLE_BYTES) return scatter(0, n);
    std::vector<std::thread> pool;
    const int64_t per = (n + nthreads - 1) / nthreads;
    int64_t done_to = std::min<int64_t>(n, per);   // columns [per, done_to) have a thread; no exception leaves a C entry
    try {
        for (int t = 1; t < nthreads; ++t) {
            pool.emplace_back(scatter, std::min<int64_t>(n, t * per), std::min<int64_t>(n, (t + 1) * per));
            done_to = std::min<int64_t>(n, (t + 1) * per);
        }
    } catch (...) {
    }
    scatter(0, std::min<int64_t>(n, per));
    if (done_to < n) scatter(done_to, n);
    for (std::thread& th : pool) th.join();
}

}  // namespace rflu
