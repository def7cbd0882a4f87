// Host-side check of the two pure pieces of the host entry's way back (csrc/host_wayback.hpp): the chunk plan (which rows travel together)
// and the threaded column scatter (a landed chunk into the caller's columns).  Compiled and run by tests/test_host_wayback.py (no GPU).
#include <cstdio>
#include <vector>
#include "host_wayback.hpp"
using namespace rflu;

static int bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (bad++ < 20) { printf(__VA_ARGS__); printf("  [%s]\n", #cond); } } } while (0)

// W = 0: no report arrives (the engine path, or a stream schedule that reports nothing): the plain list of chunk ends
static void check_plan(int64_t m, int64_t n, int64_t chunk, int64_t W)
{
    ChunkPlan p{m, chunk};
    const int64_t mn = std::min(m, n);
    int64_t prev = -1;   // the report before this one
    for (int64_t k = 1; W > 0 && prev < mn; ++k) {
        const int64_t r = std::min(k * W, mn), have = p.have();
        const bool added = p.report(r);
        if (added) CHECK(p.have() > have && p.have() <= r, "m=%lld n=%lld chunk=%lld W=%lld: report %lld made piece [%lld, %lld)\n", (long long)m, (long long)n, (long long)chunk, (long long)W, (long long)r, (long long)have, (long long)p.have());
        // within one chunk of the end no report is held back, and once the report before was there too a piece is at most one block
        // column's worth of reports
        if (r + chunk >= m && r > have) CHECK(added, "m=%lld n=%lld chunk=%lld W=%lld: report %lld held back\n", (long long)m, (long long)n, (long long)chunk, (long long)W, (long long)r);
        if (added && prev >= 0 && prev + chunk >= m)
            CHECK(p.have() - have <= W, "m=%lld n=%lld chunk=%lld W=%lld: piece [%lld, %lld) merges reports\n", (long long)m, (long long)n, (long long)chunk, (long long)W, (long long)have, (long long)p.have());
        prev = r;
    }
    const size_t reported = p.ends.size();
    CHECK(p.complete() == p.ends.size() - reported, "complete() miscounts\n");
    // in order, disjoint, covering [0, m) exactly; no piece larger than a bounce buffer
    int64_t at = 0;
    for (size_t k = 0; k < p.ends.size(); ++k) {
        CHECK(p.start(k) == at && p.ends[k] > at, "m=%lld n=%lld chunk=%lld W=%lld: piece %zu is [%lld, %lld) after %lld\n", (long long)m, (long long)n, (long long)chunk, (long long)W, k, (long long)p.start(k), (long long)p.ends[k], (long long)at);
        CHECK(p.ends[k] - at <= std::min(chunk, m), "m=%lld n=%lld chunk=%lld W=%lld: piece %zu has %lld rows\n", (long long)m, (long long)n, (long long)chunk, (long long)W, k, (long long)(p.ends[k] - at));
        at = p.ends[k];
    }
    CHECK(at == m, "m=%lld n=%lld chunk=%lld W=%lld: pieces end at %lld\n", (long long)m, (long long)n, (long long)chunk, (long long)W, (long long)at);
    if (W == 0) {   // the list as the engine path wrote it out before
        std::vector<int64_t> ends;
        for (int64_t r = 0; r < m;) { r = std::min(m, r + chunk); ends.push_back(r); }
        CHECK(ends == p.ends, "m=%lld chunk=%lld: plain list differs\n", (long long)m, (long long)chunk);
    }
}

// rows [r0, r0 + rows) of an m x n matrix (leading dimension lda > m, sentinel everywhere) from a packed chunk of distinct values
template <typename T>
static void check_scatter(int64_t rows, int64_t n, int nthreads)
{
    const int64_t r0 = 2, m = r0 + rows + 1, lda = m + 3;
    const T sentinel = T(-1);
    std::vector<T> A((size_t)lda * (size_t)n, sentinel), src((size_t)rows * (size_t)n);
    for (size_t i = 0; i < src.size(); ++i) src[i] = T(i % 1000003 + 1);
    scatter_columns(A.data(), lda, r0, src.data(), rows, n, nthreads);
    int64_t wrong = 0;
    for (int64_t j = 0; j < n; ++j)
        for (int64_t i = 0; i < lda; ++i) {
            const bool inside = i >= r0 && i < r0 + rows;
            wrong += A[(size_t)(j * lda + i)] != (inside ? src[(size_t)(j * rows + i - r0)] : sentinel);
        }
    CHECK(wrong == 0, "scatter rows=%lld n=%lld threads=%d (%zu bytes): %lld elements wrong\n", (long long)rows, (long long)n, nthreads, src.size() * sizeof(T), (long long)wrong);
}

int main()
{
    long plans = 0, scatters = 0;
    for (int64_t m : {8192, 8200, 10000, 12288, 16384, 16385})
        for (int64_t chunk : {(int64_t)64, (int64_t)512, (int64_t)1024, (int64_t)2048, m, m + 1})
            for (int64_t n : {m, m - 1808})
                for (int64_t W : {0, 256, 512}) { check_plan(m, n, chunk, W); ++plans; }
    // (rows, n): below the 8 MiB threshold (one thread whatever nthreads), just below it, above it with n not a multiple of any nthreads,
    // and above it with fewer columns than threads
    const int64_t shapes[][2] = {{5, 1001}, {16, 65535}, {16, 70001}, {350000, 3}};
    for (const auto& s : shapes)
        for (int nthreads : {1, 2, 3, 8, 64}) { check_scatter<double>(s[0], s[1], nthreads); ++scatters; }
    check_scatter<float>(32, 70001, 3);
    ++scatters;
    static_assert(SCATTER_SINGLE_BYTES == (size_t)8 << 20, "the single-thread threshold is 8 MiB");
    CHECK((size_t)16 * 65535 * 8 < SCATTER_SINGLE_BYTES && (size_t)16 * 70001 * 8 >= SCATTER_SINGLE_BYTES && (size_t)350000 * 3 * 8 >= SCATTER_SINGLE_BYTES, "shapes miss the threshold\n");
    printf("host_wayback_check: %ld chunk plans, %ld scatters, %d violations\n", plans, scatters, bad);
    return bad ? 1 : 0;
}
