// Host-side check of the schedule choice (csrc/schedule_plan.hpp: plan_schedule, the function every entry of driver.cpp asks): a table of
// expected plans (default environment, 256 CUs), and invariants over a grid of shapes, element sizes, block widths, tunings and handle
// states -- among them that a host entry sent through the engine gets a plan the engine serves to the end, so that getrf_rm's guard
// ("host entry through the engine asked for a schedule the engine cannot serve") cannot fire.  Compiled and run by
// tests/test_schedule_plan.py (no GPU).
#include <cstdio>
#include <vector>
#include "schedule_plan.hpp"
using namespace rflu;

static int bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (bad++ < 20) { printf(__VA_ARGS__); printf("  [%s]\n", #cond); } } } while (0)

static SchedIn call(int64_t m, int64_t n, int entry = ENTRY_RM, size_t esize = 8, int pivot = 1, int64_t blocksize = 0)
{
    SchedIn in;
    in.m = m; in.n = n; in.esize = esize; in.pivot = pivot; in.blocksize = blocksize; in.entry = entry;
    in.ld = (n + 15) / 16 * 16;
    return in;
}

struct Row {
    const char* name;
    SchedIn in;
    int path;
    int64_t Wb, b_switch, eng_end;   // -1: not checked
};

int main()
{
    // ---- the table (expected values derived from the schedule rules as they were before they moved into plan_schedule) ----
    SchedIn noeng = call(16384, 16384);
    noeng.tune.engine = 0;
    SchedIn prof = call(16384, 16384);
    prof.prof = true;
    SchedIn cus304 = call(16384, 16384);
    cus304.num_cus = 304;
    const int REC = RFLU_PATH_HIP_RECURSIVE, BLK = RFLU_PATH_HIP_BLOCKED, LA = RFLU_PATH_HIP_LOOKAHEAD, ENG = RFLU_PATH_HIP_ENGINE;
    const std::vector<Row> rows = {
        {"N=512", call(512, 512), REC, -1, -1, -1},
        {"N=4096", call(4096, 4096), LA, 256, 0, 0},
        {"N=11264", call(11264, 11264), LA, 256, 12, 0},
        {"N=12288 column-major", call(12288, 12288, ENTRY_CM), ENG, 512, -1, 24},
        {"N=16384 Float64", call(16384, 16384), ENG, 512, -1, 32},
        {"N=16384 Float32", call(16384, 16384, ENTRY_RM, 4), ENG, 512, -1, 32},
        {"N=16384 NoPivot", call(16384, 16384, ENTRY_RM, 8, 0), LA, 512, 16, 0},
        {"N=16384 RFLU_ENGINE=0", noeng, LA, 512, 16, 0},
        {"N=16384 blocksize 256", call(16384, 16384, ENTRY_RM, 8, 1, 256), LA, 256, 32, 0},
        {"16000 x 15000", call(16000, 15000), ENG, 512, -1, 30},
        {"N=20480", call(20480, 20480), LA, 512, 24, 0},
        {"N=32768", call(32768, 32768), LA, 512, 48, 0},
        {"host N=8192", call(8192, 8192, ENTRY_HOST), ENG, 256, -1, 32},
        {"host N=16384 NoPivot", call(16384, 16384, ENTRY_HOST, 8, 0), LA, 512, 16, 0},
        {"profiling mode 1", prof, BLK, -1, -1, -1},
        {"304 CUs", cus304, BLK, -1, -1, -1},
    };
    for (const Row& r : rows) {
        const SchedPlan p = plan_schedule(r.in);
        CHECK(p.path == r.path, "%s: path %d, expected %d\n", r.name, p.path, r.path);
        CHECK(r.Wb < 0 || p.Wb == r.Wb, "%s: Wb %lld, expected %lld\n", r.name, (long long)p.Wb, (long long)r.Wb);
        CHECK(r.b_switch < 0 || p.b_switch == r.b_switch, "%s: b_switch %lld, expected %lld\n", r.name, (long long)p.b_switch, (long long)r.b_switch);
        CHECK(r.eng_end < 0 || p.eng_end == r.eng_end, "%s: eng_end %lld, expected %lld\n", r.name, (long long)p.eng_end, (long long)r.eng_end);
    }
    {
        const SchedPlan p = plan_schedule(call(12288, 12288, ENTRY_CM));
        CHECK(p.tail_overlap && p.tail_w0 == 512, "N=12288 column-major: tail overlap %d from column %lld\n", p.tail_overlap, (long long)p.tail_w0);
        const SchedPlan w = plan_schedule(call(20480, 20480));
        CHECK(w.W_wide == 1024 && w.wide_end == 4096, "N=20480: W_wide %lld wide_end %lld\n", (long long)w.W_wide, (long long)w.wide_end);
        const SchedPlan x = plan_schedule(call(32768, 32768));
        CHECK(x.W_wide == 2048 && x.wide_end == 16384, "N=32768: W_wide %lld wide_end %lld\n", (long long)x.W_wide, (long long)x.wide_end);
        const SchedPlan h = plan_schedule(call(8192, 8192, ENTRY_HOST));
        CHECK(h.host_engine && !h.host_early, "host N=8192: through the engine %d, early way back %d\n", h.host_engine, h.host_early);
        const SchedPlan hn = plan_schedule(call(16384, 16384, ENTRY_HOST, 8, 0));
        CHECK(!hn.host_engine && hn.host_early, "host N=16384 NoPivot: through the engine %d, early way back %d\n", hn.host_engine, hn.host_early);
        const SchedPlan e = plan_schedule(call(16384, 16384));
        CHECK(e.eng_wc == 512 && e.eng_ahead == 1 && e.eng_retire_leaf == (16384 - 2048) / NB && e.local_rows == 4096,
              "N=16384: engine Wc %d ahead %d retire leaf %lld local rows %lld\n", e.eng_wc, e.eng_ahead, (long long)e.eng_retire_leaf, (long long)e.local_rows);
        const SchedPlan f = plan_schedule(call(16384, 16384, ENTRY_RM, 4));
        CHECK(f.local_rows == 8192 && f.eng_retire_leaf == (16384 - 2048) / NB, "N=16384 Float32: local rows %lld retire leaf %lld\n",
              (long long)f.local_rows, (long long)f.eng_retire_leaf);
    }

    // ---- invariants over a grid ----
    long long cases = 0;
    const int64_t sizes[] = {1000, 1024, 4096, 8192, 8193, 11264, 11265, 12288, 15000, 16384, 16385, 20480, 24577, 32768, 65536};
    std::vector<SchedIn> settings;
    settings.push_back(SchedIn{});
    auto with = [&](auto fn) { SchedIn s; fn(s); settings.push_back(s); };
    with([](SchedIn& s) { s.tune.engine = 1; });
    with([](SchedIn& s) { s.tune.engine = 0; });
    with([](SchedIn& s) { s.tune.engine_replay = 1; });
    with([](SchedIn& s) { s.tune.schedule_events = 1; });
    with([](SchedIn& s) { s.tune.leafwise = 0; });
    with([](SchedIn& s) { s.tune.leafwise_rows = 4096; });
    with([](SchedIn& s) { s.tune.wide_narrow = 0; });
    with([](SchedIn& s) { s.tune.engine_rows = 8192; });
    with([](SchedIn& s) { s.tune.engine_wc = 128; s.tune.engine_ahead = 9; });
    with([](SchedIn& s) { s.tune.engine_retire = 0; s.tune.panel_local_rows = 2048; });
    with([](SchedIn& s) { s.tune.host_early_out = 0; s.tune.engine_host = 0; });
    with([](SchedIn& s) { s.tune.tail_overlap = 0; });
    with([](SchedIn& s) { s.num_cus = 304; });
    with([](SchedIn& s) { s.prof = true; });
    with([](SchedIn& s) { s.mask_failed = true; });
    with([](SchedIn& s) { s.progress = true; });
    with([](SchedIn& s) { s.tune.engine = 1; s.progress = true; });
    with([](SchedIn& s) { s.tune.engine = 1; s.aligned16 = false; });
    with([](SchedIn& s) { s.tune.engine = 1; s.roff = 64; });
    with([](SchedIn& s) { s.coop_launch = true; s.panel_local = 0; });
    for (const SchedIn& s0 : settings)
        for (int64_t m : sizes) for (int64_t n : sizes)
            for (size_t es : {(size_t)8, (size_t)4}) for (int pivot : {1, 0})
                for (int64_t bs : {(int64_t)0, (int64_t)-1, (int64_t)64, (int64_t)256, (int64_t)300, (int64_t)512, (int64_t)1024, std::min(m, n)})
                    for (int entry : {ENTRY_RM, ENTRY_CM, ENTRY_HOST}) {
                        SchedIn in = s0;
                        in.m = m; in.n = n; in.esize = es; in.pivot = pivot; in.blocksize = bs; in.entry = entry;
                        in.ld = (n + 15) / 16 * 16;
                        if (entry == ENTRY_HOST) { in.progress = false; in.roff = 0; in.aligned16 = true; }   // the host entry's own workspace, no hook yet
                        const SchedPlan p = plan_schedule(in);
                        ++cases;
                        const int64_t mn = std::min(m, n);
#define AT "m=%lld n=%lld esize=%zu pivot=%d blocksize=%lld entry=%d: ", (long long)m, (long long)n, es, pivot, (long long)bs, entry
                        if (p.host_engine) {
                            CHECK(p.path == RFLU_PATH_HIP_ENGINE && p.eng_end == p.nblk, AT);
                            // what getrf_rm decides under the host entry through the engine: the same plan, so its guard cannot fire
                            SchedIn e = in;
                            e.entry = ENTRY_HOST_ENGINE;
                            const SchedPlan q = plan_schedule(e);
                            CHECK(q.path == RFLU_PATH_HIP_ENGINE && q.eng_end == q.nblk && q.Wb == p.Wb, AT);
                        }
                        if (p.path == RFLU_PATH_HIP_ENGINE) {
                            CHECK(p.Wb % 128 == 0 && p.Wb <= 512 && m <= 16384 && p.eng_end > 0 && p.eng_end <= p.nblk, AT);
                            CHECK(p.eng_wc >= 128 && p.Wb % p.eng_wc == 0 && (n + p.eng_wc - 1) / p.eng_wc <= ENG_MAX_CB, AT);
                            CHECK(p.eng_ahead >= 1 && p.eng_ahead <= 4, AT);
                            CHECK(p.host_engine || entry == ENTRY_HOST || !in.progress, AT);   // (the host entry's hook is set only off the engine)
                            CHECK(p.eng_retire_leaf < 0 || (p.eng_retire_leaf > 0 && p.eng_retire_leaf < (m + NB - 1) / NB), AT);
                        } else {
                            CHECK(p.eng_end == 0 && p.eng_retire_leaf < 0, AT);
                        }
                        if (p.tail_overlap) CHECK(p.two_stream && p.tail_w0 > 0 && p.tail_w0 < mn, AT);
                        CHECK(p.two_stream == (p.path == RFLU_PATH_HIP_LOOKAHEAD || p.path == RFLU_PATH_HIP_ENGINE), AT);
                        CHECK(p.b_switch >= 0 && p.b_switch <= p.nblk, AT);
                        if (p.path == RFLU_PATH_HIP_LOOKAHEAD)
                            CHECK(p.Wb > 0 && p.Wb % NB == 0 && p.nblk == (mn + p.Wb - 1) / p.Wb && p.wide_end % (p.W_wide ? p.W_wide : 1) == 0 &&
                                  p.wide_end <= p.b_switch * p.Wb, AT);
                        CHECK(p.path != RFLU_PATH_HIP_RECURSIVE || bs < 0 || bs >= mn || (bs == 0 && mn < 1024), AT);
                    }
    printf("%lld cases, %d violations\n", cases, bad);
    return bad != 0;
}
