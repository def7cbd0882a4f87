// Host-side check of the persistent update engine's operation lists (csrc/engine.hpp -- the functions the host builds the initial state with and
// the device walks): over a grid of geometries, every column receives every earlier leaf exactly once and in order (the Schur updates of
// /root/reference/src/lu.jl:233-240, :265-284 in the engine's decomposition; the leaf right in front of a column reaches it on the critical-path
// stream), the leaf counts an operation waits for are sufficient and monotone, an operation's columns lie inside its column block, a leaf's
// operation index is where eng_leaf_op_index says, and a stage with columns has units.  The state the engine starts from (eng_initial_state,
// Float64 and Float32) claims, per column block, the first sequence that has units -- found here by a scan from the END of the list over
// unit counts taken from the operation's shape -- or ENG_SEQ_DONE, the same for the deferred interchanges, and counts the open claim
// words in `remaining`.  Compiled and run by tests/test_engine_geometry.py (no GPU).
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "engine.hpp"
using namespace rflu;

// units of sequence sq (2 * op + stage) of column block cb, from the operation's shape: 32-column strips, then 128 x 128 tiles of the rows below
static int units_by_shape(const EngGeo& g, int cb, int sq)
{
    const EngOp o = eng_op(g, cb, sq >> 1);
    if (o.nc <= 0) return 0;
    if ((sq & 1) == 0) return (o.nc + 31) / 32;
    const int rows = g.m - (o.j0 + o.jb);
    return rows <= 0 ? 0 : ((rows + 127) / 128) * ((o.nc + 127) / 128);
}

// violations of the initial state for element type T
template <typename T>
static int check_initial_state(const EngGeo& g, EngState* img, const char* tname)
{
    int bad = 0;
    const unsigned long long DONE = (unsigned long long)ENG_SEQ_DONE << 32;
    eng_initial_state<T>(g, img);
    unsigned long long open = 0;
    for (int cb = 0; cb < g.ncb; ++cb) {
        const EngCB& c = img->cb[cb];
        const int end = 2 * eng_nops(g, cb);
        int first = end;   // first sequence with units, found from the back
        for (int sq = end - 1; sq >= 0; --sq)
            if (units_by_shape(g, cb, sq) > 0) first = sq;
        const unsigned long long want_claim = first < end ? (unsigned long long)first << 32 : DONE;
        if (c.claim != want_claim || c.prog != 2ull * (unsigned long long)(first >> 1)) {
            if (bad++ < 10) printf("initial claim %s W=%d Wc=%d m=%d n=%d nbp=%d ahead=%d cb=%d: claim %llx prog %llu, first sequence with units %d of %d\n", tname, g.W, g.Wc, g.m, g.n,
                                   g.nbp, g.ahead, cb, c.claim, c.prog, first, end);
        }
        const int nleft = eng_nleft(g, cb);
        int lfirst = nleft;
        for (int lk = nleft - 1; lk >= 0; --lk)
            if (eng_left_units<T>(g, cb, lk) > 0) lfirst = lk;
        const unsigned long long want_lclaim = lfirst < nleft ? (unsigned long long)lfirst << 32 : DONE;
        if (c.lclaim != want_lclaim || c.lprog != (unsigned long long)lfirst) {
            if (bad++ < 10) printf("initial left claim %s W=%d Wc=%d m=%d n=%d nbp=%d ahead=%d cb=%d: lclaim %llx lprog %llu, first left op with units %d of %d\n", tname, g.W, g.Wc, g.m,
                                   g.n, g.nbp, g.ahead, cb, c.lclaim, c.lprog, lfirst, nleft);
        }
        open += (c.claim != DONE) + (c.lclaim != DONE);
    }
    if (img->remaining != open) {
        if (bad++ < 10) printf("initial remaining %s W=%d Wc=%d m=%d n=%d nbp=%d ahead=%d: %llu vs %llu open claim words\n", tname, g.W, g.Wc, g.m, g.n, g.nbp, g.ahead, img->remaining, open);
    }
    return bad;
}

int main(int argc, char** argv)
{
    int bad = 0, cases = 0;
    std::vector<EngState> image(1);
    const int Ws[] = {128, 256, 512};
    for (int W : Ws)
        for (int Wc : {128, 256, 512}) {
            if (Wc > W || W % Wc) continue;
            for (int m : {1024, 2048, 2112, 5000, 6144}) for (int n : {1024, 2048, 2112, 5000, 6144}) {
                if (m < n && m % W) continue;   // (engine_usable)
                EngGeo g{};
                g.m = m; g.n = n; g.mn = m < n ? m : n; g.W = W; g.Wc = Wc; g.pivot = 1;
                const int nblk = (g.mn + W - 1) / W;
                g.ncb = (n + Wc - 1) / Wc;
                if (g.ncb > ENG_MAX_CB) continue;
                for (int ahead : {1, 2, 3})
                for (int nbp : {nblk, nblk > 2 ? nblk / 2 : nblk}) {
                    g.nbp = nbp;
                    g.ahead = ahead;   // leaf windows over the own block column and `ahead` block columns right of it (engine.hpp)
                    ++cases;
                    bad += check_initial_state<double>(g, image.data(), "f64");
                    bad += check_initial_state<float>(g, image.data(), "f32");
                    const int served_leaves = (std::min(nbp * W, g.mn) + NB - 1) / NB;
                    // the per-block-column counts the interchange ordering rests on (engine.hpp: "order between the interchanges ..."): who has
                    // BIG(b), and where the LEAF ops of block column b end in the lists of the column blocks in front of which it lies
                    for (int b = 0; b < nbp; ++b) {
                        int users = 0;
                        for (int cb = 0; cb < g.ncb; ++cb) users += eng_nbig(g, cb) > b;
                        if (users != eng_big_users(g, b)) { if (bad++ < 10) printf("big users W=%d Wc=%d m=%d n=%d ahead=%d b=%d: %d vs %d\n", W, Wc, m, n, ahead, b, users, eng_big_users(g, b)); }
                        for (int cb = 0; cb < g.ncb; ++cb) {
                            const int pb = eng_pb(g, cb);
                            int last = -1;   // last op of cb that applies a leaf of block column b leaf by leaf
                            for (int k = 0; k < eng_nops(g, cb); ++k) {
                                const EngOp o = eng_op(g, cb, k);
                                if (o.type == ENG_OP_LEAF && o.j0 / W == b) last = k;
                            }
                            if (pb > b && pb <= b + ahead) {
                                if (eng_ops_through_block(g, cb, b) != last + 1 && !(last < 0 && eng_leaves_of_block(g, b) == 0)) { if (bad++ < 10) printf("ops through block W=%d Wc=%d m=%d n=%d ahead=%d b=%d cb=%d: %d vs %d\n", W, Wc, m, n, ahead, b, cb, eng_ops_through_block(g, cb, b), last + 1); }
                            } else if (pb != b && last >= 0) { if (bad++ < 10) printf("leaf op outside the window W=%d Wc=%d m=%d n=%d ahead=%d b=%d cb=%d\n", W, Wc, m, n, ahead, b, cb); }
                        }
                    }
                    for (int cb = 0; cb < g.ncb; ++cb) {
                        const int c_first = cb * Wc, c_last = std::min(n, c_first + Wc);
                        std::vector<std::vector<int>> got(c_last - c_first);
                        int prev_need = 0, prev_j0 = -1;
                        for (int k = 0; k < eng_nops(g, cb); ++k) {
                            const EngOp o = eng_op(g, cb, k);
                            if (o.need < prev_need) { if (bad++ < 10) printf("need not monotone W=%d Wc=%d m=%d n=%d cb=%d k=%d\n", W, Wc, m, n, cb, k); }
                            prev_need = o.need;
                            if (o.j0 <= prev_j0) { if (bad++ < 10) printf("pivot blocks out of order W=%d Wc=%d m=%d n=%d cb=%d k=%d\n", W, Wc, m, n, cb, k); }
                            prev_j0 = o.j0;
                            if (o.need * NB < o.j0 + o.jb && o.need < served_leaves) { if (bad++ < 10) printf("need too small W=%d Wc=%d m=%d n=%d cb=%d k=%d need=%d j0=%d jb=%d\n", W, Wc, m, n, cb, k, o.need, o.j0, o.jb); }
                            if (o.type == ENG_OP_LEAF && eng_leaf_op_index(g, cb, o.j0 / NB) != k) { if (bad++ < 10) printf("leaf op index W=%d Wc=%d m=%d n=%d cb=%d k=%d\n", W, Wc, m, n, cb, k); }
                            if (o.nc > 0 && eng_units_of(o, 0, g.m) <= 0) { if (bad++ < 10) printf("no stage-0 units W=%d Wc=%d m=%d n=%d cb=%d k=%d\n", W, Wc, m, n, cb, k); }
                            if (o.nc > 0 && g.m > o.j0 + o.jb && eng_units_of(o, 1, g.m) <= 0) { if (bad++ < 10) printf("no stage-1 units W=%d Wc=%d m=%d n=%d cb=%d k=%d\n", W, Wc, m, n, cb, k); }
                            if (o.nc <= 0) continue;
                            if (o.c_lo < c_first || o.c_lo + o.nc > c_last) { if (bad++ < 10) printf("columns outside the block W=%d Wc=%d m=%d n=%d cb=%d k=%d\n", W, Wc, m, n, cb, k); continue; }
                            for (int c = o.c_lo; c < o.c_lo + o.nc; ++c)
                                for (int j = o.j0; j < o.j0 + o.jb; j += NB) got[c - c_first].push_back(j / NB);
                        }
                        for (int c = c_first; c < c_last; ++c) {
                            // column c (leaf lc) owes the engine the leaves 0 .. min(lc - 1, served) - 1: leaf lc - 1 reaches the 64 columns behind
                            // it on the critical-path stream (the lookahead strip)
                            const int lc = c / NB;
                            int want = std::min(lc - 1, served_leaves);
                            if (want < 0) want = 0;
                            const std::vector<int>& v = got[c - c_first];
                            bool ok = (int)v.size() == want;
                            for (int i = 0; ok && i < want; ++i) ok = v[i] == i;
                            if (!ok && bad++ < 10) {
                                printf("W=%d Wc=%d m=%d n=%d nbp=%d column %d (leaf %d): wants leaves 0..%d, got %zu:", W, Wc, m, n, nbp, c, lc, want - 1, v.size());
                                for (size_t i = 0; i < v.size() && i < 12; ++i) printf(" %d", v[i]);
                                printf("\n");
                            }
                        }
                    }
                }
            }
        }
    printf("%d geometries, %d violations\n", cases, bad);
    return bad ? 1 : 0;
}
