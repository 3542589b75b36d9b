// The pass history of an EM fit (ml_amd/csrc/runtime/pass_history.hpp: PassRing, sparse_stats_wanted, screen_wanted,
// newest_screened_candidates) held to tables written out by hand from the rules:
//   sparse statistics, pass t:  false where the kernel does not exist, else the forced value, else false for the first two passes with
//                               a K, else nz(t - 2) <= 16 n;
//   screened E-step, pass t:    false if forced off or the block is not screenable, true if forced on, else true iff the shape is
//                               preferred, the statistics ring counts for this K and has >= 2 passes, the tracked ring has >= 2 passes,
//                               nz(t - 2) <= 16 n, and tracked pass t - 2 ran dense or had <= 16 n candidates;
//   report:                     the candidates of the newest screened pass among the last three tracked passes, else 0.
// n = 1000, so the bound is 16000. The slots are plain arrays here, written the way the handle's asynchronous copies write the pinned
// ones: a pass that leaves no count leaves its slot as it was. No GPU, no library.
#include <cstdint>
#include <cstdio>

#include "runtime/pass_history.hpp"

using namespace mlhip_rt;
using ull = unsigned long long;

static int g_checks = 0, g_failed = 0;
#define CHECK(what, got, want)                                                                                             \
    do {                                                                                                                   \
        ++g_checks;                                                                                                        \
        const ull got_ = (ull)(got), want_ = (ull)(want);                                                                  \
        if (got_ != want_) {                                                                                               \
            ++g_failed;                                                                                                    \
            std::printf("FAILED %s:%d %s, t = %d: got %llu, expected %llu\n", __FILE__, __LINE__, what, t, got_, want_);   \
        }                                                                                                                  \
    } while (0)

constexpr uint32_t N = 1000;
constexpr ull kDense = ~0ull;   // (a row's E-step runs dense whatever was wanted: sent back, or nothing to say)

/// One handle's two histories and the words behind them.
struct Handle {
    PassRing stats, tracked;
    ull nz[3], cand[3];
    explicit Handle(ull fill) : nz{fill, fill, fill}, cand{fill, fill, fill} {}

    /// A tracked E-step pass as launch_estep runs it: the decision; the pass then runs screened with `candidates` where that was wanted
    /// and `candidates` is not kDense.
    bool estep(int K, ull candidates, int force = -1, bool preferred = true, bool screenable = true)
    {
        tracked.begin(K);
        const bool wanted = screen_wanted(stats, nz, tracked, cand, K, N, force, preferred, screenable);
        const bool screened = wanted && candidates != kDense;
        if (screened) cand[tracked.slot()] = candidates;
        tracked.finish(screened);
        return wanted;
    }
    /// A self-normalising statistics pass as run_mstats runs it: the decision; the pass leaves `count`.
    bool mstats(int K, ull count, int force = -1, bool supported = true)
    {
        stats.begin(K);
        const bool sparse = sparse_stats_wanted(stats, nz, N, force, supported);
        nz[stats.slot()] = count;
        stats.finish(true);
        return sparse;
    }
    ull report() const { return newest_screened_candidates(tracked, cand); }
};

/// One iteration of a fit: the E-step pass, the report behind it, the statistics pass.
struct Row {
    ull candidates;     // of the E-step where it runs screened; kDense: it runs dense
    ull nz;             // the statistics pass leaves
    bool screen, sparse;
    ull report;
};

static void run_rows(Handle& h, int K, const Row* rows, int n_rows, const char* name)
{
    for (int t = 0; t < n_rows; ++t) {
        const Row& r = rows[t];
        CHECK(name, h.estep(K, r.candidates), r.screen);
        CHECK(name, h.report(), r.report);
        CHECK(name, h.mstats(K, r.nz), r.sparse);
    }
}

int main()
{
    int t = -1;

    // ---- one fit with K = 8 on a handle whose words all hold 1 (a count that would allow everything, were it read)
    Handle h(1);
    const Row fit[] = {
        // candidates  nz     screen sparse report
        {1,            16000, false, false, 0},            // 0: first pass with this K: dense, not screened, whatever the slots hold
        {1,            16001, false, false, 0},            // 1: second pass: the same
        {16000,        5,     true,  true,  16000},        // 2: nz(0) = 16000 allows both; tracked pass 0 ran dense
        {1,            6,     false, false, 16000},        // 3: nz(1) = 16001 forbids both; the report is still pass 2's
        {16001,        7,     true,  true,  16001},        // 4: nz(2) = 5; tracked pass 2 had 16000 candidates: allowed
        {1000000000,   8,     true,  true,  1000000000},   // 5: nz(3) = 6; tracked pass 3 ran dense
        {1,            9,     false, true,  1000000000},   // 6: tracked pass 4 had 16001 candidates: forbidden; the newest screened pass is 5
        {1,            10,    false, true,  1000000000},   // 7: tracked pass 5 had 10^9 candidates: forbidden; 5 is still among the last three
        {kDense,       11,    true,  true,  0},            // 8: wanted (pass 6 ran dense) but sent back: dense, its slot keeps pass 5's 10^9 -- and the report, with 8, 7, 6 all dense, is 0
        {123,          12,    true,  true,  123},          // 9: tracked pass 7 ran dense
        {124,          13,    true,  true,  124},          // 10: tracked pass 8 ran dense: the 10^9 in its slot is stale and must be ignored
        {kDense,       14,    true,  true,  124},          // 11: tracked pass 9 had 123; runs dense; the newest screened pass is 10
        {kDense,       15,    true,  true,  124},          // 12: dense again; 10 is the oldest of the last three
        {kDense,       16,    true,  true,  0},            // 13: 13, 12, 11 all dense: 0, though every slot holds a count
    };
    run_rows(h, 8, fit, (int)(sizeof(fit) / sizeof(fit[0])), "fit with K = 8");

    // ---- the same handle goes on with K = 5: two dense, unscreened passes again, the old words (all small) are not read, and the
    // report looks at no more passes than there are with this K
    const Row other_k[] = {
        {1,            20000, false, false, 0},            // 0
        {1,            2,     false, false, 0},            // 1
        {1,            3,     false, false, 0},            // 2: nz(0) = 20000 forbids both
        {77,           4,     true,  true,  77},           // 3: nz(1) = 2; tracked pass 1 ran dense
    };
    run_rows(h, 5, other_k, (int)(sizeof(other_k) / sizeof(other_k[0])), "the fit goes on with K = 5");

    // ---- wrap-around: ten statistics passes with distinct counts, below the bound where `low`; the decision at t is that of pass
    // t - 2's count, which at some t differs from what the count of pass t - 1 or t - 3 would give
    {
        const bool low[10] = {true, true, false, true, false, false, false, true, true, false};
        const bool sparse[10] = {false, false, true, true, false, true, false, false, false, true};   // = low[t - 2] from t = 2 on
        Handle w(0);
        for (t = 0; t < 10; ++t) {
            // (the E-step of iteration t consults the same count: screened from t = 2 on iff low[t - 2]; it runs dense every time)
            CHECK("wrap-around, E-step", w.estep(8, kDense), sparse[t]);
            CHECK("wrap-around, statistics", w.mstats(8, low[t] ? 16000 - (ull)t : 16001 + (ull)t), sparse[t]);
        }
    }

    // ---- a screen decision fails while the statistics ring counts for another K
    {
        Handle k(0);
        t = 0;
        for (int i = 0; i < 3; ++i) k.mstats(8, 1);                 // the statistics ring: three passes with K = 8, all small
        for (int i = 0; i < 2; ++i) k.estep(5, kDense);             // the tracked ring: two dense passes with K = 5
        CHECK("statistics ring of another K", k.estep(5, kDense), false);
        for (int i = 0; i < 2; ++i) k.mstats(5, 1);                 // now it counts for K = 5 and has two passes
        CHECK("statistics ring of this K", k.estep(5, kDense), true);
        // the tracked ring restarts with K = 8 (the statistics ring counts for 5): the report sees no pass, then only the new one
        CHECK("forced on, first tracked pass with K = 8", k.estep(8, 4242, 1), true);
        CHECK("report after a K change", k.report(), 4242);
        CHECK("by history, second tracked pass with K = 8", k.estep(8, 1), false);
        CHECK("report, one screened and one dense pass", k.report(), 4242);
    }

    // ---- forced routes
    {
        Handle f(1);
        t = 0;
        for (int i = 0; i < 3; ++i) { f.estep(8, kDense); f.mstats(8, 1); }    // a history that allows everything
        CHECK("by history", f.estep(8, kDense), true);
        CHECK("by history, shape not preferred", f.estep(8, kDense, -1, false), false);
        CHECK("by history, block not screenable", f.estep(8, kDense, -1, true, false), false);
        CHECK("screen forced off", f.estep(8, kDense, 0), false);
        CHECK("screen forced on, block not screenable", f.estep(8, kDense, 1, true, false), false);
        CHECK("sparse by history", f.mstats(8, 1), true);
        CHECK("sparse forced off", f.mstats(8, 1, 0), false);
        CHECK("no sparse kernel, by history", f.mstats(8, 1, -1, false), false);
        CHECK("no sparse kernel, forced on", f.mstats(8, 1, 1, false), false);
        CHECK("no sparse kernel, forced off", f.mstats(8, 1, 0, false), false);

        Handle e(1000000000);                                                  // no history, words that would forbid everything
        CHECK("screen forced on: no history, not preferred", e.estep(8, kDense, 1, false), true);
        CHECK("screen forced on, block not screenable", e.estep(8, kDense, 1, false, false), false);
        CHECK("screen forced off", e.estep(8, kDense, 0), false);
        CHECK("sparse forced on: no history", e.mstats(8, 1000000000, 1), true);
        CHECK("sparse forced off", e.mstats(8, 1000000000, 0), false);
        CHECK("sparse forced on, no sparse kernel", e.mstats(8, 1000000000, 1, false), false);
    }

    // ---- the ring itself: which passes it answers for
    {
        PassRing r;
        const ull slots[3] = {10, 11, 12};
        t = 0;
        r.begin(4);
        CHECK("no pass yet", r.count(slots, 1) != nullptr, 0);
        CHECK("slot of pass 0", r.slot(), 0);
        r.finish(true);
        r.begin(4);
        CHECK("slot of pass 1", r.slot(), 1);
        r.finish(false);
        r.begin(4);
        CHECK("slot of pass 2", r.slot(), 2);
        CHECK("pass 1 left no count", r.count(slots, 1) != nullptr, 0);
        CHECK("pass 0 left one", r.count(slots, 2) == slots + 0, 1);
        CHECK("no pass 3 back", r.count(slots, 3) != nullptr, 0);
        CHECK("back = 0 is the running pass: no count", r.count(slots, 0) != nullptr, 0);
        r.finish(true);
        r.begin(4);
        CHECK("slot of pass 3", r.slot(), 0);
        CHECK("pass 2", r.count(slots, 1) == slots + 2, 1);
        CHECK("pass 0, three back", r.count(slots, 3) == slots + 0, 1);
        CHECK("four back", r.count(slots, 4) != nullptr, 0);
        CHECK("passes", r.passes(), 3);
        r.begin(6);
        CHECK("another K: passes", r.passes(), 0);
        CHECK("another K: K", r.K(), 6);
        CHECK("another K: no pass", r.count(slots, 1) != nullptr, 0);
    }

    if (g_failed) {
        std::printf("pass_history_test: %d of %d checks FAILED\n", g_failed, g_checks);
        return 1;
    }
    std::printf("pass_history_test: ok (%d checks)\n", g_checks);
    return 0;
}
