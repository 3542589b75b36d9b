// The pass history behind the two route choices of an EM fit that depend on what earlier passes on the same data handle did: the
// sparse or the dense statistics kernel (run_mstats), the screened or the dense E-step (launch_estep). HIP-free: the rules are plain
// functions of two rings of pass counts, held to a hand-written table by tests/cpp/pass_history_test.cpp without a GPU. The handle's
// owners of the buffers behind the rings are StatsHistory and ScreenState (internal.hpp).
#pragma once
#include <cstdint>

namespace mlhip_rt {

/// Largest number of nonzero responsibilities (sparse statistics kernel) / candidates (screened E-step) per sample up to which the
/// kernels whose cost grows with them are taken.
constexpr double kSparseMaxPairs = 16.0;
constexpr double kScreenMaxPairs = kSparseMaxPairs;

/// The last three passes of one kind with one K. A pass may leave a count in its slot of three words the CALLER holds and hands in
/// (on a handle: pinned memory an asynchronous copy on the stream writes). The one who reads a count does not wait for that copy: a
/// count is asked for two passes back at the nearest while a pass runs, and every loop has waited for pass t - 2 before it starts
/// pass t (mlhip_em_step ends in a synchronisation, mlhip_em_iterate reads iteration t - 2's pack first); the newer ones only behind
/// a synchronisation of the stream (mlhip_em_screen_counts). A pass that leaves no count leaves a STALE word in its slot: count()
/// is the only reader, and it does not return it.
class PassRing {
public:
    /// A pass with K begins: another K than the last pass's starts the history again.
    void begin(int K)
    {
        if (K == K_) return;
        K_ = K;
        passes_ = 0;
    }
    /// Where the pass that has begun leaves its count.
    int slot() const { return (int)(passes_ % 3); }
    /// The pass is over; whether it left a count.
    void finish(bool left_count)
    {
        left_[slot()] = left_count;
        ++passes_;
    }
    /// The count of the pass `back` = 1, 2, 3 before the one that runs (or would begin next); null: no such pass with this K, or it
    /// left no count. (While a pass runs, the slot of back = 3 is the one it writes.)
    const unsigned long long* count(const unsigned long long* slots, uint64_t back) const
    {
        if (back < 1 || back > 3 || back > passes_) return nullptr;
        const int s = (int)((passes_ - back) % 3);
        return left_[s] ? slots + s : nullptr;
    }
    int K() const { return K_; }
    uint64_t passes() const { return passes_; }

private:
    int K_ = 0;
    uint64_t passes_ = 0;            // finished, with K_
    bool left_[3] = {false, false, false};
};

/// Whether self-normalising statistics pass t of a handle -- `stats` has begun it, `nz` holds its counts of nonzero responsibilities --
/// runs the sparse kernel (em_mstats_sparse.hip) instead of the dense one. The sparse kernel's cost grows with the nonzero
/// responsibilities, the dense kernel's does not: sparse while pass t - 2 had at most kSparseMaxPairs nonzero pairs per sample; the
/// first two passes with a K are dense. The choice depends only on the handle's call history, so a loop of mlhip_em_step and
/// mlhip_em_iterate take the same kernels in the same order. `force`: the route's 1 / 0 for the sparse / the dense kernel (-1: by
/// history), honoured where the sparse kernel exists for the shape (`supported`).
inline bool sparse_stats_wanted(const PassRing& stats, const unsigned long long* nz, uint32_t n, int force, bool supported)
{
    if (!supported) return false;
    if (force >= 0) return force == 1;
    const unsigned long long* z = stats.count(nz, 2);
    return z && (double)*z <= kSparseMaxPairs * (double)n;
}

/// Whether tracked pass t of a fit -- an E-step pass of the screened kernel's domain; `tracked` has begun it with K, `candidates`
/// holds the candidate counts of the tracked passes that ran screened -- is asked to run screened (em_estep_screen.hip). The block must be
/// one the screened kernel may start from (`screenable`: EstepState). By call history: the sparse-statistics rule holds for
/// statistics pass t - 2 with this K, and where tracked pass t - 2 was itself screened it had at most kScreenMaxPairs candidates per
/// sample -- and only at the shapes where the screened pass was measured faster (`preferred`). `force`: the route's 1 / 0 / -1. The
/// bound constants have the last word: ScreenState::run.
inline bool screen_wanted(const PassRing& stats, const unsigned long long* nz, const PassRing& tracked, const unsigned long long* candidates,
                          int K, uint32_t n, int force, bool preferred, bool screenable)
{
    if (force == 0 || !screenable) return false;
    if (force == 1) return true;
    if (!preferred || stats.K() != K || tracked.passes() < 2) return false;
    const unsigned long long* z = stats.count(nz, 2);
    if (!z || (double)*z > kSparseMaxPairs * (double)n) return false;
    const unsigned long long* c = tracked.count(candidates, 2);   // (null: that pass ran dense)
    return !c || (double)*c <= kScreenMaxPairs * (double)n;
}

/// What mlhip_em_screen_counts reports as the candidates: those of the newest screened pass among the last three tracked ones, else 0.
inline unsigned long long newest_screened_candidates(const PassRing& tracked, const unsigned long long* candidates)
{
    for (uint64_t back = 1; back <= 3; ++back)
        if (const unsigned long long* c = tracked.count(candidates, back)) return *c;
    return 0;
}

}  // namespace mlhip_rt
