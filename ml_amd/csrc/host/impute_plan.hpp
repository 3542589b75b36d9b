// The host plan of mlhip_em_impute (mlhip.h): the rows of a block with NaNs grouped by their pattern of observed coordinates. Plain
// C++17, no HIP (tests/cpp/impute_plan_test.cpp builds it with g++ from this header, impute_plan.cpp and em_math.cpp alone).
//   mask      one bit per coordinate, bit c % 64 of word c / 64 set where coordinate c is OBSERVED (not a NaN, whatever its payload);
//   pattern   a distinct mask; the patterns stand in ascending order of their words compared from word 0 on;
//   order     the rows in a stable order in which the rows of one pattern are contiguous: ascending row index inside a pattern;
//   bounds    pattern p holds order[bounds[p] .. bounds[p + 1]);
//   tiles     a pattern's rows cut into runs of at most kImputeTileRows: what one wave of a lane = row kernel takes. A tile never
//             spans two patterns, so everything a tile reads of the model is wave-uniform;
//   classes   the tiles of the patterns with 1 <= dO <= d - 1 by the register tier's paddings (impute_pad(dO), impute_pad(dM)) --
//             condition_pad's for kConditionRegisters (device.hpp) --, ascending by (PO, PM), only where d <= kImputeKernelMaxDim.
// The complete rows (dO = d) and the rows of all NaN (dO = 0) are patterns like the others in order / bounds; `complete` and
// `all_missing` name them (-1: none), and they are in no class.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace mlhip {
namespace host {

constexpr int kImputeTileRows = 64;
constexpr int kImputeKernelMaxDim = 32;

/// 4 / 8 / 16 / 32 for 1 <= n <= 32, else -1: condition_pad(kConditionRegisters, n).
inline int impute_pad(int n) { return n < 1 ? -1 : n <= 4 ? 4 : n <= 8 ? 8 : n <= 16 ? 16 : n <= kImputeKernelMaxDim ? 32 : -1; }

struct ImputeTile {
    uint32_t pattern, first, rows;                               // rows order[first .. first + rows) of `pattern`
};
struct ImputeClass {
    int po, pm;
    std::vector<ImputeTile> tiles;                               // ascending by `first`
};
struct ImputePlan {
    uint32_t d = 0, words = 0, n = 0;
    std::vector<uint64_t> masks;                                 // patterns() x words
    std::vector<uint32_t> n_observed;                            // patterns()
    std::vector<uint32_t> order;                                 // n
    std::vector<uint32_t> bounds;                                // patterns() + 1
    int64_t complete = -1, all_missing = -1;
    std::vector<ImputeClass> classes;
    uint32_t patterns() const { return (uint32_t)n_observed.size(); }
    const uint64_t* mask(uint32_t p) const { return masks.data() + (size_t)p * words; }
    bool observed(uint32_t p, uint32_t c) const { return (mask(p)[c / 64] >> (c % 64)) & 1u; }
};

/// The plan of n rows of d doubles, `ld` >= d doubles apart. The masks are built by the calling thread's team (host/team.hpp, sized
/// as the per-component factorizations' team: host_threads()), the sort runs on the calling thread. The result does not depend on
/// the number of threads.
ImputePlan impute_plan(const double* x, uint32_t n, uint32_t d, int64_t ld);

/// The tile lists of the patterns [p0, p1) cut to the rows order[pos0 .. pos1), by class as ImputePlan::classes (which is
/// impute_tiles(plan, 0, patterns(), 0, n)): what one (pattern chunk, row chunk) of the kernel route launches. Empty above
/// d = kImputeKernelMaxDim.
std::vector<ImputeClass> impute_tiles(const ImputePlan& plan, uint32_t p0, uint32_t p1, uint32_t pos0, uint32_t pos1);

}  // namespace host
}  // namespace mlhip
