// The host plan of mlhip_em_impute: masks, a stable sort by pattern, the group bounds and the per-class tile lists (impute_plan.hpp).
#include "host/impute_plan.hpp"

#include <algorithm>
#include <functional>
#include <numeric>
#include <utility>

#include "host/em_math.hpp"
#include "host/team.hpp"

namespace mlhip {
namespace host {

namespace {
constexpr uint32_t kMaskBlockRows = 4096;                        // rows one team member masks at a time
}

ImputePlan impute_plan(const double* x, uint32_t n, uint32_t d, int64_t ld)
{
    ImputePlan plan;
    plan.d = d; plan.n = n; plan.words = (d + 63) / 64;
    plan.bounds.push_back(0);
    if (!n || !d) return plan;
    const uint32_t words = plan.words;

    // every row's mask: a NaN is the one value that differs from itself, whatever its sign and payload
    std::vector<uint64_t> row_mask((size_t)n * words, 0);
    const int blocks = (int)((n + kMaskBlockRows - 1) / kMaskBlockRows);
    const std::function<void(int)> mask_block = [&](int b) {
        const uint32_t lo = (uint32_t)b * kMaskBlockRows, hi = std::min<uint64_t>(n, (uint64_t)lo + kMaskBlockRows);
        for (uint32_t i = lo; i < hi; ++i) {
            const double* row = x + (int64_t)i * ld;
            uint64_t* m = row_mask.data() + (size_t)i * words;
            for (uint32_t c = 0; c < d; ++c)
                if (row[c] == row[c]) m[c / 64] |= uint64_t(1) << (c % 64);
        }
    };
    Team::mine().for_each(blocks, blocks >= 4 ? host_threads() : 1, mask_block);

    // stable order by mask: the row index breaks ties, so equal masks keep ascending rows
    plan.order.resize(n);
    if (words == 1) {
        std::vector<std::pair<uint64_t, uint32_t>> keyed(n);
        for (uint32_t i = 0; i < n; ++i) keyed[i] = {row_mask[i], i};
        std::sort(keyed.begin(), keyed.end());
        for (uint32_t i = 0; i < n; ++i) plan.order[i] = keyed[i].second;
    } else {
        std::iota(plan.order.begin(), plan.order.end(), 0u);
        std::sort(plan.order.begin(), plan.order.end(), [&](uint32_t a, uint32_t b) {
            const uint64_t *ma = row_mask.data() + (size_t)a * words, *mb = row_mask.data() + (size_t)b * words;
            for (uint32_t w = 0; w < words; ++w)
                if (ma[w] != mb[w]) return ma[w] < mb[w];
            return a < b;
        });
    }

    // the groups
    for (uint32_t pos = 0; pos < n; ++pos) {
        const uint64_t* m = row_mask.data() + (size_t)plan.order[pos] * words;
        if (pos && std::equal(m, m + words, row_mask.data() + (size_t)plan.order[pos - 1] * words)) continue;
        if (pos) plan.bounds.push_back(pos);
        plan.masks.insert(plan.masks.end(), m, m + words);
        uint32_t dO = 0;
        for (uint32_t w = 0; w < words; ++w) dO += (uint32_t)__builtin_popcountll(m[w]);
        const uint32_t p = plan.patterns();
        plan.n_observed.push_back(dO);
        if (dO == d) plan.complete = p;
        if (dO == 0) plan.all_missing = p;
    }
    plan.bounds.push_back(n);

    plan.classes = impute_tiles(plan, 0, plan.patterns(), 0, n);
    return plan;
}

std::vector<ImputeClass> impute_tiles(const ImputePlan& plan, uint32_t p0, uint32_t p1, uint32_t pos0, uint32_t pos1)
{
    std::vector<ImputeClass> classes;
    const uint32_t d = plan.d;
    if (d > (uint32_t)kImputeKernelMaxDim) return classes;
    for (int po = 4; po <= kImputeKernelMaxDim; po *= 2)
        for (int pm = 4; pm <= kImputeKernelMaxDim; pm *= 2) {
            ImputeClass cls{po, pm, {}};
            for (uint32_t p = p0; p < p1; ++p) {
                const uint32_t dO = plan.n_observed[p];
                if (dO == 0 || dO == d || impute_pad((int)dO) != po || impute_pad((int)(d - dO)) != pm) continue;
                const uint32_t lo = std::max(plan.bounds[p], pos0), hi = std::min(plan.bounds[p + 1], pos1);
                for (uint32_t first = lo; first < hi; first += kImputeTileRows)
                    cls.tiles.push_back({p, first, std::min<uint32_t>(kImputeTileRows, hi - first)});
            }
            if (!cls.tiles.empty()) classes.push_back(std::move(cls));
        }
    return classes;
}

}  // namespace host
}  // namespace mlhip
