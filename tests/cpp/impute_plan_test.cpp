// The host plan of mlhip_em_impute alone (ml_amd/csrc/host/impute_plan.cpp): plain C++, no HIP, no libmlhip.so. For N = 0, 1, 65, 1000
// and d = 1, 3, 32, 33, 70 and four kinds of blocks -- one pattern; every row its own pattern (as far as d allows); complete and
// all-NaN rows mixed in; NaNs of different signs and payloads -- it checks that
//   the order is a permutation of the rows; equal masks are contiguous and every group's mask is the mask of each of its rows;
//   the order inside a group is ascending; the groups stand in ascending order of their masks; n_observed counts the mask's bits;
//   complete / all_missing name the right groups;
//   every tile holds rows of one pattern, at most 64, inside that pattern's group, the tiles of a pattern cover its rows exactly once,
//   and the classes are the paddings 4 / 8 / 16 / 32 of (dO, dM) -- condition_pad's for the register tier --, none above d = 32;
//   impute_tiles on a sub-range of patterns and rows covers exactly the rows of that range.
// One block of 20 000 rows has the calling thread's team build the masks. Built and run by tests/test_cpp_impute_plan.py, plain and
// with -fsanitize=address,undefined.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "host/impute_plan.hpp"

using namespace mlhip::host;

namespace {

int failures = 0;
#define CHECK(cond)                                                                       \
    do {                                                                                  \
        if (!(cond)) {                                                                    \
            if (++failures <= 20) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                                                 \
    } while (0)

double nan_with(uint64_t payload, bool negative)
{
    uint64_t bits = 0x7ff0000000000000ull | (payload & 0x000fffffffffffffull) | (negative ? 0x8000000000000000ull : 0);
    if (!(bits & 0x000fffffffffffffull)) bits |= 1;              // (a payload of zero would be an infinity)
    double v;
    std::memcpy(&v, &bits, sizeof v);
    return v;
}

int pad_of(int n) { return n <= 4 ? 4 : n <= 8 ? 8 : n <= 16 ? 16 : 32; }   // condition_pad(kConditionRegisters, n), 1 <= n <= 32

std::vector<uint64_t> mask_of(const double* row, uint32_t d)
{
    std::vector<uint64_t> m((d + 63) / 64, 0);
    for (uint32_t c = 0; c < d; ++c)
        if (!std::isnan(row[c])) m[c / 64] |= uint64_t(1) << (c % 64);
    return m;
}

void check_tiles(const ImputePlan& plan, const std::vector<ImputeClass>& classes, uint32_t p0, uint32_t p1, uint32_t pos0, uint32_t pos1)
{
    const uint32_t d = plan.d;
    std::vector<int> covered(plan.n, 0);
    if (d > 32) CHECK(classes.empty());
    for (size_t c = 0; c < classes.size(); ++c) {
        const ImputeClass& cls = classes[c];
        if (c) CHECK(classes[c - 1].po < cls.po || (classes[c - 1].po == cls.po && classes[c - 1].pm < cls.pm));
        CHECK(!cls.tiles.empty());
        for (const ImputeTile& t : cls.tiles) {
            CHECK(t.pattern >= p0 && t.pattern < p1);
            const uint32_t dO = plan.n_observed[t.pattern];
            CHECK(dO >= 1 && dO < d);
            CHECK(pad_of((int)dO) == cls.po && pad_of((int)(d - dO)) == cls.pm);
            CHECK(impute_pad((int)dO) == cls.po && impute_pad((int)(d - dO)) == cls.pm);
            CHECK(t.rows >= 1 && t.rows <= 64);
            CHECK(t.first >= plan.bounds[t.pattern] && t.first + t.rows <= plan.bounds[t.pattern + 1]);
            CHECK(t.first >= pos0 && t.first + t.rows <= pos1);
            for (uint32_t i = 0; i < t.rows; ++i) ++covered[t.first + i];
        }
    }
    for (uint32_t p = 0; p < plan.patterns(); ++p) {
        const uint32_t dO = plan.n_observed[p];
        const bool tiled = d <= 32 && dO >= 1 && dO < d && p >= p0 && p < p1;
        for (uint32_t pos = plan.bounds[p]; pos < plan.bounds[p + 1]; ++pos) CHECK(covered[pos] == (tiled && pos >= pos0 && pos < pos1 ? 1 : 0));
    }
}

void check_plan(const std::vector<double>& x, uint32_t n, uint32_t d)
{
    const ImputePlan plan = impute_plan(x.data(), n, d, d);
    CHECK(plan.n == n && plan.d == d && plan.words == (d + 63) / 64);
    CHECK(plan.order.size() == n && plan.bounds.size() == (size_t)plan.patterns() + 1);
    CHECK(plan.bounds.front() == 0 && plan.bounds.back() == n);
    CHECK(plan.masks.size() == (size_t)plan.patterns() * plan.words);
    std::vector<int> seen(n, 0);
    for (uint32_t r : plan.order) {
        CHECK(r < n);
        if (r < n) ++seen[r];
    }
    for (uint32_t i = 0; i < n; ++i) CHECK(seen[i] == 1);
    bool has_complete = false, has_empty = false;
    for (uint32_t p = 0; p < plan.patterns(); ++p) {
        CHECK(plan.bounds[p] < plan.bounds[p + 1]);
        const std::vector<uint64_t> mine(plan.mask(p), plan.mask(p) + plan.words);
        if (p) CHECK(std::vector<uint64_t>(plan.mask(p - 1), plan.mask(p - 1) + plan.words) < mine);   // ascending, so distinct
        uint32_t bits = 0;
        for (uint32_t c = 0; c < d; ++c) bits += plan.observed(p, c) ? 1 : 0;
        CHECK(bits == plan.n_observed[p]);
        for (uint32_t pos = plan.bounds[p]; pos < plan.bounds[p + 1]; ++pos) {
            CHECK(mask_of(x.data() + (size_t)plan.order[pos] * d, d) == mine);
            if (pos > plan.bounds[p]) CHECK(plan.order[pos - 1] < plan.order[pos]);
        }
        if (bits == d) { has_complete = true; CHECK(plan.complete == (int64_t)p); }
        if (bits == 0) { has_empty = true; CHECK(plan.all_missing == (int64_t)p); }
    }
    if (!has_complete) CHECK(plan.complete == -1);
    if (!has_empty) CHECK(plan.all_missing == -1);
    check_tiles(plan, plan.classes, 0, plan.patterns(), 0, n);
    if (plan.patterns() >= 3) {
        const uint32_t p0 = 1, p1 = plan.patterns() - 1, lo = plan.bounds[p0], hi = plan.bounds[p1];
        const uint32_t pos0 = lo + (hi - lo) / 3, pos1 = hi - (hi - lo) / 4;
        check_tiles(plan, impute_tiles(plan, p0, p1, pos0, pos1), p0, p1, pos0, pos1);
    }
}

}  // namespace

int main()
{
    const uint32_t rows[] = {0, 1, 65, 1000}, dims[] = {1, 3, 32, 33, 70};
    std::mt19937_64 rng(12345);
    std::normal_distribution<double> normal;
    int blocks = 0;
    for (uint32_t n : rows)
        for (uint32_t d : dims)
            for (int kind = 0; kind < 4; ++kind) {
                std::vector<double> x((size_t)n * d);
                for (double& v : x) v = normal(rng);
                for (uint32_t i = 0; i < n; ++i) {
                    double* row = x.data() + (size_t)i * d;
                    if (kind == 0) {                             // one pattern: the odd coordinates missing (d = 1: none)
                        for (uint32_t c = 1; c < d; c += 2) row[c] = std::numeric_limits<double>::quiet_NaN();
                    } else if (kind == 1) {                      // every row its own pattern: the bits of i + 1 (as far as d allows)
                        for (uint32_t c = 0; c < d && c < 20; ++c)
                            if ((i + 1) >> c & 1) row[c] = std::numeric_limits<double>::quiet_NaN();
                    } else if (kind == 2) {                      // Bernoulli(0.3), every fifth row complete, every seventh all NaN
                        for (uint32_t c = 0; c < d; ++c)
                            if (i % 7 == 3 || (i % 5 != 0 && rng() % 10 < 3)) row[c] = std::numeric_limits<double>::quiet_NaN();
                    } else {                                     // two patterns, NaNs of every sign and payload
                        for (uint32_t c = i % 2; c < d; c += 3) row[c] = nan_with(rng(), rng() & 1);
                    }
                }
                check_plan(x, n, d);
                ++blocks;
            }
    // enough rows for the team to build the masks (five blocks of 4096 rows)
    {
        const uint32_t n = 20000, d = 5;
        std::vector<double> x((size_t)n * d);
        for (double& v : x) v = rng() % 10 < 3 ? std::numeric_limits<double>::quiet_NaN() : normal(rng);
        check_plan(x, n, d);
        ++blocks;
    }
    // NaNs with different payloads fall into one pattern
    {
        std::vector<double> x = {1.0, nan_with(1, false), 2.0, nan_with(0x8000000000000ull, true), 3.0, nan_with(0xfffffffffffffull, false)};
        const ImputePlan plan = impute_plan(x.data(), 3, 2, 2);
        CHECK(plan.patterns() == 1 && plan.n_observed[0] == 1 && plan.order[0] == 0 && plan.order[2] == 2);
        CHECK(plan.classes.size() == 1 && plan.classes[0].po == 4 && plan.classes[0].pm == 4);
    }
    // a leading dimension above d: the padding is not read as coordinates
    {
        const double q = std::numeric_limits<double>::quiet_NaN();
        std::vector<double> x = {1.0, q, q, 2.0, 3.0, q};
        const ImputePlan plan = impute_plan(x.data(), 2, 2, 3);
        CHECK(plan.patterns() == 2 && plan.complete == 1 && plan.n_observed[0] == 1);
    }
    if (failures) {
        std::printf("impute_plan_test: %d failures\n", failures);
        return 1;
    }
    std::printf("impute_plan_test: ok (%d blocks)\n", blocks);
    return 0;
}
