// Sources compiled in PARTS. The first launch of any kernel of a code object loads the WHOLE object (~3 ms per MB on the MI355X box,
// rocprofv3 --hip-trace of tools/first_call.py: 5.0 ms for the first K-means launch out of a 1.5 MB object); a fit uses one
// dimension and one component count, so the template-heavy files are compiled several times with -DMLHIP_PART=n (ml_amd/csrc/Makefile),
// every part holding the instantiations of a few shapes and exporting  <entry>_part<n>(...)  -- the dispatcher (in part 1) picks the
// part by shape. One code object per part: the first fit of a process loads a few hundred KB instead of several MB.
#pragma once
#ifndef MLHIP_PART
#error "this file is compiled in parts: -DMLHIP_PART=n (see ml_amd/csrc/Makefile)"
#endif
#define MLHIP_CAT2(a, b) a##b
#define MLHIP_CAT(a, b) MLHIP_CAT2(a, b)
#define MLHIP_PART_FN(name) MLHIP_CAT(name##_part, MLHIP_PART)

#include <type_traits>

#include "device.hpp"

// ---- sources compiled in SIX parts by padded dimension (em_diag.hip, em_tied.hip): 1: D = 1, 2; 2: 3, 4; 3: 6, 8; 4: 12, 16; 5: 20, 24;
// 6: 28, 32. Every part exports  <entry>_part<n>(args, grid, stream); part 1 also holds the dispatcher.
namespace mlhip {

/// f(std::integral_constant<int, D>) for D = padded_dim(d), if this part holds D; -1 otherwise.
template <typename F> int dispatch_part_dim(int d, F&& f)
{
    switch (padded_dim(d)) {
#define MLHIP_DIM_CASE(D) case D: return f(std::integral_constant<int, D>{});
#if MLHIP_PART == 1
    MLHIP_DIM_CASE(1) MLHIP_DIM_CASE(2)
#elif MLHIP_PART == 2
    MLHIP_DIM_CASE(3) MLHIP_DIM_CASE(4)
#elif MLHIP_PART == 3
    MLHIP_DIM_CASE(6) MLHIP_DIM_CASE(8)
#elif MLHIP_PART == 4
    MLHIP_DIM_CASE(12) MLHIP_DIM_CASE(16)
#elif MLHIP_PART == 5
    MLHIP_DIM_CASE(20) MLHIP_DIM_CASE(24)
#elif MLHIP_PART == 6
    MLHIP_DIM_CASE(28) MLHIP_DIM_CASE(32)
#endif
#undef MLHIP_DIM_CASE
    default: return -1;
    }
}

template <typename Args> using DimPartFn = int(const Args&, int, hipStream_t);

/// The six parts of `entry`, declared and listed as entry##_parts (for the dispatcher in part 1).
#define MLHIP_DECLARE_DIM_PARTS(entry, Args)                                                                                     \
    int entry##_part1(const Args&, int, hipStream_t); int entry##_part2(const Args&, int, hipStream_t);                         \
    int entry##_part3(const Args&, int, hipStream_t); int entry##_part4(const Args&, int, hipStream_t);                         \
    int entry##_part5(const Args&, int, hipStream_t); int entry##_part6(const Args&, int, hipStream_t);                         \
    static DimPartFn<Args>* const entry##_parts[6] = {entry##_part1, entry##_part2, entry##_part3, entry##_part4, entry##_part5, \
                                                      entry##_part6};

/// The dispatcher: `grid` cut to the log-likelihood partials and to the partial blocks (`block` doubles each) the scratch of `a`
/// holds, then the part of a.d. Returns what the part returns (the grid), -2 where not one block fits.
template <typename Args> int launch_dim_part(const Args& a, int grid, size_t block, DimPartFn<Args>* const (&parts)[6], hipStream_t stream)
{
    if (grid > a.n_ll_partials) grid = a.n_ll_partials;
    if ((size_t)grid * block > a.partials_capacity) grid = (int)(a.partials_capacity / block);
    if (grid < 1) return -2;
    const int D = padded_dim(a.d);
    return parts[D <= 2 ? 0 : D <= 4 ? 1 : D <= 8 ? 2 : D <= 16 ? 3 : D <= 24 ? 4 : 5](a, grid, stream);
}

}  // namespace mlhip
