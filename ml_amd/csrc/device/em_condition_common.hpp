// What the conditioning kernels share (em_condition.hip, em_condition_sample.hip, em_condition_variance.hip, em_condition_quantile.hip):
// the prediction chain of a component on both tiers, the staged tile move, the register tier's waves, the two grids and the dispatch
// over the paddings. (em_condition.hip's own two kernels take the sync, the waves, the grids and the dispatch, and keep their chain and
// store written out.) Every function here is inlined into the kernel that calls it: the kernels stay one each, none with scratch, more
// LDS or fewer waves per SIMD than with this text written out (profiles/condition_shared_registers.txt, condition_shared_timing.txt).
// The record every kernel reads: [mu_O (PO) | mu_M (PM) | A^T (PO x PM: row c = observed coordinate c) | the kernel's own tail], in
// the paddings of condition_pad (device.hpp): +0.0, except the rows c >= dO of A^T: -0.0.
#pragma once
#include <type_traits>

#include "device.hpp"

namespace mlhip {

/// Steps 1 - 2 of the conditional mean's definition (em_condition.hip) on the register tier: t_j = mu_k,M[j], then
/// t_j = fma(A_k[j][c], x_c - mu_k,O[c], t_j) for ascending c, in groups of four coordinates. A coordinate c >= dO inside the last
/// group has x_c = mu_c = +0.0 and maps of -0.0, and fma(-0.0, +0.0, t) = t for EVERY t: the padding is an identity bit for bit.
/// `rec` is wave-uniform and the offsets are compile-time: mu and A reach the fma as scalar operands through the scalar cache.
/// PO and PM are the kernel's template arguments, x and tj its register arrays of those sizes. They come in as plain arguments, not as
/// template parameters, on purpose: the loops then unroll only once this text stands inside the kernel. As a template the chain is
/// unrolled on its own first, and em_condition_sample_kernel<8, 16> comes out with 32 AGPRs more and one wave per SIMD instead of two
/// (profiles/condition_shared_registers.txt). em_condition_kernel alone keeps the chain and its tile store written out (see there).
__device__ __forceinline__ void component_prediction(const double* rec, const double* x, int dO, double* tj, int PO, int PM)
{
#pragma unroll
    for (int j = 0; j < PM; ++j) tj[j] = rec[PO + j];
#pragma unroll
    for (int c0 = 0; c0 < PO; c0 += 4) {
        if (c0 < dO) {                                           // (wave-uniform: a group of four coordinates beyond dO is not run at all)
#pragma unroll
            for (int c = c0; c < c0 + 4; ++c) {
                const double z = x[c] - rec[c];
#pragma unroll
                for (int j = 0; j < PM; ++j) tj[j] = __builtin_fma(rec[PO + PM + c * PM + j], z, tj[j]);
            }
        }
    }
}

/// The same chain on the plain tier, for missing coordinate j of row i alone: the record unpadded, x_O from global memory. The same
/// order: the same bits.
__device__ __forceinline__ double plain_prediction(const double* rec, int dO, int dM, int j, const double* xt, size_t ldx, uint32_t i)
{
    const double* at = rec + dO + dM;
    double tj = rec[dO + j];
    for (int c = 0; c < dO; ++c) tj = __builtin_fma(at[(size_t)c * dM + j], xt[(size_t)c * ldx + i] - rec[c], tj);
    return tj;
}

/// What stands between a wave's stores to its staging tile and its reads of it (either way round).
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

/// `rows` x `width` contiguous doubles between global memory and a wave's staging tile (row stride S: odd, so a lane per row writes
/// without conflicts), 16 bytes per lane and trip, (row, col) carried along without a division. `mem` is 16-byte aligned.
template <bool LOAD>
__device__ __forceinline__ void move_staged(double* stage, int S, uint32_t rows, uint32_t width, double* __restrict__ mem, int lane)
{
    const uint32_t total = rows * width;
    const uint32_t step_rows = 128u / width, step_cols = 128u % width;
    uint32_t row = (2u * lane) / width, col = (2u * lane) % width;
    for (uint32_t e = 2u * lane; e < total; e += 128u) {
        uint32_t row1 = row, col1 = col + 1;
        if (col1 == width) { col1 = 0; ++row1; }
        if constexpr (LOAD) {
            if (e + 1 < total) {
                const double2 v = *reinterpret_cast<const double2*>(mem + e);
                stage[row * S + col] = v.x;
                stage[row1 * S + col1] = v.y;
            } else {
                stage[row * S + col] = mem[e];
            }
        } else {
            const double v0 = stage[row * S + col];
            if (e + 1 < total) {
                const double v1 = stage[row1 * S + col1];
                *reinterpret_cast<double2*>(mem + e) = make_double2(v0, v1);
            } else {
                mem[e] = v0;
            }
        }
        row += step_rows;
        col += step_cols;
        if (col >= width) { col -= width; ++row; }
    }
}

/// Waves per workgroup of a register-tier kernel whose per-lane state is a few arrays of PM doubles.
constexpr int condition_waves(int PM) { return PM <= 16 ? 4 : 2; }

inline uint32_t capped_grid(uint32_t blocks, int num_cus, int per_cu)
{
    const uint32_t cap = (uint32_t)(num_cus > 0 ? num_cus : 256) * per_cu;
    return blocks > cap ? cap : blocks;
}
/// The register tier's grid: tiles of 64 rows over W waves a workgroup, at most 4 workgroups per CU (the kernels stride over the rest).
inline uint32_t tile_grid(uint32_t n, int W, int num_cus) { return capped_grid(((n + 63) / 64 + W - 1) / W, num_cus, 4); }
/// The plain tier's grid: rows over 256 threads, at most 8 workgroups per CU.
inline uint32_t row_grid(uint32_t n, int num_cus) { return capped_grid((n + 255) / 256, num_cus, 8); }

/// f(PO, PM) with the register tier's paddings of (dO, dM) as std::integral_constant values, PM up to MAX_PM: the instantiations of
/// a kernel are the 4 x {4, 8, 16[, 32]} this names and no others. -1 where a padding does not exist.
template <int MAX_PM, int PO, class F>
int dispatch_missing(int dM, F& f)
{
    using O = std::integral_constant<int, PO>;
    switch (condition_pad(kConditionRegisters, dM)) {
    case 4: return f(O{}, std::integral_constant<int, 4>{});
    case 8: return f(O{}, std::integral_constant<int, 8>{});
    case 16: return f(O{}, std::integral_constant<int, 16>{});
    case 32:
        if constexpr (MAX_PM >= 32) return f(O{}, std::integral_constant<int, 32>{});
        else return -1;
    default: return -1;
    }
}
template <int MAX_PM, class F>
int dispatch_paddings(int dO, int dM, F f)
{
    switch (condition_pad(kConditionRegisters, dO)) {
    case 4: return dispatch_missing<MAX_PM, 4>(dM, f);
    case 8: return dispatch_missing<MAX_PM, 8>(dM, f);
    case 16: return dispatch_missing<MAX_PM, 16>(dM, f);
    case 32: return dispatch_missing<MAX_PM, 32>(dM, f);
    default: return -1;
    }
}

}  // namespace mlhip
