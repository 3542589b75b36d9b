// Staging of the self-normalising statistics kernels (em_mstats_wide.hip EXP = 2, em_mstats_sparse.hip): a sample's K
// log-responsibilities are normalised while the tile is written to LDS. Both kernels run this same code, so the per-sample
// (max, sum of exponentials) -- and with them lse and the log-likelihood -- are bit-identical whichever kernel ran.
#pragma once
#include "device.hpp"
#include "exp_nonpos.hpp"

namespace mlhip {
namespace mstats {

/// Partner values for all-reductions over lane bits 3, 4, 5 without the LDS pipe (a __shfl_xor of a double is two
/// ds_bpermute: ~100 cycles of latency each, six of them in a row in the staging phase where every wave of the CU waits):
/// bit 3 by a DPP row rotation, bits 4 and 5 by v_permlane16_swap / v_permlane32_swap.
__device__ __forceinline__ double partner_xor8(double v)
{
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), 0x128, 0xf, 0xf, false);   // row_ror:8
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), 0x128, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
template <bool BIT5> __device__ __forceinline__ void partners_swap(double v, double& a, double& b)
{
    // a = v, b = v; swap: afterwards (a, b) hold {own half-or-row value, partner's} such that op(a, b) is the pairwise result
    const unsigned lo = __double2loint(v), hi = __double2hiint(v);
    if constexpr (BIT5) {
        const auto l = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
        const auto h = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
        a = __hiloint2double((int)h[0], (int)l[0]);
        b = __hiloint2double((int)h[1], (int)l[1]);
    } else {
        const auto l = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
        const auto h = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
        a = __hiloint2double((int)h[0], (int)l[0]);
        b = __hiloint2double((int)h[1], (int)l[1]);
    }
}
__device__ __forceinline__ double allreduce_max_bits345(double v)
{
    double a, b;
    v = fmax(v, partner_xor8(v));
    partners_swap<false>(v, a, b);
    v = fmax(a, b);
    partners_swap<true>(v, a, b);
    return fmax(a, b);
}
__device__ __forceinline__ double allreduce_sum_bits345(double v)
{
    double a, b;
    v += partner_xor8(v);
    partners_swap<false>(v, a, b);
    v = a + b;
    partners_swap<true>(v, a, b);
    return a + b;
}

/// Normalises the NRV log-responsibilities rv[] of sample `sR` (components NRV cg .. NRV cg + NRV - 1; the 8 lanes with the
/// same lane & 7 hold all K of the sample), writes r = exp(lw - max) / sum to Rb[sR * RS + component] (0 for padding samples
/// and components >= K) and, if `write_lse`, max and sum to lse_out[i] / esum_out[i]. Returns how many of the wave's 64 x NRV
/// written responsibilities are nonzero (wave-uniform). WEIGHTED (a block with row weights): the value written is r w_i, the
/// sample's frequency weight `wi` applied AFTER the normalisation (one rounding more than r); max and sum -- hence lse -- stay the
/// sample's own. MASKS: nz[it] receives the wave's ballot of "written value `it` is nonzero" (bit = lane) -- the ballots the count
/// is made of anyway; the sparse kernel builds its buckets from them. KMASK = false: the caller has already set the rv[] of the
/// components >= K to -inf (the sparse kernel, which skips that when K fills every slot).
template <int NRV, int RS, bool WEIGHTED = false, bool MASKS = false, bool KMASK = true>
__device__ __forceinline__ uint32_t stage_self_norm(double (&rv)[NRV], int cg, int K, uint32_t i, bool live, double* Rb, int sR,
                                                     bool write_lse, double* __restrict__ lse_out, double* __restrict__ esum_out,
                                                     double wi = 1.0, unsigned long long* nz = nullptr)
{
    double m = -__builtin_inf();
#pragma unroll
    for (int it = 0; it < NRV; ++it) {
        if constexpr (KMASK)
            if (cg * NRV + it >= K) rv[it] = -__builtin_inf();      // components beyond K: exp(-inf) = 0
        m = fmax(m, rv[it]);
    }
    m = allreduce_max_bits345(m);
    double sum = 0.0;
#pragma unroll
    for (int it = 0; it < NRV; ++it) {
        rv[it] = exp_nonpos(rv[it] - m);
        sum += rv[it];
        __builtin_amdgcn_sched_barrier(0);          // one exp at a time: interleaved they spill next to 160 accumulator registers
    }
    sum = allreduce_sum_bits345(sum);
    const double inv = live ? 1.0 / sum : 0.0;                      // padding samples contribute nothing
    uint32_t nonzero = 0;
#pragma unroll
    for (int it = 0; it < NRV; ++it) {
        double r = rv[it] * inv;
        if constexpr (WEIGHTED) r = wi != 0.0 ? r * wi : 0.0;         // a row of weight 0 is not in the sample, whatever its density
        Rb[sR * RS + cg * NRV + it] = r;
        const unsigned long long b = __ballot(r != 0.0);
        if constexpr (MASKS) nz[it] = b;
        nonzero += (uint32_t)__builtin_popcountll(b);
    }
    // lse = m + log(sum) is finished by a separate pass over these two N-vectors (em_lse_finish_kernel): a log in
    // this loop, next to 160 accumulator registers, cost 0.8 ms at the headline shape in spills and scheduling
    if (cg == 0 && write_lse) {
        lse_out[i] = m;
        esum_out[i] = sum;
    }
    return nonzero;
}

}  // namespace mstats
}  // namespace mlhip
