// The fixed-order combination of per-workgroup partial blocks as a device function, shared by em_reduce_kernel (em_mstats.hip: one
// statistics buffer per launch) and the restarts' batched reduction (em_restarts.hip: one per restart in the launch) -- one text, so
// the two sum in the same order and give the same bits.
#pragma once
#include "device.hpp"

namespace mlhip {
namespace mstats {

/// stats[k*F + f] = sum_b partials[b][k][f], stats[K*F] = sum of the ll partials. Fixed order, hence reproducible run to run
/// and identical on every rank: 8 outputs per workgroup, each summed by 32 threads over the block slices b = s, s + 32, ...
/// (ascending), the 32 slice sums added in ascending s. (One thread per output walking all partial blocks, as in round 1, is
/// latency-bound: 24 us for the 528 outputs of the diagonal configuration; 8 slices, round 2: 9.6 us with 768 partial blocks --
/// the chain of dependent loads per thread is what it costs, so round 3 cuts it to a quarter.)
/// `block`: the workgroup's place among the (K F + kRedOut - 1) / kRedOut + 1 of one buffer's reduction (the last one sums the
/// log-likelihood partials); `red`: 256 doubles of the calling workgroup's LDS (256 threads).
constexpr int kRedOut = 8, kRedSlices = 32;
__device__ __forceinline__ void em_reduce_body(const double* __restrict__ partials, int n_blocks, int KP, int FP, int K, int F,
                                               const double* __restrict__ ll_partials, int n_ll, double* __restrict__ stats, int block,
                                               double* red)
{
    const int total = K * F;
    if (block * kRedOut < total) {
        const int o = threadIdx.x & (kRedOut - 1), sl = threadIdx.x / kRedOut;
        const int e = block * kRedOut + o;
        double s = 0.0;
        if (e < total) {
            const int k = e / F, f = e - k * F;
            const double* p = partials + (size_t)k * FP + f;
            int b = sl;
            for (; b + 3 * kRedSlices < n_blocks; b += 4 * kRedSlices) {          // 4 loads in flight, consumed in order
                const double v0 = p[(size_t)b * KP * FP], v1 = p[(size_t)(b + kRedSlices) * KP * FP];
                const double v2 = p[(size_t)(b + 2 * kRedSlices) * KP * FP], v3 = p[(size_t)(b + 3 * kRedSlices) * KP * FP];
                s += v0; s += v1; s += v2; s += v3;
            }
            for (; b < n_blocks; b += kRedSlices) s += p[(size_t)b * KP * FP];
        }
        red[threadIdx.x] = s;
        __syncthreads();
        if (sl == 0 && e < total) {
            double t = red[o];
#pragma unroll
            for (int q = 1; q < kRedSlices; ++q) t += red[q * kRedOut + o];
            stats[e] = t;
        }
    } else {
        // one extra block: log-likelihood partials (fixed-order tree)
        double s = 0.0;
        for (int b = threadIdx.x; b < n_ll; b += 256) s += ll_partials[b];
        red[threadIdx.x] = s;
        __syncthreads();
        for (int off = 128; off > 0; off >>= 1) {
            if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
            __syncthreads();
        }
        if (threadIdx.x == 0) stats[total] = red[0];
    }
}

}  // namespace mstats
}  // namespace mlhip
