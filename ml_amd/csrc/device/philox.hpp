// The counter-based generator of the sampling kernels (em_sample.hip, em_condition_sample.hip): Philox4x32-10 under the key
// (seed lo, seed hi) on the counter (i lo, i hi, block, stream) of a row's 64-bit GLOBAL index i. `stream`, the fourth counter word,
// keeps the calls apart that share a seed: mlhip_em_sample draws on stream 0, draw q of mlhip_em_conditional_samples on stream 1 + q.
//   U(lo, hi) = (((hi 2^32 + lo) >> 12) + 1/2) 2^-52;
//   block 1 + p:  u1 = U(w0, w1), u2 = U(w2, w3), r = sqrt(-2 log u1), z_2p = r cospi(2 u2), z_2p+1 = r sinpi(2 u2).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mlhip {

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t (&w)[4])
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

/// (((hi 2^32 + lo) >> 12) + 1/2) 2^-52: every step exact in fp64, strictly inside (0, 1).
__device__ __forceinline__ double unit_uniform(uint32_t lo, uint32_t hi)
{
    const uint64_t v = (((uint64_t)hi << 32) | lo) >> 12;
    return ((double)v + 0.5) * 0x1p-52;
}

/// The uniform of row i's block 0 on `stream`: what a label is drawn with.
__device__ __forceinline__ double draw_uniform(uint64_t i, uint64_t seed, uint32_t stream)
{
    uint32_t w[4];
    philox4x32_10((uint32_t)i, (uint32_t)(i >> 32), 0u, stream, (uint32_t)seed, (uint32_t)(seed >> 32), w);
    return unit_uniform(w[0], w[1]);
}

/// Normals z_2p, z_2p+1 of row i on `stream`.
__device__ __forceinline__ void draw_pair(uint64_t i, uint64_t seed, uint32_t p, uint32_t stream, double& z0, double& z1)
{
    uint32_t w[4];
    philox4x32_10((uint32_t)i, (uint32_t)(i >> 32), 1u + p, stream, (uint32_t)seed, (uint32_t)(seed >> 32), w);
    const double u1 = unit_uniform(w[0], w[1]), u2 = unit_uniform(w[2], w[3]);
    const double r = sqrt(-2.0 * log(u1));
    double s, c;
    sincospi(2.0 * u2, &s, &c);
    z0 = r * c;
    z1 = r * s;
}

}  // namespace mlhip
