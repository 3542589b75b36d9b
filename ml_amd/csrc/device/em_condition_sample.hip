// Conditional draws from a Gaussian mixture for gfx950: x_M | x_O for every row of a chunk and every draw of a range, from the
// log-responsibilities lw / lse an E-step kernel wrote for the MARGINAL mixture over the observed coordinates (exact form,
// with_lse = 1, fold = 0) and the table [mu_k,O | mu_k,M | A_k^T | G_k] per component: A_k = Sigma_k,MO Sigma_k,OO^-1 (host::condition),
// G_k the lower Cholesky factor of Sigma_k,M|O (host::condition_covariances). Per row i (a 64-bit GLOBAL index) and draw q, on every
// tier, in this order:
//   1. r_k = exp_nonpos(lw_k - lse)                             the responsibility em_condition.hip and em_resp_kernel form;
//   2. s_k = s_{k-1} + r_k (s_-1 = +0.0, ascending k), S = s_{K-1};
//   3. u = U(w0, w1) of Philox4x32-10 (philox.hpp) under the key (seed lo, seed hi) on the counter (i lo, i hi, 0, 1 + q);
//      label = the smallest k with u S < s_k (one fp64 product); if there is none, the largest k with r_k != 0. A component with
//      r_k == 0 has s_k == s_{k-1} and is never drawn. A row whose S is a NaN (or that has no r_k != 0 at all) gives a NaN in every
//      coordinate and the label 0xFFFFFFFF;
//   4. zeta_2p, zeta_2p+1 = draw_pair on the counter (i lo, i hi, 1 + p, 1 + q), p = 0 .. ceil(dM / 2) - 1;
//   5. with k = label: z_c = x_c - mu_k,O[c]; t_j = mu_k,M[j], t_j = fma(A_k[j][c], z_c, t_j) for c = 0 .. dO-1 ascending (the chain
//      of em_condition.hip), then t_j = fma(G_k[j][c], zeta_c, t_j) for c = 0 .. j ascending; x~_j = t_j.
// The fourth counter word is 1 + q, never the sampler's 0: a seed shared with mlhip_em_sample shares no random word with it. Row
// (i, q) is a pure function of (seed, i, q), the row's x_O and the parameters: the grid, the chunk, the row's place in the block, how
// a call is split over first_row or first_draw, the shard and the tier change no bit.
//
//   em_condition_sample_kernel<PO, PM, W>  dO, dM <= 32 (paddings 4 / 8 / 16 / 32 as em_condition_kernel), lane = row. Pass 1 over the
//                                   row's lw column forms S; pass 2 the labels of up to kDrawGroup draws at once (they wait in
//                                   LDS). Per draw: zeta (PM registers), x_O (PO, loaded behind the normals), then a wave-uniform walk
//                                   over k that runs component k only where some lane drew it (__ballot): t (PM) in VGPRs, mu, A and G as
//                                   scalar operands from the record (k is wave-uniform, the offsets compile-time), the finished row
//                                   stored into the wave's LDS tile by the lanes that drew k. The padding of the chain is the
//                                   identity of em_condition.hip (maps of -0.0 against z = +0.0); rows j >= dM are not run. Then the
//                                   sampler's epilogue: the 64 x dM tile out as contiguous 16 bytes per lane.
//   em_condition_sample_plain_kernel  any dO + dM <= 4096: thread = row, the normals go into the output row, the chain and the product
//                                   run there in place from j = dM-1 down, table from global memory. The same order: the same bits.
// Record: [mu_O (PO) | mu_M (PM) | A^T (PO x PM) | G (PM (PM+1) / 2: (j, c) at j (j+1)/2 + c)]; padding as em_condition.hip, +0.0 in G.
#include "em_condition_common.hpp"
#include "exp_nonpos.hpp"
#include "philox.hpp"

namespace mlhip {
namespace {

constexpr int kDrawGroup = 8;                    // draws whose labels one pass over the lw column forms

template <int PO, int PM, int W>
__global__ __launch_bounds__(64 * W) void em_condition_sample_kernel(const double* __restrict__ xt, const double* __restrict__ lw,
                                                                     const double* __restrict__ lse, const double* __restrict__ table,
                                                                     double* __restrict__ out, uint32_t* __restrict__ labels,
                                                                     ConditionSampleArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    constexpr int PA = PO + PM + PO * PM, PS = PA + PM * (PM + 1) / 2;
    const int dO = a.dO, dM = a.dM, K = a.K;
    const int S = dM | 1;                                        // LDS row stride of the staging tile
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double* stage = sm + (size_t)wave * 64 * S;
    uint32_t* drawn = reinterpret_cast<uint32_t*>(sm + (size_t)W * 64 * S) + (size_t)wave * 64 * kDrawGroup;

    const uint32_t tiles = (a.n + 63) / 64;
    for (uint32_t t = blockIdx.x * W + wave; t < tiles; t += gridDim.x * W) {
        const uint32_t local = t * 64 + lane;                    // (beyond n: a padding row of the block, read but never stored)
        const bool live = local < a.n;
        const uint64_t i = a.first_row + local;
        const double l = lse[local];
        double total = 0.0;
        for (int k = 0; k < K; ++k) total += live ? exp_nonpos(lw[(size_t)k * a.ldr + local] - l) : 0.0;

        for (uint32_t q0 = 0; q0 < a.n_draws; q0 += kDrawGroup) {
            const uint32_t nq = a.n_draws - q0 < (uint32_t)kDrawGroup ? a.n_draws - q0 : (uint32_t)kDrawGroup;
            double target[kDrawGroup];
            uint32_t label[kDrawGroup];
#pragma unroll
            for (int g = 0; g < kDrawGroup; ++g) {
                target[g] = 0.0;
                label[g] = kConditionSampleNoLabel;
                if ((uint32_t)g < nq) target[g] = draw_uniform(i, a.seed, 1u + a.first_draw + q0 + (uint32_t)g) * total;
                __builtin_amdgcn_sched_barrier(0);               // (one generator at a time: interleaved, their temporaries cost registers)
            }
            double s = 0.0;
            uint32_t last = kConditionSampleNoLabel;
            for (int k = 0; k < K; ++k) {
                const double r = live ? exp_nonpos(lw[(size_t)k * a.ldr + local] - l) : 0.0;
                s += r;
                last = r != 0.0 ? (uint32_t)k : last;
#pragma unroll
                for (int g = 0; g < kDrawGroup; ++g)
                    label[g] = label[g] == kConditionSampleNoLabel && target[g] < s ? (uint32_t)k : label[g];
            }
#pragma unroll
            for (int g = 0; g < kDrawGroup; ++g) {
                const uint32_t v = label[g] == kConditionSampleNoLabel ? last : label[g];
                drawn[g * 64 + lane] = total != total ? kConditionSampleNoLabel : v;   // (a lane reads back only what it wrote)
            }

            for (uint32_t g = 0; g < nq; ++g) {
                const uint32_t mine = drawn[g * 64 + lane];
                if (labels && live) labels[(size_t)(q0 + g) * a.n + local] = mine;
                double z[PM];
#pragma unroll
                for (int p = 0; p < PM / 2; ++p) {
                    z[2 * p] = 0.0;
                    z[2 * p + 1] = 0.0;
                    if (2 * p < dM) draw_pair(i, a.seed, (uint32_t)p, 1u + a.first_draw + q0 + g, z[2 * p], z[2 * p + 1]);
                    __builtin_amdgcn_sched_barrier(0);           // (one pair at a time: interleaved, their temporaries cost registers)
                }
                // x_O comes in behind the normals, once per draw: log and sincospi take some hundred registers of their own, and a
                // row held across them would not fit beside them at the larger paddings
                asm volatile("" ::: "memory");
                double x[PO];
#pragma unroll
                for (int c = 0; c < PO; ++c) x[c] = c < dO ? xt[(size_t)c * a.ldx + local] : 0.0;
                if (mine == kConditionSampleNoLabel) {
                    for (int j = 0; j < dM; ++j) stage[lane * S + j] = __builtin_nan("");
                }
                for (int k = 0; k < K; ++k) {
                    const bool run = mine == (uint32_t)k;
                    if (__ballot(run) == 0) continue;
                    const double* __restrict__ rec = table + (size_t)k * PS;   // wave-uniform -> scalar loads
                    double tj[PM];
                    component_prediction(rec, x, dO, tj, PO, PM);
#pragma unroll
                    for (int j = 0; j < PM; ++j) {
                        if (j < dM) {                            // (wave-uniform)
#pragma unroll
                            for (int c = 0; c <= j; ++c) tj[j] = __builtin_fma(rec[PA + j * (j + 1) / 2 + c], z[c], tj[j]);
                            if (run) stage[lane * S + j] = tj[j];
                        }
                    }
                }
                wave_sync();
                const uint32_t rows = a.n - t * 64 < 64 ? a.n - t * 64 : 64;
                move_staged<false>(stage, S, rows, (uint32_t)dM, out + (size_t)(q0 + g) * a.ldq + (size_t)t * 64 * (size_t)dM, lane);
                wave_sync();                                     // (the next draw's stores wait for these reads)
            }
        }
    }
}

__global__ __launch_bounds__(256) void em_condition_sample_plain_kernel(ConditionSampleArgs a)
{
    const int dO = a.dO, dM = a.dM, K = a.K;
    const size_t PS = (size_t)dO + dM + (size_t)dO * dM + (size_t)dM * (dM + 1) / 2;
    for (uint32_t local = blockIdx.x * 256u + threadIdx.x; local < a.n; local += gridDim.x * 256u) {
        const uint64_t i = a.first_row + local;
        const double l = a.lse[local];
        double total = 0.0;
        for (int k = 0; k < K; ++k) total += exp_nonpos(a.lw[(size_t)k * a.ldr + local] - l);
        for (uint32_t q = 0; q < a.n_draws; ++q) {
            const uint32_t stream = 1u + a.first_draw + q;
            const double target = draw_uniform(i, a.seed, stream) * total;
            double s = 0.0;
            uint32_t label = kConditionSampleNoLabel, last = kConditionSampleNoLabel;
            for (int k = 0; k < K; ++k) {
                const double r = exp_nonpos(a.lw[(size_t)k * a.ldr + local] - l);
                s += r;
                last = r != 0.0 ? (uint32_t)k : last;
                label = label == kConditionSampleNoLabel && target < s ? (uint32_t)k : label;
            }
            if (label == kConditionSampleNoLabel) label = last;
            if (total != total) label = kConditionSampleNoLabel;
            if (a.labels) a.labels[(size_t)q * a.n + local] = label;
            double* row = a.out + (size_t)q * a.ldq + (size_t)local * dM;
            if (label == kConditionSampleNoLabel) {
                for (int j = 0; j < dM; ++j) row[j] = __builtin_nan("");
                continue;
            }
            for (int p = 0; 2 * p < dM; ++p) {
                double z0, z1;
                draw_pair(i, a.seed, (uint32_t)p, stream, z0, z1);
                row[2 * p] = z0;
                if (2 * p + 1 < dM) row[2 * p + 1] = z1;
            }
            const double* rec = a.table + (size_t)label * PS;
            const double* G = rec + dO + dM + (size_t)dO * dM;
            for (int j = dM - 1; j >= 0; --j) {
                double tj = plain_prediction(rec, dO, dM, j, a.xt, a.ldx, local);
                const double* Gj = G + (size_t)j * (j + 1) / 2;
                for (int c = 0; c <= j; ++c) tj = __builtin_fma(Gj[c], row[c], tj);
                row[j] = tj;                                     // (zeta_j is not read again: the rows below j are done)
            }
        }
    }
}

}  // namespace

int launch_em_condition_sample(const ConditionSampleArgs& a, int num_cus, hipStream_t stream)
{
    if (a.dO < 1 || a.dM < 1 || a.dO + a.dM > kGenericMaxDim || a.K < 1) return -1;
    if ((a.ldq & 1) || a.ldq < (size_t)a.n * (size_t)a.dM) return -1;
    if (a.n == 0 || a.n_draws == 0) return 0;
    if (a.kernel == kConditionPlain) {
        const uint32_t grid = row_grid(a.n, num_cus);
        hipLaunchKernelGGL(em_condition_sample_plain_kernel, dim3(grid), dim3(256), 0, stream, a);
        return (int)grid;
    }
    return dispatch_paddings<32>(a.dO, a.dM, [&](auto po, auto pm) {
        constexpr int PO = decltype(po)::value, PM = decltype(pm)::value, W = condition_waves(PM);
        const uint32_t grid = tile_grid(a.n, W, num_cus);
        const size_t bytes = sizeof(double) * (size_t)W * 64 * (size_t)(a.dM | 1) + sizeof(uint32_t) * (size_t)W * 64 * kDrawGroup;
        // (the pointers once more as parameters of their own: __restrict__ there is what lets the table come in through scalar loads)
        hipLaunchKernelGGL((em_condition_sample_kernel<PO, PM, W>), dim3(grid), dim3(64 * W), bytes, stream, a.xt, a.lw, a.lse, a.table, a.out, a.labels, a);
        return (int)grid;
    });
}

}  // namespace mlhip
