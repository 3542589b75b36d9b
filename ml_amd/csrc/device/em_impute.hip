// The evaluation kernel of mlhip_em_impute's kernel route for gfx950: E[x_M | x_O] with a pattern per ROW. It follows
// em_condition_kernel (em_condition.hip): lane = row, 64-row tiles -- but a tile belongs to exactly one pattern, and its descriptor
// names the rows and the pattern whose records it reads (device.hpp: ImputeTile, ImputePattern). The record base is wave-uniform, so
// mu, W and A reach the fma as scalar operands; x_O, z, t and y live in VGPRs. Per row, with the record of its pattern, in this order
// (mlhip.h, mlhip_em_impute):
//   1. z_c = x_c - mu_k,O[c];
//   2. y_j = W[j][0] z_0, then fma over l = 1 .. j ascending; q = +0.0, then fma(y_j, y_j, q) for ascending j;
//   3. lw_k = fma(-0.5, q, coef_k);
//   4. the online log-sum-exp over ascending k, the statement of em_estep.hip;
//   5. r_k = exp_nonpos(lw_k - lse);
//   6. t_j = mu_k,M[j], then fma(A_k[j][c], z_c, t_j) for ascending c (component_prediction); y_j = +0.0, then fma(r_k, t_j, y_j) for
//      ascending k, only where r_k != 0.
// Steps 1 - 4 run over all components first; the second loop evaluates steps 1 - 3 again -- the same instructions on the same
// operands, the same bits -- instead of keeping K log-weights per row: no N x K block exists on this route. The skip is
// em_condition_kernel's: a wave passes over steps 6 of a component none of its rows has a share in.
// The chains run in groups of four coordinates; a coordinate c >= dO inside the last group has x_c = mu_c = +0.0, a row of W of +0.0
// and a row of A^T of -0.0: identities bit for bit. Lanes beyond the tile's rows repeat its last row and store nothing.
// The wave's rows x dM tile goes through LDS (odd row stride) and out as contiguous 16 bytes per lane (move_staged).
#include "em_condition_common.hpp"
#include "exp_nonpos.hpp"

namespace mlhip {
namespace {

/// Steps 1 - 3 for one component: the log-weight of the row whose observed coordinates are x. PO, PM: the kernel's template
/// arguments, as plain arguments for the reason component_prediction gives.
__device__ __forceinline__ double marginal_log_weight(const double* rec, const double* x, int dO, int PO, int PM)
{
    const double* w = rec + PO + PM + PO * PM;
    double z[kImputeMaxDim];
#pragma unroll
    for (int c = 0; c < PO; ++c) z[c] = x[c] - rec[c];
    double q = 0.0;
#pragma unroll
    for (int j0 = 0; j0 < PO; j0 += 4) {
        if (j0 < dO) {                                           // (wave-uniform: a group of four rows beyond dO is not run at all)
#pragma unroll
            for (int j = j0; j < j0 + 4; ++j) {
                double y = w[j * (j + 1) / 2] * z[0];
#pragma unroll
                for (int l = 1; l <= j; ++l) y = __builtin_fma(w[j * (j + 1) / 2 + l], z[l], y);
                q = __builtin_fma(y, y, q);
            }
            // Keeps the scalar loads of later rows from being hoisted (and spilled) above this point (em_estep.hip).
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    return __builtin_fma(-0.5, q, w[PO * (PO + 1) / 2]);
}

template <int PO, int PM, int W>
__global__ __launch_bounds__(64 * W) void em_impute_kernel(const double* __restrict__ xs, int d, int K,
                                                           const ImputePattern* __restrict__ patterns, const double* __restrict__ records,
                                                           const ImputeTile* __restrict__ tiles, uint32_t n_tiles, double* __restrict__ out,
                                                           double* __restrict__ lse_out, double* __restrict__ resp, size_t ldr, int skip)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    constexpr int PS = PO + PM + PO * PM + PO * (PO + 1) / 2 + 1;
    constexpr int S = PM + 1;                                    // LDS row stride of the staging tile (odd)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double* stage = sm + (size_t)wave * 64 * S;

    for (uint32_t t = blockIdx.x * W + wave; t < n_tiles; t += gridDim.x * W) {
        const uint32_t tu = __builtin_amdgcn_readfirstlane(t);   // (the wave's own tile: everything read through it is wave-uniform)
        const ImputeTile tile = tiles[tu];
        const ImputePattern* __restrict__ pat = patterns + tile.pattern;
        const int dO = (int)pat->dO, dM = (int)pat->dM;
        const double* __restrict__ table = records + pat->rec_base;
        const bool live = (uint32_t)lane < tile.rows;
        const uint32_t row = tile.first + (live ? (uint32_t)lane : tile.rows - 1);
        const double* xr = xs + (size_t)row * d;
        double x[PO];
#pragma unroll
        for (int c = 0; c < PO; ++c) x[c] = c < dO ? xr[pat->observed[c]] : 0.0;

        // steps 1 - 4
        double m = -__builtin_inf(), s = 0.0;
        for (int k = 0; k < K; ++k) {
            const double lw = marginal_log_weight(table + (size_t)k * PS, x, dO, PO, PM);
            const double e = exp_nonpos(lw == -HUGE_VAL ? -HUGE_VAL : -fabs(lw - m));
            const bool up = lw > m;
            s = up ? __builtin_fma(s, e, 1.0) : s + e;
            m = up ? lw : m;
        }
        const double l = m + log(s);
        if (live) lse_out[row] = l;

        // steps 5 - 6
        double y[PM];
#pragma unroll
        for (int j = 0; j < PM; ++j) y[j] = 0.0;
        for (int k = 0; k < K; ++k) {
            const double* __restrict__ rec = table + (size_t)k * PS;
            const double lw = marginal_log_weight(rec, x, dO, PO, PM);
            const double r = live ? exp_nonpos(lw - l) : 0.0;
            if (resp && live) resp[(size_t)k * ldr + row] = r;
            const bool share = r != 0.0;                         // (a NaN has one: it reaches the output)
            if (skip && __ballot(share) == 0) continue;
            double tj[PM];
            component_prediction(rec, x, dO, tj, PO, PM);
#pragma unroll
            for (int j = 0; j < PM; ++j) {
                const double v = __builtin_fma(r, tj[j], y[j]);
                y[j] = share ? v : y[j];
            }
        }
#pragma unroll
        for (int j = 0; j < PM; ++j)
            if (j < dM) stage[lane * S + j] = y[j];
        wave_sync();
        move_staged<false>(stage, S, tile.rows, (uint32_t)dM, out + tile.out_base, lane);
        wave_sync();                                             // (the next tile's stores wait for these reads)
    }
}

}  // namespace

int launch_em_impute(const ImputeArgs& a, int num_cus, hipStream_t stream)
{
    if (a.d < 2 || a.d > kImputeMaxDim || a.K < 1) return -1;
    if (a.n_tiles == 0) return 0;
    return dispatch_paddings<32>(a.po, a.pm, [&](auto po, auto pm) {
        constexpr int PO = decltype(po)::value, PM = decltype(pm)::value, W = condition_waves(PO > PM ? PO : PM);
        if constexpr (PO + PM > 48) {
            return -1;                                           // (dO + dM <= 32: no pattern pads to 32 x 32)
        } else {
            uint32_t grid = capped_grid((a.n_tiles + W - 1) / W, num_cus, 4);
            if (a.grid_cap > 0 && grid > (uint32_t)a.grid_cap) grid = (uint32_t)a.grid_cap;
            const size_t bytes = sizeof(double) * (size_t)W * 64 * (size_t)(PM + 1);
            hipLaunchKernelGGL((em_impute_kernel<PO, PM, W>), dim3(grid), dim3(64 * W), bytes, stream, a.x, a.d, a.K, a.patterns, a.records,
                               a.tiles, a.n_tiles, a.y, a.lse, a.resp, a.ldr, a.skip);
            return (int)grid;
        }
    });
}

}  // namespace mlhip
