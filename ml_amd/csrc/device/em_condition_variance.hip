// Conditional variance of a Gaussian mixture for gfx950: Var[x_M | x_O] of every row of a chunk, from the log-responsibilities lw / lse
// an E-step kernel wrote for the MARGINAL mixture over the observed coordinates (exact form, with_lse = 1, fold = 0) and the table
// [mu_k,O | mu_k,M | A_k^T | c_k] per component: the record of em_condition.hip with the conditioned covariance C_k = Sigma_k,M|O
// (host::condition_covariances) behind it. Per row, on every tier, in this order:
//   pass 1  steps 1 - 4 of em_condition.hip unchanged: z_c = x_c - mu_k,O[c]; t_j = mu_k,M[j], t_j = fma(A_k[j][c], z_c, t_j) for
//           ascending c; r_k = exp_nonpos(lw_k - lse); y_j = +0.0, y_j = fma(r_k, t_j, y_j) for ascending k ONLY where r_k != 0.
//           y has the bits em_condition_kernel gives.
//   pass 2  for ascending k, ONLY where r_k != 0: t_j by the same chain (the same bits as in pass 1), u_j = t_j - y_j, and
//             diagonal form  s_j = fma(u_j, u_j, C_k[j][j]),             v_j  = fma(r_k, s_j, v_j)   from v_j  = +0.0;
//             full form      s = fma(u_a, u_b, C_k[a][b]) for b <= a,    V_ab = fma(r_k, s, V_ab)    from V_ab = +0.0; V_ba a copy.
// The diagonal of the full form has the bits of the diagonal form. The centred sum cannot go below zero on the diagonal where C_k[j][j]
// >= 0: every term is r (C + u^2) >= 0 and fma rounds a non-negative value to a non-negative one. A component with r_k == 0 leaves
// v as it is -- by the definition, as step 4 of the mean --, so the wave-level skip of em_condition.hip (a wave passes over a
// component none of its 64 rows has a share in) changes no bit here either, in either pass, and a row's output is a pure function
// of the row and the parameters: the grid, the chunk, the row's place in the block, the shard and the tier change no bit.
//
//   em_condition_variance_kernel<PO, PM, W, FULL>   lane = row: x_O (PO registers), t / u, y (PM each) and the accumulators (PM, or
//                                   PM (PM + 1) / 2 with FULL) in VGPRs; k wave-uniform and the record's offsets compile-time, so mu,
//                                   A and C reach the fma as scalar operands. Paddings and the -0.0 rows of A^T: em_condition.hip's.
//                                   The rows j >= dM read the record's padding and are never stored. The output goes through LDS
//                                   (odd row stride) and out as contiguous 16 bytes per lane, kRows rows of the wave's tile at a
//                                   time: 64 in the diagonal form; in the full form as many as keep the staging tile within the
//                                   diagonal form's 64 x 33 doubles (a row is dM^2 doubles there).
//   em_condition_variance_plain_kernel   any dO + dM <= 4096: thread = row, the output row is the accumulator, y and (full form) u in
//                                   a work array of the call, table from global memory, unpadded. Same order, same bits.
// Record: [mu_O (PO) | mu_M (PM) | A^T (PO x PM) | c]: c = diag(C_k) (PM) in the diagonal form, the lower triangle of C_k packed row by
// row ((a, b) at a (a + 1) / 2 + b, for the PADDED dM) in the full form; padding +0.0, except the rows c >= dO of A^T: -0.0.
#include "em_condition_common.hpp"
#include "exp_nonpos.hpp"

namespace mlhip {
namespace {

constexpr int kVarianceMaxRegisters = 32;        // dO and dM up to which the diagonal form's register tier exists
// The full form's register tier: the largest padded dM whose instantiations at every PO report no scratch
// (profiles/condition_variance_registers.txt). This is the one place that states the bound.
constexpr int kVarianceMaxRegistersFull = 16;

constexpr int tri(int a, int b) { return a * (a + 1) / 2 + b; }

/// Rows of a wave's tile staged per round: the staging tile is kRows x (row doubles | 1) <= 64 x 33 doubles.
constexpr int stage_rows(int PM, bool full) { return !full || PM <= 4 ? 64 : PM <= 8 ? 32 : 8; }

/// Doubles of a wave's staging tile: `rows` output rows at a time, and the 64 x dM tile of the mean.
__host__ __device__ constexpr size_t stage_doubles(int rows, int dM, bool full)
{
    const size_t out = (size_t)rows * ((size_t)(full ? dM * dM : dM) | 1), mean = (size_t)64 * ((size_t)dM | 1);
    return out > mean ? out : mean;
}

constexpr int variance_waves(int PM, bool full) { return full ? (PM <= 4 ? 4 : PM <= 8 ? 2 : 1) : condition_waves(PM); }

template <int PO, int PM, int W, bool FULL>
__global__ __launch_bounds__(64 * W) void em_condition_variance_kernel(const double* __restrict__ xt, size_t ldx, uint32_t n, int dO, int dM,
                                                                       int K, const double* __restrict__ lw, size_t ldr,
                                                                       const double* __restrict__ lse, const double* __restrict__ table,
                                                                       double* __restrict__ out, double* __restrict__ means, int skip)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    constexpr int NV = FULL ? PM * (PM + 1) / 2 : PM;            // accumulators per lane, and the doubles of c in a record
    constexpr int PS = PO + PM + PO * PM + NV;
    constexpr int kRows = stage_rows(PM, FULL);
    const int width = FULL ? dM * dM : dM;                       // doubles of an output row
    const int S = width | 1, SY = dM | 1;                        // LDS row strides of the staging tile: the output's and the mean's
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double* stage = sm + (size_t)wave * stage_doubles(kRows, dM, FULL);

    const uint32_t tiles = (n + 63) / 64;
    for (uint32_t t = blockIdx.x * W + wave; t < tiles; t += gridDim.x * W) {
        const uint32_t i = t * 64 + lane;                        // (beyond n: a padding row of the block, read but never stored)
        const bool live = i < n;
        double x[PO];
#pragma unroll
        for (int c = 0; c < PO; ++c) x[c] = c < dO ? xt[(size_t)c * ldx + i] : 0.0;
        const double l = lse[i];
        double y[PM];
#pragma unroll
        for (int j = 0; j < PM; ++j) y[j] = 0.0;

        // pass 1
        for (int k = 0; k < K; ++k) {
            const double r = live ? exp_nonpos(lw[(size_t)k * ldr + i] - l) : 0.0;
            const bool share = r != 0.0;                         // (a NaN has one: it reaches the output)
            if (skip && __ballot(share) == 0) continue;
            const double* __restrict__ rec = table + (size_t)k * PS;   // wave-uniform -> scalar loads
            double tj[PM];
            component_prediction(rec, x, dO, tj, PO, PM);
#pragma unroll
            for (int j = 0; j < PM; ++j) {
                const double v = __builtin_fma(r, tj[j], y[j]);
                y[j] = share ? v : y[j];
            }
        }

        // pass 2
        double acc[NV];
#pragma unroll
        for (int e = 0; e < NV; ++e) acc[e] = 0.0;
        for (int k = 0; k < K; ++k) {
            const double r = live ? exp_nonpos(lw[(size_t)k * ldr + i] - l) : 0.0;
            const bool share = r != 0.0;
            if (skip && __ballot(share) == 0) continue;
            const double* __restrict__ rec = table + (size_t)k * PS;
            const double* __restrict__ ck = rec + PO + PM + PO * PM;
            double u[PM];
            component_prediction(rec, x, dO, u, PO, PM);
#pragma unroll
            for (int j = 0; j < PM; ++j) u[j] = u[j] - y[j];
            if constexpr (FULL) {
#pragma unroll
                for (int a = 0; a < PM; ++a)
#pragma unroll
                    for (int b = 0; b <= a; ++b) {
                        const double s = __builtin_fma(u[a], u[b], ck[tri(a, b)]);
                        const double v = __builtin_fma(r, s, acc[tri(a, b)]);
                        acc[tri(a, b)] = share ? v : acc[tri(a, b)];
                    }
            } else {
#pragma unroll
                for (int j = 0; j < PM; ++j) {
                    const double s = __builtin_fma(u[j], u[j], ck[j]);
                    const double v = __builtin_fma(r, s, acc[j]);
                    acc[j] = share ? v : acc[j];
                }
            }
        }

        const uint32_t rows = n - t * 64 < 64 ? n - t * 64 : 64;
        if (means) {                                             // (wave-uniform) the mean's tile: 64 rows x dM
#pragma unroll
            for (int j = 0; j < PM; ++j)
                if (j < dM) stage[lane * SY + j] = y[j];
            wave_sync();
            move_staged<false>(stage, SY, rows, (uint32_t)dM, means + (size_t)t * 64 * (size_t)dM, lane);
            wave_sync();                                         // (the next stores to the tile wait for these reads)
        }
#pragma unroll 1
        for (uint32_t first = 0; first < rows; first += kRows) {
            const uint32_t mine = (uint32_t)lane - first;        // this lane's row of the round, if < kRows
            if (mine < (uint32_t)kRows) {
                if constexpr (FULL) {
#pragma unroll
                    for (int a = 0; a < PM; ++a)
#pragma unroll
                        for (int b = 0; b < PM; ++b)
                            if (a < dM && b < dM) stage[mine * S + a * dM + b] = acc[a >= b ? tri(a, b) : tri(b, a)];
                } else {
#pragma unroll
                    for (int j = 0; j < PM; ++j)
                        if (j < dM) stage[mine * S + j] = acc[j];
                }
            }
            wave_sync();
            const uint32_t now = rows - first < (uint32_t)kRows ? rows - first : (uint32_t)kRows;
            move_staged<false>(stage, S, now, (uint32_t)width, out + ((size_t)t * 64 + first) * (size_t)width, lane);
            wave_sync();
        }
    }
}

__global__ __launch_bounds__(256) void em_condition_variance_plain_kernel(const double* __restrict__ xt, size_t ldx, uint32_t n, int dO, int dM,
                                                                          int K, const double* __restrict__ lw, size_t ldr,
                                                                          const double* __restrict__ lse, const double* __restrict__ table,
                                                                          double* __restrict__ out, double* __restrict__ means,
                                                                          double* __restrict__ work, int full)
{
    const size_t nc = full ? (size_t)dM * (dM + 1) / 2 : (size_t)dM;
    const size_t PS = (size_t)dO + dM + (size_t)dO * dM + nc;
    const size_t width = full ? (size_t)dM * dM : (size_t)dM;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const double l = lse[i];
        double* y = work + (size_t)i * 2 * dM;                   // the call's work array: y, then u (full form)
        double* u = y + dM;
        double* v = out + (size_t)i * width;
        for (int j = 0; j < dM; ++j) y[j] = 0.0;
        for (int k = 0; k < K; ++k) {
            const double r = exp_nonpos(lw[(size_t)k * ldr + i] - l);
            if (!(r != 0.0)) continue;
            const double* rec = table + (size_t)k * PS;
            for (int j = 0; j < dM; ++j) y[j] = __builtin_fma(r, plain_prediction(rec, dO, dM, j, xt, ldx, i), y[j]);
        }
        if (full) {
            for (int a = 0; a < dM; ++a)
                for (int b = 0; b <= a; ++b) v[(size_t)a * dM + b] = 0.0;
        } else {
            for (int j = 0; j < dM; ++j) v[j] = 0.0;
        }
        for (int k = 0; k < K; ++k) {
            const double r = exp_nonpos(lw[(size_t)k * ldr + i] - l);
            if (!(r != 0.0)) continue;
            const double* rec = table + (size_t)k * PS;
            const double* ck = rec + dO + dM + (size_t)dO * dM;
            for (int j = 0; j < dM; ++j) {
                const double uj = plain_prediction(rec, dO, dM, j, xt, ldx, i) - y[j];
                if (full) u[j] = uj;
                else v[j] = __builtin_fma(r, __builtin_fma(uj, uj, ck[j]), v[j]);
            }
            if (!full) continue;
            for (int a = 0; a < dM; ++a)
                for (int b = 0; b <= a; ++b) {
                    const size_t e = (size_t)a * dM + b;
                    v[e] = __builtin_fma(r, __builtin_fma(u[a], u[b], ck[(size_t)a * (a + 1) / 2 + b]), v[e]);
                }
        }
        if (full)
            for (int a = 0; a < dM; ++a)
                for (int b = 0; b < a; ++b) v[(size_t)b * dM + a] = v[(size_t)a * dM + b];
        if (means)
            for (int j = 0; j < dM; ++j) means[(size_t)i * dM + j] = y[j];
    }
}

}  // namespace

int em_condition_variance_route(int dO, int dM, int full)
{
    const int bound = full ? kVarianceMaxRegistersFull : kVarianceMaxRegisters;
    return dO <= kVarianceMaxRegisters && dM <= bound ? kConditionRegisters : kConditionPlain;
}

int launch_em_condition_variance(const ConditionVarianceArgs& a, int num_cus, hipStream_t stream)
{
    if (a.dO < 1 || a.dM < 1 || a.dO + a.dM > kGenericMaxDim || a.K < 1) return -1;
    if (a.n == 0) return 0;
    if (a.kernel == kConditionPlain) {
        if (!a.work) return -1;
        const uint32_t grid = row_grid(a.n, num_cus);
        hipLaunchKernelGGL(em_condition_variance_plain_kernel, dim3(grid), dim3(256), 0, stream, a.xt, a.ldx, a.n, a.dO, a.dM, a.K, a.lw, a.ldr,
                           a.lse, a.table, a.out, a.means, a.work, a.full);
        return (int)grid;
    }
    if (em_condition_variance_route(a.dO, a.dM, a.full) != kConditionRegisters) return -1;
    const auto launch = [&](auto po, auto pm, auto full) {
        constexpr int PO = decltype(po)::value, PM = decltype(pm)::value;
        constexpr bool FULL = decltype(full)::value;
        constexpr int W = variance_waves(PM, FULL);
        const uint32_t grid = tile_grid(a.n, W, num_cus);
        const size_t bytes = sizeof(double) * (size_t)W * stage_doubles(stage_rows(PM, FULL), a.dM, FULL);
        hipLaunchKernelGGL((em_condition_variance_kernel<PO, PM, W, FULL>), dim3(grid), dim3(64 * W), bytes, stream, a.xt, a.ldx, a.n, a.dO, a.dM,
                           a.K, a.lw, a.ldr, a.lse, a.table, a.out, a.means, a.skip);
        return (int)grid;
    };
    if (a.full) return dispatch_paddings<kVarianceMaxRegistersFull>(a.dO, a.dM, [&](auto po, auto pm) { return launch(po, pm, std::true_type{}); });
    return dispatch_paddings<kVarianceMaxRegisters>(a.dO, a.dM, [&](auto po, auto pm) { return launch(po, pm, std::false_type{}); });
}

}  // namespace mlhip
