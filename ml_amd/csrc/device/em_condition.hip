// Conditional mean of a Gaussian mixture for gfx950: E[x_M | x_O] of every row of a chunk, from the log-responsibilities lw / lse an
// E-step kernel wrote for the MARGINAL mixture over the observed coordinates (exact form, with_lse = 1, fold = 0) and the table
// [mu_k,O | mu_k,M | A_k^T] per component, A_k = Sigma_k,MO Sigma_k,OO^-1 (host::condition). Per row, on every tier, in this order:
//   1. z_c = x_c - mu_k,O[c]                                   one subtraction, first;
//   2. t_j = mu_k,M[j], then t_j = fma(A_k[j][c], z_c, t_j)    for c = 0 .. dO-1 ascending;
//   3. r_k = exp_nonpos(lw_k - lse)                            the responsibility em_resp_kernel (em_post.hip) forms from the same block;
//   4. y_j = +0.0, then y_j = fma(r_k, t_j, y_j)               for k = 0 .. K-1 ascending, ONLY where r_k != 0.
// A component with r_k == 0 leaves y_j as it is -- by the definition of step 4, not by arithmetic (fma(+0, t, y) would turn a y of
// -0.0 into +0.0 for t > 0 and an overflowed t into NaN) --, so row i's output is a pure function of row i and the parameters: the
// grid, the chunk, the row's place in the block and the shard it sits on change no bit, and both tiers give the same bits.
// The skip: a wave passes over component k when r_k == 0 in all of its 64 lanes (padding lanes count as 0). Every one of those rows
// would have kept its y_j by step 4, and t_j is not carried from one component to the next, so nothing the skipped work computes
// reaches an output: no bit changes. On a separated mixture most of K = 64 components go that way. skip = 0 runs them all.
//
//   em_condition_kernel<PO, PM, W>  dO, dM <= 32, lane = row: x_O (PO registers), t and y (PM each; the rows dM .. PM-1 read the
//                                   record's padding and are never stored) in VGPRs. The chain runs in groups of four coordinates; a
//                                   coordinate c >= dO inside the last group has x_c = mu_c = +0.0 and maps of -0.0 (the runtime
//                                   pads the record so), and fma(-0.0, +0.0, t) = t + (-0.0) = t for EVERY t, -0.0 included: the
//                                   padding is an identity bit for bit, not a term. k is wave-uniform, the record's offsets are
//                                   compile-time: mu and A reach the fma as scalar operands through the scalar cache (the feed of
//                                   em_tied.hip's winv). The wave's 64 x dM tile goes through LDS (odd row stride) and out as
//                                   contiguous 16 bytes per lane.
//   em_condition_plain_kernel       any dO + dM <= 4096: thread = row, the output row is the accumulator, table from global memory.
// Record: [mu_O (PO) | mu_M (PM) | A^T (PO x PM: row c = observed coordinate c, so the PM maps of one z_c are contiguous)]; padding
// +0.0, except the rows c >= dO of A^T: -0.0.
#include "em_condition_common.hpp"
#include "exp_nonpos.hpp"

namespace mlhip {
namespace {

constexpr int kConditionMaxRegisters = 32;       // dO and dM up to which the register tier exists

template <int PO, int PM, int W>
__global__ __launch_bounds__(64 * W) void em_condition_kernel(const double* __restrict__ xt, size_t ldx, uint32_t n, int dO, int dM, int K,
                                                              const double* __restrict__ lw, size_t ldr, const double* __restrict__ lse,
                                                              const double* __restrict__ table, double* __restrict__ out, int skip)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    constexpr int PS = PO + PM + PO * PM;
    const int S = dM | 1;                                        // LDS row stride of the staging tile
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double* stage = sm + (size_t)wave * 64 * S;

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

        for (int k = 0; k < K; ++k) {
            const double r = live ? exp_nonpos(lw[(size_t)k * ldr + i] - l) : 0.0;
            const bool share = r != 0.0;                         // (a NaN has one: it reaches the output)
            if (skip && __ballot(share) == 0) continue;
            const double* __restrict__ rec = table + (size_t)k * PS;   // wave-uniform -> scalar loads
            double tj[PM];
            // Steps 1 - 2 and the tile store below are written out here, not taken from em_condition_common.hpp (component_prediction,
            // move_staged<false>, which state the same text for the other kernels): either call moves this kernel's instructions, and
            // with the calls the 16 x 16 padding ran up to 3.5 % slower at unchanged register counts
            // (profiles/condition_shared_timing.txt). As written, this file compiles to the instructions it had before the header.
#pragma unroll
            for (int j = 0; j < PM; ++j) tj[j] = rec[PO + j];
#pragma unroll
            for (int c0 = 0; c0 < PO; c0 += 4) {
                if (c0 < dO) {                                   // (wave-uniform: a group of four coordinates beyond dO is not run at all)
#pragma unroll
                    for (int c = c0; c < c0 + 4; ++c) {
                        const double z = x[c] - rec[c];
#pragma unroll
                        for (int j = 0; j < PM; ++j) tj[j] = __builtin_fma(rec[PO + PM + c * PM + j], z, tj[j]);
                    }
                }
            }
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

        // the tile is rows * dM contiguous doubles of the output: two per lane and trip, (row, col) carried along without a division
        const uint32_t rows = n - t * 64 < 64 ? n - t * 64 : 64;
        const uint32_t total = rows * (uint32_t)dM;
        double* dst = out + (size_t)t * 64 * (size_t)dM;
        const uint32_t step_rows = 128u / (uint32_t)dM, step_cols = 128u % (uint32_t)dM;
        uint32_t row = (2u * lane) / (uint32_t)dM, col = (2u * lane) % (uint32_t)dM;
        for (uint32_t e = 2u * lane; e < total; e += 128u) {
            const double v0 = stage[row * S + col];
            uint32_t row1 = row, col1 = col + 1;
            if (col1 == (uint32_t)dM) { col1 = 0; ++row1; }
            if (e + 1 < total) {
                const double v1 = stage[row1 * S + col1];
                *reinterpret_cast<double2*>(dst + e) = make_double2(v0, v1);
            } else {
                dst[e] = v0;
            }
            row += step_rows;
            col += step_cols;
            if (col >= (uint32_t)dM) { col -= (uint32_t)dM; ++row; }
        }
        wave_sync();                                             // (the next tile's stores wait for these reads)
    }
}

__global__ __launch_bounds__(256) void em_condition_plain_kernel(const double* __restrict__ xt, size_t ldx, uint32_t n, int dO, int dM, int K,
                                                                 const double* __restrict__ lw, size_t ldr, const double* __restrict__ lse,
                                                                 const double* __restrict__ table, double* __restrict__ out)
{
    const size_t PS = (size_t)dO + dM + (size_t)dO * dM;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const double l = lse[i];
        double* y = out + (size_t)i * dM;
        for (int j = 0; j < dM; ++j) y[j] = 0.0;
        for (int k = 0; k < K; ++k) {
            const double r = exp_nonpos(lw[(size_t)k * ldr + i] - l);
            if (!(r != 0.0)) continue;
            const double* rec = table + (size_t)k * PS;
            const double* mu_m = rec + dO;
            const double* at = rec + dO + dM;
            for (int j = 0; j < dM; ++j) {
                double tj = mu_m[j];
                for (int c = 0; c < dO; ++c) tj = __builtin_fma(at[(size_t)c * dM + j], xt[(size_t)c * ldx + i] - rec[c], tj);
                y[j] = __builtin_fma(r, tj, y[j]);
            }
        }
    }
}

}  // namespace

int em_condition_route(int dO, int dM)
{
    return dO <= kConditionMaxRegisters && dM <= kConditionMaxRegisters ? kConditionRegisters : kConditionPlain;
}

int condition_pad(int kernel, int n)
{
    if (kernel != kConditionRegisters) return n;
    return n <= 4 ? 4 : n <= 8 ? 8 : n <= 16 ? 16 : n <= kConditionMaxRegisters ? 32 : -1;
}

int launch_em_condition(const ConditionArgs& a, int num_cus, hipStream_t stream)
{
    if (a.dO < 1 || a.dM < 1 || a.dO + a.dM > kGenericMaxDim || a.K < 1) return -1;
    if (a.n == 0) return 0;
    if (a.kernel == kConditionPlain) {
        const uint32_t grid = row_grid(a.n, num_cus);
        hipLaunchKernelGGL(em_condition_plain_kernel, dim3(grid), dim3(256), 0, stream, a.xt, a.ldx, a.n, a.dO, a.dM, a.K, a.lw, a.ldr, a.lse,
                           a.table, a.out);
        return (int)grid;
    }
    return dispatch_paddings<32>(a.dO, a.dM, [&](auto po, auto pm) {
        constexpr int PO = decltype(po)::value, PM = decltype(pm)::value, W = condition_waves(PM);
        const uint32_t grid = tile_grid(a.n, W, num_cus);
        const size_t bytes = sizeof(double) * (size_t)W * 64 * (size_t)(a.dM | 1);
        hipLaunchKernelGGL((em_condition_kernel<PO, PM, W>), dim3(grid), dim3(64 * W), bytes, stream, a.xt, a.ldx, a.n, a.dO, a.dM, a.K, a.lw,
                           a.ldr, a.lse, a.table, a.out, a.skip);
        return (int)grid;
    });
}

}  // namespace mlhip
