// Restarts of a short full-covariance EM fit, batched: R independent loops on one resident block (mlhip_em_iterate_restarts) share
// the three dispatches of an iteration. A small fit -- the reference's own benchmark regime, N = 100 .. 100 000, d = 2 .. 6, a few
// components -- leaves most of the chip idle and is bound by its dependent launches, not by arithmetic; M
// restarts of it are M copies of the same tiny pass, so they ride in the second grid dimension of
//   1. the PASS        grid (g, M): workgroup (x, m) is workgroup x of g of the solo vector-unit kernel (em_fused_small.hip
//                      em_fused_valu_kernel) on restart m's records, and writes restart m's partial blocks;
//   2. the REDUCTION   grid (blocks, M): em_reduce_kernel's sums of restart m's partial blocks;
//   3. the CLOSING     grid (K, M): em_close_kernel's arithmetic on restart m's statistics, its info block straight into pinned memory.
// Each runs the TEXT the solo launch runs (valu_pass, em_reduce_body, close_component) on the same grid g, so every restart's
// numbers are bit for bit those of mlhip_em_iterate from the same start. No workgroup waits for another, nothing spins, no atomics:
// the stream orders the three launches. Row y of a launch serves restart alive.index[y] -- the host drops a restart from the list
// when it has converged, run out of steps or raised a refinement flag (runtime/em_restarts.cpp).
#include "em_close_body.hpp"
#include "em_fused_valu_body.hpp"
#include "em_reduce_body.hpp"
#include "parts.hpp"

namespace mlhip {
namespace mstats {
namespace {

/// (x, m): the solo pass of workgroup x of gridDim.x on the records of restart alive.index[m]. The record pointer is formed from
/// kernel arguments and the workgroup's row alone -- wave-uniform, so the records come through scalar loads as in the solo kernel.
template <int D, int K>
__global__ __launch_bounds__(256) void em_restarts_pass_kernel(
    const double* __restrict__ xt, size_t ldx, uint32_t n, const double* __restrict__ shift, const double* __restrict__ records,
    size_t records_stride, double* __restrict__ partials, size_t partials_stride, int KP, int FP, double* __restrict__ ll_partials,
    size_t ll_stride, RestartsAlive alive)
{
    __shared__ double fold[4][ValuShape<D, K>::VP];
    __shared__ double red[4];
    const size_t m = alive.index[blockIdx.y];
    // (no lse is written: whoever needs a restart's lse rebuilds it with the log-responsibilities, as after the resident loop)
    valu_pass<D, K>(xt, ldx, n, shift, records + m * records_stride, nullptr, partials + m * partials_stride + (size_t)blockIdx.x * KP * FP,
                    FP, ll_partials + m * ll_stride + blockIdx.x, blockIdx.x, gridDim.x, fold, red);
}

__global__ __launch_bounds__(256) void em_restarts_reduce_kernel(const double* __restrict__ partials, size_t partials_stride, int n_blocks,
                                                                  int KP, int FP, int K, int F, const double* __restrict__ ll_partials,
                                                                  size_t ll_stride, double* __restrict__ stats, size_t stats_stride,
                                                                  RestartsAlive alive)
{
    __shared__ double red[256];
    const size_t m = alive.index[blockIdx.y];
    em_reduce_body(partials + m * partials_stride, n_blocks, KP, FP, K, F, ll_partials + m * ll_stride, n_blocks, stats + m * stats_stride,
                   (int)blockIdx.x, red);
}

#pragma clang fp contract(off)     // the host's closing arithmetic, statement by statement (em_close.hip)

template <int D>
__global__ __launch_bounds__(closing::NT) void em_restarts_close_kernel(
    const double* __restrict__ stats, size_t stats_stride, int K, const double* __restrict__ shift, double n_global, double ridge,
    double refine_limit, double* __restrict__ mixing, double* __restrict__ means, double* __restrict__ covs, size_t pack_stride,
    double* __restrict__ records, size_t records_stride, double* __restrict__ info, size_t info_stride, RestartsAlive alive)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    constexpr int PS = D + D * (D + 1) / 2 + 1;        // estep_param_stride(D)
    const size_t m = alive.index[blockIdx.y];
    closing::close_component<0, D>(stats + m * stats_stride, K, D, D, shift, n_global, ridge, refine_limit, mixing + m * pack_stride,
                                   means + m * pack_stride, covs + m * pack_stride, records + m * records_stride, PS,
                                   info + m * info_stride, (int)blockIdx.x, (int)threadIdx.x, sm);
}

template <int D, int K> bool pass_k(const RestartsArgs& a, hipStream_t stream)
{
    if constexpr (K >= 1) {
        if (a.K == K) {
            hipLaunchKernelGGL((em_restarts_pass_kernel<D, K>), dim3(a.grid, a.alive.count), dim3(256), 0, stream, a.xt, a.ldx, a.n, a.shift,
                               a.records_in, a.records_stride, a.partials, a.partials_stride, em_fused_partial_rows(a.K),
                               em_fused_partial_cols(a.d), a.ll_partials, a.ll_stride, a.alive);
            return true;
        }
        return pass_k<D, K - 1>(a, stream);
    }
    return false;
}

bool launchable(const RestartsArgs& a, int D)
{
    return a.d == D && a.K >= 1 && a.K <= valu_max_k(D) && a.grid >= 1 && a.alive.count >= 1 && a.alive.count <= kRestartsMaxBatch;
}

}  // namespace

// ---- compiled in five parts by dimension (parts.hpp): part 1 .. 5 = d 1, 2, 3, 4, 6
constexpr int kPartDim = MLHIP_PART <= 4 ? MLHIP_PART : 6;

bool MLHIP_PART_FN(launch_em_restarts_pass)(const RestartsArgs& a, hipStream_t stream)
{
    constexpr int D = kPartDim;
    return launchable(a, D) && pass_k<D, valu_max_k(D)>(a, stream);
}

bool MLHIP_PART_FN(launch_em_restarts_reduce)(const RestartsArgs& a, hipStream_t stream)
{
    if (!launchable(a, kPartDim)) return false;
    const int F = stats_count(a.d);
    const int red_blocks = (a.K * F + kRedOut - 1) / kRedOut + 1;
    hipLaunchKernelGGL(em_restarts_reduce_kernel, dim3(red_blocks, a.alive.count), dim3(256), 0, stream, a.partials, a.partials_stride, a.grid,
                       em_fused_partial_rows(a.K), em_fused_partial_cols(a.d), a.K, F, a.ll_partials, a.ll_stride, a.stats, a.stats_stride,
                       a.alive);
    return true;
}

bool MLHIP_PART_FN(launch_em_restarts_close)(const RestartsArgs& a, hipStream_t stream)
{
    constexpr int D = kPartDim;
    if (!launchable(a, D)) return false;
    hipLaunchKernelGGL((em_restarts_close_kernel<D>), dim3(a.K, a.alive.count), dim3(closing::NT), sizeof(double) * closing::scratch_doubles(D),
                       stream, a.stats, a.stats_stride, a.K, a.shift, a.n_global, a.ridge, a.refine_limit, a.mixing, a.means, a.covs,
                       a.pack_stride, a.records_out, a.records_stride, a.info, a.info_stride, a.alive);
    return true;
}

#if MLHIP_PART == 1
#define MLHIP_RESTARTS_PARTS(entry)                                                                              \
    bool entry##_part2(const RestartsArgs&, hipStream_t); bool entry##_part3(const RestartsArgs&, hipStream_t);  \
    bool entry##_part4(const RestartsArgs&, hipStream_t); bool entry##_part5(const RestartsArgs&, hipStream_t);  \
    bool entry(const RestartsArgs& a, hipStream_t stream)                                                        \
    {                                                                                                            \
        switch (a.d) {                                                                                           \
        case 1: return entry##_part1(a, stream);                                                                 \
        case 2: return entry##_part2(a, stream);                                                                 \
        case 3: return entry##_part3(a, stream);                                                                 \
        case 4: return entry##_part4(a, stream);                                                                 \
        case 6: return entry##_part5(a, stream);                                                                 \
        default: return false;                                                                                   \
        }                                                                                                        \
    }
MLHIP_RESTARTS_PARTS(launch_em_restarts_pass)
MLHIP_RESTARTS_PARTS(launch_em_restarts_reduce)
MLHIP_RESTARTS_PARTS(launch_em_restarts_close)
#undef MLHIP_RESTARTS_PARTS
#endif

}  // namespace mstats
}  // namespace mlhip
