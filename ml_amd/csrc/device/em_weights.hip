// Row weights of a resident block (mlhip_data_set_weights): the passes a weighted fit adds next to the unweighted kernels, which stay
// as they are. Frequency weights w_i >= 0 enter an EM iteration in two places:
//   * the log-likelihood  sum_i w_i lse_i          -- weighted_ll_kernel after an LSE-writing E-step, weighted_lse_finish_kernel after
//     the self-normalising statistics pass; partials in the layout em_reduce_kernel reads;
//   * the statistics      sum_i w_i r_ik Phi_i     -- where the wide kernel normalises the log-responsibilities itself (d = 12 .. 128,
//     K <= 64) it multiplies by w_i while staging (em_mstats_wide.hip, EXP = 3); elsewhere weighted_resp_kernel writes the plain
//     responsibilities w_i r_ik, which every statistics tier takes in mode kFromResp. ONE rounding more than r_ik either way.
// Responsibilities, labels and lse stay per-row quantities: nothing here writes lw or lse.
// The kernels here are grid-stride passes over N-vectors (and the N x K block) with coalesced loads, per-workgroup partials combined
// by a fixed-order tree and no atomics: the sums are reproducible run to run and, for a given n, from pass to pass. The file is a code
// object of its own: an unweighted fit never loads it.
#include "device.hpp"
#include "exp_nonpos.hpp"

namespace mlhip {
namespace {

/// Sum of the workgroup's 256 values, the tree of em_lse_finish_kernel; valid in thread 0.
__device__ __forceinline__ double block_tree_sum(double v, double* red)
{
    red[threadIdx.x] = v;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(256) void weights_attach_kernel(double* __restrict__ w, uint32_t n, uint32_t n_pad,
                                                              double* __restrict__ sum_partials, double* __restrict__ bad_partials)
{
    __shared__ double red[256];
    double sum = 0.0, bad = 0.0;
    for (uint64_t i = blockIdx.x * 256u + threadIdx.x; i < n_pad; i += (uint64_t)gridDim.x * 256u) {
        if (i >= n) { w[i] = 0.0; continue; }                       // padding rows carry no weight
        const double v = w[i];
        const bool ok = v >= 0.0 && v <= 1.7976931348623157e308;    // finite and not negative (false for a NaN)
        sum += ok ? v : 0.0;
        bad += ok ? 0.0 : 1.0;
    }
    const double s = block_tree_sum(sum, red);
    if (threadIdx.x == 0) sum_partials[blockIdx.x] = s;
    __syncthreads();
    const double b = block_tree_sum(bad, red);
    if (threadIdx.x == 0) bad_partials[blockIdx.x] = b;
}

__global__ __launch_bounds__(256) void weighted_ll_kernel(const double* __restrict__ w, const double* __restrict__ lse, uint32_t n,
                                                           double* __restrict__ ll_partials)
{
    __shared__ double red[256];
    double acc = 0.0;
    for (uint64_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) {
        const double wi = w[i];
        if (wi != 0.0) acc += wi * lse[i];                          // a row of weight 0 is not in the sample, whatever its density
    }
    const double s = block_tree_sum(acc, red);
    if (threadIdx.x == 0) ll_partials[blockIdx.x] = s;
}

/// em_lse_finish_kernel for a weighted block: lse[i] = max + log(esum) in place (the sample's own lse), one partial of w_i lse_i
/// per workgroup.
__global__ __launch_bounds__(256) void weighted_lse_finish_kernel(double* __restrict__ lse, const double* __restrict__ esum,
                                                                   const double* __restrict__ w, uint32_t n, double* __restrict__ ll_partials)
{
    __shared__ double red[256];
    double acc = 0.0;
    for (uint64_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) {
        const double l = lse[i] + log(esum[i]);
        lse[i] = l;
        const double wi = w[i];
        if (wi != 0.0) acc += wi * l;
    }
    const double s = block_tree_sum(acc, red);
    if (threadIdx.x == 0) ll_partials[blockIdx.x] = s;
}

template <bool EXP>
__global__ __launch_bounds__(256) void weighted_resp_kernel(const double* __restrict__ src, size_t lds, const double* __restrict__ lse,
                                                             const double* __restrict__ w, uint32_t n, uint32_t n_pad, int K,
                                                             double* __restrict__ out, size_t ldo)
{
    for (uint64_t i = blockIdx.x * 256u + threadIdx.x; i < n_pad; i += (uint64_t)gridDim.x * 256u) {
        const double wi = i < n ? w[i] : 0.0;
        const double l = (EXP && wi != 0.0) ? lse[i] : 0.0;
        for (int k = 0; k < K; ++k) {
            double r = 0.0;
            if (wi != 0.0) {
                r = src[(size_t)k * lds + i];
                if (EXP) r = exp_nonpos(r - l);                     // the statistics kernels' own r = exp(lw - lse)
                r *= wi;
            }
            out[(size_t)k * ldo + i] = r;
        }
    }
}

int pass_grid(uint32_t rows, uint32_t cap)
{
    uint32_t blocks = (rows + 255u) / 256u;
    if (blocks > cap) blocks = cap;
    return blocks ? (int)blocks : 1;
}

}  // namespace

int weights_grid(uint32_t n) { return pass_grid(n, 1024u); }

int launch_weights_attach(double* w, uint32_t n, uint32_t n_pad, double* sum_partials, double* bad_partials, hipStream_t stream)
{
    const int grid = weights_grid(n);
    hipLaunchKernelGGL(weights_attach_kernel, dim3(grid), dim3(256), 0, stream, w, n, n_pad, sum_partials, bad_partials);
    return grid;
}

int launch_weighted_ll(const double* w, const double* lse, uint32_t n, double* ll_partials, hipStream_t stream)
{
    const int grid = weights_grid(n);
    hipLaunchKernelGGL(weighted_ll_kernel, dim3(grid), dim3(256), 0, stream, w, lse, n, ll_partials);
    return grid;
}

void launch_weighted_lse_finish(double* lse, const double* esum, const double* w, uint32_t n, int n_ll, double* ll_partials, hipStream_t stream)
{
    hipLaunchKernelGGL(weighted_lse_finish_kernel, dim3(n_ll), dim3(256), 0, stream, lse, esum, w, n, ll_partials);
}

void launch_weighted_resp(const double* src, size_t lds, const double* lse, int mode, const double* w, uint32_t n, uint32_t n_pad, int K,
                          double* out, size_t ldo, hipStream_t stream)
{
    const int grid = pass_grid(n_pad, 8192u);
    if (mode == kFromResp)
        hipLaunchKernelGGL(weighted_resp_kernel<false>, dim3(grid), dim3(256), 0, stream, src, lds, lse, w, n, n_pad, K, out, ldo);
    else
        hipLaunchKernelGGL(weighted_resp_kernel<true>, dim3(grid), dim3(256), 0, stream, src, lds, lse, w, n, n_pad, K, out, ldo);
}

}  // namespace mlhip
