// Scoring pass of a Gaussian mixture for gfx950: per sample the log-sum-exp  lse_i = log sum_k exp(lw_ik)  and the label
// argmax_k lw_ik (first maximum wins) under caller-given parameters -- the batch form of EM::assign_responsibilities (reference
// ML/EM.cpp:176-188) in the log domain. Nothing else is written: 8 + 4 bytes per sample, no N x K block.
//
//   em_score_kernel<D>      d <= 32, the scalar-fed tier: the arithmetic of em_estep_kernel<D> (em_estep.hip) -- lane = sample,
//                           coordinates in VGPRs, records (mean, W = L^-1 packed, coef) through scalar loads, z = x - mu,
//                           y = W z, q = |y|^2, lw = fma(-0.5, q, coef), the same online log-sum-exp -- without the lw store.
//                           The running maximum of the log-sum-exp IS the running best lw (both move on the strict lw > m), so
//                           the label costs one select per component.
//   em_score_finish_kernel  the composed route: label and lse of a row chunk from the lw / lse an E-step kernel left in scratch.
//
// A row whose lse is NaN (a NaN parameter) has no maximum among its log-responsibilities lw - lse: label 0xffffffff, what
// em_resp_kernel (em_post.hip) leaves for it.
#include "device.hpp"
#include "exp_nonpos.hpp"

namespace mlhip {
namespace {

constexpr uint32_t kNoLabel = 0xffffffffu;   // ML/EM.cpp:294 starts from label -1

template <int D>
__global__ __launch_bounds__(256) void em_score_kernel(const double* __restrict__ xt, size_t ldx, uint32_t n_pad,
                                                        const double* __restrict__ params, int K,
                                                        double* __restrict__ lse_out, uint32_t* __restrict__ labels_out)
{
    constexpr int PS = D + D * (D + 1) / 2 + 1;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n_pad; i += gridDim.x * 256u) {
        double x[D];
#pragma unroll
        for (int j = 0; j < D; ++j) x[j] = xt[(size_t)j * ldx + i];

        double m = -__builtin_inf(), s = 0.0;
        uint32_t arg = kNoLabel;
        for (int k = 0; k < K; ++k) {
            const double* __restrict__ p = params + (size_t)k * PS;   // wave-uniform -> scalar loads
            double z[D];
#pragma unroll
            for (int j = 0; j < D; ++j) z[j] = x[j] - p[j];
            const double* __restrict__ w = p + D;
            double q = 0.0;
#pragma unroll
            for (int j = 0; j < D; ++j) {
                double y = w[j * (j + 1) / 2] * z[0];
#pragma unroll
                for (int l = 1; l <= j; ++l) y = __builtin_fma(w[j * (j + 1) / 2 + l], z[l], y);
                q = __builtin_fma(y, y, q);
                // Keeps the scalar loads of later rows from being hoisted (and spilled) above this point.
                if ((j & 3) == 3) __builtin_amdgcn_sched_barrier(0);
            }
            const double lw = __builtin_fma(-0.5, q, p[PS - 1]);
            // online log-sum-exp with a single exp per component, as em_estep_kernel: a component of mixing weight 0 has
            // lw = -inf and adds exp(-inf) = 0 (never the label: -inf > m is false); a genuinely NaN lw stays a NaN
            const double e = exp_nonpos(lw == -HUGE_VAL ? -HUGE_VAL : -fabs(lw - m));
            const bool up = lw > m;
            s = up ? __builtin_fma(s, e, 1.0) : s + e;
            m = up ? lw : m;
            arg = up ? (uint32_t)k : arg;
        }
        const double lse = m + log(s);
        if (lse_out) lse_out[i] = lse;
        if (labels_out) labels_out[i] = lse != lse ? kNoLabel : arg;
    }
}

__global__ __launch_bounds__(256) void em_score_finish_kernel(const double* __restrict__ lw, size_t ldr,
                                                               const double* __restrict__ lse, uint32_t n, int K,
                                                               double* __restrict__ lse_out, uint32_t* __restrict__ labels_out)
{
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const double l = lse[i];
        if (lse_out) lse_out[i] = l;
        if (labels_out) {
            double best = -__builtin_inf();
            uint32_t arg = kNoLabel;
            for (int k = 0; k < K; ++k) {
                const double v = lw[(size_t)k * ldr + i];
                const bool up = v > best;
                best = up ? v : best;
                arg = up ? (uint32_t)k : arg;
            }
            labels_out[i] = l != l ? kNoLabel : arg;
        }
    }
}

template <int D>
int launch_t(const ScoreArgs& a, hipStream_t stream)
{
    const uint32_t n_pad = padded_samples(a.n);
    uint32_t grid = n_pad / 256;
    if (grid > 2048u) grid = 2048u;               // (em_estep.hip's bound: the grid-stride loop takes the rest)
    hipLaunchKernelGGL(em_score_kernel<D>, dim3(grid), dim3(256), 0, stream, a.xt, a.ldx, n_pad, a.params, a.K, a.lse, a.labels);
    return (int)grid;
}

}  // namespace

int launch_em_score(const ScoreArgs& a, hipStream_t stream)
{
    switch (a.D) {
    case 1: return launch_t<1>(a, stream);
    case 2: return launch_t<2>(a, stream);
    case 3: return launch_t<3>(a, stream);
    case 4: return launch_t<4>(a, stream);
    case 6: return launch_t<6>(a, stream);
    case 8: return launch_t<8>(a, stream);
    case 12: return launch_t<12>(a, stream);
    case 16: return launch_t<16>(a, stream);
    case 20: return launch_t<20>(a, stream);
    case 24: return launch_t<24>(a, stream);
    case 28: return launch_t<28>(a, stream);
    case 32: return launch_t<32>(a, stream);
    default: return -1;
    }
}

void launch_em_score_finish(const double* lw, size_t ldr, const double* lse, uint32_t n, int K, double* lse_out, uint32_t* labels_out,
                            hipStream_t stream)
{
    uint32_t blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    if (blocks == 0) blocks = 1;
    hipLaunchKernelGGL(em_score_finish_kernel, dim3(blocks), dim3(256), 0, stream, lw, ldr, lse, n, K, lse_out, labels_out);
}

}  // namespace mlhip
