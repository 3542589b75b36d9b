// One EM iteration's device work for a TIED covariance -- K means, ONE Sigma = L L^T shared by every component -- in ONE kernel
// (d <= 32, K <= 64): E-step + the M-step statistics that depend on the responsibilities, X read once, only the per-sample
// log-sum-exp written. EXTENSION: the reference's ml::EM is full-covariance only (ML/EM.hpp:175); this is the pair of loops of
// EM::expectation_step (ML/EM.cpp:190-219) and the sums of EM::maximisation_step (:229-250) for K components that all carry Sigma.
// Arithmetic per sample, with x~ = x - shift:
//     y = L^-1 x~                                    (ONCE per sample, ascending-j fma chains; the full path whitens once per component)
// per (sample, component), from the record [m_k (D) | c_k], m_k = L^-1 (mu_k - shift), c_k = log pi_k - sum_j log L_jj:
//     z_j = y_j - m_kj ;  q = sum_j z_j z_j  (mean subtracted first, ascending-j fma chain) ;  lw = c_k - q/2
// then m = max_k lw, e_k = exp(lw_k - m), s = sum e_k, lse = m + log s, r_k = e_k / s, and per component
//     S0 = sum_i r,  S1_j = sum_i r x~_j                 (d + 1 numbers per component: the second moments of the whole sample,
//                                                         T = sum_i x~ x~^T, do not depend on r and are formed once per block)
//
// Mapping (the structure of em_diag.hip's em_diag_kernel): a wave owns a stream of 64-sample tiles, lane = sample. The shifted
// coordinates go to the wave's private LDS tile straight after the load -- they are the statistics GEMM's B operand -- and are then
// whitened IN PLACE in their registers (row i of L^-1 needs x~_0 .. x~_i only: descending i). The D (D + 1) / 2 entries of L^-1
// are wave-uniform and read through the scalar data cache at compile-time offsets (the feed of em_estep.hip's records: one scalar
// operand per v_fma_f64 is what the constant bus allows, and the LDS pipe stays free for the tile stores that run beside it; as LDS
// broadcasts the 528 operands of d = 32 cost one LDS read per fma). The component records are staged once per workgroup in LDS and
// read as broadcasts through ONE opaque base register (em_diag_kernel's feed: 2 VALU operations per operand, K D operands per
// tile). r then goes through the wave's LDS tile into ONE GEMM on the fp64 matrix cores,
//     stats[K x d] += R^T[K x 64] * X~[64 x d]          (v_mfma_f64_16x16x4),
// S0 is a per-lane running sum folded once at the end. No atomics; per-workgroup partials are combined in fixed order by
// em_reduce_kernel: the result is bitwise reproducible for a given grid.
#include <cstdlib>
#include "parts.hpp"

#include "em_tile_common.hpp"

namespace mlhip {
namespace mstats {
namespace {

/// RBT = 16-component row blocks that exist (K <= 16 RBT), RBW = row blocks this workgroup accumulates (blockIdx.y picks the
/// group; every group evaluates all K densities -- the normalisation needs them), CB = 16-column blocks of the d features.
template <int D, int RBT, int RBW, int CB>
__global__ __launch_bounds__(256, (D <= 16 && RBT <= 2) ? 2 : 1) void em_tied_kernel(
    const double* __restrict__ xt, size_t ldx, uint32_t n, int d, const double* __restrict__ shift,
    const double* __restrict__ winv, const double* __restrict__ params, int K, double* __restrict__ lse_out,
    double* __restrict__ partials, int KP, int FP, double* __restrict__ ll_partials)
{
    constexpr int PS = tied_param_stride_c(D);
    constexpr int KMAX = 16 * RBT;
    constexpr int JC = D % 2 == 0 ? 2 : 1;                    // dimensions per operand batch of the density loop
    constexpr int XSS = xsd<D>();
    extern __shared__ __attribute__((aligned(16))) double smem[];
    __shared__ double red[4];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    double* Xw = smem + (size_t)wave * (TS * XSS + TS * RSS);
    double* Rw = Xw + TS * XSS;
    double* recs = smem + 4 * (TS * XSS + TS * RSS);          // [KMAX][PS]: records beyond K are neutral (m = 0, c = -inf)
    constexpr int ONE = D, ZERO = D + 1;                      // LDS row: [x~_0 .. x~_(D-1) | 1 | 0]
    const int rb0 = blockIdx.y * RBW;                         // first row block accumulated here
    for (int e = tid; e < KMAX * PS; e += 256) recs[e] = params[e];
    __syncthreads();

    // feature f of the GEMM: f < d -> x~_f ; beyond -> the zero slot
    int off[CB];
#pragma unroll
    for (int c = 0; c < CB; ++c) {
        const int f = c * 16 + (lane & 15);
        off[c] = f < d ? f : ZERO;
    }

    d4 acc[RBW][CB];
    double s0[RBW];                                           // lane (g, c): partial S0 of component c of each row block
#pragma unroll
    for (int r = 0; r < RBW; ++r) {
        s0[r] = 0.0;
#pragma unroll
        for (int c = 0; c < CB; ++c) acc[r][c] = d4{0.0, 0.0, 0.0, 0.0};
    }

    const uint32_t n_tiles = (n + TS - 1) / TS;
    const uint32_t stride = gridDim.x * 4;
    const double* xbase = Xw + 16 * (lane >> 4) * XSS;
    const double* rbase = Rw + 16 * (lane >> 4) * RSS + (lane & 15);
    double ll_acc = 0.0;

    for (uint32_t tile = blockIdx.x * 4 + wave; tile < n_tiles; tile += stride) {
        // Loop-invariant values kept where em_diag_kernel keeps them: K in a scalar register (the guards below become scalar
        // compares) and the record base in ONE VGPR, so that every operand read is `ds_read base offset:imm`.
        asm volatile("" ::: "memory");
        int Kt = K;
        asm volatile("" : "+s"(Kt));
        lds_cdouble* recv = (lds_cdouble*)recs;
        asm volatile("" : "+v"(recv));
        const uint32_t i0 = tile * TS + lane;                 // (< n_pad: n_pad is a multiple of 256)
        double y[D];
#pragma unroll
        for (int j = 0; j < D; ++j) y[j] = xt[(size_t)j * ldx + i0];
#pragma unroll
        for (int j = 0; j < D; ++j) y[j] -= shift[j];          // shift is zero-padded to D entries

        // ---- 0. x~ -> the wave's LDS tile (B operand of the statistics GEMM; the previous tile's matrix phase has read its own)
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int j = 0; j < D; ++j) Xw[lane * XSS + j] = y[j];
        Xw[lane * XSS + ONE] = 1.0;
        Xw[lane * XSS + ZERO] = 0.0;

        // ---- 1. whitening, once per sample: y_i = sum_(j <= i) W_ij x~_j, ascending j, in place (descending i)
#pragma unroll
        for (int i = D - 1; i >= 0; --i) {
            const double* __restrict__ w = winv + i * (i + 1) / 2;   // (kernel argument + constant: scalar loads)
            double t = w[0] * y[0];
#pragma unroll
            for (int j = 1; j <= i; ++j) t = __builtin_fma(w[j], y[j], t);
            y[i] = t;
        }

        // ---- 2. log-densities of all K components (statically unrolled; wave-uniform guards per group of 4)
        double lwv[KMAX];
        double m = -__builtin_inf();
#pragma unroll
        for (int k4 = 0; k4 < KMAX; k4 += 4) {
            if (k4 < Kt) {
                // 4 components x JC dimensions per batch: the operands are read from LDS in one go. Every q accumulates in ascending j.
                lds_cdouble* p = recv + k4 * PS;
                double q[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) q[u] = 0.0;
#pragma unroll
                for (int j0 = 0; j0 < D; j0 += JC) {
                    double mu[4][JC];
#pragma unroll
                    for (int u = 0; u < 4; ++u)
#pragma unroll
                        for (int jj = 0; jj < JC; ++jj) mu[u][jj] = p[u * PS + j0 + jj];
#pragma unroll
                    for (int jj = 0; jj < JC; ++jj)
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            const double z = y[j0 + jj] - mu[u][jj];
                            q[u] = __builtin_fma(z, z, q[u]);
                        }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const double coef = p[u * PS + D];                               // records k >= K: coef = -inf
                    const double lw = __builtin_fma(-0.5, q[u], coef);
                    lwv[k4 + u] = lw;
                    m = lw > m ? lw : m;
                }
            } else {
#pragma unroll
                for (int u = 0; u < 4; ++u) lwv[k4 + u] = -__builtin_inf();
            }
        }
        // ---- 3. normalisation: one exp per (sample, component)
        double sum = 0.0;
#pragma unroll
        for (int k4 = 0; k4 < KMAX; k4 += 4) {
            if (k4 < Kt) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const double e = exp_nonpos(lwv[k4 + u] - m);                   // exp(-inf) = 0 for the neutral tail
                    lwv[k4 + u] = e;
                    sum += e;
                }
            } else {
#pragma unroll
                for (int u = 0; u < 4; ++u) lwv[k4 + u] = 0.0;
            }
        }
        const double lse = m + log(sum);
        const bool live = i0 < n;
        if (blockIdx.y == 0) {
            lse_out[i0] = lse;
            if (live) ll_acc += lse;
        }
        const double inv = live ? 1.0 / sum : 0.0;               // padding samples contribute nothing

        // ---- 4. responsibilities -> LDS, statistics on the matrix cores
#pragma unroll
        for (int rb = 0; rb < RBW; ++rb) {
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int it = 0; it < 16; ++it) {
                // (rb0 is uniform over the workgroup; the row-block index is resolved at compile time per group)
                double r = 0.0;
#pragma unroll
                for (int g = 0; g < RBT / RBW; ++g)
                    if (rb0 == g * RBW) r = lwv[(g * RBW + rb) * 16 + it];
                Rw[lane * RSS + it] = r * inv;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            if ((rb0 + rb) * 16 < Kt) {                          // wave-uniform: skip all-zero row blocks
                __builtin_amdgcn_s_setprio(kMatrixPhasePriority);  // see em_estep_mfma4.hip
#pragma unroll 4
                for (int sg = 0; sg < TS / 4; ++sg) {
                    const double av = rbase[sg * RSS];           // r of (sample 16 g + sg, component lane & 15)
                    const double* xr = xbase + sg * XSS;
                    s0[rb] += av;
#pragma unroll
                    for (int c = 0; c < CB; ++c)
                        acc[rb][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, xr[off[c]], acc[rb][c], 0, 0, 0);
                }
                __builtin_amdgcn_s_setprio(0);
            }
        }
    }

    // ---- epilogue: fold the 4 waves' accumulators, S0 sums and log-likelihood sums in fixed order
    // partial block of this workgroup column: [KP][FP], row = component, columns [0, d) = S1, column d = S0
    fold_waves<RBW, CB, true>(partials + (size_t)blockIdx.x * KP * FP, FP, rb0, wave, lane, acc, d, s0, d);
    // (the log-likelihood fold in this kernel's own text, not fold_log_likelihood: through the helper the register allocation of
    // <3, 2, 2, 1> grows from 162 to 172 VGPRs, one wave per SIMD less; the same holds for a shared form of the normalisation above.
    // The statistics loop is this kernel's own text too: through stats_tile d = 32, K = 40 measured 0.9 % slower, N = 1M)
    if (blockIdx.y == 0) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) ll_acc += __shfl_down(ll_acc, o, 64);
        if (lane == 0) red[wave] = ll_acc;
        __syncthreads();
        if (tid == 0) ll_partials[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
    }
}

template <int D, int RBT>
int launch_t(const TiedArgs& a, int grid, hipStream_t stream)
{
    constexpr int CB = (D + 15) / 16, RBW = rbw_of(RBT), PS = tied_param_stride_c(D), XSS = xsd<D>();
    const size_t smem = sizeof(double) * (4 * ((size_t)TS * XSS + (size_t)TS * RSS) + (size_t)16 * RBT * PS);
    hipLaunchKernelGGL((em_tied_kernel<D, RBT, RBW, CB>), dim3(grid, RBT / RBW), dim3(256), smem, stream, a.xt, a.ldx, a.n, a.d,
                       a.shift, a.winv, a.params, a.K, a.lse, a.partials, em_tied_partial_rows(a.K), em_tied_partial_cols(a.d),
                       a.ll_partials);
    return grid;
}

}  // namespace

int MLHIP_PART_FN(launch_em_tied)(const TiedArgs& a, int grid, hipStream_t stream)
{
    return dispatch_part_dim(a.d, [&](auto D) {
        return dispatch_row_blocks(a.K, [&](auto RBT) { return launch_t<decltype(D)::value, decltype(RBT)::value>(a, grid, stream); });
    });
}

#if MLHIP_PART == 1
MLHIP_DECLARE_DIM_PARTS(launch_em_tied, TiedArgs)

bool em_tied_supported(int d, int K) { return tile_shape_supported(d, K); }
int em_tied_partial_rows(int K) { return tile_partial_rows(K); }
int em_tied_partial_cols(int d) { return (d + 1 + 15) / 16 * 16; }
int em_tied_grid(int d, int K, uint32_t n, int num_cus) { return tile_grid(d, K, n, TS, num_cus, 3); }

int launch_em_tied(const TiedArgs& a, int num_cus, hipStream_t stream)
{
    if (!em_tied_supported(a.d, a.K)) return -1;
    return launch_dim_part(a, em_tied_grid(a.d, a.K, a.n, num_cus), (size_t)em_tied_partial_rows(a.K) * em_tied_partial_cols(a.d),
                           launch_em_tied_parts, stream);
}
#endif

}  // namespace mstats
}  // namespace mlhip
