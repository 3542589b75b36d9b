// Shared pieces of the kernels in which every WAVE owns a stream of 64-sample tiles and accumulates the M-step statistics on the
// fp64 matrix cores from its private LDS tiles: em_mstats_small.hip, em_fused_small.hip, em_diag.hip (both kernels), em_tied.hip.
// The density sections differ and stay in their kernels; what is here is the part they have in common, written once:
// the statistics loop, the fixed-order folds of the epilogue, the diagonal feature offsets --
// and, for the host, the shape rules of the launches (row blocks, partial rows, grid).
#pragma once
#include "em_mstats_common.hpp"
#include "exp_nonpos.hpp"

#include <type_traits>

namespace mlhip {
namespace mstats {

typedef __attribute__((address_space(3))) const double lds_cdouble;
constexpr int RSS = 17;                                      // LDS row stride of one 16-component responsibility block (odd)
template <int D> constexpr int xsd() { return (D + 2) | 1; }  // LDS row stride of a sample tile [d coords | 1 | 0], odd (em_diag, em_tied)

/// Statistics of one 64-sample tile on the matrix cores: over the 16 sample groups sg, acc[c] += r^T (B operand of column block c).
/// rbase: the lane's view of the responsibility tile -- r of (sample 16 (lane >> 4) + sg, component lane & 15) at rbase[sg * RSS];
/// bop(sg, c): the B operand, formed by the caller (one LDS read, or the product of two); S0: *s0 += r as well (the lane's partial
/// sum of responsibilities). UNROLL: sample groups per loop body. The responsibilities and the sample tile must be visible to the wave
/// (wave barrier, release fence, wave barrier after the stores); s_setprio around the loop is the caller's.
template <int CB, int UNROLL, bool S0, typename R, typename B>
__device__ __forceinline__ void stats_tile(R rbase, B bop, d4 (&acc)[CB], double* s0)
{
#pragma unroll UNROLL
    for (int sg = 0; sg < TS / 4; ++sg) {
        const double av = rbase[sg * RSS];
        if constexpr (S0) *s0 += av;
#pragma unroll
        for (int c = 0; c < CB; ++c) acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bop(sg, c), acc[c], 0, 0, 0);
    }
}

/// Epilogue: the four waves fold their accumulators into the workgroup's partial block out[KP][FP] one after the other -- every output
/// is (((0 + w0) + w1) + w2) + w3, bit-reproducible. C/D layout of v_mfma_f64_16x16x4: col = lane & 15, row = (lane >> 4) + 4 * reg.
/// rb0: first 16-component row block of this workgroup; columns f >= fcols are not written. S0: s0[r] holds the lane's partial sum of
/// responsibilities of row block r; summed over the wave's lane groups it goes to column s0col.
template <int RBW, int CB, bool S0>
__device__ __forceinline__ void fold_waves(double* out, int FP, int rb0, int wave, int lane, const d4 (&acc)[RBW][CB], int fcols,
                                           double* s0, int s0col)
{
    if constexpr (S0) {
#pragma unroll
        for (int r = 0; r < RBW; ++r) {
            double v = s0[r];
            v += __shfl_xor(v, 16, 64);
            v += __shfl_xor(v, 32, 64);
            s0[r] = v;                                           // every lane (g, c): S0 of component c over the wave's samples
        }
    }
    for (int w = 0; w < 4; ++w) {
        if (w == wave) {
#pragma unroll
            for (int r = 0; r < RBW; ++r) {
#pragma unroll
                for (int c = 0; c < CB; ++c)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int k = (rb0 + r) * 16 + (lane >> 4) + 4 * g;
                        const int f = c * 16 + (lane & 15);
                        if (f < fcols) {
                            double* p = out + (size_t)k * FP + f;
                            *p = (w == 0 ? 0.0 : *p) + acc[r][c][g];
                        }
                    }
                if constexpr (S0) {
                    if (lane < 16) {
                        double* p = out + (size_t)((rb0 + r) * 16 + lane) * FP + s0col;
                        *p = (w == 0 ? 0.0 : *p) + s0[r];
                    }
                }
            }
        }
        __syncthreads();
    }
}

/// Epilogue: the workgroup's sum of the lanes' log-likelihood sums, lanes by a shuffle tree, then waves ((0 + 1) + 2) + 3, to *out.
__device__ __forceinline__ void fold_log_likelihood(double ll_acc, double (&red)[4], int wave, int lane, int tid, double* out)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) ll_acc += __shfl_down(ll_acc, off, 64);
    if (lane == 0) red[wave] = ll_acc;
    __syncthreads();
    if (tid == 0) *out = ((red[0] + red[1]) + red[2]) + red[3];
}

/// Diagonal statistics: feature f of the GEMM as a product of two slots of the LDS row [x~_0 .. x~_(D-1) | 1 (ONE) | 0 (ZERO)]:
/// f < d -> x~_f * 1 ; d <= f < 2d -> x~_(f-d)^2 ; beyond -> 0 * 0.
template <int CB> __device__ __forceinline__ void diag_feature_offsets(int lane, int d, int ONE, int ZERO, int (&offa)[CB], int (&offb)[CB])
{
#pragma unroll
    for (int c = 0; c < CB; ++c) {
        const int f = c * 16 + (lane & 15);
        offa[c] = f < d ? f : (f < 2 * d ? f - d : ZERO);
        offb[c] = f < d ? ONE : (f < 2 * d ? f - d : ZERO);
    }
}

// ---- host: shape rules of the kernels above with up to 64 components in 16-component row blocks (em_diag.hip, em_tied.hip) ----

constexpr int rbw_of(int RBT) { return RBT >= 2 ? 2 : 1; }   // row blocks one workgroup accumulates, of RBT that exist

inline bool tile_shape_supported(int d, int K) { return d >= 1 && d <= kRegDim && K >= 1 && K <= 64; }

/// Rows of a partial block: K in whole row blocks, three of them run as four.
inline int tile_partial_rows(int K) { const int RB = (K + 15) / 16; return (RB == 1 ? 1 : RB == 2 ? 2 : 4) * 16; }

/// f(std::integral_constant<int, RBT>) for the row blocks RBT in {1, 2, 4} that hold K components; -1 beyond 64 components.
template <typename F> int dispatch_row_blocks(int K, F&& f)
{
    const int RB = (K + 15) / 16;
    if (RB == 1) return f(std::integral_constant<int, 1>{});
    if (RB == 2) return f(std::integral_constant<int, 2>{});
    if (RB <= 4) return f(std::integral_constant<int, 4>{});
    return -1;
}

/// Workgroups in x a launch uses for (d, K, n) with wave tiles of `tile_samples` -- also the number of partial blocks and
/// log-likelihood partials. `two_groups_from`: the row blocks from which the grid is halved for two row-block groups in grid.y.
/// em_tied.hip passes 3, em_diag.hip 4; 3 matches what is launched (3 row blocks run as RBT = 4 with grid.y = 2).
inline int tile_grid(int d, int K, uint32_t n, uint32_t tile_samples, int num_cus, int two_groups_from)
{
    const int RB = (K + 15) / 16;
    const uint32_t n_tiles = (n + tile_samples - 1) / tile_samples;
    const int groups = RB >= two_groups_from ? 2 : 1;
    const int per_cu = (padded_dim(d) <= 16 && RB <= 2) ? 2 : 1;     // workgroups the registers / LDS admit per CU
    int grid = per_cu * num_cus / groups;
    if ((uint32_t)grid * 4 > n_tiles) grid = (int)((n_tiles + 3) / 4);
    return grid < 1 ? 1 : grid;
}

}  // namespace mstats
}  // namespace mlhip
