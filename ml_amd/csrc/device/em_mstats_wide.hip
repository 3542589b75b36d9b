// M-step sufficient statistics, wide variant (>= 5 column blocks, i.e. d >= 8): see em_mstats.hip for the formulation
// (one fp64-MFMA GEMM stats[K x F] = R^T Phi with Phi generated in registers). This file holds the decomposition used
// for the headline shapes:
//
//   * one 512-thread workgroup per CU; the 64-sample tile (x~ rows and responsibilities of up to 64 components) is staged
//     ONCE per CU; the exp(lw - lse) normalisation is applied while staging, once per (sample, component);
//   * wave w takes column blocks w, w+8, w+16, ... (round-robin: at d = 32 waves 0-3 hold 5, waves 4-7 hold 4 of the 36
//     blocks, and the two waves sharing a SIMD -- w and w+4 -- together always hold 9) and ALL row blocks of the group:
//     RBW x CBW <= 4 x 5 accumulator tiles, so every generated B operand (one multiply, two LDS reads) feeds 4 MFMAs;
//   * software pipeline over tiles: global loads of tile t+1 are issued (unconditionally, clamped addresses) right after
//     the barrier and stay in flight during the MFMA phase of tile t; LDS tiles are double-buffered -> one barrier per
//     tile;
//   * responsibilities come in one of three forms (template EXP): 0 = plain r (caller-given, one-hot, all ones), 1 = log-
//     responsibilities with the per-sample log-sum-exp given (r = exp(lw - lse)), 2 = log-responsibilities only: the kernel
//     NORMALISES THEM ITSELF while staging (the E-step then needs no exp at all: one exp per (sample, component) in the whole
//     iteration instead of two). For that the staging roles are laid out so that the K values of one sample sit in ONE wave
//     (lane = sample-in-8 + 8 * component group, each thread 2 RBW consecutive components): max and sum over them are three
//     xor-shuffle steps inside the wave, no extra barrier; lanes of component group 0 write the sample's maximum and the sum of
//     its exponentials, which a small follow-up kernel (em_lse_finish_kernel, em_mstats.hip) turns into lse and the log-
//     likelihood partials. Needs all K components in this workgroup (a single row-block group, K <= 64).
//     3 = form 2 on a block with row weights: the staged value is r w_i (stage_self_norm<WEIGHTED>), the weights arrive in the
//     `lse` argument, which form 2 does not read (the kernels' signature, and with it every unweighted instantiation, stays as it
//     was); max and sum are written as in form 2, the weighted follow-up kernel is in em_weights.hip. Forms 0-2 are compiled in
//     parts 1-8, form 3 alone in parts 9-16: an unweighted fit loads no more code than before.
#include <type_traits>
#include "parts.hpp"

#include "em_mstats_common.hpp"
#include "em_mstats_stage.hpp"

// parts 9-16: the weighted self-normalising form (EXP = 3) of the shapes of parts 1-8
#if MLHIP_PART > 8
#define MLHIP_WIDE_WEIGHTED 1
#define MLHIP_WIDE_BASE (MLHIP_PART - 8)
#else
#define MLHIP_WIDE_BASE MLHIP_PART
#endif

#ifndef MSTATS_UNROLL_GEN
#define MSTATS_UNROLL_GEN 16   // the 16 sample groups of a tile, all of them (see the contraction loop)
#endif

namespace mlhip {
namespace mstats {
namespace {

constexpr int NW = 8;   // waves per workgroup
typedef __attribute__((address_space(3))) const double lds_cdouble;

template <int N, int I = 0, class F> __device__ __forceinline__ void static_for(F&& f)
{
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<N, I + 1>(f);
    }
}

/// CBT > 0 (round 3; single row-block and column-block group, d <= 32): the RBW x CBT accumulator tiles of the GEMM are dealt to
/// the 8 waves as (column block, row block) UNITS in column-major order, ceil / floor(RBW CBT / 8) each, instead of whole column
/// blocks with all their row blocks. At d = 16 (10 column blocks) two waves used to hold 2 x 4 tiles and six waves 1 x 4 -- the
/// contraction ran at the pace of the two; now every wave holds 5. The wave's loop is specialised per wave (switch on the
/// wave index), so which units share an operand product is known at compile time: one product per column block a wave touches.
template <int RBW, int CBW, int EXP, int DM, int CBT = 0>
__global__ __launch_bounds__(512, 2) void em_mstats_wide_kernel(
    const double* __restrict__ xt, size_t ldx, uint32_t n, int d, int D, const double* __restrict__ shift,
    const double* __restrict__ lw, size_t ldr, const double* __restrict__ lse, int K, int n_rbg, int CB_total,
    double* __restrict__ partials, int KP, int FP, double* __restrict__ lse_out, double* __restrict__ ll_out,
    unsigned long long* __restrict__ nz_count)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    constexpr int RS = RBW * 16 + 1;     // odd row stride of the responsibility tile
    constexpr int NXV = DM / NW;         // x rows staged per thread (4; 8 for d > 32; 16 for d > 64)
    constexpr int XS = tile_stride<DM>();
    constexpr bool DOUBLE_BUF = DM <= kMidDim;   // two (x~, R) tiles of 64 samples do not fit LDS above d = 64
    constexpr int NRV = RBW * 16 / NW;   // responsibility rows staged per thread (2 * RBW)
    const int da = d + 1;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rbg = blockIdx.y % n_rbg, cbg = blockIdx.y / n_rbg;
    const int rb0 = rbg * RBW;
    const int F = da * (da + 1) / 2;

    // column block c of this wave: cbg*8*CBW + c*8 + wave
    constexpr int NU = CBT > 0 ? (RBW * CBT + NW - 1) / NW : 1;   // balanced form: units per wave (at most)
    constexpr int NOFF = CBT > 0 ? NU : CBW;
    int offa[NOFF], offb[NOFF];
    const int u_lo = CBT > 0 ? wave * (RBW * CBT) / NW : 0, u_hi = CBT > 0 ? (wave + 1) * (RBW * CBT) / NW : 0;
    if constexpr (CBT > 0) {
        // unit u = (column block u / RBW, row block u % RBW); slot j of this wave is unit u_lo + j
#pragma unroll
        for (int j = 0; j < NU; ++j) {
            const int cb = (u_lo + j) / RBW;
            int a, b;
            feature_pair(cb * 16 + (lane & 15), u_lo + j < u_hi ? F : 0, da, a, b);
            offa[j] = a;
            offb[j] = b;
        }
    } else {
#pragma unroll
        for (int c = 0; c < CBW; ++c) {
            const int cb = (cbg * CBW + c) * NW + wave;
            int a, b;
            feature_pair(cb * 16 + (lane & 15), cb < CB_total ? F : 0, da, a, b);
            offa[c] = a;
            offb[c] = b;
        }
    }
    // With CBW = ceil(CB / 8) column blocks per wave and a single column group (d <= 32), only a wave's LAST block can
    // fall outside the matrix (wave-uniform); all others are unconditional, which keeps them in one basic block. With
    // several column groups (d > 32) earlier blocks of the last group may be outside too: they multiply the zero slot.
    const bool last_active = (cbg * CBW + CBW - 1) * NW + wave < CB_total;

    constexpr int AR = CBT > 0 ? 1 : RBW, AC = CBT > 0 ? NU : CBW;
    d4 acc[AR][AC];
#pragma unroll
    for (int r = 0; r < AR; ++r)
#pragma unroll
        for (int c = 0; c < AC; ++c) acc[r][c] = d4{0.0, 0.0, 0.0, 0.0};

    // staging role: sample sS of the tile, rows wave, wave+8, ... For EXP == 2 the responsibilities have their own role:
    // sample sR = 8 wave + (lane & 7), components NRV cg + it with cg = lane >> 3 -- one wave holds all K values of its 8 samples
    // (contiguous components per thread: with the odd row stride RS the 16 lanes of an LDS write phase then hit 16 different
    // bank pairs; the interleaved assignment cg + 8 it collides up to 8-fold and cost 1 ms at the headline shape).
    const int sS = lane;
    const int sR = EXP >= 2 ? 8 * wave + (lane & 7) : lane;
    const int cg = lane >> 3;
    double xv[NXV], rv[NRV], lv = 0.0;
    uint32_t nonzero = 0;                // EXP == 2: nonzero responsibilities staged by this wave (the runtime's kernel choice)
    auto prefetch = [&](uint32_t tile) {
        const uint32_t i = tile * TS + sS;           // < n_pad: always inside the allocation
#pragma unroll
        for (int it = 0; it < NXV; ++it) xv[it] = xt[(size_t)min(wave + NW * it, D - 1) * ldx + i];
        if constexpr (EXP >= 2) {
#pragma unroll
            for (int it = 0; it < NRV; ++it) rv[it] = lw[(size_t)min(cg * NRV + it, K - 1) * ldr + tile * TS + sR];
            if constexpr (EXP == 3) lv = lse[tile * TS + sR];   // the sample's weight (n_pad entries, zero beyond n)
        } else {
#pragma unroll
            for (int it = 0; it < NRV; ++it) rv[it] = lw[(size_t)min(rb0 * 16 + wave + NW * it, K - 1) * ldr + i];
            if (EXP) lv = lse[i];
        }
    };
    auto stage = [&](double* Xb, double* Rb, uint32_t tile) {
        if constexpr (EXP == 3) {
            const uint32_t i = tile * TS + sR;
            nonzero += stage_self_norm<NRV, RS, true>(rv, cg, K, i, i < n, Rb, sR, blockIdx.y == 0, lse_out, ll_out, lv);
        } else if constexpr (EXP == 2) {
            const uint32_t i = tile * TS + sR;
            nonzero += stage_self_norm<NRV, RS>(rv, cg, K, i, i < n, Rb, sR, blockIdx.y == 0, lse_out, ll_out);
        } else {
        const bool live = tile * TS + sS < n;
#pragma unroll
        for (int it = 0; it < NRV; ++it) {
            double r = rv[it];
            if (EXP) r = exp_nonpos(r - lv);
            const bool valid = live && (rb0 * 16 + wave + NW * it < K);
            Rb[sS * RS + wave + NW * it] = valid ? r : 0.0;
        }
        }
#pragma unroll
        for (int it = 0; it < NXV; ++it) {
            const int j = wave + NW * it;
            if (j < d) Xb[sS * XS + j] = xv[it] - shift[j];   // wave-uniform index: scalar load
        }
        if (wave == 0) {
            Xb[sS * XS + d] = 1.0;
            Xb[sS * XS + da] = 0.0;
        }
    };

    const uint32_t n_tiles = (n + TS - 1) / TS;
    constexpr int tile_doubles = TS * XS + TS * RS;
    int buf = 0;
    if (blockIdx.x < n_tiles) prefetch(blockIdx.x);
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x, buf ^= DOUBLE_BUF ? 1 : 0) {
        if constexpr (!DOUBLE_BUF) __syncthreads();   // single tile buffer: everyone is done reading the previous tile
        double* Xb = smem + buf * tile_doubles;
        double* Rb = Xb + TS * XS;
        stage(Xb, Rb, tile);
        __syncthreads();
        const uint32_t next = tile + gridDim.x;
        prefetch(next < n_tiles ? next : tile);      // the last iteration re-reads its own tile (discarded)
        // ---- contraction: 16 groups of 4 samples. Lane group g = lane>>4 takes sample sg + 16 g: rows 16 apart are
        // 32 banks apart for both tiles (odd strides), so the two rows of a half-wave never collide.
        const double* xbase = Xb + 16 * (lane >> 4) * XS;
        const double* rbase = Rb + 16 * (lane >> 4) * RS + (lane & 15);
        __builtin_amdgcn_s_setprio(kMatrixPhasePriority);   // see em_estep_mfma4.hip (11.78 -> 11.59 ms at d = 32, K = 64)
        if constexpr (CBT > 0) {
            auto contract = [&](auto w_) {
                constexpr int W = w_, U = RBW * CBT, LO = W * U / NW, HI = (W + 1) * U / NW, NJ = HI - LO;
                auto step = [&](int sg) {
                    const double* xr = xbase + sg * XS;
                    const double* rr = rbase + sg * RS;
                    double av[RBW];
#pragma unroll
                    for (int r = 0; r < RBW; ++r) av[r] = rr[r * 16];
                    double bv = 0.0;
                    static_for<NJ>([&](auto j_) {
                        constexpr int j = j_, u = LO + j;
                        if constexpr (j == 0 || u / RBW != (u - 1) / RBW) bv = xr[offa[j]] * xr[offb[j]];   // first unit of a column block
                        acc[0][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u % RBW], bv, acc[0][j], 0, 0, 0);
                    });
                };
                for (int sg = 0; sg < TS / 4; sg += 2) {     // two sample groups per trip (written out: `#pragma unroll 2` is refused
                    step(sg);                                // on some of the eight specialisations)
                    step(sg + 1);
                }
            };
            switch (wave) {
            case 0: contract(std::integral_constant<int, 0>{}); break;
            case 1: contract(std::integral_constant<int, 1>{}); break;
            case 2: contract(std::integral_constant<int, 2>{}); break;
            case 3: contract(std::integral_constant<int, 3>{}); break;
            case 4: contract(std::integral_constant<int, 4>{}); break;
            case 5: contract(std::integral_constant<int, 5>{}); break;
            case 6: contract(std::integral_constant<int, 6>{}); break;
            default: contract(std::integral_constant<int, 7>{}); break;
            }
        } else if constexpr (RBW * CBW < 20) {
        // Every shape but the headline's 4 x 5 tiles per wave (which sits at 256 registers): the lane's operand addresses (tile base +
        // coordinate offset) are formed ONCE per tile; inside the loop every LDS read is `ds_read base offset:imm` off running
        // pointers that advance by U sample groups per trip -- otherwise one v_add_u32 per read [r3] (d = 24, K = 64: 4.09 -> 3.97 ms).
        // [r5] also above d = 32, where it had been left out: N = 1M, K = 32, d = 128 11.58 -> 10.54 ms, d = 96 6.50 -> 5.85.
        constexpr int U = TS / 4;                    // [r5] the whole tile unrolled: no pointer advances at all (U = 4 until round 5: d = 128, K = 32 10.5 -> 10.1 ms,
                                                     // d = 32, K = 32 3.11 -> 3.00, d = 28, K = 48 3.53 -> 3.42, d = 12, K = 48 0.574 -> 0.553)
        lds_cdouble* pa[CBW];
        lds_cdouble* pb[CBW];
#pragma unroll
        for (int c = 0; c < CBW; ++c) {
            pa[c] = (lds_cdouble*)(xbase + offa[c]);
            pb[c] = (lds_cdouble*)(xbase + offb[c]);
        }
        lds_cdouble* pr = (lds_cdouble*)rbase;
#pragma unroll 1
        for (int sg0 = 0; sg0 < TS / 4; sg0 += U) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                double av[RBW];
#pragma unroll
                for (int r = 0; r < RBW; ++r) av[r] = pr[u * RS + r * 16];
#pragma unroll
                for (int c = 0; c < CBW - 1; ++c) {
                    const double bv = pa[c][u * XS] * pb[c][u * XS];
#pragma unroll
                    for (int r = 0; r < RBW; ++r)
                        acc[r][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[r], bv, acc[r][c], 0, 0, 0);
                }
                constexpr int c = CBW - 1;                   // (see the loop below for the last block)
                const double bv = pa[c][u * XS] * pb[c][u * XS];
                if (last_active) {
#pragma unroll
                    for (int r = 0; r < RBW; ++r)
                        acc[r][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[r], bv, acc[r][c], 0, 0, 0);
                }
            }
#pragma unroll
            for (int c = 0; c < CBW; ++c) {
                pa[c] += U * XS;
                pb[c] += U * XS;
            }
            pr += U * RS;
        }
        } else {
        // [r5] unrolled over the WHOLE tile (two sample groups per trip until round 5): the operand addresses become one register per column
        // block plus immediates -- no address arithmetic between the matrix instructions --, 249 registers and no scratch instead of
        // 256 + 8 bytes: headline statistics kernel 11.66 -> 11.09 ms (42.7 - 42.8 it/s from 41.6 on the same box), d = 64, K = 64 13.14 -> 12.53.
#pragma unroll MSTATS_UNROLL_GEN
        for (int sg = 0; sg < TS / 4; ++sg) {
            const double* xr = xbase + sg * XS;
            const double* rr = rbase + sg * RS;
            double av[RBW];
#pragma unroll
            for (int r = 0; r < RBW; ++r) av[r] = rr[r * 16];
#pragma unroll
            for (int c = 0; c < CBW - 1; ++c) {
                const double bv = xr[offa[c]] * xr[offb[c]];
#pragma unroll
                for (int r = 0; r < RBW; ++r)
                    acc[r][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[r], bv, acc[r][c], 0, 0, 0);
            }
            // The last block's operand is formed unconditionally (padding columns read the zero slot), so its LDS
            // reads are scheduled with the others; only its MFMAs are skipped by the waves that do not own a block.
            constexpr int c = CBW - 1;
            const double bv = xr[offa[c]] * xr[offb[c]];
            if (last_active) {
#pragma unroll
                for (int r = 0; r < RBW; ++r)
                    acc[r][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[r], bv, acc[r][c], 0, 0, 0);
            }
        }
        }
        __builtin_amdgcn_s_setprio(0);
    }

    if constexpr (EXP >= 2) {
        if (nz_count && blockIdx.y == 0 && lane == 0) atomicAdd(nz_count, (unsigned long long)nonzero);   // (an integer sum: order-free)
    }
    // ---- epilogue: partials[blockIdx.x][k][f]; C/D layout of v_mfma_f64_16x16x4: col = lane&15, row = (lane>>4) + 4*reg
    double* out = partials + (size_t)blockIdx.x * KP * FP;
    if constexpr (CBT > 0) {
#pragma unroll
        for (int j = 0; j < NU; ++j) {
            const int u = u_lo + j;
            if (u < u_hi) {
                const int cb = u / RBW, rb = u % RBW;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int k = rb * 16 + (lane >> 4) + 4 * g;
                    out[(size_t)k * FP + cb * 16 + (lane & 15)] = acc[0][j][g];
                }
            }
        }
    } else {
#pragma unroll
    for (int r = 0; r < RBW; ++r)
#pragma unroll
        for (int c = 0; c < CBW; ++c) {
            const int cb = (cbg * CBW + c) * NW + wave;
            if (cb < CB_total) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int k = (rb0 + r) * 16 + (lane >> 4) + 4 * g;
                    out[(size_t)k * FP + cb * 16 + (lane & 15)] = acc[r][c][g];
                }
            }
        }
    }
}

template <int RBW, int CBW, int DM = kRegDim, int CBT = 0>
void launch_t(const MstatsArgs& a, const Plan& p, int grid_x, hipStream_t stream)
{
    constexpr int XSD = tile_stride<DM>();
    const size_t smem = (DM <= kMidDim ? 2 : 1) * sizeof(double) * ((size_t)TS * XSD + (size_t)TS * (RBW * 16 + 1));
    const dim3 grid(grid_x, p.n_rbg * p.n_cbg);
#ifdef MLHIP_WIDE_WEIGHTED
    hipLaunchKernelGGL((em_mstats_wide_kernel<RBW, CBW, 3, DM, CBT>), grid, dim3(512), smem, stream, a.xt, a.ldx, a.n, a.d,
                       padded_dim(a.d), a.shift, a.lw, a.ldr, a.weights, a.K, p.n_rbg, p.CB, a.partials, p.KP, p.FP,
                       a.lse_out, a.ll_out, a.nz_count);
#else
    if (a.mode == kFromLogRespSelfNorm)
        hipLaunchKernelGGL((em_mstats_wide_kernel<RBW, CBW, 2, DM, CBT>), grid, dim3(512), smem, stream, a.xt, a.ldx, a.n, a.d,
                           padded_dim(a.d), a.shift, a.lw, a.ldr, a.lse, a.K, p.n_rbg, p.CB, a.partials, p.KP, p.FP,
                           a.lse_out, a.ll_out, a.nz_count);
    else if (a.mode == kFromLogResp)
        hipLaunchKernelGGL((em_mstats_wide_kernel<RBW, CBW, 1, DM, CBT>), grid, dim3(512), smem, stream, a.xt, a.ldx, a.n, a.d,
                           padded_dim(a.d), a.shift, a.lw, a.ldr, a.lse, a.K, p.n_rbg, p.CB, a.partials, p.KP, p.FP,
                           nullptr, nullptr, nullptr);
    else
        hipLaunchKernelGGL((em_mstats_wide_kernel<RBW, CBW, 0, DM, CBT>), grid, dim3(512), smem, stream, a.xt, a.ldx, a.n, a.d,
                           padded_dim(a.d), a.shift, a.lw, a.ldr, a.lse, a.K, p.n_rbg, p.CB, a.partials, p.KP, p.FP,
                           nullptr, nullptr, nullptr);
#endif
}

}  // namespace

// ---- one code object per (row blocks per workgroup, dimension class): the Makefile compiles this file eight times with
// -DMLHIP_PART=1..8 (parts 1-4: d <= 32 with RBW = part; 5-8: 32 < d <= 128 with RBW = part - 4). A fit uses one K and one d, so it
// touches one or two of them (the sample covariance is a K = 1 call: RBW = 1) and the first use of a shape loads ~0.3 MB of
// kernels instead of the 2.1 MB of all 147 instantiations (round 5: the first call of a shape was dominated by that load).
int MLHIP_PART_FN(launch_wide)(const MstatsArgs& a, const Plan& p, int grid_x, hipStream_t stream)
{
    constexpr int R = (MLHIP_WIDE_BASE - 1) % 4 + 1;
    if (p.RBW != R) return -1;
#ifdef MLHIP_WIDE_WEIGHTED
    if (a.mode != kFromLogRespSelfNormWeighted || !a.weights) return -1;
#else
    if (a.mode == kFromLogRespSelfNormWeighted) return -1;
#endif
#if MLHIP_WIDE_BASE > 4
    // 32 < d <= 128: 38..525 column blocks in column groups of 8 waves x (3, 4 or 5) blocks
#define MLHIP_BIG(C) \
    if (p.CBW == C) { \
        if (a.d <= kMidDim) launch_t<R, C, kMidDim>(a, p, grid_x, stream); else launch_t<R, C, kMaxDim>(a, p, grid_x, stream); \
    } else
    MLHIP_BIG(3) MLHIP_BIG(4) MLHIP_BIG(5)
    { return -1; }
#undef MLHIP_BIG
    return grid_x;
#else
    // balanced dealing of (column block, row block) units where whole column blocks leave the waves unevenly loaded
    // (a.plain: off)
    if (!a.plain && p.n_rbg == 1 && p.n_cbg == 1) {
        if constexpr (R == 4) {
            if (p.CB == 6) { launch_t<4, 1, kRegDim, 6>(a, p, grid_x, stream); return grid_x; }      // d = 12
            if (p.CB == 10) { launch_t<4, 2, kRegDim, 10>(a, p, grid_x, stream); return grid_x; }    // d = 16
        }
        if constexpr (R == 3) {
            if (p.CB == 10) { launch_t<3, 2, kRegDim, 10>(a, p, grid_x, stream); return grid_x; }
            if (p.CB == 6) { launch_t<3, 1, kRegDim, 6>(a, p, grid_x, stream); return grid_x; }
        }
        // (K <= 32 at d = 16: the plain form with two workgroups per CU -- the balanced one needs 130 registers -- unless the plan
        //  kept one workgroup per CU)
        if constexpr (R == 2) {
            if (p.CB == 10 && p.wg_per_cu == 1) { launch_t<2, 2, kRegDim, 10>(a, p, grid_x, stream); return grid_x; }
        }
    }
#define MLHIP_CASE(C) \
    if (p.CBW == C) { launch_t<R, C>(a, p, grid_x, stream); } else
    MLHIP_CASE(1) MLHIP_CASE(2) MLHIP_CASE(3) MLHIP_CASE(4) MLHIP_CASE(5)
    { return -1; }
#undef MLHIP_CASE
    return grid_x;
#endif
}

#if MLHIP_PART == 1
int launch_wide_part2(const MstatsArgs&, const Plan&, int, hipStream_t);
int launch_wide_part3(const MstatsArgs&, const Plan&, int, hipStream_t);
int launch_wide_part4(const MstatsArgs&, const Plan&, int, hipStream_t);
int launch_wide_part5(const MstatsArgs&, const Plan&, int, hipStream_t);
int launch_wide_part6(const MstatsArgs&, const Plan&, int, hipStream_t);
int launch_wide_part7(const MstatsArgs&, const Plan&, int, hipStream_t);
int launch_wide_part8(const MstatsArgs&, const Plan&, int, hipStream_t);
int launch_wide_part9(const MstatsArgs&, const Plan&, int, hipStream_t);
int launch_wide_part10(const MstatsArgs&, const Plan&, int, hipStream_t);
int launch_wide_part11(const MstatsArgs&, const Plan&, int, hipStream_t);
int launch_wide_part12(const MstatsArgs&, const Plan&, int, hipStream_t);
int launch_wide_part13(const MstatsArgs&, const Plan&, int, hipStream_t);
int launch_wide_part14(const MstatsArgs&, const Plan&, int, hipStream_t);
int launch_wide_part15(const MstatsArgs&, const Plan&, int, hipStream_t);
int launch_wide_part16(const MstatsArgs&, const Plan&, int, hipStream_t);

int launch_wide(const MstatsArgs& a, const Plan& p, int grid_x, hipStream_t stream)
{
    const bool big = a.d > kRegDim;
    if (a.mode == kFromLogRespSelfNormWeighted) {
        switch (p.RBW) {
        case 1: return big ? launch_wide_part13(a, p, grid_x, stream) : launch_wide_part9(a, p, grid_x, stream);
        case 2: return big ? launch_wide_part14(a, p, grid_x, stream) : launch_wide_part10(a, p, grid_x, stream);
        case 3: return big ? launch_wide_part15(a, p, grid_x, stream) : launch_wide_part11(a, p, grid_x, stream);
        case 4: return big ? launch_wide_part16(a, p, grid_x, stream) : launch_wide_part12(a, p, grid_x, stream);
        default: return -1;
        }
    }
    switch (p.RBW) {
    case 1: return big ? launch_wide_part5(a, p, grid_x, stream) : launch_wide_part1(a, p, grid_x, stream);
    case 2: return big ? launch_wide_part6(a, p, grid_x, stream) : launch_wide_part2(a, p, grid_x, stream);
    case 3: return big ? launch_wide_part7(a, p, grid_x, stream) : launch_wide_part3(a, p, grid_x, stream);
    case 4: return big ? launch_wide_part8(a, p, grid_x, stream) : launch_wide_part4(a, p, grid_x, stream);
    default: return -1;
    }
}
#endif

}  // namespace mstats
}  // namespace mlhip
