// One EM iteration's device work for DIAGONAL covariances in ONE kernel (d <= 32, K <= 64): E-step + M-step statistics,
// X read once, only the per-sample log-sum-exp written. EXTENSION: the reference's ml::EM is full-covariance only
// (ML/EM.hpp:175); this is the same pair of loops -- EM::expectation_step (ML/EM.cpp:190-219) and the sums of
// EM::maximisation_step (:229-250) -- with every covariance restricted to its diagonal, as BASELINE.json configs[1]
// (N=1M, d=16, K=16) asks. Arithmetic per (sample, component):
//     z_j = x_j - mu_kj ;  q = sum_j (z_j * iv_kj) * z_j  (ascending j; iv = 1/sigma^2) ;  lw = log pi_k - sum_j log sigma_kj - q/2
// then per sample m = max_k lw, e_k = exp(lw_k - m), s = sum e_k, lse = m + log s, r_k = e_k / s, and per component
//     S0 = sum_i r,  S1'_j = sum_i r x~_j,  S2'_j = sum_i r x~_j^2,   x~ = x - shift  (2d + 1 numbers instead of (d+1)(d+2)/2).
//
// Mapping (the structure of em_fused_small.hip): a wave owns a stream of 64-sample tiles, lane = sample while the
// densities are evaluated (coordinates in VGPRs, component records [mu | iv | coef] staged once per workgroup in LDS and read
// as broadcasts); r and x~ then go through the wave's private LDS tiles into ONE GEMM on the fp64 matrix cores,
//     stats[K x 2d] += R^T[K x 64] * Phi[64 x 2d],   Phi_i = [x~_i ; x~_i^2],
// whose B operand is generated in registers as a product of two LDS reads (x~_j * 1 or x~_j * x~_j); S0 is a per-lane
// running sum folded once at the end. No atomics; per-workgroup partials are combined in fixed order by em_reduce_kernel.
// Bound: ~3d VALU + one exp per (sample, component) against 8d bytes per sample -- VALU/latency-bound at d = K = 16, not HBM.
#include <cstdlib>
#include "parts.hpp"
#include <type_traits>

#include "em_tile_common.hpp"

#ifndef DIAG_STATS_UNROLL
#define DIAG_STATS_UNROLL 16   // the 16 sample groups of a slot, all of them [r5]: 73.8 -> 73.05 us
#endif

namespace mlhip {
namespace mstats {
namespace {

/// RBT = 16-component row blocks that exist (K <= 16 RBT), RBW = row blocks this workgroup accumulates (blockIdx.y picks the
/// group; every group evaluates all K densities -- the normalisation needs them), CB = 16-column blocks of the 2d features,
/// S = samples per lane: a wave's tile is 64 S samples. The density loop is bound by its LDS operand traffic (every
/// (component, dimension) needs mu and 1/sigma^2 as per-lane broadcast reads: 64 x 16 bytes through the CU's one LDS pipe for
/// 3 VALU operations), so two samples per lane halve it where the registers allow (measured at d = K = 16: 126 -> see DESIGN).
template <int D, int RBT, int RBW, int CB, int S>
__global__ __launch_bounds__(256, (D <= 16 && RBT <= 2) ? 2 : 1) void em_diag_kernel(
    const double* __restrict__ xt, size_t ldx, uint32_t n, int d, const double* __restrict__ shift,
    const double* __restrict__ params, int K, double* __restrict__ lse_out, double* __restrict__ partials, int KP, int FP,
    double* __restrict__ ll_partials, double ab_limit)
{
    constexpr int PS = 2 * D + 2;                             // diag_param_stride(D)
    constexpr int KMAX = 16 * RBT;
    constexpr int JC = D % 2 == 0 ? 2 : 1;                    // dimensions per operand batch of the density loop
    constexpr int XSS = xsd<D>();
    constexpr int TW = TS * S;                                // samples per wave tile
    extern __shared__ __attribute__((aligned(16))) double smem[];
    __shared__ double red[4];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    double* Xw = smem + (size_t)wave * (TS * XSS + TS * RSS);
    double* Rw = Xw + TS * XSS;
    double* recs = smem + 4 * (TS * XSS + TS * RSS);          // [KMAX][PS]: records beyond K are neutral (coef = -inf)
    constexpr int ONE = D, ZERO = D + 1;                      // LDS row: [x~_0 .. x~_(D-1) | 1 | 0]
    const int rb0 = blockIdx.y * RBW;                         // first row block accumulated here
    for (int e = tid; e < KMAX * PS; e += 256) recs[e] = params[e];
    __syncthreads();
    // Two-operation form of the density loop: with a = 1/sigma and b = -(mu - shift)/sigma the term ((x - mu) / sigma)^2 is
    // fma(a, x~, b)^2 on the shift-centred coordinate x~ -- 2 fp64 operations per (sample, component, dimension) instead of
    // 3, a third of the loop that is most of this kernel. It costs about eps (|a x~| + |b|) of every term, so it is only
    // taken while every |b| is below ab_limit (layout.hpp kDiagAbLimit: 1e-14 of a term, inside the parity tolerances);
    // otherwise -- a tight component far from the global mean -- the exact form (x - mu first) runs. Every workgroup (and
    // every rank) derives the same decision from the same records; the records in LDS are rewritten in place: mu -> b,
    // 1/sigma^2 -> a.
    bool ab;
    {
        double bm = 0.0;
        for (int e = tid; e < KMAX * D; e += 256) {
            const int k = e / D, j = e - k * D;
            if (k < K && j < d) {
                const double a = sqrt(recs[k * PS + D + j]);
                bm = fmax(bm, fabs((recs[k * PS + j] - shift[j]) * a));       // (a NaN stays out of fmax; caught below)
                if (!(a == a) || !(recs[k * PS + j] == recs[k * PS + j])) bm = __builtin_inf();
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) bm = fmax(bm, __shfl_xor(bm, off, 64));
        if (lane == 0) red[wave] = bm;
        __syncthreads();
        bm = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
        ab = bm <= ab_limit;
        if (ab) {
            for (int e = tid; e < KMAX * D; e += 256) {
                const int k = e / D, j = e - k * D;
                const double a = sqrt(recs[k * PS + D + j]);
                const double b = -((recs[k * PS + j] - shift[j]) * a);
                recs[k * PS + j] = b;
                recs[k * PS + D + j] = a;
            }
        }
        __syncthreads();
    }

    // feature f of the GEMM: f < d -> x~_f * 1 ; d <= f < 2d -> x~_(f-d)^2 ; beyond -> 0 * 0
    int offa[CB], offb[CB];
    diag_feature_offsets<CB>(lane, d, ONE, ZERO, offa, offb);

    d4 acc[RBW][CB];
    double s0[RBW];                                           // lane (g, c): partial S0 of component c of each row block
#pragma unroll
    for (int r = 0; r < RBW; ++r) {
        s0[r] = 0.0;
#pragma unroll
        for (int c = 0; c < CB; ++c) acc[r][c] = d4{0.0, 0.0, 0.0, 0.0};
    }

    const uint32_t n_tiles = (n + TW - 1) / TW;
    const uint32_t stride = gridDim.x * 4;
    const double* xbase = Xw + 16 * (lane >> 4) * XSS;
    const double* rbase = Rw + 16 * (lane >> 4) * RSS + (lane & 15);
    double ll_acc = 0.0;

    for (uint32_t tile = blockIdx.x * 4 + wave; tile < n_tiles; tile += stride) {
        // Loop-invariant values the compiler would otherwise keep in (spilled) SGPRs: K (the guards below become scalar
        // compares) and the record base, which lives in ONE VGPR so that every operand read is `ds_read base offset:imm`
        // (a constant LDS address per read gets materialised in an SGPR each: measured 279 SGPR spills at d = K = 16).
        asm volatile("" ::: "memory");
        int Kt = K;
        asm volatile("" : "+s"(Kt));
        lds_cdouble* recv = (lds_cdouble*)recs;
        asm volatile("" : "+v"(recv));
        const uint32_t i0 = tile * TW + lane;                 // sample of slot s: i0 + 64 s (< n_pad: n_pad is a multiple of 256)
        double x[S][D];
#pragma unroll
        for (int s = 0; s < S; ++s)
#pragma unroll
            for (int j = 0; j < D; ++j) x[s][j] = xt[(size_t)j * ldx + i0 + TS * s];
        if (ab) {                                             // the two-operation form works on x~ = x - shift throughout
#pragma unroll
            for (int j = 0; j < D; ++j) {
                const double sh = shift[j];
#pragma unroll
                for (int s = 0; s < S; ++s) x[s][j] -= sh;
            }
        }

        // ---- 1. log-densities of all K components (statically unrolled; wave-uniform guards per group of 4)
        double lwv[S][KMAX];
        double m[S];
#pragma unroll
        for (int s = 0; s < S; ++s) m[s] = -__builtin_inf();
        auto densities = [&](auto two_op_form) {
        constexpr bool AB = decltype(two_op_form)::value;
#pragma unroll
        for (int k4 = 0; k4 < KMAX; k4 += 4) {
            if (k4 < Kt) {
                // 4 components x JC dimensions per batch: the 2 * 4 * JC operands are read from LDS in one go, then consumed
                // by all S samples of the lane. Every q accumulates in ascending j.
                lds_cdouble* p = recv + k4 * PS;
                double q[S][4];
#pragma unroll
                for (int s = 0; s < S; ++s)
#pragma unroll
                    for (int u = 0; u < 4; ++u) q[s][u] = 0.0;
#pragma unroll
                for (int j0 = 0; j0 < D; j0 += JC) {
                    double mu[4][JC], iv[4][JC];
#pragma unroll
                    for (int u = 0; u < 4; ++u)
#pragma unroll
                        for (int jj = 0; jj < JC; ++jj) {
                            mu[u][jj] = p[u * PS + j0 + jj];
                            iv[u][jj] = p[u * PS + D + j0 + jj];
                        }
#pragma unroll
                    for (int jj = 0; jj < JC; ++jj)
#pragma unroll
                        for (int u = 0; u < 4; ++u)
#pragma unroll
                            for (int s = 0; s < S; ++s) {
                                if constexpr (AB) {
                                    const double t = __builtin_fma(iv[u][jj], x[s][j0 + jj], mu[u][jj]);   // (a, b) in the (iv, mu) slots
                                    q[s][u] = __builtin_fma(t, t, q[s][u]);
                                } else {
                                    const double z = x[s][j0 + jj] - mu[u][jj];
                                    q[s][u] = __builtin_fma(z * iv[u][jj], z, q[s][u]);
                                }
                            }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const double coef = p[u * PS + 2 * D];                          // records k >= K: coef = -inf
#pragma unroll
                    for (int s = 0; s < S; ++s) {
                        const double lw = __builtin_fma(-0.5, q[s][u], coef);
                        lwv[s][k4 + u] = lw;
                        m[s] = lw > m[s] ? lw : m[s];
                    }
                }
            } else {
#pragma unroll
                for (int s = 0; s < S; ++s)
#pragma unroll
                    for (int u = 0; u < 4; ++u) lwv[s][k4 + u] = -__builtin_inf();
            }
        }
        };
        if (ab) densities(std::true_type{}); else densities(std::false_type{});
        // ---- 2. normalisation: one exp per (sample, component)
        double inv[S];
#pragma unroll
        for (int s = 0; s < S; ++s) {
            double sum = 0.0;
#pragma unroll
            for (int k4 = 0; k4 < KMAX; k4 += 4) {
                if (k4 < Kt) {
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const double e = exp_nonpos(lwv[s][k4 + u] - m[s]);       // exp(-inf) = 0 for the neutral tail
                        lwv[s][k4 + u] = e;
                        sum += e;
                    }
                } else {
#pragma unroll
                    for (int u = 0; u < 4; ++u) lwv[s][k4 + u] = 0.0;
                }
            }
            const double lse = m[s] + log(sum);
            const bool live = i0 + TS * s < n;
            if (blockIdx.y == 0) {
                lse_out[i0 + TS * s] = lse;
                if (live) ll_acc += lse;
            }
            inv[s] = live ? 1.0 / sum : 0.0;                     // padding samples contribute nothing
        }

        // ---- 3. per 64-sample slot: tiles -> LDS, statistics on the matrix cores
#pragma unroll
        for (int s = 0; s < S; ++s) {
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int j = 0; j < D; ++j) Xw[lane * XSS + j] = ab ? x[s][j] : x[s][j] - shift[j];   // shift is zero-padded to D entries
            Xw[lane * XSS + ONE] = 1.0;
            Xw[lane * XSS + ZERO] = 0.0;
#pragma unroll
            for (int rb = 0; rb < RBW; ++rb) {
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int it = 0; it < 16; ++it) {
                    // (rb0 is uniform over the workgroup; the row-block index is resolved at compile time per group)
                    double r = 0.0;
#pragma unroll
                    for (int g = 0; g < RBT / RBW; ++g)
                        if (rb0 == g * RBW) r = lwv[s][(g * RBW + rb) * 16 + it];
                    Rw[lane * RSS + it] = r * inv[s];
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                if ((rb0 + rb) * 16 < Kt) {                          // wave-uniform: skip all-zero row blocks
                    __builtin_amdgcn_s_setprio(kMatrixPhasePriority);  // see em_estep_mfma4.hip
                    stats_tile<CB, 4, true>(rbase, [&](int sg, int c) { const double* xr = xbase + sg * XSS; return xr[offa[c]] * xr[offb[c]]; },
                                            acc[rb], &s0[rb]);
                    __builtin_amdgcn_s_setprio(0);
                }
            }
        }
    }

    // ---- epilogue: fold the 4 waves' accumulators, S0 sums and log-likelihood sums in fixed order
    // partial block of this workgroup column: [KP][FP], row = component, columns [0, 2d) features, column 2d = S0
    fold_waves<RBW, CB, true>(partials + (size_t)blockIdx.x * KP * FP, FP, rb0, wave, lane, acc, 2 * d, s0, 2 * d);
    if (blockIdx.y == 0) fold_log_likelihood(ll_acc, red, wave, lane, tid, ll_partials + blockIdx.x);
}

/// K <= 16, d <= 16 (BASELINE.json configs[1]): the two-operation density form
///     t = fma(a, x~, b) ;  q = fma(t, t, q)        a = 1 / sigma, b = -(mu - shift) / sigma
/// -- 2 vector instructions per (sample, component, dimension) instead of the 3 of the exact form -- run DIMENSION-outer: for one j the
/// operand pairs of all 16 components are contiguous (the records' trailer, layout.hpp: aT / bT, interleaved in LDS) and feed 16
/// INDEPENDENT accumulation chains per sample (q_k, which then become lw_k, e_k, r_k in place); S = 2 samples per lane share every
/// operand read. Both operands come from LDS: feeding `a` from scalar registers (one scalar source per instruction is what the
/// constant bus allows) was built in three forms and measured SLOWER than the exact kernel in spite of 20 - 24 % fewer
/// vector instructions -- scalar loads and LDS reads share one counter, so every wait in the loop becomes a wait for everything
/// (profiles/r04_diag_feed.txt). Taken while every record's flag allows it (every |b| <= kDiagAbLimit:
/// decided where the records are built, host/em_math.cpp build_diag_params and em_close_diag_kernel) and the shift is the data's;
/// otherwise the exact three-operation form runs from scalar registers. Statistics phase: that of em_diag_kernel, one row block.
template <int D, int CB, int S>
__global__ __launch_bounds__(256, 2) void em_diag_mixed_kernel(
    const double* __restrict__ xt, size_t ldx, uint32_t n, int d, const double* __restrict__ shift,
    const double* __restrict__ params, int K, double* __restrict__ lse_out, double* __restrict__ partials, int KP, int FP,
    double* __restrict__ ll_partials, int allow_two_op)
{
    constexpr int PS = diag_param_stride_c(D);
    constexpr int KMAX = 16;
    constexpr int XSS = xsd<D>();
    constexpr int TW = TS * S;                                // samples per wave tile
    extern __shared__ __attribute__((aligned(16))) double smem[];
    __shared__ double red[4];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    double* Xw = smem + (size_t)wave * (TS * XSS + TS * RSS);
    double* Rw = Xw + TS * XSS;
    double* bl = smem + 4 * (TS * XSS + TS * RSS);            // [D][KMAX] pairs (a, b): the records' trailer, interleaved
    constexpr int ONE = D, ZERO = D + 1;                      // LDS row: [x~_0 .. x~_(D-1) | 1 | 0]
    const double* __restrict__ aT = params + (size_t)KMAX * PS;
    const uint32_t n_tiles = (n + TW - 1) / TW;
    const uint32_t stride = gridDim.x * 4;
    // The samples of the wave's FIRST tile are requested before anything else, so the HBM round trip runs under the staging of the
    // records; every later tile loads its samples at its head, the other wave of the SIMD covering for the round trip. (Round 5 also
    // measured the next tile's samples requested slot by slot during the statistics phase: 2 - 3 us SLOWER -- the 32 coordinate
    // registers stay live through the matrix phase and the loads queue behind its LDS traffic; profiles/r05_diag_skeleton.txt.)
    double x[S][D];
    {
        const uint32_t t0 = blockIdx.x * 4 + wave;
        const uint32_t i0 = (t0 < n_tiles ? t0 : 0) * TW + lane;
#pragma unroll
        for (int s = 0; s < S; ++s)
#pragma unroll
            for (int j = 0; j < D; ++j) x[s][j] = xt[(size_t)j * ldx + i0 + TS * s];
    }
    for (int e = tid; e < KMAX * D; e += 256) { bl[2 * e] = aT[e]; bl[2 * e + 1] = aT[KMAX * D + e]; }
    // every record must allow the two-operation form (wave-uniform: scalar loads and compares)
    bool ab = (allow_two_op & 1) != 0;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) ab = ab && params[(size_t)k * PS + 2 * D + 1] <= kDiagAbLimit * kDiagAbLimit;   // (B2: layout.hpp; a NaN fails)
    __syncthreads();

    int offa[CB], offb[CB];
    diag_feature_offsets<CB>(lane, d, ONE, ZERO, offa, offb);
    d4 acc[CB];
    double s0 = 0.0;                                          // lane (g, c): partial S0 of component c
#pragma unroll
    for (int c = 0; c < CB; ++c) acc[c] = d4{0.0, 0.0, 0.0, 0.0};

    const double* xbase = Xw + 16 * (lane >> 4) * XSS;
    lds_cdouble* pa[CB];
    lds_cdouble* pb[CB];
#pragma unroll
    for (int c = 0; c < CB; ++c) {
        pa[c] = (lds_cdouble*)(xbase + offa[c]);
        pb[c] = (lds_cdouble*)(xbase + offb[c]);
    }
    lds_cdouble* rbase = (lds_cdouble*)(Rw + 16 * (lane >> 4) * RSS + (lane & 15));
    double ll_acc = 0.0;

    for (uint32_t tile = blockIdx.x * 4 + wave; tile < n_tiles; tile += stride) {
        asm volatile("" ::: "memory");
        typedef double d2 __attribute__((ext_vector_type(2)));
        typedef __attribute__((address_space(3))) const d2 lds_cd2;
        lds_cd2* blv = (lds_cd2*)bl;                          // ONE base register: every b read is `ds_read_b128 base offset:imm`
        asm volatile("" : "+v"(blv));
        const uint32_t i0 = tile * TW + lane;                 // sample of slot s: i0 + 64 s (< n_pad: a multiple of 256)
        if (tile != blockIdx.x * 4 + wave) {
#pragma unroll
            for (int s = 0; s < S; ++s)
#pragma unroll
                for (int j = 0; j < D; ++j) x[s][j] = xt[(size_t)j * ldx + i0 + TS * s];
        }

        // ---- 1. log-densities of all 16 component slots (records k >= K are neutral: a = b = 0, coef = -inf)
        double lwv[S][KMAX];
        double m[S];
#pragma unroll
        for (int s = 0; s < S; ++s) m[s] = -__builtin_inf();
        if (ab) {
#pragma unroll
            for (int j = 0; j < D; ++j) {                     // the two-operation form works on x~ = x - shift throughout
                const double sh = shift[j];
#pragma unroll
                for (int s = 0; s < S; ++s) x[s][j] -= sh;
            }
            // (no zeroing of the 32 sums: the first dimension's term is a plain product -- fma(t, t, +0) and t * t are the same bits --,
            // 32 register moves per 64 samples less [r5])
            // Software pipeline over the dimensions, in HALVES of 8 components: the operand pairs (a, b) of a half -- eight 16-byte LDS
            // broadcast reads -- are re-loaded for dimension j + 1 as soon as dimension j's arithmetic on that half has been ISSUED,
            // and land while the other half's 16 S instructions run (no second operand buffer; the waits are the compiler's own
            // counted lgkmcnt). Within a half the first operation of four components is issued before their second: a dependent
            // v_fma_f64 right behind its producer stalls.
            constexpr int KH = KMAX / 2;
            d2 pv[2][KH];
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int c = 0; c < KH; ++c) pv[h][c] = blv[h * KH + c];
#pragma unroll
            for (int j = 0; j < D; ++j) {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
#pragma unroll
                    for (int g = 0; g < KH; g += 4) {
                        double t[4][S];
#pragma unroll
                        for (int u = 0; u < 4; ++u)
#pragma unroll
                            for (int s = 0; s < S; ++s) t[u][s] = __builtin_fma(pv[h][g + u][0], x[s][j], pv[h][g + u][1]);
#pragma unroll
                        for (int u = 0; u < 4; ++u)
#pragma unroll
                            for (int s = 0; s < S; ++s)
                                lwv[s][h * KH + g + u] = j == 0 ? t[u][s] * t[u][s] : __builtin_fma(t[u][s], t[u][s], lwv[s][h * KH + g + u]);
                    }
                    if (j + 1 < D) {
#pragma unroll
                        for (int c = 0; c < KH; ++c) pv[h][c] = blv[(j + 1) * KMAX + h * KH + c];
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < KMAX; ++k) {
                const double coef = params[(size_t)k * PS + 2 * D];
#pragma unroll
                for (int s = 0; s < S; ++s) {
                    const double lw = __builtin_fma(-0.5, lwv[s][k], coef);
                    lwv[s][k] = lw;
                    asm("v_max_f64 %0, %0, %1" : "+v"(m[s]) : "v"(lw));             // (a NaN lw leaves m, as `lw > m ? lw : m` does)
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < KMAX; ++k) {
                if (k < K) {
                    const double* __restrict__ p = params + (size_t)k * PS;
                    double q[S];
#pragma unroll
                    for (int s = 0; s < S; ++s) q[s] = 0.0;
#pragma unroll
                    for (int j = 0; j < D; ++j)
#pragma unroll
                        for (int s = 0; s < S; ++s) {
                            const double z = x[s][j] - p[j];
                            q[s] = __builtin_fma(z * p[D + j], z, q[s]);
                        }
#pragma unroll
                    for (int s = 0; s < S; ++s) {
                        const double lw = __builtin_fma(-0.5, q[s], p[2 * D]);
                        lwv[s][k] = lw;
                        asm("v_max_f64 %0, %0, %1" : "+v"(m[s]) : "v"(lw));
                    }
                    __builtin_amdgcn_sched_barrier(0);        // one record in scalar registers at a time
                } else {
#pragma unroll
                    for (int s = 0; s < S; ++s) lwv[s][k] = -__builtin_inf();
                }
            }
#pragma unroll
            for (int j = 0; j < D; ++j) {
                const double sh = shift[j];                   // shift is zero-padded to D entries
#pragma unroll
                for (int s = 0; s < S; ++s) x[s][j] -= sh;
            }
        }
        // ---- 2. normalisation: one exp per (sample, component)
        double inv[S];
#pragma unroll
        for (int s = 0; s < S; ++s) {
            double sum = 0.0;
#pragma unroll
            for (int k8 = 0; k8 < KMAX; k8 += 8) {                                // eight chains side by side (exp_nonpos.hpp)
                double e[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) e[u] = lwv[s][k8 + u] - m[s];
                exp_nonpos_n<8>(e);                            // exp(-inf) = 0 for the neutral tail
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    lwv[s][k8 + u] = e[u];
                    sum += e[u];
                }
            }
            const double lse = m[s] + log(sum);
            const bool live = i0 + TS * s < n;
            lse_out[i0 + TS * s] = lse;
            if (live) ll_acc += lse;
            inv[s] = live ? 1.0 / sum : 0.0;                     // padding samples contribute nothing
        }

        // ---- 3. per 64-sample slot: tiles -> LDS, statistics on the matrix cores
#pragma unroll
        for (int s = 0; s < S; ++s) {
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int j = 0; j < D; ++j) Xw[lane * XSS + j] = x[s][j];
            Xw[lane * XSS + ONE] = 1.0;
            Xw[lane * XSS + ZERO] = 0.0;
#pragma unroll
            for (int it = 0; it < 16; ++it) Rw[lane * RSS + it] = lwv[s][it] * inv[s];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_s_setprio(kMatrixPhasePriority);
            stats_tile<CB, DIAG_STATS_UNROLL, true>(rbase, [&](int sg, int c) { return pa[c][sg * XSS] * pb[c][sg * XSS]; }, acc, &s0);
            __builtin_amdgcn_s_setprio(0);
        }
    }

    // ---- epilogue: the 4 waves' accumulators and S0 sums folded in fixed order  (((0 + w0) + w1) + w2) + w3  -- through LDS (every
    // wave parks its values in its own, now idle, tile region; one barrier; one store per output). Round 4 chained the waves through
    // global memory, a read-modify-write and a barrier per wave: 4.5 us of a 77 us kernel.
    s0 += __shfl_xor(s0, 16, 64);
    s0 += __shfl_xor(s0, 32, 64);
    constexpr int WREG = TS * XSS + TS * RSS;                  // doubles per wave region (>= 64 (4 CB + 1))
    static_assert(64 * (4 * CB + 1) <= WREG, "the parked accumulators must fit a wave's tile region");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int c = 0; c < CB; ++c)
#pragma unroll
        for (int g = 0; g < 4; ++g) Xw[(c * 4 + g) * 64 + lane] = acc[c][g];
    Xw[4 * CB * 64 + lane] = s0;
    __syncthreads();
    double* out = partials + (size_t)blockIdx.x * KP * FP;
    for (int e = tid; e < 4 * CB * 64; e += 256) {
        const int l = e & 63, g = (e >> 6) & 3, c = e >> 8;
        const int k = (l >> 4) + 4 * g, f = c * 16 + (l & 15);
        if (f < 2 * d)
            out[(size_t)k * FP + f] = (((0.0 + smem[e]) + smem[WREG + e]) + smem[2 * WREG + e]) + smem[3 * WREG + e];
    }
    if (tid < 16) {
        const int e = 4 * CB * 64 + tid;
        out[(size_t)tid * FP + 2 * d] = (((0.0 + smem[e]) + smem[WREG + e]) + smem[2 * WREG + e]) + smem[3 * WREG + e];
    }
    fold_log_likelihood(ll_acc, red, wave, lane, tid, ll_partials + blockIdx.x);
}

/// Bound of the two-operation density form; a.exact: the exact form always.
inline double ab_limit(const DiagArgs& a) { return a.exact ? -1.0 : kDiagAbLimit; }

/// Samples per lane: 2 while coordinates + densities of both fit the registers of 2 waves per SIMD, else 1.
constexpr int samples_per_lane(int D, int RBT) { return (D <= 16 && RBT == 1) || (D <= 8 && RBT == 2) ? 2 : 1; }

template <int D, int RBT>
int launch_t(const DiagArgs& a, int grid, hipStream_t stream)
{
    constexpr int CB = (2 * D + 15) / 16, RBW = rbw_of(RBT), PS = 2 * D + 2, XSS = xsd<D>(), S = samples_per_lane(D, RBT);
    if constexpr (RBT == 1 && D <= 16) {                          // one row block, d <= 16: the two-operation kernel
        const size_t smem = sizeof(double) * (4 * ((size_t)TS * XSS + (size_t)TS * RSS) + (size_t)32 * D);
        hipLaunchKernelGGL((em_diag_mixed_kernel<D, CB, S>), dim3(grid), dim3(256), smem, stream, a.xt, a.ldx, a.n, a.d, a.shift,
                           a.params, a.K, a.lse, a.partials, em_diag_partial_rows(a.K), em_diag_partial_cols(a.d), a.ll_partials,
                           (a.two_op && ab_limit(a) > 0) ? 1 : 0);
        return grid;
    } else {
        const size_t smem = sizeof(double) * (4 * ((size_t)TS * XSS + (size_t)TS * RSS) + (size_t)16 * RBT * PS);
        hipLaunchKernelGGL((em_diag_kernel<D, RBT, RBW, CB, S>), dim3(grid, RBT / RBW), dim3(256), smem, stream, a.xt, a.ldx, a.n, a.d,
                           a.shift, a.params, a.K, a.lse, a.partials, em_diag_partial_rows(a.K), em_diag_partial_cols(a.d),
                           a.ll_partials, ab_limit(a));
        return grid;
    }
}

}  // namespace

int MLHIP_PART_FN(launch_em_diag)(const DiagArgs& a, int grid, hipStream_t stream)
{
    return dispatch_part_dim(a.d, [&](auto D) {
        return dispatch_row_blocks(a.K, [&](auto RBT) { return launch_t<decltype(D)::value, decltype(RBT)::value>(a, grid, stream); });
    });
}

#if MLHIP_PART == 1
MLHIP_DECLARE_DIM_PARTS(launch_em_diag, DiagArgs)

bool em_diag_supported(int d, int K) { return tile_shape_supported(d, K); }
int em_diag_partial_rows(int K) { return tile_partial_rows(K); }
int em_diag_partial_cols(int d) { return (2 * d + 1 + 15) / 16 * 16; }

int em_diag_grid(int d, int K, uint32_t n, int num_cus)
{
    const uint32_t tw = (uint32_t)TS * samples_per_lane(padded_dim(d), tile_partial_rows(K) / 16);
    return tile_grid(d, K, n, tw, num_cus, 4);
}

int launch_em_diag(const DiagArgs& a, int num_cus, hipStream_t stream)
{
    if (!em_diag_supported(a.d, a.K)) return -1;
    return launch_dim_part(a, em_diag_grid(a.d, a.K, a.n, num_cus), (size_t)em_diag_partial_rows(a.K) * em_diag_partial_cols(a.d),
                           launch_em_diag_parts, stream);
}
#endif

}  // namespace mstats
}  // namespace mlhip
