// M-step sufficient statistics, SPARSE self-normalising variant (d <= 32, K <= 64): the same statistics as the wide kernel's
// EXP = 2 form (em_mstats_wide.hip) -- per component S_k = sum_i r_ik xt_i xt_i^T, xt_i = [x_i - shift ; 1], packed lower
// triangle, one partial block [KP][FP] per workgroup in the same layout, and the per-sample (max, sum of exponentials) for
// em_lse_finish_kernel -- but only the (sample, component) pairs with r != 0 are accumulated.
//
// Why: once the components of a mixture are well apart, all but a few of a sample's K responsibilities underflow to exactly 0.0
// (headline, d = 32, K = 64, after the first iterations: ~4.8 nonzero per sample). The dense GEMM R^T Phi multiplies all 64; a term
// whose r is exactly 0 adds exactly 0, so skipping them changes nothing but the summation order.
//
//   * staging: the wide kernel's roles and normalisation code (em_mstats_stage.hpp) -> (max, sum) bit-identical to it. The x~ row
//     of a sample is stored with the extra "1" coordinate left out, zero-padded to 32 coordinates and with its first 12 repeated
//     behind them (row stride XE = 45, odd): quad q of the row (4 coordinates) can then be read as quad q .. q + 2 (mod 8);
//   * buckets from the staging ballots: stage_self_norm's ballot of "staged value `it` is nonzero" holds, in byte cg, the nonzero
//     mask of component 8 cg + it over the wave's 8 samples; every wave stores its 64 mask bytes in a table [component][wave]
//     (512 bytes per tile, double-buffered with it), so the 64-bit word of a component is its bucket: bit s = tile sample s. After
//     the tile barrier wave w fetches the words of its components w, w + 8, ... (K <= 64: up to 8) in one batch and keeps them in
//     scalar registers. Entry e of a bucket is the e-th set bit -- scalar bit scans, ascending sample order, the same order in every
//     run; no list in LDS, no read of r to find the bucket, nothing that waits for an LDS store. Every bit is scanned once: a step
//     takes its four entries out of the bucket's remainder (find the lowest bit, clear that bit) and the next step goes on from
//     what is left;
//   * one LDS round trip per step of four entries, issued a step ahead: the operands of the next step -- of this bucket, or the
//     first of the wave's next nonempty one, known from its mask -- are loaded behind the MFMAs that free their registers (the
//     9-double window is not doubled: 192 accumulator registers leave no room for that). Entries past a bucket's end are sample
//     index 64, the sentinel row each tile buffer carries behind its 64 samples: r = 0 and x~ = 0, written once per launch --
//     no clamp, compare or select per lane. (The first form of this kernel read r, balloted, wrote and re-read a list and then
//     the operands: ~7 dependent round trips per component, 5.5 ms at the headline shape; DESIGN.md section 3.3e has every form
//     measured);
//   * accumulation on v_mfma_f64_4x4x4_4b (lane layout as in em_estep_mfma4.hip: A[b][i][k] <- lane 16k + 4b + i,
//     B[b][k][j] <- lane 16k + 4b + j, D[b][i][j] -> lane 16i + 4b + j): four bucket entries per step, sample k = lane >> 4. The
//     32 x 32 Gram matrix has 36 quad pairs {Q, P} with P = Q + delta (mod 8): delta = 0..3 for every Q, delta = 4 for Q < 4.
//     Block b of instruction (g, delta) takes Q = 4g + b, so the A operand is the lane's row quad b + 4g + delta -- one
//     ds_read off a per-lane base with an immediate offset (the repeated quads are what makes that possible) -- and the B
//     operand r x~ quad (b + 4g): 9 instructions for the Gram matrix. sum r x~ (two coordinate halves) and sum r stay off the
//     matrix pipe: a lane already holds r x~ of its two coordinates and r for the entry of its lane group, and adds them into
//     three accumulators of its own (three vector adds instead of three MFMAs with A = 1); the epilogue adds the four lane
//     groups in the fixed order 0, 1, 2, 3. 12 accumulator doubles per component, 192 registers for the wave's 8;
//   * the wide kernel's software pipeline: next tile's loads in flight during the accumulation, double-buffered LDS, one barrier
//     per tile. The wave's four shift values are read once per launch, and with K = 64 (every slot a component) the
//     "component >= K" masks are skipped behind a wave-uniform test.
// Choice between this kernel and the dense one: runtime/em.cpp (run_mstats), from the nonzero count both kernels report.
#include "em_mstats_common.hpp"
#include "em_mstats_stage.hpp"

namespace mlhip {
namespace mstats {
namespace {

constexpr int SNW = 8;             // waves per workgroup
constexpr int SCPW = 8;            // component slots per wave (K <= 64)
constexpr int SNRV = 8;            // responsibilities staged per thread: 64 components x 64 samples / 512 threads
constexpr int SRS = 65;            // odd row stride of the responsibility tile (64 components + 1)
constexpr int SXE = 45;            // odd row stride of the extended sample row: 32 coordinates + the first 12 again
constexpr int SNA = 12;            // accumulators per component: 9 Gram quad pairs; per lane group: 2 sum r x coordinates, sum r

template <int N, int I = 0, class F> __device__ __forceinline__ void static_for(F&& f)
{
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<N, I + 1>(f);
    }
}

/// The wave-uniform value of a 64-bit quantity every lane holds: kept in scalar registers from here on.
__device__ __forceinline__ unsigned long long uniform64(unsigned long long v)
{
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return ((unsigned long long)hi << 32) | lo;
}
/// Takes the lowest sample out of a bucket's remaining entries `rem`; an empty remainder gives the sentinel row TS.
__device__ __forceinline__ uint32_t take_lowest(unsigned long long& rem)
{
    const uint32_t s = rem ? (uint32_t)__builtin_ctzll(rem) : (uint32_t)TS;
    rem &= ~(1ull << (s & 63));                      // (empty: clears bit 0 of 0)
    return s;
}

__global__ __launch_bounds__(512, 2) void em_mstats_sparse_kernel(
    const double* __restrict__ xt, size_t ldx, uint32_t n, int d, int D, const double* __restrict__ shift,
    const double* __restrict__ lw, size_t ldr, int K, double* __restrict__ partials, int KP, int FP,
    double* __restrict__ lse_out, double* __restrict__ esum_out, unsigned long long* __restrict__ nz_count)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    constexpr int NXV = kRegDim / SNW;                // x rows staged per thread (4)
    constexpr int tile_doubles = (TS + 1) * SXE + (TS + 1) * SRS;   // 64 samples and the sentinel row TS: x~ = 0, r = 0
    // [2][64 components]: byte w of a component's word = its nonzero mask over samples 8w .. 8w + 7 (written by wave w)
    unsigned long long* masks = reinterpret_cast<unsigned long long*>(smem + 2 * tile_doubles);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // the sentinel rows of both buffers: written once, never staged over (visible after the first tile's barrier)
    if (tid < 2 * (SXE + SRS)) {
        double* t = smem + (tid >= SXE + SRS ? tile_doubles : 0);
        const int e = tid >= SXE + SRS ? tid - (SXE + SRS) : tid;
        t[e < SXE ? TS * SXE + e : (TS + 1) * SXE + TS * SRS + (e - SXE)] = 0.0;
    }

    double acc[SCPW][SNA];
#pragma unroll
    for (int c = 0; c < SCPW; ++c)
#pragma unroll
        for (int t = 0; t < SNA; ++t) acc[c][t] = 0.0;

    // staging roles as in em_mstats_wide.hip (EXP = 2, RBW = 4)
    const int sS = lane;
    const int sR = 8 * wave + (lane & 7);
    const int cg = lane >> 3;
    double xv[NXV], rv[SNRV];
    uint32_t nonzero = 0;
    double sh[NXV];                                   // shift of the wave's x rows: wave-uniform, read once per launch
#pragma unroll
    for (int it = 0; it < NXV; ++it) sh[it] = shift[min(wave + SNW * it, d - 1)];
    auto prefetch = [&](uint32_t tile) {
        const uint32_t i = tile * TS + sS;           // < n_pad: always inside the allocation
#pragma unroll
        for (int it = 0; it < NXV; ++it) xv[it] = xt[(size_t)min(wave + SNW * it, D - 1) * ldx + i];
        int c0 = cg * SNRV;
        asm volatile("" : "+v"(c0));                 // the eight row offsets are recomputed per tile: hoisted, they are 16 registers
#pragma unroll
        for (int it = 0; it < SNRV; ++it) rv[it] = lw[(size_t)(uint32_t)min(c0 + it, K - 1) * ldr + tile * TS + sR];
    };
    auto stage = [&](double* Xe, double* Rb, unsigned long long* Mk, uint32_t tile) {
        const uint32_t i = tile * TS + sR;
        unsigned long long nz[SNRV];
        int cgt = cg;
        asm volatile("" : "+v"(cgt));                // (the per-value "component >= K" lane masks: per tile, not 16 scalar registers)
        // components >= K: exp(-inf) = 0, as stage_self_norm does it itself -- here behind a wave-uniform test, nothing at K = 64
        if (K < SCPW * SNW) {
#pragma unroll
            for (int it = 0; it < SNRV; ++it)
                if (cgt * SNRV + it >= K) rv[it] = -__builtin_inf();
        }
        nonzero += stage_self_norm<SNRV, SRS, false, true, false>(rv, cgt, K, i, i < n, Rb, sR, true, lse_out, esum_out, 1.0, nz);
        // byte cg of ballot `it` = component 8 cg + it over this wave's 8 samples (lanes 8 cg .. 8 cg + 7)
        if ((lane & 7) == 0) {
            unsigned char* mb = reinterpret_cast<unsigned char*>(Mk + cg * SNRV) + wave;
#pragma unroll
            for (int it = 0; it < SNRV; ++it) mb[8 * it] = (unsigned char)(nz[it] >> (8 * cg));
        }
#pragma unroll
        for (int it = 0; it < NXV; ++it) {
            const int j = wave + SNW * it;
            const double v = j < d ? xv[it] - sh[it] : 0.0;
            Xe[sS * SXE + j] = v;
            if (j < 12) Xe[sS * SXE + 32 + j] = v;
        }
    };

    // accumulation role: bucket entry k = lane >> 4 of a step of four, block b, row / column i = j = lane & 3
    const int k4 = lane >> 4, bq = (lane >> 2) & 3, i4 = lane & 3;
    const uint32_t n_tiles = (n + TS - 1) / TS;
    int buf = 0;
    if (blockIdx.x < n_tiles) prefetch(blockIdx.x);
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x, buf ^= 1) {
        double* Xe = smem + buf * tile_doubles;
        double* Rb = Xe + (TS + 1) * SXE;
        unsigned long long* Mk = masks + buf * (SCPW * SNW);
        stage(Xe, Rb, Mk, tile);
        __syncthreads();
        // the buckets of the wave's components: one batch of independent reads, wave-uniform from here on
        unsigned long long mk[SCPW];
#pragma unroll
        for (int sl = 0; sl < SCPW; ++sl) mk[sl] = Mk[sl * SNW + wave];
#pragma unroll
        for (int sl = 0; sl < SCPW; ++sl) mk[sl] = uniform64(mk[sl]);
        __builtin_amdgcn_sched_barrier(0);           // (the 16 registers of the batch are free again before the prefetch takes its own)
        const uint32_t next = tile + gridDim.x;
        prefetch(next < n_tiles ? next : tile);      // the last iteration re-reads its own tile (discarded)
        __builtin_amdgcn_s_setprio(kMatrixPhasePriority);

        // operands of one step: the four lowest samples of `rem` (a bucket's remaining entries), of component c, are taken out
        // of it; lane group k4 takes its own. Entries past the end are the sentinel row: r = 0, x~ = 0
        const double* xlane = Xe + 4 * bq + i4;
        auto take_four = [&](unsigned long long& rem, int c, const double*& xr, const double*& rp) {
            const uint32_t s0 = take_lowest(rem), s1 = take_lowest(rem), s2 = take_lowest(rem), s3 = take_lowest(rem);
            const uint32_t four = s0 | s1 << 8 | s2 << 16 | s3 << 24;
            const uint32_t s = __builtin_amdgcn_ubfe(four, 8u * k4, 8u);   // scalar up to here; one bit-field extract per lane
            xr = xlane + s * SXE;
            rp = Rb + c + s * SRS;
        };
        // the first nonempty bucket at or behind slot J (none: an empty step)
        auto bucket_from = [&](auto J_, unsigned long long& rem, int& c) {
            constexpr int J = J_;
            rem = 0;
            c = 0;
#pragma unroll
            for (int j = SCPW - 1; j >= J; --j)
                if (mk[j]) {
                    rem = mk[j];
                    c = j * SNW + wave;
                }
        };

        double r, y[8];
        unsigned long long after;                    // the entries of the loaded step's bucket that lie behind that step
        {
            int c;
            const double *xr, *rp;
            bucket_from(std::integral_constant<int, 0>{}, after, c);
            take_four(after, c, xr, rp);
            r = *rp;
#pragma unroll
            for (int m = 0; m < 8; ++m) y[m] = xr[4 * m];
        }
        static_for<SCPW>([&](auto sl_) {
            constexpr int sl = sl_;
            // a nonempty bucket finds the operands of its first step loaded; each step loads the next one's -- this bucket's or
            // the first of the next nonempty one -- behind the MFMAs that free the registers
            // (every mask bit is scanned once: `after` is what take_four left of this bucket when it scheduled the loaded step)
            for (bool more = mk[sl] != 0; more;) {
                int c = sl * SNW + wave;
                more = after != 0;
                if (!more) bucket_from(std::integral_constant<int, sl + 1>{}, after, c);
                const double *xr, *rp;
                take_four(after, c, xr, rp);
                const double ry0 = r * y[0], ry1 = r * y[4];
                acc[sl][9] += ry0;                   // sum r x~ and sum r: the lane group's own entry, on the vector unit
                acc[sl][10] += ry1;
                acc[sl][11] += r;
#pragma unroll
                for (int dl = 0; dl < 4; ++dl) acc[sl][dl] = __builtin_amdgcn_mfma_f64_4x4x4f64(y[dl], ry0, acc[sl][dl], 0, 0, 0);
                acc[sl][8] = __builtin_amdgcn_mfma_f64_4x4x4f64(y[4], ry0, acc[sl][8], 0, 0, 0);
                r = *rp;
#pragma unroll
                for (int m = 0; m < 4; ++m) y[m] = xr[4 * m];
#pragma unroll
                for (int dl = 0; dl < 4; ++dl)
                    acc[sl][4 + dl] = __builtin_amdgcn_mfma_f64_4x4x4f64(y[4 + dl], ry1, acc[sl][4 + dl], 0, 0, 0);
#pragma unroll
                for (int m = 4; m < 8; ++m) y[m] = xr[4 * m];
            }
        });
        __builtin_amdgcn_s_setprio(0);
    }
    if (nz_count && lane == 0) atomicAdd(nz_count, (unsigned long long)nonzero);   // (an integer sum: order-free)

    // ---- epilogue: partials[blockIdx.x][c][f]; D[b][i][j] of a step sits in lane 16i + 4b + j
    const int ri = lane >> 4, rj = lane & 3;
    const int f_lin = d * (d + 1) / 2;                // packed row d: sum r x (columns 0..d-1) and sum r (column d)
#pragma unroll
    for (int sl = 0; sl < SCPW; ++sl) {
        const int c = sl * SNW + wave;
        if (c >= K) continue;
        double* out = partials + ((size_t)blockIdx.x * KP + c) * FP;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int g = t < 8 ? t / 4 : 0, dl = t < 8 ? t % 4 : 4;
            const int Q = 4 * g + bq, P = (Q + dl) & 7;
            const int a = 4 * P + ri, b = 4 * Q + rj;
            if (a < d && b < d && (dl != 0 || a >= b)) {
                const int hi = a > b ? a : b, lo = a > b ? b : a;
                out[hi * (hi + 1) / 2 + lo] = acc[sl][t];
            }
        }
        // sum r x~ (two coordinate halves) and sum r: lane group k4 holds the partial sum over its own entries; the four groups
        // are added in the fixed order 0, 1, 2, 3 (every lane ends up with the total)
        double lin[3];
#pragma unroll
        for (int h = 0; h < 3; ++h) {
            const double v = acc[sl][9 + h];
            lin[h] = ((__shfl(v, lane & 15) + __shfl(v, (lane & 15) + 16)) + __shfl(v, (lane & 15) + 32)) + __shfl(v, (lane & 15) + 48);
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int b = 4 * (bq + 4 * h) + rj;
            if (ri == 0 && b < d) out[f_lin + b] = lin[h];
        }
        if (lane == 0) out[f_lin + d] = lin[2];
    }
}

}  // namespace
}  // namespace mstats

bool em_mstats_sparse_supported(int d, int K, int num_cus)
{
    return d <= kRegDim && K <= mstats::SCPW * mstats::SNW && em_mstats_self_norm_supported(d, K, num_cus);
}

int launch_em_mstats_sparse(const MstatsArgs& a, int num_cus, hipStream_t stream)
{
    using namespace mstats;
    if (a.mode != kFromLogRespSelfNorm || !em_mstats_sparse_supported(a.d, a.K, num_cus)) return -3;
    const Plan p = make_plan(a.d, a.K, num_cus);
    const uint32_t n_tiles = (a.n + TS - 1) / TS;
    int grid_x = num_cus < p.grid_x ? num_cus : p.grid_x;       // one workgroup per CU (the dense plan may have two)
    if ((uint32_t)grid_x > n_tiles) grid_x = (int)(n_tiles ? n_tiles : 1);
    if ((size_t)grid_x * p.KP * p.FP > a.partials_capacity || p.KP < a.K || p.FP < stats_count(a.d)) return -2;
    const size_t smem = sizeof(double) * (2 * ((size_t)(TS + 1) * SXE + (size_t)(TS + 1) * SRS) + 2 * SCPW * SNW);
    hipLaunchKernelGGL(em_mstats_sparse_kernel, dim3(grid_x), dim3(512), smem, stream, a.xt, a.ldx, a.n, a.d, padded_dim(a.d),
                       a.shift, a.lw, a.ldr, a.K, a.partials, p.KP, p.FP, a.lse_out, a.ll_out, a.nz_count);
    return grid_x;
}

}  // namespace mlhip
