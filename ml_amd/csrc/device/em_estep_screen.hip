// SCREENED E-step (full covariance, FOLD, lw only, 12 <= D <= 32, K <= 64 -- the domain of em_mstats_sparse_kernel): a pass over an
// N x K log-responsibility block that an earlier pass left behind. From the stored value of a pair and four constants per component
// (em_screen_bound.hpp: formed from the block's parameter set and the new one) it bounds the pair's NEW value; a pair whose upper
// bound lies more than 746 below a lower bound of the sample's new maximum has a responsibility of exactly 0.0 whatever its true
// value is, and only its bound is stored. The other pairs -- the candidates, ~4.4 of 64 per sample at the headline shape -- are
// evaluated with the dense kernel's arithmetic (em_estep_mfma4.hip, FOLD form) and get its bits.
//
// Per tile of ST = 128 samples, one workgroup of two waves:
//   * stage: thread t holds sample t's K stored values and the sample's exactness word (bit k: the stored value of component k is an
//     evaluated one, not a bound; a dense pass marks the whole block with a launch argument instead of writing words). Lmax = the
//     largest lower bound over the exact entries; a pair is a candidate unless ub < Lmax - 746 -- written so that a NaN is a
//     candidate --, and always when its stored value is not finite or at least 2^40 in magnitude, or when it gave Lmax.
//     Non-candidates store ub; the new exactness word is the candidate word. x - shift of the sample goes to an LDS tile.
//   * buckets: one ballot per component; a candidate lane writes its sample index into the component's list of its wave at the
//     rank the ballot gives it (ascending sample order, the same in every run).
//   * evaluate: wave w takes the components 2r + w, r = 0, 1, ... (their records staged in LDS a round ahead, as the dense kernel
//     stages them); 16 bucket entries per group are gathered from the tile into the B operand of v_mfma_f64_4x4x4_4b (lane layout as
//     in em_estep_mfma4.hip) and run through the dense kernel's chain: y_{4R+i} over C = 0 .. R ascending from the initialiser
//     -W (mu - s), a_i = fma(y, y, a_i) over R ascending from 0, q = (a_0 + a_1) + (a_2 + a_3), lw = fma(-0.5, q, coef). Entries past
//     the end of a bucket read the sentinel row behind the tile and store nothing.
// The constants kernel (one wave per component) also counts the components whose bound carries no information; the runtime reads the
// count and runs the dense kernel instead when it is not 0 (runtime/em.cpp).
#include "device.hpp"
#include "em_screen_bound.hpp"

namespace mlhip {
namespace {

constexpr int ST = 128;            // samples per tile = threads per workgroup
constexpr int SXS = 33;            // odd row stride of the x tile
constexpr int SKMAX = 64;          // components
constexpr int SDMAX = 32;          // dimensions

template <int D> struct ScreenBlocks {
    static constexpr int Q = D / 4;
    static constexpr int NB = Q * (Q + 1) / 2;
    static constexpr int PS = NB * 16 + 2 * D + 1;                       // layout.hpp estep_mfma4_param_stride
    static constexpr int slot(int R, int C) { return C * Q - C * (C - 1) / 2 + (R - C); }   // column-quad major
};

/// One wave per component: the dense lower triangles of W (old) and W' (new) out of the two records, row i of M = W' L on lane i.
__global__ __launch_bounds__(64) void em_screen_constants_kernel(const double* __restrict__ rec_old, const double* __restrict__ rec_new,
                                                                 int d, int D, double* __restrict__ consts,
                                                                 unsigned* __restrict__ no_info)
{
    __shared__ double Wo[SDMAX * SXS], Wn[SDMAX * SXS], Mr[SDMAX * SXS], mu_o[SDMAX], mu_n[SDMAX];
    const int k = blockIdx.x, lane = threadIdx.x;
    const int Q = D / 4, NB = Q * (Q + 1) / 2, PS = NB * 16 + 2 * D + 1;
    const double* ro = rec_old + (size_t)k * PS;
    const double* rn = rec_new + (size_t)k * PS;
    for (int e = lane; e < NB * 16; e += 64) {
        const int t = e >> 4, kk = (e >> 2) & 3, i = e & 3;
        int C = 0;
        while (C + 1 < Q && (C + 1) * Q - (C + 1) * C / 2 <= t) ++C;
        const int R = C + (t - (C * Q - C * (C - 1) / 2));
        const int row = 4 * R + i, col = 4 * C + kk;                     // entry [k][i] of block (R, C) = W[4R + i][4C + k]
        Wo[row * SXS + col] = ro[e];
        Wn[row * SXS + col] = rn[e];
    }
    if (lane < D) {
        mu_o[lane] = ro[NB * 16 + lane];
        mu_n[lane] = rn[NB * 16 + lane];
    }
    __syncthreads();
    double f2 = 0.0, m2 = 0.0, g2 = 0.0, wmin = HUGE_VAL, wmax = 0.0;
    if (lane < d) {
        const screen::RowTerms t = screen::row_terms(lane, Wo, Wn, SXS, mu_o, mu_n, Mr + lane * SXS, 1);
        f2 = t.f2; m2 = t.m2;
        const double g = fabs(t.c) + screen::kOutward * t.cabs;
        g2 = g * g;
        wmin = wmax = fabs(Wo[lane * SXS + lane]);
    }
    // fixed-order sums over the lanes (the same constants on every device)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        f2 += __shfl_down(f2, off, 64);
        m2 += __shfl_down(m2, off, 64);
        g2 += __shfl_down(g2, off, 64);
        const double lo = __shfl_down(wmin, off, 64), hi = __shfl_down(wmax, off, 64);
        wmin = lo < wmin || lo != lo ? lo : wmin;                       // (a NaN wins: no information)
        wmax = hi > wmax || hi != hi ? hi : wmax;
    }
    if (lane == 0) {
        double out[4];
        const bool ok = screen::constants(d, f2, m2, g2, ro[NB * 16 + 2 * D], rn[NB * 16 + 2 * D], wmin, wmax, out);
        consts[4 * k + 0] = out[0]; consts[4 * k + 1] = out[1]; consts[4 * k + 2] = out[2]; consts[4 * k + 3] = out[3];
        if (!ok) atomicAdd(no_info, 1u);
    }
}

template <int D>
__global__ __launch_bounds__(ST) void em_estep_screen_kernel(
    const double* __restrict__ xt, size_t ldx, uint32_t n, uint32_t n_tiles, const double* __restrict__ params, int K,
    const double* __restrict__ shift, const double* __restrict__ consts, double* __restrict__ lw, size_t ldr,
    unsigned long long* __restrict__ exact, int all_exact, unsigned long long* __restrict__ cand_count)
{
    using B = ScreenBlocks<D>;
    constexpr int Q = B::Q, NB = B::NB, PS = B::PS;
    constexpr int NLD = (2 * PS + ST - 1) / ST;      // doubles of a round's two records each thread moves to LDS
    __shared__ double Xs[(ST + 1) * SXS];            // x - shift, sample-major; row ST: the sentinel
    __shared__ double recs[2 * PS];                  // the round's two records
    __shared__ unsigned char list[2][SKMAX][64];     // [wave][component]: the wave's candidate samples (tile index), ascending
    __shared__ unsigned cnt[2][SKMAX];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, s = lane & 15;
    const int aoff = g * 4 + (lane & 3);             // A operand: entry [k = lane >> 4][i = lane & 3] of a 16-double block
    if (tid < SXS) Xs[ST * SXS + tid] = 0.0;
    unsigned long long n_cand = 0;
    const int rounds = (K + 1) / 2;

    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t i = tile * ST + tid;          // < n_pad: always inside the allocations
        // ---- stage
#pragma unroll
        for (int j = 0; j < D; ++j) Xs[tid * SXS + j] = xt[(size_t)j * ldx + i] - shift[j];
        const unsigned long long ex = all_exact ? ~0ull : exact[i];
        double v[SKMAX];
#pragma unroll
        for (int k = 0; k < SKMAX; ++k) v[k] = lw[(size_t)(k < K ? k : K - 1) * ldr + i];
        double Lmax = -HUGE_VAL;
        int kmax = -1;
#pragma unroll
        for (int k = 0; k < SKMAX; ++k) {
            if (k < K) {
                const double lb = __builtin_fma(consts[4 * k + 2], v[k], consts[4 * k + 3]);
                const bool usable = ((ex >> k) & 1) && fabs(v[k]) < screen::kMaxStored;      // (NaN, inf: not usable)
                if (usable && lb > Lmax) { Lmax = lb; kmax = k; }
            }
        }
        const double limit = Lmax - screen::kSkipMargin;
        unsigned long long cand = 0;
#pragma unroll
        for (int k = 0; k < SKMAX; ++k) {
            if (k < K) {
                const double ub = __builtin_fma(consts[4 * k + 0], v[k], consts[4 * k + 1]);
                const bool skip = ub < limit && fabs(v[k]) < screen::kMaxStored && k != kmax;   // (a NaN anywhere: a candidate)
                if (skip) lw[(size_t)k * ldr + i] = ub;
                else cand |= 1ull << k;
            }
        }
        exact[i] = cand;
        if (i < n) n_cand += (unsigned long long)__popcll(cand);
        // ---- buckets
        for (int k = 0; k < K; ++k) {
            const bool c = (cand >> k) & 1;
            const unsigned long long b = __ballot(c);
            const unsigned rank = __builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
            if (c) list[wave][k][rank] = (unsigned char)tid;
            if (lane == 0) cnt[wave][k] = (unsigned)__popcll(b);
        }
        // ---- evaluate
        double stg[NLD];
        // (the two records of a round are contiguous: element e of the pair sits at 2 r PS + e; past the last record -- K odd, the last
        // round -- the first of the pair is read once more, nobody uses it)
        auto fetch = [&](int r) {
            const int base = 2 * r * PS, last = K * PS;
#pragma unroll
            for (int it = 0; it < NLD; ++it) {
                int e = base + min(tid + ST * it, 2 * PS - 1);
                e = e < last ? e : e - PS;
                stg[it] = params[e];
            }
        };
        fetch(0);
        for (int r = 0; r < rounds; ++r) {
            __syncthreads();                         // the buckets are written (r = 0); every wave is done with round r - 1's records
#pragma unroll
            for (int it = 0; it < NLD; ++it)
                if (tid + ST * it < 2 * PS) recs[tid + ST * it] = stg[it];
            __syncthreads();
            if (r + 1 < rounds) fetch(r + 1);
            const int k = 2 * r + wave;
            if (k >= K) continue;
            const double* __restrict__ rec = recs + wave * PS;
            const unsigned c0 = cnt[0][k], total = c0 + cnt[1][k];
            const double coef = rec[NB * 16 + 2 * D];
            for (unsigned first = 0; first < total; first += 16) {
                const unsigned e = first + s;
                const bool valid = e < total;
                const unsigned w = e >= c0 ? 1u : 0u;
                const unsigned pos = valid ? e - (w ? c0 : 0u) : 0u;      // < 64: a wave's list holds at most its 64 samples
                const unsigned smp = valid ? (unsigned)list[w][k][pos & 63u] : (unsigned)ST;
                const double* xrow = Xs + smp * SXS + g;
                double xb[Q];
#pragma unroll
                for (int C = 0; C < Q; ++C) xb[C] = xrow[4 * C];
                double qs = 0.0;
#pragma unroll
                for (int R = 0; R < Q; ++R) {
                    double acc = rec[NB * 16 + D + 4 * R + g];            // -W (mu - shift), rows 4R .. 4R + 3
#pragma unroll
                    for (int C = 0; C <= R; ++C)
                        acc = __builtin_amdgcn_mfma_f64_4x4x4f64(rec[B::slot(R, C) * 16 + aoff], xb[C], acc, 0, 0, 0);
                    qs = __builtin_fma(acc, acc, qs);
                }
                // the four lane groups hold the four row residues a_0 .. a_3 of the same 16 samples: q = (a_0 + a_1) + (a_2 + a_3)
                const double t = qs + __shfl_xor(qs, 16, 64);
                const double q = t + __shfl_xor(t, 32, 64);
                if (valid && g == 0) lw[(size_t)k * ldr + (size_t)tile * ST + smp] = __builtin_fma(-0.5, q, coef);
            }
        }
        __syncthreads();                             // the tile, the lists and the counts are free for the next tile
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n_cand += __shfl_down(n_cand, off, 64);
    if (cand_count && lane == 0) atomicAdd(cand_count, n_cand);          // (an integer sum: order-free)
}

template <int D> int launch_d(const ScreenArgs& a, int num_cus, hipStream_t stream)
{
    const uint32_t n_tiles = padded_samples(a.n) / ST;
    uint32_t grid = (uint32_t)num_cus * 3;
    if (grid > n_tiles) grid = n_tiles;
    hipLaunchKernelGGL(em_estep_screen_kernel<D>, dim3(grid), dim3(ST), 0, stream, a.xt, a.ldx, a.n, n_tiles, a.params, a.K, a.shift,
                       a.consts, a.lw, a.ldr, a.exact, a.all_exact, a.cand_count);
    return (int)grid;
}

}  // namespace

static_assert(kSampleTile % ST == 0, "a block is a whole number of tiles");

bool em_estep_screen_supported(int D, int K) { return D >= 12 && D <= SDMAX && D % 4 == 0 && K >= 1 && K <= SKMAX; }

/// Where the runtime takes the screened pass by itself: the shape at which it was measured faster than the dense one on repeated
/// alternating runs (profiles/estep_screen_ab.txt: D = 32, K = 64, E-step 11.2 -> 8.95 ms at N = 10M). Its time hardly depends on d --
/// it is bound by its rounds, one per two components --, the dense kernel's falls with d^2 and K: single runs at N = 5M
/// (profiles/estep_screen_sweep.txt) give D = 32: K = 32 2.95 -> 2.67 ms (not relied on before it is repeated), K = 16 1.54 -> 1.78 ms;
/// K = 64: D = 28, 24, 16 4.73 -> 5.35, 3.67 -> 6.06, 1.95 -> 6.22 ms. Elsewhere only MLHIP_ESTEP_SCREEN=1 screens.
bool em_estep_screen_preferred(int D, int K) { return D == 32 && K == SKMAX; }

void launch_em_screen_constants(const double* rec_old, const double* rec_new, int K, int d, int D, double* consts,
                                unsigned* no_info, hipStream_t stream)
{
    hipLaunchKernelGGL(em_screen_constants_kernel, dim3(K), dim3(64), 0, stream, rec_old, rec_new, d, D, consts, no_info);
}

int launch_em_estep_screen(const ScreenArgs& a, int num_cus, hipStream_t stream)
{
    if (!em_estep_screen_supported(a.D, a.K)) return -1;
    switch (a.D) {
    case 12: return launch_d<12>(a, num_cus, stream);
    case 16: return launch_d<16>(a, num_cus, stream);
    case 20: return launch_d<20>(a, num_cus, stream);
    case 24: return launch_d<24>(a, num_cus, stream);
    case 28: return launch_d<28>(a, num_cus, stream);
    case 32: return launch_d<32>(a, num_cus, stream);
    default: return -1;
    }
}

}  // namespace mlhip
