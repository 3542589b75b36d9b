// SCREENED E-step (full covariance, FOLD, lw only, 12 <= D <= 32, K <= 64 -- the domain of em_mstats_sparse_kernel): a pass over an
// N x K log-responsibility block that an earlier pass left behind. From the stored value of a pair and four constants per component
// (em_screen_bound.hpp: formed from the block's parameter set and the new one) it bounds the pair's NEW value; a pair whose upper
// bound lies more than 746 below a lower bound of the sample's new maximum has a responsibility of exactly 0.0 whatever its true
// value is, and only its bound is stored. The other pairs -- the candidates, ~4.4 of 64 per sample at the headline shape -- are
// evaluated with the dense kernel's arithmetic (em_estep_mfma4.hip, FOLD form) and get its bits.
//
// The tile size ST is a template parameter next to D (screen_tile<D>: one form per D, no switch at run time). ST = 256, one workgroup
// of eight waves per CU, is what every D is instantiated with; ST = 128 -- four waves, two 64-sample segments, wave w taking the
// components w, w + 4, ..., two workgroups per CU so that one's stage runs under the other's evaluation -- passes the same tests and
// was measured slower at D = 28 and 32 (DESIGN 3.3p "The pair": a record fetched twice as often, emptier groups, and no phase got
// shorter). Per tile of ST samples (three workgroup barriers per tile, none inside the component loop; written for ST = 256):
//   * stage: two threads serve a sample -- thread t and thread t + 256 hold the stored values of components 0 .. 31 and 32 .. 63 of
//     sample t & 255, their half of the sample's exactness word (bit k: the stored value of component k is an evaluated one, not a
//     bound; a dense pass marks the whole block with a launch argument instead of writing words) and half of its coordinates.
//     Lmax = the largest lower bound over the exact entries, the first maximum in ascending k -- each half's own, then combined
//     through LDS, the lower half winning a tie; a pair is a candidate unless ub < Lmax - 746 -- written so that a NaN is a
//     candidate --, and always when its stored value is not finite or at least 2^40 in magnitude, or when it gave Lmax.
//     Non-candidates store ub; the new exactness word is the candidate word, written as its two 32-bit halves. x - shift of the
//     sample goes to an LDS tile. The loads of a workgroup's NEXT tile (its stored values and words; at D <= 24 its coordinates too)
//     are issued before the component loop and land under it.
//   * buckets, in the loop that decides the candidates: one ballot per component and 64-sample segment (the four waves of a half);
//     a candidate lane writes its sample index into the component's list of its segment at the rank the ballot gives it (ascending
//     sample order, the same in every run); lane kk of the wave collects component kk's count and the wave stores its <= 32 counts
//     with one LDS write.
//   * evaluate: wave w takes the components w, w + 8, ...; its record sits in an LDS slot of the wave's own, the next one is fetched
//     into registers meanwhile and copied in when the wave is done with the slot (wave-level ordering only); 16 bucket entries per
//     group are gathered from the tile into the B operand of v_mfma_f64_4x4x4_4b (lane layout as
//     in em_estep_mfma4.hip) and run through the dense kernel's chain: y_{4R+i} over C = 0 .. R ascending from the initialiser
//     -W (mu - s), a_i = fma(y, y, a_i) over R ascending from 0, q = (a_0 + a_1) + (a_2 + a_3), lw = fma(-0.5, q, coef). Entries past
//     the end of a bucket read the sentinel row behind the tile and store nothing. A step takes 32 entries of the bucket as TWO
//     groups that share each read of the record and run as two accumulator chains; a step with at most 16 entries left runs one
//     group. The record's reads of row quad R + 1 are issued before the matrix instructions of row quad R (scheduling fences keep
//     them there), an entry's segment is found without a branch, and the two cross-lane adds of q are v_permlane16_swap and
//     v_permlane32_swap, not trips through LDS. The next tile's coordinates a tile ahead at D = 28 and 32 fit the registers in this
//     form and were measured slower; they stay loaded at the head of their own tile (DESIGN 3.3p "Two groups a step").
// The constants kernel (one wave per component) also counts the components whose bound carries no information; the runtime reads the
// count and runs the dense kernel instead when it is not 0 (runtime/em.cpp).
#include "device.hpp"
#include "em_screen_bound.hpp"
#include <type_traits>

namespace mlhip {
namespace {

/// The tile: ST samples, two threads per sample, ST / 64 segments of 64 samples x two component halves = ST / 32 waves. 256 / ST
/// workgroups share a CU (two waves per SIMD in either form); screen_tile<D> below picks the form per dimension.
template <int ST> struct ScreenTile {
    static_assert(ST == 128 || ST == 256, "one or two workgroups per CU");
    static constexpr int NT = 2 * ST;        // threads per workgroup: two per sample
    static constexpr int NSEG = ST / 64;     // 64-sample segments
    static constexpr int NW = NT / 64;       // waves
    static constexpr int PER_CU = 256 / ST;  // workgroups resident on a CU
};
constexpr int SKH = 32;            // components per half
constexpr int SXS = 33;            // odd row stride of the x tile
constexpr int SKMAX = 64;          // components
constexpr int SDMAX = 32;          // dimensions

template <int D> struct ScreenBlocks {
    static constexpr int Q = D / 4;
    static constexpr int NB = Q * (Q + 1) / 2;
    static constexpr int PS = NB * 16 + 2 * D + 1;                       // layout.hpp estep_mfma4_param_stride
    static constexpr int slot(int R, int C) { return C * Q - C * (C - 1) / 2 + (R - C); }   // column-quad major
};

/// v + (v of lane ^ 16) on every lane, without a trip through LDS: v_permlane16_swap leaves rows 0, 0, 2, 2 of v in one register and
/// rows 1, 1, 3, 3 in the other (a row: 16 lanes). The even row's value is the left operand, as in v + __shfl_xor(v, 16) on an even row.
__device__ inline double rows_sum(double v)
{
    const unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
    const auto l = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
    const auto h = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
    return __hiloint2double((int)h[0], (int)l[0]) + __hiloint2double((int)h[1], (int)l[1]);
}

/// v + (v of lane ^ 32) on every lane: v_permlane32_swap leaves the lower half of v twice in one register, the upper half in the other.
__device__ inline double halves_sum(double v)
{
    const unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
    const auto l = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
    const auto h = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
    return __hiloint2double((int)h[0], (int)l[0]) + __hiloint2double((int)h[1], (int)l[1]);
}

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

/// LDS of a workgroup, in bytes: the x tile and its sentinel row, a record slot per wave, the two halves' maxima, the segment counts
/// and the bucket lists.
template <int D, int ST> constexpr size_t screen_lds_bytes()
{
    using T = ScreenTile<ST>;
    return sizeof(double) * ((size_t)(ST + 1) * SXS +(size_t)T::NW * ScreenBlocks<D>::PS + 2 * ST) + sizeof(int) * 2 * ST +
           sizeof(unsigned) * T::NSEG * SKMAX + (size_t)SKMAX * ST;
}
static_assert(2 * screen_lds_bytes<SDMAX, 128>() <= 160 * 1024, "two 128-sample workgroups share a CU's LDS");

/// PROF: thread 0 stamps the 100 MHz clock at the phase boundaries of the workgroup's second tile (kScreenStamps slots per workgroup:
/// 0 tile start, 1 end of stage -- the sample's maximum is known --, 2 end of the candidate-and-bucket loop, the tile's stores and their barrier, 3 + 2j / 4 + 2j wave 0's j-th record copied / evaluated (j < kScreenStampRounds),
/// kScreenStampLoopEnd wave 0 out of the component loop, kScreenStampTileEnd end of tile). The normal instantiation has no stamp in it.
/// The second launch bound pins two waves per SIMD (256 registers a lane) in either form: a 256-thread workgroup alone would be
/// given 512, and a second workgroup would then not fit next to it.
template <int D, int ST, bool PROF>
__global__ __launch_bounds__(2 * ST, 2) void em_estep_screen_kernel(
    const double* __restrict__ xt, size_t ldx, uint32_t n, uint32_t n_tiles, const double* __restrict__ params, int K,
    const double* __restrict__ shift, const double* __restrict__ consts, double* __restrict__ lw, size_t ldr,
    unsigned* __restrict__ exact, int all_exact, unsigned long long* __restrict__ cand_count, unsigned long long* __restrict__ prof)
{
    using B = ScreenBlocks<D>;
    using T = ScreenTile<ST>;
    constexpr int Q = B::Q, NB = B::NB, PS = B::PS;
    constexpr int SNW = T::NW, NSEG = T::NSEG;
    constexpr int NLD = (PS + 63) / 64;              // doubles of a record each lane moves to the wave's slot
    constexpr int DH = D / 2;                        // coordinates a thread stages
    constexpr bool PFX = D <= 24;                    // the next tile's coordinates are loaded a tile ahead like its stored values (at D = 28, 32 measured slower: DESIGN 3.3p)
    extern __shared__ __attribute__((aligned(16))) double smem[];
    double* Xs = smem;                               // [ST + 1][SXS]: x - shift, sample-major; row ST: the sentinel
    double* recs = Xs + (ST + 1) * SXS;              // [SNW][PS]: a record slot per wave
    double* xL = recs + SNW * PS;                    // [2][ST]: each half's largest lower bound ...
    int* xk = reinterpret_cast<int*>(xL + 2 * ST);   // [2][ST]: ... and the component that gave it
    unsigned* cnt = reinterpret_cast<unsigned*>(xk + 2 * ST);            // [NSEG][SKMAX]: entries of a component's list per segment
    unsigned char* list = reinterpret_cast<unsigned char*>(cnt + NSEG * SKMAX);   // [SKMAX][NSEG][64]: candidate samples (tile index), ascending
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = wave / NSEG, seg = wave % NSEG; // the thread's components half * 32 .. half * 32 + 31, its sample's segment
    const int kbase = half * SKH;
    const int sl = tid & (ST - 1);                   // the thread's sample in the tile
    const int g = lane >> 4, s = lane & 15;
    const int aoff = g * 4 + (lane & 3);             // A operand: entry [k = lane >> 4][i = lane & 3] of a 16-double block
    if (tid < SXS) Xs[ST * SXS + tid] = 0.0;
    unsigned long long n_cand = 0;
    double* __restrict__ rec = recs + wave * PS;

    auto stamp = [&](uint32_t tile, int slot) {
        if constexpr (PROF) {
            if (tid == 0 && tile == blockIdx.x + gridDim.x) prof[(size_t)blockIdx.x * kScreenStamps + slot] = wall_clock64();
        }
    };
    // the registers a tile is staged from: the half's stored values, its half of the exactness word, half of the coordinates
    double v[SKH], xs[DH];
    unsigned ex = 0;
    // (rows are addressed by a pointer that moves a row on, one 64-bit add each: a row offset formed per component is a scalar
    // product kept in a lane of a spill register and read back for every use)
    auto load_x = [&](uint32_t tile) {
        const double* p = xt + (size_t)(half * DH) * ldx + (tile * ST + sl);   // sample < n_pad: always inside the allocations
#pragma unroll
        for (int j = 0; j < DH; ++j, p += ldx) xs[j] = *p;
    };
    auto load_v = [&](uint32_t tile) {
        const uint32_t i = tile * ST + sl;
        ex = all_exact ? ~0u : exact[2 * (size_t)i + half];
        if (kbase < K) {
            const double* p = lw + (size_t)kbase * ldr + i;              // components past K - 1 read row K - 1 again (never used)
#pragma unroll
            for (int kk = 0; kk < SKH; ++kk) {
                v[kk] = *p;
                if (kbase + kk + 1 < K) p += ldr;
            }
        }
    };
    double stg[NLD];
    auto fetch = [&](int k) {
#pragma unroll
        for (int it = 0; it < NLD; ++it) stg[it] = params[(size_t)k * PS + min(lane + 64 * it, PS - 1)];
    };

    if (blockIdx.x < n_tiles) {
        if (PFX) load_x(blockIdx.x);
        load_v(blockIdx.x);
    }
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t i = tile * ST + sl;
        stamp(tile, 0);
        // ---- stage
        if (!PFX) load_x(tile);
        double Lmax = -HUGE_VAL;
        int kmax = -1;
#pragma unroll
        for (int kk = 0; kk < SKH; ++kk) {
            const int k = kbase + kk;
            if (k < K) {
                const double lb = __builtin_fma(consts[4 * k + 2], v[kk], consts[4 * k + 3]);
                const bool usable = ((ex >> kk) & 1) && fabs(v[kk]) < screen::kMaxStored;    // (NaN, inf: not usable)
                if (usable && lb > Lmax) { Lmax = lb; kmax = k; }
            }
        }
        xL[half * ST + sl] = Lmax;
        xk[half * ST + sl] = kmax;
        __syncthreads();
        {
            // the first maximum in ascending k: the upper half's only where it is larger
            const double oL = xL[(half ^ 1) * ST + sl];
            const int ok = xk[(half ^ 1) * ST + sl];
            const bool other = half == 0 ? oL > Lmax : !(Lmax > oL);
            if (other) { Lmax = oL; kmax = ok; }
        }
        const double limit = Lmax - screen::kSkipMargin;
        stamp(tile, 1);
        // ---- candidates and buckets, one loop: the component's candidate lanes are balloted where they are decided
        unsigned cand = 0, counts = 0;               // counts: lane kk holds the entries of component kbase + kk in this segment
        // what the wave shares, kept per lane (from tid, not from the wave's scalars): the unrolled loop then compares and addresses
        // with immediates off one register each, where a scalar per component would sit in a lane of a spill register
        const int krel = kmax - (tid / ST) * SKH;    // the maximum's component relative to the half (never a kk when it is the other half's, or none)
        const unsigned lbase = (unsigned)(((tid / ST) * SKH * NSEG + (tid >> 6) % NSEG) * 64);   // list of component kbase, this segment
        double* ps = lw + (size_t)kbase * ldr + i;   // the sample's stored value of component kbase + kk
#pragma unroll
        for (int kk = 0; kk < SKH; ++kk) {
            const int k = kbase + kk;
            if (k < K) {
                const double ub = __builtin_fma(consts[4 * k + 0], v[kk], consts[4 * k + 1]);
                const bool skip = ub < limit && fabs(v[kk]) < screen::kMaxStored && kk != krel;   // (a NaN anywhere: a candidate)
                if (skip) *ps = ub;
                ps += ldr;
                cand |= (skip ? 0u : 1u) << kk;
                const unsigned long long b = __builtin_amdgcn_ballot_w64(!skip);
                // the candidate's place: the list's offset plus its rank among the segment's candidates (ascending sample order)
                const unsigned at = __builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, lbase));
                if (!skip) list[kk * NSEG * 64 + at] = (unsigned char)sl;   // < (k * NSEG + seg) * 64 + 64
                counts = lane == kk ? (unsigned)__popcll(b) : counts;
            }
        }
        if (lane < SKH && kbase + lane < K) cnt[seg * SKMAX + kbase + lane] = counts;   // the wave's counts in one write
        exact[2 * (size_t)i + half] = cand;
        if (i < n) n_cand += (unsigned long long)__popc(cand);
#pragma unroll
        for (int j = 0; j < DH; ++j) Xs[sl * SXS + half * DH + j] = xs[j] - shift[half * DH + j];
        const int kfirst = wave;
        if (kfirst < K) fetch(kfirst);
        // the next tile's loads land under the component loop (v, xs and ex are free from here on)
        if (tile + gridDim.x < n_tiles) {
            if (PFX) load_x(tile + gridDim.x);
            load_v(tile + gridDim.x);
        }
        __syncthreads();                             // the tile, the lists and the counts are written
        stamp(tile, 2);
        // ---- evaluate
        for (int k = kfirst, j = 0; k < K; k += SNW, ++j) {
            // the wave's slot: nobody else reads or writes it, so the wave's own order is all that has to hold
#pragma unroll
            for (int it = 0; it < NLD; ++it)
                if (lane + 64 * it < PS) rec[lane + 64 * it] = stg[it];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            if (wave == 0 && j < kScreenStampRounds) stamp(tile, 3 + 2 * j);
            if (k + SNW < K) fetch(k + SNW);
            // the ends of the segment lists in the component's bucket (NSEG = 2: c1 and c2 are the total, no entry reaches them)
            const unsigned c0 = cnt[k], c1 = c0 + cnt[SKMAX + k];
            const unsigned c2 = NSEG == 4 ? c1 + cnt[(NSEG - 2) * SKMAX + k] : c1, total = NSEG == 4 ? c2 + cnt[(NSEG - 1) * SKMAX + k] : c1;
            const double coef = rec[NB * 16 + 2 * D];
            // A step of NG groups: lane s of lane group g serves the entries first + 16 i + s, i < NG. The groups share every read of the
            // record and run as NG accumulator chains. The record's reads run one row quad ahead of the matrix instructions that use
            // them, between scheduling fences: left to itself the compiler reads the whole record first, and two groups' operands
            // beside it do not fit the registers (DESIGN 3.3p "Two groups a step").
            auto step = [&](unsigned first, auto groups) {
                constexpr int NG = decltype(groups)::value;
                double a[Q][Q], ini[Q];
                auto load_quad = [&](int R) {
                    ini[R] = rec[NB * 16 + D + 4 * R + g];               // -W (mu - shift), rows 4R .. 4R + 3
#pragma unroll
                    for (int C = 0; C <= R; ++C) a[R][C] = rec[B::slot(R, C) * 16 + aoff];
                };
                load_quad(0);
                bool valid[NG];
                unsigned smp[NG];
                double xb[NG][Q], qs[NG];
#pragma unroll
                for (int i = 0; i < NG; ++i) {
                    const unsigned e = first + 16u * i + s;
                    valid[i] = e < total;
                    // the entry's segment (< NSEG when valid) and where that segment starts in the bucket, without a branch
                    const unsigned w = (e >= c0 ? 1u : 0u) + (e >= c1 ? 1u : 0u) + (e >= c2 ? 1u : 0u);
                    unsigned base = e >= c0 ? c0 : 0u;
                    base = e >= c1 ? c1 : base;
                    base = e >= c2 ? c2 : base;
                    const unsigned at = ((unsigned)k * NSEG + (w & (NSEG - 1))) * 64 + ((e - base) & 63u);   // inside the component's lists
                    smp[i] = valid[i] ? (unsigned)list[at] : (unsigned)ST;
                    const double* xrow = Xs + smp[i] * SXS + g;
#pragma unroll
                    for (int C = 0; C < Q; ++C) xb[i][C] = xrow[4 * C];
                    qs[i] = 0.0;
                }
#pragma unroll
                for (int R = 0; R < Q; ++R) {
                    if (R + 1 < Q) load_quad(R + 1);
                    __builtin_amdgcn_sched_barrier(0);
                    double acc[NG];
#pragma unroll
                    for (int i = 0; i < NG; ++i) acc[i] = ini[R];
#pragma unroll
                    for (int C = 0; C <= R; ++C)
#pragma unroll
                        for (int i = 0; i < NG; ++i) acc[i] = __builtin_amdgcn_mfma_f64_4x4x4f64(a[R][C], xb[i][C], acc[i], 0, 0, 0);
#pragma unroll
                    for (int i = 0; i < NG; ++i) qs[i] = __builtin_fma(acc[i], acc[i], qs[i]);
                    __builtin_amdgcn_sched_barrier(0);
                }
#pragma unroll
                for (int i = 0; i < NG; ++i) {
                    // the four lane groups hold the four row residues a_0 .. a_3 of the same 16 samples: q = (a_0 + a_1) + (a_2 + a_3)
                    const double q = halves_sum(rows_sum(qs[i]));
                    if (valid[i] && g == 0) lw[(size_t)k * ldr + (size_t)tile * ST + smp[i]] = __builtin_fma(-0.5, q, coef);
                }
            };
            for (unsigned first = 0; first < total; first += 32) {
                if (total - first <= 16)                                 // (wave-uniform)
                    step(first, std::integral_constant<int, 1>{});       // a lone group: a second chain would be matrix work for nothing
                else
                    step(first, std::integral_constant<int, 2>{});
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // every lane is done with the slot before the next record goes in
            __builtin_amdgcn_wave_barrier();
            if (wave == 0 && j < kScreenStampRounds) stamp(tile, 4 + 2 * j);
        }
        stamp(tile, kScreenStampLoopEnd);
        __syncthreads();                             // the tile, the lists and the counts are free for the next tile
        stamp(tile, kScreenStampTileEnd);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n_cand += __shfl_down(n_cand, off, 64);
    if (cand_count && lane == 0) atomicAdd(cand_count, n_cand);          // (an integer sum: order-free)
}

/// The tile each dimension is instantiated with -- one form per D, no switch at run time (the measurements: DESIGN 3.3p, "The pair").
template <int D> constexpr int screen_tile = 256;

template <int D> int launch_d(const ScreenArgs& a, int num_cus, hipStream_t stream)
{
    constexpr int ST = screen_tile<D>;
    using T = ScreenTile<ST>;
    static_assert(kSampleTile % ST == 0, "a block is a whole number of tiles");
    static_assert(T::PER_CU * screen_lds_bytes<D, ST>() <= 160 * 1024, "the CU's workgroups share its LDS");
    const uint32_t n_tiles = padded_samples(a.n) / ST;
    uint32_t grid = (uint32_t)(T::PER_CU * num_cus); // what is resident at once: two waves per SIMD, the CU's LDS
    if (grid > n_tiles) grid = n_tiles;
    unsigned* exact = reinterpret_cast<unsigned*>(a.exact);              // word i as its halves 2i (components 0 .. 31) and 2i + 1
    constexpr size_t lds = screen_lds_bytes<D, ST>();
    if (a.profile)
        hipLaunchKernelGGL((em_estep_screen_kernel<D, ST, true>), dim3(grid), dim3(T::NT), lds, stream, a.xt, a.ldx,
                           a.n, n_tiles, a.params, a.K, a.shift, a.consts, a.lw, a.ldr, exact, a.all_exact, a.cand_count, a.profile);
    else
        hipLaunchKernelGGL((em_estep_screen_kernel<D, ST, false>), dim3(grid), dim3(T::NT), lds, stream, a.xt, a.ldx,
                           a.n, n_tiles, a.params, a.K, a.shift, a.consts, a.lw, a.ldr, exact, a.all_exact, a.cand_count, nullptr);
    return (int)grid;
}

template <int D> int tile_d() { return screen_tile<D>; }

}  // namespace

bool em_estep_screen_supported(int D, int K) { return D >= 12 && D <= SDMAX && D % 4 == 0 && K >= 1 && K <= SKMAX; }

/// Where the runtime takes the screened pass by itself: the shapes at which it was measured faster than the dense one on three
/// alternating runs each, by more than both spreads (profiles/estep_screen_tile_ab.txt: D = 32, K = 64, E-step 11.3 -> 6.0 ms at
/// N = 10M; D = 28, K = 64, 4.69 -> 3.89 ms at N = 5M). Its time grows with the candidates per sample, which at a smaller d are more,
/// while the dense kernel's falls with d^2 and K: at N = 5M, K = 64, D = 24 and 16 give 3.60 -> 4.40 and 1.92 -> 5.04 ms, D = 24,
/// K = 32 1.81 -> 2.73 ms, D = 32, K = 16 1.51 -> 1.46 ms (inside the spreads). D = 32, K = 32 gains (2.90 -> 2.16 ms) and stays
/// dense until tests/test_gpu_estep_screen.py's test_automatic_route, which fixes it, changes. Elsewhere only MLHIP_ESTEP_SCREEN=1 screens.
/// With the merged candidate and bucket loop (profiles/estep_screen_pair_ab.txt) D = 32, K = 16 meets the criterion too (1.53 -> 1.31 ms);
/// it is not routed yet.
bool em_estep_screen_preferred(int D, int K) { return (D == 32 || D == 28) && K == SKMAX; }

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

int em_estep_screen_tile(int D)
{
    switch (D) {
    case 12: return tile_d<12>();
    case 16: return tile_d<16>();
    case 20: return tile_d<20>();
    case 24: return tile_d<24>();
    case 28: return tile_d<28>();
    case 32: return tile_d<32>();
    default: return -1;
    }
}

}  // namespace mlhip
