// Conditional CDF and quantiles of a Gaussian mixture for gfx950: under the mixture conditioned on x_O, coordinate j of x_M follows the
// one-dimensional mixture sum_k r_k N(t_kj, s_kj^2). From the log-responsibilities lw / lse an E-step kernel wrote for the MARGINAL
// mixture over the observed coordinates (exact form, with_lse = 1, fold = 0) and the table [mu_k,O | mu_k,M | A_k^T | s_k | w_k] per
// component -- the record of em_condition.hip with s_kj = sqrt(C_k[j][j]) and w_kj = 1 / s_kj behind it -- per row, on every tier:
//   both    z_c = x_c - mu_k,O[c]; t_j = mu_k,M[j], t_j = fma(A_k[j][c], z_c, t_j) for ascending c (component_prediction);
//           r_k = exp_nonpos(lw_k - lse); a component takes part ONLY where r_k != 0.
//   CDF     a = (v_j - t_kj) * w_kj;  F_j = fma(r_k, normal_cdf(a), F_j) for ascending k from F_j = +0.0.
//   quantile at probability p, z = normal_quantile(p) from the host:
//           S = the sequential sum of r_k for ascending k from +0.0 (em_condition_sample.hip's s_{K-1}); T = p * S;
//           q_k = fma(s_kj, z, t_kj); lo = min q_k, hi = max q_k (a NaN q_k makes both NaN), g = fma(r_k, q_k, g) from +0.0;
//           start: v = g / S clamped into [lo, hi] (it leaves it only by rounding; the ends included: a row with one dominant component
//           has its answer ON an end); where lo == hi (K = 1, a row with one share) the result is lo with 0 trips; NaN where lo or T
//           is NaN or no component has a share. The search's bracket is [lo - e, hi + e], e = 2^-50 max(|lo|, |hi|). Then trips
//           n = 1, 2, ...: F(v) as above and f(v) = sum_k fma(r_k, w_kj * normal_pdf(a), f);
//           F < T ? lo = v : hi = v;  the Newton candidate c, on the logarithm of the nearer tail: T + T < S (or == S and F < T):
//           c = v + log(T / F) (F / f), else c = v - log((S - T) / (S - F)) ((S - F) / f);
//           next = c if n <= kNewtonTrips and lo < c < hi, else lo + (hi - lo) / 2;
//           STOP, keeping v, if |F - T| <= 2^-50 T (the sum of normal_cdf values is no more accurate than that), or |c - v| <= 2^-51 |v|
//           (the step is below v's own rounding), or next is not strictly inside (lo, hi) (the bracket has no double left to try), or
//           n == kQuantileMaxTrips; else v = next.
//           The cap holds whatever the data: after kNewtonTrips every trip is a bisection, so the last kQuantileMaxTrips - kNewtonTrips
//           = 60 trips alone cut the bracket to 2^-60 of its width -- below the rounding of the q_k that span it.
// Every coordinate's search is a function of the row, the parameters and p alone: the register tier runs the dM coordinates of its 64
// rows in lock-step until a ballot says no lane has a coordinate left, and a coordinate that has stopped is never written again. A
// component with r_k == 0 leaves every sum as it is, so the wave-level skip of em_condition.hip changes no bit.
//
//   em_condition_cdf_kernel<PO, PM, W>       lane = row: x_O (PO), v, t, F, y (PM each) in VGPRs; k wave-uniform and the record's offsets
//   em_condition_quantile_kernel<PO, PM, W>  compile-time, so mu, A, s and w reach the arithmetic as scalar operands; the quantile form
//                                   keeps lo, hi, v, F, f and t (PM each). Values come in and results go out through LDS (odd row
//                                   stride) as contiguous 16 bytes per lane. Paddings and the -0.0 rows of A^T: em_condition.hip's;
//                                   s and w are +0.0 beyond dM: such a coordinate has lo == hi == 0 and is never searched or stored.
//   em_condition_cdf_plain_kernel, em_condition_quantile_plain_kernel   any dO + dM <= 4096: thread = row, table from global memory,
//                                   unpadded; the CDF accumulates in its output row, the search runs one coordinate at a time in
//                                   registers (it needs no work array: its state is five doubles). Same order, same bits.
#include "em_condition_common.hpp"
#include "mlhip.h"               // MLHIP_QUANTILE_NEWTON_TRIPS, MLHIP_QUANTILE_MAX_TRIPS: the header states the search's constants
#pragma clang fp contract(off)   // every fused multiply-add below is written out: both tiers and the host's restatement round alike
#include "exp_nonpos.hpp"
#include "normal_cdf.hpp"

namespace mlhip {
namespace {

constexpr int kCdfMaxRegisters = 32;             // dO and dM up to which the CDF's register tier exists
// The quantile search's register tier: the largest padded dM whose instantiations at every PO report no scratch
// (profiles/condition_quantile_registers.txt). This is the one place that states the bound.
constexpr int kQuantileMaxRegisters = 16;
constexpr int kNewtonTrips = MLHIP_QUANTILE_NEWTON_TRIPS;   // trips on which the Newton candidate may be taken (mlhip.h: 24)
constexpr int kQuantileMaxTrips = MLHIP_QUANTILE_MAX_TRIPS;  // the cap (mlhip.h: 84)
constexpr double kQuantileTolerance = 0x1p-50;      // |F - T| <= this * T: F is as close as a sum of normal_cdf values can tell
constexpr double kQuantileResolution = 0x1p-51;     // |candidate - v| <= this * |v|: the step is below v's own rounding

constexpr int quantile_waves(int PM) { return PM <= 4 ? 4 : PM <= 8 ? 2 : 1; }
__host__ __device__ constexpr size_t stage_doubles(int dM) { return (size_t)64 * ((size_t)dM | 1); }

/// The start of a coordinate's search. True: a search runs from v inside [lo, hi], widened here; false: v is the result. The start is
/// the weighted mean of the component quantiles CLAMPED into [lo, hi] -- it leaves it only by rounding --, so it may sit ON an end: a
/// row with one dominant component has its answer there, and an end is never evaluated otherwise (the search would bisect towards it
/// to the last bit). For the same reason the bracket is widened by 2^-50 of its larger end: a candidate that lands on an end, or a
/// few roundings beyond it, is strictly inside.
__device__ __forceinline__ bool quantile_start(double& lo, double& hi, double g, double S, double T, double& v)
{
    const double mean = g / S, mid = lo + (hi - lo) / 2;
    const double v0 = mean < lo ? lo : mean > hi ? hi : mean == mean ? mean : mid;
    const bool search = lo < hi && lo <= v0 && v0 <= hi && T == T;
    v = search ? v0 : (lo <= hi && T == T ? lo : __builtin_nan(""));
    const double pad = kQuantileResolution * 2 * (__builtin_fabs(lo) > __builtin_fabs(hi) ? __builtin_fabs(lo) : __builtin_fabs(hi));
    lo = search ? lo - pad : lo;
    hi = search ? hi + pad : hi;
    return search;
}

/// Trip `trip` of a coordinate's search, F and f evaluated at v. True: the coordinate has stopped, and v is the result.
__device__ __forceinline__ bool quantile_step(double F, double f, double S, double T, int trip, double& lo, double& hi, double& v)
{
    const bool below = F < T;
    lo = below ? v : lo;
    hi = below ? hi : v;
    // Newton on log F = log T (T < S / 2) or on log (S - F) = log (S - T): near the root the plain Newton step, in a tail the one that
    // does not creep (from inside) or fly off (from outside)
    const double G = S - F, GT = S - T;
    const bool lower = below ? T + T <= S : T + T < S;   // (at the median: the form that does not cross the root from this side)
    const double c = lower ? v + ::log(T / F) * (F / f) : v - ::log(GT / G) * (G / f);
    const bool converged = __builtin_fabs(F - T) <= kQuantileTolerance * T || __builtin_fabs(c - v) <= kQuantileResolution * __builtin_fabs(v);
    const double mid = lo + (hi - lo) / 2;
    const double next = trip <= kNewtonTrips && lo < c && c < hi ? c : mid;
    const bool stop = converged || !(lo < next && next < hi) || trip >= kQuantileMaxTrips;
    v = stop ? v : next;
    return stop;
}

/// A lane's PM registers out as the wave's rows x dM tile at dst.
template <int PM>
__device__ __forceinline__ void store_tile(double* stage, const double (&value)[PM], int dM, uint32_t rows, double* __restrict__ dst, int lane)
{
    const int S = dM | 1;
#pragma unroll
    for (int j = 0; j < PM; ++j)
        if (j < dM) stage[lane * S + j] = value[j];
    wave_sync();
    move_staged<false>(stage, S, rows, (uint32_t)dM, dst, lane);
    wave_sync();                                                 // (the next stores to the tile wait for these reads)
}

template <int PO, int PM, int W>
__global__ __launch_bounds__(64 * W) void em_condition_cdf_kernel(const double* __restrict__ xt, size_t ldx, uint32_t n, int dO, int dM, int K,
                                                                  const double* __restrict__ lw, size_t ldr, const double* __restrict__ lse,
                                                                  const double* __restrict__ table, const double* __restrict__ values,
                                                                  double* __restrict__ out, double* __restrict__ means, int skip)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    constexpr int PS = PO + PM + PO * PM + 2 * PM;
    const int S = dM | 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double* stage = sm + (size_t)wave * stage_doubles(dM);

    const uint32_t tiles = (n + 63) / 64;
    for (uint32_t t = blockIdx.x * W + wave; t < tiles; t += gridDim.x * W) {
        const uint32_t i = t * 64 + lane;                        // (beyond n: a padding row of the block, read but never stored)
        const bool live = i < n;
        const uint32_t rows = n - t * 64 < 64 ? n - t * 64 : 64;
        move_staged<true>(stage, S, rows, (uint32_t)dM, const_cast<double*>(values) + (size_t)t * 64 * (size_t)dM, lane);
        wave_sync();
        double v[PM];
#pragma unroll
        for (int j = 0; j < PM; ++j) v[j] = j < dM && live ? stage[lane * S + j] : 0.0;
        wave_sync();
        double x[PO];
#pragma unroll
        for (int c = 0; c < PO; ++c) x[c] = c < dO ? xt[(size_t)c * ldx + i] : 0.0;
        const double l = lse[i];
        double F[PM], y[PM];
#pragma unroll
        for (int j = 0; j < PM; ++j) F[j] = y[j] = 0.0;

        for (int k = 0; k < K; ++k) {
            const double r = live ? exp_nonpos(lw[(size_t)k * ldr + i] - l) : 0.0;
            const bool share = r != 0.0;                         // (a NaN has one: it reaches the output)
            if (skip && __ballot(share) == 0) continue;
            const double* __restrict__ rec = table + (size_t)k * PS;   // wave-uniform -> scalar loads
            const double* __restrict__ wk = rec + PO + PM + PO * PM + PM;
            double tj[PM];
            component_prediction(rec, x, dO, tj, PO, PM);
            if (means) {                                         // (wave-uniform)
#pragma unroll
                for (int j = 0; j < PM; ++j) {
                    const double m = __builtin_fma(r, tj[j], y[j]);
                    y[j] = share ? m : y[j];
                }
            }
#pragma unroll
            for (int j = 0; j < PM; ++j) {
                const double a = (v[j] - tj[j]) * wk[j];
                const double s = __builtin_fma(r, normal_cdf(a), F[j]);
                F[j] = share ? s : F[j];
            }
        }

        if (means) store_tile<PM>(stage, y, dM, rows, means + (size_t)t * 64 * (size_t)dM, lane);
        store_tile<PM>(stage, F, dM, rows, out + (size_t)t * 64 * (size_t)dM, lane);
    }
}

template <int PO, int PM, int W>
__global__ __launch_bounds__(64 * W) void em_condition_quantile_kernel(const double* __restrict__ xt, size_t ldx, uint32_t n, int dO, int dM,
                                                                       int K, const double* __restrict__ lw, size_t ldr,
                                                                       const double* __restrict__ lse, const double* __restrict__ table,
                                                                       const double* __restrict__ probabilities, const double* __restrict__ zs,
                                                                       uint32_t n_prob, double* __restrict__ out, size_t ldq,
                                                                       uint32_t* __restrict__ iterations, double* __restrict__ means, int skip)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    constexpr int PS = PO + PM + PO * PM + 2 * PM;
    constexpr uint32_t kAll = PM == 32 ? 0xFFFFFFFFu : (1u << PM) - 1u;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double* stage = sm + (size_t)wave * stage_doubles(dM);

    const uint32_t tiles = (n + 63) / 64;
    for (uint32_t t = blockIdx.x * W + wave; t < tiles; t += gridDim.x * W) {
        const uint32_t i = t * 64 + lane;                        // (beyond n: a padding row of the block, read but never stored)
        const bool live = i < n;
        const uint32_t rows = n - t * 64 < 64 ? n - t * 64 : 64;
        double x[PO];
#pragma unroll
        for (int c = 0; c < PO; ++c) x[c] = c < dO ? xt[(size_t)c * ldx + i] : 0.0;
        const double l = lse[i];
        double S = 0.0;
        for (int k = 0; k < K; ++k) S = S + (live ? exp_nonpos(lw[(size_t)k * ldr + i] - l) : 0.0);

#pragma unroll 1
        for (uint32_t q = 0; q < n_prob; ++q) {
            const double z = zs[q];
            const double T = probabilities[q] * S;
            double lo[PM], hi[PM], v[PM], F[PM], f[PM];
#pragma unroll
            for (int j = 0; j < PM; ++j) {
                lo[j] = __builtin_inf();
                hi[j] = -__builtin_inf();
                F[j] = f[j] = 0.0;
            }
            const bool with_mean = means && q == 0;              // (wave-uniform) f carries the mean through the first sweep
            for (int k = 0; k < K; ++k) {
                const double r = live ? exp_nonpos(lw[(size_t)k * ldr + i] - l) : 0.0;
                const bool share = r != 0.0;
                if (skip && __ballot(share) == 0) continue;
                const double* __restrict__ rec = table + (size_t)k * PS;
                const double* __restrict__ sk = rec + PO + PM + PO * PM;
                double tj[PM];
                component_prediction(rec, x, dO, tj, PO, PM);
                if (with_mean) {
#pragma unroll
                    for (int j = 0; j < PM; ++j) {
                        const double m = __builtin_fma(r, tj[j], f[j]);
                        f[j] = share ? m : f[j];
                    }
                }
#pragma unroll
                for (int j = 0; j < PM; ++j) {
                    const double qk = __builtin_fma(sk[j], z, tj[j]);
                    const bool nan = qk != qk;
                    lo[j] = share && (qk < lo[j] || nan) ? qk : lo[j];
                    hi[j] = share && (qk > hi[j] || nan) ? qk : hi[j];
                    const double g = __builtin_fma(r, qk, F[j]);
                    F[j] = share ? g : F[j];
                }
            }
            if (with_mean) store_tile<PM>(stage, f, dM, rows, means + (size_t)t * 64 * (size_t)dM, lane);

            uint32_t done = live ? 0u : kAll;
            uint32_t trips[(PM + 3) / 4];                        // a byte per coordinate: kQuantileMaxTrips < 256
#pragma unroll
            for (int j = 0; j < (PM + 3) / 4; ++j) trips[j] = 0;
#pragma unroll
            for (int j = 0; j < PM; ++j)
                if (!quantile_start(lo[j], hi[j], F[j], S, T, v[j])) done |= 1u << j;

#pragma unroll 1
            for (int trip = 1; __ballot(done != kAll) != 0; ++trip) {
#pragma unroll
                for (int j = 0; j < PM; ++j) F[j] = f[j] = 0.0;
                for (int k = 0; k < K; ++k) {
                    const double r = live ? exp_nonpos(lw[(size_t)k * ldr + i] - l) : 0.0;
                    const bool share = r != 0.0;
                    if (skip && __ballot(share) == 0) continue;
                    const double* __restrict__ rec = table + (size_t)k * PS;
                    const double* __restrict__ wk = rec + PO + PM + PO * PM + PM;
                    double tj[PM];
                    component_prediction(rec, x, dO, tj, PO, PM);
#pragma unroll
                    for (int j = 0; j < PM; ++j) {
                        const double a = (v[j] - tj[j]) * wk[j];
                        double pdf;
                        const double cdf = normal_cdf_pdf(a, pdf);
                        const double s = __builtin_fma(r, cdf, F[j]);
                        const double d = __builtin_fma(r, wk[j] * pdf, f[j]);
                        F[j] = share ? s : F[j];
                        f[j] = share ? d : f[j];
                    }
                }
#pragma unroll
                for (int j = 0; j < PM; ++j) {
                    if (!(done & (1u << j))) {
                        trips[j >> 2] += 1u << (8 * (j & 3));
                        if (quantile_step(F[j], f[j], S, T, trip, lo[j], hi[j], v[j])) done |= 1u << j;
                    }
                }
            }

            store_tile<PM>(stage, v, dM, rows, out + (size_t)q * ldq + (size_t)t * 64 * (size_t)dM, lane);
            if (iterations && live) {
#pragma unroll
                for (int j = 0; j < PM; ++j)
                    if (j < dM) iterations[(size_t)q * ldq + (size_t)i * dM + j] = (trips[j >> 2] >> (8 * (j & 3))) & 255u;
            }
        }
    }
}

__global__ __launch_bounds__(256) void em_condition_cdf_plain_kernel(const double* __restrict__ xt, size_t ldx, uint32_t n, int dO, int dM, int K,
                                                                     const double* __restrict__ lw, size_t ldr, const double* __restrict__ lse,
                                                                     const double* __restrict__ table, const double* __restrict__ values,
                                                                     double* __restrict__ out, double* __restrict__ means)
{
    const size_t PS = (size_t)dO + dM + (size_t)dO * dM + 2 * (size_t)dM;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const double l = lse[i];
        double* F = out + (size_t)i * dM;                        // the output row is the accumulator
        double* y = means ? means + (size_t)i * dM : nullptr;
        for (int j = 0; j < dM; ++j) F[j] = 0.0;
        if (y)
            for (int j = 0; j < dM; ++j) y[j] = 0.0;
        for (int k = 0; k < K; ++k) {
            const double r = exp_nonpos(lw[(size_t)k * ldr + i] - l);
            if (!(r != 0.0)) continue;
            const double* rec = table + (size_t)k * PS;
            const double* wk = rec + dO + dM + (size_t)dO * dM + dM;
            for (int j = 0; j < dM; ++j) {
                const double tj = plain_prediction(rec, dO, dM, j, xt, ldx, i);
                if (y) y[j] = __builtin_fma(r, tj, y[j]);
                const double a = (values[(size_t)i * dM + j] - tj) * wk[j];
                F[j] = __builtin_fma(r, normal_cdf(a), F[j]);
            }
        }
    }
}

__global__ __launch_bounds__(256) void em_condition_quantile_plain_kernel(const double* __restrict__ xt, size_t ldx, uint32_t n, int dO, int dM,
                                                                          int K, const double* __restrict__ lw, size_t ldr,
                                                                          const double* __restrict__ lse, const double* __restrict__ table,
                                                                          const double* __restrict__ probabilities,
                                                                          const double* __restrict__ zs, uint32_t n_prob,
                                                                          double* __restrict__ out, size_t ldq, uint32_t* __restrict__ iterations,
                                                                          double* __restrict__ means)
{
    const size_t PS = (size_t)dO + dM + (size_t)dO * dM + 2 * (size_t)dM;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const double l = lse[i];
        double S = 0.0;
        for (int k = 0; k < K; ++k) S = S + exp_nonpos(lw[(size_t)k * ldr + i] - l);
        for (int j = 0; j < dM; ++j) {
            auto prediction = [&](const double* rec) { return plain_prediction(rec, dO, dM, j, xt, ldx, i); };
            if (means) {
                double y = 0.0;
                for (int k = 0; k < K; ++k) {
                    const double r = exp_nonpos(lw[(size_t)k * ldr + i] - l);
                    if (!(r != 0.0)) continue;
                    y = __builtin_fma(r, prediction(table + (size_t)k * PS), y);
                }
                means[(size_t)i * dM + j] = y;
            }
            for (uint32_t q = 0; q < n_prob; ++q) {
                const double z = zs[q];
                const double T = probabilities[q] * S;
                double lo = __builtin_inf(), hi = -__builtin_inf(), g = 0.0, v;
                for (int k = 0; k < K; ++k) {
                    const double r = exp_nonpos(lw[(size_t)k * ldr + i] - l);
                    if (!(r != 0.0)) continue;
                    const double* rec = table + (size_t)k * PS;
                    const double qk = __builtin_fma(rec[(size_t)dO + dM + (size_t)dO * dM + j], z, prediction(rec));
                    const bool nan = qk != qk;
                    lo = qk < lo || nan ? qk : lo;
                    hi = qk > hi || nan ? qk : hi;
                    g = __builtin_fma(r, qk, g);
                }
                uint32_t trips = 0;
                bool stopped = !quantile_start(lo, hi, g, S, T, v);
                while (!stopped) {
                    double F = 0.0, f = 0.0;
                    for (int k = 0; k < K; ++k) {
                        const double r = exp_nonpos(lw[(size_t)k * ldr + i] - l);
                        if (!(r != 0.0)) continue;
                        const double* rec = table + (size_t)k * PS;
                        const double w = rec[(size_t)dO + dM + (size_t)dO * dM + dM + j];
                        const double a = (v - prediction(rec)) * w;
                        double pdf;
                        const double cdf = normal_cdf_pdf(a, pdf);
                        F = __builtin_fma(r, cdf, F);
                        f = __builtin_fma(r, w * pdf, f);
                    }
                    ++trips;
                    stopped = quantile_step(F, f, S, T, (int)trips, lo, hi, v);
                }
                out[(size_t)q * ldq + (size_t)i * dM + j] = v;
                if (iterations) iterations[(size_t)q * ldq + (size_t)i * dM + j] = trips;
            }
        }
    }
}

int launch(const ConditionQuantileArgs& a, bool quantile, int num_cus, hipStream_t stream)
{
    if (a.dO < 1 || a.dM < 1 || a.dO + a.dM > kGenericMaxDim || a.K < 1) return -1;
    if (a.n == 0 || (quantile && a.n_prob == 0)) return 0;
    if (a.kernel == kConditionPlain) {
        const uint32_t grid = row_grid(a.n, num_cus);
        if (quantile)
            hipLaunchKernelGGL(em_condition_quantile_plain_kernel, dim3(grid), dim3(256), 0, stream, a.xt, a.ldx, a.n, a.dO, a.dM, a.K, a.lw, a.ldr,
                               a.lse, a.table, a.probabilities, a.z, a.n_prob, a.out, a.ldq, a.iterations, a.means);
        else
            hipLaunchKernelGGL(em_condition_cdf_plain_kernel, dim3(grid), dim3(256), 0, stream, a.xt, a.ldx, a.n, a.dO, a.dM, a.K, a.lw, a.ldr, a.lse,
                               a.table, a.values, a.out, a.means);
        return (int)grid;
    }
    if (em_condition_quantile_route(a.dO, a.dM, quantile) != kConditionRegisters) return -1;
    if (quantile)
        return dispatch_paddings<kQuantileMaxRegisters>(a.dO, a.dM, [&](auto po, auto pm) {
            constexpr int PO = decltype(po)::value, PM = decltype(pm)::value, W = quantile_waves(PM);
            const uint32_t grid = tile_grid(a.n, W, num_cus);
            hipLaunchKernelGGL((em_condition_quantile_kernel<PO, PM, W>), dim3(grid), dim3(64 * W), sizeof(double) * W * stage_doubles(a.dM), stream,
                               a.xt, a.ldx, a.n, a.dO, a.dM, a.K, a.lw, a.ldr, a.lse, a.table, a.probabilities, a.z, a.n_prob, a.out, a.ldq,
                               a.iterations, a.means, a.skip);
            return (int)grid;
        });
    return dispatch_paddings<kCdfMaxRegisters>(a.dO, a.dM, [&](auto po, auto pm) {
        constexpr int PO = decltype(po)::value, PM = decltype(pm)::value, W = condition_waves(PM);
        const uint32_t grid = tile_grid(a.n, W, num_cus);
        hipLaunchKernelGGL((em_condition_cdf_kernel<PO, PM, W>), dim3(grid), dim3(64 * W), sizeof(double) * W * stage_doubles(a.dM), stream, a.xt,
                           a.ldx, a.n, a.dO, a.dM, a.K, a.lw, a.ldr, a.lse, a.table, a.values, a.out, a.means, a.skip);
        return (int)grid;
    });
}

}  // namespace

int em_condition_quantile_route(int dO, int dM, int quantile)
{
    return dO <= kCdfMaxRegisters && dM <= (quantile ? kQuantileMaxRegisters : kCdfMaxRegisters) ? kConditionRegisters : kConditionPlain;
}

int launch_em_condition_cdf(const ConditionQuantileArgs& a, int num_cus, hipStream_t stream) { return launch(a, false, num_cus, stream); }

int launch_em_condition_quantile(const ConditionQuantileArgs& a, int num_cus, hipStream_t stream) { return launch(a, true, num_cus, stream); }

}  // namespace mlhip
