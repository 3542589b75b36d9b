// The conditioned records of mlhip_em_impute's kernel route for gfx950: one WAVE per (pattern, component), the matrices in LDS, as
// em_close.hip closes an M-step. With P patterns in the thousands the host conditioning (P x K factorizations, one pattern after the
// other) costs more than the whole evaluation, so it is done here. Per (p, k), with O / M the pattern's observed / missing
// coordinates ascending:
//   1. S = Sigma_k,OO gathered by O into LDS (lane = row);
//   2. L L^T = S in place, column by column: lane i forms s = S[i][j] - sum_{l<j} L[i][l] L[j][l] (ascending l), lane j takes
//      L[j][j] = sqrt(s), the lanes below divide by it. A pivot that is not > 0 or not finite sets *flag (a plain vector store) and
//      is taken as 1.0: everything written stays finite, and the host returns the domain error of mlhip_em_condition;
//   3. W = L^-1, lane c its column c: W[c][c] = 1 / L[c][c]; W[i][c] = -(sum_{l=c}^{i-1} L[i][l] W[l][c]) / L[i][i];
//   4. coef = log pi_k - sum_j log L[j][j] (ascending j);
//   5. A_k = Sigma_k,MO Sigma_k,OO^-1, lane j its row j: L y = Sigma_k,O M_j forward, L^T a = y backward -- the substitutions of
//      host::condition, every lane alone with its own column of a scratch tile;
//   6. the padded record [mu_O | mu_M | A^T | W | coef] (device.hpp: ImputePattern), written lane by lane.
// The results are held to the longdouble restatement within the factorization's backward-error bound, not to the host's bits.
#include "em_condition_common.hpp"

namespace mlhip {
namespace {

constexpr int LD = kImputeMaxDim + 1;                            // LDS row stride (odd: a lane per row reads without conflicts)

__global__ __launch_bounds__(64) void em_impute_records_kernel(int d, int K, const double* __restrict__ means, const double* __restrict__ covs,
                                                              const double* __restrict__ log_mixing,
                                                              const ImputePattern* __restrict__ patterns, double* __restrict__ records,
                                                              uint32_t* __restrict__ flag)
{
    __shared__ double S[kImputeMaxDim * LD], Wm[kImputeMaxDim * LD], Y[kImputeMaxDim * LD];
    const int lane = threadIdx.x;
    const uint32_t p = blockIdx.x / (uint32_t)K;
    const int k = (int)(blockIdx.x % (uint32_t)K);
    const ImputePattern& pat = patterns[p];
    const int dO = (int)pat.dO, dM = (int)pat.dM;
    const int PO = (int)pat.po, PM = (int)pat.pm;
    const double* cov = covs + (size_t)k * d * d;
    const double* mu = means + (size_t)k * d;

    // 1. gather (lane = row i of S)
    if (lane < dO) {
        const uint32_t oi = pat.observed[lane];
        for (int j = 0; j < dO; ++j) S[lane * LD + j] = cov[(size_t)oi * d + pat.observed[j]];
    }
    wave_sync();

    // 2. factor in place: the lower triangle of S becomes L
    for (int j = 0; j < dO; ++j) {
        double s = 0.0;
        if (lane >= j && lane < dO) {
            s = S[lane * LD + j];
            for (int l = 0; l < j; ++l) s -= S[lane * LD + l] * S[j * LD + l];
        }
        if (lane == j) {
            if (!(s > 0.0) || !(s < __builtin_inf())) {
                *flag = 1u;
                s = 1.0;
            }
            S[j * LD + j] = sqrt(s);
        }
        wave_sync();
        if (lane > j && lane < dO) S[lane * LD + j] = s / S[j * LD + j];
        wave_sync();
    }

    // 3. W = L^-1: lane c forms column c from the rows above it that it wrote itself
    if (lane < dO) {
        const int c = lane;
        Wm[c * LD + c] = 1.0 / S[c * LD + c];
        for (int i = c + 1; i < dO; ++i) {
            double t = 0.0;
            for (int l = c; l < i; ++l) t += S[i * LD + l] * Wm[l * LD + c];
            Wm[i * LD + c] = -t / S[i * LD + i];
        }
    }

    // 5. the maps: lane j solves for missing coordinate j in column j of Y
    if (lane < dM) {
        const uint32_t mj = pat.missing[lane];
        for (int c = 0; c < dO; ++c) {
            double t = cov[(size_t)pat.observed[c] * d + mj];
            for (int l = 0; l < c; ++l) t -= S[c * LD + l] * Y[l * LD + lane];
            Y[c * LD + lane] = t / S[c * LD + c];
        }
        for (int c = dO - 1; c >= 0; --c) {
            double t = Y[c * LD + lane];
            for (int l = c + 1; l < dO; ++l) t -= S[l * LD + c] * Y[l * LD + lane];
            Y[c * LD + lane] = t / S[c * LD + c];
        }
    }
    wave_sync();

    // 6. the record
    double* rec = records + pat.rec_base + (size_t)k * (PO + PM + PO * PM + PO * (PO + 1) / 2 + 1);
    if (lane < PO) rec[lane] = lane < dO ? mu[pat.observed[lane]] : 0.0;
    if (lane < PM) rec[PO + lane] = lane < dM ? mu[pat.missing[lane]] : 0.0;
    double* at = rec + PO + PM;
    for (int e = lane; e < PO * PM; e += 64) {
        const int c = e / PM, j = e % PM;
        at[e] = c >= dO ? -0.0 : (j < dM ? Y[c * LD + j] : 0.0);
    }
    double* w = at + PO * PM;
    for (int j = 0; j < PO; ++j)
        if (lane <= j) w[j * (j + 1) / 2 + lane] = j < dO ? Wm[j * LD + lane] : 0.0;
    if (lane == 0) {
        // 4.
        double sum_log = 0.0;
        for (int j = 0; j < dO; ++j) sum_log += log(S[j * LD + j]);
        w[PO * (PO + 1) / 2] = log_mixing[k] - sum_log;
    }
}

}  // namespace

void launch_em_impute_records(const ImputeRecordsArgs& a, hipStream_t stream)
{
    if (!a.n_patterns || a.K < 1) return;
    hipLaunchKernelGGL(em_impute_records_kernel, dim3(a.n_patterns * (uint32_t)a.K), dim3(64), 0, stream, a.d, a.K, a.means, a.covs,
                       a.log_mixing, a.patterns, a.records, a.flag);
}

}  // namespace mlhip
