// Host-side dense helpers of the EM path (tiny d x d work that stays on the CPU):
// what EM::process_covariances (reference ML/EM.cpp:274-287) and the closing lines of
// EM::maximisation_step (ML/EM.cpp:242, 250-257) do, expressed on raw column-major buffers.
#pragma once
#include <cstddef>
#include <cstdint>

namespace mlhip {
namespace host {

/// Lower Cholesky factor of the symmetric d x d matrix A (column-major); what Eigen::LLT computes at
/// ML/EM.cpp:279. A non-positive-definite A yields NaNs, silently, like the reference (no info() check).
void cholesky_lower(int d, const double* A, double* L);

/// inverse = A^-1 via L y = e_c, L^T x = y (the llt.solve(Identity) of ML/EM.cpp:280);
/// sqrt_det = prod L_ii (ML/EM.cpp:281-285).
void process_covariance(int d, const double* cov, double* inverse, double* sqrt_det);

/// One E-step record per component for the device kernel (layout: device/device.hpp estep_param_stride):
/// [mean(D) | W = L^-1 packed lower, row-major | log(pi) - sum log L_jj], coordinates >= d zero-padded.
void build_estep_params(int d, int D, int K, const double* mixing, const double* means, const double* covariances,
                        double* records);

/// Same for the 4x4-block matrix-core E-step kernel (layout: device/layout.hpp estep_mfma4_param_stride). With a `shift`
/// (the data's d-vector) the second vector of every record, -W (mu - shift), is filled too; returns whether the kernel's FOLD
/// form may use it: every entry of every W_k (mu_k - shift) finite and at most `fold_limit` in magnitude.
bool build_estep_params_mfma4(int d, int D, int K, const double* mixing, const double* means, const double* covariances,
                              const double* shift, double fold_limit, double* records);

/// M-step closing arithmetic from the all-reduced shifted statistics (device/device.hpp stats_count):
///   mean_k = shift + S1'/S0 ; cov_k = (M2' - S1' (S1'/S0)^T) / S0 + ridge I ; pi_k = S0 / N.
/// Algebraically the reference's  sum_i r_ik (x_i - mean_k)(x_i - mean_k)^T / S0  (ML/EM.cpp:245-257).
/// `ridge` is the data handle's covariance ridge (mlhip.h: default 1e-15, the constant of ML/EM.cpp:252), one plain add per diagonal entry.
void finalize_mstep(int d, int K, const double* stats, const double* shift, double n_global, double ridge, double* mixing,
                    double* means, double* covariances);

/// Diagonal-covariance extension: K_padded records [mean(D) | 1/sigma^2 (D) | log(pi) - sum log sigma | two-op flag] and the
/// dimension-major trailer [1/sigma | -(mean - shift)/sigma] behind them (layout.hpp diag_param_stride / diag_param_doubles)
/// from variances[K*d]; sigma_j = sqrt(var_j) is the diagonal Cholesky factor, 1/sigma^2 = (1/sigma)/sigma what
/// llt.solve(I) yields for it (ML/EM.cpp:279-285 restricted to a diagonal matrix).
/// `records` receives K_padded >= K records; those beyond K are neutral (coef = -inf: log-density -inf, responsibility 0).
void build_diag_params(int d, int D, int K, int K_padded, const double* mixing, const double* means, const double* variances,
                       const double* shift, double* records);

/// Diagonal closing arithmetic from the all-reduced statistics [S1'(d) | S2'(d) | S0] per component:
///   mean_k = shift + S1'/S0 ; var_kj = (S2'_j - S1'_j (S1'_j/S0)) / S0 + ridge ; pi_k = S0 / N   (ML/EM.cpp:242-257, diagonal).
void finalize_mstep_diag(int d, int K, const double* stats, const double* shift, double n_global, double ridge, double* mixing,
                         double* means, double* variances);

/// Tied-covariance extension (ONE Sigma = L L^T for all components): the whitening block winv = L^-1 (layout.hpp
/// tied_winv_doubles: packed lower triangle, rows d .. D-1 zero) and K_padded records [m_k = L^-1 (mean_k - shift) (D) |
/// log(pi_k) - sum_j log L_jj] (tied_param_stride) from the one d x d covariance; records beyond K are neutral (coef = -inf).
void build_tied_params(int d, int D, int K, int K_padded, const double* mixing, const double* means, const double* covariance,
                       const double* shift, double* winv, double* records);

/// Tied closing arithmetic from the all-reduced statistics [S1'(d) | S0] per component and the total scatter
/// T = sum_i w_i xt_i xt_i^T (packed like one component's full statistics: stats_count(d) doubles, xt = [x - shift ; 1]):
///   mean_k = shift + S1'_k/S0_k ; pi_k = S0_k / W ; Sigma = (T - sum_k S1'_k (S1'_k/S0_k)^T) / W + ridge I
/// (k ascending per entry; the ridge of ML/EM.cpp:252-256 once) == sum_k pi_k Sigma_k over finalize_mstep's Sigma_k.
void finalize_mstep_tied(int d, int K, const double* stats, const double* total_scatter, const double* shift, double total_weight,
                         double ridge, double* mixing, double* means, double* covariance);

/// The covariance mode of an EM call: K full matrices (K d d doubles), K diagonals (K d variances) or the one matrix all components
/// share (d d). The values are mlhip.h's MLHIP_COVARIANCE_* (runtime/internal.hpp checks that).
enum class Covariance : int { Full = 0, Diagonal = 1, Tied = 2 };

/// The mode an ABI `covariance_type` names; std::invalid_argument("bad covariance_type") for any other value.
Covariance covariance_from_abi(int covariance_type);

/// Doubles in the covariance array of `mode`.
std::size_t covariance_doubles(Covariance mode, int K, int d);

/// The covariance array of `mode` as K full d x d matrices in `full`: a diagonal becomes a diagonal matrix (+0.0 elsewhere), the tied
/// matrix K copies, full matrices a copy.
void covariances_as_full(Covariance mode, int K, int d, const double* covariance, double* full);

/// K full matrices and the mixing weights pi as the covariance array of `mode`: the diagonals; the pooled sum_k pi_k Sigma_k -- per
/// entry v = 0, then v += pi_k Sigma_k[e] in ascending k: the order is part of the results' bits --; a copy.
void covariances_from_full(Covariance mode, int K, int d, const double* mixing, const double* full, double* covariance);

/// Conditioning of a mixture over (x_O, x_M) on the observed block (mlhip_em_condition, mlhip.h). `observed`: n_observed distinct
/// coordinates < d in any order (column c of an observed row holds coordinate observed[c]); the missing ones are the complement, ascending.
/// Per component, on the covariance as a full matrix (covariances_as_full: a diagonal gives maps of +0.0, the tied matrix K equal maps):
///   means_observed[k][c] = mu_k[O_c]; covariances_observed[k] = Sigma_k,OO (dO x dO, always full); means_missing[k][j] = mu_k[M_j];
///   maps[k] = A_k = Sigma_k,MO Sigma_k,OO^-1 (dM x dO, row j = missing coordinate j), row j solved as L y = Sigma_k,O M_j (forward),
///   L^T a = y (backward) with L = cholesky_lower(Sigma_k,OO) -- the substitutions of process_covariance.
/// std::domain_error when a Sigma_k,OO is not positive definite (a factor with a non-finite entry or a diagonal that is not > 0).
void condition(Covariance mode, int K, int d, const double* means, const double* covariance, const unsigned int* observed, int n_observed,
               double* means_observed, double* covariances_observed, double* maps, double* means_missing);

/// The covariances of the conditioned components (mlhip_em_condition_covariances, mlhip.h), `observed` as for condition(). Per
/// component, with L = cholesky_lower(Sigma_k,OO) (condition()'s factor) and Y = L^-1 Sigma_k,OM (its forward substitution):
///   covariances_missing[k] = C_k = Sigma_k,MM - Y^T Y (dM x dM; entry (a, b), b <= a: t = Sigma[M_a][M_b], t -= Y[l][a] Y[l][b] for
///   ascending l; mirrored, so symmetric by construction); factors[k] = G_k = cholesky_lower(C_k), row-major (row j, column c at
///   j dM + c), +0.0 above the diagonal; `factors` may be null. A diagonal gives C_k = diag(sigma^2_M) and G_k = diag(sqrt) exactly,
/// the tied matrix K copies. std::domain_error when a Sigma_k,OO or a C_k is not positive definite.
void condition_covariances(Covariance mode, int K, int d, const double* covariance, const unsigned int* observed, int n_observed,
                           double* covariances_missing, double* factors);

/// Tells the host-side math how many ranks share this node, so that the OpenMP teams of the per-component
/// factorizations together stay within the host's cores (MLHIP_HOST_THREADS overrides the per-rank thread count).
void set_host_ranks(int local_ranks);
/// The threads a host-side region of this process may use (what set_host_ranks or MLHIP_HOST_THREADS left; at most 8 by default).
int host_threads();

}  // namespace host
}  // namespace mlhip
