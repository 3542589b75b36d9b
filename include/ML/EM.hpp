#pragma once
#ifdef MLHIP_ML_EIGEN_API_HPP
#error "ML/EM.hpp and ML/EigenApi.hpp share their class names: include one family per translation unit"
#endif
#define MLHIP_ML_EM_HPP
/* ml::EM -- Gaussian-mixture Expectation-Maximisation with the public interface of the reference's
 * ML/EM.hpp:18-198 (same method names, defaults, exceptions and result semantics), executed on an MI355X:
 * the E-step / M-step loops of ML/EM.cpp:190-263 run as HIP kernels through the C ABI in mlhip.h; this class keeps
 * the driver loop (ML/EM.cpp:91-174), the convergence test and the host-side point query. */
#include <cstdint>
#include <memory>
#include <random>
#include <vector>

#include "Clustering.hpp"
#include "Dense.hpp"
#include "dll.hpp"

struct mlhip_data;

namespace ml {

class EM : public Clustering::Model {
public:
    /** @throw std::invalid_argument If `number_components == 0`. */
    DLL_DECLSPEC EM(unsigned int number_components);
    DLL_DECLSPEC ~EM() override;
    EM(const EM&) = delete;
    EM& operator=(const EM&) = delete;

    DLL_DECLSPEC void set_seed(unsigned int seed);
    /** @throw std::domain_error If `absolute_tolerance < 0`. */
    DLL_DECLSPEC void set_absolute_tolerance(double absolute_tolerance);
    /** @throw std::domain_error If `relative_tolerance < 0`. */
    DLL_DECLSPEC void set_relative_tolerance(double relative_tolerance);
    /** @throw std::invalid_argument If `maximum_steps < 2`. */
    DLL_DECLSPEC void set_maximum_steps(unsigned int maximum_steps);
    /** @throw std::invalid_argument If `means_initialiser` is null. */
    DLL_DECLSPEC void set_means_initialiser(std::shared_ptr<const Clustering::CentroidsInitialiser> means_initialiser);
    /** @throw std::invalid_argument If `responsibilities_initialiser` is null. */
    DLL_DECLSPEC void set_responsibilities_initialiser(std::shared_ptr<const Clustering::ResponsibilitiesInitialiser> responsibilities_initialiser);
    void set_verbose(bool verbose) { verbose_ = verbose; }
    void set_maximise_first(bool maximise_first) { maximise_first_ = maximise_first; }
    /** EXTENSION -- not part of the reference API, whose EM is full-covariance only (reference ML/EM.hpp:175). With
    `Diagonal` every covariance is restricted to its diagonal (the E-/M-step loops of ML/EM.cpp:190-263 on the diagonal
    entries only; covariances() returns diagonal matrices). Default `Full` == the reference's behaviour.
    One fused kernel serves number_dimensions <= 32 and number_components <= 64; other shapes run the full-covariance kernels on
    diagonal matrices (slower, never refused).
    With `Tied` all components share ONE covariance (scikit-learn's 'tied'): Sigma = sum_k pi_k Sigma_k of the full M-step, the ridge
    (covariance_regularisation(), default 1e-15) once; covariances() returns number_components() copies of it, so the point query and the batch queries work unchanged. The
    start is the pooled sum_k pi_k Sigma_k of the starting covariances (the sample covariance on the default start). One kernel per
    iteration serves unweighted fits with number_dimensions <= 32 and number_components <= 64; other shapes and weighted fits run the
    full-covariance kernels on copies of Sigma and pool the result (mlhip_em_step_tied). */
    enum class CovarianceType { Full, Diagonal, Tied };
    void set_covariance_type(CovarianceType covariance_type) { covariance_type_ = covariance_type; }
    CovarianceType covariance_type() const { return covariance_type_; }
    /** EXTENSION -- scikit-learn's `reg_covar`; the reference hard-wires 1e-15 (ML/EM.cpp:252), which stays the default. Every M-step
    of the next fit() adds this value to the diagonal of each covariance it forms (Full: every component's; Diagonal: every variance;
    Tied: the one covariance, once) -- the `maximise_first` start included. The starting covariance (the sample covariance) and the
    exact N == K fit are not touched (mlhip_data_set_covariance_ridge). 0 is allowed.
    @throw std::domain_error If the value is negative or not finite. */
    DLL_DECLSPEC void set_covariance_regularisation(double covariance_regularisation);
    double covariance_regularisation() const { return covariance_regularisation_; }

    /** EXTENSION -- the reference's EM has no restarts (its KMeans has set_number_initialisations; scikit-learn's GaussianMixture has
    `n_init`). fit() then runs this many EM loops on the one uploaded sample and keeps the best: start r is what a solo fit would
    begin from, drawn from the seeded PRNG in order r = 0, 1, ... (the loops consume no random numbers, so the starts are those of
    that many consecutive solo fit() calls on one object after one set_seed). Among the loops that converged the greatest final
    log-likelihood wins, the first of equals; if none converged the same rule runs over all (mlhip_em_select_restart). fit() returns
    the winner's converged(); steps_done(), log_likelihood(), the parameters, responsibilities() and labels() are the winner's. Short
    fits of few components in few dimensions run their restarts side by side on the GPU (mlhip_em_iterate_restarts). The exact
    N == K fit ignores the setting; verbose mode runs the loops one after the other, an `Initialisation r` line in front of each.
    (Verbose mode puts the winner's responsibilities back with one E-step on the inputs of its last one: with full covariances that is
    the solo verbose fit's state bit for bit; in Diagonal and Tied mode it runs the full-covariance E-step on the expanded matrices,
    so responsibilities() may differ from the solo verbose fit's in the last bits there, and on a multi-rank job it is one more
    collective E-step. The bit-for-bit statement above is about the non-verbose fit.)
    Default 1: the reference's behaviour. @throw std::invalid_argument If `number_initialisations == 0`. */
    DLL_DECLSPEC void set_number_initialisations(unsigned int number_initialisations);
    unsigned int number_initialisations() const { return number_initialisations_; }
    /** Extension: the initialisation the fitted state belongs to (0 with one initialisation). */
    unsigned int best_initialisation() const { return best_initialisation_; }
    /** Extension: final log-likelihood, iterations and convergence flag (0 / 1) of every initialisation of the last fit(). */
    const std::vector<double>& initialisation_log_likelihoods() const { return initialisation_log_likelihoods_; }
    const std::vector<unsigned int>& initialisation_steps() const { return initialisation_steps_; }
    const std::vector<int>& initialisation_converged() const { return initialisation_converged_; }

    /** @brief Fits the model. @param[in] data Column-major, a data point in every column (this rank's row shard when an
    all-reduce hook is installed on the device context). @return `true` if fitting converged.
    @throw std::invalid_argument If `data` has no rows or fewer columns than components.
    @throw std::runtime_error On device failures (no GPU, HIP or collective errors). */
    DLL_DECLSPEC bool fit(ConstMatrixRef data) override;
    /** Extension (not in the reference surface): the same fit of a WEIGHTED sample -- `weights[i]` >= 0 is the frequency weight of
    column i of `data` (integer weights: the fit of the sample with point i repeated weights[i] times, without the copies). The
    log-likelihood, its convergence test and every M-step are weighted; responsibilities() and labels() stay per point; the
    initialisers see points, not weights; the N < K and N == K branches count points (mlhip_data_set_weights).
    @throw std::invalid_argument If `weights.size() != data.cols()`, a weight is negative or not finite, or their total is not positive. */
    DLL_DECLSPEC bool fit(ConstMatrixRef data, ConstVectorRef weights);

    unsigned int number_components() const { return number_components_; }
    unsigned int number_clusters() const override { return number_components(); }
    /** `number_dimensions` x number_components(). */
    const MatrixXd& means() const { return means_; }
    const MatrixXd& centroids() const override { return means(); }
    const std::vector<MatrixXd>& covariances() const { return covariances_; }
    /** @throw std::invalid_argument If `k >= number_components()`. */
    DLL_DECLSPEC const MatrixXd& covariance(unsigned int k) const;
    const VectorXd& mixing_probabilities() const { return mixing_probabilities_; }
    /** `sample_size` x number_components(): the responsibilities of the last E-step. They stay on the device after
    fit() and are copied to the host on the first call (N x K doubles), unlike the reference which always holds them. */
    DLL_DECLSPEC const MatrixXd& responsibilities() const;
    /** Extension: rows [first_row, first_row + number_rows) of responsibilities() as a number_rows x number_components() matrix,
    WITHOUT materialising the whole block on the host when it still lives on the device (what a slice of a 5 GB block costs).
    @throw std::invalid_argument If the range exceeds the sample. */
    DLL_DECLSPEC MatrixXd responsibilities_rows(Index first_row, Index number_rows) const;
    double log_likelihood() const { return log_likelihood_; }
    std::shared_ptr<const Clustering::CentroidsInitialiser> means_initialiser() const { return means_initialiser_; }
    /** Posterior component probabilities of one point under the fitted parameters (host-side).
    @throw std::invalid_argument If `x.size() != means().rows()` or `u.size() != number_components()`. */
    DLL_DECLSPEC void assign_responsibilities(ConstVectorRef x, VectorRef u) const;
    /** Extension (not in the reference surface): log sum_k pi_k N(x_i | mu_k, Sigma_k) of every column of `data` (a data point in
    every column, like fit's; any number of them) under the fitted parameters, computed on the device in one pass that writes 12
    bytes per point (mlhip_em_score). The block is uploaded in row batches (2^24 points; MLHIP_SCORE_ROWS overrides), so it may be
    larger than the fit's; the results do not depend on the batch size. The fit's own device block and responsibilities() are not
    touched. In a row-sharded job every rank scores its own block and must pass the same number of batches.
    @throw std::invalid_argument If `data.rows() != means().rows()` or the model has not been fitted.
    @throw std::runtime_error On device failures (no GPU: there is no CPU fallback). */
    DLL_DECLSPEC VectorXd log_densities(ConstMatrixRef data) const;
    /** Extension: the mean of log_densities(data), summed sequentially in row order (comparable with log_likelihood()); NaN for an
    empty block (the other batch queries return empty results for one). */
    DLL_DECLSPEC double mean_log_density(ConstMatrixRef data) const;
    /** Extension (model selection; scikit-learn's `_n_parameters`): the free parameters of the fitted mixture in the covariance mode
    it was FITTED in -- K d(d+1)/2 for Full, K d for Diagonal, d(d+1)/2 for Tied --, plus K d for the means and K - 1 for the mixing
    probabilities. Host only. @throw std::invalid_argument If the model has not been fitted. */
    DLL_DECLSPEC std::size_t number_parameters() const;
    /** Extension: the Bayesian information criterion of the fitted model on `data`, -2 N mean_log_density(data) +
    number_parameters() log N with N = data.cols(), as scikit-learn defines it (lower is better); the scoring pass of log_densities,
    no kernel of its own. Weights play no part. Throws like log_densities; an empty block gives NaN. */
    DLL_DECLSPEC double bic(ConstMatrixRef data) const;
    /** Extension: the Akaike information criterion, -2 N mean_log_density(data) + 2 number_parameters(). */
    DLL_DECLSPEC double aic(ConstMatrixRef data) const;
    /** Extension: argmax_k of every point's log-responsibilities, first maximum wins (the same pass as log_densities). */
    DLL_DECLSPEC std::vector<unsigned int> assign_labels(ConstMatrixRef data) const;
    /** Extension: the data.cols() x number_components() posteriors of `data` (the batch form of assign_responsibilities, normalised
    in the log domain). This one needs the N x K block: an E-step per row batch on a temporary device block. */
    DLL_DECLSPEC MatrixXd calculate_responsibilities(ConstMatrixRef data) const;
    /** Extension (scikit-learn's GaussianMixture.sample): `n` points drawn from the fitted mixture on the device, a point in every
    column (means().rows() x n: what fit takes); `labels`, if given, receives the component every point was drawn from. Point i is
    a pure function of (seed, i) and the fitted parameters (mlhip_em_sample: Philox4x32-10 counters, Box-Muller normals, the lower
    Cholesky factors of covariances()): the same seed gives the same points, a longer draw starts with the shorter one, and the
    result does not depend on the row batches (those of log_densities) or the device group it runs on. The model's own random
    engine is not touched: a fit after a sample draws what it would have drawn.
    @throw std::invalid_argument If `n < 0` or the model has not been fitted.
    @throw std::domain_error If a covariance is not positive definite.
    @throw std::runtime_error On device failures (no GPU: there is no CPU fallback). */
    DLL_DECLSPEC MatrixXd sample(Index n, std::uint64_t seed = 0, std::vector<unsigned int>* labels = nullptr) const;
    /** Extension (Gaussian-mixture regression, imputation): E[x_M | x_O] under the fitted mixture for every column of
    `data_observed`, on the device. `observed`: distinct coordinates < means().rows() in any order, at least one and not all of them;
    row c of `data_observed` holds coordinate observed[c] of every point. Returns (number of missing coordinates) x data.cols(): a
    point in every column, the missing coordinates in ascending order. `log_densities`, if given, receives data.cols() values: the
    log-density of every x_O under the marginal mixture. The definition and its fixed evaluation order: mlhip_em_condition,
    mlhip_em_conditional_means. The result does not depend on the row batches (those of log_densities) or the device group it runs on;
    the model is not changed.
    @throw std::invalid_argument If the model has not been fitted, `observed` is empty, holds every coordinate, one that is out of
    range or one twice, or `data_observed.rows() != observed.size()`.
    @throw std::domain_error If the observed block of a covariance is not positive definite.
    @throw std::runtime_error On device failures (no GPU: there is no CPU fallback). */
    DLL_DECLSPEC MatrixXd conditional_means(const std::vector<unsigned int>& observed, ConstMatrixRef data_observed,
                                            double* log_densities = nullptr) const;
    /** Extension (imputation of a table with gaps): `data` (means().rows() x N, a point in every column) with every NaN replaced by
    its conditional expectation under the fitted mixture given the coordinates THAT point has -- every point its own pattern of
    NaNs -- on the device. Observed entries keep their bits; a complete point comes back as it is, a point of all NaN as the
    mixture's mean. `log_densities`, if given, receives data.cols() values: the log-density of every point's observed coordinates
    under the marginal mixture (0 for a point of all NaN). `responsibilities`, if given, is resized to number_components() x
    data.cols(): the posterior membership of every point given what it has. The definition and its fixed evaluation order:
    mlhip_em_impute. A point's results do not depend on the other points, their order, the row batches (those of log_densities)
    or the device group it runs on; the model is not changed.
    @throw std::invalid_argument If the model has not been fitted or `data.rows() != means().rows()`.
    @throw std::domain_error If the observed block of a covariance is not positive definite for some point's pattern.
    @throw std::runtime_error On device failures (no GPU: there is no CPU fallback). */
    DLL_DECLSPEC MatrixXd impute(ConstMatrixRef data, double* log_densities = nullptr, MatrixXd* responsibilities = nullptr) const;
    /** Extension: the covariances Sigma_k,M|O of the conditioned components, K matrices of (number of missing coordinates)^2, the
    missing coordinates in ascending order (mlhip_em_condition_covariances; host only, no device). `observed` as for conditional_means.
    @throw std::invalid_argument If the model has not been fitted or for bad coordinates.
    @throw std::domain_error If the observed block of a covariance, or a conditioned covariance, is not positive definite. */
    DLL_DECLSPEC std::vector<MatrixXd> conditional_covariances(const std::vector<unsigned int>& observed) const;
    /** Extension (multiple imputation, predictive intervals): `n_draws` draws from p(x_M | x_O) under the fitted mixture for every
    column of `data_observed`, on the device. Arguments as for conditional_means. Returns (number of missing coordinates) x
    (n_draws * data.cols()): draw q of point i in column q * data.cols() + i. `labels`, if given, receives n_draws * data.cols()
    components, in the same order. Draw q of point i is a pure function of (seed, i, q), the point's observed coordinates and the
    parameters (mlhip_em_conditional_samples holds the definition): it does not depend on the row batches or the device group, and a
    seed shared with sample() shares no random word with it. The model and its random engine are not changed.
    @throw std::invalid_argument As conditional_means, or if n_draws < 0 or n_draws > 2^32 - 1.
    @throw std::domain_error If the observed block of a covariance, or a conditioned covariance, is not positive definite.
    @throw std::runtime_error On device failures (no GPU: there is no CPU fallback). */
    DLL_DECLSPEC MatrixXd conditional_samples(const std::vector<unsigned int>& observed, ConstMatrixRef data_observed, Index n_draws,
                                              std::uint64_t seed = 0, std::vector<unsigned int>* labels = nullptr) const;
    /** Extension (error bars on an imputed value, heteroscedastic regression bands): the predictive covariance Var[x_M | x_O] =
    sum_k r_k (Sigma_k,M|O + (t_k - y)(t_k - y)^T) of every column of `data_observed` under the fitted mixture, on the device; t_k the
    component predictions, r_k the marginal responsibilities, y = conditional_means. Arguments as for conditional_means. Returns
    (number of missing coordinates) x data.cols(), the variances of point i in column i -- with `full_covariance` (dM * dM) x
    data.cols(), column i holding the (symmetric) matrix of point i, whose diagonal has the bits of the default form. `means`, if
    given, receives conditional_means' result, bit for bit. The definition and its fixed evaluation order:
    mlhip_em_conditional_variances. The result does not depend on the row batches or the device group; the model is not changed.
    @throw std::invalid_argument As conditional_means.
    @throw std::domain_error If the observed block of a covariance, or a conditioned covariance, is not positive definite.
    @throw std::runtime_error On device failures (no GPU: there is no CPU fallback). */
    DLL_DECLSPEC MatrixXd conditional_variances(const std::vector<unsigned int>& observed, ConstMatrixRef data_observed,
                                                bool full_covariance = false, MatrixXd* means = nullptr) const;
    /** Extension (exceedance probabilities, the probability integral transform, p-values of an observed value): the predictive CDF
    P(x_j <= v | x_O) of every missing coordinate j under the fitted mixture, on the device, for every column of `data_observed` at
    that point's own values: `values` is (number of missing coordinates) x data.cols(), the missing coordinates in ascending order.
    Arguments as for conditional_means; returns a matrix of the shape of `values`. Given x_O, coordinate j follows the
    one-dimensional mixture sum_k r_k N(t_kj, Sigma_k,M|O[j][j]); the definition and its fixed evaluation order:
    mlhip_em_conditional_cdfs. The result does not depend on the row batches or the device group; the model is not changed.
    @throw std::invalid_argument As conditional_means, or if `values` has another shape.
    @throw std::domain_error If the observed block of a covariance, or a conditioned covariance, is not positive definite.
    @throw std::runtime_error On device failures (no GPU: there is no CPU fallback). */
    DLL_DECLSPEC MatrixXd conditional_cdfs(const std::vector<unsigned int>& observed, ConstMatrixRef data_observed, ConstMatrixRef values) const;
    /** Extension (exact predictive intervals and medians): the quantiles of the same one-dimensional mixtures, the inverse of
    conditional_cdfs, at every probability of `probabilities` (each strictly inside (0, 1)). Returns (number of missing coordinates) x
    (probabilities.size() * data.cols()): the quantiles at probability q of point i in column q * data.cols() + i, as conditional_samples
    lays out its draws. A safeguarded Newton search per (point, coordinate) inside the bracket of the components' own quantiles, with a
    fixed start, stopping rule and trip cap (mlhip_em_conditional_quantiles holds the definition): a pure function of the point, the
    parameters and the probability.
    @throw std::invalid_argument As conditional_means, or for a probability that is a NaN or not strictly inside (0, 1).
    @throw std::domain_error If the observed block of a covariance, or a conditioned covariance, is not positive definite.
    @throw std::runtime_error On device failures (no GPU: there is no CPU fallback). */
    DLL_DECLSPEC MatrixXd conditional_quantiles(const std::vector<unsigned int>& observed, ConstMatrixRef data_observed,
                                                const std::vector<double>& probabilities) const;
    const std::vector<unsigned int>& labels() const override { return labels_; }
    bool converged() const override { return converged_; }
    /** Extension: number of E-M iterations the last fit() ran. */
    unsigned int steps_done() const { return steps_done_; }
    /** Extension: frees the HBM copy of the data kept for responsibilities(). */
    DLL_DECLSPEC void release_device_data();

private:
    bool fit_weighted(ConstMatrixRef data, const double* weights);   // weights: null for the unweighted fit
    std::default_random_engine prng_;
    std::shared_ptr<const Clustering::CentroidsInitialiser> means_initialiser_;
    std::shared_ptr<const Clustering::ResponsibilitiesInitialiser> responsibilities_initialiser_;
    VectorXd mixing_probabilities_;
    MatrixXd means_;
    mutable MatrixXd responsibilities_;
    mutable bool responsibilities_on_device_ = false;
    std::vector<MatrixXd> covariances_;
    std::vector<MatrixXd> inverse_covariances_;
    VectorXd sqrt_covariance_determinants_;
    std::vector<unsigned int> labels_;
    double absolute_tolerance_;
    double relative_tolerance_;
    double log_likelihood_;
    unsigned int number_components_;
    unsigned int maximum_steps_;
    unsigned int steps_done_;
    bool verbose_;
    bool maximise_first_;
    bool converged_;
    CovarianceType covariance_type_ = CovarianceType::Full;
    CovarianceType fitted_covariance_type_ = CovarianceType::Full;   // the mode of the last fit(): number_parameters()
    mlhip_data* device_data_ = nullptr;
    double covariance_regularisation_ = 1e-15;   // MLHIP_DEFAULT_COVARIANCE_RIDGE
    unsigned int number_initialisations_ = 1;
    unsigned int best_initialisation_ = 0;
    std::vector<double> initialisation_log_likelihoods_;
    std::vector<unsigned int> initialisation_steps_;
    std::vector<int> initialisation_converged_;

    struct FitJob;                                                   // what the pieces of one fit share (EM.cpp)
    bool finish_exact_fit(unsigned int number_dimensions);
    void make_start(FitJob& job, double* covariance);
    bool run_verbose(const FitJob& job, double* covariance, std::vector<double>* last_inputs);
    void process_covariances(Index number_dimensions);
    std::vector<double> flat_covariances() const;                    // covariances() as one number_components() x d x d array
    void require_fitted_for(ConstMatrixRef data) const;
    void require_fitted() const;
    struct ConditionDims;                                            // the dimensions of a conditional call (EM.cpp)
    struct Conditioned;                                              // the model conditioned on observed coordinates (EM.cpp)
    /// The argument checks every conditional call on data opens with: a fitted shape, `observed` against it, the data's rows.
    ConditionDims check_conditional_call(const std::vector<unsigned int>& observed, ConstMatrixRef data_observed) const;
    /// What condition() adds to the marginal parts and the regression maps: nothing, the missing coordinates' covariances, those and
    /// their factors, or those and their scales.
    enum class ConditionParts { Marginal, Covariances, Factors, Scales };
    Conditioned condition(const std::vector<unsigned int>& observed, ConditionParts parts) const;
    /// conditional_cdfs (`values` given) and conditional_quantiles (`probabilities` given) behind their own argument checks.
    MatrixXd conditional_distribution(const std::vector<unsigned int>& observed, ConstMatrixRef data_observed, const ConstMatrixRef* values,
                                      const std::vector<double>* probabilities) const;
    void score(ConstMatrixRef data, double* log_density, unsigned int* labels) const;
};

}  // namespace ml
