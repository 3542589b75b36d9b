// ml::EM -- driver loop of Gaussian-mixture EM with the behaviour of the reference's ML/EM.cpp:17-188; the
// E-step / M-step bodies (ML/EM.cpp:190-263) and the label pass (:289-304) execute on the GPU through mlhip.h.
#include "ML/EM.hpp"

#include <algorithm>
#include <cmath>
#include <iostream>
#include <limits>
#include <stdexcept>
#include <typeinfo>

#include "DeviceInit.hpp"
#include "ML/Device.hpp"
#include "ML/LinearAlgebra.hpp"
#include "host/em_math.hpp"
#include "mlhip.h"

namespace ml {

using device::check;

namespace {
namespace host = mlhip::host;
using host::Covariance;

/// Owns a device block until release(): a fit that throws, and every batch of a query, frees its block.
struct DataGuard {
    mlhip_data* h = nullptr;
    ~DataGuard() { if (h) mlhip_data_free(h); }
    mlhip_data* release() { mlhip_data* t = h; h = nullptr; return t; }
};

void print_row(const double* p, Index n, Index stride)
{
    for (Index j = 0; j < n; ++j) std::cout << (j ? " " : "") << p[j * stride];
}
}  // namespace

/// What the pieces of one fit share: the sample, its device block, the shapes and the mode.
struct EM::FitJob {
    ConstMatrixRef data;
    mlhip_ctx* ctx;
    mlhip_data* dev;
    unsigned int d, n, K;                        // dimensions, this rank's points, components
    Covariance mode;
    std::vector<double> full;                    // K d d doubles: a start's full covariances, in the end the published ones
    std::vector<double> sample_covariance;       // formed once, by the first start that needs it
};

EM::EM(const unsigned int number_components)
    : means_initialiser_(std::make_shared<Clustering::Forgy>())
    , responsibilities_initialiser_(std::make_shared<Clustering::ClosestCentroid>(means_initialiser_))
    , mixing_probabilities_(number_components)
    , covariances_(number_components)
    , inverse_covariances_(number_components)
    , sqrt_covariance_determinants_(number_components)
    , absolute_tolerance_(1e-8)
    , relative_tolerance_(1e-8)
    , log_likelihood_(0)
    , number_components_(number_components)
    , maximum_steps_(1000)
    , steps_done_(0)
    , verbose_(false)
    , maximise_first_(false)
    , converged_(false)
{
    if (!number_components) throw std::invalid_argument("EM: At least one component required");
}

EM::~EM()
{
    if (device_data_) mlhip_data_free(device_data_);
}

void EM::release_device_data()
{
    if (device_data_) {
        if (responsibilities_on_device_) {
            try { (void)responsibilities(); } catch (...) {}
        }
        mlhip_data_free(device_data_);
        device_data_ = nullptr;
    }
    responsibilities_on_device_ = false;
}

void EM::set_seed(unsigned int seed) { prng_.seed(seed); }

void EM::set_absolute_tolerance(double absolute_tolerance)
{
    if (absolute_tolerance < 0) throw std::domain_error("EM: Negative absolute tolerance");
    absolute_tolerance_ = absolute_tolerance;
}

void EM::set_relative_tolerance(double relative_tolerance)
{
    if (relative_tolerance < 0) throw std::domain_error("EM: Negative relative tolerance");
    relative_tolerance_ = relative_tolerance;
}

void EM::set_covariance_regularisation(double covariance_regularisation)
{
    if (!(covariance_regularisation >= 0) || !std::isfinite(covariance_regularisation))
        throw std::domain_error("EM: Negative covariance regularisation");
    covariance_regularisation_ = covariance_regularisation;
}

void EM::set_number_initialisations(unsigned int number_initialisations)
{
    if (!number_initialisations) throw std::invalid_argument("EM: At least 1 initialisation required");
    number_initialisations_ = number_initialisations;
}

void EM::set_maximum_steps(unsigned int maximum_steps)
{
    if (maximum_steps < 2) throw std::invalid_argument("EM: At least two steps required for convergence test");
    maximum_steps_ = maximum_steps;
}

void EM::set_means_initialiser(std::shared_ptr<const Clustering::CentroidsInitialiser> means_initialiser)
{
    if (!means_initialiser) throw std::invalid_argument("EM: Null means initialiser");
    means_initialiser_ = means_initialiser;
}

void EM::set_responsibilities_initialiser(std::shared_ptr<const Clustering::ResponsibilitiesInitialiser> responsibilities_initialiser)
{
    if (!responsibilities_initialiser) throw std::invalid_argument("EM: Null responsibilities initialiser");
    responsibilities_initialiser_ = responsibilities_initialiser;
}

const MatrixXd& EM::covariance(unsigned int k) const
{
    if (k >= number_components_) throw std::invalid_argument("EM: Bad component index");
    return covariances_[k];
}

const MatrixXd& EM::responsibilities() const
{
    if (responsibilities_on_device_ && device_data_) {
        // Lazy device -> host copy of the N x K block (column-major, like the reference's member); the host matrix
        // (N*K doubles, 5 GB at the headline size) is only allocated now.
        responsibilities_.resize(static_cast<Index>(labels_.size()), number_components_);
        check(mlhip_em_responsibilities(device::context(), device_data_, number_components_, responsibilities_.data(),
                                        responsibilities_.rows()));
        responsibilities_on_device_ = false;
    }
    return responsibilities_;
}

MatrixXd EM::responsibilities_rows(Index first_row, Index number_rows) const
{
    const Index n = static_cast<Index>(labels_.size());
    if (first_row < 0 || number_rows < 0 || first_row > n || number_rows > n - first_row)
        throw std::invalid_argument("EM: Row range beyond the sample");
    MatrixXd out(number_rows, number_components_);
    if (responsibilities_on_device_ && device_data_) {
        check(mlhip_em_responsibilities_rows(device::context(), device_data_, number_components_, static_cast<uint64_t>(first_row),
                                             static_cast<uint64_t>(number_rows), out.data(), std::max<Index>(number_rows, 1)));
    } else {
        for (unsigned int k = 0; k < number_components_; ++k)
            std::copy_n(responsibilities_.col(k) + first_row, number_rows, out.col(k));
    }
    return out;
}

bool EM::fit(ConstMatrixRef data) { return fit_weighted(data, nullptr); }

bool EM::fit(ConstMatrixRef data, ConstVectorRef weights)
{
    if (weights.size() != data.cols()) throw std::invalid_argument("EM: One weight per data point required");
    return fit_weighted(data, weights.data());
}

bool EM::fit_weighted(ConstMatrixRef data, const double* weights)
{
    converged_ = false;
    steps_done_ = 0;
    best_initialisation_ = 0;
    const auto number_dimensions = static_cast<unsigned int>(data.rows());
    const auto sample_size = static_cast<unsigned int>(data.cols());
    const unsigned int K = number_components_;
    if (!number_dimensions) throw std::invalid_argument("EM: At least one dimension required");
    fitted_covariance_type_ = covariance_type_;

    // A previous fit's device block is no longer needed (its responsibilities are superseded).
    responsibilities_on_device_ = false;
    release_device_data();

    // The exact fit (N == K) and the "not enough data" test are about the WHOLE sample: in a row-sharded multi-rank job
    // (a hook or a communicator installed on the facade's context, which therefore exists already) the local shard may
    // be smaller than K, even empty, and every rank must still take the same branch and join the same collectives.
    int world = 1, rank = 0;
    mlhip_ctx* ctx = device::peek_context();
    if (ctx) check(mlhip_ctx_world(ctx, &world, &rank));
    if (world == 1) {
        if (sample_size < K) throw std::invalid_argument("EM: Not enough data ");
        if (sample_size > K) ctx = device::context();     // (N == K needs no device at all)
    }

    means_.resize(number_dimensions, K);
    mixing_probabilities_.fill(1. / static_cast<double>(K));
    labels_.resize(sample_size);

    if (world == 1 && sample_size == K) {
        // An exact deterministic fit: one Gaussian per sample, zero variance (ML/EM.cpp:108-118). Host only.
        responsibilities_.setZero(sample_size, sample_size);
        for (unsigned int i = 0; i < sample_size; ++i) {
            responsibilities_(i, i) = 1;
            std::copy_n(data.col(i), number_dimensions, means_.col(i));
            labels_[i] = i;
        }
        return finish_exact_fit(number_dimensions);
    }

    // ---- move the sample block to HBM (stays resident for the whole fit) ---------------------------------
    DataGuard dev;
    check(mlhip_data_upload(ctx, data.data(), number_dimensions, sample_size, data.outerStride(), &dev.h));
    // Row weights stay attached for the handle's lifetime: every statistics pass and log-likelihood below is weighted, the
    // initialisers' draws and the nearest-centroid pass see rows (mlhip.h, mlhip_data_set_weights).
    if (weights) check(mlhip_data_set_weights(ctx, dev.h, weights));
    // Before any M-step, so that the `maximise_first` start is regularised like every later one (mlhip_data_set_covariance_ridge).
    check(mlhip_data_set_covariance_ridge(ctx, dev.h, covariance_regularisation_));
    uint64_t n_global = 0;
    check(mlhip_data_shape(dev.h, nullptr, nullptr, &n_global));
    if (n_global < K) throw std::invalid_argument("EM: Not enough data ");       // the same on every rank
    if (n_global == K) {
        // The exact fit of a row-sharded sample: component (first_row + i) is this rank's sample i; the means are
        // put together across ranks, everything else is local (ML/EM.cpp:108-118).
        Index first_row = 0, total = 0;
        Clustering::detail::locate_rows(ctx, sample_size, first_row, total);
        responsibilities_.setZero(sample_size, K);
        means_.setZero();
        for (unsigned int i = 0; i < sample_size; ++i) {
            const auto g = static_cast<unsigned int>(first_row) + i;
            responsibilities_(i, g) = 1;
            std::copy_n(data.col(i), number_dimensions, means_.col(g));
            labels_[i] = g;
        }
        Clustering::detail::sum_across_ranks(ctx, means_);
        return finish_exact_fit(number_dimensions);
    }

    // The mode (extension, see ML/EM.hpp) and the parameter set in its form: mixing_probabilities_, means_ and `covariance`.
    static_assert(static_cast<int>(CovarianceType::Full) == static_cast<int>(Covariance::Full) &&
                      static_cast<int>(CovarianceType::Diagonal) == static_cast<int>(Covariance::Diagonal) &&
                      static_cast<int>(CovarianceType::Tied) == static_cast<int>(Covariance::Tied),
                  "CovarianceType names the modes in host::Covariance's order");
    FitJob job{data, ctx, dev.h, number_dimensions, sample_size, K, static_cast<Covariance>(covariance_type_), {}, {}};
    job.full.resize(host::covariance_doubles(Covariance::Full, K, number_dimensions));
    const std::size_t kd = static_cast<std::size_t>(number_dimensions) * K;
    const std::size_t n_cov = host::covariance_doubles(job.mode, K, number_dimensions);
    std::vector<double> covariance(n_cov);

    // R starts, drawn one after the other as R consecutive solo fits would draw them (the loops consume no random numbers), then the R
    // loops on the one resident block: the sample is uploaded once, weights, ridge and sample covariance are set once.
    const unsigned int R = number_initialisations_;
    std::vector<double> all_mixing, all_means, all_covariances;
    for (unsigned int r = 0; r < R; ++r) {
        make_start(job, covariance.data());
        all_mixing.insert(all_mixing.end(), mixing_probabilities_.data(), mixing_probabilities_.data() + K);
        all_means.insert(all_means.end(), means_.data(), means_.data() + kd);
        all_covariances.insert(all_covariances.end(), covariance.begin(), covariance.end());
    }
    std::vector<uint32_t> steps(R, 0);
    initialisation_converged_.assign(R, 0);
    initialisation_log_likelihoods_.assign(R, 0.0);
    uint32_t best = 0;
    if (!verbose_) {
        // The whole loop in one library call (same steps, same convergence test: ML/EM.cpp:143-170), with the M-step's closing
        // arithmetic and the K covariance factorizations on the device between two tests; several starts in one call of their own.
        if (R == 1)
            check(mlhip_em_iterate(ctx, dev.h, K, static_cast<int>(job.mode), all_mixing.data(), all_means.data(), all_covariances.data(),
                                   maximum_steps_, absolute_tolerance_, relative_tolerance_, steps.data(), initialisation_converged_.data(),
                                   initialisation_log_likelihoods_.data(), nullptr));
        else
            check(mlhip_em_iterate_restarts(ctx, dev.h, K, static_cast<int>(job.mode), R, all_mixing.data(), all_means.data(),
                                            all_covariances.data(), maximum_steps_, absolute_tolerance_, relative_tolerance_, steps.data(),
                                            initialisation_converged_.data(), initialisation_log_likelihoods_.data(), nullptr, &best));
    } else {
        // one start after the other; the winner's E-step state is put back by one E-step on the inputs of its last one
        std::vector<double> last_inputs, best_inputs;
        for (unsigned int r = 0; r < R; ++r) {
            if (R > 1) std::cout << "Initialisation " << r << "\n";
            std::copy_n(all_mixing.data() + static_cast<std::size_t>(r) * K, K, mixing_probabilities_.data());
            std::copy_n(all_means.data() + r * kd, kd, means_.data());
            std::copy_n(all_covariances.data() + r * n_cov, n_cov, covariance.data());
            steps_done_ = 0;
            initialisation_converged_[r] = run_verbose(job, covariance.data(), R > 1 ? &last_inputs : nullptr) ? 1 : 0;
            steps[r] = steps_done_;
            initialisation_log_likelihoods_[r] = log_likelihood_;
            std::copy_n(mixing_probabilities_.data(), K, all_mixing.data() + static_cast<std::size_t>(r) * K);
            std::copy_n(means_.data(), kd, all_means.data() + r * kd);
            std::copy_n(covariance.data(), n_cov, all_covariances.data() + r * n_cov);
            uint32_t so_far = 0;
            check(mlhip_em_select_restart(r + 1, initialisation_log_likelihoods_.data(), initialisation_converged_.data(), &so_far));
            if (so_far == r) best_inputs = last_inputs;
            best = so_far;
        }
        if (best + 1 != R) {
            // the winner's last E-step again (full covariances of its mode)
            host::covariances_as_full(job.mode, K, number_dimensions, best_inputs.data() + K + kd, job.full.data());
            double ll = 0;
            check(mlhip_em_expectation(ctx, dev.h, K, best_inputs.data(), best_inputs.data() + K, job.full.data(), &ll));
        }
    }

    // take the winner
    best_initialisation_ = best;
    initialisation_steps_.assign(steps.begin(), steps.end());
    std::copy_n(all_mixing.data() + static_cast<std::size_t>(best) * K, K, mixing_probabilities_.data());
    std::copy_n(all_means.data() + best * kd, kd, means_.data());
    log_likelihood_ = initialisation_log_likelihoods_[best];
    steps_done_ = steps[best];
    converged_ = initialisation_converged_[best] != 0;
    if (converged_) check(mlhip_em_labels(ctx, dev.h, K, labels_.data()));   // EM::calculate_labels, on convergence only

    // publish: every covariances_[k] is a full matrix (diagonal: a diagonal one; tied: each holds Sigma)
    host::covariances_as_full(job.mode, K, number_dimensions, all_covariances.data() + best * n_cov, job.full.data());
    const std::size_t dd = static_cast<std::size_t>(number_dimensions) * number_dimensions;
    for (unsigned int k = 0; k < K; ++k) {
        covariances_[k].resize(number_dimensions, number_dimensions);
        std::copy_n(job.full.data() + dd * k, dd, covariances_[k].data());
    }
    process_covariances(number_dimensions);
    // The responsibilities of the last E-step stay in HBM; responsibilities() allocates and fetches them on demand.
    responsibilities_.resize(0, 0);
    responsibilities_on_device_ = true;
    device_data_ = dev.release();
    return converged_;
}

bool EM::finish_exact_fit(unsigned int number_dimensions)
{
    for (unsigned int k = 0; k < number_components_; ++k) covariances_[k].setZero(number_dimensions, number_dimensions);
    log_likelihood_ = std::numeric_limits<double>::infinity();
    converged_ = true;
    initialisation_log_likelihoods_.assign(1, log_likelihood_);      // (the exact fit ignores number_initialisations(), like KMeans)
    initialisation_steps_.assign(1, 0);
    initialisation_converged_.assign(1, 1);
    return converged_;
}

// Start r -- what a solo fit would begin from, drawn from prng_ in order r = 0, 1, ... -- into mixing_probabilities_, means_ and
// `covariance` (the mode's form).
void EM::make_start(FitJob& job, double* covariance)
{
    const unsigned int K = job.K;
    const std::size_t dd = static_cast<std::size_t>(job.d) * job.d;
    mixing_probabilities_.fill(1. / static_cast<double>(K));
    if (maximise_first_) {
        // Start from responsibilities, then one M-step (ML/EM.cpp:120-125).
        const auto* closest = dynamic_cast<const Clustering::ClosestCentroid*>(responsibilities_initialiser_.get());
        const Clustering::ResponsibilitiesInitialiser& initialiser = *responsibilities_initialiser_;
        if (closest && typeid(initialiser) == typeid(Clustering::ClosestCentroid)) {
            // Library ClosestCentroid: draw the centroids on the host exactly as it would, run the nearest-centroid
            // pass (strict '<', first minimum wins: ML/Clustering.cpp:77-88) on the GPU and accumulate the one-hot
            // M-step from labels -- no N x K matrix is materialised.
            MatrixXd centroids(job.d, K);
            Clustering::detail::init_centroids(*closest->centroids_initialiser(), job.data, prng_, K, centroids, job.ctx, job.dev);
            double inertia = 0;
            uint64_t changed = 0;
            check(mlhip_kmeans_assign(job.ctx, job.dev, K, centroids.data(), &inertia, &changed));
            std::vector<unsigned int> hard(job.n);
            check(mlhip_kmeans_labels(job.ctx, job.dev, hard.data()));
            check(mlhip_em_maximisation_from_labels(job.ctx, job.dev, K, hard.data(), mixing_probabilities_.data(), means_.data(),
                                                    job.full.data()));
        } else {
            // User-defined initialiser: it fills a host N x K matrix, which is shipped to the device once.
            responsibilities_.resize(job.n, K);
            responsibilities_initialiser_->init(job.data, prng_, K, responsibilities_);
            check(mlhip_em_maximisation_from(job.ctx, job.dev, K, responsibilities_.data(), responsibilities_.rows(),
                                             mixing_probabilities_.data(), means_.data(), job.full.data()));
        }
    } else {
        // Sensible guesses: initialiser's means, every covariance = sample covariance (ML/EM.cpp:127-135).
        Clustering::detail::init_centroids(*means_initialiser_, job.data, prng_, K, means_, job.ctx, job.dev);   // identical on all ranks
        if (job.sample_covariance.empty()) {
            job.sample_covariance.resize(dd);
            check(mlhip_sample_covariance(job.ctx, job.dev, nullptr, job.sample_covariance.data()));
        }
        host::covariances_as_full(Covariance::Tied, K, job.d, job.sample_covariance.data(), job.full.data());
    }
    // Diagonal: the diagonal of the starting covariances (a one-hot / responsibility-weighted M-step entry by entry, or the sample
    // variances). Tied: their pooled sum_k pi_k Sigma_k (ascending k) -- the tied M-step of the starting responsibilities, or, from K
    // copies of the sample covariance with pi_k = 1 / K, that sum of K equal terms.
    host::covariances_from_full(job.mode, K, job.d, mixing_probabilities_.data(), job.full.data(), covariance);
}

// The verbose loop of one start: one E-step + M-step per trip through the per-step entry point of the mode, printed as the reference
// prints. Returns whether it converged; `last_inputs` (may be null) receives the parameters its last E-step ran on.
bool EM::run_verbose(const FitJob& job, double* covariance, std::vector<double>* last_inputs)
{
    const unsigned int K = job.K;
    const auto step_of_mode = job.mode == Covariance::Tied ? mlhip_em_step_tied : job.mode == Covariance::Diagonal ? mlhip_em_step_diag : mlhip_em_step;
    const std::size_t n_cov = host::covariance_doubles(job.mode, K, job.d);
    double old_log_likelihood = -std::numeric_limits<double>::infinity();
    for (unsigned int step = 0; step < maximum_steps_; ++step) {
        if (last_inputs) {
            last_inputs->assign(mixing_probabilities_.data(), mixing_probabilities_.data() + K);
            last_inputs->insert(last_inputs->end(), means_.data(), means_.data() + static_cast<std::size_t>(job.d) * K);
            last_inputs->insert(last_inputs->end(), covariance, covariance + n_cov);
        }
        // One E-step + M-step on the device; parameters are updated in place (ML/EM.cpp:145-147).
        check(step_of_mode(job.ctx, job.dev, K, mixing_probabilities_.data(), means_.data(), covariance, &log_likelihood_,
                           mixing_probabilities_.data(), means_.data(), covariance));
        ++steps_done_;

        std::cout << "Step " << step << "\n";
        std::cout << "Log-likelihood == " << log_likelihood_ << "\n";
        std::cout << "Mixing probabilities == ";
        print_row(mixing_probabilities_.data(), K, 1);
        std::cout << "\n";
        for (unsigned int k = 0; k < K; ++k) {
            std::cout << "Mean[" << k << "] == ";
            print_row(means_.col(k), job.d, 1);
            std::cout << "\n";
        }
        std::cout << "Responsibilities (first 10 rows):\n";
        // (only the rows that are printed cross the bus: ML/EM.cpp:155-156 prints topRows(10))
        MatrixXd r(std::min(job.n, 10u), K);
        check(mlhip_em_responsibilities_rows(job.ctx, job.dev, K, 0, static_cast<uint64_t>(r.rows()), r.data(), r.rows()));
        for (unsigned int i = 0; i < std::min(job.n, 10u); ++i) {
            print_row(r.data() + i, K, r.rows());
            std::cout << "\n";
        }
        std::cout << std::endl;

        if (step > 0) {
            const double ll_change = std::abs(log_likelihood_ - old_log_likelihood);
            if (ll_change < absolute_tolerance_ + relative_tolerance_ * std::max(std::abs(old_log_likelihood), std::abs(log_likelihood_)))
                return true;
        }
        old_log_likelihood = log_likelihood_;
    }
    return false;
}

std::vector<double> EM::flat_covariances() const
{
    const std::size_t dd = static_cast<std::size_t>(means_.rows()) * static_cast<std::size_t>(means_.rows());
    std::vector<double> flat(dd * number_components_);
    for (unsigned int k = 0; k < number_components_; ++k) std::copy_n(covariances_[k].data(), dd, flat.data() + dd * k);
    return flat;
}

void EM::assign_responsibilities(ConstVectorRef x, VectorRef u) const
{
    if (x.size() != means().rows()) throw std::invalid_argument("Wrong x size");
    if (u.size() != static_cast<Index>(number_components())) throw std::invalid_argument("Wrong u size");
    if (inverse_covariances_.empty() || inverse_covariances_[0].rows() != x.size())
        throw std::invalid_argument("EM: model has no fitted covariance decompositions");
    std::vector<double> diff(static_cast<std::size_t>(x.size()));
    double total = 0;
    for (unsigned int k = 0; k < number_components_; ++k) {
        const double* mean = means_.col(k);
        for (Index j = 0; j < x.size(); ++j) diff[static_cast<std::size_t>(j)] = x[j] - mean[j];
        const double q = LinearAlgebra::xAx_symmetric(inverse_covariances_[k], diff);
        u[k] = std::exp(-0.5 * q) * mixing_probabilities_[k] / sqrt_covariance_determinants_[k];
        total += u[k];
    }
    for (unsigned int k = 0; k < number_components_; ++k) u[k] /= total;
}

void EM::require_fitted_for(ConstMatrixRef data) const
{
    if (data.rows() != means().rows()) throw std::invalid_argument("Wrong data size");
    require_fitted();
}

void EM::require_fitted() const
{
    (void)device::context();                                 // (no GPU: the "no CPU fallback" error, whatever the model holds)
    if (inverse_covariances_.empty() || inverse_covariances_[0].rows() != means().rows())
        throw std::invalid_argument("EM: model has no fitted covariance decompositions");
}

void EM::score(ConstMatrixRef data, double* log_density, unsigned int* labels) const
{
    require_fitted_for(data);
    const Index d = data.rows(), n = data.cols(), batch = Clustering::detail::score_batch_rows();
    if (!n) return;
    const std::vector<double> cov_flat = flat_covariances();
    mlhip_ctx* ctx = device::context();
    for (Index first = 0; first < n; first += batch) {
        const Index rows = std::min(batch, n - first);
        DataGuard dev;
        check(mlhip_data_upload(ctx, data.col(first), static_cast<uint32_t>(d), static_cast<uint64_t>(rows), data.outerStride(), &dev.h));
        check(mlhip_em_score(ctx, dev.h, number_components_, MLHIP_COVARIANCE_FULL, mixing_probabilities_.data(), means_.data(),
                             cov_flat.data(), log_density ? log_density + first : nullptr, labels ? labels + first : nullptr));
    }
}

VectorXd EM::log_densities(ConstMatrixRef data) const
{
    VectorXd out(data.cols());
    score(data, out.data(), nullptr);
    return out;
}

double EM::mean_log_density(ConstMatrixRef data) const
{
    const VectorXd v = log_densities(data);
    double sum = 0;
    for (Index i = 0; i < v.size(); ++i) sum += v[i];
    return sum / static_cast<double>(v.size());
}

std::size_t EM::number_parameters() const
{
    // (the exact N == K fit counts too: its parameters exist, though its zero covariances have no decompositions)
    if (means().rows() == 0 || means().cols() != static_cast<Index>(number_components_))
        throw std::invalid_argument("EM: the model has not been fitted");
    const std::size_t d = static_cast<std::size_t>(means().rows()), K = number_components_;
    const std::size_t triangle = d * (d + 1) / 2;
    const std::size_t covariance = fitted_covariance_type_ == CovarianceType::Full       ? K * triangle
                                   : fitted_covariance_type_ == CovarianceType::Diagonal ? K * d
                                                                                         : triangle;
    return covariance + K * d + K - 1;
}

double EM::bic(ConstMatrixRef data) const
{
    const double n = static_cast<double>(data.cols()), p = static_cast<double>(number_parameters());
    return -2.0 * n * mean_log_density(data) + p * std::log(n);
}

double EM::aic(ConstMatrixRef data) const
{
    const double n = static_cast<double>(data.cols()), p = static_cast<double>(number_parameters());
    return -2.0 * n * mean_log_density(data) + 2.0 * p;
}

std::vector<unsigned int> EM::assign_labels(ConstMatrixRef data) const
{
    std::vector<unsigned int> out(static_cast<std::size_t>(data.cols()));
    score(data, nullptr, out.data());
    return out;
}

MatrixXd EM::calculate_responsibilities(ConstMatrixRef data) const
{
    require_fitted_for(data);
    const Index d = data.rows(), n = data.cols();
    const unsigned int K = number_components_;
    MatrixXd out(n, K);
    if (!n) return out;
    // (a batch holds its rows x K log-responsibilities on the device: at most 2^27 doubles of them)
    const Index batch = std::max<Index>(256, std::min(Clustering::detail::score_batch_rows(), (Index(1) << 27) / K));
    const std::vector<double> cov_flat = flat_covariances();
    mlhip_ctx* ctx = device::context();
    for (Index first = 0; first < n; first += batch) {
        const Index rows = std::min(batch, n - first);
        DataGuard dev;
        double ll = 0;
        check(mlhip_data_upload(ctx, data.col(first), static_cast<uint32_t>(d), static_cast<uint64_t>(rows), data.outerStride(), &dev.h));
        check(mlhip_em_expectation(ctx, dev.h, K, mixing_probabilities_.data(), means_.data(), cov_flat.data(), &ll));
        check(mlhip_em_responsibilities(ctx, dev.h, K, out.data() + first, n));
    }
    return out;
}

MatrixXd EM::sample(Index n, std::uint64_t seed, std::vector<unsigned int>* labels) const
{
    if (n < 0) throw std::invalid_argument("EM: Negative number of samples");
    const Index d = means().rows();
    // (the order of require_fitted_for: the shape -- here: that there is one --, the device, the decompositions)
    if (d == 0) throw std::invalid_argument("EM: model has no fitted covariance decompositions");
    require_fitted();
    MatrixXd out(d, n);
    if (labels) labels->resize(static_cast<std::size_t>(n));
    if (!n) return out;
    const std::vector<double> cov_flat = flat_covariances();
    mlhip_ctx* ctx = device::context();
    static_assert(sizeof(unsigned int) == sizeof(uint32_t), "labels are 32-bit");
    const Index batch = Clustering::detail::score_batch_rows();
    for (Index first = 0; first < n; first += batch) {
        const Index rows = std::min(batch, n - first);
        check(mlhip_em_sample(ctx, static_cast<uint32_t>(d), number_components_, MLHIP_COVARIANCE_FULL, mixing_probabilities_.data(),
                              means_.data(), cov_flat.data(), seed, static_cast<uint64_t>(first), static_cast<uint64_t>(rows), out.col(first), d,
                              labels ? reinterpret_cast<uint32_t*>(labels->data()) + first : nullptr));
    }
    return out;
}

namespace {
/// The checks of `observed` that the conditional calls share, against the model's dimension d (> 0).
void check_observed(const std::vector<unsigned int>& observed, Index d)
{
    if (observed.empty() || static_cast<Index>(observed.size()) >= d)
        throw std::invalid_argument("EM: between 1 and d - 1 coordinates must be observed");
    std::vector<char> seen(static_cast<std::size_t>(d), 0);
    for (const unsigned int c : observed) {
        if (static_cast<Index>(c) >= d) throw std::invalid_argument("EM: observed coordinate out of range");
        if (seen[c]) throw std::invalid_argument("EM: observed coordinate given twice");
        seen[c] = 1;
    }
}

/// f(context, handle, first, rows) for every batch of columns [first, first + rows) of `data_observed`, uploaded for the call.
template <class F> void for_each_batch(ConstMatrixRef data_observed, F&& f)
{
    mlhip_ctx* ctx = device::context();
    const Index n = data_observed.cols(), batch = Clustering::detail::score_batch_rows();
    for (Index first = 0; first < n; first += batch) {
        const Index rows = std::min(batch, n - first);
        DataGuard dev;
        check(mlhip_data_upload(ctx, data_observed.col(first), static_cast<uint32_t>(data_observed.rows()), static_cast<uint64_t>(rows),
                                data_observed.outerStride(), &dev.h));
        f(ctx, dev.h, first, rows);
    }
}

/// A result of `blocks` blocks (one per draw or probability) of n points x `width` values, block q of point i at (q * n + i) * width.
/// A batch's call writes its blocks batch rows apart, the result's lie n apart: target() is where the call writes -- the result
/// itself where the batch is all n points, else a buffer --, and scatter() then copies the buffer's blocks to their places.
template <class T> struct BlockScatter {
    T* out;                                                      // (null: the result is not asked for)
    Index width, blocks, n;
    std::vector<T> block;
    T* target(Index rows)
    {
        if (!out || rows == n) return out;
        block.resize(static_cast<std::size_t>(blocks * rows * width));
        return block.data();
    }
    void scatter(Index first, Index rows) const
    {
        if (!out || rows == n) return;
        for (Index q = 0; q < blocks; ++q)
            std::copy_n(block.data() + static_cast<std::size_t>(q * rows * width), rows * width, out + (q * n + first) * width);
    }
};
}  // namespace

struct EM::ConditionDims {
    Index d, d_observed, d_missing, n;
};

/// The model conditioned on the observed coordinates, as the mlhip_em_conditional_* calls take it.
struct EM::Conditioned {
    std::vector<double> means_observed, covariances_observed, maps, means_missing, covariances_missing, factors, scales, inverse_scales;
};

EM::ConditionDims EM::check_conditional_call(const std::vector<unsigned int>& observed, ConstMatrixRef data_observed) const
{
    const Index d = means_.rows();
    // (the order of sample: that there is a shape, the arguments against it; then, in condition(), the device and the decompositions)
    if (d == 0) throw std::invalid_argument("EM: model has no fitted covariance decompositions");
    check_observed(observed, d);
    const Index d_observed = static_cast<Index>(observed.size());
    if (data_observed.rows() != d_observed) throw std::invalid_argument("Wrong data size");
    return {d, d_observed, d - d_observed, data_observed.cols()};
}

EM::Conditioned EM::condition(const std::vector<unsigned int>& observed, ConditionParts parts) const
{
    require_fitted();
    const unsigned int K = number_components_;
    const Index d = means_.rows(), d_observed = static_cast<Index>(observed.size()), d_missing = d - d_observed;
    const std::vector<double> cov_flat = flat_covariances();
    Conditioned c;
    c.means_observed.resize(static_cast<std::size_t>(K * d_observed));
    c.covariances_observed.resize(static_cast<std::size_t>(K * d_observed * d_observed));
    c.maps.resize(static_cast<std::size_t>(K * d_missing * d_observed));
    c.means_missing.resize(static_cast<std::size_t>(K * d_missing));
    static_assert(sizeof(unsigned int) == sizeof(uint32_t), "coordinates are 32-bit");
    const uint32_t* coordinates = reinterpret_cast<const uint32_t*>(observed.data());
    check(mlhip_em_condition(static_cast<uint32_t>(d), K, MLHIP_COVARIANCE_FULL, means_.data(), cov_flat.data(), coordinates,
                             static_cast<uint32_t>(d_observed), c.means_observed.data(), c.covariances_observed.data(), c.maps.data(),
                             c.means_missing.data()));
    if (parts == ConditionParts::Marginal) return c;
    c.covariances_missing.resize(static_cast<std::size_t>(K * d_missing * d_missing));
    if (parts == ConditionParts::Factors) c.factors.resize(c.covariances_missing.size());
    check(mlhip_em_condition_covariances(static_cast<uint32_t>(d), K, MLHIP_COVARIANCE_FULL, cov_flat.data(), coordinates,
                                         static_cast<uint32_t>(d_observed), c.covariances_missing.data(),
                                         c.factors.empty() ? nullptr : c.factors.data()));
    if (parts != ConditionParts::Scales) return c;
    c.scales.resize(static_cast<std::size_t>(K * d_missing));
    c.inverse_scales.resize(c.scales.size());
    check(mlhip_em_condition_scales(K, static_cast<uint32_t>(d_missing), c.covariances_missing.data(), c.scales.data(), c.inverse_scales.data()));
    return c;
}

MatrixXd EM::conditional_means(const std::vector<unsigned int>& observed, ConstMatrixRef data_observed, double* log_densities) const
{
    const ConditionDims s = check_conditional_call(observed, data_observed);
    const Conditioned c = condition(observed, ConditionParts::Marginal);
    MatrixXd out(s.d_missing, s.n);
    if (!s.n) return out;
    for_each_batch(data_observed, [&](mlhip_ctx* ctx, mlhip_data* block, Index first, Index) {
        check(mlhip_em_conditional_means(ctx, block, number_components_, static_cast<uint32_t>(s.d_missing), mixing_probabilities_.data(),
                                         c.means_observed.data(), c.covariances_observed.data(), c.maps.data(), c.means_missing.data(),
                                         out.col(first), s.d_missing, log_densities ? log_densities + first : nullptr));
    });
    return out;
}

MatrixXd EM::impute(ConstMatrixRef data, double* log_densities, MatrixXd* responsibilities) const
{
    const Index d = means_.rows(), n = data.cols();
    // (the order of sample: that there is a shape, the arguments against it, then the device and the decompositions)
    if (d == 0) throw std::invalid_argument("EM: model has no fitted covariance decompositions");
    if (data.rows() != d) throw std::invalid_argument("Wrong data size");
    require_fitted();
    const unsigned int K = number_components_;
    MatrixXd out(d, n);
    if (responsibilities) responsibilities->resize(K, n);
    if (!n) return out;
    const std::vector<double> cov_flat = flat_covariances();
    mlhip_ctx* ctx = device::context();
    const Index batch = Clustering::detail::score_batch_rows();
    std::vector<double> packed;                                  // (mlhip_em_impute takes contiguous points)
    for (Index first = 0; first < n; first += batch) {
        const Index rows = std::min(batch, n - first);
        const double* x = data.col(first);
        if (data.outerStride() != d) {
            packed.resize(static_cast<std::size_t>(rows * d));
            for (Index i = 0; i < rows; ++i) std::copy_n(data.col(first + i), d, packed.data() + i * d);
            x = packed.data();
        }
        check(mlhip_em_impute(ctx, static_cast<uint32_t>(d), K, MLHIP_COVARIANCE_FULL, mixing_probabilities_.data(), means_.data(),
                              cov_flat.data(), x, static_cast<uint64_t>(rows), out.col(first), log_densities ? log_densities + first : nullptr,
                              responsibilities ? responsibilities->col(first) : nullptr));
    }
    return out;
}

std::vector<MatrixXd> EM::conditional_covariances(const std::vector<unsigned int>& observed) const
{
    const Index d = means().rows();
    if (d == 0) throw std::invalid_argument("EM: model has no fitted covariance decompositions");
    check_observed(observed, d);
    require_fitted();
    const unsigned int K = number_components_;
    const Index d_missing = d - static_cast<Index>(observed.size());
    const std::vector<double> cov_flat = flat_covariances();
    std::vector<double> flat(static_cast<std::size_t>(K * d_missing * d_missing));
    static_assert(sizeof(unsigned int) == sizeof(uint32_t), "coordinates are 32-bit");
    check(mlhip_em_condition_covariances(static_cast<uint32_t>(d), K, MLHIP_COVARIANCE_FULL, cov_flat.data(),
                                         reinterpret_cast<const uint32_t*>(observed.data()), static_cast<uint32_t>(observed.size()),
                                         flat.data(), nullptr));
    std::vector<MatrixXd> out;
    for (unsigned int k = 0; k < K; ++k) {
        MatrixXd c(d_missing, d_missing);
        std::copy_n(flat.data() + static_cast<std::size_t>(k) * d_missing * d_missing, d_missing * d_missing, c.data());   // (symmetric)
        out.push_back(std::move(c));
    }
    return out;
}

MatrixXd EM::conditional_samples(const std::vector<unsigned int>& observed, ConstMatrixRef data_observed, Index n_draws, std::uint64_t seed,
                                 std::vector<unsigned int>* labels) const
{
    const ConditionDims s = check_conditional_call(observed, data_observed);
    if (n_draws < 0 || static_cast<std::uint64_t>(n_draws) > 0xFFFFFFFFull) throw std::invalid_argument("EM: n_draws must be 0 .. 2^32 - 1");
    const Conditioned c = condition(observed, ConditionParts::Factors);
    MatrixXd out(s.d_missing, n_draws * s.n);
    if (labels) labels->assign(static_cast<std::size_t>(n_draws * s.n), 0u);
    if (!s.n || !n_draws) return out;
    BlockScatter<double> draws{out.data(), s.d_missing, n_draws, s.n, {}};
    BlockScatter<uint32_t> draw_labels{labels ? labels->data() : nullptr, 1, n_draws, s.n, {}};
    for_each_batch(data_observed, [&](mlhip_ctx* ctx, mlhip_data* block, Index first, Index rows) {
        check(mlhip_em_conditional_samples(ctx, block, number_components_, static_cast<uint32_t>(s.d_missing), mixing_probabilities_.data(),
                                           c.means_observed.data(), c.covariances_observed.data(), c.maps.data(), c.means_missing.data(),
                                           c.factors.data(), seed, static_cast<uint64_t>(first), 0u, static_cast<uint32_t>(n_draws),
                                           draws.target(rows), s.d_missing, draw_labels.target(rows)));
        draws.scatter(first, rows);
        draw_labels.scatter(first, rows);
    });
    return out;
}

MatrixXd EM::conditional_variances(const std::vector<unsigned int>& observed, ConstMatrixRef data_observed, bool full_covariance,
                                   MatrixXd* means) const
{
    const ConditionDims s = check_conditional_call(observed, data_observed);
    const Conditioned c = condition(observed, ConditionParts::Covariances);
    const Index width = full_covariance ? s.d_missing * s.d_missing : s.d_missing;
    MatrixXd out(width, s.n);
    if (means) means->resize(s.d_missing, s.n);
    if (!s.n) return out;
    for_each_batch(data_observed, [&](mlhip_ctx* ctx, mlhip_data* block, Index first, Index) {
        check(mlhip_em_conditional_variances(ctx, block, number_components_, static_cast<uint32_t>(s.d_missing), mixing_probabilities_.data(),
                                             c.means_observed.data(), c.covariances_observed.data(), c.maps.data(), c.means_missing.data(),
                                             c.covariances_missing.data(), full_covariance ? 1 : 0, out.col(first), width,
                                             means ? means->col(first) : nullptr, s.d_missing, nullptr));
    });
    return out;
}

MatrixXd EM::conditional_distribution(const std::vector<unsigned int>& observed, ConstMatrixRef data_observed, const ConstMatrixRef* values,
                                      const std::vector<double>* probabilities) const
{
    const ConditionDims s = check_conditional_call(observed, data_observed);
    if (values && (values->rows() != s.d_missing || values->cols() != s.n)) throw std::invalid_argument("EM: values must hold one row per missing coordinate and one column per point");
    const Index n_probabilities = probabilities ? static_cast<Index>(probabilities->size()) : 1;
    if (probabilities) {
        if (static_cast<std::uint64_t>(n_probabilities) > 0xFFFFFFFFull) throw std::invalid_argument("EM: too many probabilities");
        for (const double p : *probabilities)
            if (!(p > 0.0 && p < 1.0)) throw std::invalid_argument("EM: a probability must lie strictly inside (0, 1)");
    }
    const Conditioned c = condition(observed, ConditionParts::Scales);
    MatrixXd out(s.d_missing, n_probabilities * s.n);
    if (!s.n || !n_probabilities) return out;
    BlockScatter<double> quantiles{out.data(), s.d_missing, n_probabilities, s.n, {}};
    for_each_batch(data_observed, [&](mlhip_ctx* ctx, mlhip_data* block, Index first, Index rows) {
        if (values) {
            check(mlhip_em_conditional_cdfs(ctx, block, number_components_, static_cast<uint32_t>(s.d_missing), mixing_probabilities_.data(),
                                            c.means_observed.data(), c.covariances_observed.data(), c.maps.data(), c.means_missing.data(),
                                            c.scales.data(), c.inverse_scales.data(), values->col(first), values->outerStride(), out.col(first),
                                            s.d_missing, nullptr, s.d_missing, nullptr));
            return;
        }
        check(mlhip_em_conditional_quantiles(ctx, block, number_components_, static_cast<uint32_t>(s.d_missing), mixing_probabilities_.data(),
                                             c.means_observed.data(), c.covariances_observed.data(), c.maps.data(), c.means_missing.data(),
                                             c.scales.data(), c.inverse_scales.data(), probabilities->data(),
                                             static_cast<uint32_t>(n_probabilities), quantiles.target(rows), s.d_missing, nullptr, s.d_missing,
                                             nullptr, nullptr));
        quantiles.scatter(first, rows);
    });
    return out;
}

MatrixXd EM::conditional_cdfs(const std::vector<unsigned int>& observed, ConstMatrixRef data_observed, ConstMatrixRef values) const
{
    return conditional_distribution(observed, data_observed, &values, nullptr);
}

MatrixXd EM::conditional_quantiles(const std::vector<unsigned int>& observed, ConstMatrixRef data_observed,
                                   const std::vector<double>& probabilities) const
{
    return conditional_distribution(observed, data_observed, nullptr, &probabilities);
}

void EM::process_covariances(const Index number_dimensions)
{
    // Inverse and sqrt(det) of every covariance for the host point query (ML/EM.cpp:274-287).
    for (unsigned int k = 0; k < number_components_; ++k) {
        inverse_covariances_[k].resize(number_dimensions, number_dimensions);
        check(mlhip_process_covariance(static_cast<uint32_t>(number_dimensions), covariances_[k].data(),
                                       inverse_covariances_[k].data(), &sqrt_covariance_determinants_[k]));
    }
}

}  // namespace ml
