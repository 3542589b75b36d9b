// Flat C handles over the C++ facade (include/mlpp_c.h). Error text goes through the same thread-local slot as
// mlhip_last_error(): a failing facade call rethrows the C-ABI message, a facade-level exception is recorded here.
#include "mlpp_c.h"

#include <algorithm>
#include <limits>
#include <memory>
#include <random>
#include <stdexcept>
#include <string>

#include "host/facade/DeviceInit.hpp"
#include "ML/Clustering.hpp"
#include "ML/Device.hpp"
#include "ML/EM.hpp"
#include "ML/KMeans.hpp"
#include "ML/LinearAlgebra.hpp"
#include "ML/LinearRegression.hpp"
#include "mlhip.h"

extern "C" void mlhip_set_last_error_(const char* msg);   // defined in runtime/context.cpp

using namespace ml;

struct mlpp_centroids_initialiser { std::shared_ptr<const Clustering::CentroidsInitialiser> p; };
struct mlpp_responsibilities_initialiser { std::shared_ptr<const Clustering::ResponsibilitiesInitialiser> p; };
struct mlpp_em { EM em; Index d = 0; Index n = 0; explicit mlpp_em(unsigned K) : em(K) {} };
struct mlpp_kmeans { Clustering::KMeans km; Index d = 0; Index n = 0; explicit mlpp_kmeans(unsigned K) : km(K) {} };

namespace {
template <class F> int guarded(F&& f)
{
    try { f(); return MLHIP_OK; }
    catch (const std::invalid_argument& e) { mlhip_set_last_error_(e.what()); return MLHIP_E_INVALID_ARGUMENT; }
    catch (const std::domain_error& e) { mlhip_set_last_error_(e.what()); return MLHIP_E_DOMAIN; }
    catch (const std::exception& e) { mlhip_set_last_error_(e.what()); return MLHIP_E_RUNTIME; }
}
void need(const void* p) { if (!p) throw std::invalid_argument("null handle or pointer"); }
std::default_random_engine make_engine(int seed_set, uint32_t seed)
{
    std::default_random_engine e;
    if (seed_set) e.seed(seed);
    return e;
}
/// min(capacity, v.size()) entries of v to `out`, v.size() to *count (the per-initialisation getters).
template <class T, class U> void copy_per_initialisation(const std::vector<T>& v, U* out, uint32_t capacity, uint32_t* count)
{
    need(count);
    if (capacity) need(out);
    *count = static_cast<uint32_t>(v.size());
    for (uint32_t r = 0; r < capacity && r < v.size(); ++r) out[r] = static_cast<U>(v[r]);
}
}  // namespace

extern "C" {

int mlpp_forgy_create(mlpp_centroids_initialiser** out) { return guarded([&] { need(out); *out = new mlpp_centroids_initialiser{std::make_shared<Clustering::Forgy>()}; }); }
int mlpp_random_partition_create(mlpp_centroids_initialiser** out) { return guarded([&] { need(out); *out = new mlpp_centroids_initialiser{std::make_shared<Clustering::RandomPartition>()}; }); }
int mlpp_kpp_create(mlpp_centroids_initialiser** out) { return guarded([&] { need(out); *out = new mlpp_centroids_initialiser{std::make_shared<Clustering::KPP>()}; }); }
int mlpp_fixed_point_kpp_create(mlpp_centroids_initialiser** out)
{
    return guarded([&] { need(out); *out = new mlpp_centroids_initialiser{std::make_shared<Clustering::FixedPointKPP>()}; });
}
int mlpp_fixed_centroids_create(const double* centroids, uint32_t K, uint32_t d, mlpp_centroids_initialiser** out)
{
    return guarded([&] {
        need(out); need(centroids);
        MatrixXd c(d, K);
        std::copy_n(centroids, static_cast<std::size_t>(K) * d, c.data());   // K x d row-major == d x K column-major
        *out = new mlpp_centroids_initialiser{std::make_shared<Clustering::FixedCentroids>(c)};
    });
}
int mlpp_centroids_initialiser_destroy(mlpp_centroids_initialiser* h) { delete h; return MLHIP_OK; }
int mlpp_centroids_initialiser_run(const mlpp_centroids_initialiser* h, const double* data, uint64_t n, uint32_t d, uint32_t K,
                                   int seed_set, uint32_t seed, double* centroids_out)
{
    return guarded([&] {
        need(h); need(data); need(centroids_out);
        auto prng = make_engine(seed_set, seed);
        h->p->init(ConstMatrixRef(data, d, static_cast<Index>(n)), prng, K, MatrixRef(centroids_out, d, K, d));
    });
}
int mlpp_centroids_initialiser_run_on_device(const mlpp_centroids_initialiser* h, const double* data, uint64_t n, uint32_t d, uint32_t K,
                                             int seed_set, uint32_t seed, double* centroids_out)
{
    return guarded([&] {
        need(h); need(data); need(centroids_out);
        auto prng = make_engine(seed_set, seed);
        mlhip_ctx* ctx = device::context();
        mlhip_data* dev = nullptr;
        device::check(mlhip_data_upload(ctx, data, d, n, d, &dev));
        struct Free { mlhip_data* p; ~Free() { mlhip_data_free(p); } } free_it{dev};
        Clustering::detail::init_centroids(*h->p, ConstMatrixRef(data, d, static_cast<Index>(n)), prng, K, MatrixRef(centroids_out, d, K, d), ctx, dev);
    });
}
int mlpp_closest_centroid_create(const mlpp_centroids_initialiser* ci, mlpp_responsibilities_initialiser** out)
{
    return guarded([&] {
        need(out);
        *out = new mlpp_responsibilities_initialiser{std::make_shared<Clustering::ClosestCentroid>(ci ? ci->p : nullptr)};
    });
}
int mlpp_responsibilities_initialiser_destroy(mlpp_responsibilities_initialiser* h) { delete h; return MLHIP_OK; }
int mlpp_responsibilities_initialiser_run(const mlpp_responsibilities_initialiser* h, const double* data, uint64_t n, uint32_t d,
                                          uint32_t K, int seed_set, uint32_t seed, double* resp_out)
{
    return guarded([&] {
        need(h); need(data); need(resp_out);
        auto prng = make_engine(seed_set, seed);
        h->p->init(ConstMatrixRef(data, d, static_cast<Index>(n)), prng, K, MatrixRef(resp_out, static_cast<Index>(n), K, static_cast<Index>(n)));
    });
}

// ---- EM ----
int mlpp_em_create(uint32_t K, mlpp_em** out) { return guarded([&] { need(out); *out = new mlpp_em(K); }); }
int mlpp_em_destroy(mlpp_em* h) { delete h; return MLHIP_OK; }
int mlpp_em_set_seed(mlpp_em* h, uint32_t v) { return guarded([&] { need(h); h->em.set_seed(v); }); }
int mlpp_em_set_absolute_tolerance(mlpp_em* h, double v) { return guarded([&] { need(h); h->em.set_absolute_tolerance(v); }); }
int mlpp_em_set_relative_tolerance(mlpp_em* h, double v) { return guarded([&] { need(h); h->em.set_relative_tolerance(v); }); }
int mlpp_em_set_covariance_regularisation(mlpp_em* h, double v) { return guarded([&] { need(h); h->em.set_covariance_regularisation(v); }); }
int mlpp_em_covariance_regularisation(const mlpp_em* h, double* out) { return guarded([&] { need(h); need(out); *out = h->em.covariance_regularisation(); }); }
int mlpp_em_set_number_initialisations(mlpp_em* h, uint32_t v) { return guarded([&] { need(h); h->em.set_number_initialisations(v); }); }
int mlpp_em_number_initialisations(const mlpp_em* h, uint32_t* out) { return guarded([&] { need(h); need(out); *out = h->em.number_initialisations(); }); }
int mlpp_em_best_initialisation(const mlpp_em* h, uint32_t* out) { return guarded([&] { need(h); need(out); *out = h->em.best_initialisation(); }); }
int mlpp_em_initialisation_log_likelihoods(const mlpp_em* h, double* out, uint32_t capacity, uint32_t* count)
{
    return guarded([&] { need(h); copy_per_initialisation(h->em.initialisation_log_likelihoods(), out, capacity, count); });
}
int mlpp_em_initialisation_steps(const mlpp_em* h, uint32_t* out, uint32_t capacity, uint32_t* count)
{
    return guarded([&] { need(h); copy_per_initialisation(h->em.initialisation_steps(), out, capacity, count); });
}
int mlpp_em_initialisation_converged(const mlpp_em* h, int* out, uint32_t capacity, uint32_t* count)
{
    return guarded([&] { need(h); copy_per_initialisation(h->em.initialisation_converged(), out, capacity, count); });
}
int mlpp_em_set_maximum_steps(mlpp_em* h, uint32_t v) { return guarded([&] { need(h); h->em.set_maximum_steps(v); }); }
int mlpp_em_set_means_initialiser(mlpp_em* h, const mlpp_centroids_initialiser* i) { return guarded([&] { need(h); h->em.set_means_initialiser(i ? i->p : nullptr); }); }
int mlpp_em_set_responsibilities_initialiser(mlpp_em* h, const mlpp_responsibilities_initialiser* i) { return guarded([&] { need(h); h->em.set_responsibilities_initialiser(i ? i->p : nullptr); }); }
int mlpp_em_set_verbose(mlpp_em* h, int v) { return guarded([&] { need(h); h->em.set_verbose(v != 0); }); }
int mlpp_em_set_maximise_first(mlpp_em* h, int v) { return guarded([&] { need(h); h->em.set_maximise_first(v != 0); }); }
int mlpp_em_set_covariance_type(mlpp_em* h, int covariance_type)
{
    return guarded([&] {
        need(h);
        h->em.set_covariance_type(covariance_type == 2 ? ml::EM::CovarianceType::Tied
                                  : covariance_type ? ml::EM::CovarianceType::Diagonal : ml::EM::CovarianceType::Full);
    });
}
int mlpp_em_fit(mlpp_em* h, const double* data, uint64_t n, uint32_t d, int* converged)
{
    return guarded([&] {
        need(h); need(converged);
        if (n && d) need(data);
        const bool ok = h->em.fit(ConstMatrixRef(data, d, static_cast<Index>(n)));
        h->d = d; h->n = static_cast<Index>(n);
        *converged = ok ? 1 : 0;
    });
}
int mlpp_em_fit_weighted(mlpp_em* h, const double* data, const double* weights, uint64_t n, uint32_t d, int* converged)
{
    return guarded([&] {
        need(h); need(converged);
        if (n && d) need(data);
        if (n) need(weights);
        const bool ok = h->em.fit(ConstMatrixRef(data, d, static_cast<Index>(n)), ConstVectorRef(weights, static_cast<Index>(n)));
        h->d = d; h->n = static_cast<Index>(n);
        *converged = ok ? 1 : 0;
    });
}
int mlpp_em_number_components(const mlpp_em* h, uint32_t* out) { return guarded([&] { need(h); need(out); *out = h->em.number_components(); }); }
int mlpp_em_dims(const mlpp_em* h, uint32_t* d, uint64_t* n) { return guarded([&] { need(h); if (d) *d = static_cast<uint32_t>(h->em.means().rows()); if (n) *n = static_cast<uint64_t>(h->em.labels().size()); }); }
int mlpp_em_means(const mlpp_em* h, double* out) { return guarded([&] { need(h); need(out); std::copy_n(h->em.means().data(), h->em.means().size(), out); }); }
int mlpp_em_covariance(const mlpp_em* h, uint32_t k, double* out) { return guarded([&] { need(h); need(out); const MatrixXd& c = h->em.covariance(k); std::copy_n(c.data(), c.size(), out); }); }
int mlpp_em_mixing_probabilities(const mlpp_em* h, double* out) { return guarded([&] { need(h); need(out); std::copy_n(h->em.mixing_probabilities().data(), h->em.mixing_probabilities().size(), out); }); }
int mlpp_em_responsibilities(const mlpp_em* h, double* out) { return guarded([&] { need(h); need(out); const MatrixXd& r = h->em.responsibilities(); std::copy_n(r.data(), r.size(), out); }); }
int mlpp_em_responsibilities_rows(const mlpp_em* h, uint64_t first_row, uint64_t n_rows, double* out)
{
    return guarded([&] {
        need(h); need(out);
        const MatrixXd r = h->em.responsibilities_rows(static_cast<Index>(first_row), static_cast<Index>(n_rows));
        std::copy_n(r.data(), r.size(), out);
    });
}
int mlpp_em_log_likelihood(const mlpp_em* h, double* out) { return guarded([&] { need(h); need(out); *out = h->em.log_likelihood(); }); }
int mlpp_em_labels(const mlpp_em* h, uint32_t* out) { return guarded([&] { need(h); need(out); std::copy(h->em.labels().begin(), h->em.labels().end(), out); }); }
int mlpp_em_converged(const mlpp_em* h, int* out) { return guarded([&] { need(h); need(out); *out = h->em.converged() ? 1 : 0; }); }
int mlpp_em_steps_done(const mlpp_em* h, uint32_t* out) { return guarded([&] { need(h); need(out); *out = h->em.steps_done(); }); }
int mlpp_em_assign_responsibilities(const mlpp_em* h, const double* x, uint32_t xlen, double* u, uint32_t ulen)
{
    return guarded([&] { need(h); need(x); need(u); h->em.assign_responsibilities(ConstVectorRef(x, xlen), VectorRef(u, ulen)); });
}

int mlpp_em_score_samples(const mlpp_em* h, const double* data, uint64_t n, uint32_t d, double* out)
{
    return guarded([&] {
        need(h); need(data); need(out);
        const VectorXd v = h->em.log_densities(ConstMatrixRef(data, d, static_cast<Index>(n), d));
        std::copy_n(v.data(), v.size(), out);
    });
}
int mlpp_em_predict(const mlpp_em* h, const double* data, uint64_t n, uint32_t d, uint32_t* out)
{
    return guarded([&] {
        need(h); need(data); need(out);
        const std::vector<unsigned int> v = h->em.assign_labels(ConstMatrixRef(data, d, static_cast<Index>(n), d));
        std::copy(v.begin(), v.end(), out);
    });
}
int mlpp_em_number_parameters(const mlpp_em* h, uint64_t* out)
{
    return guarded([&] { need(h); need(out); *out = h->em.number_parameters(); });
}
int mlpp_em_bic(const mlpp_em* h, const double* data, uint64_t n, uint32_t d, double* out)
{
    return guarded([&] { need(h); need(data); need(out); *out = h->em.bic(ConstMatrixRef(data, d, static_cast<Index>(n), d)); });
}
int mlpp_em_aic(const mlpp_em* h, const double* data, uint64_t n, uint32_t d, double* out)
{
    return guarded([&] { need(h); need(data); need(out); *out = h->em.aic(ConstMatrixRef(data, d, static_cast<Index>(n), d)); });
}
int mlpp_silhouette_samples(const double* x, uint64_t n, uint32_t d, const uint32_t* labels, uint32_t K, const uint64_t* rows, uint64_t n_rows,
                            double* s_out)
{
    return guarded([&] {
        need(x); need(labels); need(s_out);
        if (n > static_cast<uint64_t>(std::numeric_limits<Index>::max())) throw std::invalid_argument("silhouette: Too many samples");
        std::vector<unsigned int> l(labels, labels + n);
        for (const unsigned int v : l)
            if (v >= K) throw std::invalid_argument("silhouette: a label is not below K");
        std::vector<Index> r;
        if (rows) {
            if (!n_rows) return;
            r.reserve(n_rows);
            for (uint64_t i = 0; i < n_rows; ++i) {
                if (rows[i] >= n) throw std::invalid_argument("silhouette: a row index is out of range");
                r.push_back(static_cast<Index>(rows[i]));
            }
        }
        const VectorXd s = Clustering::silhouette_samples(ConstMatrixRef(x, d, static_cast<Index>(n), d), l, r);
        std::copy_n(s.data(), s.size(), s_out);
    });
}
int mlpp_em_sample(const mlpp_em* h, uint64_t n, uint64_t seed, double* x_out, uint32_t* labels_out)
{
    return guarded([&] {
        need(h);
        if (n) need(x_out);
        if (n > static_cast<uint64_t>(std::numeric_limits<Index>::max())) throw std::invalid_argument("EM: Too many samples");
        std::vector<unsigned int> labels;
        const MatrixXd x = h->em.sample(static_cast<Index>(n), seed, labels_out ? &labels : nullptr);
        std::copy_n(x.data(), x.size(), x_out);
        if (labels_out) std::copy(labels.begin(), labels.end(), labels_out);
    });
}
int mlpp_em_conditional_means(const mlpp_em* h, const uint32_t* observed, uint32_t n_observed, const double* data_observed, uint64_t n,
                              double* out, double* log_density_out)
{
    return guarded([&] {
        need(h);
        if (n_observed) need(observed);
        if (n && n_observed) { need(data_observed); need(out); }
        if (n > static_cast<uint64_t>(std::numeric_limits<Index>::max())) throw std::invalid_argument("EM: Too many samples");
        const std::vector<unsigned int> coordinates(observed, observed + n_observed);
        const MatrixXd y = h->em.conditional_means(coordinates, ConstMatrixRef(data_observed, n_observed, static_cast<Index>(n), n_observed),
                                                   log_density_out);
        std::copy_n(y.data(), y.size(), out);
    });
}
int mlpp_em_impute(const mlpp_em* h, const double* data, uint64_t n, uint32_t d, double* out, double* log_density_out, double* responsibilities_out)
{
    return guarded([&] {
        need(h);
        if (n && d) { need(data); need(out); }
        if (n > static_cast<uint64_t>(std::numeric_limits<Index>::max())) throw std::invalid_argument("EM: Too many samples");
        MatrixXd shares;
        const MatrixXd y = h->em.impute(ConstMatrixRef(data, d, static_cast<Index>(n), d), log_density_out, responsibilities_out ? &shares : nullptr);
        std::copy_n(y.data(), y.size(), out);
        if (responsibilities_out) std::copy_n(shares.data(), shares.size(), responsibilities_out);
    });
}
int mlpp_em_conditional_covariances(const mlpp_em* h, const uint32_t* observed, uint32_t n_observed, double* out)
{
    return guarded([&] {
        need(h);
        if (n_observed) need(observed);
        need(out);
        const std::vector<unsigned int> coordinates(observed, observed + n_observed);
        for (const MatrixXd& c : h->em.conditional_covariances(coordinates)) out = std::copy_n(c.data(), c.size(), out);
    });
}
int mlpp_em_conditional_samples(const mlpp_em* h, const uint32_t* observed, uint32_t n_observed, const double* data_observed, uint64_t n,
                                uint64_t n_draws, uint64_t seed, double* out, uint32_t* labels_out)
{
    return guarded([&] {
        need(h);
        if (n_observed) need(observed);
        if (n && n_observed) need(data_observed);
        if (n && n_observed && n_draws) need(out);
        if (n > static_cast<uint64_t>(std::numeric_limits<Index>::max())) throw std::invalid_argument("EM: Too many samples");
        if (n_draws > 0xFFFFFFFFull) throw std::invalid_argument("EM: n_draws must be 0 .. 2^32 - 1");
        const std::vector<unsigned int> coordinates(observed, observed + n_observed);
        std::vector<unsigned int> labels;
        const MatrixXd x = h->em.conditional_samples(coordinates, ConstMatrixRef(data_observed, n_observed, static_cast<Index>(n), n_observed),
                                                     static_cast<Index>(n_draws), seed, labels_out ? &labels : nullptr);
        std::copy_n(x.data(), x.size(), out);
        if (labels_out) std::copy(labels.begin(), labels.end(), labels_out);
    });
}
int mlpp_em_conditional_variances(const mlpp_em* h, const uint32_t* observed, uint32_t n_observed, const double* data_observed, uint64_t n,
                                  int full, double* out, double* means_out)
{
    return guarded([&] {
        need(h);
        if (n_observed) need(observed);
        if (n && n_observed) { need(data_observed); need(out); }
        if (n > static_cast<uint64_t>(std::numeric_limits<Index>::max())) throw std::invalid_argument("EM: Too many samples");
        const std::vector<unsigned int> coordinates(observed, observed + n_observed);
        MatrixXd means;
        const MatrixXd v = h->em.conditional_variances(coordinates, ConstMatrixRef(data_observed, n_observed, static_cast<Index>(n), n_observed),
                                                       full != 0, means_out ? &means : nullptr);
        std::copy_n(v.data(), v.size(), out);
        if (means_out) std::copy_n(means.data(), means.size(), means_out);
    });
}
int mlpp_em_conditional_cdfs(const mlpp_em* h, const uint32_t* observed, uint32_t n_observed, const double* data_observed, uint64_t n,
                             const double* values, double* out)
{
    return guarded([&] {
        need(h);
        if (n_observed) need(observed);
        if (n && n_observed) { need(data_observed); need(values); need(out); }
        if (n > static_cast<uint64_t>(std::numeric_limits<Index>::max())) throw std::invalid_argument("EM: Too many samples");
        const std::vector<unsigned int> coordinates(observed, observed + n_observed);
        const Index d = h->em.means().rows(), missing = d > static_cast<Index>(n_observed) ? d - static_cast<Index>(n_observed) : 0;
        const MatrixXd v = h->em.conditional_cdfs(coordinates, ConstMatrixRef(data_observed, n_observed, static_cast<Index>(n), n_observed),
                                                  ConstMatrixRef(values, missing, static_cast<Index>(n), missing));
        std::copy_n(v.data(), v.size(), out);
    });
}
int mlpp_em_conditional_quantiles(const mlpp_em* h, const uint32_t* observed, uint32_t n_observed, const double* data_observed, uint64_t n,
                                  const double* probabilities, uint64_t n_probabilities, double* out)
{
    return guarded([&] {
        need(h);
        if (n_observed) need(observed);
        if (n_probabilities) need(probabilities);
        if (n && n_observed) need(data_observed);
        if (n && n_observed && n_probabilities) need(out);
        if (n > static_cast<uint64_t>(std::numeric_limits<Index>::max())) throw std::invalid_argument("EM: Too many samples");
        if (n_probabilities > 0xFFFFFFFFull) throw std::invalid_argument("EM: too many probabilities");
        const std::vector<unsigned int> coordinates(observed, observed + n_observed);
        const std::vector<double> p(probabilities, probabilities + n_probabilities);
        const MatrixXd v = h->em.conditional_quantiles(coordinates, ConstMatrixRef(data_observed, n_observed, static_cast<Index>(n), n_observed), p);
        std::copy_n(v.data(), v.size(), out);
    });
}
int mlpp_em_predict_proba(const mlpp_em* h, const double* data, uint64_t n, uint32_t d, double* out)
{
    return guarded([&] {
        need(h); need(data); need(out);
        const MatrixXd r = h->em.calculate_responsibilities(ConstMatrixRef(data, d, static_cast<Index>(n), d));
        std::copy_n(r.data(), r.size(), out);
    });
}

// ---- KMeans ----
int mlpp_kmeans_create(uint32_t K, mlpp_kmeans** out) { return guarded([&] { need(out); *out = new mlpp_kmeans(K); }); }
int mlpp_kmeans_destroy(mlpp_kmeans* h) { delete h; return MLHIP_OK; }
int mlpp_kmeans_set_seed(mlpp_kmeans* h, uint32_t v) { return guarded([&] { need(h); h->km.set_seed(v); }); }
int mlpp_kmeans_set_absolute_tolerance(mlpp_kmeans* h, double v) { return guarded([&] { need(h); h->km.set_absolute_tolerance(v); }); }
int mlpp_kmeans_set_maximum_steps(mlpp_kmeans* h, uint32_t v) { return guarded([&] { need(h); h->km.set_maximum_steps(v); }); }
int mlpp_kmeans_set_number_initialisations(mlpp_kmeans* h, uint32_t v) { return guarded([&] { need(h); h->km.set_number_initialisations(v); }); }
int mlpp_kmeans_set_centroids_initialiser(mlpp_kmeans* h, const mlpp_centroids_initialiser* i) { return guarded([&] { need(h); h->km.set_centroids_initialiser(i ? i->p : nullptr); }); }
int mlpp_kmeans_set_verbose(mlpp_kmeans* h, int v) { return guarded([&] { need(h); h->km.set_verbose(v != 0); }); }
int mlpp_kmeans_fit(mlpp_kmeans* h, const double* data, uint64_t n, uint32_t d, int* converged)
{
    return guarded([&] {
        need(h); need(converged);
        if (n && d) need(data);
        const bool ok = h->km.fit(ConstMatrixRef(data, d, static_cast<Index>(n)));
        h->d = d; h->n = static_cast<Index>(n);
        *converged = ok ? 1 : 0;
    });
}
int mlpp_kmeans_fit_weighted(mlpp_kmeans* h, const double* data, const double* weights, uint64_t n, uint32_t d, int* converged)
{
    return guarded([&] {
        need(h); need(converged);
        if (n && d) need(data);
        if (n) need(weights);
        const bool ok = h->km.fit(ConstMatrixRef(data, d, static_cast<Index>(n)), ConstVectorRef(weights, static_cast<Index>(n)));
        h->d = d; h->n = static_cast<Index>(n);
        *converged = ok ? 1 : 0;
    });
}
int mlpp_kmeans_number_clusters(const mlpp_kmeans* h, uint32_t* out) { return guarded([&] { need(h); need(out); *out = h->km.number_clusters(); }); }
int mlpp_kmeans_dims(const mlpp_kmeans* h, uint32_t* d, uint64_t* n) { return guarded([&] { need(h); if (d) *d = static_cast<uint32_t>(h->km.centroids().rows()); if (n) *n = static_cast<uint64_t>(h->km.labels().size()); }); }
int mlpp_kmeans_centroids(const mlpp_kmeans* h, double* out) { return guarded([&] { need(h); need(out); std::copy_n(h->km.centroids().data(), h->km.centroids().size(), out); }); }
int mlpp_kmeans_labels(const mlpp_kmeans* h, uint32_t* out) { return guarded([&] { need(h); need(out); std::copy(h->km.labels().begin(), h->km.labels().end(), out); }); }
int mlpp_kmeans_inertia(const mlpp_kmeans* h, double* out) { return guarded([&] { need(h); need(out); *out = h->km.inertia(); }); }
int mlpp_kmeans_converged(const mlpp_kmeans* h, int* out) { return guarded([&] { need(h); need(out); *out = h->km.converged() ? 1 : 0; }); }
int mlpp_kmeans_steps_done(const mlpp_kmeans* h, uint32_t* out) { return guarded([&] { need(h); need(out); *out = h->km.steps_done(); }); }
int mlpp_kmeans_assign_label(const mlpp_kmeans* h, const double* x, uint32_t xlen, uint32_t* label, double* dist2)
{
    return guarded([&] {
        need(h); need(x); need(label); need(dist2);
        if (static_cast<Index>(xlen) != h->km.centroids().rows()) throw std::invalid_argument("Wrong x size");
        const auto r = h->km.assign_label(ConstVectorRef(x, xlen));
        *label = r.first;
        *dist2 = r.second;
    });
}

int mlpp_kmeans_predict(const mlpp_kmeans* h, const double* data, uint64_t n, uint32_t d, uint32_t* labels, double* dist2)
{
    return guarded([&] {
        need(h); need(data); need(labels);
        VectorXd dist;
        const std::vector<unsigned int> v = h->km.assign_labels(ConstMatrixRef(data, d, static_cast<Index>(n), d), dist2 ? &dist : nullptr);
        std::copy(v.begin(), v.end(), labels);
        if (dist2) std::copy_n(dist.data(), dist.size(), dist2);
    });
}

// ---- LinearAlgebra ----
int mlpp_xAx_symmetric(const double* A, uint32_t rows, uint32_t cols, const double* x, uint32_t xlen, double* out)
{
    return guarded([&] {
        need(A); need(x); need(out);
        MatrixXd m(rows, cols);
        std::copy_n(A, static_cast<std::size_t>(rows) * cols, m.data());
        *out = LinearAlgebra::xAx_symmetric(m, ConstVectorRef(x, xlen));
    });
}
int mlpp_xxT(const double* x, uint32_t n, double* dest)
{
    return guarded([&] {
        need(x); need(dest);
        VectorXd v(n);
        std::copy_n(x, n, v.data());
        MatrixXd m;
        LinearAlgebra::xxT(v, m);
        std::copy_n(m.data(), m.size(), dest);
    });
}
int mlpp_add_a_xxT(const double* x, uint32_t n, double* dest, uint32_t drows, uint32_t dcols, double a)
{
    return guarded([&] {
        need(x); need(dest);
        VectorXd v(n);
        std::copy_n(x, n, v.data());
        MatrixXd m(drows, dcols);
        std::copy_n(dest, static_cast<std::size_t>(drows) * dcols, m.data());
        LinearAlgebra::add_a_xxT(v, m, a);
        std::copy_n(m.data(), m.size(), dest);
    });
}

int mlpp_calculate_XXt_beta(const double* X, uint64_t n, uint32_t q, const double* y, uint64_t ylen, const double* lambda,
                            uint32_t lambda_len, double* XXt, double* beta)
{
    return guarded([&] {
        need(X); need(y); need(lambda); need(XXt); need(beta);
        LDLT decomposition;
        const VectorXd b = LinearRegression::calculate_XXt_beta(ConstMatrixRef(X, q, static_cast<Index>(n)),
                                                                ConstVectorRef(y, static_cast<Index>(ylen)),
                                                                MatrixRef(XXt, q, q, q), decomposition,
                                                                ConstVectorRef(lambda, lambda_len));
        std::copy_n(b.data(), b.size(), beta);
    });
}

int mlpp_device_context(mlhip_ctx** out)
{
    return guarded([&] { need(out); *out = device::context(); });
}

int mlpp_device_set_context(mlhip_ctx* ctx)
{
    return guarded([&] { device::set_context(ctx); });
}

}  // extern "C"
