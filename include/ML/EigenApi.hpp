#pragma once
/* The reference's class API with the reference's OWN types: header-only ml::EM, ml::Clustering::KMeans and the library
 * initialisers whose accessors ARE Eigen objects -- `const Eigen::MatrixXd& means()`, `const std::vector<Eigen::MatrixXd>&
 * covariances()`, `const Eigen::VectorXd& mixing_probabilities()`, `const Eigen::MatrixXd& responsibilities()`,
 * `const Eigen::MatrixXd& centroids()` (reference ML/EM.hpp:100-135, ML/KMeans.hpp:34-60) -- so that code which chains Eigen on
 * them, like the reference's own tests (`(means - em.means()).norm()`, `em.responsibilities().row(i).transpose()`,
 * Tests/test_EM.cpp:56-101, Tests/test_KMeans.cpp:57-90), compiles as written. The classes are thin owners of the flat C handles
 * of include/mlpp_c.h (the same handles the Python surface uses): every call goes to libmlhip.so, results are copied into Eigen
 * members after fit() -- responsibilities lazily, on first access, like the C++ facade of include/ML/EM.hpp.
 *
 * Use INSTEAD of include/ML/{EM,KMeans,Clustering}.hpp in a translation unit (the two families share their names; the classes
 * here live in the inline namespace ml::eigen_api so that their symbols never meet the library's): put include/eigen_api in
 * front of include/ on the include path and `#include "ML/EM.hpp"` resolves to this header.
 * Limits: user-defined initialisers cannot cross the C handles -- subclass the initialiser bases of include/ML/Clustering.hpp
 * (EigenCentroidsInitialiser) with the C++ facade for that; LinearAlgebra / LinearRegression helpers are in their own headers.
 * NOT VERIFIED AGAINST REAL EIGEN in this repository's build environment (Eigen is absent there): compiled and run against the
 * stand-in tests/cpp/eigen_shim only (tests/cpp/eigen_api_test.cpp); see INTEGRATION.md. */
#if defined(MLHIP_ML_EM_HPP) || defined(MLHIP_ML_KMEANS_HPP) || defined(MLHIP_ML_CLUSTERING_HPP)
#error "ML/EigenApi.hpp replaces ML/EM.hpp / ML/KMeans.hpp / ML/Clustering.hpp in a translation unit: include one family only"
#endif
#define MLHIP_ML_EIGEN_API_HPP

#include <Eigen/Core>

#include <algorithm>
#include <cstdint>
#include <memory>
#include <random>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../mlhip.h"
#include "../mlpp_c.h"

namespace ml {
inline namespace eigen_api {

namespace detail {
/// A failed C call as the exception the reference throws there (ML/EM.cpp:35-100, ML/KMeans.cpp:21-148).
inline void check(int status)
{
    if (status == MLHIP_OK) return;
    const std::string msg = mlhip_last_error();
    if (status == MLHIP_E_INVALID_ARGUMENT) throw std::invalid_argument(msg);
    if (status == MLHIP_E_DOMAIN) throw std::domain_error(msg);
    throw std::runtime_error(msg);
}
/// The d x N block as the contiguous memory the C handles take (a copy only when the columns are strided).
struct Block {
    Eigen::MatrixXd copy;
    const double* p;
    explicit Block(Eigen::Ref<const Eigen::MatrixXd> data) : p(data.data())
    {
        if (data.outerStride() != data.rows()) { copy = data; p = copy.data(); }
    }
};
}  // namespace detail

namespace Clustering {

/** Initialisers (ML/Clustering.hpp:58-125): owners of the library's implementations. */
class CentroidsInitialiser {
public:
    virtual ~CentroidsInitialiser() { if (h_) mlpp_centroids_initialiser_destroy(h_); }
    CentroidsInitialiser(const CentroidsInitialiser&) = delete;
    CentroidsInitialiser& operator=(const CentroidsInitialiser&) = delete;
    const mlpp_centroids_initialiser* handle() const { return h_; }
protected:
    CentroidsInitialiser() = default;
    mlpp_centroids_initialiser* h_ = nullptr;
};
class Forgy : public CentroidsInitialiser { public: Forgy() { detail::check(mlpp_forgy_create(&h_)); } };
class RandomPartition : public CentroidsInitialiser { public: RandomPartition() { detail::check(mlpp_random_partition_create(&h_)); } };
class KPP : public CentroidsInitialiser { public: KPP() { detail::check(mlpp_kpp_create(&h_)); } };
class FixedPointKPP : public CentroidsInitialiser { public: FixedPointKPP() { detail::check(mlpp_fixed_point_kpp_create(&h_)); } };

class ResponsibilitiesInitialiser {
public:
    virtual ~ResponsibilitiesInitialiser() { if (h_) mlpp_responsibilities_initialiser_destroy(h_); }
    ResponsibilitiesInitialiser(const ResponsibilitiesInitialiser&) = delete;
    ResponsibilitiesInitialiser& operator=(const ResponsibilitiesInitialiser&) = delete;
    const mlpp_responsibilities_initialiser* handle() const { return h_; }
protected:
    ResponsibilitiesInitialiser() = default;
    mlpp_responsibilities_initialiser* h_ = nullptr;
};
class ClosestCentroid : public ResponsibilitiesInitialiser {
public:
    /** @throw std::invalid_argument If `centroids_initialiser` is null (ML/Clustering.cpp:68). */
    explicit ClosestCentroid(std::shared_ptr<const CentroidsInitialiser> centroids_initialiser) : centroids_initialiser_(centroids_initialiser)
    {
        detail::check(mlpp_closest_centroid_create(centroids_initialiser ? centroids_initialiser->handle() : nullptr, &h_));
    }
private:
    std::shared_ptr<const CentroidsInitialiser> centroids_initialiser_;
};

/** Abstract clustering model (ML/Clustering.hpp:17-55). */
class Model {
public:
    virtual ~Model() {}
    virtual bool fit(Eigen::Ref<const Eigen::MatrixXd> data) = 0;
    virtual unsigned int number_clusters() const = 0;
    virtual const std::vector<unsigned int>& labels() const = 0;
    virtual const Eigen::MatrixXd& centroids() const = 0;
    virtual bool converged() const = 0;
};

/** K-means (ML/KMeans.hpp:16-111). */
class KMeans : public Model {
public:
    explicit KMeans(unsigned int number_clusters) : number_clusters_(number_clusters) { detail::check(mlpp_kmeans_create(number_clusters, &h_)); }
    ~KMeans() override { if (h_) mlpp_kmeans_destroy(h_); }
    KMeans(const KMeans&) = delete;
    KMeans& operator=(const KMeans&) = delete;

    bool fit(Eigen::Ref<const Eigen::MatrixXd> data) override { return fit_block(data, nullptr); }
    /** Extension: the fit of a weighted sample (ml::Clustering::KMeans::fit(data, weights) of ML/KMeans.hpp): weights(i) >= 0 is the
    frequency weight of column i. @throw std::invalid_argument If `weights.size() != data.cols()` or the weights are refused. */
    bool fit(Eigen::Ref<const Eigen::MatrixXd> data, Eigen::Ref<const Eigen::VectorXd> weights)
    {
        if (weights.size() != data.cols()) throw std::invalid_argument("KMeans: One weight per data point required");
        return fit_block(data, weights.data());                      // (a Ref<const VectorXd> is contiguous)
    }

private:
    bool fit_block(Eigen::Ref<const Eigen::MatrixXd> data, const double* weights)
    {
        const detail::Block block(data);
        int converged = 0;
        const uint64_t n = static_cast<uint64_t>(data.cols());
        const uint32_t dims = static_cast<uint32_t>(data.rows());
        detail::check(weights ? mlpp_kmeans_fit_weighted(h_, block.p, weights, n, dims, &converged)
                              : mlpp_kmeans_fit(h_, block.p, n, dims, &converged));
        centroids_.resize(data.rows(), number_clusters_);
        detail::check(mlpp_kmeans_centroids(h_, centroids_.data()));
        labels_.resize(static_cast<std::size_t>(data.cols()));
        static_assert(sizeof(unsigned int) == sizeof(uint32_t), "labels are 32-bit");
        detail::check(mlpp_kmeans_labels(h_, reinterpret_cast<uint32_t*>(labels_.data())));
        detail::check(mlpp_kmeans_inertia(h_, &inertia_));
        converged_ = converged != 0;
        return converged_;
    }

public:
    unsigned int number_clusters() const override { return number_clusters_; }
    const std::vector<unsigned int>& labels() const override { return labels_; }
    const Eigen::MatrixXd& centroids() const override { return centroids_; }
    void set_seed(unsigned int seed) { detail::check(mlpp_kmeans_set_seed(h_, seed)); }
    void set_absolute_tolerance(double absolute_tolerance) { detail::check(mlpp_kmeans_set_absolute_tolerance(h_, absolute_tolerance)); }
    void set_maximum_steps(unsigned int maximum_steps) { detail::check(mlpp_kmeans_set_maximum_steps(h_, maximum_steps)); }
    void set_number_initialisations(unsigned int number_initialisations) { detail::check(mlpp_kmeans_set_number_initialisations(h_, number_initialisations)); }
    void set_centroids_initialiser(std::shared_ptr<const CentroidsInitialiser> centroids_initialiser)
    {
        detail::check(mlpp_kmeans_set_centroids_initialiser(h_, centroids_initialiser ? centroids_initialiser->handle() : nullptr));
        centroids_initialiser_ = centroids_initialiser;
    }
    void set_verbose(bool verbose) { detail::check(mlpp_kmeans_set_verbose(h_, verbose ? 1 : 0)); }
    /** (label, squared distance) of the nearest centroid (ML/KMeans.cpp:153-165). */
    std::pair<unsigned int, double> assign_label(Eigen::Ref<const Eigen::VectorXd> x) const
    {
        uint32_t label = 0;
        double dist2 = 0;
        const Eigen::VectorXd contiguous(x);
        detail::check(mlpp_kmeans_assign_label(h_, contiguous.data(), static_cast<uint32_t>(contiguous.size()), &label, &dist2));
        return std::make_pair(static_cast<unsigned int>(label), dist2);
    }
    /** Extension (not in the reference surface): assign_label for every column of `data`, on the device; with
    `squared_distances` also the squared distance of every point to its centroid. */
    std::vector<unsigned int> assign_labels(Eigen::Ref<const Eigen::MatrixXd> data, Eigen::VectorXd* squared_distances = nullptr) const
    {
        const detail::Block block(data);
        std::vector<unsigned int> labels(static_cast<std::size_t>(data.cols()));
        if (squared_distances) squared_distances->resize(data.cols());
        static_assert(sizeof(unsigned int) == sizeof(uint32_t), "labels are 32-bit");
        detail::check(mlpp_kmeans_predict(h_, block.p, static_cast<uint64_t>(data.cols()), static_cast<uint32_t>(data.rows()),
                                          reinterpret_cast<uint32_t*>(labels.data()), squared_distances ? squared_distances->data() : nullptr));
        return labels;
    }
    double inertia() const { return inertia_; }
    bool converged() const override { return converged_; }

private:
    mlpp_kmeans* h_ = nullptr;
    std::shared_ptr<const CentroidsInitialiser> centroids_initialiser_;
    Eigen::MatrixXd centroids_;
    std::vector<unsigned int> labels_;
    double inertia_ = 0;
    unsigned int number_clusters_;
    bool converged_ = false;
};

/** Extension: the exact silhouette value (Euclidean) of points of `data` (a point in every column) under `labels`, on the device;
`rows`: the points to evaluate, in any order (empty: all). The definition, its fixed arithmetic and the exceptions: the function of
the same name in ML/Clustering.hpp. silhouette_score: their mean, summed in row order. */
inline Eigen::VectorXd silhouette_samples(Eigen::Ref<const Eigen::MatrixXd> data, const std::vector<unsigned int>& labels,
                                          const std::vector<Eigen::Index>& rows = {})
{
    if (labels.size() != static_cast<std::size_t>(data.cols())) throw std::invalid_argument("silhouette: one label per data point required");
    unsigned int top = 0;
    for (const unsigned int l : labels) top = l > top ? l : top;
    if (top == static_cast<unsigned int>(-1)) throw std::invalid_argument("silhouette: a label is too large");
    std::vector<uint64_t> index;
    for (const Eigen::Index r : rows) {
        if (r < 0 || r >= data.cols()) throw std::invalid_argument("silhouette: a row index is out of range");
        index.push_back(static_cast<uint64_t>(r));
    }
    const detail::Block block(data);
    Eigen::VectorXd out(rows.empty() ? data.cols() : static_cast<Eigen::Index>(rows.size()));
    detail::check(mlpp_silhouette_samples(block.p, static_cast<uint64_t>(data.cols()), static_cast<uint32_t>(data.rows()), labels.data(),
                                          top + 1, rows.empty() ? nullptr : index.data(), index.size(), out.data()));
    return out;
}
inline double silhouette_score(Eigen::Ref<const Eigen::MatrixXd> data, const std::vector<unsigned int>& labels,
                               const std::vector<Eigen::Index>& rows = {})
{
    const Eigen::VectorXd v = silhouette_samples(data, labels, rows);
    double sum = 0;
    for (Eigen::Index i = 0; i < v.size(); ++i) sum += v[i];
    return sum / static_cast<double>(v.size());
}

}  // namespace Clustering

/** Gaussian-mixture EM (ML/EM.hpp:18-198). */
class EM : public Clustering::Model {
public:
    explicit EM(unsigned int number_components) : number_components_(number_components), covariances_(number_components)
    {
        detail::check(mlpp_em_create(number_components, &h_));
    }
    ~EM() override { if (h_) mlpp_em_destroy(h_); }
    EM(const EM&) = delete;
    EM& operator=(const EM&) = delete;

    void set_seed(unsigned int seed) { detail::check(mlpp_em_set_seed(h_, seed)); }
    void set_absolute_tolerance(double absolute_tolerance) { detail::check(mlpp_em_set_absolute_tolerance(h_, absolute_tolerance)); }
    void set_relative_tolerance(double relative_tolerance) { detail::check(mlpp_em_set_relative_tolerance(h_, relative_tolerance)); }
    void set_maximum_steps(unsigned int maximum_steps) { detail::check(mlpp_em_set_maximum_steps(h_, maximum_steps)); }
    void set_means_initialiser(std::shared_ptr<const Clustering::CentroidsInitialiser> means_initialiser)
    {
        detail::check(mlpp_em_set_means_initialiser(h_, means_initialiser ? means_initialiser->handle() : nullptr));
        means_initialiser_ = means_initialiser;
    }
    void set_responsibilities_initialiser(std::shared_ptr<const Clustering::ResponsibilitiesInitialiser> responsibilities_initialiser)
    {
        detail::check(mlpp_em_set_responsibilities_initialiser(h_, responsibilities_initialiser ? responsibilities_initialiser->handle() : nullptr));
        responsibilities_initialiser_ = responsibilities_initialiser;
    }
    void set_verbose(bool verbose) { detail::check(mlpp_em_set_verbose(h_, verbose ? 1 : 0)); }
    void set_maximise_first(bool maximise_first) { detail::check(mlpp_em_set_maximise_first(h_, maximise_first ? 1 : 0)); }
    /** Extension (ML/EM.hpp): full covariances (default, the reference), diagonal ones, or ONE covariance tied across the components. */
    enum class CovarianceType { Full = 0, Diagonal = 1, Tied = 2 };
    void set_covariance_type(CovarianceType covariance_type) { detail::check(mlpp_em_set_covariance_type(h_, static_cast<int>(covariance_type))); }

    /** Extension (ML/EM.hpp): what every M-step adds to the diagonal of each covariance it forms; default 1e-15, the reference's constant.
    @throw std::domain_error If the value is negative or not finite. */
    void set_covariance_regularisation(double covariance_regularisation)
    {
        detail::check(mlpp_em_set_covariance_regularisation(h_, covariance_regularisation));
    }
    double covariance_regularisation() const
    {
        double v = 0;
        detail::check(mlpp_em_covariance_regularisation(h_, &v));
        return v;
    }

private:
    template <class T> std::vector<T> per_initialisation(int (*get)(const mlpp_em*, T*, uint32_t, uint32_t*)) const
    {
        uint32_t count = 0;
        detail::check(get(h_, nullptr, 0, &count));
        std::vector<T> v(count);
        if (count) detail::check(get(h_, v.data(), count, &count));
        return v;
    }

public:
    /** Extension (ML/EM.hpp): fit() runs this many EM loops from consecutive starts on the one uploaded sample and keeps the best
    (default 1, the reference). @throw std::invalid_argument If `number_initialisations == 0`. */
    void set_number_initialisations(unsigned int number_initialisations)
    {
        detail::check(mlpp_em_set_number_initialisations(h_, number_initialisations));
    }
    unsigned int number_initialisations() const
    {
        uint32_t v = 0;
        detail::check(mlpp_em_number_initialisations(h_, &v));
        return v;
    }
    /** Extension: the initialisation the fitted state belongs to, and every initialisation's final log-likelihood, iterations and
    convergence flag (0 / 1) from the last fit(). */
    unsigned int best_initialisation() const
    {
        uint32_t v = 0;
        detail::check(mlpp_em_best_initialisation(h_, &v));
        return v;
    }
    std::vector<double> initialisation_log_likelihoods() const { return per_initialisation<double>(mlpp_em_initialisation_log_likelihoods); }
    std::vector<unsigned int> initialisation_steps() const
    {
        const std::vector<uint32_t> v = per_initialisation<uint32_t>(mlpp_em_initialisation_steps);
        return std::vector<unsigned int>(v.begin(), v.end());
    }
    std::vector<int> initialisation_converged() const { return per_initialisation<int>(mlpp_em_initialisation_converged); }

    bool fit(Eigen::Ref<const Eigen::MatrixXd> data) override { return fit_block(data, nullptr); }
    /** Extension: the fit of a weighted sample (ml::EM::fit(data, weights) of ML/EM.hpp): weights(i) >= 0 is the frequency weight of
    column i. @throw std::invalid_argument If `weights.size() != data.cols()` or the weights are refused. */
    bool fit(Eigen::Ref<const Eigen::MatrixXd> data, Eigen::Ref<const Eigen::VectorXd> weights)
    {
        if (weights.size() != data.cols()) throw std::invalid_argument("EM: One weight per data point required");
        return fit_block(data, weights.data());                      // (a Ref<const VectorXd> is contiguous)
    }

private:
    bool fit_block(Eigen::Ref<const Eigen::MatrixXd> data, const double* weights)
    {
        const detail::Block block(data);
        int converged = 0;
        const uint64_t n = static_cast<uint64_t>(data.cols());
        const uint32_t dims = static_cast<uint32_t>(data.rows());
        detail::check(weights ? mlpp_em_fit_weighted(h_, block.p, weights, n, dims, &converged) : mlpp_em_fit(h_, block.p, n, dims, &converged));
        const Eigen::Index d = data.rows();
        means_.resize(d, number_components_);
        detail::check(mlpp_em_means(h_, means_.data()));
        mixing_probabilities_.resize(number_components_);
        detail::check(mlpp_em_mixing_probabilities(h_, mixing_probabilities_.data()));
        for (unsigned int k = 0; k < number_components_; ++k) {
            covariances_[k].resize(d, d);
            detail::check(mlpp_em_covariance(h_, k, covariances_[k].data()));
        }
        labels_.resize(static_cast<std::size_t>(data.cols()));
        static_assert(sizeof(unsigned int) == sizeof(uint32_t), "labels are 32-bit");
        detail::check(mlpp_em_labels(h_, reinterpret_cast<uint32_t*>(labels_.data())));
        detail::check(mlpp_em_log_likelihood(h_, &log_likelihood_));
        converged_ = converged != 0;
        responsibilities_fetched_ = false;
        return converged_;
    }

public:
    unsigned int number_components() const { return number_components_; }
    unsigned int number_clusters() const override { return number_components_; }
    const Eigen::MatrixXd& means() const { return means_; }
    const Eigen::MatrixXd& centroids() const override { return means_; }
    const std::vector<Eigen::MatrixXd>& covariances() const { return covariances_; }
    /** @throw std::invalid_argument If `k >= number_components()` (ML/EM.cpp:84-89). */
    const Eigen::MatrixXd& covariance(unsigned int k) const
    {
        if (k >= number_components_) throw std::invalid_argument("EM: Bad component index");
        return covariances_[k];
    }
    const Eigen::VectorXd& mixing_probabilities() const { return mixing_probabilities_; }
    /** N x number_components(); copied from the device on the first call after a fit. */
    const Eigen::MatrixXd& responsibilities() const
    {
        if (!responsibilities_fetched_) {
            responsibilities_.resize(static_cast<Eigen::Index>(labels_.size()), number_components_);
            detail::check(mlpp_em_responsibilities(h_, responsibilities_.data()));
            responsibilities_fetched_ = true;
        }
        return responsibilities_;
    }
    double log_likelihood() const { return log_likelihood_; }
    std::shared_ptr<const Clustering::CentroidsInitialiser> means_initialiser() const { return means_initialiser_; }
    /** @throw std::invalid_argument If `x.size() != means().rows()` or `u.size() != number_components()` (ML/EM.cpp:178-183). */
    void assign_responsibilities(Eigen::Ref<const Eigen::VectorXd> x, Eigen::Ref<Eigen::VectorXd> u) const
    {
        const Eigen::VectorXd contiguous(x);
        Eigen::VectorXd out(u.size());
        detail::check(mlpp_em_assign_responsibilities(h_, contiguous.data(), static_cast<uint32_t>(contiguous.size()), out.data(),
                                                      static_cast<uint32_t>(out.size())));
        u = out;
    }
    /** Extensions (not in the reference surface): the batch queries of a fitted model on a block with a data point in every column
    (any number of them), computed on the device. log_densities: log sum_k pi_k N(x_i | mu_k, Sigma_k) per point; mean_log_density:
    their mean, summed in row order (NaN for an empty block); assign_labels: argmax_k of the log-responsibilities, first maximum
    wins; calculate_responsibilities: the data.cols() x number_components() posteriors.
    @throw std::invalid_argument If `data.rows() != means().rows()` or the model has not been fitted. */
    Eigen::VectorXd log_densities(Eigen::Ref<const Eigen::MatrixXd> data) const
    {
        const detail::Block block(data);
        Eigen::VectorXd out(data.cols());
        detail::check(mlpp_em_score_samples(h_, block.p, static_cast<uint64_t>(data.cols()), static_cast<uint32_t>(data.rows()), out.data()));
        return out;
    }
    double mean_log_density(Eigen::Ref<const Eigen::MatrixXd> data) const
    {
        const Eigen::VectorXd v = log_densities(data);
        double sum = 0;
        for (Eigen::Index i = 0; i < v.size(); ++i) sum += v[i];
        return sum / static_cast<double>(v.size());
    }
    /** Extensions (model selection): the free parameters of the fitted mixture in the mode it was fitted in, and scikit-learn's
    BIC / AIC of the fitted model on `data`: -2 N mean_log_density(data) + number_parameters() log N, and + 2 number_parameters(). */
    std::size_t number_parameters() const
    {
        uint64_t p = 0;
        detail::check(mlpp_em_number_parameters(h_, &p));
        return static_cast<std::size_t>(p);
    }
    double bic(Eigen::Ref<const Eigen::MatrixXd> data) const
    {
        const detail::Block block(data);
        double out = 0;
        detail::check(mlpp_em_bic(h_, block.p, static_cast<uint64_t>(data.cols()), static_cast<uint32_t>(data.rows()), &out));
        return out;
    }
    double aic(Eigen::Ref<const Eigen::MatrixXd> data) const
    {
        const detail::Block block(data);
        double out = 0;
        detail::check(mlpp_em_aic(h_, block.p, static_cast<uint64_t>(data.cols()), static_cast<uint32_t>(data.rows()), &out));
        return out;
    }
    std::vector<unsigned int> assign_labels(Eigen::Ref<const Eigen::MatrixXd> data) const
    {
        const detail::Block block(data);
        std::vector<unsigned int> out(static_cast<std::size_t>(data.cols()));
        detail::check(mlpp_em_predict(h_, block.p, static_cast<uint64_t>(data.cols()), static_cast<uint32_t>(data.rows()),
                                      reinterpret_cast<uint32_t*>(out.data())));
        return out;
    }
    Eigen::MatrixXd calculate_responsibilities(Eigen::Ref<const Eigen::MatrixXd> data) const
    {
        const detail::Block block(data);
        Eigen::MatrixXd out(data.cols(), static_cast<Eigen::Index>(number_components_));
        detail::check(mlpp_em_predict_proba(h_, block.p, static_cast<uint64_t>(data.cols()), static_cast<uint32_t>(data.rows()), out.data()));
        return out;
    }
    /** Extension (ML/EM.hpp): `n` points drawn from the fitted mixture on the device, a point in every column (means().rows() x n);
    `labels`, if given, receives the components drawn. Point i is a pure function of (seed, i) and the fitted parameters.
    @throw std::invalid_argument If `n < 0` or the model has not been fitted. */
    Eigen::MatrixXd sample(Eigen::Index n, std::uint64_t seed = 0, std::vector<unsigned int>* labels = nullptr) const
    {
        if (n < 0) throw std::invalid_argument("EM: Negative number of samples");
        Eigen::MatrixXd out(means_.rows(), n);
        if (labels) labels->resize(static_cast<std::size_t>(n));
        static_assert(sizeof(unsigned int) == sizeof(uint32_t), "labels are 32-bit");
        detail::check(mlpp_em_sample(h_, static_cast<uint64_t>(n), seed, out.data(),
                                     labels ? reinterpret_cast<uint32_t*>(labels->data()) : nullptr));
        return out;
    }
    /** Extension (ML/EM.hpp): E[x_M | x_O] under the fitted mixture for every column of `data_observed` (row c = coordinate
    observed[c]); returns (number of missing coordinates) x data_observed.cols(), the missing coordinates ascending. `log_densities`,
    if given, receives the log-density of every x_O under the marginal mixture.
    @throw std::invalid_argument If the model has not been fitted, for bad coordinates or `data_observed.rows() != observed.size()`.
    @throw std::domain_error If the observed block of a covariance is not positive definite. */
    Eigen::MatrixXd conditional_means(const std::vector<unsigned int>& observed, Eigen::Ref<const Eigen::MatrixXd> data_observed,
                                      double* log_densities = nullptr) const
    {
        if (data_observed.rows() != static_cast<Eigen::Index>(observed.size())) throw std::invalid_argument("Wrong data size");
        const Eigen::Index missing = means_.rows() > data_observed.rows() ? means_.rows() - data_observed.rows() : 0;
        const detail::Block block(data_observed);
        Eigen::MatrixXd out(missing, data_observed.cols());
        static_assert(sizeof(unsigned int) == sizeof(uint32_t), "coordinates are 32-bit");
        detail::check(mlpp_em_conditional_means(h_, reinterpret_cast<const uint32_t*>(observed.data()), static_cast<uint32_t>(observed.size()),
                                                block.p, static_cast<uint64_t>(data_observed.cols()), out.data(), log_densities));
        return out;
    }
    /** Extension (ML/EM.hpp): `data` (a point in every column) with every NaN replaced by its conditional expectation under the fitted
    mixture given the coordinates that point has. `log_densities`, if given, receives the log-density of every point's observed
    coordinates under the marginal mixture; `responsibilities`, if given, is resized to number_components() x data.cols().
    @throw std::invalid_argument If the model has not been fitted or `data.rows() != means().rows()`.
    @throw std::domain_error If the observed block of a covariance is not positive definite for some point's pattern. */
    Eigen::MatrixXd impute(Eigen::Ref<const Eigen::MatrixXd> data, double* log_densities = nullptr,
                           Eigen::MatrixXd* responsibilities = nullptr) const
    {
        if (data.rows() != means_.rows()) throw std::invalid_argument("Wrong data size");
        const detail::Block block(data);
        Eigen::MatrixXd out(data.rows(), data.cols());
        if (responsibilities) responsibilities->resize(means_.cols(), data.cols());
        detail::check(mlpp_em_impute(h_, block.p, static_cast<uint64_t>(data.cols()), static_cast<uint32_t>(data.rows()), out.data(), log_densities,
                                     responsibilities ? responsibilities->data() : nullptr));
        return out;
    }
    /** Extension (ML/EM.hpp): the covariances of the conditioned components, K matrices of (number of missing coordinates)^2. Host only.
    @throw std::invalid_argument If the model has not been fitted or for bad coordinates.
    @throw std::domain_error If a block is not positive definite. */
    std::vector<Eigen::MatrixXd> conditional_covariances(const std::vector<unsigned int>& observed) const
    {
        const Eigen::Index d = means_.rows(), dO = static_cast<Eigen::Index>(observed.size()), missing = d > dO ? d - dO : 0;
        const Eigen::Index K = means_.cols();
        std::vector<double> flat(static_cast<std::size_t>(K * missing * missing) + 1);
        static_assert(sizeof(unsigned int) == sizeof(uint32_t), "coordinates are 32-bit");
        detail::check(mlpp_em_conditional_covariances(h_, reinterpret_cast<const uint32_t*>(observed.data()), static_cast<uint32_t>(observed.size()),
                                                      flat.data()));
        std::vector<Eigen::MatrixXd> out;
        for (Eigen::Index k = 0; k < K; ++k) {
            Eigen::MatrixXd c(missing, missing);
            std::copy_n(flat.data() + k * missing * missing, missing * missing, c.data());
            out.push_back(c);
        }
        return out;
    }
    /** Extension (ML/EM.hpp): `n_draws` draws from p(x_M | x_O) under the fitted mixture for every column of `data_observed`; returns
    (number of missing coordinates) x (n_draws * data_observed.cols()), draw q of point i in column q * data_observed.cols() + i.
    `labels`, if given, receives the components drawn, in the same order.
    @throw std::invalid_argument As conditional_means, or if n_draws < 0 or n_draws > 2^32 - 1.
    @throw std::domain_error If a block is not positive definite. */
    Eigen::MatrixXd conditional_samples(const std::vector<unsigned int>& observed, Eigen::Ref<const Eigen::MatrixXd> data_observed,
                                        Eigen::Index n_draws, std::uint64_t seed = 0, std::vector<unsigned int>* labels = nullptr) const
    {
        if (data_observed.rows() != static_cast<Eigen::Index>(observed.size())) throw std::invalid_argument("Wrong data size");
        if (n_draws < 0) throw std::invalid_argument("EM: n_draws must be 0 .. 2^32 - 1");
        const Eigen::Index missing = means_.rows() > data_observed.rows() ? means_.rows() - data_observed.rows() : 0;
        const detail::Block block(data_observed);
        Eigen::MatrixXd out(missing, n_draws * data_observed.cols());
        if (labels) labels->assign(static_cast<std::size_t>(n_draws * data_observed.cols()), 0u);
        static_assert(sizeof(unsigned int) == sizeof(uint32_t), "coordinates are 32-bit");
        detail::check(mlpp_em_conditional_samples(h_, reinterpret_cast<const uint32_t*>(observed.data()), static_cast<uint32_t>(observed.size()),
                                                  block.p, static_cast<uint64_t>(data_observed.cols()), static_cast<uint64_t>(n_draws), seed,
                                                  out.data(), labels ? reinterpret_cast<uint32_t*>(labels->data()) : nullptr));
        return out;
    }
    /** Extension (ML/EM.hpp): the predictive covariance Var[x_M | x_O] of every column of `data_observed` under the fitted mixture;
    returns (number of missing coordinates) x data_observed.cols(), or with `full_covariance` its square x data_observed.cols(), column
    i holding the matrix of point i. `means`, if given, receives conditional_means' result.
    @throw std::invalid_argument As conditional_means.
    @throw std::domain_error If a block is not positive definite. */
    Eigen::MatrixXd conditional_variances(const std::vector<unsigned int>& observed, Eigen::Ref<const Eigen::MatrixXd> data_observed,
                                          bool full_covariance = false, Eigen::MatrixXd* means = nullptr) const
    {
        if (data_observed.rows() != static_cast<Eigen::Index>(observed.size())) throw std::invalid_argument("Wrong data size");
        const Eigen::Index missing = means_.rows() > data_observed.rows() ? means_.rows() - data_observed.rows() : 0;
        const detail::Block block(data_observed);
        Eigen::MatrixXd out(full_covariance ? missing * missing : missing, data_observed.cols());
        if (means) means->resize(missing, data_observed.cols());
        static_assert(sizeof(unsigned int) == sizeof(uint32_t), "coordinates are 32-bit");
        detail::check(mlpp_em_conditional_variances(h_, reinterpret_cast<const uint32_t*>(observed.data()), static_cast<uint32_t>(observed.size()),
                                                    block.p, static_cast<uint64_t>(data_observed.cols()), full_covariance ? 1 : 0, out.data(),
                                                    means ? means->data() : nullptr));
        return out;
    }
    /** Extension (ML/EM.hpp): the predictive CDF P(x_j <= v | x_O) per missing coordinate of every column of `data_observed` at that
    point's own `values` ((number of missing coordinates) x data_observed.cols()); returns a matrix of that shape.
    @throw std::invalid_argument As conditional_means, or if `values` has another shape.
    @throw std::domain_error If a block is not positive definite. */
    Eigen::MatrixXd conditional_cdfs(const std::vector<unsigned int>& observed, Eigen::Ref<const Eigen::MatrixXd> data_observed,
                                     Eigen::Ref<const Eigen::MatrixXd> values) const
    {
        if (data_observed.rows() != static_cast<Eigen::Index>(observed.size())) throw std::invalid_argument("Wrong data size");
        const Eigen::Index missing = means_.rows() > data_observed.rows() ? means_.rows() - data_observed.rows() : 0;
        if (values.rows() != missing || values.cols() != data_observed.cols())
            throw std::invalid_argument("EM: values must hold one row per missing coordinate and one column per point");
        const detail::Block block(data_observed), at(values);
        Eigen::MatrixXd out(missing, data_observed.cols());
        static_assert(sizeof(unsigned int) == sizeof(uint32_t), "coordinates are 32-bit");
        detail::check(mlpp_em_conditional_cdfs(h_, reinterpret_cast<const uint32_t*>(observed.data()), static_cast<uint32_t>(observed.size()), block.p,
                                               static_cast<uint64_t>(data_observed.cols()), at.p, out.data()));
        return out;
    }
    /** Extension (ML/EM.hpp): the quantiles of the same one-dimensional mixtures at every probability (each strictly inside (0, 1));
    returns (number of missing coordinates) x (probabilities.size() * data_observed.cols()), probability q of point i in column
    q * data_observed.cols() + i.
    @throw std::invalid_argument As conditional_means, or for a probability that is a NaN or not strictly inside (0, 1).
    @throw std::domain_error If a block is not positive definite. */
    Eigen::MatrixXd conditional_quantiles(const std::vector<unsigned int>& observed, Eigen::Ref<const Eigen::MatrixXd> data_observed,
                                          const std::vector<double>& probabilities) const
    {
        if (data_observed.rows() != static_cast<Eigen::Index>(observed.size())) throw std::invalid_argument("Wrong data size");
        const Eigen::Index missing = means_.rows() > data_observed.rows() ? means_.rows() - data_observed.rows() : 0;
        const detail::Block block(data_observed);
        Eigen::MatrixXd out(missing, static_cast<Eigen::Index>(probabilities.size()) * data_observed.cols());
        static_assert(sizeof(unsigned int) == sizeof(uint32_t), "coordinates are 32-bit");
        detail::check(mlpp_em_conditional_quantiles(h_, reinterpret_cast<const uint32_t*>(observed.data()), static_cast<uint32_t>(observed.size()),
                                                    block.p, static_cast<uint64_t>(data_observed.cols()), probabilities.data(),
                                                    static_cast<uint64_t>(probabilities.size()), out.data()));
        return out;
    }
    const std::vector<unsigned int>& labels() const override { return labels_; }
    bool converged() const override { return converged_; }

private:
    mlpp_em* h_ = nullptr;
    std::shared_ptr<const Clustering::CentroidsInitialiser> means_initialiser_;
    std::shared_ptr<const Clustering::ResponsibilitiesInitialiser> responsibilities_initialiser_;
    unsigned int number_components_;
    Eigen::MatrixXd means_;
    std::vector<Eigen::MatrixXd> covariances_;
    Eigen::VectorXd mixing_probabilities_;
    mutable Eigen::MatrixXd responsibilities_;
    mutable bool responsibilities_fetched_ = false;
    std::vector<unsigned int> labels_;
    double log_likelihood_ = 0;
    bool converged_ = false;
};

}  // namespace eigen_api
}  // namespace ml
