#pragma once
#ifdef MLHIP_ML_EIGEN_API_HPP
#error "ML/KMeans.hpp and ML/EigenApi.hpp share their class names: include one family per translation unit"
#endif
#define MLHIP_ML_KMEANS_HPP
/* ml::Clustering::KMeans -- Lloyd K-means with the public interface of the reference's ML/KMeans.hpp:18-125,
 * executed on an MI355X: assignment_step/update_step (ML/KMeans.cpp:153-192) run as one HIP kernel per step through
 * the C ABI in mlhip.h; this class keeps fit/fit_once (ML/KMeans.cpp:25-114) and the host-side point query. */
#include <memory>
#include <random>
#include <utility>
#include <vector>

#include "Clustering.hpp"
#include "Dense.hpp"
#include "dll.hpp"

struct mlhip_data;

namespace ml {
namespace Clustering {

class KMeans : public Model {
public:
    /** @throw std::invalid_argument If `number_clusters == 0`. */
    DLL_DECLSPEC KMeans(unsigned int number_clusters);
    DLL_DECLSPEC ~KMeans() override;
    KMeans(const KMeans&) = delete;
    KMeans& operator=(const KMeans&) = delete;

    DLL_DECLSPEC bool fit(ConstMatrixRef data) override;
    /** Extension (not in the reference surface): the same fit of a WEIGHTED sample -- `weights[i]` >= 0 is the frequency weight of
    column i of `data` (integer weights: the fit of the sample with point i repeated weights[i] times, without the copies). Every
    update forms the weighted means sum_i w_i x_i / sum_i w_i (a cluster of total weight 0 goes to the origin, like an empty one);
    inertia() is sum_i w_i dist_i, accumulated sequentially in point order, and is what the initialisations are compared by;
    labels() cover every point; the initialisers see points, not weights; the N < K and N == K branches count points
    (mlhip_kmeans_step_weighted). All arguments are checked before any device work.
    @throw std::invalid_argument If `weights.size() != data.cols()`, a weight is negative or not finite, or their total is not positive. */
    DLL_DECLSPEC bool fit(ConstMatrixRef data, ConstVectorRef weights);
    unsigned int number_clusters() const override { return num_clusters_; }
    const std::vector<unsigned int>& labels() const override { return labels_; }
    const MatrixXd& centroids() const override { return centroids_; }
    DLL_DECLSPEC void set_seed(unsigned int seed);
    /** @throw std::domain_error If `absolute_tolerance < 0`. */
    DLL_DECLSPEC void set_absolute_tolerance(double absolute_tolerance);
    /** @throw std::invalid_argument If `maximum_steps < 2`. */
    DLL_DECLSPEC void set_maximum_steps(unsigned int maximum_steps);
    /** @throw std::invalid_argument If `number_initialisations < 1`. */
    DLL_DECLSPEC void set_number_initialisations(unsigned int number_initialisations);
    /** @throw std::invalid_argument If `centroids_initialiser` is null. */
    DLL_DECLSPEC void set_centroids_initialiser(std::shared_ptr<const CentroidsInitialiser> centroids_initialiser);
    void set_verbose(bool verbose) { verbose_ = verbose; }
    /** Label and squared Euclidean distance of the nearest centroid (host-side point query). */
    DLL_DECLSPEC std::pair<unsigned int, double> assign_label(ConstVectorRef x) const;
    /** Extension (not in the reference surface): assign_label for every column of `data` on the device (the assignment kernel of
    fit on a temporary device block, uploaded in row batches of 2^24 points; MLHIP_SCORE_ROWS overrides): the labels, and in
    `*squared_distances` (when given) the squared distance of every point to its centroid -- the values assign_label returns.
    @throw std::invalid_argument If `data.rows() != centroids().rows()`. @throw std::runtime_error On device failures. */
    DLL_DECLSPEC std::vector<unsigned int> assign_labels(ConstMatrixRef data, VectorXd* squared_distances = nullptr) const;
    double inertia() const { return inertia_; }
    bool converged() const override { return converged_; }
    /** Extension: number of Lloyd steps the last fit_once ran. */
    unsigned int steps_done() const { return steps_done_; }

private:
    std::vector<unsigned int> labels_;
    MatrixXd centroids_;
    MatrixXd old_centroids_;
    VectorXd work_vector_;
    std::default_random_engine prng_;
    std::shared_ptr<const CentroidsInitialiser> centroids_initialiser_;
    double absolute_tolerance_;
    double inertia_;
    unsigned int maximum_steps_;
    unsigned int num_inits_;
    unsigned int num_clusters_;
    unsigned int steps_done_;
    bool verbose_;
    bool converged_;
    const double* fit_weights_ = nullptr;   // the weights of the fit in progress (null: unweighted)

    bool fit_impl(ConstMatrixRef data);
    /// exact_fit: the WHOLE sample has exactly K rows (one cluster per sample, ML/KMeans.cpp:67-75).
    bool fit_once(ConstMatrixRef data, mlhip_data* device_data, bool exact_fit);
    void fetch_assignment(mlhip_data* device_data, std::size_t sample_size);
    void sequential_inertia(mlhip_data* device_data, std::size_t sample_size);
};

}  // namespace Clustering
}  // namespace ml
