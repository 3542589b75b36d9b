/* mlpp_c.h -- flat C handles over the C++ facade (the headers under include/ML), so that the Python surface
 * ml_amd.cppyml.clustering (the mirror of the reference's pybind11 module, cppyml/clustering.cpp:75-185) is plain
 * ctypes and needs neither pybind11 nor Eigen. Every function returns 0 or an MLHIP_E_* code (see mlhip.h);
 * mlhip_last_error() holds the message. std::invalid_argument / std::domain_error map to MLHIP_E_INVALID_ARGUMENT /
 * MLHIP_E_DOMAIN -- the Python side raises ValueError for both, as pybind11 does for the reference. */
#ifndef MLPP_C_H
#define MLPP_C_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mlpp_centroids_initialiser mlpp_centroids_initialiser;           /* shared_ptr<const CentroidsInitialiser> */
typedef struct mlpp_responsibilities_initialiser mlpp_responsibilities_initialiser;
typedef struct mlpp_em mlpp_em;
typedef struct mlpp_kmeans mlpp_kmeans;

/* ---- initialisers (cppyml/clustering.cpp:79-101) ---- */
int mlpp_forgy_create(mlpp_centroids_initialiser** out);
int mlpp_random_partition_create(mlpp_centroids_initialiser** out);
int mlpp_kpp_create(mlpp_centroids_initialiser** out);
/* Extension: K-means++ seeding from exact integer cumulative weights (ML::Clustering::FixedPointKPP): the D^2 distribution of KPP,
 * but not its draws; on the GPU every draw stays on the device, whatever N. */
int mlpp_fixed_point_kpp_create(mlpp_centroids_initialiser** out);
/* Extension: fixed centroids, K x d row-major (row k = centroid k). */
int mlpp_fixed_centroids_create(const double* centroids, uint32_t K, uint32_t d, mlpp_centroids_initialiser** out);
int mlpp_centroids_initialiser_destroy(mlpp_centroids_initialiser* h);
/* Runs the initialiser on N x d row-major data with a std::default_random_engine seeded with `seed` (seed_set != 0)
 * or default-constructed; out: K x d row-major. For tests of the host-side initialisers. */
int mlpp_centroids_initialiser_run(const mlpp_centroids_initialiser* h, const double* data, uint64_t n, uint32_t d,
                                   uint32_t K, int seed_set, uint32_t seed, double* centroids_out);
/* The same through the path `fit` takes: the data is uploaded to the facade's GPU and the initialiser's O(N) passes (K-means++
 * distances, RandomPartition's running means: SURVEY 8 f1) run there; the result is bit-identical to the host run above. */
int mlpp_centroids_initialiser_run_on_device(const mlpp_centroids_initialiser* h, const double* data, uint64_t n, uint32_t d,
                                             uint32_t K, int seed_set, uint32_t seed, double* centroids_out);
int mlpp_closest_centroid_create(const mlpp_centroids_initialiser* centroids_initialiser, mlpp_responsibilities_initialiser** out);
int mlpp_responsibilities_initialiser_destroy(mlpp_responsibilities_initialiser* h);
/* out: N x K column-major. */
int mlpp_responsibilities_initialiser_run(const mlpp_responsibilities_initialiser* h, const double* data, uint64_t n,
                                          uint32_t d, uint32_t K, int seed_set, uint32_t seed, double* resp_out);

/* ---- EM (cppyml/clustering.cpp:103-146; data = N x d row-major == d x N column-major) ---- */
int mlpp_em_create(uint32_t number_components, mlpp_em** out);
int mlpp_em_destroy(mlpp_em* h);
int mlpp_em_set_seed(mlpp_em* h, uint32_t seed);
int mlpp_em_set_absolute_tolerance(mlpp_em* h, double v);
int mlpp_em_set_relative_tolerance(mlpp_em* h, double v);
int mlpp_em_set_maximum_steps(mlpp_em* h, uint32_t v);
int mlpp_em_set_means_initialiser(mlpp_em* h, const mlpp_centroids_initialiser* init);
int mlpp_em_set_responsibilities_initialiser(mlpp_em* h, const mlpp_responsibilities_initialiser* init);
int mlpp_em_set_verbose(mlpp_em* h, int v);
int mlpp_em_set_maximise_first(mlpp_em* h, int v);
/* Extension (ml::EM::set_covariance_type): 0 = full covariances (the reference), 1 = diagonal, 2 = tied (one covariance shared by
 * all components); any other nonzero value selects diagonal, as it always did. */
int mlpp_em_set_covariance_type(mlpp_em* h, int covariance_type);
/* EXTENSION: ml::EM::set_covariance_regularisation / covariance_regularisation (scikit-learn's reg_covar; default 1e-15). A negative or
 * non-finite value: MLHIP_E_DOMAIN, the model keeps its value. */
int mlpp_em_set_covariance_regularisation(mlpp_em* h, double v);
int mlpp_em_covariance_regularisation(const mlpp_em* h, double* out);
/* EXTENSION: ml::EM::set_number_initialisations / number_initialisations (restarts; the reference's EM has none, default 1) and what the
 * last fit recorded per initialisation. 0 initialisations: MLHIP_E_INVALID_ARGUMENT, the model keeps its value. The three per-
 * initialisation getters write min(capacity, *count) entries to `out` (NULL with capacity 0: ask for the count alone) and the number
 * of initialisations the last fit ran to *count (0 before any fit; 1 for the exact N == K fit). */
int mlpp_em_set_number_initialisations(mlpp_em* h, uint32_t v);
int mlpp_em_number_initialisations(const mlpp_em* h, uint32_t* out);
int mlpp_em_best_initialisation(const mlpp_em* h, uint32_t* out);
int mlpp_em_initialisation_log_likelihoods(const mlpp_em* h, double* out, uint32_t capacity, uint32_t* count);
int mlpp_em_initialisation_steps(const mlpp_em* h, uint32_t* out, uint32_t capacity, uint32_t* count);
int mlpp_em_initialisation_converged(const mlpp_em* h, int* out, uint32_t capacity, uint32_t* count);
int mlpp_em_fit(mlpp_em* h, const double* data, uint64_t n, uint32_t d, int* converged);
/* Extension (ml::EM::fit(data, weights)): the fit of a weighted sample, weights[i] >= 0 the frequency weight of point i (n values). */
int mlpp_em_fit_weighted(mlpp_em* h, const double* data, const double* weights, uint64_t n, uint32_t d, int* converged);
int mlpp_em_number_components(const mlpp_em* h, uint32_t* out);
int mlpp_em_dims(const mlpp_em* h, uint32_t* d, uint64_t* n);
int mlpp_em_means(const mlpp_em* h, double* out /* d x K column-major, like EM::means() */);
int mlpp_em_covariance(const mlpp_em* h, uint32_t k, double* out /* d x d */);
int mlpp_em_mixing_probabilities(const mlpp_em* h, double* out);
int mlpp_em_responsibilities(const mlpp_em* h, double* out /* N x K column-major */);
/* Extension: rows [first_row, first_row + n_rows) only (n_rows x K column-major) -- no N x K host copy while the block is on the device. */
int mlpp_em_responsibilities_rows(const mlpp_em* h, uint64_t first_row, uint64_t n_rows, double* out);
int mlpp_em_log_likelihood(const mlpp_em* h, double* out);
int mlpp_em_labels(const mlpp_em* h, uint32_t* out);
int mlpp_em_converged(const mlpp_em* h, int* out);
int mlpp_em_steps_done(const mlpp_em* h, uint32_t* out);
int mlpp_em_assign_responsibilities(const mlpp_em* h, const double* x, uint32_t xlen, double* u, uint32_t ulen);
/* Extensions (not in the reference surface): the batch queries of ml::EM on N x d row-major data under the fitted parameters --
 * EM::log_densities (out: n doubles), EM::assign_labels (out: n labels), EM::calculate_responsibilities (out: N x K column-major). */
int mlpp_em_score_samples(const mlpp_em* h, const double* data, uint64_t n, uint32_t d, double* out);
int mlpp_em_predict(const mlpp_em* h, const double* data, uint64_t n, uint32_t d, uint32_t* out);
int mlpp_em_predict_proba(const mlpp_em* h, const double* data, uint64_t n, uint32_t d, double* out);
/* Extensions (model selection): EM::number_parameters (host only; the mode the model was fitted in), EM::bic and EM::aic on N x d
 * row-major data -- -2 N (mean log-density) + p log N and + 2 p, scikit-learn's definitions; the scoring pass of mlpp_em_score_samples. */
int mlpp_em_number_parameters(const mlpp_em* h, uint64_t* out);
int mlpp_em_bic(const mlpp_em* h, const double* data, uint64_t n, uint32_t d, double* out);
int mlpp_em_aic(const mlpp_em* h, const double* data, uint64_t n, uint32_t d, double* out);
/* Extension: Clustering::silhouette_samples -- exact silhouette values (Euclidean) of rows of x (n x d row-major) under `labels`
 * (n labels, each < K), on the device (mlhip_silhouette holds the definition and the fixed arithmetic). rows: n_rows row indices in
 * any order, repeats allowed; NULL: all n rows in order. s_out: one double per evaluated row. Every row meets every other, so there
 * are no row batches: the block is uploaded once, and a block that does not fit the device is refused. */
int mlpp_silhouette_samples(const double* x, uint64_t n, uint32_t d, const uint32_t* labels, uint32_t K, const uint64_t* rows, uint64_t n_rows,
                            double* s_out);
/* Extension: EM::sample -- n points drawn from the fitted mixture on the device, point i a pure function of (seed, i) and the
 * parameters (mlhip_em_sample). x_out: n x d row-major (a point in every row); labels_out (n, the components drawn) may be NULL.
 * n = 0 writes nothing. */
int mlpp_em_sample(const mlpp_em* h, uint64_t n, uint64_t seed, double* x_out, uint32_t* labels_out);
/* Extension: EM::conditional_means -- E[x_M | x_O] under the fitted mixture for n points (mlhip_em_condition,
 * mlhip_em_conditional_means). observed: n_observed distinct coordinates; data_observed: n x n_observed row-major (column c =
 * coordinate observed[c]); out: n x (d - n_observed) row-major, the missing coordinates ascending; log_density_out (n) may be NULL.
 * n = 0 writes nothing. */
int mlpp_em_conditional_means(const mlpp_em* h, const uint32_t* observed, uint32_t n_observed, const double* data_observed, uint64_t n,
                              double* out, double* log_density_out);
/* Extension: EM::impute -- every NaN of n points replaced by its conditional expectation under the fitted mixture given the
 * coordinates that point has (mlhip_em_impute). data and out: n x d row-major; log_density_out (n) and responsibilities_out (n x K
 * row-major) may be NULL. n = 0 writes nothing. */
int mlpp_em_impute(const mlpp_em* h, const double* data, uint64_t n, uint32_t d, double* out, double* log_density_out,
                   double* responsibilities_out);
/* Extension: EM::conditional_covariances -- the covariances of the conditioned components (mlhip_em_condition_covariances; host
 * only). out: K x dM x dM, dM = d - n_observed. */
int mlpp_em_conditional_covariances(const mlpp_em* h, const uint32_t* observed, uint32_t n_observed, double* out);
/* Extension: EM::conditional_samples -- n_draws draws from p(x_M | x_O) under the fitted mixture for n points
 * (mlhip_em_conditional_samples). observed, data_observed as for mlpp_em_conditional_means; out: n_draws x n x (d - n_observed)
 * row-major, draw-major; labels_out (n_draws x n, the components drawn) may be NULL. n = 0 or n_draws = 0 writes nothing. */
int mlpp_em_conditional_samples(const mlpp_em* h, const uint32_t* observed, uint32_t n_observed, const double* data_observed, uint64_t n,
                                uint64_t n_draws, uint64_t seed, double* out, uint32_t* labels_out);
/* Extension: EM::conditional_variances -- the per-row predictive covariance Var[x_M | x_O] under the fitted mixture for n points
 * (mlhip_em_conditional_variances). observed, data_observed as for mlpp_em_conditional_means; out: n x dM row-major, dM =
 * d - n_observed, or with full != 0 n x dM x dM (the matrix of point i in row i); means_out (n x dM, the bits of
 * mlpp_em_conditional_means) may be NULL. n = 0 writes nothing. */
int mlpp_em_conditional_variances(const mlpp_em* h, const uint32_t* observed, uint32_t n_observed, const double* data_observed, uint64_t n,
                                  int full, double* out, double* means_out);
/* Extension: EM::conditional_cdfs -- P(x_j <= v | x_O) per missing coordinate under the fitted mixture for n points
 * (mlhip_em_conditional_cdfs). observed, data_observed as for mlpp_em_conditional_means; values and out: n x dM row-major, dM =
 * d - n_observed, the missing coordinates in ascending order. n = 0 writes nothing. */
int mlpp_em_conditional_cdfs(const mlpp_em* h, const uint32_t* observed, uint32_t n_observed, const double* data_observed, uint64_t n,
                             const double* values, double* out);
/* Extension: EM::conditional_quantiles -- the inverse of mlpp_em_conditional_cdfs at n_probabilities probabilities, each strictly
 * inside (0, 1) (mlhip_em_conditional_quantiles). out: n_probabilities x n x dM row-major, probability-major. n = 0 or
 * n_probabilities = 0 writes nothing. */
int mlpp_em_conditional_quantiles(const mlpp_em* h, const uint32_t* observed, uint32_t n_observed, const double* data_observed, uint64_t n,
                                  const double* probabilities, uint64_t n_probabilities, double* out);

/* ---- KMeans (cppyml/clustering.cpp:148-183) ---- */
int mlpp_kmeans_create(uint32_t number_clusters, mlpp_kmeans** out);
int mlpp_kmeans_destroy(mlpp_kmeans* h);
int mlpp_kmeans_set_seed(mlpp_kmeans* h, uint32_t seed);
int mlpp_kmeans_set_absolute_tolerance(mlpp_kmeans* h, double v);
int mlpp_kmeans_set_maximum_steps(mlpp_kmeans* h, uint32_t v);
int mlpp_kmeans_set_number_initialisations(mlpp_kmeans* h, uint32_t v);
int mlpp_kmeans_set_centroids_initialiser(mlpp_kmeans* h, const mlpp_centroids_initialiser* init);
int mlpp_kmeans_set_verbose(mlpp_kmeans* h, int v);
int mlpp_kmeans_fit(mlpp_kmeans* h, const double* data, uint64_t n, uint32_t d, int* converged);
/* Extension (ml::Clustering::KMeans::fit(data, weights)): the fit of a weighted sample, weights[i] >= 0 the frequency weight of point i
 * (n values); checked before any device work. */
int mlpp_kmeans_fit_weighted(mlpp_kmeans* h, const double* data, const double* weights, uint64_t n, uint32_t d, int* converged);
int mlpp_kmeans_number_clusters(const mlpp_kmeans* h, uint32_t* out);
int mlpp_kmeans_dims(const mlpp_kmeans* h, uint32_t* d, uint64_t* n);
int mlpp_kmeans_centroids(const mlpp_kmeans* h, double* out /* K x d row-major == d x K column-major */);
int mlpp_kmeans_labels(const mlpp_kmeans* h, uint32_t* out);
int mlpp_kmeans_inertia(const mlpp_kmeans* h, double* out);
int mlpp_kmeans_converged(const mlpp_kmeans* h, int* out);
int mlpp_kmeans_steps_done(const mlpp_kmeans* h, uint32_t* out);
int mlpp_kmeans_assign_label(const mlpp_kmeans* h, const double* x, uint32_t xlen, uint32_t* label, double* dist2);
/* Extension: KMeans::assign_labels on N x d row-major data -- labels (n) and, unless dist2 is NULL, the squared distances (n doubles). */
int mlpp_kmeans_predict(const mlpp_kmeans* h, const double* data, uint64_t n, uint32_t d, uint32_t* labels, double* dist2);

/* ---- LinearAlgebra helpers (ML/LinearAlgebra.hpp:18-31), column-major ---- */
int mlpp_xAx_symmetric(const double* A, uint32_t rows, uint32_t cols, const double* x, uint32_t xlen, double* out);
int mlpp_xxT(const double* x, uint32_t n, double* dest /* n x n */);
int mlpp_add_a_xxT(const double* x, uint32_t n, double* dest, uint32_t drows, uint32_t dcols, double a);

/* ---- LinearRegression::calculate_XXt_beta (ML/LinearRegression.hpp:412): X is N x q row-major == q x N column-major ---- */
int mlpp_calculate_XXt_beta(const double* X, uint64_t n, uint32_t q, const double* y, uint64_t ylen, const double* lambda,
                            uint32_t lambda_len, double* XXt /* q x q */, double* beta /* q */);

/* ---- device context of the facade (include/ML/Device.hpp): the process-wide mlhip_ctx the model classes run on. A
 * row-sharded job installs its all-reduce hook on it (mlhip_ctx_set_allreduce) before calling fit() on every rank. ---- */
int mlpp_device_context(struct mlhip_ctx** out);          /* ml::device::context(): created on first use, not owned by the caller */
int mlpp_device_set_context(struct mlhip_ctx* ctx);       /* ml::device::set_context(); NULL restores the default */

#ifdef __cplusplus
}
#endif
#endif /* MLPP_C_H */
