// EM::set_number_initialisations of the C++ facade (include/ML/EM.hpp). `host`: the setter, its exception and the getters, no device
// needed; `gpu`: a fit with 3 initialisations whose starts come from a means initialiser of this test's own (start r: the sample's
// points r, r + 401, r + 802 -- no random numbers, so the Python side can form them again); the fitted parameters are printed for
// tests/test_cpp_em_restarts.py to hold against the winner of Data.em_iterate_restarts from the same starts.
// With -DRESTARTS_EIGEN and include/eigen_api first on the include path: the same surface through the Eigen-typed API
// (include/ML/EigenApi.hpp, against tests/cpp/eigen_shim: a stand-in, NOT Eigen), whose EM has the library's initialisers only: the
// seeded default start, checked for the surface's own consistency.
#ifdef RESTARTS_EIGEN
#include <Eigen/Core>
#endif

#include <cstdio>
#include <cmath>
#include <cstring>
#include <memory>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "ML/EM.hpp"

#ifdef RESTARTS_EIGEN
#ifndef MLHIP_ML_EIGEN_API_HPP
#error "include/eigen_api must precede include/ on the include path"
#endif
using Matrix = Eigen::MatrixXd;
#else
using Matrix = ml::MatrixXd;
#endif

static int failures = 0;
#define ASSERT_TRUE(cond) do { if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static const int D = 2, K = 3, N = 1203, STEPS = 6, R = 3;

static Matrix blobs()
{
    std::mt19937_64 rng(5);
    std::normal_distribution<double> g;
    Matrix x(D, N);
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < D; ++j) x(j, i) = g(rng) + 5.0 * static_cast<double>((i + 2 * j) % 3);
    return x;
}

static void host()
{
    ml::EM em(K);
    ASSERT_TRUE(em.number_initialisations() == 1u);
    em.set_number_initialisations(4);
    ASSERT_TRUE(em.number_initialisations() == 4u);
    bool thrown = false;
    try {
        em.set_number_initialisations(0);
    } catch (const std::invalid_argument& e) {
        thrown = std::string(e.what()) == "EM: At least 1 initialisation required";
    }
    ASSERT_TRUE(thrown);
    ASSERT_TRUE(em.number_initialisations() == 4u);
    ASSERT_TRUE(em.best_initialisation() == 0u);
    ASSERT_TRUE(em.initialisation_log_likelihoods().empty() && em.initialisation_steps().empty() && em.initialisation_converged().empty());
}

static void gpu()
{
    const Matrix x = blobs();
    ml::EM em(K);
    em.set_seed(7);
    em.set_maximum_steps(STEPS);
    em.set_absolute_tolerance(0);
    em.set_relative_tolerance(0);
    em.set_number_initialisations(R);
#ifndef RESTARTS_EIGEN
    struct Rotating : ml::Clustering::CentroidsInitialiser {
        mutable int call = 0;
        void init(ml::ConstMatrixRef data, std::default_random_engine&, unsigned int number_clusters, ml::MatrixRef centroids) const override
        {
            // start r: the points r, r + 401, r + 802 of the sample
            for (unsigned int k = 0; k < number_clusters; ++k)
                for (ml::Index j = 0; j < data.rows(); ++j) centroids(j, k) = data(j, call + 401 * static_cast<ml::Index>(k));
            ++call;
        }
    };
    em.set_means_initialiser(std::make_shared<Rotating>());
#endif
    em.fit(x);
    ASSERT_TRUE(em.number_initialisations() == static_cast<unsigned int>(R));
    ASSERT_TRUE(em.initialisation_log_likelihoods().size() == static_cast<std::size_t>(R));
    ASSERT_TRUE(em.initialisation_steps().size() == static_cast<std::size_t>(R) && em.initialisation_converged().size() == static_cast<std::size_t>(R));
    const unsigned int best = em.best_initialisation();
    ASSERT_TRUE(best < static_cast<unsigned int>(R));
    ASSERT_TRUE(em.log_likelihood() == em.initialisation_log_likelihoods()[best]);
    ASSERT_TRUE(em.initialisation_steps()[best] == static_cast<unsigned int>(STEPS));
#ifndef RESTARTS_EIGEN
    ASSERT_TRUE(em.steps_done() == static_cast<unsigned int>(STEPS));
#endif
    ASSERT_TRUE(!em.converged() && em.initialisation_converged()[best] == 0);
    for (int r = 0; r < R; ++r) ASSERT_TRUE(!(em.initialisation_log_likelihoods()[r] > em.log_likelihood()));   // none converged: the greatest wins
#ifndef RESTARTS_EIGEN
    // the sample (row-major N x D), then the fitted state, one value per line
    std::printf("shape %d %d %d %d %d\n", N, D, K, STEPS, R);
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < D; ++j) std::printf("x %.17g\n", x(j, i));
    std::printf("best %u\n", best);
    for (int r = 0; r < R; ++r) std::printf("lls %.17g\n", em.initialisation_log_likelihoods()[r]);
    std::printf("ll %.17g\n", em.log_likelihood());
    for (int k = 0; k < K; ++k) std::printf("pi %.17g\n", em.mixing_probabilities()(k));
    for (int k = 0; k < K; ++k)
        for (int j = 0; j < D; ++j) std::printf("mu %.17g\n", em.means()(j, k));
    for (int k = 0; k < K; ++k)
        for (int a = 0; a < D; ++a)
            for (int b = 0; b < D; ++b) std::printf("cov %.17g\n", em.covariances()[k](a, b));
#endif
}

int main(int argc, char** argv)
{
    const bool on_gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    try {
        host();
        if (on_gpu) gpu();
    } catch (const std::exception& e) {
        std::printf("FAIL: unexpected exception: %s\n", e.what());
        return 1;
    }
    if (failures) return 1;
    std::printf("em_restarts_test: ok (%s)\n", on_gpu ? "gpu" : "host");
    return 0;
}
