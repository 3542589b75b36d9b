// set_covariance_regularisation / covariance_regularisation of the Eigen-typed, header-only API (include/ML/EigenApi.hpp through
// include/eigen_api), built against tests/cpp/eigen_shim (a stand-in, NOT Eigen). `host`: the default, the round trip and
// std::domain_error on a negative and on a non-finite value; `gpu`: the collinear sample of ridge_fit_test.cpp fitted from a seeded
// maximise_first start (this API has the library's initialisers only) in the three covariance types with r = 1e-3 -- every
// parameter finite, every diagonal entry of every covariance >= r.
#include <Eigen/Core>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <random>
#include <stdexcept>

#include "ML/EM.hpp"        // -I include/eigen_api comes first: this is include/ML/EigenApi.hpp

#ifndef MLHIP_ML_EIGEN_API_HPP
#error "include/eigen_api must precede include/ on the include path"
#endif

static int failures = 0;
#define ASSERT_TRUE(cond) do { if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)
#define ASSERT_THROW(expr, type) do { bool ok_ = false; try { expr; } catch (const type&) { ok_ = true; } catch (...) {} \
    if (!ok_) { std::printf("FAIL %s:%d: %s did not throw %s\n", __FILE__, __LINE__, #expr, #type); ++failures; } } while (0)

static const int D = 16, K = 8, N = 4001, STEPS = 10;
static const double R = 1e-3;

static Eigen::MatrixXd collinear_blobs()
{
    std::mt19937_64 rng(17);
    std::normal_distribution<double> g;
    Eigen::MatrixXd x(D, N);
    for (int i = 0; i < N; ++i) {
        for (int j = 0; j < D; ++j) x(j, i) = g(rng) + 3.0 * static_cast<double>((i + 3 * j) % K) + 2.0;
        x(D - 1, i) = x(0, i);
    }
    return x;
}

static void host()
{
    ml::EM em(K);
    ASSERT_TRUE(em.covariance_regularisation() == 1e-15);
    em.set_covariance_regularisation(R);
    ASSERT_TRUE(em.covariance_regularisation() == R);
    em.set_covariance_regularisation(0.0);
    ASSERT_TRUE(em.covariance_regularisation() == 0.0);
    em.set_covariance_regularisation(R);
    ASSERT_THROW(em.set_covariance_regularisation(-1e-3), std::domain_error);
    ASSERT_THROW(em.set_covariance_regularisation(std::numeric_limits<double>::quiet_NaN()), std::domain_error);
    ASSERT_THROW(em.set_covariance_regularisation(std::numeric_limits<double>::infinity()), std::domain_error);
    ASSERT_TRUE(em.covariance_regularisation() == R);
}

static void gpu()
{
    const Eigen::MatrixXd x = collinear_blobs();
    const ml::EM::CovarianceType types[3] = {ml::EM::CovarianceType::Full, ml::EM::CovarianceType::Diagonal, ml::EM::CovarianceType::Tied};
    for (int t = 0; t < 3; ++t) {
        ml::EM em(K);
        em.set_seed(3);
        em.set_covariance_type(types[t]);
        em.set_maximum_steps(STEPS);
        em.set_absolute_tolerance(0);
        em.set_relative_tolerance(0);
        em.set_maximise_first(true);
        em.set_responsibilities_initialiser(std::make_shared<ml::Clustering::ClosestCentroid>(std::make_shared<ml::Clustering::KPP>()));
        em.set_covariance_regularisation(R);
        em.fit(x);
        ASSERT_TRUE(std::isfinite(em.log_likelihood()));
        for (int k = 0; k < K; ++k) {
            ASSERT_TRUE(std::isfinite(em.mixing_probabilities()(k)));
            for (int a = 0; a < D; ++a) {
                ASSERT_TRUE(std::isfinite(em.means()(a, k)));
                for (int b = 0; b < D; ++b) ASSERT_TRUE(std::isfinite(em.covariance(static_cast<unsigned int>(k))(a, b)));
                ASSERT_TRUE(em.covariance(static_cast<unsigned int>(k))(a, a) >= R);
            }
        }
    }
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
    std::printf("ridge_fit_eigen_test %s: %d failure(s)\n", on_gpu ? "gpu" : "host", failures);
    return failures ? 1 : 0;
}
