// EM::set_covariance_regularisation / covariance_regularisation of the C++ facade (include/ML/EM.hpp). `host`: the default, the round
// trip and std::domain_error on a negative and on a non-finite value, no device needed; `gpu`: a sample with two collinear columns
// (the last coordinate repeats the first, so every M-step's covariance is singular up to rounding) fitted from a maximise_first
// start in the three covariance types with the ridge r = 1e-3 -- every parameter finite, every diagonal entry of every covariance
// >= r (Sigma_k = S_k + r I with diag(S_k) >= 0 up to rounding far below r (1 - 1e-6)).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <random>
#include <stdexcept>

#include "ML/EM.hpp"

using Matrix = ml::MatrixXd;

static int failures = 0;
#define ASSERT_TRUE(cond) do { if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)
#define ASSERT_THROW(expr, type) do { bool ok_ = false; try { expr; } catch (const type&) { ok_ = true; } catch (...) {} \
    if (!ok_) { std::printf("FAIL %s:%d: %s did not throw %s\n", __FILE__, __LINE__, #expr, #type); ++failures; } } while (0)

static const int D = 16, K = 8, N = 4001, STEPS = 10;
static const double R = 1e-3;

static Matrix collinear_blobs()
{
    std::mt19937_64 rng(17);
    std::normal_distribution<double> g;
    Matrix x(D, N);
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
    ASSERT_TRUE(em.covariance_regularisation() == R);                          // a refused value changes nothing
}

static void gpu()
{
    const Matrix x = collinear_blobs();
    Matrix start(D, K);
    for (int k = 0; k < K; ++k)
        for (int j = 0; j < D; ++j) start(j, k) = x(j, k);                     // the first K points
    const ml::EM::CovarianceType types[3] = {ml::EM::CovarianceType::Full, ml::EM::CovarianceType::Diagonal, ml::EM::CovarianceType::Tied};
    for (int t = 0; t < 3; ++t) {
        ml::EM em(K);
        em.set_covariance_type(types[t]);
        em.set_maximum_steps(STEPS);
        em.set_absolute_tolerance(0);
        em.set_relative_tolerance(0);
        em.set_maximise_first(true);
        em.set_responsibilities_initialiser(
            std::make_shared<ml::Clustering::ClosestCentroid>(std::make_shared<ml::Clustering::FixedCentroids>(start)));
        em.set_covariance_regularisation(R);
        em.fit(x);
        ASSERT_TRUE(em.steps_done() == static_cast<unsigned int>(STEPS));
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
    if (failures) return 1;
    std::printf("ridge_fit_test: ok (%s)\n", on_gpu ? "gpu" : "host");
    return 0;
}
