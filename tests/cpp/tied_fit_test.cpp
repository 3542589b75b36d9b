// EM::CovarianceType::Tied of the C++ facade (include/ML/EM.hpp). `host`: the type is accepted and reported, no device needed;
// `gpu`: a fit from fixed means -- every covariance is the one shared matrix, bit for bit -- whose parameters are printed for the
// Python side (tests/test_cpp_tied_fit.py) to hold against mlhip_em_iterate from the same start.
// With -DTIED_EIGEN and include/eigen_api first on the include path: the same enum value through the Eigen-typed API
// (include/ML/EigenApi.hpp, against tests/cpp/eigen_shim: a stand-in, NOT Eigen), whose EM has the library's initialisers only.
#ifdef TIED_EIGEN
#include <Eigen/Core>
#endif

#include <cstdio>
#include <cmath>
#include <cstring>
#include <memory>
#include <random>
#include <stdexcept>

#include "ML/EM.hpp"

#ifdef TIED_EIGEN
#ifndef MLHIP_ML_EIGEN_API_HPP
#error "include/eigen_api must precede include/ on the include path"
#endif
using Matrix = Eigen::MatrixXd;
#else
using Matrix = ml::MatrixXd;
#endif

static int failures = 0;
#define ASSERT_TRUE(cond) do { if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static const int D = 4, K = 3, N = 1501, STEPS = 5;

static Matrix blobs()
{
    std::mt19937_64 rng(11);
    std::normal_distribution<double> g;
    Matrix x(D, N);
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < D; ++j) x(j, i) = g(rng) + 4.0 * static_cast<double>((i + j) % 3) + 2.0;
    return x;
}

static void host()
{
    ml::EM em(K);
#ifdef TIED_EIGEN
    ASSERT_TRUE(static_cast<int>(ml::EM::CovarianceType::Tied) == 2);       // (the value mlpp_em_set_covariance_type takes)
    em.set_covariance_type(ml::EM::CovarianceType::Tied);
#else
    ASSERT_TRUE(em.covariance_type() == ml::EM::CovarianceType::Full);
    em.set_covariance_type(ml::EM::CovarianceType::Tied);
    ASSERT_TRUE(em.covariance_type() == ml::EM::CovarianceType::Tied);
#endif
}

#ifdef TIED_EIGEN
static void gpu()
{
    // the same seeded fit in the three modes: tied -> one matrix for every component, bit for bit; full -> the components differ;
    // diagonal -> no off-diagonal entry
    const Matrix x = blobs();
    const ml::EM::CovarianceType types[3] = {ml::EM::CovarianceType::Tied, ml::EM::CovarianceType::Full, ml::EM::CovarianceType::Diagonal};
    for (int t = 0; t < 3; ++t) {
        ml::EM em(K);
        em.set_seed(3);
        em.set_maximum_steps(STEPS);
        em.set_absolute_tolerance(0);
        em.set_relative_tolerance(0);
        em.set_covariance_type(types[t]);
        em.fit(x);
        bool same = true;
        double off = 0.0, sum = 0.0;
        for (int a = 0; a < D; ++a)
            for (int b = 0; b < D; ++b) {
                same = same && em.covariances()[0](a, b) == em.covariances()[K - 1](a, b);
                if (a != b) off += std::fabs(em.covariances()[0](a, b));
            }
        for (int k = 0; k < K; ++k) sum += em.mixing_probabilities()(k);
        ASSERT_TRUE(std::fabs(sum - 1.0) < 1e-12);
        if (t == 0) {
            ASSERT_TRUE(same && off > 0.0);
            for (int a = 0; a < D; ++a)
                for (int b = 0; b < a; ++b) ASSERT_TRUE(em.covariances()[0](a, b) == em.covariances()[0](b, a));
        }
        if (t == 1) ASSERT_TRUE(!same && off > 0.0);
        if (t == 2) ASSERT_TRUE(!same && off == 0.0);
    }
}
#else

static void gpu()
{
    const Matrix x = blobs();
    Matrix start(D, K);
    for (int k = 0; k < K; ++k)
        for (int j = 0; j < D; ++j) start(j, k) = 2.0 + 4.0 * static_cast<double>((k + j) % 3);
    ml::EM em(K);
    em.set_covariance_type(ml::EM::CovarianceType::Tied);
    em.set_maximum_steps(STEPS);
    em.set_absolute_tolerance(0);
    em.set_relative_tolerance(0);
    em.set_means_initialiser(std::make_shared<ml::Clustering::FixedCentroids>(start));
    em.fit(x);
    ASSERT_TRUE(em.steps_done() == static_cast<unsigned int>(STEPS));
    ASSERT_TRUE(em.covariances().size() == static_cast<std::size_t>(K));
    for (int a = 0; a < D; ++a)
        for (int b = 0; b < D; ++b) ASSERT_TRUE(em.covariances()[0](a, b) == em.covariances()[K - 1](a, b));
    // the sample (row-major N x D), then the fitted parameters, one value per line
    std::printf("shape %d %d %d %d\n", N, D, K, STEPS);
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < D; ++j) std::printf("x %.17g\n", x(j, i));
    for (int k = 0; k < K; ++k)
        for (int j = 0; j < D; ++j) std::printf("start %.17g\n", start(j, k));
    std::printf("ll %.17g\n", em.log_likelihood());
    for (int k = 0; k < K; ++k) std::printf("pi %.17g\n", em.mixing_probabilities()(k));
    for (int k = 0; k < K; ++k)
        for (int j = 0; j < D; ++j) std::printf("mu %.17g\n", em.means()(j, k));
    for (int a = 0; a < D; ++a)
        for (int b = 0; b < D; ++b) std::printf("cov %.17g\n", em.covariances()[0](a, b));
}
#endif

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
    std::printf("tied_fit_test: ok (%s)\n", on_gpu ? "gpu" : "host");
    return 0;
}
