// EM::fit(data, weights) of the C++ facade (include/ML/EM.hpp) and, with -DWEIGHTED_EIGEN and include/eigen_api first on the
// include path, of the Eigen-typed API (include/ML/EigenApi.hpp, against tests/cpp/eigen_shim: a stand-in, NOT Eigen).
// `host`: argument errors, no device needed; `gpu`: a fit with integer weights against the fit of the replicated sample.
#ifdef WEIGHTED_EIGEN
#include <Eigen/Core>
#endif

#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <stdexcept>
#include <vector>

#include "ML/EM.hpp"

#ifdef WEIGHTED_EIGEN
#ifndef MLHIP_ML_EIGEN_API_HPP
#error "include/eigen_api must precede include/ on the include path"
#endif
using Matrix = Eigen::MatrixXd;
using Vector = Eigen::VectorXd;
#else
using Matrix = ml::MatrixXd;
using Vector = ml::VectorXd;
#endif

static int failures = 0;
#define ASSERT_TRUE(cond) do { if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)
#define ASSERT_THROW(expr, type) do { bool ok_ = false; try { expr; } catch (const type&) { ok_ = true; } catch (...) {} \
    if (!ok_) { std::printf("FAIL %s:%d: %s did not throw %s\n", __FILE__, __LINE__, #expr, #type); ++failures; } } while (0)

static Matrix blobs(int d, int n, unsigned seed)
{
    std::mt19937_64 rng(seed);
    std::normal_distribution<double> g;
    Matrix x(d, n);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < d; ++j) x(j, i) = g(rng) + 4.0 * static_cast<double>((i + j) % 3) + 2.0;
    return x;
}

static void host()
{
    const Matrix x = blobs(3, 10, 1);
    Vector w(9);
    for (int i = 0; i < 9; ++i) w(i) = 1.0;
    ml::EM em(2);
    ASSERT_THROW(em.fit(x, w), std::invalid_argument);               // one weight per point, checked before any device call
}

static std::unique_ptr<ml::EM> model(int K)
{
    auto em = std::make_unique<ml::EM>(K);
    em->set_seed(3);
    em->set_maximum_steps(4);
    em->set_absolute_tolerance(0);
    em->set_relative_tolerance(0);
    return em;
}

static void compare(const ml::EM& a, const ml::EM& b, int d, int K)
{
    ASSERT_TRUE(std::fabs(a.log_likelihood() - b.log_likelihood()) <= 1e-11 * std::fabs(b.log_likelihood()));
    for (int k = 0; k < K; ++k) {
        ASSERT_TRUE(std::fabs(a.mixing_probabilities()(k) - b.mixing_probabilities()(k)) <= 1e-11);
        for (int j = 0; j < d; ++j)
            ASSERT_TRUE(std::fabs(a.means()(j, k) - b.means()(j, k)) <= 1e-10 * (1.0 + std::fabs(b.means()(j, k))));
    }
}

static void gpu()
{
    const int d = 4, K = 3, n = 3001;
    const Matrix x = blobs(d, n, 7);
    Vector w(n);
    auto weighted = model(K), other = model(K);
#ifdef WEIGHTED_EIGEN
    // the Eigen-typed API has the library's initialisers only, and those see points: with every weight 1 the same points are
    // drawn and W = N, so the weighted route must give the plain fit up to rounding
    for (int i = 0; i < n; ++i) w(i) = 1.0;
    weighted->fit(x, w);
    other->fit(x);
#else
    // integer weights against the fit of the replicated sample from the same fixed start
    int total = 0;
    for (int i = 0; i < n; ++i) { w(i) = static_cast<double>((i * 7 + 3) % 4); total += (i * 7 + 3) % 4; }
    Matrix rep(d, total);
    for (int i = 0, c = 0; i < n; ++i)
        for (int r = 0; r < static_cast<int>(w(i)); ++r, ++c)
            for (int j = 0; j < d; ++j) rep(j, c) = x(j, i);
    Matrix start(d, K);
    for (int k = 0; k < K; ++k)
        for (int j = 0; j < d; ++j) start(j, k) = 2.0 + 4.0 * static_cast<double>((k + j) % 3);
    weighted->set_means_initialiser(std::make_shared<ml::Clustering::FixedCentroids>(start));
    other->set_means_initialiser(std::make_shared<ml::Clustering::FixedCentroids>(start));
    weighted->fit(x, w);
    other->fit(rep);
#endif
#ifdef WEIGHTED_EIGEN
    {
        // one component: after the first M-step the parameters are the weighted mean and covariance whatever point the initialiser
        // drew, so non-uniform integer weights can be held against the fit of the replicated sample (a fit that ignored the
        // weights would miss it in the first digits)
        int total = 0;
        Vector w1(n);
        for (int i = 0; i < n; ++i) { w1(i) = static_cast<double>((i * 7 + 3) % 4); total += (i * 7 + 3) % 4; }
        Matrix rep(d, total);
        for (int i = 0, c = 0; i < n; ++i)
            for (int r = 0; r < static_cast<int>(w1(i)); ++r, ++c)
                for (int j = 0; j < d; ++j) rep(j, c) = x(j, i);
        auto one_w = model(1), one_r = model(1), one_plain = model(1);
        one_w->fit(x, w1);
        one_r->fit(rep);
        one_plain->fit(x);
        compare(*one_w, *one_r, d, 1);
        ASSERT_TRUE(std::fabs(one_w->covariance(0)(0, 0) - one_r->covariance(0)(0, 0)) <= 1e-10 * std::fabs(one_r->covariance(0)(0, 0)));
        ASSERT_TRUE(std::fabs(one_w->means()(0, 0) - one_plain->means()(0, 0)) > 1e-6);   // (the weights do move the answer)
    }
#endif
    ASSERT_TRUE(weighted->labels().size() == static_cast<std::size_t>(n));   // per point, not per unit of weight
    compare(*weighted, *other, d, K);
    Vector bad = w;
    bad(5) = -1.0;
    ASSERT_THROW(weighted->fit(x, bad), std::invalid_argument);
    // the same object, unweighted again: the fit of a fresh object with the same settings
    auto fresh = model(K);
    weighted->set_seed(3);
    weighted->set_means_initialiser(std::make_shared<ml::Clustering::Forgy>());
    weighted->fit(x);
    fresh->fit(x);
    ASSERT_TRUE(weighted->log_likelihood() == fresh->log_likelihood());
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
    std::printf("weighted_fit_test: ok (%s)\n", on_gpu ? "gpu" : "host");
    return 0;
}
