// KMeans::fit(data, weights) of the C++ facade (include/ML/KMeans.hpp) and, with -DWEIGHTED_EIGEN and include/eigen_api first on the
// include path, of the Eigen-typed API (include/ML/EigenApi.hpp, against tests/cpp/eigen_shim: a stand-in, NOT Eigen).
// `host`: argument errors, no device needed; `gpu`: a fit with integer weights of a sample on the grid 2^-10 Z against the fit of
// the replicated sample -- every sum is exact there, so the centroids are compared with ==.
#ifdef WEIGHTED_EIGEN
#include <Eigen/Core>
#endif

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <random>
#include <stdexcept>
#include <vector>

#include "ML/KMeans.hpp"

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
using ml::Clustering::KMeans;

static int failures = 0;
#define ASSERT_TRUE(cond) do { if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)
#define ASSERT_THROW(expr, type) do { bool ok_ = false; try { expr; } catch (const type&) { ok_ = true; } catch (...) {} \
    if (!ok_) { std::printf("FAIL %s:%d: %s did not throw %s\n", __FILE__, __LINE__, #expr, #type); ++failures; } } while (0)

/// Three blobs on the grid 2^-10 Z, |x| < 16.
static Matrix blobs(int d, int n, unsigned seed)
{
    std::mt19937_64 rng(seed);
    std::uniform_int_distribution<int> offset(-2048, 2048);
    Matrix x(d, n);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < d; ++j) x(j, i) = 8.0 * static_cast<double>((i + j) % 3 - 1) + static_cast<double>(offset(rng)) / 1024.0;
    return x;
}

static Vector ones(int n, double value = 1.0)
{
    Vector w(n);
    for (int i = 0; i < n; ++i) w(i) = value;
    return w;
}

static void host()
{
    // all of these are refused before any device call: they throw std::invalid_argument with or without a GPU
    const Matrix x = blobs(3, 10, 1);
    KMeans km(2);
    ASSERT_THROW(km.fit(x, ones(9)), std::invalid_argument);          // one weight per point
    Vector bad = ones(10);
    bad(3) = -1.0;
    ASSERT_THROW(km.fit(x, bad), std::invalid_argument);
    bad(3) = std::numeric_limits<double>::quiet_NaN();
    ASSERT_THROW(km.fit(x, bad), std::invalid_argument);
    bad(3) = std::numeric_limits<double>::infinity();
    ASSERT_THROW(km.fit(x, bad), std::invalid_argument);
    ASSERT_THROW(km.fit(x, ones(10, 0.0)), std::invalid_argument);    // a total that is not positive
}

static void replicated(const Matrix& x, int d, int n, Vector& w, Matrix& rep)
{
    int total = 0;
    for (int i = 0; i < n; ++i) { w(i) = static_cast<double>((i * 7 + 3) % 5); total += (i * 7 + 3) % 5; }
    rep = Matrix(d, total);
    for (int i = 0, c = 0; i < n; ++i)
        for (int r = 0; r < static_cast<int>(w(i)); ++r, ++c)
            for (int j = 0; j < d; ++j) rep(j, c) = x(j, i);
}

static void gpu()
{
    const int d = 4, n = 1501;
    const Matrix x = blobs(d, n, 7);
    Vector w(n);
    Matrix rep;
    replicated(x, d, n, w, rep);
#ifdef WEIGHTED_EIGEN
    // the Eigen-typed API has the library's initialisers only, and those see points. One cluster: whatever point is drawn, the first
    // update gives the weighted mean -- held against the fit of the replicated sample (a fit that ignored the weights would miss it)
    const int K = 1;
    KMeans weighted(K), other(K), plain(K);
    ASSERT_TRUE(weighted.fit(x, w));
    ASSERT_TRUE(other.fit(rep));
    ASSERT_TRUE(plain.fit(x));
    ASSERT_TRUE(weighted.centroids()(0, 0) != plain.centroids()(0, 0));
    // with every weight 1 the same points are drawn and every sum is the same: the plain fit, bit for bit
    KMeans unit(3), same(3);
    unit.set_seed(9);
    same.set_seed(9);
    unit.fit(x, ones(n));
    same.fit(x);
    for (int k = 0; k < 3; ++k)
        for (int j = 0; j < d; ++j) ASSERT_TRUE(unit.centroids()(j, k) == same.centroids()(j, k));
    ASSERT_TRUE(unit.inertia() == same.inertia());
#else
    const int K = 3;
    Matrix start(d, K);
    for (int k = 0; k < K; ++k)
        for (int j = 0; j < d; ++j) start(j, k) = 8.0 * static_cast<double>((k + j) % 3 - 1) + 0.5;
    KMeans weighted(K), other(K);
    weighted.set_centroids_initialiser(std::make_shared<ml::Clustering::FixedCentroids>(start));
    other.set_centroids_initialiser(std::make_shared<ml::Clustering::FixedCentroids>(start));
    weighted.set_number_initialisations(2);                              // (the winner goes through the weighted assignment)
    other.set_number_initialisations(2);
    ASSERT_TRUE(weighted.fit(x, w));
    ASSERT_TRUE(other.fit(rep));
#endif
    ASSERT_TRUE(weighted.labels().size() == static_cast<std::size_t>(n));   // per point, not per unit of weight
    for (int k = 0; k < K; ++k)
        for (int j = 0; j < d; ++j) ASSERT_TRUE(weighted.centroids()(j, k) == other.centroids()(j, k));
    ASSERT_TRUE(std::fabs(weighted.inertia() - other.inertia()) <= 1e-13 * other.inertia());
    Vector bad = w;
    bad(5) = -1.0;
    ASSERT_THROW(weighted.fit(x, bad), std::invalid_argument);
#ifndef WEIGHTED_EIGEN
    // the same object, unweighted again: the fit of a fresh object with the same settings
    KMeans fresh(K);
    fresh.set_centroids_initialiser(std::make_shared<ml::Clustering::FixedCentroids>(start));
    fresh.set_number_initialisations(2);
    weighted.fit(x);
    fresh.fit(x);
    ASSERT_TRUE(weighted.inertia() == fresh.inertia());
    for (int k = 0; k < K; ++k)
        for (int j = 0; j < d; ++j) ASSERT_TRUE(weighted.centroids()(j, k) == fresh.centroids()(j, k));
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
    std::printf("kmeans_weighted_fit_test: ok (%s)\n", on_gpu ? "gpu" : "host");
    return 0;
}
