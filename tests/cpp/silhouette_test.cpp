// Clustering::silhouette_samples / silhouette_score and EM::number_parameters / bic / aic of both C++ surfaces against the C surface:
// the functions of include/ML/Clustering.hpp and include/ML/EM.hpp (the default build of this file) and the Eigen-typed ones
// (include/ML/EigenApi.hpp through include/eigen_api, against tests/cpp/eigen_shim -- a stand-in, NOT Eigen; built with
// -DSILHOUETTE_TEST_EIGEN) give the bits of mlpp_silhouette_samples, and the criteria the bits of their formulas on
// mean_log_density. The two class families share their names, so one translation unit holds one of them. `host`: what needs no
// device (argument errors, the parameter count of an exact fit); `gpu`: the rest.
#ifdef SILHOUETTE_TEST_EIGEN
#include <Eigen/Core>
#endif

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <stdexcept>
#include <vector>

#include "ML/Clustering.hpp"
#include "ML/EM.hpp"
#include "mlhip.h"
#include "mlpp_c.h"

#ifdef SILHOUETTE_TEST_EIGEN
#ifndef MLHIP_ML_EIGEN_API_HPP
#error "include/eigen_api must precede include/ on the include path"
#endif
using Matrix = Eigen::MatrixXd;
using RowIndex = Eigen::Index;
#else
using Matrix = ml::MatrixXd;
using RowIndex = ml::Index;
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
        for (int j = 0; j < d; ++j) x(j, i) = g(rng) + 5.0 * static_cast<double>((i % 3 + j) % 3);
    return x;
}

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

static void host()
{
    const Matrix x = blobs(3, 6, 1);
    const std::vector<unsigned int> good = {0, 1, 0, 1, 0, 1};
    ASSERT_THROW(ml::Clustering::silhouette_samples(x, {0, 1, 0}), std::invalid_argument);                     // one label per point
    ASSERT_THROW(ml::Clustering::silhouette_samples(x, {2, 2, 2, 2, 2, 2}), std::invalid_argument);            // one non-empty cluster
    ASSERT_THROW(ml::Clustering::silhouette_samples(x, good, std::vector<RowIndex>{6}), std::invalid_argument);
    ASSERT_THROW(ml::Clustering::silhouette_samples(x, good, std::vector<RowIndex>{-1}), std::invalid_argument);
    ASSERT_THROW(ml::Clustering::silhouette_score(x, {0, 1, 0}), std::invalid_argument);
    double out[6];
    const uint32_t labels[6] = {0, 1, 0, 1, 0, 1};
    const uint64_t far[1] = {6};
    ASSERT_TRUE(mlpp_silhouette_samples(nullptr, 6, 3, labels, 2, nullptr, 0, out) == MLHIP_E_INVALID_ARGUMENT);
    ASSERT_TRUE(mlpp_silhouette_samples(x.data(), 6, 3, nullptr, 2, nullptr, 0, out) == MLHIP_E_INVALID_ARGUMENT);
    ASSERT_TRUE(mlpp_silhouette_samples(x.data(), 6, 3, labels, 2, nullptr, 0, nullptr) == MLHIP_E_INVALID_ARGUMENT);
    ASSERT_TRUE(mlpp_silhouette_samples(x.data(), 6, 3, labels, 1, nullptr, 0, out) == MLHIP_E_INVALID_ARGUMENT);   // a label >= K
    ASSERT_TRUE(mlpp_silhouette_samples(x.data(), 6, 3, labels, 2, far, 1, out) == MLHIP_E_INVALID_ARGUMENT);

    // the parameter count: an unfitted model throws; the exact fit (N == K) needs no device
    ml::EM em(2);
    ASSERT_THROW(em.number_parameters(), std::invalid_argument);
    ASSERT_THROW(em.bic(x), std::invalid_argument);
    ASSERT_THROW(em.aic(x), std::invalid_argument);
    Matrix pair(3, 2);
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 3; ++j) pair(j, i) = static_cast<double>(3 * i + j * j);
    em.fit(pair);
    ASSERT_TRUE(em.number_parameters() == 2 * 6 + 2 * 3 + 1);
    mlpp_em* h = nullptr;
    uint64_t p = 0;
    ASSERT_TRUE(mlpp_em_create(2, &h) == 0);
    ASSERT_TRUE(mlpp_em_number_parameters(h, &p) == MLHIP_E_INVALID_ARGUMENT);
    ASSERT_TRUE(mlpp_em_number_parameters(h, nullptr) == MLHIP_E_INVALID_ARGUMENT);
    mlpp_em_destroy(h);
}

static void gpu()
{
    const int d = 5, n = 700;
    const Matrix x = blobs(d, n, 2);
    std::vector<unsigned int> labels(n);
    for (int i = 0; i < n; ++i) labels[static_cast<std::size_t>(i)] = static_cast<unsigned int>(i % 3);
    const auto s = ml::Clustering::silhouette_samples(x, labels);
    ASSERT_TRUE(s.size() == n);
    std::vector<double> c(n);
    ASSERT_TRUE(mlpp_silhouette_samples(x.data(), n, d, labels.data(), 3, nullptr, 0, c.data()) == 0);
    double sum = 0;
    bool equal = true, sensible = true;
    for (int i = 0; i < n; ++i) {
        equal = equal && same_bits(s[i], c[static_cast<std::size_t>(i)]);
        sensible = sensible && s[i] > 0.3 && s[i] <= 1.0;      // three blobs 5 apart, unit noise
        sum += s[i];
    }
    ASSERT_TRUE(equal);
    ASSERT_TRUE(sensible);
    ASSERT_TRUE(same_bits(ml::Clustering::silhouette_score(x, labels), sum / n));
    const std::vector<RowIndex> rows = {699, 3, 3};
    const auto part = ml::Clustering::silhouette_samples(x, labels, rows);
    ASSERT_TRUE(part.size() == 3 && same_bits(part[0], s[699]) && same_bits(part[1], s[3]) && same_bits(part[2], s[3]));
    ASSERT_TRUE(same_bits(ml::Clustering::silhouette_score(x, labels, rows), (s[699] + s[3] + s[3]) / 3.0));

    ml::EM em(3);
    em.set_seed(4);
    em.fit(x);
    const double p = static_cast<double>(em.number_parameters()), score = em.mean_log_density(x), nn = static_cast<double>(n);
    ASSERT_TRUE(em.number_parameters() == 3 * 15 + 3 * 5 + 2);
    ASSERT_TRUE(same_bits(em.bic(x), -2.0 * nn * score + p * std::log(nn)));
    ASSERT_TRUE(same_bits(em.aic(x), -2.0 * nn * score + 2.0 * p));
}

int main(int argc, char** argv)
{
    const bool on_gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    if (on_gpu) gpu(); else host();
    if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
    std::printf("silhouette_test %s: ok\n", on_gpu ? "gpu" : "host");
    return 0;
}
