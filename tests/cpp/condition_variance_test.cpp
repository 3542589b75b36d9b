// EM::conditional_variances of both C++ surfaces against the C surface: ml::EM::conditional_variances (include/ML/EM.hpp; the default
// build of this file) and the Eigen-typed one (include/ML/EigenApi.hpp through include/eigen_api, against tests/cpp/eigen_shim -- a
// stand-in, NOT Eigen; built with -DCONDITION_TEST_EIGEN) give the bits of mlpp_em_conditional_variances on a model fitted the same
// way, in both forms, and their mean the bits of conditional_means. The two class families share their names, so one translation unit
// holds one of them. `host`: what needs no device (the model that was never fitted, bad coordinates); `gpu`: the rest.
#ifdef CONDITION_TEST_EIGEN
#include <Eigen/Core>
#endif

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <stdexcept>
#include <vector>

#include "ML/EM.hpp"
#include "mlhip.h"
#include "mlpp_c.h"

#ifdef CONDITION_TEST_EIGEN
#ifndef MLHIP_ML_EIGEN_API_HPP
#error "include/eigen_api must precede include/ on the include path"
#endif
using Matrix = Eigen::MatrixXd;
#else
using Matrix = ml::MatrixXd;
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
    for (int i = 0; i < n; ++i) {
        const double common = g(rng);                          // (correlated coordinates: the maps are not zero)
        for (int j = 0; j < d; ++j) x(j, i) = g(rng) + 0.7 * common + 4.0 * static_cast<double>((i + j) % 3) + 2.0;
    }
    return x;
}

static Matrix rows_of(const Matrix& x, const std::vector<unsigned int>& observed, int n)
{
    Matrix out(static_cast<int>(observed.size()), n);
    for (int i = 0; i < n; ++i)
        for (std::size_t c = 0; c < observed.size(); ++c) out(static_cast<int>(c), i) = x(static_cast<int>(observed[c]), i);
    return out;
}

static void host()
{
    ml::EM em(2);                                              // not fitted: as conditional_means on such a model
    const Matrix two(2, 5);
    ASSERT_THROW(em.conditional_variances({0, 1}, two), std::invalid_argument);
    ASSERT_THROW(em.conditional_variances({0, 1}, two, true), std::invalid_argument);
    mlpp_em* h = nullptr;
    ASSERT_TRUE(mlpp_em_create(2, &h) == 0);
    const uint32_t obs[2] = {0, 1};
    double out[5];
    ASSERT_TRUE(mlpp_em_conditional_variances(h, obs, 2, two.data(), 5, 0, out, nullptr) == MLHIP_E_INVALID_ARGUMENT);
    ASSERT_TRUE(mlpp_em_conditional_variances(nullptr, obs, 2, two.data(), 5, 0, out, nullptr) == MLHIP_E_INVALID_ARGUMENT);
    mlpp_em_destroy(h);

    // two points, two components: the exact fit needs no device. Bad coordinates throw before anything else is looked at. (No points:
    // in gpu() -- every call on a model with parameters asks for the device first, as conditional_means does.)
    Matrix pair(3, 2);
    const double values[6] = {0.0, 1.0, 2.0, 3.0, 5.0, 4.0};
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 3; ++j) pair(j, i) = values[3 * i + j];
    ml::EM fitted(2);
    fitted.fit(pair);
    const Matrix one(1, 4);
    ASSERT_THROW(fitted.conditional_variances({}, Matrix(0, 4)), std::invalid_argument);
    ASSERT_THROW(fitted.conditional_variances({0, 1, 2}, Matrix(3, 4)), std::invalid_argument);
    ASSERT_THROW(fitted.conditional_variances({3}, one), std::invalid_argument);
    ASSERT_THROW(fitted.conditional_variances({1, 1}, Matrix(2, 4)), std::invalid_argument);
    ASSERT_THROW(fitted.conditional_variances({0, 1}, one), std::invalid_argument);   // (one row, two coordinates)
}

static void gpu()
{
    const int d = 5, K = 3, n = 3001, m = 1777;
    const Matrix train = blobs(d, n, 7);
    ml::EM em(K);
    em.set_seed(3);
    em.fit(train);
    mlpp_em* h = nullptr;
    int converged = 0;
    ASSERT_TRUE(mlpp_em_create(K, &h) == 0 && mlpp_em_set_seed(h, 3) == 0);
    ASSERT_TRUE(mlpp_em_fit(h, train.data(), n, d, &converged) == 0);

    const std::vector<unsigned int> observed = {3, 0, 4};
    const int dM = d - static_cast<int>(observed.size());
    const Matrix x_o = rows_of(blobs(d, m, 8), observed, m);
    std::vector<double> want(static_cast<std::size_t>(m) * dM), want_full(static_cast<std::size_t>(m) * dM * dM), want_means(want.size()),
        plain_means(want.size());
    ASSERT_TRUE(mlpp_em_conditional_variances(h, observed.data(), 3, x_o.data(), m, 0, want.data(), want_means.data()) == 0);
    ASSERT_TRUE(mlpp_em_conditional_variances(h, observed.data(), 3, x_o.data(), m, 1, want_full.data(), nullptr) == 0);
    ASSERT_TRUE(mlpp_em_conditional_means(h, observed.data(), 3, x_o.data(), m, plain_means.data(), nullptr) == 0);
    ASSERT_TRUE(std::memcmp(want_means.data(), plain_means.data(), sizeof(double) * want.size()) == 0);

    Matrix means;
    const Matrix v = em.conditional_variances(observed, x_o, false, &means);
    ASSERT_TRUE(v.rows() == dM && v.cols() == m && means.rows() == dM && means.cols() == m);
    ASSERT_TRUE(std::memcmp(v.data(), want.data(), sizeof(double) * want.size()) == 0);
    ASSERT_TRUE(std::memcmp(means.data(), want_means.data(), sizeof(double) * want.size()) == 0);
    const Matrix y = em.conditional_means(observed, x_o);
    ASSERT_TRUE(std::memcmp(y.data(), want_means.data(), sizeof(double) * want.size()) == 0);
    const Matrix full = em.conditional_variances(observed, x_o, true);
    ASSERT_TRUE(full.rows() == dM * dM && full.cols() == m);
    ASSERT_TRUE(std::memcmp(full.data(), want_full.data(), sizeof(double) * want_full.size()) == 0);
    bool positive = true, diagonal = true;
    for (int i = 0; i < m; ++i)
        for (int j = 0; j < dM; ++j) {
            positive = positive && v(j, i) > 0.0 && std::isfinite(v(j, i));
            const double on_diagonal = full(j * dM + j, i), alone = v(j, i);
            diagonal = diagonal && std::memcmp(&on_diagonal, &alone, sizeof(double)) == 0;
        }
    ASSERT_TRUE(positive);
    ASSERT_TRUE(diagonal);

    const Matrix none(3, 0);
    const Matrix empty = em.conditional_variances(observed, none, true);
    ASSERT_TRUE(empty.rows() == dM * dM && empty.cols() == 0);
    ASSERT_TRUE(mlpp_em_conditional_variances(h, observed.data(), 3, nullptr, 0, 0, nullptr, nullptr) == 0);
    ASSERT_THROW(em.conditional_variances(observed, Matrix(2, 4)), std::invalid_argument);
    ASSERT_THROW(em.conditional_variances({0, 5, 1}, x_o), std::invalid_argument);
    mlpp_em_destroy(h);
}

int main(int argc, char** argv)
{
    const bool on_gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    host();
    if (on_gpu) gpu();
    std::printf("condition_variance_test %s: %d failure(s)\n", on_gpu ? "gpu" : "host", failures);
    return failures ? 1 : 0;
}
