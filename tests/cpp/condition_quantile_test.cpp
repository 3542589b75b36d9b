// EM::conditional_cdfs and EM::conditional_quantiles of both C++ surfaces against the C surface: ml::EM (include/ML/EM.hpp; the default
// build of this file) and the Eigen-typed one (include/ML/EigenApi.hpp through include/eigen_api, against tests/cpp/eigen_shim -- a
// stand-in, NOT Eigen; built with -DCONDITION_TEST_EIGEN) give the bits of mlpp_em_conditional_cdfs / mlpp_em_conditional_quantiles on a
// model fitted the same way. The two class families share their names, so one translation unit holds one of them. `host`: what needs no
// device (the model that was never fitted, bad coordinates, bad probabilities, a wrong shape of values); `gpu`: the rest.
#ifdef CONDITION_TEST_EIGEN
#include <Eigen/Core>
#endif

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
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

static Matrix rows_of(const Matrix& x, const std::vector<unsigned int>& coordinates, int n)
{
    Matrix out(static_cast<int>(coordinates.size()), n);
    for (int i = 0; i < n; ++i)
        for (std::size_t c = 0; c < coordinates.size(); ++c) out(static_cast<int>(c), i) = x(static_cast<int>(coordinates[c]), i);
    return out;
}

static void host()
{
    ml::EM em(2);                                              // not fitted: as conditional_means on such a model
    const Matrix two(2, 5), none(0, 5);
    ASSERT_THROW(em.conditional_cdfs({0, 1}, two, none), std::invalid_argument);
    ASSERT_THROW(em.conditional_quantiles({0, 1}, two, {0.5}), std::invalid_argument);
    mlpp_em* h = nullptr;
    ASSERT_TRUE(mlpp_em_create(2, &h) == 0);
    const uint32_t obs[2] = {0, 1};
    const double p[1] = {0.5};
    double out[5];
    ASSERT_TRUE(mlpp_em_conditional_cdfs(h, obs, 2, two.data(), 5, out, out) == MLHIP_E_INVALID_ARGUMENT);
    ASSERT_TRUE(mlpp_em_conditional_quantiles(h, obs, 2, two.data(), 5, p, 1, out) == MLHIP_E_INVALID_ARGUMENT);
    ASSERT_TRUE(mlpp_em_conditional_cdfs(nullptr, obs, 2, two.data(), 5, out, out) == MLHIP_E_INVALID_ARGUMENT);
    ASSERT_TRUE(mlpp_em_conditional_quantiles(nullptr, obs, 2, two.data(), 5, p, 1, out) == MLHIP_E_INVALID_ARGUMENT);
    mlpp_em_destroy(h);

    // two points, two components: the exact fit needs no device. Bad arguments throw before anything else is looked at.
    Matrix pair(3, 2);
    const double values[6] = {0.0, 1.0, 2.0, 3.0, 5.0, 4.0};
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 3; ++j) pair(j, i) = values[3 * i + j];
    ml::EM fitted(2);
    fitted.fit(pair);
    const Matrix one(1, 4), at(2, 4);
    ASSERT_THROW(fitted.conditional_cdfs({}, Matrix(0, 4), Matrix(3, 4)), std::invalid_argument);
    ASSERT_THROW(fitted.conditional_cdfs({0, 1, 2}, Matrix(3, 4), Matrix(0, 4)), std::invalid_argument);
    ASSERT_THROW(fitted.conditional_cdfs({3}, one, at), std::invalid_argument);
    ASSERT_THROW(fitted.conditional_cdfs({1, 1}, Matrix(2, 4), Matrix(1, 4)), std::invalid_argument);
    ASSERT_THROW(fitted.conditional_cdfs({0, 1}, one, Matrix(1, 4)), std::invalid_argument);    // (one row, two coordinates)
    ASSERT_THROW(fitted.conditional_cdfs({0}, one, Matrix(1, 4)), std::invalid_argument);       // (values: one row, two missing coordinates)
    ASSERT_THROW(fitted.conditional_cdfs({0}, one, Matrix(2, 3)), std::invalid_argument);       // (values: three columns, four points)
    ASSERT_THROW(fitted.conditional_quantiles({3}, one, {0.5}), std::invalid_argument);
    ASSERT_THROW(fitted.conditional_quantiles({0, 1}, one, {0.5}), std::invalid_argument);
    ASSERT_THROW(fitted.conditional_quantiles({0}, one, {0.5, 0.0}), std::invalid_argument);
    ASSERT_THROW(fitted.conditional_quantiles({0}, one, {1.0}), std::invalid_argument);
    ASSERT_THROW(fitted.conditional_quantiles({0}, one, {-0.25}), std::invalid_argument);
    ASSERT_THROW(fitted.conditional_quantiles({0}, one, {std::numeric_limits<double>::quiet_NaN()}), std::invalid_argument);
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

    const std::vector<unsigned int> observed = {3, 0, 4}, missing = {1, 2};
    const int dM = d - static_cast<int>(observed.size());
    const Matrix fresh = blobs(d, m, 8);
    const Matrix x_o = rows_of(fresh, observed, m), x_m = rows_of(fresh, missing, m);
    const std::vector<double> p = {0.05, 0.5, 0.95};
    const int P = static_cast<int>(p.size());
    std::vector<double> want_cdf(static_cast<std::size_t>(m) * dM), want_q(static_cast<std::size_t>(P) * m * dM), y(want_cdf.size());
    ASSERT_TRUE(mlpp_em_conditional_cdfs(h, observed.data(), 3, x_o.data(), m, x_m.data(), want_cdf.data()) == 0);
    ASSERT_TRUE(mlpp_em_conditional_quantiles(h, observed.data(), 3, x_o.data(), m, p.data(), p.size(), want_q.data()) == 0);
    ASSERT_TRUE(mlpp_em_conditional_means(h, observed.data(), 3, x_o.data(), m, y.data(), nullptr) == 0);

    const Matrix F = em.conditional_cdfs(observed, x_o, x_m);
    ASSERT_TRUE(F.rows() == dM && F.cols() == m);
    ASSERT_TRUE(std::memcmp(F.data(), want_cdf.data(), sizeof(double) * want_cdf.size()) == 0);
    const Matrix q = em.conditional_quantiles(observed, x_o, p);
    ASSERT_TRUE(q.rows() == dM && q.cols() == static_cast<long>(P) * m);
    ASSERT_TRUE(std::memcmp(q.data(), want_q.data(), sizeof(double) * want_q.size()) == 0);
    bool inside = true, ordered = true;
    for (int i = 0; i < m; ++i)
        for (int j = 0; j < dM; ++j) {
            inside = inside && F(j, i) > 0.0 && F(j, i) < 1.0;
            ordered = ordered && q(j, i) < q(j, m + i) && q(j, m + i) < q(j, 2 * m + i) && std::isfinite(q(j, i)) && std::isfinite(q(j, 2 * m + i));
        }
    ASSERT_TRUE(inside);
    ASSERT_TRUE(ordered);
    // the CDF at the median is a half
    Matrix median(dM, m);
    for (int i = 0; i < m; ++i)
        for (int j = 0; j < dM; ++j) median(j, i) = q(j, m + i);
    const Matrix half = em.conditional_cdfs(observed, x_o, median);
    bool halves = true;
    for (int i = 0; i < m; ++i)
        for (int j = 0; j < dM; ++j) halves = halves && std::fabs(half(j, i) - 0.5) <= 1e-12;
    ASSERT_TRUE(halves);

    const Matrix none(3, 0);
    ASSERT_TRUE(em.conditional_cdfs(observed, none, Matrix(dM, 0)).cols() == 0);
    const Matrix empty = em.conditional_quantiles(observed, none, p);
    ASSERT_TRUE(empty.rows() == dM && empty.cols() == 0);
    ASSERT_TRUE(em.conditional_quantiles(observed, x_o, {}).cols() == 0);
    ASSERT_TRUE(mlpp_em_conditional_cdfs(h, observed.data(), 3, nullptr, 0, nullptr, nullptr) == 0);
    ASSERT_TRUE(mlpp_em_conditional_quantiles(h, observed.data(), 3, nullptr, 0, p.data(), p.size(), nullptr) == 0);
    ASSERT_THROW(em.conditional_cdfs(observed, Matrix(2, 4), Matrix(dM, 4)), std::invalid_argument);
    ASSERT_THROW(em.conditional_quantiles({0, 5, 1}, x_o, p), std::invalid_argument);
    mlpp_em_destroy(h);
}

int main(int argc, char** argv)
{
    const bool on_gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    host();
    if (on_gpu) gpu();
    std::printf("condition_quantile_test %s: %d failure(s)\n", on_gpu ? "gpu" : "host", failures);
    return failures ? 1 : 0;
}
