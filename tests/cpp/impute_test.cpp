// EM::impute of both C++ surfaces against the C surface: ml::EM::impute (include/ML/EM.hpp; the default build of this file) and the
// Eigen-typed one (include/ML/EigenApi.hpp through include/eigen_api, against tests/cpp/eigen_shim -- a stand-in, NOT Eigen; built
// with -DIMPUTE_TEST_EIGEN) give the bits of mlpp_em_impute on a model fitted the same way: imputed block, log-densities and
// responsibilities; observed entries keep their bits, complete points come back as they are. The two class families share their
// names, so one translation unit holds one of them. `host`: what needs no device (the model that was never fitted, null handles,
// mlhip_em_impute_plan and mlhip_em_impute_route); `gpu`: the rest.
#ifdef IMPUTE_TEST_EIGEN
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

#ifdef IMPUTE_TEST_EIGEN
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

static const double kNaN = std::numeric_limits<double>::quiet_NaN();

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

static void host()
{
    ml::EM em(2);                                              // not fitted
    const Matrix two(2, 5);
    ASSERT_THROW(em.impute(two), std::invalid_argument);
    mlpp_em* h = nullptr;
    ASSERT_TRUE(mlpp_em_create(2, &h) == 0);
    double out[10];
    ASSERT_TRUE(mlpp_em_impute(h, two.data(), 5, 2, out, nullptr, nullptr) == MLHIP_E_INVALID_ARGUMENT);
    ASSERT_TRUE(mlpp_em_impute(nullptr, two.data(), 5, 2, out, nullptr, nullptr) == MLHIP_E_INVALID_ARGUMENT);
    mlpp_em_destroy(h);

    // the plan of a block whose grouping is known: rows 0 and 2 miss coordinate 1, row 1 is complete, row 3 is all NaN
    const double x[8] = {1.0, kNaN, 2.0, 3.0, 4.0, kNaN, kNaN, kNaN};
    uint32_t patterns = 0, order[4], bounds[5], n_observed[4];
    ASSERT_TRUE(mlhip_em_impute_plan(x, 4, 2, &patterns, order, bounds, n_observed) == MLHIP_OK);
    ASSERT_TRUE(patterns == 3 && order[0] == 3 && order[1] == 0 && order[2] == 2 && order[3] == 1);
    ASSERT_TRUE(bounds[0] == 0 && bounds[1] == 1 && bounds[2] == 3 && bounds[3] == 4);
    ASSERT_TRUE(n_observed[0] == 0 && n_observed[1] == 1 && n_observed[2] == 2);
    ASSERT_TRUE(mlhip_em_impute_plan(x, 4, 2, nullptr, order, bounds, n_observed) == MLHIP_E_INVALID_ARGUMENT);
    int route = -1;
    uint64_t launches = 0;
    ASSERT_TRUE(mlhip_em_impute_route(2, 3, x, 4, &route, &launches) == MLHIP_OK && route == MLHIP_IMPUTE_KERNEL && launches == 3);
    ASSERT_TRUE(mlhip_em_impute_route(33, 3, nullptr, 0, &route, nullptr) == MLHIP_OK && route == MLHIP_IMPUTE_COMPOSED);
    ASSERT_TRUE(mlhip_em_impute(nullptr, 2, 3, MLHIP_COVARIANCE_FULL, x, x, x, x, 4, out, nullptr, nullptr) == MLHIP_E_INVALID_ARGUMENT);
}

static void gpu()
{
    const int d = 5, K = 3, n = 3001, m = 777;
    const Matrix train = blobs(d, n, 7);
    ml::EM em(K);
    em.set_seed(3);
    em.fit(train);
    mlpp_em* h = nullptr;
    int converged = 0;
    ASSERT_TRUE(mlpp_em_create(K, &h) == 0 && mlpp_em_set_seed(h, 3) == 0);
    ASSERT_TRUE(mlpp_em_fit(h, train.data(), n, d, &converged) == 0);

    Matrix x = blobs(d, m, 8);
    std::mt19937_64 rng(9);
    for (int i = 3; i < m; ++i)                                 // (points 0 - 2 complete, point 3 all NaN)
        for (int j = 0; j < d; ++j)
            if (i == 3 || rng() % 10 < 3) x(j, i) = kNaN;
    std::vector<double> want(static_cast<std::size_t>(m) * d), want_density(m), want_shares(static_cast<std::size_t>(m) * K);
    ASSERT_TRUE(mlpp_em_impute(h, x.data(), m, d, want.data(), want_density.data(), want_shares.data()) == 0);

    std::vector<double> density(m);
    Matrix shares;
    const Matrix y = em.impute(x, density.data(), &shares);
    ASSERT_TRUE(y.rows() == d && y.cols() == m && shares.rows() == K && shares.cols() == m);
    ASSERT_TRUE(std::memcmp(y.data(), want.data(), sizeof(double) * want.size()) == 0);
    ASSERT_TRUE(std::memcmp(density.data(), want_density.data(), sizeof(double) * want_density.size()) == 0);
    ASSERT_TRUE(std::memcmp(shares.data(), want_shares.data(), sizeof(double) * want_shares.size()) == 0);
    const Matrix without = em.impute(x);
    ASSERT_TRUE(std::memcmp(without.data(), want.data(), sizeof(double) * want.size()) == 0);
    bool kept = true, finite = true;
    for (int i = 0; i < m; ++i)
        for (int j = 0; j < d; ++j) {
            finite = finite && std::isfinite(y(j, i));
            const double was = x(j, i), is = y(j, i);
            if (!std::isnan(was)) kept = kept && std::memcmp(&was, &is, sizeof(double)) == 0;
        }
    ASSERT_TRUE(kept && finite);
    double sum = 0;
    for (int k = 0; k < K; ++k) sum += shares(k, 10);
    ASSERT_TRUE(std::fabs(sum - 1.0) <= 1e-12 && want_density[3] == 0.0);

    const Matrix none(d, 0);
    const Matrix empty = em.impute(none);
    ASSERT_TRUE(empty.rows() == d && empty.cols() == 0);
    ASSERT_TRUE(mlpp_em_impute(h, nullptr, 0, d, nullptr, nullptr, nullptr) == 0);
    ASSERT_THROW(em.impute(Matrix(4, 3)), std::invalid_argument);
    mlpp_em_destroy(h);
}

int main(int argc, char** argv)
{
    const bool on_gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    host();
    if (on_gpu) gpu();
    std::printf("impute_test %s: %d failure(s)\n", on_gpu ? "gpu" : "host", failures);
    return failures ? 1 : 0;
}
