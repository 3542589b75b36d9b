// EM::conditional_means of both C++ surfaces against the C surface: ml::EM::conditional_means (include/ML/EM.hpp; the default build
// of this file) and the Eigen-typed one (include/ML/EigenApi.hpp through include/eigen_api, against tests/cpp/eigen_shim -- a
// stand-in, NOT Eigen; built with -DCONDITION_TEST_EIGEN) give the bits of mlpp_em_conditional_means on a model fitted the same way,
// and the affine map of mlhip_em_condition at K = 1. The two class families share their names, so one translation unit holds one of
// them. `host`: what needs no device (the model that was never fitted, mlhip_em_condition itself); `gpu`: the rest.
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
    ml::EM em(2);                                              // not fitted: as sample on such a model
    const Matrix two(2, 5);
    ASSERT_THROW(em.conditional_means({0, 1}, two), std::invalid_argument);
    mlpp_em* h = nullptr;
    ASSERT_TRUE(mlpp_em_create(2, &h) == 0);
    const uint32_t obs[2] = {0, 1};
    double out[5];
    ASSERT_TRUE(mlpp_em_conditional_means(h, obs, 2, two.data(), 5, out, nullptr) == MLHIP_E_INVALID_ARGUMENT);
    ASSERT_TRUE(mlpp_em_conditional_means(nullptr, obs, 2, two.data(), 5, out, nullptr) == MLHIP_E_INVALID_ARGUMENT);
    mlpp_em_destroy(h);

    // mlhip_em_condition on a 3 x 3 model whose answer is known in closed form: Sigma = [[2, 1, 0], [1, 2, 0], [0, 0, 1]], O = {1}
    const double mean[3] = {1.0, 2.0, 3.0};
    const double cov[9] = {2, 1, 0, 1, 2, 0, 0, 0, 1};
    const uint32_t one[1] = {1};
    double mu_o[1], s_oo[1], maps[2], mu_m[2];
    ASSERT_TRUE(mlhip_em_condition(3, 1, MLHIP_COVARIANCE_FULL, mean, cov, one, 1, mu_o, s_oo, maps, mu_m) == MLHIP_OK);
    ASSERT_TRUE(mu_o[0] == 2.0 && s_oo[0] == 2.0 && mu_m[0] == 1.0 && mu_m[1] == 3.0);
    ASSERT_TRUE(std::fabs(maps[0] - 0.5) <= 1e-15 && maps[1] == 0.0);
    const uint32_t twice[2] = {1, 1};
    ASSERT_TRUE(mlhip_em_condition(3, 1, MLHIP_COVARIANCE_FULL, mean, cov, twice, 2, mu_o, s_oo, maps, mu_m) == MLHIP_E_INVALID_ARGUMENT);
    const double indefinite[9] = {1, 2, 0, 2, 1, 0, 0, 0, 1};
    const uint32_t pair[2] = {0, 1};
    double mu_o2[2], s_oo2[4], maps2[2], mu_m2[1];
    ASSERT_TRUE(mlhip_em_condition(3, 1, MLHIP_COVARIANCE_FULL, mean, indefinite, pair, 2, mu_o2, s_oo2, maps2, mu_m2) == MLHIP_E_DOMAIN);
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
    std::vector<double> want(static_cast<std::size_t>(m) * dM), want_density(m);
    ASSERT_TRUE(mlpp_em_conditional_means(h, observed.data(), 3, x_o.data(), m, want.data(), want_density.data()) == 0);

    std::vector<double> density(m);
    const Matrix y = em.conditional_means(observed, x_o, density.data());
    ASSERT_TRUE(y.rows() == dM && y.cols() == m);
    ASSERT_TRUE(std::memcmp(y.data(), want.data(), sizeof(double) * want.size()) == 0);
    ASSERT_TRUE(std::memcmp(density.data(), want_density.data(), sizeof(double) * want_density.size()) == 0);
    const Matrix without = em.conditional_means(observed, x_o);
    ASSERT_TRUE(std::memcmp(without.data(), want.data(), sizeof(double) * want.size()) == 0);
    bool finite = true;
    for (std::size_t i = 0; i < want.size(); ++i) finite = finite && std::isfinite(want[i]);
    ASSERT_TRUE(finite);

    const Matrix none(3, 0);
    const Matrix empty = em.conditional_means(observed, none);
    ASSERT_TRUE(empty.rows() == dM && empty.cols() == 0);
    ASSERT_TRUE(mlpp_em_conditional_means(h, observed.data(), 3, nullptr, 0, nullptr, nullptr) == 0);

    const Matrix wrong(2, 4);
    ASSERT_THROW(em.conditional_means(observed, wrong), std::invalid_argument);
    ASSERT_THROW(em.conditional_means({}, none), std::invalid_argument);
    ASSERT_THROW(em.conditional_means({0, 1, 2, 3, 4}, Matrix(5, 2)), std::invalid_argument);
    ASSERT_THROW(em.conditional_means({0, 5, 1}, x_o), std::invalid_argument);
    ASSERT_THROW(em.conditional_means({0, 1, 1}, x_o), std::invalid_argument);
    mlpp_em_destroy(h);
}

int main(int argc, char** argv)
{
    const bool on_gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    host();
    if (on_gpu) gpu();
    std::printf("condition_test %s: %d failure(s)\n", on_gpu ? "gpu" : "host", failures);
    return failures ? 1 : 0;
}
