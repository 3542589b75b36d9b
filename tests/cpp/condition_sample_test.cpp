// EM::conditional_samples / EM::conditional_covariances of both C++ surfaces against the C surface: ml::EM (include/ML/EM.hpp; the
// default build of this file) and the Eigen-typed one (include/ML/EigenApi.hpp through include/eigen_api, against
// tests/cpp/eigen_shim -- a stand-in, NOT Eigen; built with -DCONDITION_TEST_EIGEN) give the bits of mlpp_em_conditional_samples and
// mlpp_em_conditional_covariances on a model fitted the same way, and those of the C ABI call mlhip_em_conditional_samples on the
// parameters the model reports. `host`: what needs no device; `gpu`: the rest.
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
    ml::EM em(2);                                              // not fitted
    const Matrix two(2, 5);
    ASSERT_THROW(em.conditional_samples({0, 1}, two, 1), std::invalid_argument);
    ASSERT_THROW(em.conditional_covariances({0}), std::invalid_argument);
    mlpp_em* h = nullptr;
    ASSERT_TRUE(mlpp_em_create(2, &h) == 0);
    const uint32_t obs[2] = {0, 1};
    double out[5];
    ASSERT_TRUE(mlpp_em_conditional_samples(h, obs, 2, two.data(), 5, 1, 0, out, nullptr) == MLHIP_E_INVALID_ARGUMENT);
    ASSERT_TRUE(mlpp_em_conditional_samples(nullptr, obs, 2, two.data(), 5, 1, 0, out, nullptr) == MLHIP_E_INVALID_ARGUMENT);
    ASSERT_TRUE(mlpp_em_conditional_covariances(h, obs, 1, out) == MLHIP_E_INVALID_ARGUMENT);
    mlpp_em_destroy(h);

    // mlhip_em_condition_covariances in closed form: Sigma = [[2, 1, 0], [1, 2, 0], [0, 0, 1]], O = {1}: C = [[1.5, 0], [0, 1]]
    const double cov[9] = {2, 1, 0, 1, 2, 0, 0, 0, 1};
    const uint32_t one[1] = {1};
    double c[4], g[4];
    ASSERT_TRUE(mlhip_em_condition_covariances(3, 1, MLHIP_COVARIANCE_FULL, cov, one, 1, c, g) == MLHIP_OK);
    ASSERT_TRUE(std::fabs(c[0] - 1.5) <= 1e-15 && c[1] == 0.0 && c[2] == 0.0 && c[3] == 1.0);
    ASSERT_TRUE(std::fabs(g[0] - std::sqrt(1.5)) <= 1e-15 && g[1] == 0.0 && g[2] == 0.0 && g[3] == 1.0);
    const uint32_t twice[2] = {1, 1};
    ASSERT_TRUE(mlhip_em_condition_covariances(3, 1, MLHIP_COVARIANCE_FULL, cov, twice, 2, c, g) == MLHIP_E_INVALID_ARGUMENT);
    const double indefinite[9] = {1, 2, 0, 2, 1, 0, 0, 0, 1};
    const uint32_t first[1] = {0};
    ASSERT_TRUE(mlhip_em_condition_covariances(3, 1, MLHIP_COVARIANCE_FULL, indefinite, first, 1, c, g) == MLHIP_E_DOMAIN);
}

static void gpu()
{
    const int d = 5, K = 3, n = 3001, m = 1777, draws = 3;
    const std::uint64_t seed = 11;
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
    std::vector<double> want(static_cast<std::size_t>(draws) * m * dM);
    std::vector<uint32_t> want_labels(static_cast<std::size_t>(draws) * m);
    ASSERT_TRUE(mlpp_em_conditional_samples(h, observed.data(), 3, x_o.data(), m, draws, seed, want.data(), want_labels.data()) == 0);

    std::vector<unsigned int> labels;
    const Matrix x = em.conditional_samples(observed, x_o, draws, seed, &labels);
    ASSERT_TRUE(x.rows() == dM && x.cols() == draws * m && labels.size() == want_labels.size());
    ASSERT_TRUE(std::memcmp(x.data(), want.data(), sizeof(double) * want.size()) == 0);
    ASSERT_TRUE(std::memcmp(labels.data(), want_labels.data(), sizeof(uint32_t) * want_labels.size()) == 0);
    const Matrix without = em.conditional_samples(observed, x_o, draws, seed);
    ASSERT_TRUE(std::memcmp(without.data(), want.data(), sizeof(double) * want.size()) == 0);
    const Matrix first = em.conditional_samples(observed, x_o, 1, seed);
    ASSERT_TRUE(std::memcmp(first.data(), want.data(), sizeof(double) * m * dM) == 0);
    bool finite = true, in_range = true;
    for (std::size_t i = 0; i < want.size(); ++i) finite = finite && std::isfinite(want[i]);
    for (std::size_t i = 0; i < want_labels.size(); ++i) in_range = in_range && want_labels[i] < static_cast<uint32_t>(K);
    ASSERT_TRUE(finite && in_range);

    // the covariances: both surfaces, and the C ABI call on the model's parameters
    std::vector<double> want_c(static_cast<std::size_t>(K) * dM * dM);
    ASSERT_TRUE(mlpp_em_conditional_covariances(h, observed.data(), 3, want_c.data()) == 0);
    const std::vector<Matrix> c = em.conditional_covariances(observed);
    ASSERT_TRUE(static_cast<int>(c.size()) == K);
    for (int k = 0; k < K && k < static_cast<int>(c.size()); ++k)
        ASSERT_TRUE(c[k].rows() == dM && c[k].cols() == dM && std::memcmp(c[k].data(), want_c.data() + static_cast<std::size_t>(k) * dM * dM, sizeof(double) * dM * dM) == 0);

    const Matrix none(3, 0);
    const Matrix empty = em.conditional_samples(observed, none, draws, seed);
    ASSERT_TRUE(empty.rows() == dM && empty.cols() == 0);
    const Matrix no_draws = em.conditional_samples(observed, x_o, 0, seed);
    ASSERT_TRUE(no_draws.rows() == dM && no_draws.cols() == 0);
    ASSERT_TRUE(mlpp_em_conditional_samples(h, observed.data(), 3, nullptr, 0, draws, seed, nullptr, nullptr) == 0);

    const Matrix wrong(2, 4);
    ASSERT_THROW(em.conditional_samples(observed, wrong, 1), std::invalid_argument);
    ASSERT_THROW(em.conditional_samples({}, none, 1), std::invalid_argument);
    ASSERT_THROW(em.conditional_samples({0, 5, 1}, x_o, 1), std::invalid_argument);
    ASSERT_THROW(em.conditional_samples({0, 1, 1}, x_o, 1), std::invalid_argument);
    ASSERT_THROW(em.conditional_samples(observed, x_o, -1), std::invalid_argument);
    ASSERT_THROW(em.conditional_covariances({0, 1, 2, 3, 4}), std::invalid_argument);
    mlpp_em_destroy(h);
}

int main(int argc, char** argv)
{
    const bool on_gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    host();
    if (on_gpu) gpu();
    std::printf("condition_sample_test %s: %d failure(s)\n", on_gpu ? "gpu" : "host", failures);
    return failures ? 1 : 0;
}
