// EM::sample of both C++ surfaces against the C surface: ml::EM::sample (include/ML/EM.hpp; the default build of this file) and the
// Eigen-typed ml::EM::sample (include/ML/EigenApi.hpp through include/eigen_api, against tests/cpp/eigen_shim -- a stand-in, NOT
// Eigen; built with -DSAMPLE_TEST_EIGEN) give the bits and labels of mlpp_em_sample on a model fitted the same way. The two class
// families share their names, so one translation unit holds one of them. `host`: the model that was never fitted; `gpu`: the rest.
#ifdef SAMPLE_TEST_EIGEN
#include <Eigen/Core>
#endif

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <stdexcept>
#include <vector>

#include "ML/EM.hpp"
#include "mlhip.h"
#include "mlpp_c.h"

#ifdef SAMPLE_TEST_EIGEN
#ifndef MLHIP_ML_EIGEN_API_HPP
#error "include/eigen_api must precede include/ on the include path"
#endif
using Matrix = Eigen::MatrixXd;
using Size = Eigen::Index;
#else
using Matrix = ml::MatrixXd;
using Size = ml::Index;
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
    ml::EM em(2);                                              // not fitted: as the batch queries on such a model
    ASSERT_THROW(em.sample(10), std::invalid_argument);
    ASSERT_THROW(em.sample(-1), std::invalid_argument);
    mlpp_em* h = nullptr;
    ASSERT_TRUE(mlpp_em_create(2, &h) == 0);
    double x[30];
    ASSERT_TRUE(mlpp_em_sample(h, 10, 0, x, nullptr) == MLHIP_E_INVALID_ARGUMENT);
    ASSERT_TRUE(mlpp_em_sample(nullptr, 10, 0, x, nullptr) == MLHIP_E_INVALID_ARGUMENT);
    mlpp_em_destroy(h);
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

    std::vector<double> want(static_cast<std::size_t>(m) * d);
    std::vector<uint32_t> want_labels(m);
    ASSERT_TRUE(mlpp_em_sample(h, m, 42, want.data(), want_labels.data()) == 0);

    std::vector<unsigned int> labels;
    const Matrix x = em.sample(m, 42, &labels);
    ASSERT_TRUE(x.rows() == d && x.cols() == m && labels.size() == static_cast<std::size_t>(m));
    ASSERT_TRUE(std::memcmp(x.data(), want.data(), sizeof(double) * want.size()) == 0);
    bool same_labels = true, in_range = true;
    for (int i = 0; i < m; ++i) {
        same_labels = same_labels && labels[static_cast<std::size_t>(i)] == want_labels[static_cast<std::size_t>(i)];
        in_range = in_range && labels[static_cast<std::size_t>(i)] < static_cast<unsigned int>(K);
    }
    ASSERT_TRUE(same_labels && in_range);

    const Matrix without_labels = em.sample(m, 42);
    ASSERT_TRUE(std::memcmp(without_labels.data(), want.data(), sizeof(double) * want.size()) == 0);
    const Matrix other_seed = em.sample(m, 43);
    ASSERT_TRUE(std::memcmp(other_seed.data(), want.data(), sizeof(double) * want.size()) != 0);
    const Matrix by_default = em.sample(m), seed_zero = em.sample(m, 0);
    ASSERT_TRUE(std::memcmp(by_default.data(), seed_zero.data(), sizeof(double) * want.size()) == 0);

    std::vector<unsigned int> none(3, 7u);
    const Matrix empty = em.sample(0, 42, &none);
    ASSERT_TRUE(empty.rows() == d && empty.cols() == 0 && none.empty());
    ASSERT_TRUE(mlpp_em_sample(h, 0, 42, nullptr, nullptr) == 0);
    ASSERT_THROW(em.sample(static_cast<Size>(-1)), std::invalid_argument);
    // a sample is something fit takes
    ml::EM again(K);
    again.set_seed(1);
    again.fit(x);
    ASSERT_TRUE(again.means().rows() == d);
    mlpp_em_destroy(h);
}

int main(int argc, char** argv)
{
    const bool on_gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    host();
    if (on_gpu) gpu();
    std::printf("sample_test %s: %d failure(s)\n", on_gpu ? "gpu" : "host", failures);
    return failures ? 1 : 0;
}
