// The batch queries of the Eigen-typed, header-only API (include/ML/EigenApi.hpp through include/eigen_api): log_densities,
// mean_log_density, assign_labels, calculate_responsibilities, KMeans::assign_labels with Eigen return types. Built against
// tests/cpp/eigen_shim (a stand-in, NOT Eigen: it shows the call sites are well-formed against the header and the numbers behind
// them right; it proves nothing about real Eigen). `host`: argument errors; `gpu`: against the point queries of the fitted models.
#include <Eigen/Core>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <stdexcept>
#include <vector>

#include "ML/EM.hpp"        // -I include/eigen_api comes first: this is include/ML/EigenApi.hpp
#include "ML/KMeans.hpp"

#ifndef MLHIP_ML_EIGEN_API_HPP
#error "include/eigen_api must precede include/ on the include path"
#endif

static int failures = 0;
#define ASSERT_TRUE(cond) do { if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)
#define ASSERT_THROW(expr, type) do { bool ok_ = false; try { expr; } catch (const type&) { ok_ = true; } catch (...) {} \
    if (!ok_) { std::printf("FAIL %s:%d: %s did not throw %s\n", __FILE__, __LINE__, #expr, #type); ++failures; } } while (0)

static Eigen::MatrixXd blobs(int d, int n, unsigned seed)
{
    std::mt19937_64 rng(seed);
    std::normal_distribution<double> g;
    Eigen::MatrixXd x(d, n);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < d; ++j) x(j, i) = g(rng) + 4.0 * static_cast<double>((i + j) % 3) + 2.0;
    return x;
}

static void host()
{
    const Eigen::MatrixXd y = blobs(3, 10, 1);
    ml::EM em(2);
    ASSERT_THROW(em.log_densities(y), std::invalid_argument);
    ASSERT_THROW(em.assign_labels(y), std::invalid_argument);
    ASSERT_THROW(em.calculate_responsibilities(y), std::invalid_argument);
    ml::Clustering::KMeans km(2);
    ASSERT_THROW(km.assign_labels(y), std::invalid_argument);
}

static void gpu()
{
    const int d = 5, K = 3;
    const Eigen::MatrixXd train = blobs(d, 4001, 7), test = blobs(d, 2777, 8);
    ml::EM em(K);
    em.set_seed(3);
    em.fit(train);
    const Eigen::VectorXd dens = em.log_densities(test);
    const std::vector<unsigned int> labels = em.assign_labels(test);
    const Eigen::MatrixXd post = em.calculate_responsibilities(test);
    ASSERT_TRUE(dens.size() == test.cols() && labels.size() == static_cast<std::size_t>(test.cols()));
    ASSERT_TRUE(post.rows() == test.cols() && post.cols() == K);
    double sum = 0;
    Eigen::VectorXd u(K);
    for (int i = 0; i < test.cols(); ++i) {
        sum += dens[i];
        em.assign_responsibilities(test.col(i), u);
        unsigned int best = 0;
        for (int k = 0; k < K; ++k) {
            ASSERT_TRUE(std::abs(post(i, k) - u[k]) <= 1e-12);
            if (u[k] > u[best]) best = static_cast<unsigned int>(k);
        }
        ASSERT_TRUE(labels[static_cast<std::size_t>(i)] == best);
    }
    ASSERT_TRUE(em.mean_log_density(test) == sum / static_cast<double>(test.cols()));
    ASSERT_THROW(em.log_densities(blobs(d + 1, 10, 9)), std::invalid_argument);

    ml::Clustering::KMeans km(4);
    km.set_seed(5);
    km.fit(train);
    Eigen::VectorXd dist;
    const std::vector<unsigned int> kl = km.assign_labels(test, &dist);
    ASSERT_TRUE(km.assign_labels(test) == kl);
    for (int i = 0; i < test.cols(); ++i) {
        const auto r = km.assign_label(test.col(i));
        ASSERT_TRUE(r.first == kl[static_cast<std::size_t>(i)] && r.second == dist[i]);
    }
}

int main(int argc, char** argv)
{
    const bool on_gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    host();
    if (on_gpu) gpu();
    std::printf("predict_eigen_test %s: %d failure(s)\n", on_gpu ? "gpu" : "host", failures);
    return failures ? 1 : 0;
}
