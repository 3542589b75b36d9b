// The batch queries of the C++ facade (extensions): EM::log_densities / mean_log_density / assign_labels /
// calculate_responsibilities and KMeans::assign_labels from ordinary C++17. `host`: argument errors, no GPU needed; `gpu`: against
// the single-point queries of the same fitted models.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <stdexcept>
#include <vector>

#include "ML/EM.hpp"
#include "ML/KMeans.hpp"

using namespace ml;

#define REQUIRE(cond)                                                              \
    do {                                                                           \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

template <class E, class F> bool throws(F&& f)
{
    try { f(); } catch (const E&) { return true; } catch (...) { return false; }
    return false;
}

static MatrixXd blobs(Index d, Index n, unsigned seed)
{
    std::mt19937_64 rng(seed);
    std::normal_distribution<double> g;
    MatrixXd x(d, n);
    for (Index i = 0; i < n; ++i)
        for (Index j = 0; j < d; ++j) x(j, i) = g(rng) + 4.0 * static_cast<double>((i + j) % 3) + 2.0;
    return x;
}

static void host()
{
    MatrixXd y = blobs(3, 10, 1);
    EM em(2);                                                  // not fitted: as assign_responsibilities on such a model
    REQUIRE(throws<std::invalid_argument>([&] { em.log_densities(y); }));
    REQUIRE(throws<std::invalid_argument>([&] { em.assign_labels(y); }));
    REQUIRE(throws<std::invalid_argument>([&] { em.calculate_responsibilities(y); }));
    REQUIRE(throws<std::invalid_argument>([&] { em.mean_log_density(y); }));
    Clustering::KMeans km(2);
    REQUIRE(throws<std::invalid_argument>([&] { km.assign_labels(y); }));
}

static void gpu()
{
    const Index d = 5, n = 4001, K = 3;
    MatrixXd train = blobs(d, n, 7), test = blobs(d, 2777, 8);
    EM em(K);
    em.set_seed(3);
    em.fit(train);
    const VectorXd dens = em.log_densities(test);
    const std::vector<unsigned int> labels = em.assign_labels(test);
    const MatrixXd post = em.calculate_responsibilities(test);
    REQUIRE(dens.size() == test.cols() && static_cast<Index>(labels.size()) == test.cols());
    REQUIRE(post.rows() == test.cols() && post.cols() == K);
    double sum = 0;
    std::vector<double> u(K);
    for (Index i = 0; i < test.cols(); ++i) {
        REQUIRE(std::isfinite(dens[i]));
        sum += dens[i];
        em.assign_responsibilities(ConstVectorRef(test.col(i), d), VectorRef(u));
        unsigned int best = 0;
        for (Index k = 0; k < K; ++k) {
            REQUIRE(std::abs(post(i, k) - u[static_cast<std::size_t>(k)]) <= 1e-12);
            if (u[static_cast<std::size_t>(k)] > u[best]) best = static_cast<unsigned int>(k);
        }
        // (well separated blobs: no row within rounding of a tie)
        REQUIRE(labels[static_cast<std::size_t>(i)] == best);
    }
    REQUIRE(em.mean_log_density(test) == sum / static_cast<double>(test.cols()));
    MatrixXd wrong = blobs(d + 1, 10, 9);
    REQUIRE(throws<std::invalid_argument>([&] { em.log_densities(wrong); }));
    // the fit's own block is untouched: its responsibilities are still there
    REQUIRE(em.responsibilities().rows() == n);

    Clustering::KMeans km(4);
    km.set_seed(5);
    km.fit(train);
    VectorXd dist;
    const std::vector<unsigned int> kl = km.assign_labels(test, &dist);
    REQUIRE(km.assign_labels(test) == kl);
    for (Index i = 0; i < test.cols(); ++i) {
        const auto r = km.assign_label(ConstVectorRef(test.col(i), d));
        REQUIRE(r.first == kl[static_cast<std::size_t>(i)] && r.second == dist[i]);   // the same bits
    }
    REQUIRE(throws<std::invalid_argument>([&] { km.assign_labels(wrong); }));
}

int main(int argc, char** argv)
{
    const bool on_gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    host();
    if (on_gpu) gpu();
    std::printf("predict_test %s ok\n", on_gpu ? "gpu" : "host");
    return 0;
}
