// host::condition (ml_amd/csrc/host/em_math.cpp) as a stand-alone program, for a build of that file and this one under
// -fsanitize=address,undefined (tests/test_cpp_condition.py): exactly sized heap buffers, so that a read or write past any of the four
// outputs or the inputs is an error report, over the shapes and modes of tests/test_condition_host.py, with the identities
// Sigma_OO A^T = Sigma_OM checked on the way. Prints "condition host ok" and returns 0.
#include <cmath>
#include <cstdio>
#include <memory>
#include <numeric>
#include <random>
#include <stdexcept>
#include <vector>

#include "host/em_math.hpp"

using mlhip::host::Covariance;

static int failures = 0;

static void run(Covariance mode, int K, int d, std::vector<unsigned int> observed, unsigned seed)
{
    std::mt19937_64 rng(seed);
    std::normal_distribution<double> g;
    const int dO = static_cast<int>(observed.size()), dM = d - dO;
    const std::size_t dd = static_cast<std::size_t>(d) * d, count = mlhip::host::covariance_doubles(mode, K, d);
    std::unique_ptr<double[]> means(new double[static_cast<std::size_t>(K) * d]), cov(new double[count]);
    for (int i = 0; i < K * d; ++i) means[i] = 2.5 * g(rng);
    if (mode == Covariance::Diagonal) {
        for (std::size_t i = 0; i < count; ++i) {
            const double v = g(rng);
            cov[i] = 0.5 + v * v;
        }
    } else {
        std::vector<double> a(dd);
        for (std::size_t k = 0; k < count / dd; ++k) {
            for (double& v : a) v = g(rng);
            for (int r = 0; r < d; ++r)
                for (int c = 0; c < d; ++c) {
                    double s = r == c ? 0.5 : 0.0;
                    for (int l = 0; l < d; ++l) s += a[static_cast<std::size_t>(l) * d + r] * a[static_cast<std::size_t>(l) * d + c] / d;
                    cov[k * dd + static_cast<std::size_t>(c) * d + r] = s;
                }
        }
    }
    std::unique_ptr<unsigned int[]> obs(new unsigned int[dO]);
    std::copy(observed.begin(), observed.end(), obs.get());
    std::unique_ptr<double[]> mu_o(new double[static_cast<std::size_t>(K) * dO]), s_oo(new double[static_cast<std::size_t>(K) * dO * dO]),
        maps(new double[static_cast<std::size_t>(K) * dM * dO]), mu_m(new double[static_cast<std::size_t>(K) * dM]);
    mlhip::host::condition(mode, K, d, means.get(), cov.get(), obs.get(), dO, mu_o.get(), s_oo.get(), maps.get(), mu_m.get());

    std::vector<char> seen(d, 0);
    for (unsigned int c : observed) seen[c] = 1;
    std::vector<int> missing;
    for (int j = 0; j < d; ++j)
        if (!seen[j]) missing.push_back(j);
    std::vector<double> full(static_cast<std::size_t>(K) * dd);
    mlhip::host::covariances_as_full(mode, K, d, cov.get(), full.data());
    double worst = 0;
    for (int k = 0; k < K; ++k)
        for (int j = 0; j < dM; ++j)
            for (int a = 0; a < dO; ++a) {
                double s = 0, scale = 0;
                for (int b = 0; b < dO; ++b) {
                    const double term = s_oo[(static_cast<std::size_t>(k) * dO + b) * dO + a] * maps[(static_cast<std::size_t>(k) * dM + j) * dO + b];
                    s += term;
                    scale += std::fabs(term);
                }
                const double want = full[k * dd + static_cast<std::size_t>(missing[j]) * d + observed[a]];
                const double err = std::fabs(s - want) / (scale + std::fabs(want) + 1e-300);
                worst = err > worst ? err : worst;
            }
    std::printf("mode %d K %d d %d dO %d: residual of Sigma_OO A^T = Sigma_OM %.2e\n", static_cast<int>(mode), K, d, dO, worst);
    if (!(worst <= 1e-10)) ++failures;
}

int main()
{
    run(Covariance::Full, 2, 3, {2, 0}, 1);
    run(Covariance::Full, 3, 8, {0, 2, 4, 6, 7}, 2);
    run(Covariance::Full, 3, 7, {6, 1, 3}, 3);
    std::vector<unsigned int> first16(16);
    std::iota(first16.begin(), first16.end(), 0u);
    run(Covariance::Full, 2, 32, first16, 4);
    std::vector<unsigned int> forty;
    for (unsigned int c = 0; c < 40; ++c) forty.push_back((c * 23u + 3u) % 70u);     // 23 is coprime to 70: 40 distinct coordinates
    run(Covariance::Full, 2, 70, forty, 5);
    std::vector<unsigned int> sixty;
    for (unsigned int c = 0; c < 60; ++c) sixty.push_back((c * 23u + 3u) % 70u);
    run(Covariance::Full, 1, 70, sixty, 6);                                          // dO = 60 >= 48: the panelled factorisation
    run(Covariance::Diagonal, 4, 9, {7, 2, 3, 0}, 7);
    run(Covariance::Tied, 5, 11, {10, 4, 5, 1, 0, 8}, 8);
    run(Covariance::Full, 1, 2, {1}, 9);
    bool refused = false;
    const double mean[3] = {0, 0, 0}, indefinite[9] = {1, 2, 0, 2, 1, 0, 0, 0, 1};
    const unsigned int pair[2] = {0, 1};
    double mu_o[2], s_oo[4], maps[2], mu_m[1];
    try {
        mlhip::host::condition(Covariance::Full, 1, 3, mean, indefinite, pair, 2, mu_o, s_oo, maps, mu_m);
    } catch (const std::domain_error&) {
        refused = true;
    }
    if (!refused) ++failures;
    std::printf(failures ? "condition host FAILED\n" : "condition host ok\n");
    return failures ? 1 : 0;
}
