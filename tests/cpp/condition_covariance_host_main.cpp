// host::condition_covariances (ml_amd/csrc/host/em_math.cpp) as a stand-alone program, for a build of that file and this one under
// -fsanitize=address,undefined (tests/test_cpp_condition_sample.py): exactly sized heap buffers, so that a read or write past either
// output or the inputs is an error report, over the shapes and modes of tests/cpp/condition_host_main.cpp, with the identities
// C = Sigma_MM - A Sigma_OM (A from host::condition) and G G^T = C checked on the way, once with and once without the factors.
// Prints "condition covariance host ok" and returns 0.
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
    const std::size_t dd = static_cast<std::size_t>(d) * d, mm = static_cast<std::size_t>(dM) * dM;
    const std::size_t count = mlhip::host::covariance_doubles(mode, K, d);
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
    std::unique_ptr<double[]> c_m(new double[K * mm]), factors(new double[K * mm]), c_only(new double[K * mm]);
    mlhip::host::condition_covariances(mode, K, d, cov.get(), obs.get(), dO, c_m.get(), factors.get());
    mlhip::host::condition_covariances(mode, K, d, cov.get(), obs.get(), dO, c_only.get(), nullptr);
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
    double worst_schur = 0, worst_factor = 0;
    bool same = true, shape = true;
    for (int k = 0; k < K; ++k)
        for (int a = 0; a < dM; ++a)
            for (int b = 0; b < dM; ++b) {
                const double c = c_m[k * mm + static_cast<std::size_t>(a) * dM + b];
                same = same && c == c_only[k * mm + static_cast<std::size_t>(a) * dM + b] && c == c_m[k * mm + static_cast<std::size_t>(b) * dM + a];
                double s = full[k * dd + static_cast<std::size_t>(missing[b]) * d + missing[a]], scale = std::fabs(s);
                for (int l = 0; l < dO; ++l) {
                    const double term = maps[(static_cast<std::size_t>(k) * dM + a) * dO + l] * full[k * dd + static_cast<std::size_t>(missing[b]) * d + observed[l]];
                    s -= term;
                    scale += std::fabs(term);
                }
                worst_schur = std::fmax(worst_schur, std::fabs(s - c) / (scale + 1e-300));
                double p = 0, pscale = 0;
                for (int l = 0; l < dM; ++l) {
                    const double term = factors[k * mm + static_cast<std::size_t>(a) * dM + l] * factors[k * mm + static_cast<std::size_t>(b) * dM + l];
                    p += term;
                    pscale += std::fabs(term);
                }
                worst_factor = std::fmax(worst_factor, std::fabs(p - c) / (pscale + std::fabs(c) + 1e-300));
                if (b > a) shape = shape && factors[k * mm + static_cast<std::size_t>(a) * dM + b] == 0.0;
                if (b == a) shape = shape && factors[k * mm + static_cast<std::size_t>(a) * dM + b] > 0.0;
            }
    std::printf("mode %d K %d d %d dO %d: residual of C = Sigma_MM - A Sigma_OM %.2e, of G G^T = C %.2e\n", static_cast<int>(mode), K, d, dO,
                worst_schur, worst_factor);
    if (!(worst_schur <= 1e-10) || !(worst_factor <= 1e-10) || !same || !shape) ++failures;
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
    std::vector<unsigned int> ten;
    for (unsigned int c = 0; c < 10; ++c) ten.push_back((c * 23u + 3u) % 70u);
    run(Covariance::Full, 1, 70, ten, 6);                                            // dM = 60 >= 48: the panelled factorisation of C
    run(Covariance::Diagonal, 4, 9, {7, 2, 3, 0}, 7);
    run(Covariance::Tied, 5, 11, {10, 4, 5, 1, 0, 8}, 8);
    run(Covariance::Full, 1, 2, {1}, 9);
    int refused = 0;
    const double indefinite[9] = {1, 2, 0, 2, 1, 0, 0, 0, 1};
    const unsigned int pair[2] = {0, 1}, one[1] = {0};
    std::unique_ptr<double[]> c1(new double[1]), g1(new double[1]), c4(new double[4]), g4(new double[4]);
    try {
        mlhip::host::condition_covariances(Covariance::Full, 1, 3, indefinite, pair, 2, c1.get(), g1.get());   // Sigma_OO indefinite
    } catch (const std::domain_error&) {
        ++refused;
    }
    try {
        mlhip::host::condition_covariances(Covariance::Full, 1, 3, indefinite, one, 1, c4.get(), g4.get());    // the complement is
    } catch (const std::domain_error&) {
        ++refused;
    }
    if (refused != 2) ++failures;
    std::printf(failures ? "condition covariance host FAILED\n" : "condition covariance host ok\n");
    return failures ? 1 : 0;
}
