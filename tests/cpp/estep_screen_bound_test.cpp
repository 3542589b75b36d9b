// The bound constants of the screened E-step (ml_amd/csrc/device/em_screen_bound.hpp, the text the device kernel compiles too) in
// their host form, held against a long double evaluation of the true new log-responsibility  lw' = coef' - |W' (x - mu')|^2 / 2  of
// the parameters as the records hold them (doubles):  alpha' lw + A'  <=  lw'  <=  alpha lw + A  for every pair, lw the stored value
// of the old parameters. Random parameter pairs at d = 12, 21, 32 with tiny to large drift, a drift just below and just above the
// point where the bound loses its information (f = 1 - gamma), a covariance of condition number 1e8, a mixing weight of 0 on either
// side, far rows at the edge of the guard on W's diagonal, and 30 chained passes in which a stored value is never refreshed (a bound of a bound of ...). No GPU, no library.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "device/em_screen_bound.hpp"

using ld = long double;
namespace sc = mlhip::screen;

struct Component {
    int d;
    std::vector<double> mu, L, W;   // L, W = L^-1: dense lower triangles, row stride d
    double coef;
};

static void invert_lower(int d, const std::vector<double>& L, std::vector<double>& W)
{
    W.assign((size_t)d * d, 0.0);
    for (int j = 0; j < d; ++j) {
        W[j * d + j] = (double)(1.0L / (ld)L[j * d + j]);
        for (int i = j + 1; i < d; ++i) {
            ld s = 0;
            for (int l = j; l < i; ++l) s += (ld)L[i * d + l] * (ld)W[l * d + j];
            W[i * d + j] = (double)(-s / (ld)L[i * d + i]);
        }
    }
}

static Component make(int d, std::mt19937_64& rng, double spread, double log_pi, const std::vector<double>* scales = nullptr)
{
    std::normal_distribution<double> g;
    Component c;
    c.d = d;
    c.mu.resize(d);
    c.L.assign((size_t)d * d, 0.0);
    for (int i = 0; i < d; ++i) {
        c.mu[i] = 3.0 * g(rng);
        for (int j = 0; j < i; ++j) c.L[i * d + j] = spread * g(rng) / std::sqrt((double)d);
        c.L[i * d + i] = (scales ? (*scales)[i] : 1.0) * (1.0 + 0.3 * std::fabs(g(rng)));
    }
    invert_lower(d, c.L, c.W);
    ld ldet = 0;
    for (int i = 0; i < d; ++i) ldet += std::log((ld)c.L[i * d + i]);
    c.coef = (double)((ld)log_pi - ldet);
    return c;
}

static Component drifted(const Component& o, std::mt19937_64& rng, double drift, double log_pi)
{
    std::normal_distribution<double> g;
    const int d = o.d;
    Component c = o;
    for (int i = 0; i < d; ++i) {
        c.mu[i] += drift * g(rng) * std::fabs(o.L[i * d + i]);
        for (int j = 0; j <= i; ++j) c.L[i * d + j] += drift * g(rng) * std::fabs(o.L[i * d + i]) / std::sqrt((double)d);
        if (!(c.L[i * d + i] > 0.1 * o.L[i * d + i])) c.L[i * d + i] = 0.1 * o.L[i * d + i];
    }
    invert_lower(d, c.L, c.W);
    ld ldet = 0;
    for (int i = 0; i < d; ++i) ldet += std::log((ld)c.L[i * d + i]);
    c.coef = (double)((ld)log_pi - ldet);
    return c;
}

static ld true_lw(const Component& c, const std::vector<double>& x)
{
    ld q = 0;
    for (int i = 0; i < c.d; ++i) {
        ld y = 0;
        for (int j = 0; j <= i; ++j) y += (ld)c.W[i * c.d + j] * ((ld)x[j] - (ld)c.mu[j]);
        q += y * y;
    }
    return (ld)c.coef - q / 2;
}

/// The host form of the constants: the device kernel's sums, row by row.
static bool host_constants(const Component& o, const Component& n, double out[4])
{
    const int d = o.d;
    std::vector<double> M((size_t)d * d);
    double f2 = 0, m2 = 0, g2 = 0, wmin = HUGE_VAL, wmax = 0;
    for (int i = 0; i < d; ++i) {
        const sc::RowTerms t = sc::row_terms(i, o.W.data(), n.W.data(), d, o.mu.data(), n.mu.data(), M.data() + (size_t)i * d, 1);
        f2 += t.f2; m2 += t.m2;
        const double g = std::fabs(t.c) + sc::kOutward * t.cabs;
        g2 += g * g;
        const double w = std::fabs(o.W[i * d + i]);
        wmin = w < wmin ? w : wmin;
        wmax = w > wmax ? w : wmax;
    }
    return sc::constants(d, f2, m2, g2, o.coef, n.coef, wmin, wmax, out);
}

static long pairs = 0, cases = 0, informative = 0;
static int failures = 0;

static void fail(const char* what, double a, double b)
{
    if (++failures <= 10) std::printf("FAIL %s: %.17g against %.17g\n", what, a, b);
}

/// Samples around the old component from its own scale out to `reach` standard deviations.
static std::vector<std::vector<double>> samples(const Component& c, std::mt19937_64& rng, int count, double reach)
{
    std::normal_distribution<double> g;
    std::vector<std::vector<double>> X;
    for (int s = 0; s < count; ++s) {
        const double scale = reach * (s + 1) / count;
        std::vector<double> z(c.d), x(c.d);
        for (double& v : z) v = scale * g(rng);
        for (int i = 0; i < c.d; ++i) {
            ld t = c.mu[i];
            for (int j = 0; j <= i; ++j) t += (ld)c.L[i * c.d + j] * z[j];
            x[i] = (double)t;
        }
        X.push_back(x);
    }
    return X;
}

static bool check_pair(const Component& o, const Component& n, std::mt19937_64& rng, bool expect_info_known = false, bool expect_info = true,
                       double reach = 60.0)
{
    double k[4];
    const bool info = host_constants(o, n, k);
    ++cases;
    if (expect_info_known && info != expect_info) fail("information flag", info, expect_info);
    if (!info) {
        if (!(k[0] == 0.0 && k[1] == HUGE_VAL && k[2] == 0.0 && k[3] == -HUGE_VAL)) fail("constants without information", k[1], k[3]);
        return false;
    }
    ++informative;
    if (!(k[0] >= 0.0)) fail("alpha >= 0", k[0], 0.0);
    for (const auto& x : samples(o, rng, 40, reach)) {
        const double stored = (double)true_lw(o, x);
        const ld truth = true_lw(n, x);
        const double ub = std::fma(k[0], stored, k[1]), lb = std::fma(k[2], stored, k[3]);
        if (!((ld)ub >= truth)) fail("upper bound", ub, (double)truth);
        if (!((ld)lb <= truth)) fail("lower bound", lb, (double)truth);
        ++pairs;
    }
    return true;
}

int main()
{
    std::mt19937_64 rng(20241020);
    const int dims[] = {12, 21, 32};
    const double drifts[] = {0.0, 1e-15, 1e-9, 1e-5, 1e-3, 1e-2, 5e-2, 0.2, 1.0, 5.0};
    // random pairs, tiny to large drift
    for (int d : dims)
        for (double drift : drifts)
            for (int rep = 0; rep < 4; ++rep) {
                const Component o = make(d, rng, 0.5, std::log(0.02 + 0.1 * rep));
                check_pair(o, drifted(o, rng, drift, std::log(0.03 + 0.1 * rep)), rng);
            }
    // f just below and just above 1 - gamma: L' = L / (1 - phi) gives M = (1 - phi) I, f = phi sqrt(d); mu' = mu + L e_0 t gives gamma ~ t (1 - phi)
    for (int d : dims)
        for (double side : {-1e-6, 1e-6}) {
            const Component o = make(d, rng, 0.5, std::log(0.1));
            Component n = o;
            const double t = 0.25, phi = (1.0 - t) / (std::sqrt((double)d) - t) * (1.0 + side);   // 1 - phi sqrt(d) = t (1 - phi) at side = 0
            for (double& v : n.L) v /= 1.0 - phi;
            for (int i = 0; i < d; ++i) n.mu[i] = o.mu[i] + o.L[i * d] * t;
            invert_lower(d, n.L, n.W);
            n.coef = o.coef - d * std::log(1.0 / (1.0 - phi));
            check_pair(o, n, rng, true, side < 0);
        }
    // a covariance of condition number 1e8 (standard deviations 1 .. 1e4)
    for (int d : dims) {
        std::vector<double> scales(d);
        for (int i = 0; i < d; ++i) scales[i] = std::pow(10.0, 4.0 * i / (d - 1));
        for (double drift : {0.0, 1e-9, 1e-4, 1e-2}) {
            const Component o = make(d, rng, 0.5, std::log(0.1), &scales);
            if (!check_pair(o, drifted(o, rng, drift, std::log(0.1)), rng) && drift <= 1e-4) fail("ill-conditioned pair lost its information", drift, 0);
        }
    }
    // at the edge of the guard on the diagonal of W (standard deviations 1 .. 4e4: a ratio of up to 1e5), rows out to 1.5e5 standard
    // deviations (|lw| up to ~2^39, just inside what the kernel bounds from): where the allowance for the solve is largest
    for (int d : dims) {
        std::vector<double> scales(d);
        for (int i = 0; i < d; ++i) scales[i] = std::pow(10.0, 4.6 * i / (d - 1));
        for (double drift : {0.0, 1e-9, 1e-5}) {
            const Component o = make(d, rng, 0.5, std::log(0.1), &scales);
            check_pair(o, drifted(o, rng, drift, std::log(0.1)), rng, false, true, 1.5e5);
        }
    }
    // a mixing weight of 0 on either side: log 0 in coef, no information
    for (int d : dims) {
        const Component o = make(d, rng, 0.5, std::log(0.1));
        Component z = o;
        z.coef = -HUGE_VAL;
        check_pair(o, z, rng, true, false);
        check_pair(z, o, rng, true, false);
        Component nan = o;
        nan.W[d] = std::nan("");                 // (row 1, column 0)
        check_pair(o, nan, rng, true, false);
        check_pair(nan, o, rng, true, false);
    }
    // 30 chained passes: a pair's stored value is replaced by its upper bound in every pass and never refreshed
    for (int d : dims) {
        Component cur = make(d, rng, 0.5, std::log(0.1));
        const auto X = samples(cur, rng, 40, 60.0);
        std::vector<double> stored;
        for (const auto& x : X) stored.push_back((double)true_lw(cur, x));
        for (int pass = 0; pass < 30; ++pass) {
            const Component next = drifted(cur, rng, pass % 3 == 0 ? 1e-3 : 1e-6, std::log(0.1 + 0.001 * pass));
            double k[4];
            ++cases;
            if (!host_constants(cur, next, k)) { fail("chained pass lost its information", pass, 0); break; }
            for (size_t s = 0; s < X.size(); ++s) {
                stored[s] = std::fma(k[0], stored[s], k[1]);
                if (!((ld)stored[s] >= true_lw(next, X[s]))) fail("chained upper bound", stored[s], (double)true_lw(next, X[s]));
                ++pairs;
            }
            cur = next;
        }
    }
    if (failures) {
        std::printf("estep_screen_bound_test: %d failures\n", failures);
        return 1;
    }
    std::printf("estep_screen_bound_test: ok (%ld cases, %ld with information, %ld pairs)\n", cases, informative, pairs);
    return 0;
}
