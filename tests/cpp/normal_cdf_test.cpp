// device/normal_cdf.hpp as host code, in a program of its own (tests/test_cpp_normal_cdf.py builds it with
// -fsanitize=address,undefined and runs it): the special values, no step down over a dense grid, the library's erfc as a coarse
// second opinion, the quantile's round trip and oddness. The accuracy proper is measured against a 40-digit reference in
// tests/test_normal_cdf.py.
#include <cmath>
#include <cstdio>
#include <limits>

#include "normal_cdf.hpp"

static int failures = 0;
#define ASSERT_TRUE(cond) do { if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

int main()
{
    using mlhip::normal_cdf;
    using mlhip::normal_pdf;
    using mlhip::normal_quantile;
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    ASSERT_TRUE(normal_cdf(-inf) == 0.0 && normal_cdf(inf) == 1.0 && std::isnan(normal_cdf(nan)));
    ASSERT_TRUE(normal_cdf(0.0) == 0.5 && normal_cdf(-0.0) == 0.5);
    ASSERT_TRUE(normal_cdf(-40.0) == 0.0 && normal_cdf(-1e300) == 0.0 && normal_cdf(1e300) == 1.0);
    ASSERT_TRUE(normal_cdf(-38.0) > 0.0 && normal_cdf(-38.0) < 1e-300);
    ASSERT_TRUE(normal_pdf(0.0) == 3.98942280401432677940e-01 && normal_pdf(inf) == 0.0 && std::isnan(normal_pdf(nan)));

    // no step down, and the library's erfc within its own argument's rounding: erfc(-a / sqrt 2) / 2 carries (1 + a^2) ulp of that
    double before = 0.0, worst = 0.0;
    for (int i = 0; i <= 470000; ++i) {
        const double a = -38.0 + i * 1e-4;
        const double F = normal_cdf(a);
        ASSERT_TRUE(F >= before);
        before = F;
        const double ref = 0.5 * std::erfc(-a * 0.70710678118654752440);
        if (ref >= std::numeric_limits<double>::min()) {
            const double err = std::fabs(F - ref) / ref / (1.0 + a * a);
            worst = err > worst ? err : worst;
        }
    }
    std::printf("normal_cdf against erfc: worst %.2e (1 + a^2)\n", worst);
    ASSERT_TRUE(worst <= 8 * 0x1p-53);

    // the quantile: +0.0 at a half, odd where 1 - p is exact, NaN outside (0, 1), and back through the CDF
    ASSERT_TRUE(normal_quantile(0.5) == 0.0 && !std::signbit(normal_quantile(0.5)));
    ASSERT_TRUE(std::isnan(normal_quantile(0.0)) && std::isnan(normal_quantile(1.0)) && std::isnan(normal_quantile(nan)) && std::isnan(normal_quantile(-0.5)));
    for (int e = 1; e <= 300; ++e) {
        const double p = std::pow(10.0, -e), z = normal_quantile(p);
        ASSERT_TRUE(z < 0.0 && std::isfinite(z));
        // one ulp of z moves Phi by |z| ulp(z) phi / Phi ~ z^2 2^-52 relative; the CDF's own 6e-16 beside it
        ASSERT_TRUE(std::fabs(normal_cdf(z) - p) <= p * (8 * 0x1p-53 + z * z * 0x1p-52));
    }
    for (int i = 1; i < 1024; ++i) {
        const double p = i / 1024.0;                             // (1 - p is exact)
        ASSERT_TRUE(normal_quantile(p) == -normal_quantile(1.0 - p));
        ASSERT_TRUE(i == 1 || normal_quantile(p) > normal_quantile((i - 1) / 1024.0));
    }
    std::printf("normal_cdf_test: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
