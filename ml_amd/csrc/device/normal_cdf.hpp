// The standard normal CDF and density for the conditional CDF / quantile kernels (em_condition_quantile.hip), and the quantile
// function the host turns probabilities into z-scores with. No table, no library call, no branch on the argument: ONE form for every a,
//     Phi(-t) = exp(-t^2 / 2) * y * P(s),   t = min(|a|, 40),  y = 4 / (4 + t),  s = 1 - 2.2 (1 - y)   (s in [-1, 1] for t in [0, 40]),
// with P the degree-25 interpolant of erfcx(t / sqrt 2) / (2 y) at the Chebyshev nodes in s (truncation < 1e-18; the coefficients sum,
// in the Horner order at s = 1, to 0.5 EXACTLY, so Phi(0) = 0.5), and Phi(a) = 1 - Phi(-a) for a > 0. The exponential is exp_nonpos of
// h / -2, h = fl(t * t), corrected for the square's rounding by the exact remainder l = fma(t, t, -h): e (1 - l / 2) -- without it the
// argument's rounding alone costs |a|^2 / 2 ulp in the tail. Fixed fma order, 1 division, 26 fma for P, 20 operations of exp_nonpos.
// Phi(-inf) = 0 (t = 40: exp_nonpos gives exactly 0 below -745.2; the true Phi(-38.5) is already below the smallest subnormal),
// Phi(+inf) = 1, NaN -> NaN; Phi(-t) <= 0.5 is enforced, so the function does not step down across 0.
// Measured against mpmath at 40 digits on the grid of tests/test_normal_cdf.py (a in [-38, 9], 55 014 points): relative error <= 6.01e-16
// (5.4 ulp: the exponential's 1, the division's, the 26-term Horner chain's and three products') wherever the result is a normal number
// (a >= -37.5); below, where the format itself has no relative accuracy left, the error is <= 1.84 spacings of the subnormals
// (2^-1074). The test asserts twice both. Plain C++: the same text compiles for the host.
#pragma once
#include <cmath>
#include "exp_nonpos.hpp"

namespace mlhip {

/// Phi(a) and, in `pdf`, phi(a) = exp_nonpos(-(a * a) / 2) / sqrt(2 pi) from the same exponential (before its correction).
MLHIP_EXP_FN double normal_cdf_pdf(double a, double& pdf)
{
    double t = __builtin_fabs(a);
    t = t > 40.0 ? 40.0 : t;                                       // (a NaN stays a NaN)
    const double h = t * t;
    const double l = __builtin_fma(t, t, -h);                      // exact: t * t = h + l
    // (exp_nonpos converts its argument's multiple of ln 2 to an int, which a NaN has none of: it is kept out of the call and comes back
    // through l below, and through t into the density)
    double e = exp_nonpos(h == h ? -0.5 * h : 0.0);
    pdf = h == h ? e * 3.98942280401432677940e-01 : t;             // 1 / sqrt(2 pi)
    e = __builtin_fma(-0.5 * l, e, e);
    const double inv = 1.0 / (4.0 + t);
    const double y = 4.0 * inv;
    const double s = __builtin_fma(-2.2, t * inv, 1.0);
    double p = -3.5616201178717097e-12;                            // s^25
    p = __builtin_fma(p, s, 1.4304836415634612e-13);
    p = __builtin_fma(p, s, 4.156875033198687e-11);
    p = __builtin_fma(p, s, -3.1510090637675974e-11);
    p = __builtin_fma(p, s, -2.3961638006367336e-10);
    p = __builtin_fma(p, s, 4.5132276558319005e-10);
    p = __builtin_fma(p, s, 7.616101808787145e-10);
    p = __builtin_fma(p, s, -3.6239182985901363e-09);
    p = __builtin_fma(p, s, 5.17917442552542e-10);
    p = __builtin_fma(p, s, 2.1751721630760914e-08);
    p = __builtin_fma(p, s, -3.023841186173345e-08);
    p = __builtin_fma(p, s, -1.1141473563501418e-07);
    p = __builtin_fma(p, s, 3.16230487060742e-07);
    p = __builtin_fma(p, s, 5.519693638234361e-07);
    p = __builtin_fma(p, s, -2.6992962518367036e-06);
    p = __builtin_fma(p, s, -3.416941566285219e-06);
    p = __builtin_fma(p, s, 2.2666143288859767e-05);
    p = __builtin_fma(p, s, 3.7020355213816946e-05);
    p = __builtin_fma(p, s, -0.00018807762353158263);
    p = __builtin_fma(p, s, -0.0006311061539636845);
    p = __builtin_fma(p, s, 0.0008330788582040306);
    p = __builtin_fma(p, s, 0.010817311005331433);
    p = __builtin_fma(p, s, 0.03926582960010864);
    p = __builtin_fma(p, s, 0.09112701348669128);
    p = __builtin_fma(p, s, 0.15524857171253112);
    p = __builtin_fma(p, s, 0.2034730626815634);
    double x = e * (y * p);
    x = x > 0.5 ? 0.5 : x;
    return a > 0.0 ? 1.0 - x : x;
}

MLHIP_EXP_FN double normal_cdf(double a)
{
    double pdf;
    return normal_cdf_pdf(a, pdf);
}

MLHIP_EXP_FN double normal_pdf(double a)
{
    double pdf;
    normal_cdf_pdf(a, pdf);
    return pdf;
}

/// Phi^-1(p) on the host, p inside (0, 1) (else NaN): the rational start of Abramowitz & Stegun 26.2.23 (|error| < 4.5e-4) on the lower
/// tail, then four Halley steps on normal_cdf (cubic: the third already moves z by less than an ulp); p > 0.5 is -Phi^-1(1 - p), and
/// 1 - p is exact there, so the function is odd about 0.5 wherever 1 - p is a double. normal_quantile(0.5) = +0.0.
inline double normal_quantile(double p)
{
    if (!(p > 0.0 && p < 1.0)) return std::nan("");
    if (p == 0.5) return 0.0;
    if (p > 0.5) return -normal_quantile(1.0 - p);
    const double u = std::sqrt(-2.0 * std::log(p));
    double z = -(u - (2.515517 + u * (0.802853 + u * 0.010328)) / (1.0 + u * (1.432788 + u * (0.189269 + u * 0.001308))));
    for (int step = 0; step < 4; ++step) {
        double pdf;
        const double f = normal_cdf_pdf(z, pdf) - p;
        if (!(pdf > 0.0)) break;
        const double dz = f / pdf;
        z -= dz / __builtin_fma(0.5 * z, dz, 1.0);
    }
    return z;
}

}  // namespace mlhip
