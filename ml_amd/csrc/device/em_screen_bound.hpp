// Bound constants of the screened E-step (em_estep_screen.hip): from the parameter set a stored log-responsibility block belongs to
// (mu, W = L^-1, coef) and the new one (mu', W', coef'), per component four numbers such that for every sample
//     lw'  <=  alpha  * lw + A        (upper bound of the new value)
//     lw'  >=  alpha' * lw + A'       (lower bound)
// where lw is the stored value of that pair. With z = W (x - mu), q = |z|^2 = 2 (coef - lw):  y' = W' (x - mu') = M z + c,
// M = W' L, c = W' (mu - mu'). f = |I - M|_F bounds |M z - z| <= f |z|, so with a = 1 - f, b = 1 + f, g = |c|:
//     |y'| >= a sqrt(q) - g,   |y'| <= b sqrt(q) + g,   and with 2 sqrt(q) <= q + 1
//     q' >= a (a - g) q - a g          (a > g, else "no information")
//     q' <= b (b + g) q + b g + g^2
// i.e. alpha = a (a - g), A = coef' - alpha coef + a g / 2, alpha' = b (b + g), A' = coef' - alpha' coef - (b g + g^2) / 2.
// alpha >= 0: an UPPER bound of lw in place of lw still gives an upper bound of lw' (the recurrence stays sound on bounds).
// Everything is rounded outward by a relative 2^-40: f and g up, alpha down and A up, alpha' up and A' down. On top of f comes an
// allowance for the rounding of the triangular solve M W = W': d 2^-50 (wmax / wmin) (1 + |M|_F), with the ratio of the largest to the
// smallest diagonal entry of W standing in for cond(W). That term is an ESTIMATE of the solve's forward error, not a proven bound (the
// diagonal ratio does not bound the conditioning of a triangular matrix); beyond a ratio of kMaxDiagRatio the bound is given up.
// Plain C++: the device kernel and the host (tests/cpp) compile the same text.
#pragma once
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MLHIP_SCREEN_HD __host__ __device__
#else
#define MLHIP_SCREEN_HD
#endif

namespace mlhip {
namespace screen {

constexpr double kOutward = 0x1p-40;          // relative outward rounding
constexpr double kMaxDiagRatio = 1.0e5;       // max W_jj / min W_jj beyond which the triangular solve is not trusted: no information
constexpr double kSkipMargin = 746.0;         // exp(t) is exactly 0 in fp64 for t < -745.2 (the dense LSE form's own constant)
constexpr double kMaxStored = 0x1p40;         // stored values at or beyond this magnitude are never bounded from

/// What row i of the two whitening matrices contributes. Wo / Wn: dense lower triangles, row stride ldw. M_row: scratch of i + 1 doubles
/// (stride ms) that receives row i of M = W' L, from the substitution M W = W' (column i down to 0).
struct RowTerms {
    double f2;        // sum_j (delta_ij - M_ij)^2
    double m2;        // sum_j M_ij^2
    double c;         // (W' (mu - mu'))_i
    double cabs;      // sum_j |W'_ij (mu - mu')_j|
};

MLHIP_SCREEN_HD inline RowTerms row_terms(int i, const double* Wo, const double* Wn, int ldw, const double* mu_o, const double* mu_n,
                                          double* M_row, int ms)
{
    RowTerms t{0.0, 0.0, 0.0, 0.0};
    for (int j = i; j >= 0; --j) {
        double s = Wn[i * ldw + j];
        for (int l = j + 1; l <= i; ++l) s -= M_row[l * ms] * Wo[l * ldw + j];
        const double m = s / Wo[j * ldw + j];
        M_row[j * ms] = m;
        const double e = (j == i ? 1.0 : 0.0) - m;
        t.f2 += e * e;
        t.m2 += m * m;
    }
    for (int j = 0; j <= i; ++j) {
        const double p = Wn[i * ldw + j] * (mu_o[j] - mu_n[j]);
        t.c += p;
        t.cabs += std::fabs(p);
    }
    return t;
}

/// The four constants of one component from the sums over its rows: f2 = sum f2_i, m2 = sum m2_i, g2 = sum (|c_i| + 2^-40 cabs_i)^2;
/// wmin / wmax: the smallest and largest diagonal entry of the OLD whitening matrix (the divisors of the solve). Returns false -- and
/// the constants that make every pair a candidate -- when the bound carries no information.
MLHIP_SCREEN_HD inline bool constants(int d, double f2, double m2, double g2, double coef_o, double coef_n, double wmin, double wmax,
                                      double out[4])
{
    const double inf = HUGE_VAL;
    out[0] = 0.0; out[1] = inf; out[2] = 0.0; out[3] = -inf;
    // (every comparison is written so that a NaN fails it)
    if (!(f2 >= 0.0 && f2 < inf && m2 < inf && g2 >= 0.0 && g2 < inf)) return false;
    if (!(std::fabs(coef_o) < inf && std::fabs(coef_n) < inf)) return false;
    if (!(wmin > 0.0 && wmax < inf && wmax <= kMaxDiagRatio * wmin)) return false;
    const double solve = (double)d * 0x1p-50 * (wmax / wmin) * (1.0 + std::sqrt(m2));      // (estimate: see the head of the file)
    const double f = std::sqrt(f2) * (1.0 + kOutward) + kOutward * std::sqrt((double)d) * (1.0 + std::sqrt(m2)) + solve;
    const double g = std::sqrt(g2) * (1.0 + kOutward);
    const double a = (1.0 - f) * (1.0 - kOutward), b = (1.0 + f) * (1.0 + kOutward);
    if (!(a > g)) return false;
    const double alpha = a * (a - g) * (1.0 - 4 * kOutward);
    const double alpha_l = b * (b + g) * (1.0 + 4 * kOutward);
    const double ag = 0.5 * a * g * (1.0 + kOutward);
    const double bg = 0.5 * (b * g + g * g) * (1.0 + 4 * kOutward);
    const double A = (coef_n - alpha * coef_o) + ag;
    const double Al = (coef_n - alpha_l * coef_o) - bg;
    const double pad_u = 4 * kOutward * (std::fabs(coef_n) + alpha * std::fabs(coef_o) + ag + 1.0);
    const double pad_l = 4 * kOutward * (std::fabs(coef_n) + alpha_l * std::fabs(coef_o) + bg + 1.0);
    if (!(alpha >= 0.0 && alpha_l < inf)) return false;
    out[0] = alpha; out[1] = A + pad_u; out[2] = alpha_l; out[3] = Al - pad_l;
    return true;
}

}  // namespace screen
}  // namespace mlhip
