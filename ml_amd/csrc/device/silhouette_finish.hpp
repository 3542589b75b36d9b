// The closing arithmetic of the silhouette (silhouette.hip's second kernel, mlhip_silhouette_finish, and a device group's host side):
// from the sums D_c = sum_{j in cluster c} |x_i - x_j| of one row i with label `own`, and the cluster sizes n_c,
//     a = D_own / (n_own - 1),   b = min over c != own with n_c > 0 of D_c / n_c (the FIRST minimum),   s = (b - a) / max(a, b),
// with s = 0 and a = 0 for a row alone in its cluster, and s = 0 where max(a, b) = 0 (scikit-learn's conventions). One division per
// cluster, one for s; a NaN among the means that enter stays (in b and s). Labels no row carries (n_c = 0) are passed over. The
// clusters are fed in ascending order, one call each, so that the device need not hold K sums per row. Plain C++: the same text
// compiles for the host.
#pragma once
#include <cstdint>

#if defined(__HIP_DEVICE_COMPILE__) || defined(__HIPCC__)
#define MLHIP_SILHOUETTE_FN __device__ __host__ __forceinline__
#else
#define MLHIP_SILHOUETTE_FN inline
#endif

namespace mlhip {

struct SilhouetteFinish {
    uint32_t own;
    double own_sum, b;

    MLHIP_SILHOUETTE_FN void begin(uint32_t own_label)
    {
        own = own_label;
        own_sum = 0.0;
        b = __builtin_inf();
    }
    /// Cluster c of n_c rows with this row's sum of distances to them; ascending c.
    MLHIP_SILHOUETTE_FN void add(uint32_t c, double n_c, double sum)
    {
        if (c == own) { own_sum = sum; return; }
        if (!(n_c > 0.0)) return;
        const double mean = sum / n_c;
        if (mean < b || mean != mean) b = mean;                    // (strict: the first minimum wins; a NaN is kept from then on)
    }
    MLHIP_SILHOUETTE_FN void end(double n_own, double& a_out, double& b_out, double& s_out) const
    {
        b_out = b;
        if (!(n_own > 1.0)) { a_out = 0.0; s_out = 0.0; return; }  // alone in its cluster
        const double a = own_sum / (n_own - 1.0);
        const double larger = a > b || a != a ? a : b;             // (a NaN in either is the larger one: it reaches s)
        a_out = a;
        s_out = larger == 0.0 ? 0.0 : (b - a) / larger;
    }
};

}  // namespace mlhip
