// Exact integer arithmetic of the fixed-point K-means++ draw (FixedPointKPP, include/ML/Clustering.hpp), shared by the kernels
// (kpp_fixed_point.hip), the runtime's exchange between ranks (runtime/kmeans.cpp) and the host restatement (host/facade/Clustering.cpp):
// every route forms the same integers, so every route picks the same row.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace mlhip {
namespace fixed_point {

typedef unsigned __int128 u128;

/// Offset added to a frexp exponent (-1073 .. 1024) so that it crosses the ranks' double all-reduce as a positive integer; 0 stands
/// for "no positive weight".
constexpr int kExponentBias = 1100;

/// q = floor(w * 2^(52 - E)) for a weight 0 <= w < 2^E given by its bits (sign bit clear): an integer below 2^52, formed with
/// integer shifts of w's significand only (w = m 2^(f - 1075), f the biased exponent; a subnormal w has f = 0 and no hidden bit).
__host__ __device__ __forceinline__ uint64_t quantise(uint64_t bits, int E)
{
    int f = (int)(bits >> 52);
    uint64_t m = bits & ((uint64_t(1) << 52) - 1);
    if (f != 0) m |= uint64_t(1) << 52;
    else f = 1;
    const int sh = f - 1023 - E;                   // q = m 2^sh
    if (sh >= 0) return m << sh;                   // (only a subnormal largest weight: E <= -1022)
    return -sh >= 64 ? 0 : m >> -sh;
}

/// floor(u * T) exactly, for a double 0 <= u < 1 and an integer T < 2^84: u = m 2^(e - 53) with a 53-bit integer m, so
/// u T = (m (T >> 42) 2^42 + m (T mod 2^42)) 2^(e - 53), both products below 2^95.
inline u128 scaled_floor(double u, u128 T)
{
    if (!(u > 0.0) || T == 0) return 0;
    int e = 0;
    const double f = std::frexp(u, &e);            // u = f 2^e, f in [0.5, 1), e <= 0
    const uint64_t m = (uint64_t)std::ldexp(f, 53);
    const u128 low = (u128)m * (uint64_t)(T & ((u128(1) << 42) - 1));
    const u128 r = (u128)m * (uint64_t)(T >> 42) + (low >> 42);   // floor(u T 2^(53 - e - 42))
    const int s = 53 - e - 42;                     // >= 11
    return s >= 128 ? 0 : r >> s;
}

}  // namespace fixed_point
}  // namespace mlhip
