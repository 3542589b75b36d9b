// Weighted K-means update for gfx950 (EXTENSION, mlhip_kmeans_*_weighted): the per-cluster sums sum_i w_i x_i, the weighted counts
// sum_i w_i and the weighted inertia sum_i w_i |x_i - c_label(i)|^2 of a block with row weights, as a sweep AFTER the assignment of
// the shape's route (kmeans.hip, kmeans_mfma.hip, big_dim.hip, generic_dim.hip run with accumulate = 0: labels and distances do not
// depend on the weights) and its reduction. Modelled on kmeans_update_kernel / kmeans_reduce_kernel of kmeans.hip, which stay as they
// are.
//
// The sums are EXACT sums of rounded products: p = w_i x_ij is one IEEE product; t = p 2^(94 - ej - ew) with max|x_j| < 2^ej and
// max w < 2^ew over the WHOLE sample (all ranks), so |t| < 2^94, and the scaling is exact: it is applied as two powers of two f1_j,
// f2_j (each a normal double whatever ej + ew is; the runtime chooses them, KmWeightedArgs::factors). t is cut into three 32-bit
// limbs (split_limbs: what lies below one unit, i.e. below 2^-94 max w max|x_j|, is dropped) and added with 64-bit INTEGER atomics into
// workgroup-private LDS accumulators. The weighted count of a cluster is accumulated the same way from w_i 2^(94 - ew), three limbs: a
// cluster takes 3d + 3 words. Integer addition is associative: sums and counts do not depend on the order in which lanes, waves,
// workgroups, shards or ranks contribute. No floating-point atomics; plain vector stores.
#include "device.hpp"
#include "exact_sum.hpp"

namespace mlhip {
namespace {

constexpr int BSW = 1024;

/// One sweep over X (dimension-major, unpadded), the labels and distances the assignment just wrote, and the weights. The LDS
/// accumulators are chunked like kmeans_update_kernel's: by DIMENSION first (a chunk holds the limbs of DC dimensions for all
/// clusters; X is read once over all passes), by clusters as well (KC < K) only when one dimension of all K clusters does not fit.
/// A chunk's words are flushed into the workgroup's partial block [inertia_w, unused, K x (3d + 3) words]; `with_sums` = 0: the
/// weighted inertia only (mlhip_kmeans_assign_weighted).
__global__ __launch_bounds__(BSW) void kmeans_weighted_update_kernel(
    const double* __restrict__ xt, size_t ldx, uint32_t n, int d, const uint32_t* __restrict__ labels, const double* __restrict__ min_dist,
    const double* __restrict__ w, const double* __restrict__ factors, int K, int KC, int DC, int with_sums, double* __restrict__ partials,
    size_t pstride)
{
    extern __shared__ u64 acc_lds[];      // [KC][3*DC + 3]
    __shared__ double red[BSW / 64];
    const int tid = threadIdx.x;
    double* my_part = partials + (size_t)blockIdx.x * pstride;
    const uint32_t first = blockIdx.x * (uint32_t)BSW + tid, stride = gridDim.x * (uint32_t)BSW;

    // weighted inertia: per-lane sums in row order, then the fixed-order wave and workgroup tree of the unweighted inertia
    double inertia = 0.0;
    {
#pragma clang fp contract(off)
        for (uint32_t i = first; i < n; i += stride) {
            const double p = w[i] * min_dist[i];
            inertia += p;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) inertia += __shfl_down(inertia, off, 64);
    if ((tid & 63) == 0) red[tid >> 6] = inertia;
    __syncthreads();
    if (tid == 0) {
        double a = 0.0;
        for (int v = 0; v < BSW / 64; ++v) a += red[v];   // fixed order
        my_part[0] = a;
        my_part[1] = 0.0;
    }
    if (!with_sums) return;

    const int W = 3 * d + 3;              // words per cluster in the partial block: the limbs of d sums, then of the count
    const int WC = 3 * DC + 3;            // words per cluster in LDS (the last three: the count, used by the first dimension chunk)
    const double* __restrict__ f1 = factors;
    const double* __restrict__ f2 = factors + d;
    const double c1 = factors[2 * d], c2 = factors[2 * d + 1];
    u64* my_words = reinterpret_cast<u64*>(my_part + 2);
    for (int k0 = 0; k0 < K; k0 += KC) {
        const int kc = min(KC, K - k0);
        for (int j0 = 0; j0 < d; j0 += DC) {
            const int dc = min(DC, d - j0);
            for (int e = tid; e < kc * WC; e += BSW) acc_lds[e] = 0;
            __syncthreads();
            for (uint32_t i = first; i < n; i += stride) {
                const uint32_t rel = labels[i] - (uint32_t)k0;
                const double wi = w[i];
                if (rel < (uint32_t)kc && wi != 0.0) {             // (a row of weight 0 adds 0 to every word)
                    u64* row = acc_lds + (size_t)rel * WC;
                    for (int j = 0; j < dc; ++j) {
                        u64 w0, w1, w2;
                        const double p = wi * xt[(size_t)(j0 + j) * ldx + i];
                        split_limbs((p * f1[j0 + j]) * f2[j0 + j], w0, w1, w2);
                        atomicAdd(row + 3 * j, w0);
                        atomicAdd(row + 3 * j + 1, w1);
                        atomicAdd(row + 3 * j + 2, w2);
                    }
                    if (j0 == 0) {
                        u64 w0, w1, w2;
                        split_limbs((wi * c1) * c2, w0, w1, w2);
                        atomicAdd(row + 3 * DC, w0);
                        atomicAdd(row + 3 * DC + 1, w1);
                        atomicAdd(row + 3 * DC + 2, w2);
                    }
                }
            }
            __syncthreads();
            for (int e = tid; e < kc * 3 * dc; e += BSW) {
                const int k = e / (3 * dc), v = e - k * 3 * dc;
                my_words[(size_t)(k0 + k) * W + 3 * j0 + v] = acc_lds[(size_t)k * WC + v];
            }
            if (j0 == 0)
                for (int e = tid; e < kc * 3; e += BSW) {
                    const int k = e / 3, v = e - k * 3;
                    my_words[(size_t)(k0 + k) * W + 3 * d + v] = acc_lds[(size_t)k * WC + 3 * DC + v];
                }
            __syncthreads();
        }
    }
}

/// One output element of [inertia_w, n_changed, counts_w(K), sums(K*d)] by one wave, the lanes striding over the workgroups' partial
/// blocks: the inertia by kmeans_reduce_element's lane-strided sums and shuffle tree; counts and coordinate sums as integer sums of the
/// limb words (order-free), converted to double once and scaled back by the two powers of two. out[1] (n_changed: a count of rows,
/// written by the assignment's own reduction) is left alone.
__global__ __launch_bounds__(256) void kmeans_weighted_reduce_kernel(const double* __restrict__ partials, int n_blocks, size_t pstride, int K,
                                                                      int d, int with_sums, const double* __restrict__ factors,
                                                                      double* __restrict__ out)
{
    const int total = 2 + (with_sums ? K * (d + 1) : 0);
    const int e = blockIdx.x * 4 + (threadIdx.x >> 6);        // wave-uniform
    const int lane = threadIdx.x & 63;
    if (e == 0) {
        double v = 0.0;
        for (int b = lane; b < n_blocks; b += 64) v += partials[(size_t)b * pstride];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if (lane == 0) out[0] = v;
        return;
    }
    if (e < 2 || e >= total) return;
    const int W = 3 * d + 3;
    const int k = (e - 2) / (d + 1), j = (e - 2) - k * (d + 1);   // j == d: the count
    const u64* words = reinterpret_cast<const u64*>(partials + 2) + (size_t)k * W + 3 * j;
    u64 w0 = 0, w1 = 0, w2 = 0;
    for (int b = lane; b < n_blocks; b += 64) {
        const u64* p = words + (size_t)b * pstride;
        w0 += p[0];
        w1 += p[1];
        w2 += p[2];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        w0 += __shfl_down(w0, off, 64);
        w1 += __shfl_down(w1, off, 64);
        w2 += __shfl_down(w2, off, 64);
    }
    if (lane == 0) {                                              // (the conversion of kmeans_reduce_kernel)
        w1 += w0 >> 32;  w0 &= 0xffffffffull;
        const long long top = (long long)w2 + (long long)(w1 >> 32);
        w1 &= 0xffffffffull;
        const double v = __builtin_fma((double)top, 0x1p64, __builtin_fma((double)w1, 0x1p32, (double)w0));
        if (j == d) out[2 + k] = (v / factors[2 * d + 1]) / factors[2 * d];
        else out[2 + K + (size_t)k * d + j] = (v / factors[d + j]) / factors[j];
    }
}

inline int weighted_grid(uint32_t n, int num_cus)
{
    int grid = num_cus * 2;                                       // two 1024-thread workgroups per CU, like the unweighted sweep
    const uint32_t need = (n + BSW - 1) / BSW;
    if ((uint32_t)grid > need) grid = (int)(need ? need : 1);
    return grid;
}

}  // namespace

size_t kmeans_weighted_scratch_doubles(int d, int K, int num_cus)
{
    return (size_t)num_cus * 2 * (2 + (size_t)K * (3 * d + 3));
}

int launch_kmeans_weighted(const KmWeightedArgs& a, int num_cus, hipStream_t stream)
{
    const int grid = weighted_grid(a.n, num_cus);
    const size_t pstride = 2 + (size_t)a.K * (3 * a.d + 3);
    if ((size_t)grid * pstride > a.partials_capacity) return -2;
    // as many whole dimensions of all K clusters as fit 64 KB of LDS (two workgroups per CU); if not even one does, chunk the clusters too
    const size_t budget = 64 * 1024 / sizeof(u64);
    const size_t per_cluster = budget / (size_t)a.K;
    int KC = a.K, DC = per_cluster >= 6 ? (int)((per_cluster - 3) / 3) : 0;
    if (DC > a.d) DC = a.d;
    if (DC < 1) {
        DC = 1;
        KC = (int)(budget / 6);
    }
    const size_t smem = a.with_sums ? sizeof(u64) * (size_t)KC * (3 * DC + 3) : 0;
    hipLaunchKernelGGL(kmeans_weighted_update_kernel, dim3(grid), dim3(BSW), smem, stream, a.xt, a.ldx, a.n, a.d, a.labels, a.min_dist,
                       a.weights, a.factors, a.K, KC, DC, a.with_sums, a.partials, pstride);
    const int total = 2 + (a.with_sums ? a.K * (a.d + 1) : 0);
    hipLaunchKernelGGL(kmeans_weighted_reduce_kernel, dim3((total + 3) / 4), dim3(256), 0, stream, a.partials, grid, pstride, a.K, a.d,
                       a.with_sums, a.factors, a.out);
    return grid;
}

}  // namespace mlhip
