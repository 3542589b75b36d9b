// Sampler of a Gaussian mixture for gfx950: row i (a 64-bit GLOBAL index) of the sample is a pure function of (seed, i) --
//   Philox4x32-10, key (seed lo, seed hi), counter (i lo, i hi, block, 0);  U(lo, hi) = (((hi 2^32 + lo) >> 12) + 1/2) 2^-52;
//   block 0:      label = #{k < K-1 : U(w0, w1) >= t_k}, t_k the normalised prefix sums of the mixing weights (host, fp64);
//   block 1 + p:  u1 = U(w0, w1), u2 = U(w2, w3), r = sqrt(-2 log u1), z_2p = r cospi(2 u2), z_2p+1 = r sinpi(2 u2);
//   x_j = mu_kj + sum_{c <= j} L_k[j][c] z_c, evaluated as acc = mu_j, acc = fma(L_jc, z_c, acc) for c = 0 .. j on every route --
// so the rows do not depend on the grid, the chunking of a call or the number of shards, bit for bit.
//
//   em_sample_kernel<DP, W, LdsTable>  d <= 64, lane = row: the d normals in registers (DP: the padded dimension the loops are
//                                      unrolled for; d itself is a wave-uniform argument), the triangular product in place from
//                                      j = d-1 down, the wave's 64 x d tile through LDS (odd row stride: conflict-free writes) and out
//                                      as contiguous 16 bytes per lane. L_k / mu_k per lane from LDS (LdsTable) or global memory.
//   em_sample_plain_kernel             64 < d <= 4096: the normals go to the output row, the product runs there in place.
// The generator: philox.hpp, on its stream 0.
// Table: [L of component 0 .. (packed lower triangle, row by row: (j, c) at j (j+1)/2 + c) | mu (K x d)]; a tied model holds ONE L.
#include "em_condition_common.hpp"   // the staged tile store
#include "philox.hpp"

namespace mlhip {
namespace {

constexpr int kSampleLdsBytes = 64 * 1024;       // what one workgroup takes at most (as every kernel of this library)
constexpr uint32_t kSampleLdsThresholds = 2048;  // K up to which the label thresholds sit in LDS

/// Row i's component: block 0 against the thresholds (ascending, so the count is the first k with u < t_k).
__device__ __forceinline__ uint32_t draw_label(uint64_t i, uint64_t seed, const double* thresholds, uint32_t K)
{
    const double u = draw_uniform(i, seed, 0u);
    uint32_t label = 0;
    while (label + 1 < K && u >= thresholds[label]) ++label;
    return label;
}

template <int DP, int W, bool LdsTable>
__global__ __launch_bounds__(64 * W) void em_sample_kernel(SampleArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int d = a.d;
    const int S = d | 1;                                         // LDS row stride of the staging tile
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double* stage = sm + (size_t)wave * 64 * S;
    double* after = sm + (size_t)W * 64 * S;
    const bool thr_lds = a.K <= kSampleLdsThresholds;
    if (thr_lds)
        for (uint32_t i = threadIdx.x; i < a.K; i += 64 * W) after[i] = a.thresholds[i];
    double* tab = after + (thr_lds ? a.K : 0);
    if (LdsTable)
        for (size_t i = threadIdx.x; i < a.table_doubles; i += 64 * W) tab[i] = a.table[i];
    __syncthreads();
    const double* thresholds = thr_lds ? after : a.thresholds;
    const size_t mu_offset = a.table_doubles - (size_t)a.K * d;

    const uint64_t tiles = (a.n + 63) / 64;
    for (uint64_t t = (uint64_t)blockIdx.x * W + wave; t < tiles; t += (uint64_t)gridDim.x * W) {
        const uint64_t local = t * 64 + lane;
        const bool live = local < a.n;
        const uint64_t i = a.first_row + local;
        const uint32_t label = draw_label(i, a.seed, thresholds, a.K);
        if (a.labels && live) a.labels[local] = label;
        if (!a.x) continue;

        double z[DP + 1];
#pragma unroll
        for (int p = 0; p < (DP + 1) / 2; ++p)
            if (2 * p < d) draw_pair(i, a.seed, (uint32_t)p, 0u, z[2 * p], z[2 * p + 1]);

        const double* Lk;
        const double* mu;
        if (LdsTable) {
            Lk = tab + (size_t)label * a.l_stride;
            mu = tab + mu_offset + (size_t)label * d;
        } else {
            Lk = a.table + (size_t)label * a.l_stride;
            mu = a.table + mu_offset + (size_t)label * d;
        }
#pragma unroll
        for (int j = DP - 1; j >= 0; --j) {
            if (j < d) {
                double acc = mu[j];
#pragma unroll
                for (int c = 0; c <= j; ++c) acc = __builtin_fma(Lk[j * (j + 1) / 2 + c], z[c], acc);
                z[j] = acc;                                      // (z_j is not read again: rows below j are done)
                stage[lane * S + j] = acc;
            }
        }
        wave_sync();
        const uint64_t rows = a.n - t * 64 < 64 ? a.n - t * 64 : 64;
        move_staged<false>(stage, S, (uint32_t)rows, (uint32_t)d, a.x + t * 64 * (uint64_t)d, lane);
        wave_sync();                                             // (the next tile's stores wait for these reads)
    }
}

__global__ __launch_bounds__(256) void em_sample_plain_kernel(SampleArgs a)
{
    const int d = a.d;
    const size_t mu_offset = a.table_doubles - (size_t)a.K * d;
    for (uint64_t local = (uint64_t)blockIdx.x * 256 + threadIdx.x; local < a.n; local += (uint64_t)gridDim.x * 256) {
        const uint64_t i = a.first_row + local;
        const uint32_t label = draw_label(i, a.seed, a.thresholds, a.K);
        if (a.labels) a.labels[local] = label;
        if (!a.x) continue;
        double* row = a.x + local * (uint64_t)d;
        for (int p = 0; 2 * p < d; ++p) {
            double z0, z1;
            draw_pair(i, a.seed, (uint32_t)p, 0u, z0, z1);
            row[2 * p] = z0;
            if (2 * p + 1 < d) row[2 * p + 1] = z1;
        }
        const double* Lk = a.table + (size_t)label * a.l_stride;
        const double* mu = a.table + mu_offset + (size_t)label * d;
        for (int j = d - 1; j >= 0; --j) {
            const double* Lj = Lk + (size_t)j * (j + 1) / 2;
            double acc = mu[j];
            for (int c = 0; c <= j; ++c) acc = __builtin_fma(Lj[c], row[c], acc);
            row[j] = acc;
        }
    }
}

constexpr int waves_for(int DP) { return DP <= 16 ? 4 : DP <= 32 ? 2 : 1; }

/// LDS bytes of the register tier without / with the table beside the staging tile and the thresholds.
size_t lds_bytes(int d, uint32_t K, size_t table_doubles, bool with_table)
{
    const int DP = padded_dim(d);
    size_t doubles = (size_t)waves_for(DP) * 64 * (size_t)(d | 1);
    if (K <= kSampleLdsThresholds) doubles += K;
    if (with_table) doubles += table_doubles;
    return doubles * sizeof(double);
}

template <int DP>
int launch_t(const SampleArgs& a, int num_cus, hipStream_t stream)
{
    constexpr int W = waves_for(DP);
    const uint64_t tiles = (a.n + 63) / 64;
    uint64_t grid = (tiles + W - 1) / W;
    const uint64_t cap = (uint64_t)(num_cus > 0 ? num_cus : 256) * 4;
    if (grid > cap) grid = cap;
    if (grid == 0) grid = 1;
    const bool lds = a.kernel == kSampleLdsTable;
    const size_t bytes = lds_bytes(a.d, a.K, a.table_doubles, lds);
    if (bytes > (size_t)kSampleLdsBytes) return -1;
    if (lds) hipLaunchKernelGGL((em_sample_kernel<DP, W, true>), dim3((uint32_t)grid), dim3(64 * W), bytes, stream, a);
    else hipLaunchKernelGGL((em_sample_kernel<DP, W, false>), dim3((uint32_t)grid), dim3(64 * W), bytes, stream, a);
    return (int)grid;
}

}  // namespace

int em_sample_route(int d, uint32_t K)
{
    if (d > kMidDim) return kSamplePlain;
    // (a full model's table: K factors and K means -- a tied or diagonal model of the same shape takes the same route)
    const size_t table = (size_t)K * ((size_t)d * (d + 1) / 2 + d);
    if (table > (size_t)kSampleLdsBytes / sizeof(double)) return kSampleGlobalTable;
    return lds_bytes(d, K, table, true) <= (size_t)kSampleLdsBytes ? kSampleLdsTable : kSampleGlobalTable;
}

int launch_em_sample(const SampleArgs& a, int num_cus, hipStream_t stream)
{
    if (a.d < 1 || a.d > kGenericMaxDim || a.K < 1) return -1;
    if (a.n == 0) return 0;
    if (a.kernel == kSamplePlain) {
        if (a.d <= kMidDim) return -1;
        uint64_t grid = (a.n + 255) / 256;
        const uint64_t cap = (uint64_t)(num_cus > 0 ? num_cus : 256) * 8;
        if (grid > cap) grid = cap;
        hipLaunchKernelGGL(em_sample_plain_kernel, dim3((uint32_t)grid), dim3(256), 0, stream, a);
        return (int)grid;
    }
    if (a.d > kMidDim) return -1;
    switch (padded_dim(a.d)) {
    case 1: return launch_t<1>(a, num_cus, stream);
    case 2: return launch_t<2>(a, num_cus, stream);
    case 3: return launch_t<3>(a, num_cus, stream);
    case 4: return launch_t<4>(a, num_cus, stream);
    case 6: return launch_t<6>(a, num_cus, stream);
    case 8: return launch_t<8>(a, num_cus, stream);
    case 12: return launch_t<12>(a, num_cus, stream);
    case 16: return launch_t<16>(a, num_cus, stream);
    case 20: return launch_t<20>(a, num_cus, stream);
    case 24: return launch_t<24>(a, num_cus, stream);
    case 28: return launch_t<28>(a, num_cus, stream);
    case 32: return launch_t<32>(a, num_cus, stream);
    case 40: return launch_t<40>(a, num_cus, stream);
    case 48: return launch_t<48>(a, num_cus, stream);
    case 56: return launch_t<56>(a, num_cus, stream);
    case 64: return launch_t<64>(a, num_cus, stream);
    default: return -1;
    }
}

}  // namespace mlhip
