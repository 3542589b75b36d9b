// Silhouette values: for every evaluated row i the sums D_ic = sum_{j in cluster c} |x_i - x_j| over ALL columns j of the block,
// the exact O(N^2 d) pair loop in the direct form -- z = x_i - x_j (one rounding), q = z_0 z_0, q = fma(z_j, z_j, q) ascending,
// sqrt(q) correctly rounded. Every term is >= 0: no cancellation wherever the data sit (the expansion |x|^2 + |y|^2 - 2 x.y loses
// 3e-5 of the silhouette on a sample shifted by 1e6).
//
// Order of the sums (mlhip.h): the columns are taken cluster-sorted (a stable counting sort of the rows by label), every cluster's
// run is cut into chunks of kSilhouetteChunk columns, the distances of a chunk are added one after the other, and the chunk sums of
// a cluster in ascending order (silhouette_fold_kernel). No grid, tile or switch enters: a row's result is a function of the data,
// the labels and the block alone.
//
// Mapping: lane = evaluated row, its padded coordinates in 2 P VGPRs; a workgroup of four waves owns (256 evaluated rows) x (one
// chunk) and walks the units chunk-major with a grid stride, so the workgroups running together read the same chunks. A column is a
// wave-uniform operand. Two feeds, both from the cluster-sorted sample-major copy the runtime gathers once per call:
//   scalar -- the column's P doubles come as scalar loads (as the scalar-fed E-step feeds its records, em_estep.hip): an SGPR pair
//             is the second operand of the subtraction, no LDS, no barrier;
//   LDS    -- the workgroup copies the chunk (256 P doubles, 64 KB at P = 32) into LDS, coalesced, and every lane reads the same
//             address (a broadcast, 16 bytes per read).
// What binds the loop is what em_diag.hip's header says of its own: per (column, dimension) 2 fp64 VALU operations against 8 bytes
// of operand feed; behind them the square root's sequence and one addition per column. profiles/silhouette_timing.txt has what
// was measured and what was not.
//
// The plain tier (d up to 4096, MLHIP_SILHOUETTE=plain) walks a lane's coordinates from memory in the same operation order: the
// padded coordinates of the register tier are +0.0 on both sides and add fma(0, 0, q) = q, so both tiers give the same bits.
#include "device.hpp"
#include "silhouette_finish.hpp"

namespace mlhip {
namespace {

#pragma clang fp contract(off)

/// One distance in the order mlhip.h fixes: x holds the lane's row, col the column, P coordinates each.
template <int P, class Col>
__device__ __forceinline__ double distance_to(const double (&x)[P], Col col)
{
    double z = x[0] - col[0];
    double q = z * z;
#pragma unroll
    for (int j = 1; j < P; ++j) {
        z = x[j] - col[j];
        q = __builtin_fma(z, z, q);
    }
    return __builtin_sqrt(q);
}

template <int P, bool LDS>
__global__ __launch_bounds__(256) void silhouette_kernel(const double* __restrict__ rows, size_t ldm, uint32_t m,
                                                         const double* __restrict__ cols, const uint32_t* __restrict__ chunk_first,
                                                         const uint32_t* __restrict__ chunk_len, uint32_t n_chunks, uint32_t row_tiles,
                                                         double* __restrict__ partials, size_t ldp)
{
    extern __shared__ double staged[];                            // LDS feed: kSilhouetteChunk x P
    const uint64_t units = (uint64_t)n_chunks * row_tiles;
    for (uint64_t u = blockIdx.x; u < units; u += gridDim.x) {
        const uint32_t t = (uint32_t)(u / row_tiles), tile = (uint32_t)(u % row_tiles);
        const uint32_t r = tile * kSilhouetteRowTile + threadIdx.x;
        const uint32_t rr = r < m ? r : m - 1;                    // (lanes beyond the block compute on its last row and write nothing)
        double x[P];
#pragma unroll
        for (int j = 0; j < P; ++j) x[j] = rows[(size_t)j * ldm + rr];
        const uint32_t first = chunk_first[t], len = chunk_len[t];
        const double* __restrict__ col = cols + (size_t)first * P;
        double acc = 0.0;                                         // (0 + the first distance is that distance)
        if (LDS) {
            __syncthreads();                                      // (the previous unit's reads are done)
            for (uint32_t i = threadIdx.x; i < len * (uint32_t)P; i += 256) staged[i] = col[i];
            __syncthreads();
            for (uint32_t c = 0; c < len; ++c) acc += distance_to<P>(x, staged + (size_t)c * P);
        } else {
#pragma unroll 2
            for (uint32_t c = 0; c < len; ++c) acc += distance_to<P>(x, col + (size_t)c * P);
        }
        if (r < m) partials[(size_t)t * ldp + r] = acc;
    }
}

__global__ __launch_bounds__(256) void silhouette_plain_kernel(const double* __restrict__ rows, size_t ldm, uint32_t m,
                                                               const double* __restrict__ cols, int d,
                                                               const uint32_t* __restrict__ chunk_first,
                                                               const uint32_t* __restrict__ chunk_len, uint32_t n_chunks, uint32_t row_tiles,
                                                               double* __restrict__ partials, size_t ldp)
{
    const uint64_t units = (uint64_t)n_chunks * row_tiles;
    for (uint64_t u = blockIdx.x; u < units; u += gridDim.x) {
        const uint32_t t = (uint32_t)(u / row_tiles), tile = (uint32_t)(u % row_tiles);
        const uint32_t r = tile * kSilhouetteRowTile + threadIdx.x;
        const uint32_t rr = r < m ? r : m - 1;
        const uint32_t first = chunk_first[t], len = chunk_len[t];
        const double* __restrict__ x = rows + rr;
        double acc = 0.0;
        for (uint32_t c = 0; c < len; ++c) {
            const double* __restrict__ col = cols + (size_t)(first + c) * d;
            double z = x[0] - col[0];
            double q = z * z;
            for (int j = 1; j < d; ++j) {
                z = x[(size_t)j * ldm] - col[j];
                q = __builtin_fma(z, z, q);
            }
            acc += __builtin_sqrt(q);
        }
        if (r < m) partials[(size_t)t * ldp + r] = acc;
    }
}

__global__ __launch_bounds__(256) void silhouette_fold_kernel(const double* __restrict__ partials, size_t ldp, uint32_t m, uint32_t K,
                                                              const uint32_t* __restrict__ cluster_chunks, const uint32_t* __restrict__ counts,
                                                              const uint32_t* __restrict__ own, double* __restrict__ a_out,
                                                              double* __restrict__ b_out, double* __restrict__ s_out,
                                                              double* __restrict__ sums, size_t lds)
{
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r >= m) return;
    SilhouetteFinish f;
    const uint32_t mine = sums ? 0 : own[r];
    f.begin(mine);
    for (uint32_t c = 0; c < K; ++c) {
        const uint32_t from = cluster_chunks[c], to = cluster_chunks[c + 1];
        double sum = 0.0;
        for (uint32_t t = from; t < to; ++t) sum += partials[(size_t)t * ldp + r];
        if (sums) sums[(size_t)c * lds + r] = sum;
        else f.add(c, (double)counts[c], sum);
    }
    if (sums) return;
    double a, b, s;
    f.end((double)counts[mine], a, b, s);
    if (a_out) a_out[r] = a;
    if (b_out) b_out[r] = b;
    if (s_out) s_out[r] = s;
}

__global__ __launch_bounds__(256) void silhouette_gather_columns_kernel(const double* __restrict__ xt, size_t ldx, int d,
                                                                        const uint32_t* __restrict__ order, uint32_t n,
                                                                        double* __restrict__ cols, int stride)
{
    const uint64_t total = (uint64_t)n * (uint32_t)stride;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) {
        const uint32_t c = (uint32_t)(i / (uint32_t)stride);
        const int j = (int)(i % (uint32_t)stride);
        cols[i] = j < d ? xt[(size_t)j * ldx + order[c]] : 0.0;
    }
}

__global__ __launch_bounds__(256) void silhouette_gather_rows_kernel(const double* __restrict__ xt, size_t ldx, int d,
                                                                     const uint32_t* __restrict__ index, uint32_t m,
                                                                     double* __restrict__ rows, size_t ldm, int pad)
{
    const uint64_t total = (uint64_t)m * (uint32_t)pad;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) {
        const int j = (int)(i / m);
        const uint32_t r = (uint32_t)(i % m);
        rows[(size_t)j * ldm + r] = j < d ? xt[(size_t)j * ldx + index[r]] : 0.0;
    }
}

uint32_t copy_grid(uint64_t total)
{
    const uint64_t blocks = (total + 255) / 256;
    return (uint32_t)(blocks < 1 ? 1 : blocks > 65536 ? 65536 : blocks);
}

template <int P>
void launch_p(const SilhouetteArgs& a, uint32_t grid, uint32_t row_tiles, hipStream_t stream)
{
    if (a.feed == kSilhouetteLdsFeed)
        hipLaunchKernelGGL((silhouette_kernel<P, true>), dim3(grid), dim3(256), sizeof(double) * kSilhouetteChunk * P, stream, a.rows, a.ldm,
                           a.m, a.cols, a.chunk_first, a.chunk_len, a.n_chunks, row_tiles, a.partials, a.ldp);
    else
        hipLaunchKernelGGL((silhouette_kernel<P, false>), dim3(grid), dim3(256), 0, stream, a.rows, a.ldm, a.m, a.cols, a.chunk_first,
                           a.chunk_len, a.n_chunks, row_tiles, a.partials, a.ldp);
}

}  // namespace

int silhouette_tier(int d) { return d <= kSilhouetteMaxRegisters ? kSilhouetteRegisters : kSilhouettePlain; }

int silhouette_pad(int kernel, int d)
{
    if (kernel != kSilhouetteRegisters) return d;
    return d <= 2 ? 2 : d <= 4 ? 4 : d <= 8 ? 8 : d <= 16 ? 16 : d <= kSilhouetteMaxRegisters ? 32 : -1;
}

void launch_silhouette_gather_columns(const double* xt, size_t ldx, int d, const uint32_t* order, uint32_t n, double* cols, int stride,
                                      hipStream_t stream)
{
    if (!n) return;
    hipLaunchKernelGGL(silhouette_gather_columns_kernel, dim3(copy_grid((uint64_t)n * stride)), dim3(256), 0, stream, xt, ldx, d, order, n,
                       cols, stride);
}

void launch_silhouette_gather_rows(const double* xt, size_t ldx, int d, const uint32_t* index, uint32_t m, double* rows, size_t ldm, int pad,
                                   hipStream_t stream)
{
    if (!m) return;
    hipLaunchKernelGGL(silhouette_gather_rows_kernel, dim3(copy_grid((uint64_t)m * pad)), dim3(256), 0, stream, xt, ldx, d, index, m, rows,
                       ldm, pad);
}

int launch_silhouette(const SilhouetteArgs& a, int num_cus, hipStream_t stream)
{
    if (a.d < 1 || a.d > kGenericMaxDim) return -1;
    if (!a.m || !a.n_chunks) return 0;
    const uint32_t row_tiles = (a.m + kSilhouetteRowTile - 1) / kSilhouetteRowTile;
    const uint64_t units = (uint64_t)a.n_chunks * row_tiles;
    uint64_t grid = a.grid > 0 ? (uint64_t)a.grid : (uint64_t)(num_cus > 0 ? num_cus : 256) * 8;
    if (grid > units) grid = units;
    if (a.kernel == kSilhouettePlain) {
        hipLaunchKernelGGL(silhouette_plain_kernel, dim3((uint32_t)grid), dim3(256), 0, stream, a.rows, a.ldm, a.m, a.cols, a.d, a.chunk_first,
                           a.chunk_len, a.n_chunks, row_tiles, a.partials, a.ldp);
        return (int)grid;
    }
    switch (silhouette_pad(kSilhouetteRegisters, a.d)) {
    case 2: launch_p<2>(a, (uint32_t)grid, row_tiles, stream); break;
    case 4: launch_p<4>(a, (uint32_t)grid, row_tiles, stream); break;
    case 8: launch_p<8>(a, (uint32_t)grid, row_tiles, stream); break;
    case 16: launch_p<16>(a, (uint32_t)grid, row_tiles, stream); break;
    case 32: launch_p<32>(a, (uint32_t)grid, row_tiles, stream); break;
    default: return -1;
    }
    return (int)grid;
}

void launch_silhouette_fold(const SilhouetteFoldArgs& a, hipStream_t stream)
{
    if (!a.m) return;
    hipLaunchKernelGGL(silhouette_fold_kernel, dim3((a.m + 255) / 256), dim3(256), 0, stream, a.partials, a.ldp, a.m, a.K, a.cluster_chunks,
                       a.counts, a.own, a.a_out, a.b_out, a.s_out, a.sums, a.lds);
}

}  // namespace mlhip
