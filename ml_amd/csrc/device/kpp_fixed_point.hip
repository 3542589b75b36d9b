// The fixed-point K-means++ draw (FixedPointKPP, include/ML/Clustering.hpp) on the resident block: three kernels per centroid.
//   update:   one pass over X (dimension-major) -- the squared distance of every row to the newest centroid (ascending-j chain
//             s = fma(x_j - c_j, x_j - c_j, s), the bits of mlhip_min_squared_distances), the running minimum written back to w,
//             and the largest new weight's bit pattern (non-negative doubles order like their bits; a non-finite weight has bits
//             >= 0x7ff0...) per workgroup, folded by one workgroup into one 64-bit slot;
//   quantise: one pass over w -- q_i = floor(w_i 2^(52 - E)) < 2^52 (E: the largest frexp exponent of the whole sample, from the
//             ranks' exchange), split into a 20-bit high and a 32-bit low part whose block sums are formed with integer adds only
//             (per block of 4096 rows: below 2^32 and 2^44), folded by one workgroup into the rank's two totals -- exact, whatever
//             the order of the additions (one slot per workgroup, not atomics: 24k workgroups adding into one address serialise);
//   locate:   one workgroup -- a scan of the block sums finds the block in which the cumulative sum first exceeds the target, a
//             scan over that block's 4096 rows the row itself.
#include "device.hpp"
#include "fixed_point.hpp"

namespace mlhip {
namespace {

using fixed_point::u128;
typedef unsigned long long ull;

constexpr int kFpChunk = 4096;               // rows per workgroup of the update and quantise passes
constexpr int kFpPer = kFpChunk / 256;       // rows per thread

/// Block-wide reduction of one 64-bit value per thread of a 256-thread block (result valid in thread 0).
template <class Op> __device__ __forceinline__ ull block_reduce_256(ull v, ull* red, Op op)
{
    red[threadIdx.x] = v;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] = op(red[threadIdx.x], red[threadIdx.x + off]);
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(256) void fp_kpp_update_kernel(const double* __restrict__ xt, size_t ldx, int d, uint32_t n,
                                                             const double* __restrict__ centroid, int first, double* __restrict__ w,
                                                             ull* __restrict__ bmax)
{
    __shared__ ull red[256];
    const uint32_t base = blockIdx.x * (uint32_t)kFpChunk + threadIdx.x;
    // the rows of this thread (clamped to the last row: the loads stay inside the block, the extra results are dropped)
    uint32_t row[kFpPer];
    double s[kFpPer];
#pragma unroll
    for (int t = 0; t < kFpPer; ++t) {
        row[t] = min(base + (uint32_t)t * 256u, n - 1);
        s[t] = 0.0;
    }
    // ascending j, kFpPer independent chains: kFpPer loads in flight per thread and step
    for (int j = 0; j < d; ++j) {
        const double cj = centroid[j];
        const double* col = xt + (size_t)j * ldx;
#pragma unroll
        for (int t = 0; t < kFpPer; ++t) {
            const double e = col[row[t]] - cj;
            s[t] = __builtin_fma(e, e, s[t]);
        }
    }
    ull m = 0;
#pragma unroll
    for (int t = 0; t < kFpPer; ++t) {
        const uint32_t i = base + (uint32_t)t * 256u;
        if (i < n) {
            const double v = first ? s[t] : fmin(w[i], s[t]);
            w[i] = v;
            const ull bits = (ull)__double_as_longlong(v) & 0x7fffffffffffffffull;
            m = bits > m ? bits : m;
        }
    }
    m = block_reduce_256(m, red, [](ull a, ull b) { return a > b ? a : b; });
    if (threadIdx.x == 0) bmax[blockIdx.x] = m;
}

__global__ __launch_bounds__(256) void fp_kpp_quantise_kernel(const double* __restrict__ w, uint32_t n, int E, ull* __restrict__ bsum)
{
    __shared__ ull red[256];
    const uint32_t base = blockIdx.x * (uint32_t)kFpChunk + threadIdx.x;
    ull hi = 0, lo = 0;
#pragma unroll
    for (int t = 0; t < kFpPer; ++t) {
        const uint32_t i = base + (uint32_t)t * 256u;
        if (i < n) {
            const uint64_t q = fixed_point::quantise((uint64_t)__double_as_longlong(w[i]) & 0x7fffffffffffffffull, E);
            hi += q >> 32;
            lo += q & 0xffffffffull;
        }
    }
    const auto add = [](ull a, ull b) { return a + b; };
    hi = block_reduce_256(hi, red, add);
    __syncthreads();                                  // (every thread has read red[0])
    lo = block_reduce_256(lo, red, add);
    if (threadIdx.x == 0) {
        bsum[2 * (size_t)blockIdx.x] = hi;
        bsum[2 * (size_t)blockIdx.x + 1] = lo;
    }
}

/// One workgroup: out[0] = max_b v[b] (sum = 0), or out[0] = sum_b v[2b], out[1] = sum_b v[2b + 1] (sum = 1); integers, so exact.
__global__ __launch_bounds__(1024) void fp_kpp_fold_kernel(const ull* __restrict__ v, int nb, int sum, ull* __restrict__ out)
{
    __shared__ ull a[1024], b[1024];
    const int tid = threadIdx.x;
    ull x = 0, y = 0;
    for (int i = tid; i < nb; i += 1024) {
        if (sum) {
            x += v[2 * (size_t)i];
            y += v[2 * (size_t)i + 1];
        } else {
            x = v[i] > x ? v[i] : x;
        }
    }
    a[tid] = x;
    b[tid] = y;
    __syncthreads();
    for (int off = 512; off > 0; off >>= 1) {
        if (tid < off) {
            a[tid] = sum ? a[tid] + a[tid + off] : (a[tid + off] > a[tid] ? a[tid + off] : a[tid]);
            b[tid] += b[tid + off];
        }
        __syncthreads();
    }
    if (tid == 0) {
        out[0] = a[0];
        if (sum) out[1] = b[0];
    }
}

__device__ __forceinline__ u128 block_value(const ull* bsum, int b) { return ((u128)bsum[2 * (size_t)b] << 32) + bsum[2 * (size_t)b + 1]; }

/// out[0] = row0 + the smallest local row i with q_0 + ... + q_i > target (0 <= target < this rank's total: exactly one row).
__global__ __launch_bounds__(1024) void fp_kpp_locate_kernel(const double* __restrict__ w, uint32_t n, int E, const ull* __restrict__ bsum,
                                                              int nb, ull target_lo, ull target_hi, ull row0, ull* __restrict__ out)
{
    __shared__ u128 scan[1024];
    __shared__ ull scan_rows[1024];
    __shared__ int found_block;
    __shared__ ull found_rest;
    const int tid = threadIdx.x;
    const u128 target = ((u128)target_hi << 64) | target_lo;
    if (tid == 0) found_block = -1;
    // 1. the block: every thread sums a contiguous segment of the block sums; exclusive scan of the segment sums
    const int seg = (nb + 1023) / 1024;
    const int b0 = min(nb, tid * seg), b1 = min(nb, b0 + seg);
    u128 acc = 0;
    for (int b = b0; b < b1; ++b) acc += block_value(bsum, b);
    scan[tid] = acc;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const u128 add = tid >= off ? scan[tid - off] : (u128)0;
        __syncthreads();
        scan[tid] += add;
        __syncthreads();
    }
    u128 pre = scan[tid] - acc;
    if (pre <= target && target < pre + acc) {       // (one thread: the segments tile [0, total))
        for (int b = b0; b < b1; ++b) {
            const u128 v = block_value(bsum, b);
            if (target < pre + v) {
                found_block = b;
                found_rest = (ull)(target - pre);    // < v < 2^64
                break;
            }
            pre += v;
        }
    }
    __syncthreads();
    if (found_block < 0) return;                     // (target beyond the total: out[0] keeps the caller's sentinel)
    // 2. the row inside that block: four consecutive rows per thread, exclusive scan of the thread sums (all below 2^64)
    const uint32_t first = (uint32_t)found_block * (uint32_t)kFpChunk + 4u * (uint32_t)tid;
    const ull rest = found_rest;
    ull q[4], qs = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t i = first + (uint32_t)k;
        q[k] = i < n ? fixed_point::quantise((uint64_t)__double_as_longlong(w[i]) & 0x7fffffffffffffffull, E) : 0;
        qs += q[k];
    }
    scan_rows[tid] = qs;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const ull add = tid >= off ? scan_rows[tid - off] : 0;
        __syncthreads();
        scan_rows[tid] += add;
        __syncthreads();
    }
    ull c = scan_rows[tid] - qs;
    if (c <= rest && rest < c + qs) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            c += q[k];
            if (c > rest) { out[0] = row0 + first + (uint32_t)k; break; }
        }
    }
}

}  // namespace

int fp_kpp_blocks(uint32_t n) { return (int)((n + kFpChunk - 1) / kFpChunk); }

void launch_fp_kpp_update(const double* xt, size_t ldx, int d, uint32_t n, const double* centroid, int first, double* w, uint64_t* bmax,
                          uint64_t* wmax, hipStream_t stream)
{
    if (n == 0) return;
    const int nb = fp_kpp_blocks(n);
    hipLaunchKernelGGL(fp_kpp_update_kernel, dim3(nb), dim3(256), 0, stream, xt, ldx, d, n, centroid, first, w, reinterpret_cast<ull*>(bmax));
    hipLaunchKernelGGL(fp_kpp_fold_kernel, dim3(1), dim3(1024), 0, stream, reinterpret_cast<const ull*>(bmax), nb, 0, reinterpret_cast<ull*>(wmax));
}

void launch_fp_kpp_quantise(const double* w, uint32_t n, int E, uint64_t* bsum, uint64_t* total, hipStream_t stream)
{
    if (n == 0) return;
    const int nb = fp_kpp_blocks(n);
    hipLaunchKernelGGL(fp_kpp_quantise_kernel, dim3(nb), dim3(256), 0, stream, w, n, E, reinterpret_cast<ull*>(bsum));
    hipLaunchKernelGGL(fp_kpp_fold_kernel, dim3(1), dim3(1024), 0, stream, reinterpret_cast<const ull*>(bsum), nb, 1, reinterpret_cast<ull*>(total));
}

void launch_fp_kpp_locate(const double* w, uint32_t n, int E, const uint64_t* bsum, uint64_t target_lo, uint64_t target_hi, uint64_t row0,
                          uint64_t* out, hipStream_t stream)
{
    if (n == 0) return;
    hipLaunchKernelGGL(fp_kpp_locate_kernel, dim3(1), dim3(1024), 0, stream, w, n, E, reinterpret_cast<const ull*>(bsum), fp_kpp_blocks(n),
                       (ull)target_lo, (ull)target_hi, (ull)row0, reinterpret_cast<ull*>(out));
}

}  // namespace mlhip
