// The sums every K-means route shares: exact fixed-point limb accumulation and the fixed-order workgroup sums of a partial block's
// [inertia, n_changed]. Users: the assignment kernel, both update sweeps and the reduction of kmeans.hip, kmeans_mfma.hip,
// kmeans_resident.hip (limbs), big_dim.hip and generic_dim.hip (workgroup sums). Everything here is __forceinline__: the kernels are
// built with -ffp-contract=fast-honor-pragmas, so what is fused is decided in the caller, after inlining, under the caller's pragmas.
#pragma once

namespace mlhip {

typedef unsigned long long u64;

/// t (|t| < 2^94, only the integer part is kept) -> limbs: t = i2 * 2^64 + u1 * 2^32 + u0 (+ dropped fraction), with
/// u0, u1 in [0, 2^32). The limbs of many samples are summed with 64-bit INTEGER atomics: integer addition is associative,
/// so the sums do not depend on the order in which lanes, waves, workgroups or GPUs contribute.
__device__ __forceinline__ void split_limbs(double t, u64& w0, u64& w1, u64& w2)
{
    const double h2 = floor(t * 0x1p-64);
    const double r = __builtin_fma(-h2, 0x1p64, t);         // exact, in [0, 2^64)
    const double h1 = floor(r * 0x1p-32);
    const double l = __builtin_fma(-h1, 0x1p32, r);          // exact, in [0, 2^32)
    w2 = (u64)(long long)(int)h2;                            // |h2| < 2^30
    w1 = (u64)(unsigned)h1;
    w0 = (u64)(unsigned)l;                                   // truncates the fraction below one unit
}

/// The limbs of t added to limb triple j of an accumulator row (LDS or global memory): words 3j, 3j + 1, 3j + 2.
__device__ __forceinline__ void add_limbs(u64* row, int j, double t)
{
    u64 w0, w1, w2;
    split_limbs(t, w0, w1, w2);
    atomicAdd(row + 3 * j, w0);
    atomicAdd(row + 3 * j + 1, w1);
    atomicAdd(row + 3 * j + 2, w2);
}

/// Summed limb words -> double, rounded once: the carries go up (w0 -> w1 -> the signed top), then two fused multiply-adds.
__device__ __forceinline__ double limbs_to_double(u64 w0, u64 w1, u64 w2)
{
    w1 += w0 >> 32;  w0 &= 0xffffffffull;
    const long long top = (long long)w2 + (long long)(w1 >> 32);
    w1 &= 0xffffffffull;
    return __builtin_fma((double)top, 0x1p64, __builtin_fma((double)w1, 0x1p32, (double)w0));
}

/// The waves' sums of a workgroup of NW waves -> my_part[0] (inertia) and my_part[1] (n_changed) in a FIXED order: the waves ascending
/// from +0.0 (no partial is -0: every sum starts at +0.0 and adds squares or counts, so 0.0 + r0 has r0's bits). Lane 0 of every wave
/// holds its wave's sums. WITH_CHANGED = false: the inertia alone, my_part[1] = 0. `red`: 2 NW doubles of the kernel's LDS (NW).
template <int NW, bool WITH_CHANGED = true>
__device__ __forceinline__ void fold_wave_sums(double inertia, double changed, double* red, double* my_part)
{
    const int tid = threadIdx.x;
    if ((tid & 63) == 0) {
        red[tid >> 6] = inertia;
        if (WITH_CHANGED) red[NW + (tid >> 6)] = changed;
    }
    __syncthreads();
    if (tid == 0) {
        double a = 0.0, b = 0.0;
        for (int w = 0; w < NW; ++w) {                       // fixed order
            a += red[w];
            if (WITH_CHANGED) b += red[NW + w];
        }
        my_part[0] = a;
        my_part[1] = b;
    }
}

/// The lanes' contributions -> my_part[0], my_part[1]: the shuffle tree of each wave, then fold_wave_sums. (kmeans_assign_kernel and
/// kmeans_mfma_kernel spell the tree out and call fold_wave_sums: with the tree inlined from here, the compiler's choices in their
/// sample loops shift and some instantiations come out with other registers.)
template <int NW, bool WITH_CHANGED = true>
__device__ __forceinline__ void fold_block_sums(double inertia, double changed, double* red, double* my_part)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        inertia += __shfl_down(inertia, off, 64);
        if (WITH_CHANGED) changed += __shfl_down(changed, off, 64);
    }
    fold_wave_sums<NW, WITH_CHANGED>(inertia, changed, red, my_part);
}

}  // namespace mlhip
