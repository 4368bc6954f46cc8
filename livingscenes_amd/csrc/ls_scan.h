// ls_scan.h -- the two-level scans: the top level (mise.hip, mcubes.hip, meshmetrics.hip, meshcluster.hip: one workgroup over the sums of the blocks
// below) and, under it, the block-wise scan of a device array that meshmetrics.hip and meshcluster.hip share.
#pragma once
#include "ls_common.h"

namespace ls {

// exclusive scan of blk[0 .. nblk) in place by one workgroup of 1024 threads, any nblk; returns the sum of everything to every thread
template <typename T>
__device__ T scan_top_block(T* blk, int nblk) {
    __shared__ T lds[1024];
    const int tid = threadIdx.x;
    const int per = (nblk + 1023) / 1024;
    const int b0 = tid * per;
    T s = T(0);
    for (int k = 0; k < per; ++k)
        if (b0 + k < nblk) s += blk[b0 + k];
    lds[tid] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const T a = tid >= o ? lds[tid - o] : T(0);
        __syncthreads();
        lds[tid] += a;
        __syncthreads();
    }
    T run = tid > 0 ? lds[tid - 1] : T(0);
    for (int k = 0; k < per; ++k)
        if (b0 + k < nblk) {
            const T v = blk[b0 + k];
            blk[b0 + k] = run;
            run += v;
        }
    return lds[1023];
}

constexpr int SCAN_T = 256, SCAN_ITEMS = 16, SCAN_PER_BLOCK = SCAN_T * SCAN_ITEMS;
constexpr int SCAN_MAX_BLOCKS = 4096;                 // the top-level scan: 1024 threads x 4
constexpr long long SCAN_MAX_N = (long long)SCAN_PER_BLOCK * SCAN_MAX_BLOCKS;
inline long long scan_blocks(long long n) { return (n + SCAN_PER_BLOCK - 1) / SCAN_PER_BLOCK; }

// ------------------------------------------------------------------------------------------------ two-level scan of a device array (count -> offsets, area -> cumsum)
template <typename T>
__device__ T block_scan_excl(T v, T* lds, T& total) {    // SCAN_T threads; exclusive prefix of v in thread order
    const int tid = threadIdx.x;
    lds[tid] = v;
    __syncthreads();
    for (int o = 1; o < SCAN_T; o <<= 1) {
        const T a = tid >= o ? lds[tid - o] : T(0);
        __syncthreads();
        lds[tid] += a;
        __syncthreads();
    }
    total = lds[SCAN_T - 1];
    const T ex = tid > 0 ? lds[tid - 1] : T(0);
    __syncthreads();
    return ex;
}

// the block sums of x[b * SCAN_PER_BLOCK ...] (block b of an n-element array), written to *blk_b
template <typename In, typename T>
__device__ void scan_reduce_block(const In* __restrict__ x, long long n, long long b, T* __restrict__ blk_b) {
    __shared__ T lds[SCAN_T];
    const long long base = b * SCAN_PER_BLOCK + (long long)threadIdx.x * SCAN_ITEMS;
    T s = T(0);
    for (int k = 0; k < SCAN_ITEMS; ++k)
        if (base + k < n) s += (T)x[base + k];
    T total;
    block_scan_excl<T>(s, lds, total);
    if (threadIdx.x == 0) *blk_b = total;
}

template <typename In, typename T>
__global__ __launch_bounds__(SCAN_T) void scan_reduce_kernel(const In* __restrict__ x, long long n, T* __restrict__ blk) {
    scan_reduce_block<In, T>(x, n, blockIdx.x, blk + blockIdx.x);
}

// exclusive scan of the nblk block sums in place (ls_scan.h); total_out = sum of everything
template <typename T>
__global__ __launch_bounds__(1024) void scan_top_kernel(T* __restrict__ blk, int nblk, long long* __restrict__ total_out) {
    const T total = scan_top_block<T>(blk, nblk);
    if (threadIdx.x == 1023) *total_out = (long long)total;
}

// out[i] = prefix of x over block b: exclusive (INCL = false) or inclusive, blk_b (the scanned sum of the blocks before b) added
template <typename In, typename T, bool INCL>
__device__ void scan_apply_block(const In* __restrict__ x, long long n, long long b, T blk_b, T* __restrict__ out) {
    __shared__ T lds[SCAN_T];
    const long long base = b * SCAN_PER_BLOCK + (long long)threadIdx.x * SCAN_ITEMS;
    T v[SCAN_ITEMS];
    T s = T(0);
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        v[k] = base + k < n ? (T)x[base + k] : T(0);
        s += v[k];
    }
    T total;
    T run = block_scan_excl<T>(s, lds, total) + blk_b;
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        if (INCL) run += v[k];
        if (base + k < n) out[base + k] = run;
        if (!INCL) run += v[k];
    }
}

template <typename In, typename T, bool INCL>
__global__ __launch_bounds__(SCAN_T) void scan_apply_kernel(const In* __restrict__ x, long long n, const T* __restrict__ blk,
                                                            T* __restrict__ out) {
    scan_apply_block<In, T, INCL>(x, n, blockIdx.x, blk[blockIdx.x], out);
}

template <typename In, typename T, bool INCL>
void scan(const In* x, long long n, T* blk, T* out, long long* total_out, hipStream_t st) {
    const int nblk = (int)scan_blocks(n);
    hipLaunchKernelGGL((scan_reduce_kernel<In, T>), dim3(nblk), dim3(SCAN_T), 0, st, x, n, blk);
    hipLaunchKernelGGL((scan_top_kernel<T>), dim3(1), dim3(1024), 0, st, blk, nblk, total_out);
    hipLaunchKernelGGL((scan_apply_kernel<In, T, INCL>), dim3(nblk), dim3(SCAN_T), 0, st, x, n, blk, out);
}

}  // namespace ls
