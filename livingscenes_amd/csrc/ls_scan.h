// ls_scan.h -- the top level of the two-level scans (mise.hip, mcubes.hip, meshmetrics.hip): one workgroup over the sums of the blocks below.
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

}  // namespace ls
