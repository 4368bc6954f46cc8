// ls_ragged.h -- what the ragged batch ops share (meshmetrics.hip: many meshes per call, match.hip: many matching problems per call):
// item p of a batch owns the rows [off[p], off[p+1]) of a packed array, `off` being a host int64 array of count + 1 entries that the entry
// checks and copies into its workspace on the stream; kernels with one thread (or wave) per row find the owner by binary search.
#pragma once
#include <algorithm>
#include <initializer_list>
#include <vector>

#include "ls_common.h"

namespace ls {

// the item p with off[p] <= i < off[p + 1] (i < off[count]; items with an empty range are never the owner)
__device__ __forceinline__ int owner(const long long* __restrict__ off, int count, long long i) {
    int lo = 0, hi = count - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= i) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// off[0] = 0, never decreasing, at most per_max per item, ending at total.  `unit` names an item in the messages ("mesh", "problem").
inline int check_ranges(const char* op, const char* unit, const char* what, int count, const long long* off, long long total, long long per_max) {
    LS_REQUIRE(off, "%s: null %s", op, what);
    LS_REQUIRE(off[0] == 0, "%s: %s[0] is %lld, not 0", op, what, off[0]);
    for (int p = 0; p < count; ++p) {
        LS_REQUIRE(off[p + 1] >= off[p], "%s: %s %d: %s decreases (%lld -> %lld)", op, unit, p, what, off[p], off[p + 1]);
        LS_REQUIRE(off[p + 1] - off[p] <= per_max, "%s: %s %d: %lld rows in %s, at most %lld per %s", op, unit, p, off[p + 1] - off[p], what, per_max,
                   unit);
    }
    LS_REQUIRE(off[count] == total, "%s: %s %d: %s ends at %lld, which disagrees with the total %lld", op, unit, count - 1, what, off[count], total);
    return LS_OK;
}

// the device copy of a batch's offsets: the given arrays of count + 1 int64 back to back (a null array: zeros)
inline std::vector<long long> pack_offsets(int count, std::initializer_list<const long long*> arrays) {
    std::vector<long long> o(arrays.size() * (size_t)(count + 1), 0);
    size_t k = 0;
    for (const long long* a : arrays) {
        if (a) std::copy(a, a + count + 1, o.begin() + k * (size_t)(count + 1));
        ++k;
    }
    return o;
}

// pageable host memory: the copy has read `host` when it returns
inline int upload_offsets(long long* dev, const std::vector<long long>& host, hipStream_t st) {
    LS_HIP_CHECK(hipMemcpyAsync(dev, host.data(), host.size() * sizeof(long long), hipMemcpyHostToDevice, st));
    return LS_OK;
}

}  // namespace ls
