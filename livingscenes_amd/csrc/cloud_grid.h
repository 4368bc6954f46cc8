// cloud_grid.h -- scene memory: the voxel grid of cloudmerge.hip and cloudnear.hip, stated once.  The rules are those of
// include/livingscenes_hip.h (ls_cloud_merge_f32, ls_cloud_nearest_f32) and, as NumPy, of tests/merge_oracle.py (cells, transform):
//   pose        y_a = ((R_a0 x_0 + R_a1 x_1) + R_a2 x_2) + t_a in fp32, every product and sum rounded; g == NULL: the row bit for bit
//   cell        c_a = floor(y_a inv) in fp32, clamped to [-2^30, 2^30], as an int; inv = 1.0f / edge formed once on the host; a row with a non-finite
//               coordinate has no cell
//   table       open addressing, 2 n slots for n rows: a cell's walk starts at first_slot and steps by one, wrapping at T
// Every product and sum here is rounded: the including file sets `#pragma clang fp contract(off)` AHEAD of this include (it holds for
// the rest of the translation unit, so this header does not repeat it).
#pragma once
#include <climits>
#include <cmath>
#include <cstdio>

#include "ls_common.h"

namespace ls {
namespace cloud {

constexpr int NO_CELL = INT_MIN;              // [0] of a cell triple: the row has no cell / the slot is empty (cells are clamped to [-2^30, 2^30])
constexpr unsigned NO_SLOT = 0xFFFFFFFFu;     // slot_of[i]: the row is in no slot (no cell, or the table overflowed)
constexpr float CELL_MAX = 1073741824.0f;     // 2^30

// the cell of the row y (NO_CELL thrice: a non-finite coordinate) -> finite?
__device__ __forceinline__ bool cell_of(const float (&y)[3], float inv, int (&c)[3]) {
    const bool finite = isfinite(y[0]) && isfinite(y[1]) && isfinite(y[2]);
    for (int k = 0; k < 3; ++k) c[k] = finite ? (int)fminf(fmaxf(floorf(y[k] * inv), -CELL_MAX), CELL_MAX) : NO_CELL;
    return finite;
}

// a row under the pose g [3,4] (null: the row bit for bit)
__device__ __forceinline__ void pose_row(const float* __restrict__ g, float x0, float x1, float x2, float (&y)[3]) {
    y[0] = x0, y[1] = x1, y[2] = x2;
    if (g)
        for (int r = 0; r < 3; ++r) y[r] = ((g[r * 4 + 0] * x0 + g[r * 4 + 1] * x1) + g[r * 4 + 2] * x2) + g[r * 4 + 3];
}

// the first slot of a cell's probe walk in a table of T slots (T < 2^32).  The high-word product, not %: where a cell lands does not
// change a result, but it sets the probe lengths.
__device__ __forceinline__ long long first_slot(int c0, int c1, int c2, long long T) {
    const unsigned long long hsh = mix64(mix64(((unsigned long long)(unsigned)c0 << 32) | (unsigned)c1) + (unsigned long long)(unsigned)c2);
    return (long long)(((hsh >> 32) * (unsigned long long)T) >> 32);
}

// The claim walk of row `me` with the cell (c0, c1, c2) in the table of T slots from slot t0: an empty slot (-1) is claimed with an integer
// CAS, an occupied one is the cell's iff its occupant has the same cell -- `cell` is the cell array from the base the table's indices
// count from, and a slot's occupant never changes its cell, so all rows of a cell meet in one slot.  -> the slot, with the occupant seen
// there (me: the slot was free, or already mine), or NO_SLOT after T steps.
__device__ __forceinline__ unsigned claim_slot(int* __restrict__ table, long long t0, long long T, const int* __restrict__ cell, int c0, int c1,
                                               int c2, int me, int& occupant) {
    long long s = first_slot(c0, c1, c2, T);
    for (long long step = 0; step < T; ++step) {
        const long long slot = t0 + s;
        occupant = atomicCAS(&table[slot], -1, me);
        if (occupant == -1) occupant = me;
        const int* oc = cell + (long long)occupant * 3;                  // the slot is mine: my own cell
        if ((oc[0] == c0) & (oc[1] == c1) & (oc[2] == c2)) return (unsigned)slot;
        if (++s == T) s = 0;
    }
    return NO_SLOT;
}

// The edge of problem p's grid, checked on the host: finite and positive, with inv = 1.0f / edge -- the one rounding of the definition --
// finite, and where r2 is asked for, r2 = edge * edge finite and positive.  `noun` and `name` are what the messages call the edge.
inline int check_edge(const char* op, int p, const char* noun, const char* name, float edge, float* inv, float* r2 = nullptr) {
    LS_REQUIRE(std::isfinite(edge) && edge > 0.0f, "%s: problem %d: the %s must be finite and > 0, got %g", op, p, noun, (double)edge);
    *inv = 1.0f / edge;
    LS_REQUIRE(std::isfinite(*inv), "%s: problem %d: 1 / %s overflows fp32 (%s %g)", op, p, name, name, (double)edge);
    if (r2) {
        *r2 = edge * edge;
        LS_REQUIRE(std::isfinite(*r2) && *r2 > 0.0f, "%s: problem %d: %s^2 is not a finite positive fp32 (%s %g)", op, p, name, name, (double)edge);
    }
    return LS_OK;
}

// The refusal of a workspace that is missing or smaller than `need`; the message names the size query of `op`, ls_<op>_workspace_bytes,
// with its arguments: P (a batch; 0: a single problem), a, and b (< 0: the query has none).
inline int check_workspace(const char* op, const void* workspace, size_t workspace_bytes, size_t need, int P, long long a, long long b) {
    if (workspace && workspace_bytes >= need) return LS_OK;
    char args[80];
    int n = P > 0 ? snprintf(args, sizeof args, "%d, ", P) : 0;
    n += snprintf(args + n, sizeof args - n, "%lld", a);
    if (b >= 0) snprintf(args + n, sizeof args - n, ", %lld", b);
    set_error("%s: workspace %zu < required %zu (ls_%s_workspace_bytes(%s))", op, workspace ? workspace_bytes : (size_t)0, need, op, args);
    return LS_ERR_WORKSPACE;
}

}  // namespace cloud
}  // namespace ls
