// cloudmerge.hip -- scene memory: the cloud an instance keeps (A) and a registered new observation of it (B) merged on a voxel grid, first
// point of a cell wins.  The definition is in include/livingscenes_hip.h (ls_cloud_merge_f32) and, as NumPy, in tests/merge_oracle.py; the
// pose, the cell, the table and its claim walk are those of cloud_grid.h.  What this file adds:
//   candidates  the rows of A as given, then the rows of B under the pose g
//   keep        candidate i is kept iff no candidate j < i of its problem has the same cell triple
//   output      the kept candidates of every problem back to back in ascending candidate order: point, candidate index, offsets
// Method: a table of 2 n_p slots per problem holds candidate indices.  After the claim walk a thread lowers its cell's slot to its own
// index (atomicMin): which candidate claimed a slot depends on the race, the minimum it ends with does not.  Then flag, scan (ls_scan.h),
// scatter.  Integer atomics only: a problem's output is the same bits alone, in any batch and in any run.  Every kernel is written once,
// for a problem locator (OneCloud / RaggedClouds, as the meshes of meshcluster.hip); the number of launches does not depend on P.
#include <climits>
#include <cmath>
#include <vector>

#include "ls_common.h"
#include "ls_ragged.h"
#include "ls_scan.h"

// the arithmetic of the definition as written: no contraction of a * b + c into an fma anywhere in this file
#pragma clang fp contract(off)
#include "cloud_grid.h"

namespace ls {
namespace cmg {
using namespace cloud;

// ------------------------------------------------------------------------------------------------ which problem: one, or one of a ragged batch
struct CloudRef {
    const float* A;
    long long a;
    const float* B;
    long long b;
    const float* g;        // [3,4] or null
    float inv;
    long long c0;          // global index of the problem's first candidate
    long long t0, T;       // its table: first slot, slots (2 (a + b))
};

struct OneCloud {
    const float* A;
    long long a;
    const float* B;
    long long b;
    const float* g;
    float inv;
    __device__ long long candidates() const { return a + b; }
    __device__ int cand_owner(long long) const { return 0; }
    __device__ long long first(int p) const { return p == 0 ? 0 : a + b; }   // p in [0, P]
    __device__ CloudRef cloud(int) const { return {A, a, B, b, g, inv, 0, 0, 2 * (a + b)}; }
};

enum { OFF_A = 0, OFF_B, OFF_C, OFF_ARRAYS };   // the device copy of a batch's offsets: rows of A, rows of B, candidates

struct RaggedClouds {
    const float* A;
    const float* B;
    const float* g;            // [P,3,4] or null
    const long long* offs;
    const float* inv;          // [P]
    int P;
    long long n_total;
    __device__ const long long* off(int k) const { return offs + (size_t)k * (P + 1); }
    __device__ long long candidates() const { return n_total; }
    __device__ int cand_owner(long long i) const { return owner(off(OFF_C), P, i); }
    __device__ long long first(int p) const { return off(OFF_C)[p]; }
    __device__ CloudRef cloud(int p) const {
        const long long *ao = off(OFF_A), *bo = off(OFF_B), *co = off(OFF_C);
        return {A + ao[p] * 3, ao[p + 1] - ao[p], B + bo[p] * 3, bo[p + 1] - bo[p], g ? g + (size_t)p * 12 : nullptr, inv[p],
                co[p], 2 * co[p], 2 * (co[p + 1] - co[p])};
    }
};

// candidate i of the problem: a row of A as it is, or a row of B under g
__device__ __forceinline__ void candidate(const CloudRef& C, long long i, float (&y)[3]) {
    if (i < C.a) {
        for (int k = 0; k < 3; ++k) y[k] = C.A[i * 3 + k];
        return;
    }
    const float* __restrict__ x = C.B + (i - C.a) * 3;
    pose_row(C.g, x[0], x[1], x[2], y);
}

// cell [n,3]: the candidates' cells (NO_CELL in [0]: none)
template <class Clouds>
__global__ __launch_bounds__(256) void cell_kernel(Clouds L, int* __restrict__ cell) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= L.candidates()) return;
    const CloudRef C = L.cloud(L.cand_owner(i));
    float y[3];
    candidate(C, i - C.c0, y);
    int c[3];
    cell_of(y, C.inv, c);
    for (int k = 0; k < 3; ++k) cell[i * 3 + k] = c[k];
}

// the table of a problem: slot s holds the lowest LOCAL index seen so far of the candidates of one cell (-1: free).  A problem has at most
// n_p cells for 2 n_p slots.
template <class Clouds>
__global__ __launch_bounds__(256) void hash_kernel(Clouds L, const int* __restrict__ cell, int* __restrict__ table, unsigned* __restrict__ slot_of,
                                                   int* __restrict__ status) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= L.candidates()) return;
    const int c0 = cell[i * 3 + 0], c1 = cell[i * 3 + 1], c2 = cell[i * 3 + 2];
    if (c0 == NO_CELL) {
        slot_of[i] = NO_SLOT;
        return;
    }
    const int p = L.cand_owner(i);
    const CloudRef C = L.cloud(p);
    const int me = (int)(i - C.c0);
    int occupant;
    const unsigned found = claim_slot(table, C.t0, C.T, cell + C.c0 * 3, c0, c1, c2, me, occupant);
    if (found != NO_SLOT && occupant > me) atomicMin(&table[found], me);   // a slot's index only ever falls: below me already, nothing to do
    slot_of[i] = found;
    if (found == NO_SLOT) status[p] = LS_ERR_WORKSPACE;
}

// keep[i]: candidate i is the lowest index of its cell
template <class Clouds>
__global__ __launch_bounds__(256) void keep_kernel(Clouds L, const int* __restrict__ table, const unsigned* __restrict__ slot_of,
                                                   int* __restrict__ keep) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= L.candidates()) return;
    const unsigned s = slot_of[i];
    keep[i] = s != NO_SLOT && (long long)table[s] == i - L.first(L.cand_owner(i)) ? 1 : 0;
}

// the kept candidates at their rank pos[i] (the exclusive scan of keep): point and local candidate index
template <class Clouds>
__global__ __launch_bounds__(256) void scatter_kernel(Clouds L, const int* __restrict__ keep, const int* __restrict__ pos, float* __restrict__ out_pts,
                                                      int* __restrict__ out_src) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= L.candidates() || !keep[i]) return;
    const CloudRef C = L.cloud(L.cand_owner(i));
    float y[3];
    candidate(C, i - C.c0, y);
    const long long o = pos[i];
    for (int k = 0; k < 3; ++k) out_pts[o * 3 + k] = y[k];
    out_src[o] = (int)(i - C.c0);
}

// out_off[p] = the rank of problem p's first candidate (p == P, or no candidate from p on: the total); status_out = status
template <class Clouds>
__global__ __launch_bounds__(256) void offsets_kernel(Clouds L, int P, const int* __restrict__ pos, const long long* __restrict__ total,
                                                      const int* __restrict__ status, long long* __restrict__ out_off, int* __restrict__ status_out) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p > P) return;
    const long long f = L.first(p);
    out_off[p] = f < L.candidates() ? (long long)pos[f] : *total;
    if (p < P && status_out) status_out[p] = status[p];
}

}  // namespace cmg
}  // namespace ls

using namespace ls;
using namespace ls::cmg;

namespace {
struct Ws {
    long long* offs;      // a batch: the device copy of the offsets
    float* inv;           // a batch: [P]
    int* status;          // [P]
    long long* total;     // kept candidates in all
    int* cell;            // [n,3]
    int* table;           // [2 n]
    unsigned* slot_of;    // [n]
    int* keep;            // [n]
    int* pos;             // [n]
    int* blk;             // the scan's block sums
    size_t bytes;         // of the whole layout
};

// the layout depends on (P, n) alone (ws null: a sizing pass; n_offs = 0: a single problem)
Ws layout(void* ws, size_t n_offs, int P, long long n) {
    Arena a(ws);
    Ws w;
    w.offs = a.take<long long>(n_offs);
    w.inv = a.take<float>(n_offs ? (size_t)P : 0);
    w.status = a.take<int>((size_t)P);
    w.total = a.take<long long>(1);
    w.cell = a.take<int>((size_t)n * 3);
    w.table = a.take<int>((size_t)n * 2);
    w.slot_of = a.take<unsigned>((size_t)n);
    w.keep = a.take<int>((size_t)n);
    w.pos = a.take<int>((size_t)n);
    w.blk = a.take<int>((size_t)scan_blocks(n));
    w.bytes = a.bytes();
    return w;
}

// the launch sequence: P problems located by L, n candidates in all
template <class Clouds>
int merge_launch(const Clouds& L, int P, long long n, const Ws& w, float* out_pts, int* out_src, long long* out_off, int* status_out, hipStream_t st) {
    if (n == 0) {   // nothing to look at: every offset is 0
        LS_HIP_CHECK(hipMemsetAsync(out_off, 0, ((size_t)P + 1) * sizeof(long long), st));
        if (status_out) LS_HIP_CHECK(hipMemsetAsync(status_out, 0, (size_t)P * sizeof(int), st));
        return LS_OK;
    }
    const int nb = cdiv(n, 256);
    LS_HIP_CHECK(hipMemsetAsync(w.status, 0, (size_t)P * sizeof(int), st));             // LS_OK
    LS_HIP_CHECK(hipMemsetAsync(w.table, 0xFF, (size_t)n * 2 * sizeof(int), st));       // -1: free
    hipLaunchKernelGGL(cell_kernel<Clouds>, dim3(nb), dim3(256), 0, st, L, w.cell);
    hipLaunchKernelGGL(hash_kernel<Clouds>, dim3(nb), dim3(256), 0, st, L, w.cell, w.table, w.slot_of, w.status);
    hipLaunchKernelGGL(keep_kernel<Clouds>, dim3(nb), dim3(256), 0, st, L, w.table, w.slot_of, w.keep);
    scan<int, int, false>(w.keep, n, w.blk, w.pos, w.total, st);
    hipLaunchKernelGGL(scatter_kernel<Clouds>, dim3(nb), dim3(256), 0, st, L, w.keep, w.pos, out_pts, out_src);
    hipLaunchKernelGGL(offsets_kernel<Clouds>, dim3(cdiv((long long)P + 1, 256)), dim3(256), 0, st, L, P, w.pos, w.total, w.status, out_off, status_out);
    LS_LAUNCH_CHECK();
    return LS_OK;
}

int check_common(const char* op, long long a, long long b, const float* A, const float* B, const float* out_pts, const int* out_src,
                 const long long* out_off) {
    LS_REQUIRE(a >= 0 && b >= 0, "%s: negative size (%lld kept rows, %lld new rows)", op, a, b);
    LS_REQUIRE(a + b <= INT_MAX, "%s: %lld + %lld candidates exceed %d (int candidate indices)", op, a, b, INT_MAX);
    LS_REQUIRE((a == 0 || A) && (b == 0 || B), "%s: null A / B with %lld and %lld rows", op, a, b);
    LS_REQUIRE(out_off && (a + b == 0 || (out_pts && out_src)), "%s: null out_pts / out_src / out_off", op);
    return LS_OK;
}
}  // namespace

extern "C" {

size_t ls_cloud_merge_workspace_bytes(long long a, long long b) {
    if (a < 0 || b < 0 || a + b > INT_MAX) return 0;
    return layout(nullptr, 0, 1, a + b).bytes;
}

int ls_cloud_merge_f32(const float* A, long long a, const float* B, long long b, const float* g, float voxel, float* out_pts, int32_t* out_src,
                       long long* out_off, int* status_out, void* workspace, size_t workspace_bytes, void* stream) {
    const char* op = "cloud_merge";
    int rc = check_common(op, a, b, A, B, out_pts, out_src, out_off);
    if (rc != LS_OK) return rc;
    float inv;
    rc = check_edge(op, 0, "voxel edge", "voxel", voxel, &inv);
    if (rc != LS_OK) return rc;
    rc = check_workspace(op, workspace, workspace_bytes, ls_cloud_merge_workspace_bytes(a, b), 0, a, b);
    if (rc != LS_OK) return rc;
    const Ws w = layout(workspace, 0, 1, a + b);
    return merge_launch(OneCloud{A, a, B, b, g, inv}, 1, a + b, w, out_pts, out_src, out_off, status_out, (hipStream_t)stream);
}

size_t ls_cloud_merge_batch_workspace_bytes(int P, long long a_total, long long b_total) {
    if (P < 1 || a_total < 0 || b_total < 0 || a_total + b_total > INT_MAX) return 0;
    return layout(nullptr, (size_t)OFF_ARRAYS * (P + 1), P, a_total + b_total).bytes;
}

int ls_cloud_merge_batch_f32(int P, const float* A, long long a_total, const long long* a_off, const float* B, long long b_total,
                             const long long* b_off, const float* g, const float* voxel, float* out_pts, int32_t* out_src, long long* out_off,
                             int* status_out, void* workspace, size_t workspace_bytes, void* stream) {
    const char* op = "cloud_merge_batch";
    LS_REQUIRE(P >= 1, "%s: P must be at least 1, got %d", op, P);
    int rc = check_common(op, a_total, b_total, A, B, out_pts, out_src, out_off);
    if (rc != LS_OK) return rc;
    rc = check_ranges(op, "problem", "a_off", P, a_off, a_total, INT_MAX);
    if (rc != LS_OK) return rc;
    rc = check_ranges(op, "problem", "b_off", P, b_off, b_total, INT_MAX);
    if (rc != LS_OK) return rc;
    LS_REQUIRE(voxel, "%s: null voxel", op);
    std::vector<long long> c_off(P + 1, 0);
    std::vector<float> inv(P);
    for (int p = 0; p < P; ++p) {
        c_off[p + 1] = a_off[p + 1] + b_off[p + 1];
        rc = check_edge(op, p, "voxel edge", "voxel", voxel[p], &inv[p]);
        if (rc != LS_OK) return rc;
    }
    rc = check_workspace(op, workspace, workspace_bytes, ls_cloud_merge_batch_workspace_bytes(P, a_total, b_total), P, a_total, b_total);
    if (rc != LS_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const Ws w = layout(workspace, (size_t)OFF_ARRAYS * (P + 1), P, a_total + b_total);
    rc = upload_offsets(w.offs, pack_offsets(P, {a_off, b_off, c_off.data()}), st);
    if (rc != LS_OK) return rc;
    LS_HIP_CHECK(hipMemcpyAsync(w.inv, inv.data(), (size_t)P * sizeof(float), hipMemcpyHostToDevice, st));   // pageable: read when it returns
    return merge_launch(RaggedClouds{A, B, g, w.offs, w.inv, P, a_total + b_total}, P, a_total + b_total, w, out_pts, out_src, out_off, status_out, st);
}

}  // extern "C"
