// cloudcarve.hip -- scene memory: the kept cloud of an instance (A) carved by posed depth views of it.  A kept row that a view looks
// THROUGH lies in observed free space and may be dropped; a row a view confirms, a row it cannot see and a row it cannot judge stay.  The
// definition is in include/livingscenes_hip.h (ls_cloud_carve_f32) and, as NumPy, in tests/carve_oracle.py; the arithmetic of one
// (row, view), the keep rule and the pieces of the workspace are those of carve_plan.h.  What this file adds:
//   carve      a workgroup owns one chunk of CARVE_CHUNK rows of ONE problem, found from the chunk offsets as in cloudnear.hip, so the
//              problem's views are the same for the whole workgroup: E, the intrinsics and the image base are indexed from blockIdx alone
//              and stay in scalar registers.  One thread per row loops over the views and gathers at most (2k+1)^2 pixels per view (the
//              images are small and stay in L2): state, seen, free, the keep flag.  The histograms come from a ballot: one integer add
//              per wave, view and state, and one per wave and per-problem counter.
//   compact    flag -> scan (ls_scan.h) -> scatter, as in cloudmerge.hip: the kept rows of every problem back to back, the same bits
// Launches, whatever P and the number of views: a call with rows makes 2 memsets (counts, view_counts; the latter only with views) and 6
// kernels (carve, the scan's three, scatter, offsets); a call without rows makes 4 memsets at most and no kernel.  No host
// synchronisation, no allocation, integer atomics only and no floating-point sum anywhere: a problem's outputs are the same bits alone,
// in any batch and in any run.  Every kernel is written once, for a problem locator (OneCarve / RaggedCarve).
#include <climits>
#include <cmath>
#include <vector>

#include "ls_common.h"
#include "ls_ragged.h"
#include "ls_scan.h"

// the arithmetic of the definition as written: no contraction of a * b + c into an fma anywhere in this file
#pragma clang fp contract(off)
#include "carve_plan.h"
#include "cloud_grid.h"   // check_workspace: the refusal that names the size query

namespace ls {
namespace ccv {
using namespace cp;

// ------------------------------------------------------------------------------------------------ which problem: one, or one of a ragged batch
struct CarveRef {
    const float* A;        // the problem's rows
    long long a;           // their number
    long long a0;          // global index of its first row
    long long v0, v1;      // its views
    long long q0;          // its first chunk
    long long s0;          // the first byte of its block of `state`
};

struct OneCarve {
    const float* A;
    long long a, views;
    __device__ long long rows() const { return a; }
    __device__ int chunk_owner(long long) const { return 0; }
    __device__ long long first(int p) const { return p == 0 ? 0 : a; }   // p in [0, P]
    __device__ CarveRef problem(int) const { return {A, a, 0, 0, views, 0, 0}; }
};

enum { OFF_A = 0, OFF_V, OFF_Q, OFF_S, OFF_ARRAYS };   // the device copy of a batch's offsets: rows, views, chunks, bytes of state

struct RaggedCarve {
    const float* A;
    const long long* offs;
    int P;
    long long a_total;
    __device__ const long long* off(int k) const { return offs + (size_t)k * (P + 1); }
    __device__ long long rows() const { return a_total; }
    __device__ int chunk_owner(long long c) const { return owner(off(OFF_Q), P, c); }
    __device__ long long first(int p) const { return off(OFF_A)[p]; }
    __device__ CarveRef problem(int p) const {
        const long long *ao = off(OFF_A), *vo = off(OFF_V);
        return {A + ao[p] * 3, ao[p + 1] - ao[p], ao[p], vo[p], vo[p + 1], off(OFF_Q)[p], off(OFF_S)[p]};
    }
};

struct CarveArgs {
    const float* depth;            // [views_total,H,W]
    const double* K;               // [views_total,4]
    const double* E;               // [views_total,3,4]
    int H, W;
    double tol, znear;
    int window, min_free, max_seen, empty_is_free;
    int* seen;                     // [a_total]
    int* free_views;               // [a_total]
    long long* counts;             // [P,4]
    long long* view_counts;        // [views_total,5]
    unsigned char* state;          // nullable
};

// one integer add per wave: the lanes with `flag`.  Every lane of the wave calls it.
__device__ __forceinline__ void count_wave(bool flag, long long* __restrict__ where) {
    const unsigned long long m = __ballot(flag);
    if ((threadIdx.x & (kWave - 1)) == 0 && m) atomicAdd((unsigned long long*)where, (unsigned long long)__popcll(m));
}

// workgroup = one chunk of rows of one problem, one thread per row: the loop over the problem's views around carve_point_view
template <class Carve>
__global__ __launch_bounds__(CARVE_CHUNK) void carve_kernel(Carve L, CarveArgs G, int* __restrict__ keep) {
    const int p = L.chunk_owner(blockIdx.x);
    const CarveRef C = L.problem(p);
    const long long qi = ((long long)blockIdx.x - C.q0) * CARVE_CHUNK + threadIdx.x;
    const bool live = qi < C.a;
    float x[3] = {0.f, 0.f, 0.f};
    if (live)
        for (int k = 0; k < 3; ++k) x[k] = C.A[qi * 3 + k];
    const size_t image = (size_t)G.H * (size_t)G.W;
    int seen = 0, free_views = 0, out = 0;
    for (long long v = C.v0; v < C.v1; ++v) {                             // the same views for every thread of the workgroup
        int st = CARVE_OUT;
        if (live)
            st = carve_point_view(G.E + v * 12, G.K + v * 4, x, G.depth + (size_t)v * image, G.W, G.H, G.tol, G.znear, G.window,
                                  G.empty_is_free != 0);
        seen += st == CARVE_SEEN;
        free_views += st == CARVE_FREE;
        out += st == CARVE_OUT;
        if (live && G.state) G.state[(size_t)C.s0 + (size_t)(v - C.v0) * (size_t)C.a + (size_t)qi] = (unsigned char)st;
        for (int s = 0; s < CARVE_STATES; ++s) count_wave(live && st == s, G.view_counts + v * CARVE_STATES + s);
    }
    const bool drop = live && carve_drop(seen, free_views, G.min_free, G.max_seen);
    if (live) {
        G.seen[C.a0 + qi] = seen;
        G.free_views[C.a0 + qi] = free_views;
        keep[C.a0 + qi] = drop ? 0 : 1;
    }
    long long* cnt = G.counts + (size_t)p * CNT_FIELDS;
    count_wave(live && seen >= 1, cnt + CNT_SEEN);
    count_wave(live && free_views >= 1, cnt + CNT_FREE);
    count_wave(drop, cnt + CNT_DROPPED);
    count_wave(live && out == (int)(C.v1 - C.v0), cnt + CNT_OUT);
}

// the kept rows at their rank pos[i] (the exclusive scan of keep): the row bit for bit and its index in its problem
template <class Carve>
__global__ __launch_bounds__(CARVE_CHUNK) void scatter_kernel(Carve L, const int* __restrict__ keep, const int* __restrict__ pos,
                                                              float* __restrict__ out_pts, int* __restrict__ out_src) {
    const CarveRef C = L.problem(L.chunk_owner(blockIdx.x));
    const long long qi = ((long long)blockIdx.x - C.q0) * CARVE_CHUNK + threadIdx.x;
    if (qi >= C.a || !keep[C.a0 + qi]) return;
    const long long o = pos[C.a0 + qi];
    for (int k = 0; k < 3; ++k) out_pts[o * 3 + k] = C.A[qi * 3 + k];
    out_src[o] = (int)qi;
}

// out_off[p] = the rank of problem p's first row (p == P, or no row from p on: the total); status_out = LS_OK
template <class Carve>
__global__ __launch_bounds__(256) void offsets_kernel(Carve L, int P, const int* __restrict__ pos, const long long* __restrict__ total,
                                                      long long* __restrict__ out_off, int* __restrict__ status_out) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p > P) return;
    const long long f = L.first(p);
    out_off[p] = f < L.rows() ? (long long)pos[f] : *total;
    if (p < P && status_out) status_out[p] = LS_OK;
}

}  // namespace ccv
}  // namespace ls

using namespace ls;
using namespace ls::ccv;

namespace {
struct Ws {
    long long* offs;      // a batch: the device copy of the offsets
    int* keep;            // [a]
    int* pos;             // [a]
    int* blk;             // the scan's block sums
    long long* total;     // kept rows in all
    size_t bytes;         // of the whole layout
};

// the one layout: the pieces of carve_plan.h from one Arena (ws null: a sizing pass; n_off_arrays = 0: a single problem)
Ws layout(void* ws, int n_off_arrays, int P, long long a) {
    const CarvePieces c = carve_pieces(P, a, n_off_arrays, SCAN_PER_BLOCK);
    Arena ar(ws);
    Ws w;
    w.offs = ar.take<long long>(c.offs);
    w.keep = ar.take<int>(c.keep);
    w.pos = ar.take<int>(c.pos);
    w.blk = ar.take<int>(c.blk);
    w.total = ar.take<long long>(c.total);
    w.bytes = ar.bytes();
    return w;
}

struct Outs {
    float* out_pts;
    int* out_src;
    long long* out_off;
    int* status_out;
};

// the launch sequence: P problems located by L, a rows, `views` views and `chunks` chunks of rows in all
template <class Carve>
int carve_launch(const Carve& L, int P, long long a, long long views, long long chunks, const CarveArgs& G, const Ws& w, const Outs& O, hipStream_t st) {
    LS_HIP_CHECK(hipMemsetAsync(G.counts, 0, (size_t)P * CNT_FIELDS * sizeof(long long), st));
    if (views > 0) LS_HIP_CHECK(hipMemsetAsync(G.view_counts, 0, (size_t)views * CARVE_STATES * sizeof(long long), st));
    if (a == 0) {   // nothing to look at: every offset is 0
        LS_HIP_CHECK(hipMemsetAsync(O.out_off, 0, ((size_t)P + 1) * sizeof(long long), st));
        if (O.status_out) LS_HIP_CHECK(hipMemsetAsync(O.status_out, 0, (size_t)P * sizeof(int), st));
        return LS_OK;
    }
    hipLaunchKernelGGL(carve_kernel<Carve>, dim3((unsigned)chunks), dim3(CARVE_CHUNK), 0, st, L, G, w.keep);
    scan<int, int, false>(w.keep, a, w.blk, w.pos, w.total, st);
    hipLaunchKernelGGL(scatter_kernel<Carve>, dim3((unsigned)chunks), dim3(CARVE_CHUNK), 0, st, L, w.keep, w.pos, O.out_pts, O.out_src);
    hipLaunchKernelGGL(offsets_kernel<Carve>, dim3(cdiv((long long)P + 1, 256)), dim3(256), 0, st, L, P, w.pos, w.total, O.out_off, O.status_out);
    LS_LAUNCH_CHECK();
    return LS_OK;
}

bool sizes_ok(long long a, long long views) { return a >= 0 && a <= SCAN_MAX_N && views >= 0 && views <= INT_MAX; }

int check_common(const char* op, const float* A, long long a, long long views, int H, int W, const CarveArgs& G, const Outs& O) {
    LS_REQUIRE(a >= 0 && views >= 0, "%s: negative size (%lld kept rows, %lld views)", op, a, views);
    LS_REQUIRE(a <= SCAN_MAX_N, "%s: %lld kept rows exceed %lld (the scan's reach)", op, a, SCAN_MAX_N);
    LS_REQUIRE(views <= INT_MAX, "%s: %lld views exceed %d (int view counts)", op, views, INT_MAX);
    LS_REQUIRE(H >= 1 && W >= 1, "%s: the image must have at least one pixel, got %d x %d", op, H, W);
    LS_REQUIRE(a == 0 || (A && O.out_pts && O.out_src && G.seen && G.free_views), "%s: null A / out_pts / out_src / seen / free with %lld rows", op, a);
    LS_REQUIRE(O.out_off && G.counts, "%s: null out_off / counts", op);
    LS_REQUIRE(views == 0 || (G.depth && G.K && G.E && G.view_counts), "%s: null depth / intrinsics / world_to_cam / view_counts with %lld views", op,
               views);
    return LS_OK;
}

int check_scalars(const char* op, const CarveArgs& G) {
    const int bad = carve_bad_scalar(G.tol, G.znear, G.window, G.min_free, G.max_seen, G.empty_is_free);
    LS_REQUIRE(bad != 1, "%s: tol must be finite and >= 0, got %g", op, G.tol);
    LS_REQUIRE(bad != 2, "%s: znear must be finite and > 0, got %g", op, G.znear);
    LS_REQUIRE(bad != 3, "%s: window must be 0, 1 or %d (pixels to every side), got %d", op, CARVE_MAX_WINDOW, G.window);
    LS_REQUIRE(bad != 4, "%s: min_free must be >= 1 (0 would drop rows no view looks through), got %d", op, G.min_free);
    LS_REQUIRE(bad != 5, "%s: max_seen must be >= 0, got %d", op, G.max_seen);
    LS_REQUIRE(bad != 6, "%s: empty_is_free must be 0 or 1, got %d", op, G.empty_is_free);
    return LS_OK;
}
}  // namespace

extern "C" {

size_t ls_cloud_carve_workspace_bytes(long long a, long long views) {
    if (!sizes_ok(a, views)) return 0;
    return layout(nullptr, 0, 1, a).bytes;
}

int ls_cloud_carve_f32(const float* A, long long a, const float* depth, long long views, int height, int width, const double* intrinsics,
                       const double* world_to_cam, double tol, double znear, int window, int min_free, int max_seen, int empty_is_free,
                       float* out_pts, int32_t* out_src, long long* out_off, int32_t* seen, int32_t* free_views, long long* counts,
                       long long* view_counts, uint8_t* state, int* status_out, void* workspace, size_t workspace_bytes, void* stream) {
    const char* op = "cloud_carve";
    const CarveArgs G{depth, intrinsics, world_to_cam, height, width, tol, znear, window, min_free, max_seen, empty_is_free,
                      seen, free_views, counts, view_counts, state};
    const Outs O{out_pts, out_src, out_off, status_out};
    int rc = check_common(op, A, a, views, height, width, G, O);
    if (rc != LS_OK) return rc;
    rc = check_scalars(op, G);
    if (rc != LS_OK) return rc;
    rc = cloud::check_workspace(op, workspace, workspace_bytes, ls_cloud_carve_workspace_bytes(a, views), 0, a, views);
    if (rc != LS_OK) return rc;
    const Ws w = layout(workspace, 0, 1, a);
    return carve_launch(OneCarve{A, a, views}, 1, a, views, carve_chunks(a), G, w, O, (hipStream_t)stream);
}

size_t ls_cloud_carve_batch_workspace_bytes(int P, long long a_total, long long views_total) {
    if (P < 1 || !sizes_ok(a_total, views_total)) return 0;
    return layout(nullptr, OFF_ARRAYS, P, a_total).bytes;
}

int ls_cloud_carve_batch_f32(int P, const float* A, long long a_total, const long long* a_off, const float* depth, long long views_total,
                             const long long* view_off, int height, int width, const double* intrinsics, const double* world_to_cam, double tol,
                             double znear, int window, int min_free, int max_seen, int empty_is_free, float* out_pts, int32_t* out_src,
                             long long* out_off, int32_t* seen, int32_t* free_views, long long* counts, long long* view_counts, uint8_t* state,
                             int* status_out, void* workspace, size_t workspace_bytes, void* stream) {
    const char* op = "cloud_carve_batch";
    LS_REQUIRE(P >= 1, "%s: P must be at least 1, got %d", op, P);
    const CarveArgs G{depth, intrinsics, world_to_cam, height, width, tol, znear, window, min_free, max_seen, empty_is_free,
                      seen, free_views, counts, view_counts, state};
    const Outs O{out_pts, out_src, out_off, status_out};
    int rc = check_common(op, A, a_total, views_total, height, width, G, O);
    if (rc != LS_OK) return rc;
    rc = check_ranges(op, "problem", "a_off", P, a_off, a_total, SCAN_MAX_N);
    if (rc != LS_OK) return rc;
    rc = check_ranges(op, "problem", "view_off", P, view_off, views_total, INT_MAX);
    if (rc != LS_OK) return rc;
    rc = check_scalars(op, G);
    if (rc != LS_OK) return rc;
    rc = cloud::check_workspace(op, workspace, workspace_bytes, ls_cloud_carve_batch_workspace_bytes(P, a_total, views_total), P, a_total, views_total);
    if (rc != LS_OK) return rc;
    std::vector<long long> q_off(P + 1, 0), s_off(P + 1, 0);
    for (int p = 0; p < P; ++p) {
        const long long a = a_off[p + 1] - a_off[p];
        q_off[p + 1] = q_off[p] + carve_chunks(a);
        s_off[p + 1] = s_off[p] + a * (view_off[p + 1] - view_off[p]);
    }
    hipStream_t st = (hipStream_t)stream;
    const Ws w = layout(workspace, OFF_ARRAYS, P, a_total);
    rc = upload_offsets(w.offs, pack_offsets(P, {a_off, view_off, q_off.data(), s_off.data()}), st);
    if (rc != LS_OK) return rc;
    return carve_launch(RaggedCarve{A, w.offs, P, a_total}, P, a_total, views_total, q_off[P], G, w, O, st);
}

}  // extern "C"
