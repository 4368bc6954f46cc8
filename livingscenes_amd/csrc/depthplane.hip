// depthplane.hip -- scene memory: a normal per pixel of posed depth views, and the depth fusion of depthfuse.hip with integer weights and
// a point-to-plane value inside the band.  The state is the fuse's (two int32 volumes, sum and n), so every reader of it runs on a
// weighted state as it is.  The definitions are in include/livingscenes_hip.h (ls_depth_normals_f32, ls_depth_fuse_weighted_f32) and,
// as NumPy, in tests/plane_oracle.py; the arithmetic of one pixel and of one (voxel, view) is plane_plan.h, whose steps 1 - 5 are the
// functions of fuse_plan.h and carve_plan.h themselves.  What this file adds:
//   normals        one thread per pixel; a workgroup owns DN_CHUNK consecutive pixels of ONE view (the view is blockIdx / chunks-per-view),
//                  so the intrinsics and max_jump are indexed from blockIdx alone and stay in scalar registers.  Up to four neighbour loads
//                  per pixel from the same image rows; the histogram is one integer add per wave, view and state from a ballot.
//   weighted fuse  the shape of fuse_kernel: a workgroup owns FUSE_CHUNK consecutive voxels of ONE problem, one thread per voxel keeps
//                  (sum, n) in registers over the problem's views; E, K, the weights and the image bases are scalar; one depth gather and,
//                  for a NEAR voxel-view with normals, three normal gathers, from images that stay in L2.
// Launches of the normals: the copy of max_jump into the workspace, 1 memset (counts) and 1 kernel; of a weighted fuse: the copy of the
// host arrays into the workspace, 1 memset (view_counts) and 1 kernel -- whatever P and the number of views.  No host synchronisation, no
// allocation, integer atomics only.
#include <climits>
#include <cmath>
#include <vector>

#include "ls_common.h"
#include "ls_ragged.h"
#include "ls_workspace.h"

// the arithmetic of the definitions as written: no contraction of a * b + c into an fma anywhere in this file
#pragma clang fp contract(off)
#include "plane_plan.h"

namespace ls {
namespace dpl {
using namespace fp;
using namespace pp;

// one integer add per wave: the lanes with `flag`.  Every lane of the wave calls it.
__device__ __forceinline__ void count_wave(bool flag, long long* __restrict__ where) {
    const unsigned long long m = __ballot(flag);
    if ((threadIdx.x & (kWave - 1)) == 0 && m) atomicAdd((unsigned long long*)where, (unsigned long long)__popcll(m));
}

// workgroup = one chunk of pixels of one view, one thread per pixel
__global__ __launch_bounds__(DN_CHUNK) void normals_kernel(const float* __restrict__ depth, const double* __restrict__ K, const double* __restrict__ jumps,
                                                           int H, int W, long long chunks, float* __restrict__ normals, unsigned char* __restrict__ state,
                                                           long long* __restrict__ counts) {
    const long long v = (long long)blockIdx.x / chunks;
    const long long pixels = (long long)H * W;
    const long long idx = ((long long)blockIdx.x - v * chunks) * DN_CHUNK + threadIdx.x;
    const bool live = idx < pixels;
    int st = -1;
    if (live) {
        const unsigned u = (unsigned)idx, w = (unsigned)W;                  // idx < 2^31
        float n[3];
        st = plane_normal(depth + (size_t)v * (size_t)pixels, W, H, (int)(u % w), (int)(u / w), K + v * 4, jumps[v], n);
        const size_t at = (size_t)v * (size_t)pixels + (size_t)idx;
        normals[at * 3 + 0] = n[0];
        normals[at * 3 + 1] = n[1];
        normals[at * 3 + 2] = n[2];
        state[at] = (unsigned char)st;
    }
    for (int s = 0; s < DN_STATES; ++s) count_wave(st == s, counts + v * DN_STATES + s);
}

struct WeightedArgs {
    int* sum;                      // [P,nx,ny,nz]
    int* n;                        // [P,nx,ny,nz]
    int ny, nz;
    long long voxels;              // nx ny nz
    long long chunks;              // per problem
    const long long* view_off;     // [P+1], in the workspace
    const double* grids;           // [P,5]: origin, voxel, trunc, in the workspace
    const float* depth;            // [views_total,H,W]
    const float* normals;          // [views_total,H,W,3] or null
    const double* K;               // [views_total,4]
    const double* E;               // [views_total,3,4]
    int H, W;
    double znear;
    int empty_is_free;
    int weights[FW_WEIGHTS];
    long long* view_counts;        // [views_total,7]
};

// workgroup = one chunk of voxels of one problem, one thread per voxel: the loop over the problem's views around plane_voxel_view
__global__ __launch_bounds__(FUSE_CHUNK) void fuse_weighted_kernel(WeightedArgs G) {
    const long long p = (long long)blockIdx.x / G.chunks;
    const long long v0 = G.view_off[p], v1 = G.view_off[p + 1];
    if (v0 == v1) return;                                                 // the whole workgroup: nothing to fuse, nothing is touched
    const long long idx = ((long long)blockIdx.x - p * G.chunks) * FUSE_CHUNK + threadIdx.x;
    const bool live = idx < G.voxels;
    const double* g = G.grids + p * FUSE_GRID_WORDS;
    const double h = g[3], trunc = g[4];
    const long long at = p * G.voxels + idx;
    double x[3] = {0.0, 0.0, 0.0};
    int sum = 0, n = 0;
    if (live) {
        const unsigned u = (unsigned)idx, nz = (unsigned)G.nz, ny = (unsigned)G.ny;   // idx < 2^31
        const int k = (int)(u % nz), j = (int)((u / nz) % ny), i = (int)((u / nz) / ny);
        x[0] = fuse_position(g[0], h, i);
        x[1] = fuse_position(g[1], h, j);
        x[2] = fuse_position(g[2], h, k);
        sum = G.sum[at];
        n = G.n[at];
    }
    const size_t image = (size_t)G.H * (size_t)G.W;
    for (long long v = v0; v < v1; ++v) {                                 // the same views for every thread of the workgroup
        int cls = -1;
        if (live) {
            int q, w;
            cls = plane_voxel_view(G.E + v * 12, G.K + v * 4, x, G.depth + (size_t)v * image, G.normals ? G.normals + (size_t)v * image * 3 : nullptr,
                                   G.W, G.H, trunc, G.znear, G.empty_is_free != 0, G.weights, &q, &w);
            cls = plane_update(cls, q, w, &sum, &n);
        }
        for (int s = 0; s < FW_CLASSES; ++s) count_wave(cls == s, G.view_counts + v * FW_CLASSES + s);
    }
    if (live) {
        G.sum[at] = sum;
        G.n[at] = n;
    }
}

}  // namespace dpl
}  // namespace ls

using namespace ls;
using namespace ls::dpl;

namespace {
struct Ws {
    long long* words;     // view_off [P+1], then the grids [P,5] as float64
    size_t offs;          // the number of offset words
    size_t bytes;         // of the whole layout
};

// the one layout of the weighted fuse: the piece of fuse_plan.h from one Arena (ws null: a sizing pass)
Ws layout(void* ws, int P) {
    const FusePieces c = fuse_pieces(P);
    Arena ar(ws);
    Ws w;
    w.words = ar.take<long long>(c.offs + c.grids);
    w.offs = c.offs;
    w.bytes = ar.bytes();
    return w;
}

// the one layout of the normals: max_jump [views]
size_t jumps_layout(void* ws, long long views, double** jumps) {
    Arena ar(ws);
    double* j = ar.take<double>(plane_pieces(views));
    if (jumps) *jumps = j;
    return ar.bytes();
}

bool sizes_ok(int P, int nx, int ny, int nz, long long views) { return fuse_sizes_ok(P, nx, ny, nz) && views >= 0 && views <= INT_MAX; }

// everything the host decides, then the copy, the memset and the kernel
int weighted_run(const char* op, int P, int32_t* sum, int32_t* n, int nx, int ny, int nz, const double* origin, const double* voxel,
                 const double* trunc, const float* depth, const float* normals, long long views, const long long* view_off, int H, int W,
                 const double* K, const double* E, double znear, int empty_is_free, const int* weights, long long* view_counts, void* workspace,
                 size_t workspace_bytes, size_t need, hipStream_t st) {
    LS_REQUIRE(P >= 1, "%s: P must be at least 1, got %d", op, P);
    LS_REQUIRE(nx >= 1 && ny >= 1 && nz >= 1, "%s: dims must be at least 1, got %d x %d x %d", op, nx, ny, nz);
    LS_REQUIRE(fuse_sizes_ok(P, nx, ny, nz), "%s: P * nx * ny * nz = %d * %d * %d * %d reaches 2^31 (int32 state indices)", op, P, nx, ny, nz);
    LS_REQUIRE(views >= 0, "%s: negative size (%lld views)", op, views);
    LS_REQUIRE(views <= INT_MAX, "%s: %lld views exceed %d (int view counts)", op, views, INT_MAX);
    LS_REQUIRE(H >= 1 && W >= 1, "%s: the image must have at least one pixel, got %d x %d", op, H, W);
    LS_REQUIRE(sum && n, "%s: null sum / n", op);
    LS_REQUIRE(origin && voxel && trunc, "%s: null origin / voxel / trunc", op);
    LS_REQUIRE(weights, "%s: null weights", op);
    LS_REQUIRE(views == 0 || (depth && K && E && view_counts), "%s: null depth / intrinsics / world_to_cam / view_counts with %lld views", op, views);
    int rc = check_ranges(op, "problem", "view_off", P, view_off, views, INT_MAX);
    if (rc != LS_OK) return rc;
    for (int p = 0; p < P; ++p) {
        const int bad = fuse_bad_grid(origin + (size_t)p * 3, voxel[p], trunc[p]);
        LS_REQUIRE(bad != 1, "%s: problem %d: origin must be finite, got (%g, %g, %g)", op, p, origin[p * 3], origin[p * 3 + 1], origin[p * 3 + 2]);
        LS_REQUIRE(bad != 2, "%s: problem %d: voxel must be finite and > 0, got %g", op, p, voxel[p]);
        LS_REQUIRE(bad != 3, "%s: problem %d: trunc must be finite and > 0, got %g", op, p, trunc[p]);
    }
    const int bad = fuse_bad_scalar(znear, empty_is_free);
    LS_REQUIRE(bad != 1, "%s: znear must be finite and > 0, got %g", op, znear);
    LS_REQUIRE(bad != 2, "%s: empty_is_free must be 0 or 1, got %d", op, empty_is_free);
    const int bw = plane_bad_weight(weights);
    LS_REQUIRE(bw < 0, "%s: weights[%d] must be in 1 .. %d (w_plane, w_proj, w_free, w_empty), got %d", op, bw, FW_MAX_WEIGHT, weights[bw < 0 ? 0 : bw]);
    if (!(workspace && workspace_bytes >= need)) {
        set_error("%s: workspace %zu < required %zu (ls_%s_workspace_bytes)", op, workspace ? workspace_bytes : (size_t)0, need, op);
        return LS_ERR_WORKSPACE;
    }
    if (views == 0) return LS_OK;                                          // no problem has a view: nothing changes
    const Ws w = layout(workspace, P);
    std::vector<long long> host(w.offs + (size_t)P * FUSE_GRID_WORDS);
    std::copy(view_off, view_off + P + 1, host.begin());
    double* grids = (double*)(host.data() + w.offs);                       // 8-byte words both
    for (int p = 0; p < P; ++p) {
        for (int a = 0; a < 3; ++a) grids[p * FUSE_GRID_WORDS + a] = origin[p * 3 + a];
        grids[p * FUSE_GRID_WORDS + 3] = voxel[p];
        grids[p * FUSE_GRID_WORDS + 4] = trunc[p];
    }
    rc = upload_offsets(w.words, host, st);
    if (rc != LS_OK) return rc;
    const long long voxels = (long long)nx * ny * nz, chunks = fuse_chunks(voxels);
    WeightedArgs G{sum, n, ny, nz, voxels, chunks, w.words, (const double*)(w.words + w.offs), depth, normals, K, E, H, W, znear, empty_is_free, {0, 0, 0, 0},
                   view_counts};
    for (int k = 0; k < FW_WEIGHTS; ++k) G.weights[k] = weights[k];
    LS_HIP_CHECK(hipMemsetAsync(view_counts, 0, (size_t)views * FW_CLASSES * sizeof(long long), st));
    hipLaunchKernelGGL(fuse_weighted_kernel, dim3((unsigned)(chunks * P)), dim3(FUSE_CHUNK), 0, st, G);
    LS_LAUNCH_CHECK();
    return LS_OK;
}
}  // namespace

extern "C" {

size_t ls_depth_normals_workspace_bytes(long long views, int height, int width) {
    if (!plane_sizes_ok(views, height, width)) return 0;
    return jumps_layout(nullptr, views, nullptr);
}

int ls_depth_normals_f32(const float* depth, long long views, int height, int width, const double* intrinsics, const double* max_jump,
                         float* normals_out, uint8_t* state_out, long long* counts_out, void* workspace, size_t workspace_bytes, void* stream) {
    const char* op = "depth_normals";
    LS_REQUIRE(views >= 0, "%s: negative size (%lld views)", op, views);
    LS_REQUIRE(height >= 1 && width >= 1, "%s: the image must have at least one pixel, got %d x %d", op, height, width);
    LS_REQUIRE(plane_sizes_ok(views, height, width), "%s: views * height * width = %lld * %d * %d reaches 2^31 (int32 pixel indices)", op, views, height,
               width);
    LS_REQUIRE(views == 0 || (depth && intrinsics && max_jump && normals_out && state_out && counts_out),
               "%s: null depth / intrinsics / max_jump / normals_out / state_out / counts_out with %lld views", op, views);
    for (long long v = 0; v < views; ++v)
        LS_REQUIRE(!plane_bad_jump(max_jump[v]), "%s: view %lld: max_jump must be finite and > 0, got %g", op, v, max_jump[v]);
    const size_t need = ls_depth_normals_workspace_bytes(views, height, width);
    if (!(workspace && workspace_bytes >= need)) {
        set_error("%s: workspace %zu < required %zu (ls_%s_workspace_bytes)", op, workspace ? workspace_bytes : (size_t)0, need, op);
        return LS_ERR_WORKSPACE;
    }
    if (views == 0) return LS_OK;
    hipStream_t st = (hipStream_t)stream;
    double* jumps = nullptr;
    jumps_layout(workspace, views, &jumps);
    LS_HIP_CHECK(hipMemcpyAsync(jumps, max_jump, (size_t)views * sizeof(double), hipMemcpyHostToDevice, st));
    const long long chunks = plane_chunks((long long)height * width);
    LS_HIP_CHECK(hipMemsetAsync(counts_out, 0, (size_t)views * DN_STATES * sizeof(long long), st));
    hipLaunchKernelGGL(normals_kernel, dim3((unsigned)(chunks * views)), dim3(DN_CHUNK), 0, st, depth, intrinsics, jumps, height, width, chunks, normals_out,
                       state_out, counts_out);
    LS_LAUNCH_CHECK();
    return LS_OK;
}

size_t ls_depth_fuse_weighted_workspace_bytes(int nx, int ny, int nz, long long views) {
    if (!sizes_ok(1, nx, ny, nz, views)) return 0;
    return layout(nullptr, 1).bytes;
}

int ls_depth_fuse_weighted_f32(int32_t* sum, int32_t* n, int nx, int ny, int nz, const double* origin, double voxel, double trunc, const float* depth,
                               const float* normals, long long views, int height, int width, const double* intrinsics, const double* world_to_cam,
                               double znear, int empty_is_free, const int* weights, long long* view_counts, void* workspace, size_t workspace_bytes,
                               void* stream) {
    const long long view_off[2] = {0, views};
    return weighted_run("depth_fuse_weighted", 1, sum, n, nx, ny, nz, origin, &voxel, &trunc, depth, normals, views, view_off, height, width, intrinsics,
                        world_to_cam, znear, empty_is_free, weights, view_counts, workspace, workspace_bytes,
                        ls_depth_fuse_weighted_workspace_bytes(nx, ny, nz, views), (hipStream_t)stream);
}

size_t ls_depth_fuse_weighted_batch_workspace_bytes(int P, int nx, int ny, int nz, long long views_total) {
    if (!sizes_ok(P, nx, ny, nz, views_total)) return 0;
    return layout(nullptr, P).bytes;
}

int ls_depth_fuse_weighted_batch_f32(int P, int32_t* sum, int32_t* n, int nx, int ny, int nz, const double* origin, const double* voxel,
                                     const double* trunc, const float* depth, const float* normals, long long views_total, const long long* view_off,
                                     int height, int width, const double* intrinsics, const double* world_to_cam, double znear, int empty_is_free,
                                     const int* weights, long long* view_counts, void* workspace, size_t workspace_bytes, void* stream) {
    return weighted_run("depth_fuse_weighted_batch", P, sum, n, nx, ny, nz, origin, voxel, trunc, depth, normals, views_total, view_off, height, width,
                        intrinsics, world_to_cam, znear, empty_is_free, weights, view_counts, workspace, workspace_bytes,
                        ls_depth_fuse_weighted_batch_workspace_bytes(P, nx, ny, nz, views_total), (hipStream_t)stream);
}

}  // extern "C"
