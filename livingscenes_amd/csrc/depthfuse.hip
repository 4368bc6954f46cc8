// depthfuse.hip -- scene memory: posed depth views of an instance fused into a truncated signed distance volume, and the volume read out
// of that state.  The state of a problem is two int32 volumes [nx,ny,nz] (k fastest, as mcubes.hip reads a volume): `sum`, the quantised
// truncated distances, and `n`, the observation count; both are updated in place and a fresh state is all zeros.  The definition is in
// include/livingscenes_hip.h (ls_depth_fuse_f32) and, as NumPy, in tests/fuse_oracle.py; the arithmetic of one (voxel, view), the update
// and the value of a sample are those of fuse_plan.h, the projection is the carve's (carve_plan.h).  What this file adds:
//   fuse       a workgroup owns one chunk of FUSE_CHUNK consecutive voxels of ONE problem (every problem of a call has the same dims, so
//              the problem is blockIdx / chunks-per-problem): its grid and its views are the same for the whole workgroup, E, the
//              intrinsics and the image base are indexed from blockIdx alone and stay in scalar registers.  One thread per voxel reads
//              (sum, n) once, loops over the problem's views in the call's order with the pair in registers, gathers one pixel per view
//              (the images are small and stay in L2) and writes the pair once.  The histogram comes from a ballot: one integer add per
//              wave, view and class.  A problem without views is left before anything is read.
//   volume     one thread per voxel: D, the valid flag, three ballots for the counts.
// Launches of a fuse, whatever P and the number of views: the copy of the host arrays into the workspace, 1 memset (view_counts) and 1
// kernel; of a volume: 1 memset (counts) and 1 kernel.  No host synchronisation, no allocation, integer atomics only: the update is
// integer, so the state does not depend on the order of the views, on how they are split over calls or on the batch (a saturated voxel
// alone depends on the order, which is the call's).  The single entry is the batch of one problem.
#include <climits>
#include <cmath>
#include <vector>

#include "ls_common.h"
#include "ls_ragged.h"
#include "ls_workspace.h"

// the arithmetic of the definition as written: no contraction of a * b + c into an fma anywhere in this file
#pragma clang fp contract(off)
#include "fuse_plan.h"

namespace ls {
namespace dfu {
using namespace fp;

struct FuseArgs {
    int* sum;                      // [P,nx,ny,nz]
    int* n;                        // [P,nx,ny,nz]
    int ny, nz;
    long long voxels;              // nx ny nz
    long long chunks;              // per problem
    const long long* view_off;     // [P+1], in the workspace
    const double* grids;           // [P,5]: origin, voxel, trunc, in the workspace
    const float* depth;            // [views_total,H,W]
    const double* K;               // [views_total,4]
    const double* E;               // [views_total,3,4]
    int H, W;
    double znear;
    int empty_is_free;
    long long* view_counts;        // [views_total,6]
};

// one integer add per wave: the lanes with `flag`.  Every lane of the wave calls it.
__device__ __forceinline__ void count_wave(bool flag, long long* __restrict__ where) {
    const unsigned long long m = __ballot(flag);
    if ((threadIdx.x & (kWave - 1)) == 0 && m) atomicAdd((unsigned long long*)where, (unsigned long long)__popcll(m));
}

// workgroup = one chunk of voxels of one problem, one thread per voxel: the loop over the problem's views around fuse_voxel_view
__global__ __launch_bounds__(FUSE_CHUNK) void fuse_kernel(FuseArgs G) {
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
            int q;
            cls = fuse_voxel_view(G.E + v * 12, G.K + v * 4, x, G.depth + (size_t)v * image, G.W, G.H, trunc, G.znear, G.empty_is_free != 0, &q);
            cls = fuse_update(cls, q, &sum, &n);
        }
        for (int s = 0; s < FUSE_CLASSES; ++s) count_wave(cls == s, G.view_counts + v * FUSE_CLASSES + s);
    }
    if (live) {
        G.sum[at] = sum;
        G.n[at] = n;
    }
}

// state to volume, one thread per voxel of the whole batch
__global__ __launch_bounds__(FUSE_CHUNK) void volume_kernel(const int* __restrict__ sum, const int* __restrict__ n, long long voxels, long long chunks,
                                                            int min_obs, double* __restrict__ volume, unsigned char* __restrict__ valid_out,
                                                            long long* __restrict__ counts) {
    const long long p = (long long)blockIdx.x / chunks;
    const long long idx = ((long long)blockIdx.x - p * chunks) * FUSE_CHUNK + threadIdx.x;
    const bool live = idx < voxels;
    bool valid = false;
    double D = 1.0;
    int obs = -1;
    if (live) {
        const long long at = p * voxels + idx;
        obs = n[at];
        D = fuse_value(sum[at], obs, min_obs, &valid);
        volume[at] = D;
        valid_out[at] = valid ? 1 : 0;
    }
    long long* cnt = counts + p * VOL_FIELDS;
    count_wave(valid, cnt + VOL_VALID);
    count_wave(valid && D <= 0.0, cnt + VOL_INSIDE);
    count_wave(obs == 0, cnt + VOL_UNSEEN);
}

}  // namespace dfu
}  // namespace ls

using namespace ls;
using namespace ls::dfu;

namespace {
struct Ws {
    long long* words;     // view_off [P+1], then the grids [P,5] as float64
    size_t offs;          // the number of offset words
    size_t bytes;         // of the whole layout
};

// the one layout: the piece of fuse_plan.h from one Arena (ws null: a sizing pass)
Ws layout(void* ws, int P) {
    const FusePieces c = fuse_pieces(P);
    Arena ar(ws);
    Ws w;
    w.words = ar.take<long long>(c.offs + c.grids);
    w.offs = c.offs;
    w.bytes = ar.bytes();
    return w;
}

bool sizes_ok(int P, int nx, int ny, int nz, long long views) { return fuse_sizes_ok(P, nx, ny, nz) && views >= 0 && views <= INT_MAX; }

// everything the host decides, then the copy, the memset and the kernel
int fuse_run(const char* op, int P, int32_t* sum, int32_t* n, int nx, int ny, int nz, const double* origin, const double* voxel, const double* trunc,
             const float* depth, long long views, const long long* view_off, int H, int W, const double* K, const double* E, double znear,
             int empty_is_free, long long* view_counts, void* workspace, size_t workspace_bytes, size_t need, hipStream_t st) {
    LS_REQUIRE(P >= 1, "%s: P must be at least 1, got %d", op, P);
    LS_REQUIRE(nx >= 1 && ny >= 1 && nz >= 1, "%s: dims must be at least 1, got %d x %d x %d", op, nx, ny, nz);
    LS_REQUIRE(fuse_sizes_ok(P, nx, ny, nz), "%s: P * nx * ny * nz = %d * %d * %d * %d reaches 2^31 (int32 state indices)", op, P, nx, ny, nz);
    LS_REQUIRE(views >= 0, "%s: negative size (%lld views)", op, views);
    LS_REQUIRE(views <= INT_MAX, "%s: %lld views exceed %d (int view counts)", op, views, INT_MAX);
    LS_REQUIRE(H >= 1 && W >= 1, "%s: the image must have at least one pixel, got %d x %d", op, H, W);
    LS_REQUIRE(sum && n, "%s: null sum / n", op);
    LS_REQUIRE(origin && voxel && trunc, "%s: null origin / voxel / trunc", op);
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
    const FuseArgs G{sum, n, ny, nz, voxels, chunks, w.words, (const double*)(w.words + w.offs), depth, K, E, H, W, znear, empty_is_free, view_counts};
    LS_HIP_CHECK(hipMemsetAsync(view_counts, 0, (size_t)views * FUSE_CLASSES * sizeof(long long), st));
    hipLaunchKernelGGL(fuse_kernel, dim3((unsigned)(chunks * P)), dim3(FUSE_CHUNK), 0, st, G);
    LS_LAUNCH_CHECK();
    return LS_OK;
}
}  // namespace

extern "C" {

size_t ls_depth_fuse_workspace_bytes(int nx, int ny, int nz, long long views) {
    if (!sizes_ok(1, nx, ny, nz, views)) return 0;
    return layout(nullptr, 1).bytes;
}

int ls_depth_fuse_f32(int32_t* sum, int32_t* n, int nx, int ny, int nz, const double* origin, double voxel, double trunc, const float* depth,
                      long long views, int height, int width, const double* intrinsics, const double* world_to_cam, double znear, int empty_is_free,
                      long long* view_counts, void* workspace, size_t workspace_bytes, void* stream) {
    const long long view_off[2] = {0, views};
    return fuse_run("depth_fuse", 1, sum, n, nx, ny, nz, origin, &voxel, &trunc, depth, views, view_off, height, width, intrinsics, world_to_cam, znear,
                    empty_is_free, view_counts, workspace, workspace_bytes, ls_depth_fuse_workspace_bytes(nx, ny, nz, views), (hipStream_t)stream);
}

size_t ls_depth_fuse_batch_workspace_bytes(int P, int nx, int ny, int nz, long long views_total) {
    if (!sizes_ok(P, nx, ny, nz, views_total)) return 0;
    return layout(nullptr, P).bytes;
}

int ls_depth_fuse_batch_f32(int P, int32_t* sum, int32_t* n, int nx, int ny, int nz, const double* origin, const double* voxel, const double* trunc,
                            const float* depth, long long views_total, const long long* view_off, int height, int width, const double* intrinsics,
                            const double* world_to_cam, double znear, int empty_is_free, long long* view_counts, void* workspace,
                            size_t workspace_bytes, void* stream) {
    return fuse_run("depth_fuse_batch", P, sum, n, nx, ny, nz, origin, voxel, trunc, depth, views_total, view_off, height, width, intrinsics,
                    world_to_cam, znear, empty_is_free, view_counts, workspace, workspace_bytes,
                    ls_depth_fuse_batch_workspace_bytes(P, nx, ny, nz, views_total), (hipStream_t)stream);
}

int ls_tsdf_volume_f64(const int32_t* sum, const int32_t* n, int B, int nx, int ny, int nz, int min_obs, double* volume_out, uint8_t* valid_out,
                       long long* counts_out, void* stream) {
    const char* op = "tsdf_volume";
    LS_REQUIRE(B >= 1, "%s: B must be at least 1, got %d", op, B);
    LS_REQUIRE(nx >= 1 && ny >= 1 && nz >= 1, "%s: dims must be at least 1, got %d x %d x %d", op, nx, ny, nz);
    LS_REQUIRE(fuse_sizes_ok(B, nx, ny, nz), "%s: B * nx * ny * nz = %d * %d * %d * %d reaches 2^31 (int32 state indices)", op, B, nx, ny, nz);
    LS_REQUIRE(min_obs >= 1, "%s: min_obs must be >= 1 (a sample never observed has no distance), got %d", op, min_obs);
    LS_REQUIRE(sum && n && volume_out && valid_out && counts_out, "%s: null sum / n / volume_out / valid_out / counts_out", op);
    hipStream_t st = (hipStream_t)stream;
    const long long voxels = (long long)nx * ny * nz, chunks = fuse_chunks(voxels);
    LS_HIP_CHECK(hipMemsetAsync(counts_out, 0, (size_t)B * VOL_FIELDS * sizeof(long long), st));
    hipLaunchKernelGGL(volume_kernel, dim3((unsigned)(chunks * B)), dim3(FUSE_CHUNK), 0, st, sum, n, voxels, chunks, min_obs, volume_out, valid_out,
                       counts_out);
    LS_LAUNCH_CHECK();
    return LS_OK;
}

}  // extern "C"
