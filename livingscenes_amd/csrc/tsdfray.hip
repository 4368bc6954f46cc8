// tsdfray.hip -- scene memory: the fused state of an instance (depthfuse.hip: sum, n) RAYCAST into depth, normal and state images from
// posed cameras, and a predicted view COMPARED with an observed one.  The definitions are in include/livingscenes_hip.h
// (ls_tsdf_raycast_f64, ls_depth_compare_f32) and, as NumPy, in tests/tsdf_ray_oracle.py; the arithmetic of a ray is tsdfray_plan.h
// (ray_cast), which tests/tools/tsdfray_plan_run.cpp runs on the host; the value at a point is tsdfsample_plan.h's.  What this file adds:
//   raycast    a workgroup owns one 16 x 16 tile of ONE view, one thread per pixel, each wave a compact 8 x 8 block of the tile, so the
//              rays of a wave walk neighbouring cells and their corner gathers hit the same lines.  The view's problem is found from
//              blockIdx alone (a search over view_off): grid, camera and intrinsics stay in scalar registers.  The march is the bounded
//              loop of ray_cast: the trip count is an integer known before the loop; a ray that has stopped idles until its wave is
//              done.  A thread keeps the (sum, n) of its cell's eight corners in registers while consecutive samples stay in the cell
//              (with step <= 1 the same or an adjacent cell): the same numbers, so no bit of the result changes.  The histogram comes
//              from ballots: one integer add per wave, view and state.
//   compare    one thread per pixel, a workgroup on 256 consecutive pixels of one view: the class and the same ballot histogram.
// Launches of a raycast, whatever P and the number of views: the copy of the host arrays into the workspace, 1 memset (counts) and 1
// kernel; of a comparison: 1 memset and 1 kernel.  No host synchronisation, no allocation, no floating-point atomics: every output is
// the same bits in any run and in any batch.  The single entry is the batch of one problem.
#include <climits>
#include <cmath>
#include <vector>

#include "ls_common.h"
#include "ls_ragged.h"
#include "ls_workspace.h"

// the arithmetic of the definition as written: no contraction of a * b + c into an fma anywhere in this file
#pragma clang fp contract(off)
#include "tsdfray_plan.h"

namespace ls {
namespace trk {
using namespace tr;

constexpr int RAY_THREADS = RAY_TILE * RAY_TILE;
static_assert(RAY_THREADS == 4 * kWave && RAY_WAVE_W * RAY_WAVE_H == kWave, "a tile is four waves, each on an 8 x 8 block");

struct RayArgs {
    const int* sum;                // [P,nx,ny,nz]
    const int* n;                  // [P,nx,ny,nz]
    int dims[3];
    long long voxels;              // nx ny nz
    int min_obs, P;
    const long long* view_off;     // [P+1], in the workspace
    const double* grids;           // [P,6]: origin, voxel, trunc, trunc / voxel, in the workspace
    const double* M;               // [views,3,4] camera to memory frame
    const double* K;               // [views,4]
    int H, W, tiles_x;
    long long tiles;               // per view
    double znear, step;
    float* depth;                  // [views,H,W]
    float* normal;                 // [views,H,W,3]
    unsigned char* state;          // [views,H,W]
    long long* counts;             // [views,5]
};

// one integer add per wave: the lanes with `flag`.  Every lane of the wave calls it.
__device__ __forceinline__ void count_wave(bool flag, long long* __restrict__ where) {
    const unsigned long long m = __ballot(flag);
    if ((threadIdx.x & (kWave - 1)) == 0 && m) atomicAdd((unsigned long long*)where, (unsigned long long)__popcll(m));
}

// the eight corners of a cell of one problem's state: 16 loads in flight before the first use
struct DeviceFetch {
    const int* __restrict__ sum;
    const int* __restrict__ n;
    int d0, d1, d2;
    __device__ __forceinline__ void operator()(const int (&i)[3], int (&s)[8], int (&c)[8]) const {
        const int dims[3] = {d0, d1, d2};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const long long at = ts::sample_corner(dims, i, k);
            s[k] = sum[at];
            c[k] = n[at];
        }
    }
};

// workgroup = one tile of one view, one thread per pixel: ray_setup and ray_cast
__global__ __launch_bounds__(RAY_THREADS) void tsdf_raycast_kernel(RayArgs G) {
    const long long v = (long long)blockIdx.x / G.tiles;
    const int tile = (int)((long long)blockIdx.x - v * G.tiles);
    const int p = owner(G.view_off, G.P, v);
    const double* grid = G.grids + (size_t)p * RAY_GRID_WORDS;
    const double origin[3] = {grid[0], grid[1], grid[2]};
    int px, py;
    ray_pixel(tile % G.tiles_x, tile / G.tiles_x, (int)threadIdx.x, &px, &py);
    int st = -1;
    if (px < G.W && py < G.H) {
        double a[3], b[3];
        float depth, nrm[3];
        ray_setup(G.M + v * 12, G.K + v * 4, origin, grid[3], px, py, a, b);
        const DeviceFetch fetch{G.sum + (size_t)p * G.voxels, G.n + (size_t)p * G.voxels, G.dims[0], G.dims[1], G.dims[2]};
        st = ray_cast(a, b, G.dims, G.znear, G.step, G.min_obs, grid[4], grid[5], fetch, &depth, nrm);
        const size_t at = ((size_t)v * G.H + py) * G.W + px;
        G.depth[at] = depth;
        G.normal[at * 3 + 0] = nrm[0];
        G.normal[at * 3 + 1] = nrm[1];
        G.normal[at * 3 + 2] = nrm[2];
        G.state[at] = (unsigned char)st;
    }
    for (int s = 0; s < RAY_STATES; ++s) count_wave(st == s, G.counts + v * RAY_STATES + s);
}

// workgroup = 256 consecutive pixels of one view
__global__ __launch_bounds__(256) void depth_compare_kernel(const float* __restrict__ observed, const float* __restrict__ depth,
                                                            const unsigned char* __restrict__ state, long long pixels, long long chunks, double tol,
                                                            unsigned char* __restrict__ cls_out, long long* __restrict__ counts) {
    const long long v = (long long)blockIdx.x / chunks;
    const long long i = ((long long)blockIdx.x - v * chunks) * 256 + threadIdx.x;
    int cls = -1;
    if (i < pixels) {
        const size_t at = (size_t)v * pixels + i;
        cls = view_class(observed[at], depth[at], state[at], tol);
        cls_out[at] = (unsigned char)cls;
    }
    for (int s = 0; s < VIEW_CLASSES; ++s) count_wave(cls == s, counts + v * VIEW_CLASSES + s);
}

}  // namespace trk
}  // namespace ls

using namespace ls;
using namespace ls::trk;

namespace {
struct Ws {
    long long* words;     // view_off [P+1], then the grids [P,6] as float64
    size_t offs;          // the number of offset words
    size_t bytes;         // of the whole layout
};

// the one layout: the piece of tsdfray_plan.h from one Arena (ws null: a sizing pass)
Ws layout(void* ws, int P) {
    const RayPieces c = ray_pieces(P);
    Arena ar(ws);
    Ws w;
    w.words = ar.take<long long>(c.offs + c.grids);
    w.offs = c.offs;
    w.bytes = ar.bytes();
    return w;
}

// views * tiles workgroups and views * H * W pixels, both below 2^31
bool image_ok(long long views, int H, int W) {
    if (views < 0 || views > INT_MAX || H < 1 || W < 1) return false;
    const long long pixels = (long long)H * (long long)W;                  // < 2^62
    if (pixels >= (1ll << 31)) return false;
    return views == 0 || pixels <= ((1ll << 31) - 1) / views;
}

size_t raycast_need(int P, int nx, int ny, int nz, long long views, int H, int W) {
    if (!fp::fuse_sizes_ok(P, nx, ny, nz) || !image_ok(views, H, W)) return 0;
    return layout(nullptr, P).bytes;
}

// everything the host decides, then the copy, the memset and the kernel
int raycast_run(const char* op, int P, const int32_t* sum, const int32_t* n, int nx, int ny, int nz, int min_obs, const double* origin,
                const double* voxel, const double* trunc, const double* M, const double* K, long long views, const long long* view_off, int H, int W,
                double znear, double step, float* depth, float* normal, uint8_t* state, long long* counts, void* workspace, size_t workspace_bytes,
                hipStream_t st) {
    LS_REQUIRE(P >= 1, "%s: P must be at least 1, got %d", op, P);
    LS_REQUIRE(nx >= 1 && ny >= 1 && nz >= 1, "%s: dims must be at least 1, got %d x %d x %d", op, nx, ny, nz);
    LS_REQUIRE(fp::fuse_sizes_ok(P, nx, ny, nz), "%s: P * nx * ny * nz = %d * %d * %d * %d reaches 2^31 (int32 state indices)", op, P, nx, ny, nz);
    LS_REQUIRE(min_obs >= 1, "%s: min_obs must be >= 1 (a sample never observed has no distance), got %d", op, min_obs);
    LS_REQUIRE(views >= 0, "%s: negative size (%lld views)", op, views);
    LS_REQUIRE(H >= 1 && W >= 1, "%s: the image must have at least one pixel, got %d x %d", op, H, W);
    LS_REQUIRE(image_ok(views, H, W), "%s: %lld views of %d x %d pixels reach 2^31 (int pixel indices)", op, views, H, W);
    LS_REQUIRE(sum && n, "%s: null sum / n", op);
    LS_REQUIRE(origin && voxel && trunc, "%s: null origin / voxel / trunc", op);
    LS_REQUIRE(views == 0 || (M && K && depth && normal && state && counts),
               "%s: null cam_to_world / intrinsics / depth / normal / state / counts with %lld views", op, views);
    int rc = check_ranges(op, "problem", "view_off", P, view_off, views, INT_MAX);
    if (rc != LS_OK) return rc;
    const int bad = ray_bad_scalar(znear, step);
    LS_REQUIRE(bad != 1, "%s: znear must be finite and > 0, got %g", op, znear);
    LS_REQUIRE(bad != 2, "%s: step must lie in [1/16, 1] voxels (above 1 a sample could skip a cell), got %g", op, step);
    const int dims[3] = {nx, ny, nz};
    LS_REQUIRE(ray_max_trips(dims, step) <= RAY_MAX_TRIPS, "%s: dims %d x %d x %d at step %g let a ray take %lld samples, at most %lld", op, nx, ny, nz,
               step, ray_max_trips(dims, step), RAY_MAX_TRIPS);
    const Ws sizes = layout(nullptr, P);
    std::vector<long long> host(sizes.offs + (size_t)P * RAY_GRID_WORDS);
    double* grids = (double*)(host.data() + sizes.offs);                   // 8-byte words both
    for (int p = 0; p < P; ++p) {
        const int badg = fp::fuse_bad_grid(origin + (size_t)p * 3, voxel[p], trunc[p]);
        LS_REQUIRE(badg != 1, "%s: problem %d: origin must be finite, got (%g, %g, %g)", op, p, origin[p * 3], origin[p * 3 + 1], origin[p * 3 + 2]);
        LS_REQUIRE(badg != 2, "%s: problem %d: voxel must be finite and > 0, got %g", op, p, voxel[p]);
        LS_REQUIRE(badg != 3, "%s: problem %d: trunc must be finite and > 0, got %g", op, p, trunc[p]);
        const double toh = ts::sample_trunc_over_h(voxel[p], trunc[p]);
        LS_REQUIRE(toh == toh, "%s: problem %d: trunc / voxel overflows float64 (trunc %g, voxel %g)", op, p, trunc[p], voxel[p]);
        double* gr = grids + (size_t)p * RAY_GRID_WORDS;
        for (int a = 0; a < 3; ++a) gr[a] = origin[(size_t)p * 3 + a];
        gr[3] = voxel[p], gr[4] = trunc[p], gr[5] = toh;
    }
    std::copy(view_off, view_off + P + 1, host.begin());
    const size_t need = raycast_need(P, nx, ny, nz, views, H, W);
    if (!(workspace && workspace_bytes >= need)) {
        set_error("%s: workspace %zu < required %zu (ls_%s_workspace_bytes)", op, workspace ? workspace_bytes : (size_t)0, need, op);
        return LS_ERR_WORKSPACE;
    }
    if (views == 0) return LS_OK;                                          // no problem has a view: nothing is written
    const Ws w = layout(workspace, P);
    rc = upload_offsets(w.words, host, st);
    if (rc != LS_OK) return rc;
    RayArgs G{};
    G.sum = sum, G.n = n;
    G.dims[0] = nx, G.dims[1] = ny, G.dims[2] = nz;
    G.voxels = (long long)nx * ny * nz;
    G.min_obs = min_obs, G.P = P;
    G.view_off = w.words;
    G.grids = (const double*)(w.words + w.offs);
    G.M = M, G.K = K;
    G.H = H, G.W = W, G.tiles_x = (W + RAY_TILE - 1) / RAY_TILE;
    G.tiles = ray_tiles(H, W);
    G.znear = znear, G.step = step;
    G.depth = depth, G.normal = normal, G.state = state, G.counts = counts;
    LS_HIP_CHECK(hipMemsetAsync(counts, 0, (size_t)views * RAY_STATES * sizeof(long long), st));
    hipLaunchKernelGGL(tsdf_raycast_kernel, dim3((unsigned)(views * G.tiles)), dim3(RAY_THREADS), 0, st, G);
    LS_LAUNCH_CHECK();
    return LS_OK;
}
}  // namespace

extern "C" {

size_t ls_tsdf_raycast_workspace_bytes(int nx, int ny, int nz, long long views, int height, int width) {
    return raycast_need(1, nx, ny, nz, views, height, width);
}

size_t ls_tsdf_raycast_batch_workspace_bytes(int P, int nx, int ny, int nz, long long views_total, int height, int width) {
    return raycast_need(P, nx, ny, nz, views_total, height, width);
}

int ls_tsdf_raycast_f64(const int32_t* sum, const int32_t* n, int nx, int ny, int nz, int min_obs, const double* origin, double voxel, double trunc,
                        const double* cam_to_world, const double* intrinsics, long long views, int height, int width, double znear, double step,
                        float* depth, float* normal, uint8_t* state, long long* counts, void* workspace, size_t workspace_bytes, void* stream) {
    const long long view_off[2] = {0, views};
    return raycast_run("tsdf_raycast", 1, sum, n, nx, ny, nz, min_obs, origin, &voxel, &trunc, cam_to_world, intrinsics, views, view_off, height, width,
                       znear, step, depth, normal, state, counts, workspace, workspace_bytes, (hipStream_t)stream);
}

int ls_tsdf_raycast_batch_f64(int P, const int32_t* sum, const int32_t* n, int nx, int ny, int nz, int min_obs, const double* origin,
                              const double* voxel, const double* trunc, const double* cam_to_world, const double* intrinsics, long long views_total,
                              const long long* view_off, int height, int width, double znear, double step, float* depth, float* normal, uint8_t* state,
                              long long* counts, void* workspace, size_t workspace_bytes, void* stream) {
    return raycast_run("tsdf_raycast_batch", P, sum, n, nx, ny, nz, min_obs, origin, voxel, trunc, cam_to_world, intrinsics, views_total, view_off,
                       height, width, znear, step, depth, normal, state, counts, workspace, workspace_bytes, (hipStream_t)stream);
}

int ls_depth_compare_f32(const float* observed, const float* depth, const uint8_t* state, long long views, int height, int width, double tol,
                         uint8_t* cls, long long* counts, void* stream) {
    const char* op = "depth_compare";
    LS_REQUIRE(views >= 0, "%s: negative size (%lld views)", op, views);
    LS_REQUIRE(height >= 1 && width >= 1, "%s: the image must have at least one pixel, got %d x %d", op, height, width);
    LS_REQUIRE(image_ok(views, height, width), "%s: %lld views of %d x %d pixels reach 2^31 (int pixel indices)", op, views, height, width);
    LS_REQUIRE(tol == tol && tol > 0.0, "%s: tol must be > 0, got %g", op, tol);
    LS_REQUIRE(views == 0 || (observed && depth && state && cls && counts), "%s: null observed / depth / state / cls / counts with %lld views", op, views);
    if (views == 0) return LS_OK;
    hipStream_t st = (hipStream_t)stream;
    const long long pixels = (long long)height * width, chunks = (pixels + 255) / 256;
    LS_HIP_CHECK(hipMemsetAsync(counts, 0, (size_t)views * VIEW_CLASSES * sizeof(long long), st));
    hipLaunchKernelGGL(depth_compare_kernel, dim3((unsigned)(views * chunks)), dim3(256), 0, st, observed, depth, state, pixels, chunks, tol, cls, counts);
    LS_LAUNCH_CHECK();
    return LS_OK;
}

}  // extern "C"
