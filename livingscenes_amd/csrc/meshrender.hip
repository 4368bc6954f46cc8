// meshrender.hip -- depth views of triangle meshes and their back-projection to point clouds: the device counterpart of the reference's
// utils/render.py (render_depth renders with pyrender / OpenGL, pointcloud back-projects).  The definition -- projection, snap to 1/256
// pixel, integer edge functions with inclusive edges, perspective-correct depth, the 64-bit (depth bits, face) key whose minimum wins a
// pixel -- is in include/livingscenes_hip.h (ls_mesh_render_depth_f64) and, as NumPy, in tests/render_oracle.py; its integer part is
// render_plan.h.  What this file adds:
//   items      one per (view, face): mesh m of a batch is rendered into the views [view_off[m], view_off[m + 1]), its items are view-major
//   raster     a thread does steps 1 - 5 for its item and walks the clipped box itself when it has at most RENDER_SMALL_BOX pixels; the
//              items of a wave with a larger box are walked by 64 lanes together, one item after the other: by that wave, or -- where the
//              call has few items, so that a few waves would walk whole images -- by one wave per strip of the image in a second pass
//              (render_plan.h: render_strips).  A pixel a face cannot win (plain load of the key, which only ever falls: a stale value
//              is merely conservative) costs no atomic.
//   resolve    key -> depth, face; pixels hit per view
//   points     flag (d > 0), scan (ls_scan.h), scatter: the pixels of every view in ascending pixel index, as np.where lists them
// Integer atomics only (atomicMin on the key, one counter add per wave and view from a ballot): every output is the same bits in any run
// and any batch.  Every kernel is written once, for a mesh locator (OneMesh / RaggedMeshes, as in meshmetrics.hip); the number of launches
// depends on nothing.
#include <climits>
#include <cmath>
#include <vector>

#include "ls_common.h"
#include "ls_ragged.h"
#include "ls_scan.h"

// the arithmetic of the definition as written: no contraction of a * b + c into an fma anywhere in this file
#pragma clang fp contract(off)
#include "render_plan.h"

namespace ls {
namespace mr {
using namespace rp;

enum { CNT_PIXELS = 0, CNT_FACES, CNT_NEAR, CNT_SNAP, CNT_FIELDS };

// ------------------------------------------------------------------------------------------------ which mesh: one, or one of a ragged batch
struct Item {
    const double* V;
    int nv;
    const int32_t* F;
    long long view;
    int face;    // local to the mesh
};

struct OneMesh {
    const double* V;
    int nv;
    const int32_t* F;
    int nf;
    long long n_items;   // n_views * nf
    __device__ long long items() const { return n_items; }
    __device__ Item item(long long g) const { return {V, nv, F, g / nf, (int)(g % nf)}; }   // g < n_items: nf > 0
};

enum { OFF_V = 0, OFF_F, OFF_VIEW, OFF_ITEM, OFF_ARRAYS };   // the device copy of a batch's offsets: vertices, faces, views, items

struct RaggedMeshes {
    const double* V;
    const int32_t* F;
    const long long* offs;
    int M;
    long long n_items;
    __device__ const long long* off(int k) const { return offs + (size_t)k * (M + 1); }
    __device__ long long items() const { return n_items; }
    __device__ Item item(long long g) const {
        const int m = owner(off(OFF_ITEM), M, g);   // a mesh without faces or without views owns no item
        const long long *vo = off(OFF_V), *fo = off(OFF_F);
        const long long nf = fo[m + 1] - fo[m], l = g - off(OFF_ITEM)[m];
        return {V + vo[m] * 3, (int)(vo[m + 1] - vo[m]), F + fo[m] * 3, off(OFF_VIEW)[m] + l / nf, (int)(l % nf)};
    }
};

// ------------------------------------------------------------------------------------------------ steps 1 - 5 of one (view, face)
enum { ST_NONE = 0, ST_RASTER, ST_NEAR, ST_SNAP, ST_BAD_INDEX };   // ST_NONE: nothing to draw (no item, zero area or an empty box)

struct Setup {
    long long xs[3], ys[3], A;
    double iz[3];
    Box box;
    int state;
    bool counted;   // reached step 5 with A != 0
};

__device__ __forceinline__ Setup face_setup(const Item& it, const double* __restrict__ E, const double* __restrict__ K, int W, int H, double znear) {
    Setup s{};
    s.state = ST_NONE;
    s.box = {0, -1, 0, -1};
    const double fx = K[0], fy = K[1], cx = K[2], cy = K[3];
    double u[3], v[3];
    bool near = false;
    for (int i = 0; i < 3; ++i) {
        const int vi = it.F[(size_t)it.face * 3 + i];
        if ((unsigned)vi >= (unsigned)it.nv) {
            s.state = ST_BAD_INDEX;
            return s;
        }
        const double x = it.V[(size_t)vi * 3 + 0], y = it.V[(size_t)vi * 3 + 1], z = it.V[(size_t)vi * 3 + 2];
        double c[3];
        for (int r = 0; r < 3; ++r) c[r] = ((E[r * 4 + 0] * x + E[r * 4 + 1] * y) + E[r * 4 + 2] * z) + E[r * 4 + 3];
        if (!(c[2] >= znear) || !(fabs(c[2]) <= DBL_MAX)) near = true;   // c.z < znear, NaN or inf
        u[i] = fx * (c[0] / c[2]) + cx;
        v[i] = fy * (c[1] / c[2]) + cy;
        s.iz[i] = 1.0 / c[2];
    }
    if (near) {
        s.state = ST_NEAR;
        return s;
    }
    bool ok = true;
    for (int i = 0; i < 3; ++i) {
        s.xs[i] = s.ys[i] = 0;
        ok = snap(u[i], &s.xs[i]) && ok;
        ok = snap(v[i], &s.ys[i]) && ok;
    }
    if (!ok) {
        s.state = ST_SNAP;
        return s;
    }
    s.A = area2(s.xs, s.ys);
    if (s.A == 0) return s;
    s.counted = true;
    s.box = pixel_box(s.xs, s.ys, W, H);
    if (!box_empty(s.box)) s.state = ST_RASTER;
    return s;
}

// step 6 and 7 at pixel (px, py) of the view whose keys are `keys`
__device__ __forceinline__ void shade(const long long (&xs)[3], const long long (&ys)[3], const double (&iz)[3], int face, int px, int py, int W,
                                      unsigned long long* __restrict__ keys) {
    const long long X = (long long)RENDER_SUB * px, Y = (long long)RENDER_SUB * py;
    const long long e0 = edge(xs, ys, 1, 2, X, Y), e1 = edge(xs, ys, 2, 0, X, Y), e2 = edge(xs, ys, 0, 1, X, Y);
    if (!covered(e0, e1, e2)) return;
    const double z = (double)(e0 + e1 + e2) / (((double)e0 * iz[0] + (double)e1 * iz[1]) + (double)e2 * iz[2]);
    const unsigned long long key = pixel_key(__float_as_uint((float)z), face);
    unsigned long long* k = keys + (size_t)py * W + px;
    if (*k <= key) return;   // it cannot win
    atomicMin(k, key);
}

__device__ __forceinline__ long long bcast(long long v, int src) {
    const int lo = __shfl((int)(unsigned)(unsigned long long)v, src), hi = __shfl((int)((unsigned long long)v >> 32), src);
    return (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}
__device__ __forceinline__ double bcast(double v, int src) { return __longlong_as_double(bcast(__double_as_longlong(v), src)); }

// counts[view][which] += the lanes of the wave with `flag` and that view: one add per wave and view.  Every lane of the wave calls it.
__device__ __forceinline__ void count_per_view(bool flag, long long view, int which, unsigned long long* __restrict__ counts) {
    const int lane = threadIdx.x & (kWave - 1);
    unsigned long long todo = __ballot(flag);
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        const long long v = bcast(view, src);
        const unsigned long long same = __ballot(flag && view == v);
        if (lane == src) atomicAdd(&counts[(size_t)v * CNT_FIELDS + which], (unsigned long long)__popcll(same));
        todo &= ~same;
    }
}

// the lanes of a wave walk together, one after the other, the boxes of its lanes with `big`, clipped to the rows [row0, row1]
__device__ __forceinline__ void walk_large(unsigned long long big, const Setup& s, const Item& it, int row0, int row1, int W, size_t image,
                                           unsigned long long* __restrict__ keys) {
    const int lane = threadIdx.x & (kWave - 1);
    while (big) {   // the same for every lane of the wave
        const int src = __ffsll((long long)big) - 1;
        big &= big - 1;
        long long xs[3], ys[3];
        double iz[3];
        for (int i = 0; i < 3; ++i) {
            xs[i] = bcast(s.xs[i], src);
            ys[i] = bcast(s.ys[i], src);
            iz[i] = bcast(s.iz[i], src);
        }
        const int x0 = __shfl(s.box.x0, src), x1 = __shfl(s.box.x1, src);
        const int y0 = max(__shfl(s.box.y0, src), row0), y1 = min(__shfl(s.box.y1, src), row1);
        const int face = __shfl(it.face, src);
        unsigned long long* kv = keys + (size_t)bcast(it.view, src) * image;
        if (y0 > y1) continue;
        const int bw = x1 - x0 + 1, n = bw * (y1 - y0 + 1);   // at most H W < 2^31
        for (int p = lane; p < n; p += kWave) shade(xs, ys, iz, face, x0 + p % bw, y0 + p / bw, W, kv);
    }
}

// keys [views,H,W] start at RENDER_NO_KEY, counts [views,4] at 0, *status at 0.  own_large: no strip pass follows (render_plan.h)
template <class Meshes>
__global__ __launch_bounds__(256) void raster_kernel(Meshes L, const double* __restrict__ E, const double* __restrict__ K, int H, int W, double znear,
                                                     bool own_large, unsigned long long* __restrict__ keys, unsigned long long* __restrict__ counts,
                                                     int* __restrict__ status) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool live = g < L.items();   // no early return: the lanes of a wave work together below
    Item it{nullptr, 0, nullptr, 0, 0};
    Setup s{};
    s.state = ST_NONE;
    if (live) {
        it = L.item(g);
        s = face_setup(it, E + it.view * 12, K + it.view * 4, W, H, znear);
        if (s.state == ST_BAD_INDEX) *status = LS_ERR_INVALID;
    }
    count_per_view(s.counted, it.view, CNT_FACES, counts);
    count_per_view(s.state == ST_NEAR, it.view, CNT_NEAR, counts);
    count_per_view(s.state == ST_SNAP, it.view, CNT_SNAP, counts);
    const size_t image = (size_t)H * W;
    const bool draw = s.state == ST_RASTER;
    if (draw && box_small(s.box)) {
        unsigned long long* kv = keys + (size_t)it.view * image;
        for (int py = s.box.y0; py <= s.box.y1; ++py)
            for (int px = s.box.x0; px <= s.box.x1; ++px) shade(s.xs, s.ys, s.iz, it.face, px, py, W, kv);
    }
    if (own_large) walk_large(__ballot(draw && !box_small(s.box)), s, it, 0, H - 1, W, image, keys);
}

// the strip pass: one wave per (64 items, strip of `rows` rows) repeats steps 1 - 5 for its items and walks their large boxes inside its
// strip.  rows == 0: the rasteriser walked them itself, nothing to do.
template <class Meshes>
__global__ __launch_bounds__(64) void strip_kernel(Meshes L, const double* __restrict__ E, const double* __restrict__ K, int H, int W, double znear,
                                                   int rows, unsigned long long* __restrict__ keys) {
    if (rows == 0) return;
    const long long g = (long long)blockIdx.x * kWave + threadIdx.x;
    Item it{nullptr, 0, nullptr, 0, 0};
    Setup s{};
    s.state = ST_NONE;
    if (g < L.items()) {
        it = L.item(g);
        s = face_setup(it, E + it.view * 12, K + it.view * 4, W, H, znear);
    }
    const int row0 = blockIdx.y * rows;
    walk_large(__ballot(s.state == ST_RASTER && !box_small(s.box)), s, it, row0, min(row0 + rows, H) - 1, W, (size_t)H * W, keys);
}

// depth [views,H,W] (0: nothing hit), face [views,H,W] (-1: none), counts[view][CNT_PIXELS]
__global__ __launch_bounds__(256) void resolve_kernel(const unsigned long long* __restrict__ keys, long long n, long long image, float* __restrict__ depth,
                                                      int32_t* __restrict__ face, unsigned long long* __restrict__ counts) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    bool hit = false;
    if (g < n) {
        const unsigned long long k = keys[g];
        hit = k != RENDER_NO_KEY;
        depth[g] = hit ? __uint_as_float((unsigned)(k >> 32)) : 0.0f;
        face[g] = hit ? (int32_t)(unsigned)k : -1;
    }
    count_per_view(hit, g < n ? g / image : 0, CNT_PIXELS, counts);
}

// ------------------------------------------------------------------------------------------------ back-projection
__global__ __launch_bounds__(256) void hit_flag_kernel(const float* __restrict__ depth, long long n, int* __restrict__ flag) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g < n) flag[g] = depth[g] > 0.0f ? 1 : 0;
}

// the hit pixels at their rank pos[g] (the exclusive scan of flag): point (M null: in the camera frame) and pixel index py W + px
__global__ __launch_bounds__(256) void points_kernel(const float* __restrict__ depth, long long n, int H, int W, const double* __restrict__ K,
                                                     const double* __restrict__ M, const int* __restrict__ flag, const int* __restrict__ pos,
                                                     float* __restrict__ pts, int32_t* __restrict__ pix) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= n || !flag[g]) return;
    const long long image = (long long)H * W, view = g / image;
    const int p = (int)(g - view * image), py = p / W, px = p - py * W;
    const double* k = K + view * 4;
    const double d = (double)depth[g];
    const double xc = (((double)px - k[2]) / k[0]) * d, yc = (((double)py - k[3]) / k[1]) * d, zc = d;
    const long long o = pos[g];
    if (M) {
        const double* m = M + view * 12;
        for (int r = 0; r < 3; ++r) pts[o * 3 + r] = (float)(((m[r * 4 + 0] * xc + m[r * 4 + 1] * yc) + m[r * 4 + 2] * zc) + m[r * 4 + 3]);
    } else {
        pts[o * 3 + 0] = (float)xc;
        pts[o * 3 + 1] = (float)yc;
        pts[o * 3 + 2] = (float)zc;
    }
    pix[o] = p;
}

// off[v] = the rank of view v's first pixel, off[views] = the total
__global__ __launch_bounds__(256) void point_offsets_kernel(const int* __restrict__ pos, const long long* __restrict__ total, long long views,
                                                            long long image, long long* __restrict__ off) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v > views) return;
    off[v] = v < views ? (long long)pos[v * image] : *total;
}

}  // namespace mr
}  // namespace ls

using namespace ls;
using namespace ls::mr;

namespace {
constexpr long long MAX_PIXELS = INT_MAX;   // views H W: int32 pixel ranks

// the launch sequence: the meshes located by L, n_items (view, face) items, `views` images
template <class Meshes>
int render_launch(const Meshes& L, long long n_items, long long views, const double* E, const double* K, int H, int W, double znear,
                  unsigned long long* keys, float* depth_out, int32_t* face_out, long long* counts_out, int* status_out, hipStream_t st) {
    const long long n = views * H * W;
    LS_HIP_CHECK(hipMemsetAsync(keys, 0xFF, (size_t)n * sizeof(unsigned long long), st));   // RENDER_NO_KEY
    LS_HIP_CHECK(hipMemsetAsync(counts_out, 0, (size_t)views * CNT_FIELDS * sizeof(long long), st));
    LS_HIP_CHECK(hipMemsetAsync(status_out, 0, sizeof(int), st));
    unsigned long long* counts = (unsigned long long*)counts_out;
    const Strips strips = render_strips(n_items, H);
    const bool own_large = strips.count == 1;
    hipLaunchKernelGGL(raster_kernel<Meshes>, dim3(std::max(cdiv(n_items, 256), 1)), dim3(256), 0, st, L, E, K, H, W, znear, own_large, keys, counts,
                       status_out);
    hipLaunchKernelGGL(strip_kernel<Meshes>, own_large ? dim3(1) : dim3(std::max(cdiv(n_items, kWave), 1), strips.count), dim3(kWave), 0, st, L, E, K,
                       H, W, znear, own_large ? 0 : strips.rows, keys);
    hipLaunchKernelGGL(resolve_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, keys, n, (long long)H * W, depth_out, face_out, counts);
    LS_LAUNCH_CHECK();
    return LS_OK;
}

int check_render(const char* op, long long views, int H, int W, double znear, const double* E, const double* K, const float* depth_out,
                 const int32_t* face_out, const long long* counts_out, const int* status_out) {
    LS_REQUIRE(views >= 0, "%s: negative number of views (%lld)", op, views);
    LS_REQUIRE(H >= 1 && W >= 1, "%s: the image must have at least one pixel, got %d x %d", op, H, W);
    LS_REQUIRE(views * (long long)H <= MAX_PIXELS && views * (long long)H * W <= MAX_PIXELS, "%s: %lld views of %d x %d pixels exceed %lld pixels (int32 pixel ranks)",
               op, views, H, W, MAX_PIXELS);
    LS_REQUIRE(znear > 0 && znear < (double)INFINITY, "%s: znear must be positive and finite, got %g", op, znear);
    LS_REQUIRE(status_out, "%s: null status_out", op);
    LS_REQUIRE(views == 0 || (E && K && depth_out && face_out && counts_out), "%s: null world_to_cam / intrinsics / depth_out / face_out / counts_out", op);
    return LS_OK;
}

size_t render_bytes(long long views, int H, int W, int M, int n_off_arrays) {
    if (views < 0 || H < 1 || W < 1 || M < 0 || views * (long long)H > MAX_PIXELS || views * (long long)H * W > MAX_PIXELS) return 0;
    return render_layout(views, H, W, M, n_off_arrays).bytes;
}

int check_render_workspace(const char* op, const void* ws, size_t have, size_t need) {
    if (need && (!ws || have < need)) {
        set_error("%s: workspace too small (%zu bytes, need %zu: ls_%s_workspace_bytes)", op, have, need, op);
        return LS_ERR_WORKSPACE;
    }
    return LS_OK;
}
}  // namespace

extern "C" {

size_t ls_mesh_render_depth_workspace_bytes(int n_views, int height, int width) { return render_bytes(n_views, height, width, 1, 0); }

int ls_mesh_render_depth_f64(const double* vertices, int nv, const int32_t* faces, int nf, int n_views, const double* world_to_cam,
                             const double* intrinsics, int height, int width, double znear, float* depth_out, int32_t* face_out,
                             long long* counts_out, int* status_out, void* workspace, size_t workspace_bytes, void* stream) {
    const char* op = "mesh_render_depth";
    LS_REQUIRE(nv >= 0 && nf >= 0, "%s: negative size (nv %d, nf %d)", op, nv, nf);
    LS_REQUIRE(nf == 0 || (vertices && faces && nv > 0), "%s: null vertices / faces with nf = %d", op, nf);
    int rc = check_render(op, n_views, height, width, znear, world_to_cam, intrinsics, depth_out, face_out, counts_out, status_out);
    if (rc != LS_OK) return rc;
    const long long n_items = (long long)n_views * nf;
    LS_REQUIRE(n_items <= INT_MAX, "%s: %d views of %d faces exceed %d (view, face) items", op, n_views, nf, INT_MAX);
    hipStream_t st = (hipStream_t)stream;
    if (n_views == 0) {
        LS_HIP_CHECK(hipMemsetAsync(status_out, 0, sizeof(int), st));
        return LS_OK;
    }
    rc = check_render_workspace(op, workspace, workspace_bytes, ls_mesh_render_depth_workspace_bytes(n_views, height, width));
    if (rc != LS_OK) return rc;
    const RenderLayout l = render_layout(n_views, height, width, 1, 0);
    return render_launch(OneMesh{vertices, nv, faces, nf, n_items}, n_items, n_views, world_to_cam, intrinsics, height, width, znear,
                         (unsigned long long*)((char*)workspace + l.keys), depth_out, face_out, counts_out, status_out, st);
}

size_t ls_mesh_render_depth_batch_workspace_bytes(int M, long long views_total, int height, int width) {
    return render_bytes(views_total, height, width, M, OFF_ARRAYS);
}

int ls_mesh_render_depth_batch_f64(int M, const double* vertices, long long nv_total, const long long* vert_off, const int32_t* faces,
                                   long long nf_total, const long long* face_off, long long views_total, const long long* view_off,
                                   const double* world_to_cam, const double* intrinsics, int height, int width, double znear, float* depth_out,
                                   int32_t* face_out, long long* counts_out, int* status_out, void* workspace, size_t workspace_bytes,
                                   void* stream) {
    const char* op = "mesh_render_depth_batch";
    LS_REQUIRE(M >= 0 && nv_total >= 0 && nf_total >= 0, "%s: negative size (M %d, nv_total %lld, nf_total %lld)", op, M, nv_total, nf_total);
    int rc = check_ranges(op, "mesh", "vert_off", M, vert_off, nv_total, INT_MAX);
    if (rc != LS_OK) return rc;
    rc = check_ranges(op, "mesh", "face_off", M, face_off, nf_total, INT_MAX);
    if (rc != LS_OK) return rc;
    rc = check_render(op, views_total, height, width, znear, world_to_cam, intrinsics, depth_out, face_out, counts_out, status_out);
    if (rc != LS_OK) return rc;
    rc = check_ranges(op, "mesh", "view_off", M, view_off, views_total, INT_MAX);
    if (rc != LS_OK) return rc;
    LS_REQUIRE(nf_total == 0 || (vertices && faces), "%s: null vertices / faces with nf_total = %lld", op, nf_total);
    std::vector<long long> item_off(M + 1, 0);
    for (int m = 0; m < M; ++m) {
        const long long nf = face_off[m + 1] - face_off[m], nvw = view_off[m + 1] - view_off[m];
        LS_REQUIRE(nf == 0 || vert_off[m + 1] > vert_off[m], "%s: mesh %d: %lld faces and no vertices", op, m, nf);
        item_off[m + 1] = item_off[m] + nf * nvw;   // each factor is at most INT_MAX
        LS_REQUIRE(item_off[m + 1] <= INT_MAX, "%s: more than %d (view, face) items up to mesh %d", op, INT_MAX, m);
    }
    hipStream_t st = (hipStream_t)stream;
    if (views_total == 0) {
        LS_HIP_CHECK(hipMemsetAsync(status_out, 0, sizeof(int), st));
        return LS_OK;
    }
    rc = check_render_workspace(op, workspace, workspace_bytes, ls_mesh_render_depth_batch_workspace_bytes(M, views_total, height, width));
    if (rc != LS_OK) return rc;
    const RenderLayout l = render_layout(views_total, height, width, M, OFF_ARRAYS);
    long long* offs = (long long*)((char*)workspace + l.offs);
    rc = upload_offsets(offs, pack_offsets(M, {vert_off, face_off, view_off, item_off.data()}), st);
    if (rc != LS_OK) return rc;
    return render_launch(RaggedMeshes{vertices, faces, offs, M, item_off[M]}, item_off[M], views_total, world_to_cam, intrinsics, height, width,
                         znear, (unsigned long long*)((char*)workspace + l.keys), depth_out, face_out, counts_out, status_out, st);
}

namespace {
struct PointsWs {
    int* flag;
    int* pos;
    int* blk;
    long long* total;
    size_t bytes;
};
PointsWs points_layout(void* ws, long long n) {
    Arena a(ws);
    PointsWs w;
    w.flag = a.take<int>((size_t)n);
    w.pos = a.take<int>((size_t)n);
    w.blk = a.take<int>((size_t)scan_blocks(n));
    w.total = a.take<long long>(1);
    w.bytes = a.bytes();
    return w;
}
bool points_sizes_ok(long long views, int H, int W) {
    return views >= 0 && H >= 1 && W >= 1 && views * (long long)H <= SCAN_MAX_N && views * (long long)H * W <= SCAN_MAX_N;
}
}  // namespace

size_t ls_depth_points_workspace_bytes(long long views, int height, int width) {
    if (!points_sizes_ok(views, height, width)) return 0;
    return points_layout(nullptr, views * height * width).bytes;
}

int ls_depth_points_f32(const float* depth, long long views, int height, int width, const double* intrinsics, const double* cam_to_world,
                        float* pts_out, int32_t* pix_out, long long* off_out, void* workspace, size_t workspace_bytes, void* stream) {
    const char* op = "depth_points";
    LS_REQUIRE(views >= 0 && height >= 1 && width >= 1, "%s: %lld views of %d x %d pixels", op, views, height, width);
    LS_REQUIRE(points_sizes_ok(views, height, width), "%s: %lld views of %d x %d pixels exceed %lld pixels (the scan's reach)", op, views, height,
               width, SCAN_MAX_N);
    LS_REQUIRE(off_out, "%s: null off_out", op);
    hipStream_t st = (hipStream_t)stream;
    const long long n = views * height * width;
    if (n == 0) {
        LS_HIP_CHECK(hipMemsetAsync(off_out, 0, sizeof(long long), st));
        return LS_OK;
    }
    LS_REQUIRE(depth && intrinsics && pts_out && pix_out, "%s: null depth / intrinsics / pts_out / pix_out", op);
    const int rc = check_render_workspace(op, workspace, workspace_bytes, ls_depth_points_workspace_bytes(views, height, width));
    if (rc != LS_OK) return rc;
    const PointsWs w = points_layout(workspace, n);
    const int nb = cdiv(n, 256);
    hipLaunchKernelGGL(hit_flag_kernel, dim3(nb), dim3(256), 0, st, depth, n, w.flag);
    scan<int, int, false>(w.flag, n, w.blk, w.pos, w.total, st);
    hipLaunchKernelGGL(points_kernel, dim3(nb), dim3(256), 0, st, depth, n, height, width, intrinsics, cam_to_world, w.flag, w.pos, pts_out, pix_out);
    hipLaunchKernelGGL(point_offsets_kernel, dim3(cdiv(views + 1, 256)), dim3(256), 0, st, w.pos, w.total, views, (long long)height * width, off_out);
    LS_LAUNCH_CHECK();
    return LS_OK;
}

}  // extern "C"
