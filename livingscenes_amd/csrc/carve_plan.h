// carve_plan.h -- the see-through test of the scene memory (cloudcarve.hip), the one statement of it: the camera-frame position of a kept
// row under a posed view, the pixel its ray is rounded to, the class of a window pixel against the row's depth, the state of a (row, view)
// from the classes of its window, the rule that drops a row, and the pieces of the workspace.  Pure functions: no HIP, no global state.
// The kernel is a loop around carve_point_view; a plain C++17 compiler accepts the file, and tests/test_cloud_carve_cpu.py replays it
// against the NumPy twin of the definition (tests/carve_oracle.py; the definition itself: include/livingscenes_hip.h, ls_cloud_carve_f32).
// Everything is float64 and no a * b + c is contracted into an fma: clang is told here, any other compiler by -ffp-contract=off.
#pragma once
#include <cmath>
#include <cstddef>

#if defined(__HIPCC__)
#define LS_CP_HD __host__ __device__ inline
#else
#define LS_CP_HD inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace ls {
namespace cp {

enum { CARVE_OUT = 0, CARVE_SEEN, CARVE_FREE, CARVE_OCCLUDED, CARVE_MIXED, CARVE_STATES };   // the state of a (row, view), by value
enum { PIX_EMPTY = 0, PIX_FRONT, PIX_BEHIND, PIX_HIT };                                       // the class of a window pixel
enum { CNT_SEEN = 0, CNT_FREE, CNT_DROPPED, CNT_OUT, CNT_FIELDS };                            // counts[p]
constexpr int CARVE_MAX_WINDOW = 2;       // the window reaches k pixels to every side, k in {0, 1, 2}
constexpr int CARVE_CHUNK = 256;          // rows per workgroup, one per thread, all of ONE problem

LS_CP_HD bool finite64(double v) { return fabs(v) <= 1.7976931348623157e308; }   // NaN fails the comparison

// step 1: c = ((E[:,0] x0 + E[:,1] x1) + E[:,2] x2) + E[:,3], E [3,4] row-major, x the fp32 row widened
LS_CP_HD void carve_camera(const double* E, const float* x, double (&c)[3]) {
    const double x0 = (double)x[0], x1 = (double)x[1], x2 = (double)x[2];
    for (int r = 0; r < 3; ++r) c[r] = ((E[r * 4 + 0] * x0 + E[r * 4 + 1] * x1) + E[r * 4 + 2] * x2) + E[r * 4 + 3];
}

// steps 2 and 3: false = OUT; else the pixel (qx, qy) the row's ray is rounded to.  K = (fx, fy, cx, cy).  The bounds are compared on the
// doubles, so a NaN fails them and the conversion to int is exact.
LS_CP_HD bool carve_pixel(const double (&c)[3], const double* K, int W, int H, double znear, int* qx, int* qy) {
    if (!(finite64(c[0]) && finite64(c[1]) && finite64(c[2])) || c[2] < znear) return false;
    const double u = K[0] * (c[0] / c[2]) + K[2], v = K[1] * (c[1] / c[2]) + K[3];
    const double rx = floor(u + 0.5), ry = floor(v + 0.5);
    if (!(rx >= 0.0 && rx <= (double)(W - 1) && ry >= 0.0 && ry <= (double)(H - 1))) return false;
    *qx = (int)rx;
    *qy = (int)ry;
    return true;
}

// step 4: one window pixel of depth `depth` against the row at depth z
LS_CP_HD int carve_pixel_class(float depth, double z, double tol) {
    const double d = (double)depth;
    if (!(d > 0.0)) return PIX_EMPTY;                    // 0, negative and NaN
    const double lo = d - tol, hi = d + tol;
    if (z < lo) return PIX_FRONT;
    if (z > hi) return PIX_BEHIND;
    return PIX_HIT;                                      // both ends inclusive
}

// step 5: the state of the (row, view) from the classes of the n_in window pixels inside the image (n_in >= 1: the centre pixel is)
LS_CP_HD int carve_state(int n_in, int n_hit, int n_front, int n_behind, int n_empty, bool empty_is_free) {
    if (n_hit > 0) return CARVE_SEEN;
    if (n_front + (empty_is_free ? n_empty : 0) == n_in) return CARVE_FREE;
    if (n_behind > 0 && n_front == 0) return CARVE_OCCLUDED;
    return CARVE_MIXED;
}

// steps 1 - 5 for the row x and one view: E [3,4], K [4], depth [H,W] of that view
LS_CP_HD int carve_point_view(const double* E, const double* K, const float* x, const float* depth, int W, int H, double tol, double znear, int k,
                              bool empty_is_free) {
    double c[3];
    carve_camera(E, x, c);
    int qx, qy;
    if (!carve_pixel(c, K, W, H, znear, &qx, &qy)) return CARVE_OUT;
    int n_in = 0, n_hit = 0, n_front = 0, n_behind = 0, n_empty = 0;
    for (int dy = -k; dy <= k; ++dy) {
        const int y = qy + dy;
        if (y < 0 || y >= H) continue;
        for (int dx = -k; dx <= k; ++dx) {
            const int xx = qx + dx;
            if (xx < 0 || xx >= W) continue;
            const int cls = carve_pixel_class(depth[(size_t)y * (size_t)W + (size_t)xx], c[2], tol);
            ++n_in;
            n_hit += cls == PIX_HIT;
            n_front += cls == PIX_FRONT;
            n_behind += cls == PIX_BEHIND;
            n_empty += cls == PIX_EMPTY;
        }
    }
    return carve_state(n_in, n_hit, n_front, n_behind, n_empty, empty_is_free);
}

// the keep rule: a row is dropped iff at least min_free views look through it and at most max_seen views confirm it
LS_CP_HD bool carve_drop(int seen, int free_views, int min_free, int max_seen) { return free_views >= min_free && seen <= max_seen; }

LS_CP_HD long long carve_chunks(long long a) { return (a + CARVE_CHUNK - 1) / CARVE_CHUNK; }

// the scalars a call accepts: tol finite and >= 0, znear finite and > 0, window in [0, CARVE_MAX_WINDOW], min_free >= 1, max_seen >= 0,
// empty_is_free 0 or 1 -> 0, or the number of the first argument that is refused (1 .. 6, in that order)
LS_CP_HD int carve_bad_scalar(double tol, double znear, int window, int min_free, int max_seen, int empty_is_free) {
    if (!(finite64(tol) && tol >= 0.0)) return 1;
    if (!(finite64(znear) && znear > 0.0)) return 2;
    if (window < 0 || window > CARVE_MAX_WINDOW) return 3;
    if (min_free < 1) return 4;
    if (max_seen < 0) return 5;
    if (empty_is_free != 0 && empty_is_free != 1) return 6;
    return 0;
}

// The pieces of the workspace as element counts, in the order the one Arena of cloudcarve.hip takes them: the device copy of a batch's
// n_off_arrays int64 arrays of P + 1 entries (0: a single problem), the keep flags, their ranks, the scan's block sums (blocks of
// scan_per_block rows: SCAN_PER_BLOCK of ls_scan.h) and its total.  A function of (P, a_total) alone: the views are read where they lie.
struct CarvePieces { size_t offs, keep, pos, blk, total; };
LS_CP_HD CarvePieces carve_pieces(int P, long long a_total, int n_off_arrays, int scan_per_block) {
    CarvePieces c;
    c.offs = (size_t)n_off_arrays * (size_t)(P + 1);
    c.keep = (size_t)a_total;
    c.pos = (size_t)a_total;
    c.blk = (size_t)((a_total + scan_per_block - 1) / scan_per_block);
    c.total = 1;
    return c;
}

}  // namespace cp
}  // namespace ls
