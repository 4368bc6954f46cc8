// plane_plan.h -- the normals of a depth map and the weighted point-to-plane depth fusion of the scene memory (depthplane.hip), the one
// statement of both: the back-projected point of a pixel, the usable neighbours, the two differences, the normal and its state; the
// class, the quantised value and the integer weight of a (voxel, view), the weighted update of the state, what a call accepts and the
// pieces of the workspaces.  Pure functions: no HIP, no global state.  The kernels are loops around plane_normal and plane_voxel_view /
// plane_update; a plain C++17 compiler accepts the file, and tests/test_depth_plane_cpu.py replays it against the NumPy twin of the
// definitions (tests/plane_oracle.py; the definitions themselves: include/livingscenes_hip.h, ls_depth_normals_f32 and
// ls_depth_fuse_weighted_f32).  Steps 1 - 5 of the weighted fuse ARE those of the fuse: fuse_camera and fuse_distance (fuse_plan.h) and
// carve_pixel (carve_plan.h) are called, not restated.  Everything is float64 and no a * b + c is contracted into an fma: clang is told
// here, any other compiler by -ffp-contract=off.
#pragma once
#include <cmath>
#include <cstddef>

#include "fuse_plan.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace ls {
namespace pp {

using cp::finite64;

enum { DN_NO_DEPTH = 0, DN_VALID, DN_NO_NEIGHBOUR, DN_DEGENERATE, DN_STATES };                               // the state of a pixel, by value
enum { FW_OUT = 0, FW_EMPTY, FW_OCCLUDED, FW_NEAR_PLANE, FW_NEAR_PROJ, FW_FREE, FW_SATURATED, FW_CLASSES };   // the class of a (voxel, view)
enum { FW_W_PLANE = 0, FW_W_PROJ, FW_W_FREE, FW_W_EMPTY, FW_WEIGHTS };                                        // weights[4]
constexpr int DN_CHUNK = 256;             // pixels per workgroup, one per thread, all of ONE view
constexpr int FW_MAX_WEIGHT = 255;        // a weight is an integer in 1 .. 255

// ------------------------------------------------------------------------------------------------ the normals of a depth map
// a DEPTH pixel: d finite and > 0 (NaN fails both)
LS_CP_HD bool plane_is_depth(double d) { return finite64(d) && d > 0.0; }

// P(x, y) = (d * ((double)x - cx) / fx, d * ((double)y - cy) / fy, d): the product first, then the quotient.  K = (fx, fy, cx, cy)
LS_CP_HD void plane_point(double d, int x, int y, const double* K, double (&P)[3]) {
    P[0] = d * ((double)x - K[2]) / K[0];
    P[1] = d * ((double)y - K[3]) / K[1];
    P[2] = d;
}

// the neighbour (x, y) of a pixel of depth d: usable iff inside the image, a DEPTH pixel and |d_nb - d| <= max_jump -> its point
LS_CP_HD bool plane_neighbour(const float* depth, int W, int H, int x, int y, double d, double max_jump, const double* K, double (&P)[3]) {
    if (x < 0 || x >= W || y < 0 || y >= H) return false;
    const double dn = (double)depth[(size_t)y * (size_t)W + (size_t)x];
    if (!plane_is_depth(dn) || !(fabs(dn - d) <= max_jump)) return false;
    plane_point(dn, x, y, K, P);
    return true;
}

// the difference along one axis (dx, dy) = (1, 0) or (0, 1): central if both neighbours are usable, else forward, else backward, else none
LS_CP_HD bool plane_difference(const float* depth, int W, int H, int x, int y, int dx, int dy, double d, double max_jump, const double* K,
                               const double (&P)[3], double (&a)[3]) {
    double Pp[3], Pm[3];
    const bool up = plane_neighbour(depth, W, H, x + dx, y + dy, d, max_jump, K, Pp);
    const bool um = plane_neighbour(depth, W, H, x - dx, y - dy, d, max_jump, K, Pm);
    if (!up && !um) return false;
    for (int r = 0; r < 3; ++r) a[r] = (up ? Pp[r] : P[r]) - (um ? Pm[r] : P[r]);
    return true;
}

// the whole definition for the pixel (x, y) of one view: depth [H,W], K [4] -> the state; n = the float64 normal rounded ONCE to fp32,
// (0, 0, 0) unless VALID
LS_CP_HD int plane_normal(const float* depth, int W, int H, int x, int y, const double* K, double max_jump, float (&n)[3]) {
    n[0] = n[1] = n[2] = 0.0f;
    const double d = (double)depth[(size_t)y * (size_t)W + (size_t)x];
    if (!plane_is_depth(d)) return DN_NO_DEPTH;
    double P[3], a[3], b[3];
    plane_point(d, x, y, K, P);
    const bool ha = plane_difference(depth, W, H, x, y, 1, 0, d, max_jump, K, P, a);
    const bool hb = plane_difference(depth, W, H, x, y, 0, 1, d, max_jump, K, P, b);
    if (!(ha && hb)) return DN_NO_NEIGHBOUR;
    const double m[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
    const double mm = (m[0] * m[0] + m[1] * m[1]) + m[2] * m[2];
    if (!(finite64(mm) && mm > 0.0)) return DN_DEGENERATE;                 // 0, inf and NaN (mm is a sum of squares: never negative)
    const double len = sqrt(mm);
    double u[3] = {m[0] / len, m[1] / len, m[2] / len};
    const double t = (u[0] * P[0] + u[1] * P[1]) + u[2] * P[2];
    if (!(t < 0.0 || t > 0.0)) return DN_DEGENERATE;                       // the plane holds the camera centre (or t is NaN)
    if (t > 0.0) {
        for (int r = 0; r < 3; ++r) u[r] = -u[r];                          // faces the camera: n . P < 0
    }
    for (int r = 0; r < 3; ++r) n[r] = (float)u[r];
    return DN_VALID;
}

LS_CP_HD long long plane_chunks(long long pixels) { return (pixels + DN_CHUNK - 1) / DN_CHUNK; }

// the sizes the normals accept: views >= 0, H, W >= 1 and max(views, 1) H W < 2^31 (int32 pixel indices, the launch grid)
LS_CP_HD bool plane_sizes_ok(long long views, int H, int W) {
    if (views < 0 || H < 1 || W < 1) return false;
    const long long lim = 1ll << 31;
    const long long px = (long long)H * (long long)W;                    // < 2^62
    if (px >= lim || views >= lim) return false;
    return px * (views > 0 ? views : 1) < lim;
}

// max_jump of one view: finite and > 0
LS_CP_HD bool plane_bad_jump(double max_jump) { return !(finite64(max_jump) && max_jump > 0.0); }

// the workspace of the normals in 8-byte words: the device copy of max_jump [views] float64 (at least one word)
LS_CP_HD size_t plane_pieces(long long views) { return (size_t)(views > 0 ? views : 1); }

// ------------------------------------------------------------------------------------------------ the weighted fuse
// the weights of a call: each in 1 .. FW_MAX_WEIGHT -> -1, or the index of the first one that is refused
LS_CP_HD int plane_bad_weight(const int* weights) {
    for (int k = 0; k < FW_WEIGHTS; ++k)
        if (weights[k] < 1 || weights[k] > FW_MAX_WEIGHT) return k;
    return -1;
}

// a normal the fuse can use: three finite components, not all of them zero (the normals kernel writes (0, 0, 0) unless VALID)
LS_CP_HD bool plane_usable_normal(const float* n) {
    const double a = (double)n[0], b = (double)n[1], c = (double)n[2];
    return finite64(a) && finite64(b) && finite64(c) && (a != 0.0 || b != 0.0 || c != 0.0);
}

// the NEAR value against the plane of the pixel: s_n = ((n_x (c_x - p_x) + n_y (c_y - p_y)) + n_z (c_z - p_z)), clamped to [-trunc, trunc]
// (a NaN -- an overflow of the caller's normal -- reads -trunc), q = (int) floor(value / trunc * 16384 + 0.5)
LS_CP_HD int plane_value(const float* n, const double (&c)[3], const double (&p)[3], double trunc) {
    const double s = (((double)n[0] * (c[0] - p[0]) + (double)n[1] * (c[1] - p[1])) + (double)n[2] * (c[2] - p[2]));
    const double value = s > -trunc ? (s < trunc ? s : trunc) : -trunc;
    return (int)floor(value / trunc * (double)fp::FUSE_SCALE + 0.5);
}

// all steps before the update for the voxel at x and one view: E [3,4], K [4], depth [H,W] and normals [H,W,3] (nullable) of that view
// -> the class; *q = the quantised value and *w = the weight of a NEAR_PLANE, NEAR_PROJ or FREE voxel-view, else 0
LS_CP_HD int plane_voxel_view(const double* E, const double* K, const double (&x)[3], const float* depth, const float* normals, int W, int H,
                              double trunc, double znear, bool empty_is_free, const int* weights, int* q, int* w) {
    double c[3];
    fp::fuse_camera(E, x, c);                                              // step 1
    int qx, qy;
    *q = 0;
    *w = 0;
    if (!cp::carve_pixel(c, K, W, H, znear, &qx, &qy)) return FW_OUT;      // steps 2 and 3
    const size_t at = (size_t)qy * (size_t)W + (size_t)qx;
    const float dpx = depth[at];
    const int cls = fp::fuse_distance(dpx, c[2], trunc, empty_is_free, q);  // steps 4 and 5, and the projective q
    if (cls == fp::FUSE_EMPTY) return FW_EMPTY;
    if (cls == fp::FUSE_OCCLUDED) return FW_OCCLUDED;
    if (cls == fp::FUSE_FREE) {
        *w = (double)dpx > 0.0 ? weights[FW_W_FREE] : weights[FW_W_EMPTY];
        return FW_FREE;
    }
    if (normals && plane_usable_normal(normals + at * 3)) {
        double p[3];
        plane_point((double)dpx, qx, qy, K, p);
        *q = plane_value(normals + at * 3, c, p, trunc);
        *w = weights[FW_W_PLANE];
        return FW_NEAR_PLANE;
    }
    *w = weights[FW_W_PROJ];
    return FW_NEAR_PROJ;
}

// the update: the state of the voxel takes a NEAR_PLANE, NEAR_PROJ or FREE voxel-view unless n + w would pass 65535 -> the class counted
LS_CP_HD int plane_update(int cls, int q, int w, int* sum, int* n) {
    if (cls != FW_NEAR_PLANE && cls != FW_NEAR_PROJ && cls != FW_FREE) return cls;
    if (*n + w > fp::FUSE_MAX_OBS) return FW_SATURATED;
    *sum += w * q;
    *n += w;
    return cls;
}

}  // namespace pp
}  // namespace ls
