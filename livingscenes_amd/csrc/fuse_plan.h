// fuse_plan.h -- the depth fusion of the scene memory (depthfuse.hip), the one statement of it: the position of a voxel, its camera-frame
// position under a posed view, the class of the (voxel, view) against the pixel its ray is rounded to, the quantised truncated distance,
// the integer update of the state, the value of a sample of the volume, what a call accepts and the pieces of the workspace.  Pure
// functions: no HIP, no global state.  The kernel is a loop around fuse_voxel_view and fuse_update; a plain C++17 compiler accepts the
// file, and tests/test_depth_fuse_cpu.py replays it against the NumPy twin of the definition (tests/fuse_oracle.py; the definition
// itself: include/livingscenes_hip.h, ls_depth_fuse_f32).  The projection (steps 2 and 3) is the carve's, carve_plan.h: carve_pixel.
// Everything is float64 and no a * b + c is contracted into an fma: clang is told here, any other compiler by -ffp-contract=off.
#pragma once
#include <cmath>
#include <cstddef>

#include "carve_plan.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace ls {
namespace fp {

using cp::finite64;

enum { FUSE_OUT = 0, FUSE_EMPTY, FUSE_OCCLUDED, FUSE_NEAR, FUSE_FREE, FUSE_SATURATED, FUSE_CLASSES };   // the class of a (voxel, view), by value
enum { VOL_VALID = 0, VOL_INSIDE, VOL_UNSEEN, VOL_FIELDS };                                             // counts[p] of the volume
constexpr int FUSE_CHUNK = 256;           // voxels per workgroup, one per thread, all of ONE problem
constexpr int FUSE_SCALE = 16384;         // t in [-1, 1] is kept as round(t * FUSE_SCALE)
constexpr int FUSE_MAX_OBS = 65535;       // n stops here, so |sum| <= 65535 * 16384 < 2^30
constexpr int FUSE_GRID_WORDS = 5;        // origin[3], voxel, trunc of one problem

// step 1, first half: x_a = origin_a + h * (double)index_a, one multiply and one add
LS_CP_HD double fuse_position(double origin, double h, int index) { return origin + h * (double)index; }

// step 1, second half: c = ((E[:,0] x0 + E[:,1] x1) + E[:,2] x2) + E[:,3], E [3,4] row-major (carve_camera with a float64 position)
LS_CP_HD void fuse_camera(const double* E, const double (&x)[3], double (&c)[3]) {
    for (int r = 0; r < 3; ++r) c[r] = ((E[r * 4 + 0] * x[0] + E[r * 4 + 1] * x[1]) + E[r * 4 + 2] * x[2]) + E[r * 4 + 3];
}

// steps 4 - 6: the pixel's depth against the voxel at depth z -> EMPTY, OCCLUDED, NEAR or FREE; *q = the quantised t of a NEAR or FREE
// voxel-view (an EMPTY one taken as free is FREE with q = FUSE_SCALE), else 0
LS_CP_HD int fuse_distance(float depth, double z, double trunc, bool empty_is_free, int* q) {
    *q = 0;
    const double d = (double)depth;
    if (!(d > 0.0)) {                                    // 0, negative and NaN
        if (!empty_is_free) return FUSE_EMPTY;
        *q = FUSE_SCALE;                                 // t = +1
        return FUSE_FREE;
    }
    const double s = d - z;                              // along the optical axis; +inf for an infinite depth, never NaN: z is finite
    if (s < -trunc) return FUSE_OCCLUDED;
    const double t = (s < trunc ? s : trunc) / trunc;
    *q = (int)floor(t * (double)FUSE_SCALE + 0.5);
    return s <= trunc ? FUSE_NEAR : FUSE_FREE;
}

// steps 1 - 6 for the voxel at x and one view: E [3,4], K [4], depth [H,W] of that view
LS_CP_HD int fuse_voxel_view(const double* E, const double* K, const double (&x)[3], const float* depth, int W, int H, double trunc, double znear,
                             bool empty_is_free, int* q) {
    double c[3];
    fuse_camera(E, x, c);
    int qx, qy;
    *q = 0;
    if (!cp::carve_pixel(c, K, W, H, znear, &qx, &qy)) return FUSE_OUT;
    return fuse_distance(depth[(size_t)qy * (size_t)W + (size_t)qx], c[2], trunc, empty_is_free, q);
}

// steps 7 and 8: the state of the voxel takes a NEAR or FREE voxel-view unless it is saturated -> the class that is counted
LS_CP_HD int fuse_update(int cls, int q, int* sum, int* n) {
    if (cls != FUSE_NEAR && cls != FUSE_FREE) return cls;
    if (*n == FUSE_MAX_OBS) return FUSE_SATURATED;
    *sum += q;
    *n += 1;
    return cls;
}

// state to volume: D = (double)sum / ((double)n * 16384.0) where n >= min_obs, else exactly +1.0
LS_CP_HD double fuse_value(int sum, int n, int min_obs, bool* valid) {
    *valid = n >= min_obs;
    return *valid ? (double)sum / ((double)n * (double)FUSE_SCALE) : 1.0;
}

LS_CP_HD long long fuse_chunks(long long voxels) { return (voxels + FUSE_CHUNK - 1) / FUSE_CHUNK; }

// the sizes a call accepts: P >= 1, dims >= 1 and P nx ny nz < 2^31 (int32 state indices)
LS_CP_HD bool fuse_sizes_ok(int P, int nx, int ny, int nz) {
    if (P < 1 || nx < 1 || ny < 1 || nz < 1) return false;
    const long long lim = 1ll << 31;
    const long long xy = (long long)nx * (long long)ny;              // < 2^62
    if (xy >= lim) return false;
    const long long vox = xy * (long long)nz;                        // < 2^62
    if (vox >= lim) return false;
    return vox * (long long)P < lim;
}

// the grid of one problem: origin finite, voxel and trunc finite and > 0 -> 0, or the number of the first refused field (1 origin, 2 voxel, 3 trunc)
LS_CP_HD int fuse_bad_grid(const double* origin, double voxel, double trunc) {
    if (!(finite64(origin[0]) && finite64(origin[1]) && finite64(origin[2]))) return 1;
    if (!(finite64(voxel) && voxel > 0.0)) return 2;
    if (!(finite64(trunc) && trunc > 0.0)) return 3;
    return 0;
}

// the scalars of a call: znear finite and > 0, empty_is_free 0 or 1 -> 0, or 1 / 2
LS_CP_HD int fuse_bad_scalar(double znear, int empty_is_free) {
    if (!(finite64(znear) && znear > 0.0)) return 1;
    if (empty_is_free != 0 && empty_is_free != 1) return 2;
    return 0;
}

// The one piece of the workspace, in 8-byte words: view_off [P+1] int64, then P grids of FUSE_GRID_WORDS float64.  A function of P alone:
// the state, the views and the counts are read and written where they lie.
struct FusePieces { size_t offs, grids; };
LS_CP_HD FusePieces fuse_pieces(int P) {
    FusePieces c;
    c.offs = (size_t)P + 1;
    c.grids = (size_t)P * FUSE_GRID_WORDS;
    return c;
}

}  // namespace fp
}  // namespace ls
