// tsdfray_plan.h -- the fused state of the scene memory (depthfuse.hip: sum, n) SEEN from a camera, the one statement of it: the ray of a
// pixel in grid units, the slab test against the grid, the bounded march, the sample at a depth, the state machine of a ray, the depth
// and the normal of a hit, the comparison of a predicted view with an observed one, what a call accepts and the pieces of the workspace.
// Pure functions: no HIP, no global state.  The kernel of tsdfray.hip is ray_cast with a fetch that reads global memory; a plain C++17
// compiler accepts the file, and tests/test_tsdf_ray_cpu.py replays it (tests/tools/tsdfray_plan_run.cpp) against the NumPy twin of the
// definition (tests/tsdf_ray_oracle.py; the definition itself: include/livingscenes_hip.h, ls_tsdf_raycast_f64 / ls_depth_compare_f32).
// The value at a point is tsdfsample_plan.h's, unchanged: sample_corner, sample_value and, through it, fp::fuse_value.  The ray parameter
// IS the camera depth: no square root on the marching path.  NO secant iteration (one linear interpolation between the two samples that
// bracket the crossing) and NO empty-space skipping (every sample of the march is taken).  Everything is float64 and no a * b + c is
// contracted into an fma: clang is told here, any other compiler by -ffp-contract=off.
#pragma once
#include <cmath>
#include <cstddef>

#include "tsdfsample_plan.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace ls {
namespace tr {

using cp::finite64;

enum { RAY_OUTSIDE = 0, RAY_FREE, RAY_UNSEEN, RAY_BEHIND, RAY_HIT, RAY_STATES };                 // the state of a pixel's ray, by value
enum { VIEW_NO_OBS = 0, VIEW_UNKNOWN, VIEW_AGREE, VIEW_IN_FRONT, VIEW_THROUGH, VIEW_CLASSES };   // the class of a compared pixel
constexpr int RAY_TILE = 16;              // a workgroup owns a RAY_TILE x RAY_TILE tile of ONE view, one thread per pixel
constexpr int RAY_WAVE_W = 8;             // each wave of 64 a compact RAY_WAVE_W x RAY_WAVE_H block of the tile
constexpr int RAY_WAVE_H = 8;
constexpr int RAY_GRID_WORDS = ts::SAMPLE_GRID_WORDS;   // origin[3], voxel, trunc, trunc / voxel of one problem
constexpr long long RAY_MAX_TRIPS = 1ll << 20;          // the samples a call lets one ray take: a larger (max dim - 1) / step is refused

// step 1: the ray of pixel (px, py) in grid units.  M [3,4] camera to memory frame (x right, y down, z forward), K = (fx, fy, cx, cy):
// u_a(z) = a_a + z * b_a is the grid coordinate at camera depth z.
LS_CP_HD void ray_setup(const double* M, const double* K, const double* origin, double h, int px, int py, double (&a)[3], double (&b)[3]) {
    const double rx = ((double)px - K[2]) / K[0], ry = ((double)py - K[3]) / K[1];
    for (int r = 0; r < 3; ++r) {
        a[r] = (M[r * 4 + 3] - origin[r]) / h;
        b[r] = ((M[r * 4 + 0] * rx + M[r * 4 + 1] * ry) + M[r * 4 + 2]) / h;
    }
}

// the most samples a ray can take on a grid: no axis advances more than `step` voxels per sample, so (max dim - 1) / step steps cross the
// grid; + 2 for the sample at z_in and one rounding.  ray_span never returns more.
LS_CP_HD long long ray_max_trips(const int (&dims)[3], double step) {
    int m = dims[0] > dims[1] ? dims[0] : dims[1];
    if (dims[2] > m) m = dims[2];
    return (long long)ceil((double)(m - 1) / step) + 2;
}

// steps 2 and 3: the slab test against [0, n_a - 1] on every axis and the march.  false = OUTSIDE: a value that is not finite, a
// dimension below 2, max |b_a| = 0, an axis with b_a = 0 whose a_a lies outside, or !(z_in <= z_out).  Else the samples are
// z_k = z_in + (double)k * dz, k = 0 .. *K, with dz = step / max |b_a| and *K = floor((z_out - z_in) / dz), at most ray_max_trips - 1
// (with a camera so far away that its quotients round to more than the grid's width, the march ends there; the samples are clamped to
// the grid in any case).
LS_CP_HD bool ray_span(const double (&a)[3], const double (&b)[3], const int (&dims)[3], double znear, double step, double* z_in, double* dz,
                       long long* K) {
    *z_in = znear, *dz = 0.0, *K = 0;
    if (dims[0] < 2 || dims[1] < 2 || dims[2] < 2) return false;
    double lo = znear, hi = INFINITY, bmax = 0.0;
    for (int r = 0; r < 3; ++r) {
        if (!(finite64(a[r]) && finite64(b[r]))) return false;
        const double far = (double)(dims[r] - 1);
        if (b[r] == 0.0) {
            if (!(a[r] >= 0.0 && a[r] <= far)) return false;
            continue;
        }
        const double q0 = (0.0 - a[r]) / b[r], q1 = (far - a[r]) / b[r];
        if (!(finite64(q0) && finite64(q1))) return false;
        const double mn = q0 < q1 ? q0 : q1, mx = q0 < q1 ? q1 : q0;
        if (mn > lo) lo = mn;
        if (mx < hi) hi = mx;
        const double ab = fabs(b[r]);
        if (ab > bmax) bmax = ab;
    }
    if (bmax == 0.0 || !(lo <= hi)) return false;
    const double d = step / bmax;
    const double q = (hi - lo) / d;
    if (!(finite64(d) && finite64(q))) return false;
    const double cap = (double)(ray_max_trips(dims, step) - 1);
    *z_in = lo, *dz = d;
    *K = (long long)floor(q < cap ? q : cap);
    return true;
}

// step 4, first half: the cell of the sample at depth z.  u_a = a_a + z * b_a clamped to [0, n_a - 1]; i_a = min((int)floor(u_a), n_a - 2),
// f_a = u_a - (double)i_a in [0, 1].  dims >= 2 (ray_span).
LS_CP_HD void ray_cell(const double (&a)[3], const double (&b)[3], double z, const int (&dims)[3], int (&i)[3], double (&f)[3]) {
    for (int r = 0; r < 3; ++r) {
        double u = a[r] + z * b[r];
        const double far = (double)(dims[r] - 1);
        u = !(u >= 0.0) ? 0.0 : (u > far ? far : u);
        int ir = (int)floor(u);
        if (ir > dims[r] - 2) ir = dims[r] - 2;
        i[r] = ir;
        f[r] = u - (double)ir;
    }
}

// step 6: the unit normal of a hit from the gradient at z*, (0, 0, 0) where the sample is not SAMPLED or the gradient vanishes
LS_CP_HD void ray_normal(int what, const double (&g)[3], float (&nrm)[3]) {
    const double gg = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
    nrm[0] = nrm[1] = nrm[2] = 0.0f;
    if (what != ts::SAMPLE_SAMPLED || !(gg > 0.0)) return;
    const double len = sqrt(gg);
    for (int r = 0; r < 3; ++r) nrm[r] = (float)(g[r] / len);
}

// steps 3 - 6 for one ray.  fetch(i, s, n) reads the (sum, n) of the eight corners of cell i (sample_corner's order); it is called only
// when the cell differs from the previous sample's, which cannot change a bit: the corners are the same numbers.  -> the state; a HIT
// writes *depth = (float) z* and the normal, every other state depth 0 and normal 0.
template <class Fetch>
LS_CP_HD int ray_cast(const double (&a)[3], const double (&b)[3], const int (&dims)[3], double znear, double step, int min_obs, double trunc,
                      double trunc_over_h, Fetch fetch, float* depth, float (&nrm)[3]) {
    *depth = 0.0f;
    nrm[0] = nrm[1] = nrm[2] = 0.0f;
    double z_in, dz;
    long long K;
    if (!ray_span(a, b, dims, znear, step, &z_in, &dz, &K)) return RAY_OUTSIDE;
    int s[8], n[8], at[3] = {-1, -1, -1}, i[3];
    double f[3], g[3], phi, phi_prev = 0.0;
    bool prev_sampled = false, all_sampled = true;
    int state = -1;
    double z_star = 0.0;
    for (long long k = 0; k <= K; ++k) {
        const double z = z_in + (double)k * dz;
        ray_cell(a, b, z, dims, i, f);
        if (i[0] != at[0] || i[1] != at[1] || i[2] != at[2]) {
            fetch(i, s, n);
            at[0] = i[0], at[1] = i[1], at[2] = i[2];
        }
        const bool sampled = ts::sample_value(s, n, min_obs, f, trunc, trunc_over_h, &phi, g) == ts::SAMPLE_SAMPLED;
        if (sampled && phi <= 0.0) {
            state = RAY_BEHIND;
            if (k > 0 && prev_sampled && phi_prev > 0.0) {
                state = RAY_HIT;
                z_star = (z_in + (double)(k - 1) * dz) + dz * (phi_prev / (phi_prev - phi));
            }
            break;
        }
        prev_sampled = sampled;
        phi_prev = phi;
        all_sampled = all_sampled && sampled;
    }
    if (state < 0) return all_sampled ? RAY_FREE : RAY_UNSEEN;
    if (state == RAY_BEHIND) return state;
    ray_cell(a, b, z_star, dims, i, f);
    if (i[0] != at[0] || i[1] != at[1] || i[2] != at[2]) fetch(i, s, n);
    const int what = ts::sample_value(s, n, min_obs, f, trunc, trunc_over_h, &phi, g);
    *depth = (float)z_star;
    ray_normal(what, g, nrm);
    return RAY_HIT;
}

// the view comparison of one pixel: comparisons only
LS_CP_HD int view_class(float d_obs, float d_pred, int ray_state, double tol) {
    if (!((double)d_obs > 0.0)) return VIEW_NO_OBS;          // 0, negative and NaN
    if (ray_state != RAY_HIT) return VIEW_UNKNOWN;
    const double s = (double)d_obs - (double)d_pred;         // +inf for an infinite observation
    if (s < -tol) return VIEW_IN_FRONT;
    if (s > tol) return VIEW_THROUGH;
    return VIEW_AGREE;                                       // both ends inclusive
}

// the scalars of a raycast: znear finite and > 0, 1/16 <= step <= 1 -> 0, or 1 / 2
LS_CP_HD int ray_bad_scalar(double znear, double step) {
    if (!(finite64(znear) && znear > 0.0)) return 1;
    if (!(step >= 0.0625 && step <= 1.0)) return 2;
    return 0;
}

LS_CP_HD long long ray_tiles(int H, int W) { return (long long)((H + RAY_TILE - 1) / RAY_TILE) * (long long)((W + RAY_TILE - 1) / RAY_TILE); }

// the pixel of thread t of the tile (tx, ty): wave t / 64 owns the 8 x 8 block (wave % 2, wave / 2) of the tile, its lanes row-major
LS_CP_HD void ray_pixel(int tx, int ty, int t, int* px, int* py) {
    const int wave = t / (RAY_WAVE_W * RAY_WAVE_H), lane = t % (RAY_WAVE_W * RAY_WAVE_H);
    *px = tx * RAY_TILE + (wave % (RAY_TILE / RAY_WAVE_W)) * RAY_WAVE_W + lane % RAY_WAVE_W;
    *py = ty * RAY_TILE + (wave / (RAY_TILE / RAY_WAVE_W)) * RAY_WAVE_H + lane / RAY_WAVE_W;
}

// The one piece of the workspace, in 8-byte words: view_off [P+1] int64, then P grids of RAY_GRID_WORDS float64 -- one upload.  A
// function of P alone: the state, the cameras and the outputs are read and written where they lie.
struct RayPieces { size_t offs, grids; };
LS_CP_HD RayPieces ray_pieces(int P) {
    RayPieces c;
    c.offs = (size_t)P + 1;
    c.grids = (size_t)P * RAY_GRID_WORDS;
    return c;
}

}  // namespace tr
}  // namespace ls
