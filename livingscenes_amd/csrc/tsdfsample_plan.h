// tsdfsample_plan.h -- the fused state of the scene memory (depthfuse.hip: sum, n) READ at a point, the one statement of it: the grid
// coordinate of a posed query and the cell it falls in, the validity of the eight corners of that cell, the trilinear value of
// D = fuse_value(sum, n) in metres and the exact derivative of that interpolant, one Gauss-Newton record of the registration on the field,
// its cost, what a call accepts and the pieces of the workspace.  Pure functions: no HIP, no global state.  The kernels of tsdficp.hip are
// loops around sample_cell, sample_value and gn_record; a plain C++17 compiler accepts the file, and tests/test_tsdf_sample_cpu.py replays
// it (tests/tools/tsdf_sample_plan_run.cpp) against the NumPy twin of the definition (tests/tsdf_sample_oracle.py; the definition itself:
// include/livingscenes_hip.h, ls_tsdf_sample_f32 / ls_tsdf_icp_f32).  The posed query y is an INPUT here: it is formed in fp32 by the
// expression of ls_cloud_merge_f32, which cloud_grid.h states once (pose_row).  Everything below is float64 and no a * b + c is
// contracted into an fma: clang is told here, any other compiler by -ffp-contract=off.
#pragma once
#include <cmath>
#include <cstddef>

#include "fuse_plan.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace ls {
namespace ts {

using cp::finite64;

enum { SAMPLE_OUT = 0, SAMPLE_UNSEEN, SAMPLE_SAMPLED, SAMPLE_STATES };   // the state of a query, by value
enum { CNT_FINITE = 0, CNT_INSIDE, CNT_SAMPLED, CNT_FIELDS };            // counts[p]
constexpr int SAMPLE_CHUNK = 256;         // queries per workgroup, one per thread, all of ONE problem: the chunk of the float64 sums
constexpr int SAMPLE_WAVE = 64;           // the first tree of a chunk's sum runs over 64 consecutive queries
constexpr int SAMPLE_GRID_WORDS = 6;      // origin[3], voxel, trunc, trunc / voxel of one problem
constexpr int GN_MOMENTS = 28;            // phi^2, J phi [6], the upper triangle of J J^T by rows [21]: the record layout of the plane ICP

LS_CP_HD double sample_lerp(double a, double b, double f) { return a + f * (b - a); }

// step 2: the cell of the posed query y (fp32, widened here).  *finite = every component of y is finite.  false = OUT: a non-finite
// component, a dimension below 2 (no cell), or a grid coordinate u_a = (y_a - origin_a) / h outside [0, n_a - 1] (compared on the
// doubles: a NaN fails).  Else the base index i_a = min((int)floor(u_a), n_a - 2) -- the far face belongs to the last cell -- and
// f_a = u_a - (double)i_a in [0, 1].
LS_CP_HD bool sample_cell(const float (&y)[3], const double* origin, double h, const int (&dims)[3], int (&i)[3], double (&f)[3], bool* finite) {
    *finite = finite64((double)y[0]) && finite64((double)y[1]) && finite64((double)y[2]);
    if (!*finite || dims[0] < 2 || dims[1] < 2 || dims[2] < 2) return false;
    bool inside = true;
    for (int a = 0; a < 3; ++a) {
        const double u = ((double)y[a] - origin[a]) / h;
        const bool ok = u >= 0.0 && u <= (double)(dims[a] - 1);
        inside = inside && ok;
        int ia = ok ? (int)floor(u) : 0;
        if (ia > dims[a] - 2) ia = dims[a] - 2;
        i[a] = ia;
        f[a] = u - (double)ia;
    }
    return inside;
}

// where corner c = 4 alpha + 2 beta + gamma of the cell (i_0, i_1, i_2) lies in a [nx,ny,nz] volume, k fastest
LS_CP_HD long long sample_corner(const int (&dims)[3], const int (&i)[3], int c) {
    return ((long long)(i[0] + (c >> 2)) * dims[1] + (long long)(i[1] + ((c >> 1) & 1))) * dims[2] + (long long)(i[2] + (c & 1));
}

// steps 3 - 6 from the eight corners (s, n)[4 alpha + 2 beta + gamma]: UNSEEN if a corner has n < min_obs, else SAMPLED with
//   value     D along axis 2: a[2 alpha + beta] = lerp(D[.. 0], D[.. 1], f_2); along axis 1: b[alpha] = lerp(a[alpha 0], a[alpha 1], f_1);
//             along axis 0: v = lerp(b[0], b[1], f_0); phi = trunc * v
//   gradient  G_2 = lerp over axis 0 of (lerp over axis 1 of (D[alpha beta 1] - D[alpha beta 0]));
//             G_1 = lerp over axis 0 of (lerp over axis 2 of (D[alpha 1 gamma] - D[alpha 0 gamma]));
//             G_0 = lerp over axis 1 of (lerp over axis 2 of (D[1 beta gamma] - D[0 beta gamma])); grad_a = trunc_over_h * G_a
// -- the derivative of the interpolant above, which is affine in every f_a.  A query that is not SAMPLED gets phi = +trunc, grad = 0.
LS_CP_HD int sample_value(const int (&s)[8], const int (&n)[8], int min_obs, const double (&f)[3], double trunc, double trunc_over_h,
                          double* phi, double (&grad)[3]) {
    double D[8];
    bool all = true;
    for (int c = 0; c < 8; ++c) {
        bool valid;
        D[c] = fp::fuse_value(s[c], n[c], min_obs, &valid);
        all = all && valid;
    }
    *phi = trunc;
    grad[0] = grad[1] = grad[2] = 0.0;
    if (!all) return SAMPLE_UNSEEN;
    double a[4], d2[4], d1[4], d0[4];
    for (int ab = 0; ab < 4; ++ab) {
        a[ab] = sample_lerp(D[2 * ab], D[2 * ab + 1], f[2]);
        d2[ab] = D[2 * ab + 1] - D[2 * ab];
    }
    for (int al = 0; al < 2; ++al)
        for (int ga = 0; ga < 2; ++ga) d1[2 * al + ga] = D[4 * al + 2 + ga] - D[4 * al + ga];
    for (int bg = 0; bg < 4; ++bg) d0[bg] = D[4 + bg] - D[bg];
    const double b0 = sample_lerp(a[0], a[1], f[1]), b1 = sample_lerp(a[2], a[3], f[1]);
    *phi = trunc * sample_lerp(b0, b1, f[0]);
    const double G2 = sample_lerp(sample_lerp(d2[0], d2[1], f[1]), sample_lerp(d2[2], d2[3], f[1]), f[0]);
    const double G1 = sample_lerp(sample_lerp(d1[0], d1[1], f[2]), sample_lerp(d1[2], d1[3], f[2]), f[0]);
    const double G0 = sample_lerp(sample_lerp(d0[0], d0[1], f[2]), sample_lerp(d0[2], d0[3], f[2]), f[1]);
    grad[0] = trunc_over_h * G0;
    grad[1] = trunc_over_h * G1;
    grad[2] = trunc_over_h * G2;
    return SAMPLE_SAMPLED;
}

// What a SAMPLED query adds to the Gauss-Newton record of its chunk: rho = phi, J = (grad, y x grad) in the twist order (v, omega), y
// the posed query widened to float64; m = (rho^2, J rho [6], J J^T [21, the upper triangle by rows]).  The gradient is NOT normalised and
// nothing is weighted.  Any other query adds zeros.
LS_CP_HD void gn_record(bool sampled, double rho, const float (&y)[3], const double (&grad)[3], double (&m)[GN_MOMENTS]) {
    double yd[3], J[6];
    for (int r = 0; r < 3; ++r) yd[r] = sampled ? (double)y[r] : 0.0, J[r] = sampled ? grad[r] : 0.0;
    if (!sampled) rho = 0.0;
    J[3] = yd[1] * J[2] - yd[2] * J[1];
    J[4] = yd[2] * J[0] - yd[0] * J[2];
    J[5] = yd[0] * J[1] - yd[1] * J[0];
    m[0] = rho * rho;
    for (int r = 0; r < 6; ++r) m[1 + r] = J[r] * rho;
    int e = 7;
    for (int r = 0; r < 6; ++r)
        for (int c = r; c < 6; ++c) m[e++] = J[r] * J[c];
}

// the cost of an iteration: the truncated quadratic of ls_cloud_icp_f32 with trunc in the place of r
LS_CP_HD double icp_cost(long long f, long long w, double Q, double trunc) {
    return f > 0 ? (Q + (double)(f - w) * (trunc * trunc)) / (double)f : 0.0;
}

LS_CP_HD long long sample_chunks(long long b) { return (b + SAMPLE_CHUNK - 1) / SAMPLE_CHUNK; }

// The chunk rule, stated on an array: the record of the chunk whose `count` <= SAMPLE_CHUNK values are v[0 .. count) with stride `stride`
// (a missing query adds 0.0) -- a fixed tree over each 64 (l with l + 32, l + 16, ..., l + 1), then (w0 + w1) + (w2 + w3).  The kernels
// form the same tree with wave shuffles and four LDS words; a problem's sum is its records added in chunk order from 0.0.
LS_CP_HD double sample_chunk_record(const double* v, int count, int stride) {
    double w[SAMPLE_CHUNK];
    for (int l = 0; l < SAMPLE_CHUNK; ++l) w[l] = l < count ? v[(size_t)l * (size_t)stride] : 0.0;
    for (int k = 0; k < SAMPLE_CHUNK / SAMPLE_WAVE; ++k)
        for (int o = SAMPLE_WAVE / 2; o > 0; o >>= 1)
            for (int l = 0; l < o; ++l) w[k * SAMPLE_WAVE + l] += w[k * SAMPLE_WAVE + l + o];
    return (w[0] + w[SAMPLE_WAVE]) + (w[2 * SAMPLE_WAVE] + w[3 * SAMPLE_WAVE]);
}

// the grid of one problem beyond fuse_bad_grid: trunc / voxel, formed once on the host, must be finite -> it, or a NaN for a refused one
LS_CP_HD double sample_trunc_over_h(double voxel, double trunc) {
    const double r = trunc / voxel;
    return finite64(r) ? r : NAN;
}

// The pieces of the workspace.  words: b_off [P+1] and q_off [P+1] (the chunks of every problem) as int64, then P grids of
// SAMPLE_GRID_WORDS float64 -- one upload; per chunk of queries one float64 sum and three int counts; the ICP adds its pose and previous
// cost per problem and one record of GN_MOMENTS float64 per chunk.  sum_p ceil(b_p / c) <= floor(b / c) + P.
struct SamplePieces { size_t offs, grids, chunks, poses, costs, moments; };
LS_CP_HD SamplePieces sample_pieces(int P, long long b_total, bool icp) {
    SamplePieces c;
    c.offs = 2 * ((size_t)P + 1);
    c.grids = (size_t)P * SAMPLE_GRID_WORDS;
    c.chunks = (size_t)(b_total / SAMPLE_CHUNK) + (size_t)P;
    c.poses = icp ? (size_t)P * 12 : 0;
    c.costs = icp ? (size_t)P : 0;
    c.moments = icp ? c.chunks * GN_MOMENTS : 0;
    return c;
}

}  // namespace ts
}  // namespace ls
