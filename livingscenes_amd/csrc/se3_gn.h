// se3_gn.h -- the 6-DoF Gauss-Newton step the scene memory's registrations share (cloudnear.hip: ls_cloud_icp_plane_f32; tsdficp.hip:
// ls_tsdf_icp_f32): the fixed tree that adds a wave's float64 values, and the solve and retraction that turn the 28 summed moments
// (Q, sum J rho [6], sum J J^T [21, the upper triangle by rows]) into g_{k+1}.  Written once: both operators' poses come from this text.
// Every product and sum here is rounded: the including file sets `#pragma clang fp contract(off)` AHEAD of this include (it holds for
// the rest of the translation unit, so this header does not repeat it).
#pragma once
#include <cmath>

#include "ls_common.h"
#include "svd3.h"

namespace ls {
namespace gn {

// the sum of a wave in a fixed tree (lane l with l + 32, l + 16, ..., l + 1) -> lane 0
__device__ __forceinline__ double wave_tree_f64(double v) {
    for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_down(v, o, kWave);
    return v;
}

// The point-to-plane update from the 28 sums: M xi = b by Cholesky in float64 in a fixed order (column by column, every inner sum from
// k = 0 upwards), xi = (v, omega); Delta = exp(xi) by Rodrigues with the left Jacobian for the translation (first order below
// theta = 1e-6); R' = R_Delta R_k, t' = R_Delta t_k + t_Delta in float64; R' onto SO(3) by kabsch_rotation(R'^T), its polar factor;
// rounded to fp32.  false (g untouched) = a pivot that is not > 1e-12 times its original diagonal entry, or anything non-finite.
__device__ __forceinline__ bool plane_update(const double* sums, float* g) {
    double L[6][6], b[6], z[6], xi[6];
    {
        int e = 7;
        for (int r = 0; r < 6; ++r)
            for (int c = r; c < 6; ++c) L[c][r] = sums[e++];            // the lower triangle holds M, then L in place
        for (int r = 0; r < 6; ++r) b[r] = -sums[1 + r];
    }
    for (int j = 0; j < 6; ++j) {
        const double mjj = L[j][j];
        double d = mjj;
        for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
        if (!isfinite(d) || !(d > 1e-12 * mjj)) return false;
        const double l = sqrt(d);
        L[j][j] = l;
        for (int i = j + 1; i < 6; ++i) {
            double v = L[i][j];
            for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
            L[i][j] = v / l;
        }
    }
    for (int i = 0; i < 6; ++i) {
        double v = b[i];
        for (int k = 0; k < i; ++k) v -= L[i][k] * z[k];
        z[i] = v / L[i][i];
    }
    for (int i = 5; i >= 0; --i) {
        double v = z[i];
        for (int k = i + 1; k < 6; ++k) v -= L[k][i] * xi[k];
        xi[i] = v / L[i][i];
    }
    for (int i = 0; i < 6; ++i)
        if (!isfinite(xi[i])) return false;
    const double w0 = xi[3], w1 = xi[4], w2 = xi[5];
    const double th = sqrt((w0 * w0 + w1 * w1) + w2 * w2);
    const double K[3][3] = {{0.0, -w2, w1}, {w2, 0.0, -w0}, {-w1, w0, 0.0}};
    double ca = 1.0, cb = 0.5, cc = 0.0, cd = 0.0;                      // R_Delta = I + ca K + cd K^2, V = I + cb K + cc K^2
    if (!(th < 1e-6)) {
        ca = sin(th) / th;
        cb = cd = (1.0 - cos(th)) / (th * th);
        cc = (th - sin(th)) / (th * th * th);
    }
    double Rd[3][3], Vd[3][3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            const double kk = (K[r][0] * K[0][c] + K[r][1] * K[1][c]) + K[r][2] * K[2][c], id = r == c ? 1.0 : 0.0;
            Rd[r][c] = (id + ca * K[r][c]) + cd * kk;
            Vd[r][c] = (id + cb * K[r][c]) + cc * kk;
        }
    double H[9], t[3];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c)                                       // H = R'^T
            H[c * 3 + r] = (Rd[r][0] * (double)g[0 * 4 + c] + Rd[r][1] * (double)g[1 * 4 + c]) + Rd[r][2] * (double)g[2 * 4 + c];
        const double rt = (Rd[r][0] * (double)g[3] + Rd[r][1] * (double)g[7]) + Rd[r][2] * (double)g[11];
        const double td = (Vd[r][0] * xi[0] + Vd[r][1] * xi[1]) + Vd[r][2] * xi[2];
        t[r] = rt + td;
        if (!isfinite(t[r])) return false;
    }
    float R[9];
    if (kabsch_rotation(H, R) != LS_KABSCH_OK) return false;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) g[r * 4 + c] = R[r * 3 + c];
        g[r * 4 + 3] = (float)t[r];
    }
    return true;
}

}  // namespace gn
}  // namespace ls
