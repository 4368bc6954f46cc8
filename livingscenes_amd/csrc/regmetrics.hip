// regmetrics.hip -- the four numbers the relocalisation evaluation keeps of a registration, for a ragged batch of P (reference cloud,
// rescan cloud, predicted pose, ground-truth pose) tuples in one call (ls_reg_metrics_batch):
//   rre_deg   rotation_error            lib_more/pose_estimation.py:157-180  180/pi acos(clamp((tr(R_pred^T R_gt) - 1) / 2, -1, 1)), unfolded
//   rte       translation_error         lib_more/pose_estimation.py:183-196  |t_pred - t_gt|
//   rmse      compute_transformation_error  lib_more/pose_estimation.py:214-233  end-point RMSE of pc1 under pred vs gt and of pc2 under the inverses
//   chamfer   chamfer_distance_torch    evaluate.py:111-123 on every chamfer_stride-th row (eval_3rscan.py:401: inst[:, ::10]), read in place
// Everything is float64 arithmetic on the fp32 inputs.  Pair p owns X[x_off[p] .. x_off[p+1]) and Y[y_off[p] .. y_off[p+1]) (host int64
// offsets, checked on the host and copied into the workspace on the stream, ls_ragged.h).
//
// The per-pair reduction rule: every sum is cut into chunks that depend on the pair alone -- EPE_CHUNK rows of one of its clouds for the
// end-point error, NN_CHUNK strided rows of one cloud (the queries of one direction) for the Chamfer distance.  One workgroup owns one chunk,
// adds it in a fixed order (a thread's rows in row order, then a fixed LDS tree) and writes ONE float64 partial; the last kernel adds a
// pair's partials in chunk order.  No floating-point atomics, so a pair's four values are the same bits alone, first, last or anywhere in
// a batch.  Workgroups find their pair by binary search (ls::owner) of the host-built chunk offsets.  Four launches, whatever P.
#include <climits>
#include <cmath>
#include <vector>

#include "ls_common.h"
#include "ls_ragged.h"

// two transforms of one point by bit-equal poses must give bit-equal results (pred == gt: rmse == 0 exactly): no contraction outside the
// nearest-neighbour loop, which opts in
#pragma clang fp contract(off)

namespace ls {
namespace rm {

constexpr int EPE_T = 256, EPE_ROWS = 4, EPE_CHUNK = EPE_T * EPE_ROWS;   // end-point error: rows per workgroup
constexpr int NN_T = 256, NN_CHUNK = NN_T;                                // Chamfer: queries per workgroup, one per thread
constexpr int NN_TILE = 512;                                              // candidates per LDS tile (12 KB)

// what the pose kernel leaves for the others, per pair (float64, row-major 3 x 4)
struct Pose {
    double pred[12], gt[12], pred_inv[12], gt_inv[12], pg[12];   // pg = pred o gt^-1
    double rre, rte;
    double pad[2];
};
static_assert(sizeof(Pose) == 512, "Pose");

// the device copy of the offsets: OFF_ARRAYS arrays of P + 1 int64 back to back
enum { OFF_X = 0, OFF_Y, OFF_EPE, OFF_NN, OFF_ARRAYS };

__host__ __device__ inline long long cdivll(long long a, long long b) { return (a + b - 1) / b; }

__device__ __forceinline__ void apply(const double* __restrict__ g, double x, double y, double z, double (&o)[3]) {
    for (int r = 0; r < 3; ++r) o[r] = ((g[r * 4 + 0] * x + g[r * 4 + 1] * y) + g[r * 4 + 2] * z) + g[r * 4 + 3];
}
// (R | t)^-1 = (R^T | -R^T t)
__device__ __forceinline__ void invert(const double* __restrict__ g, double* __restrict__ o) {
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) o[r * 4 + c] = g[c * 4 + r];
        o[r * 4 + 3] = -((g[0 * 4 + r] * g[3] + g[1 * 4 + r] * g[7]) + g[2 * 4 + r] * g[11]);
    }
}
// a o b = (Ra Rb | Ra tb + ta)
__device__ __forceinline__ void compose(const double* __restrict__ a, const double* __restrict__ b, double* __restrict__ o) {
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) o[r * 4 + c] = (a[r * 4 + 0] * b[0 * 4 + c] + a[r * 4 + 1] * b[1 * 4 + c]) + a[r * 4 + 2] * b[2 * 4 + c];
        o[r * 4 + 3] = ((a[r * 4 + 0] * b[3] + a[r * 4 + 1] * b[7]) + a[r * 4 + 2] * b[11]) + a[r * 4 + 3];
    }
}

// one thread per pair
__global__ __launch_bounds__(64) void pose_kernel(const float* __restrict__ pred, const float* __restrict__ gt, int P, Pose* __restrict__ poses) {
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= P) return;
    Pose q;
    for (int k = 0; k < 12; ++k) {
        q.pred[k] = (double)pred[(size_t)p * 12 + k];
        q.gt[k] = (double)gt[(size_t)p * 12 + k];
    }
    invert(q.pred, q.pred_inv);
    invert(q.gt, q.gt_inv);
    compose(q.pred, q.gt_inv, q.pg);
    double tr = 0.0;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) tr += q.pred[r * 4 + c] * q.gt[r * 4 + c];
    const double c = fmin(fmax((tr - 1.0) / 2.0, -1.0), 1.0);
    q.rre = 180.0 * acos(c) / 3.14159265358979323846;
    const double dx = q.pred[3] - q.gt[3], dy = q.pred[7] - q.gt[7], dz = q.pred[11] - q.gt[11];
    q.rte = sqrt((dx * dx + dy * dy) + dz * dz);
    q.pad[0] = q.pad[1] = 0.0;
    poses[p] = q;
}

// the sum of v over the T threads of the workgroup in a fixed tree order, valid in thread 0
template <int T>
__device__ __forceinline__ double block_sum(double v, double* __restrict__ lds) {
    lds[threadIdx.x] = v;
    __syncthreads();
    for (int o = T / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) lds[threadIdx.x] += lds[threadIdx.x + o];
        __syncthreads();
    }
    return lds[0];
}

// chunk c of pair p: c < ceil(n_p / EPE_CHUNK) is a chunk of X (|pred x - gt x|^2), the others are chunks of Y (|pred^-1 y - gt^-1 y|^2)
__global__ __launch_bounds__(EPE_T) void epe_kernel(const float* __restrict__ X, const float* __restrict__ Y, const long long* __restrict__ offs, int P,
                                                    const Pose* __restrict__ poses, double* __restrict__ part) {
    __shared__ double lds[EPE_T];
    __shared__ double g[24];
    const long long* epe_off = offs + (size_t)OFF_EPE * (P + 1);
    const int p = owner(epe_off, P, blockIdx.x);
    const long long x0 = offs[(size_t)OFF_X * (P + 1) + p], x1 = offs[(size_t)OFF_X * (P + 1) + p + 1];
    const long long y0 = offs[(size_t)OFF_Y * (P + 1) + p], y1 = offs[(size_t)OFF_Y * (P + 1) + p + 1];
    long long c = blockIdx.x - epe_off[p];
    const long long cx = cdivll(x1 - x0, EPE_CHUNK);
    const bool on_x = c < cx;
    if (!on_x) c -= cx;
    const float* __restrict__ pts = on_x ? X + x0 * 3 : Y + y0 * 3;
    const long long n = on_x ? x1 - x0 : y1 - y0;
    if (threadIdx.x < 24) {
        const Pose& q = poses[p];
        const int k = threadIdx.x % 12;
        g[threadIdx.x] = threadIdx.x < 12 ? (on_x ? q.pred[k] : q.pred_inv[k]) : (on_x ? q.gt[k] : q.gt_inv[k]);
    }
    __syncthreads();
    double s = 0.0;
    for (int k = 0; k < EPE_ROWS; ++k) {
        const long long i = c * EPE_CHUNK + (long long)k * EPE_T + threadIdx.x;
        if (i < n) {
            const double x = (double)pts[i * 3 + 0], y = (double)pts[i * 3 + 1], z = (double)pts[i * 3 + 2];
            double a[3], b[3];
            apply(g, x, y, z, a);
            apply(g + 12, x, y, z, b);
            const double ex = a[0] - b[0], ey = a[1] - b[1], ez = a[2] - b[2];
            s += (ex * ex + ey * ey) + ez * ez;
        }
    }
    const double total = block_sum<EPE_T>(s, lds);
    if (threadIdx.x == 0) part[blockIdx.x] = total;
}

// rows used of a cloud of n rows: 0, s, 2 s, ...
__host__ __device__ inline long long strided(long long n, int s) { return cdivll(n, s); }

// chunk c of pair p, with n' / m' the strided rows of X_p / Y_p:
//   c <  ceil(n' / NN_CHUNK): queries A_i = pred x'_i, candidates the rows y'_j                   (sum_i min_j |A_i - y'_j|^2)
//   the others:               queries y'_j,            candidates B_i = (pred o gt^-1) y'_i       (sum_j min_i |y'_j - B_i|^2)
// Either way the candidates are strided rows of Y_p, staged through LDS in tiles of NN_TILE and transformed as they are staged; a thread
// keeps its query and the running minimum in registers.
__global__ __launch_bounds__(NN_T) void nn_kernel(const float* __restrict__ X, const float* __restrict__ Y, const long long* __restrict__ offs, int P,
                                                  int stride, const Pose* __restrict__ poses, double* __restrict__ part) {
    __shared__ double cand[NN_TILE][3];
    __shared__ double lds[NN_T];
    __shared__ double g[12];
    const long long* nn_off = offs + (size_t)OFF_NN * (P + 1);
    const int p = owner(nn_off, P, blockIdx.x);
    const long long x0 = offs[(size_t)OFF_X * (P + 1) + p], x1 = offs[(size_t)OFF_X * (P + 1) + p + 1];
    const long long y0 = offs[(size_t)OFF_Y * (P + 1) + p], y1 = offs[(size_t)OFF_Y * (P + 1) + p + 1];
    const long long ns = strided(x1 - x0, stride), ms = strided(y1 - y0, stride);
    long long c = blockIdx.x - nn_off[p];
    const long long c1 = cdivll(ns, NN_CHUNK);
    const bool dir1 = c < c1;
    if (!dir1) c -= c1;
    if (threadIdx.x < 12) g[threadIdx.x] = dir1 ? poses[p].pred[threadIdx.x] : poses[p].pg[threadIdx.x];
    __syncthreads();
    const float* __restrict__ Yp = Y + y0 * 3;
    const long long nq = dir1 ? ns : ms;
    const long long qi = c * NN_CHUNK + threadIdx.x;
    const bool live = qi < nq;
    double q[3] = {0.0, 0.0, 0.0};
    if (live) {
        const float* __restrict__ r = (dir1 ? X + x0 * 3 : Yp) + qi * stride * 3;
        if (dir1) apply(g, (double)r[0], (double)r[1], (double)r[2], q);
        else { q[0] = (double)r[0]; q[1] = (double)r[1]; q[2] = (double)r[2]; }
    }
    double best = INFINITY;
    for (long long base = 0; base < ms; base += NN_TILE) {
        const int cnt = (int)(ms - base < NN_TILE ? ms - base : NN_TILE);
        for (int j = threadIdx.x; j < cnt; j += NN_T) {
            const float* __restrict__ r = Yp + (base + j) * stride * 3;
            double v[3] = {(double)r[0], (double)r[1], (double)r[2]};
            if (!dir1) apply(g, (double)r[0], (double)r[1], (double)r[2], v);
            cand[j][0] = v[0]; cand[j][1] = v[1]; cand[j][2] = v[2];
        }
        __syncthreads();
        {
#pragma clang fp contract(fast)
            for (int j = 0; j < cnt; ++j) {   // every lane reads the same LDS address: a broadcast, no bank conflict
                const double dx = q[0] - cand[j][0], dy = q[1] - cand[j][1], dz = q[2] - cand[j][2];
                const double d = dx * dx + dy * dy + dz * dz;
                best = d < best ? d : best;
            }
        }
        __syncthreads();
    }
    const double total = block_sum<NN_T>(live ? best : 0.0, lds);
    if (threadIdx.x == 0) part[blockIdx.x] = total;
}

// one thread per pair: its partials in chunk order -> out[p] = (rre_deg, rte, rmse, chamfer)
__global__ __launch_bounds__(64) void final_kernel(const long long* __restrict__ offs, int P, int stride, const Pose* __restrict__ poses,
                                                   const double* __restrict__ epe_part, const double* __restrict__ nn_part, double* __restrict__ out) {
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= P) return;
    const long long n = offs[(size_t)OFF_X * (P + 1) + p + 1] - offs[(size_t)OFF_X * (P + 1) + p];
    const long long m = offs[(size_t)OFF_Y * (P + 1) + p + 1] - offs[(size_t)OFF_Y * (P + 1) + p];
    const long long* epe_off = offs + (size_t)OFF_EPE * (P + 1);
    const long long* nn_off = offs + (size_t)OFF_NN * (P + 1);
    double se = 0.0;
    for (long long k = epe_off[p]; k < epe_off[p + 1]; ++k) se += epe_part[k];
    const long long ns = strided(n, stride), ms = strided(m, stride);
    const long long mid = nn_off[p] + cdivll(ns, NN_CHUNK);
    double s1 = 0.0, s2 = 0.0;
    for (long long k = nn_off[p]; k < mid; ++k) s1 += nn_part[k];
    for (long long k = mid; k < nn_off[p + 1]; ++k) s2 += nn_part[k];
    out[(size_t)p * 4 + 0] = poses[p].rre;
    out[(size_t)p * 4 + 1] = poses[p].rte;
    out[(size_t)p * 4 + 2] = sqrt(se / (3.0 * (double)(n + m)));
    out[(size_t)p * 4 + 3] = s1 / (double)ns + s2 / (double)ms;
}

}  // namespace rm
}  // namespace ls

using namespace ls;
using namespace ls::rm;

namespace {
// upper bounds of the chunk counts from the totals alone (sum_p ceil(r_p / c) <= floor(sum_p r_p / c) + P)
long long epe_chunks_max(int P, long long n_total, long long m_total) { return n_total / EPE_CHUNK + m_total / EPE_CHUNK + 2LL * P; }
long long nn_chunks_max(int P, long long n_total, long long m_total, int s) {
    return n_total / ((long long)NN_CHUNK * s) + m_total / ((long long)NN_CHUNK * s) + 2LL * P;
}
struct Ws {
    long long* offs;
    Pose* poses;
    double* epe_part;
    double* nn_part;
    size_t bytes;   // of the whole layout
};
Ws layout(void* ws, int P, long long n_total, long long m_total, int s) {   // ws null: a sizing pass
    Arena a(ws);
    Ws w;
    w.offs = a.take<long long>((size_t)OFF_ARRAYS * (P + 1));
    w.poses = a.take<Pose>((size_t)P);
    w.epe_part = a.take<double>((size_t)epe_chunks_max(P, n_total, m_total));
    w.nn_part = a.take<double>((size_t)nn_chunks_max(P, n_total, m_total, s));
    w.bytes = a.bytes();
    return w;
}
}  // namespace

extern "C" {

size_t ls_reg_metrics_batch_workspace_bytes(int P, long long n_total, long long m_total, int chamfer_stride) {
    if (P < 1 || n_total < 0 || m_total < 0 || chamfer_stride < 1) return 0;
    return layout(nullptr, P, n_total, m_total, chamfer_stride).bytes;
}

int ls_reg_metrics_batch(int P, const float* X, long long n_total, const long long* x_off, const float* Y, long long m_total, const long long* y_off,
                         const float* pred, const float* gt, int chamfer_stride, double* out, void* workspace, size_t workspace_bytes,
                         void* stream) {
    const char* op = "reg_metrics_batch";
    LS_REQUIRE(P >= 1, "%s: P must be at least 1, got %d", op, P);
    LS_REQUIRE(chamfer_stride >= 1, "%s: chamfer_stride must be at least 1, got %d", op, chamfer_stride);
    LS_REQUIRE(n_total >= 0 && m_total >= 0, "%s: negative total (n_total %lld, m_total %lld)", op, n_total, m_total);
    LS_REQUIRE(X && Y && pred && gt && out, "%s: null X / Y / pred / gt / out", op);
    int rc = check_ranges(op, "problem", "x_off", P, x_off, n_total, INT_MAX);
    if (rc != LS_OK) return rc;
    rc = check_ranges(op, "problem", "y_off", P, y_off, m_total, INT_MAX);
    if (rc != LS_OK) return rc;
    std::vector<long long> epe_off(P + 1, 0), nn_off(P + 1, 0);
    for (int p = 0; p < P; ++p) {
        const long long n = x_off[p + 1] - x_off[p], m = y_off[p + 1] - y_off[p];
        LS_REQUIRE(n > 0 && m > 0, "%s: problem %d: empty cloud (%lld and %lld rows)", op, p, n, m);
        epe_off[p + 1] = epe_off[p] + cdivll(n, EPE_CHUNK) + cdivll(m, EPE_CHUNK);
        nn_off[p + 1] = nn_off[p] + cdivll(strided(n, chamfer_stride), NN_CHUNK) + cdivll(strided(m, chamfer_stride), NN_CHUNK);
    }
    LS_REQUIRE(epe_off[P] <= INT_MAX && nn_off[P] <= INT_MAX, "%s: %lld + %lld workgroups, at most %d per launch", op, epe_off[P], nn_off[P], INT_MAX);
    const size_t need = ls_reg_metrics_batch_workspace_bytes(P, n_total, m_total, chamfer_stride);
    if (!workspace || workspace_bytes < need) {
        set_error("%s: workspace %zu < required %zu (ls_reg_metrics_batch_workspace_bytes(%d, %lld, %lld, %d))", op,
                  workspace ? workspace_bytes : (size_t)0, need, P, n_total, m_total, chamfer_stride);
        return LS_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const Ws w = layout(workspace, P, n_total, m_total, chamfer_stride);
    rc = upload_offsets(w.offs, pack_offsets(P, {x_off, y_off, epe_off.data(), nn_off.data()}), st);
    if (rc != LS_OK) return rc;
    const int pb = cdiv(P, 64);
    hipLaunchKernelGGL(pose_kernel, dim3(pb), dim3(64), 0, st, pred, gt, P, w.poses);
    hipLaunchKernelGGL(epe_kernel, dim3((unsigned)epe_off[P]), dim3(EPE_T), 0, st, X, Y, w.offs, P, w.poses, w.epe_part);
    hipLaunchKernelGGL(nn_kernel, dim3((unsigned)nn_off[P]), dim3(NN_T), 0, st, X, Y, w.offs, P, chamfer_stride, w.poses, w.nn_part);
    hipLaunchKernelGGL(final_kernel, dim3(pb), dim3(64), 0, st, w.offs, P, chamfer_stride, w.poses, w.epe_part, w.nn_part, out);
    LS_LAUNCH_CHECK();
    return LS_OK;
}

}  // extern "C"
