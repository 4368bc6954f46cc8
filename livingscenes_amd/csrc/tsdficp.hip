// tsdficp.hip -- scene memory: the fused state of an instance (depthfuse.hip: sum, n) READ at posed points, and a rescan REGISTERED onto
// it.  The definitions are in include/livingscenes_hip.h (ls_tsdf_sample_f32, ls_tsdf_icp_f32) and, as NumPy, in
// tests/tsdf_sample_oracle.py; the arithmetic of a query is tsdfsample_plan.h, which tests/tools/tsdf_sample_plan_run.cpp runs on the
// host; the posed query is cloud_grid.h's (pose_row, the expression of ls_cloud_merge_f32); the solve and the retraction of the
// registration are se3_gn.h's, shared with the point-to-plane ICP of cloudnear.hip.  What this file adds:
//   sample     a workgroup owns one chunk of SAMPLE_CHUNK consecutive queries of ONE problem, one thread per query: the problem's grid,
//              pose and trunc / h are indexed from blockIdx alone and stay in scalar registers.  A query inside the grid issues the 16
//              loads of its eight corners' (sum, n) before the first use, then value, gradient and state.  The chunk's counts come
//              from three ballots, its sum of phi^2 from a fixed tree inside each wave and a fixed tree over the four waves: one record
//              per chunk.  Queries arrive in no spatial order, so the corner gathers are scattered (not sorted here).
//   final      one workgroup per problem: the integer counts in any order, the chunk records in chunk order.
//   icp        per iteration the sample under g_k with, over the SAMPLED queries, the 28 float64 Gauss-Newton moments in registers and
//              through the same two trees; then one wave per problem adds the records in chunk order, applies the stop tests of
//              ls_cloud_icp_plane_f32 and solves for g_{k+1} (plane_update).  A stopped problem is frozen: its sample workgroups return
//              at once, so its phi / grad / state / chunk records ARE its last live sample's, the sample at g_out.
// Launches: a sample: the copy of the host arrays into the workspace and 2 kernels, whatever P; an ICP: the copy and 2 max_iter + 4
// kernels, whatever P and whenever problems stop.  No host synchronisation, no allocation, no floating-point atomics (no atomics at all);
// hipGetLastError() after every launch, the pass named.  The single entries are the batch of one problem.
#include <climits>
#include <cmath>
#include <vector>

#include "ls_common.h"
#include "ls_ragged.h"
#include "ls_workspace.h"

// the arithmetic of the definition as written: no contraction of a * b + c into an fma anywhere in this file
#pragma clang fp contract(off)
#include "cloud_grid.h"
#include "se3_gn.h"
#include "tsdfsample_plan.h"

namespace ls {
namespace tsk {
using namespace ts;

constexpr int ICP_RUNNING = -1;
static_assert(SAMPLE_CHUNK == 4 * kWave && SAMPLE_WAVE == kWave, "the chunk rule: four waves of 64");

struct SampleArgs {
    const int* sum;                // [P,nx,ny,nz]
    const int* n;                  // [P,nx,ny,nz]
    int dims[3];
    long long voxels;              // nx ny nz
    int min_obs, P;
    const float* B;                // [b_total,3]
    const long long* b_off;        // [P+1], in the workspace
    const long long* q_off;        // [P+1]: the chunks of every problem, in the workspace
    const double* grids;           // [P,6]: origin, voxel, trunc, trunc / voxel, in the workspace
    const float* g;                // [P,3,4] or null: the pose of the queries
    const int* stop;               // the ICP: [P], a problem that is not ICP_RUNNING is frozen; null: a plain sample
    double* phi;                   // [b_total]
    double* grad;                  // [b_total,3]
    unsigned char* state;          // [b_total]
    double* part;                  // per chunk: the sum of phi^2 over its SAMPLED queries
    int* part_cnt;                 // per chunk: CNT_FIELDS counts
    double* mom;                   // the ICP: per chunk GN_MOMENTS float64
};

// the sum of a chunk, one value per thread: the fixed tree inside each wave, then the fixed tree over the four waves -> thread 0.
// Every thread of the workgroup calls it.
__device__ __forceinline__ double chunk_tree(double (&wave_part)[SAMPLE_CHUNK / kWave], double v) {
    const double s = gn::wave_tree_f64(v);
    __syncthreads();                                                      // the previous use of wave_part has been read
    if ((threadIdx.x & (kWave - 1)) == 0) wave_part[threadIdx.x / kWave] = s;
    __syncthreads();
    return (wave_part[0] + wave_part[1]) + (wave_part[2] + wave_part[3]);
}

// workgroup = one chunk of queries of one problem under the problem's pose.  ICP: the problem's g_k, frozen once stopped, and the moments.
template <bool ICP>
__global__ __launch_bounds__(SAMPLE_CHUNK) void tsdf_sample_kernel(SampleArgs G) {
    __shared__ double wave_part[SAMPLE_CHUNK / kWave];
    __shared__ double wave_mom[GN_MOMENTS][SAMPLE_CHUNK / kWave];
    const int p = owner(G.q_off, G.P, (long long)blockIdx.x);
    if (ICP && G.stop[p] != ICP_RUNNING) return;                          // the whole workgroup: a stopped problem is frozen
    const long long b0 = G.b_off[p], b = G.b_off[p + 1] - b0;
    const long long qi = ((long long)blockIdx.x - G.q_off[p]) * SAMPLE_CHUNK + threadIdx.x;
    const bool live = qi < b;
    const double* grid = G.grids + (size_t)p * SAMPLE_GRID_WORDS;
    const double origin[3] = {grid[0], grid[1], grid[2]};
    const double h = grid[3], trunc = grid[4], toh = grid[5];
    const float* g = G.g ? G.g + (size_t)p * 12 : nullptr;
    float y[3] = {0.f, 0.f, 0.f};
    double phi = trunc, grad[3] = {0.0, 0.0, 0.0};
    int what = SAMPLE_OUT;
    bool finite = false;
    if (live) {
        const float* __restrict__ row = G.B + (b0 + qi) * 3;
        cloud::pose_row(g, row[0], row[1], row[2], y);
        int i[3];
        double f[3];
        if (sample_cell(y, origin, h, G.dims, i, f, &finite)) {
            const long long base = (long long)p * G.voxels;
            int s[8], n[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) {                                 // 16 loads in flight before the first use
                const long long at = base + sample_corner(G.dims, i, c);
                s[c] = G.sum[at];
                n[c] = G.n[at];
            }
            what = sample_value(s, n, G.min_obs, f, trunc, toh, &phi, grad);
        }
        G.phi[b0 + qi] = phi;
        for (int a = 0; a < 3; ++a) G.grad[(b0 + qi) * 3 + a] = grad[a];
        G.state[b0 + qi] = (unsigned char)what;
    }
    const bool sampled = what == SAMPLE_SAMPLED;
    const int n_finite = __syncthreads_count(finite), n_inside = __syncthreads_count(live && what != SAMPLE_OUT),
              n_sampled = __syncthreads_count(sampled);
    double m[GN_MOMENTS];
    if (ICP) gn_record(sampled, phi, y, grad, m);
    else m[0] = sampled ? phi * phi : 0.0;
    const double q = chunk_tree(wave_part, m[0]);
    if (threadIdx.x == 0) {
        G.part[blockIdx.x] = q;
        int* cnt = G.part_cnt + (size_t)blockIdx.x * CNT_FIELDS;
        cnt[CNT_FINITE] = n_finite, cnt[CNT_INSIDE] = n_inside, cnt[CNT_SAMPLED] = n_sampled;
    }
    if (ICP) {
        const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
#pragma unroll
        for (int e = 1; e < GN_MOMENTS; ++e) {
            const double v = gn::wave_tree_f64(m[e]);
            if (lane == 0) wave_mom[e][wave] = v;
        }
        __syncthreads();
        double* rec = G.mom + (size_t)blockIdx.x * GN_MOMENTS;
        if (threadIdx.x == 0) rec[0] = q;
        else if (threadIdx.x < GN_MOMENTS) {
            const double* v = wave_mom[threadIdx.x];
            rec[threadIdx.x] = (v[0] + v[1]) + (v[2] + v[3]);
        }
    }
}

// workgroup = one problem: counts (integers, any order) and sum_phi2 (the chunk records in chunk order)
__global__ __launch_bounds__(256) void tsdf_final_kernel(int P, const long long* __restrict__ q_off, const double* __restrict__ part,
                                                         const int* __restrict__ part_cnt, long long* __restrict__ counts,
                                                         double* __restrict__ sum_phi2) {
    __shared__ long long lds[CNT_FIELDS][256];
    const int p = blockIdx.x;
    const long long q0 = q_off[p], q1 = q_off[p + 1];
    long long v[CNT_FIELDS] = {0, 0, 0};
    for (long long q = q0 + threadIdx.x; q < q1; q += 256)
        for (int k = 0; k < CNT_FIELDS; ++k) v[k] += part_cnt[q * CNT_FIELDS + k];
    for (int k = 0; k < CNT_FIELDS; ++k) lds[k][threadIdx.x] = v[k];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o)
            for (int k = 0; k < CNT_FIELDS; ++k) lds[k][threadIdx.x] += lds[k][threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x < CNT_FIELDS) counts[(size_t)p * CNT_FIELDS + threadIdx.x] = lds[threadIdx.x][0];
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (long long q = q0; q < q1; ++q) s += part[q];
        sum_phi2[p] = s;
    }
}

// g_0 (null: the identity as a matrix), E_{-1} = 0, every problem running
__global__ __launch_bounds__(256) void tsdf_icp_init_kernel(int P, const float* __restrict__ g0, float* __restrict__ gk, double* __restrict__ e_prev,
                                                            int* __restrict__ stop, int* __restrict__ iters) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P * 12) return;
    gk[i] = g0 ? g0[i] : ((i % 12) % 5 == 0 ? 1.0f : 0.0f);
    if (i % 12 == 0) {
        e_prev[i / 12] = 0.0;
        stop[i / 12] = ICP_RUNNING;
        iters[i / 12] = 0;
    }
}

struct SolveArgs {
    int k, max_iter, min_matched;
    double rel_thr;
    const long long* q_off;
    const double* grids;
    const int* part_cnt;
    const double* mom;
    float* gk;
    double* e_prev;
    int* stop;
    int* iters;
    float* g_out;
    float* g_trace;                // [P, max_iter+1, 12] or null
    double* stat_trace;            // [P, max_iter+1, 3] = (f, w, Q) or null
};

// workgroup (one wave) = one problem that still runs, after the sample of iteration k: the chunk records added in chunk order (lane e the
// e-th moment, three lanes the counts), then one lane applies the stop tests of the definition or solves for g_{k+1}
__global__ __launch_bounds__(kWave) void tsdf_icp_solve_kernel(SolveArgs S) {
    static_assert(GN_MOMENTS + CNT_FIELDS <= kWave, "one lane per quantity");
    __shared__ double sums[GN_MOMENTS];
    __shared__ long long cnts[CNT_FIELDS];
    const int p = blockIdx.x;
    if (S.stop[p] != ICP_RUNNING) return;
    const long long q0 = S.q_off[p], q1 = S.q_off[p + 1];
    const int e = threadIdx.x;
    if (e < GN_MOMENTS) {
        double s = 0.0;
        for (long long q = q0; q < q1; ++q) s += S.mom[(size_t)q * GN_MOMENTS + e];
        sums[e] = s;
    } else if (e < GN_MOMENTS + CNT_FIELDS) {
        long long s = 0;
        for (long long q = q0; q < q1; ++q) s += S.part_cnt[q * CNT_FIELDS + (e - GN_MOMENTS)];
        cnts[e - GN_MOMENTS] = s;
    }
    __syncthreads();
    if (e != 0) return;
    float* g = S.gk + (size_t)p * 12;
    const long long f = cnts[CNT_FINITE], w = cnts[CNT_SAMPLED];
    const double Q = sums[0];
    const double E = icp_cost(f, w, Q, S.grids[(size_t)p * SAMPLE_GRID_WORDS + 4]);
    if (S.g_trace)
        for (int i = 0; i < 12; ++i) S.g_trace[((size_t)p * (S.max_iter + 1) + S.k) * 12 + i] = g[i];
    if (S.stat_trace) {
        double* st = S.stat_trace + ((size_t)p * (S.max_iter + 1) + S.k) * 3;
        st[0] = (double)f, st[1] = (double)w, st[2] = Q;
    }
    int why = ICP_RUNNING;
    float g_next[12];
    for (int i = 0; i < 12; ++i) g_next[i] = g[i];
    if (w < S.min_matched) why = LS_ICP_STARVED;
    else if (S.k >= 1 && S.e_prev[p] - E <= S.rel_thr * S.e_prev[p]) why = LS_ICP_CONVERGED;
    else if (S.k == S.max_iter) why = LS_ICP_MAX_ITER;
    else if (!gn::plane_update(sums, g_next)) why = LS_ICP_DEGENERATE;
    if (why != ICP_RUNNING) {
        S.stop[p] = why;
        S.iters[p] = S.k;
        for (int i = 0; i < 12; ++i) S.g_out[(size_t)p * 12 + i] = g[i];
        return;
    }
    for (int i = 0; i < 12; ++i) g[i] = g_next[i];
    S.e_prev[p] = E;
}

}  // namespace tsk
}  // namespace ls

using namespace ls;
using namespace ls::tsk;

namespace {
struct Ws {
    long long* words;     // b_off [P+1], q_off [P+1], then the grids [P,6] as float64
    size_t offs;          // the number of offset words
    double* part;
    int* part_cnt;
    float* gk;
    double* e_prev;
    double* mom;
    size_t bytes;
};

// the one layout: the pieces of tsdfsample_plan.h from one Arena (ws null: a sizing pass)
Ws layout(void* ws, int P, long long b_total, bool icp) {
    const SamplePieces c = sample_pieces(P, b_total, icp);
    Arena ar(ws);
    Ws w;
    w.words = ar.take<long long>(c.offs + c.grids);
    w.offs = c.offs;
    w.part = ar.take<double>(c.chunks);
    w.part_cnt = ar.take<int>(c.chunks * CNT_FIELDS);
    w.gk = ar.take<float>(c.poses);
    w.e_prev = ar.take<double>(c.costs);
    w.mom = ar.take<double>(c.moments);
    w.bytes = ar.bytes();
    return w;
}

size_t workspace_need(int P, int nx, int ny, int nz, long long b_total, bool icp) {
    if (!fp::fuse_sizes_ok(P, nx, ny, nz) || b_total < 0 || b_total > INT_MAX) return 0;
    return layout(nullptr, P, b_total, icp).bytes;
}

#define LS_TSDF_PASS(name)                                                                                   \
    do {                                                                                                     \
        hipError_t _e = hipGetLastError();                                                                   \
        if (_e != hipSuccess) {                                                                              \
            ls::set_error("%s: the %s pass failed to launch: %s (%s:%d)", op, name, hipGetErrorString(_e), __FILE__, __LINE__); \
            return LS_ERR_HIP;                                                                               \
        }                                                                                                    \
    } while (0)

struct IcpCall {
    const float* g0;
    int max_iter;
    double rel_thr;
    int min_matched;
    float* g_out;
    int* stop;
    int* iters;
    float* g_trace;
    double* stat_trace;
};

// everything the host decides, then the copy of the host arrays and the passes.  icp null: a sample under the pose g.
int run(const char* op, int P, const int32_t* sum, const int32_t* n, int nx, int ny, int nz, int min_obs, const double* origin, const double* voxel,
        const double* trunc, const float* B, long long b_total, const long long* b_off, const float* g, const IcpCall* icp, double* phi, double* grad,
        uint8_t* state, long long* counts, double* sum_phi2, void* workspace, size_t workspace_bytes, hipStream_t st) {
    LS_REQUIRE(P >= 1, "%s: P must be at least 1, got %d", op, P);
    LS_REQUIRE(nx >= 1 && ny >= 1 && nz >= 1, "%s: dims must be at least 1, got %d x %d x %d", op, nx, ny, nz);
    LS_REQUIRE(fp::fuse_sizes_ok(P, nx, ny, nz), "%s: P * nx * ny * nz = %d * %d * %d * %d reaches 2^31 (int32 state indices)", op, P, nx, ny, nz);
    LS_REQUIRE(min_obs >= 1, "%s: min_obs must be >= 1 (a sample never observed has no distance), got %d", op, min_obs);
    LS_REQUIRE(b_total >= 0, "%s: negative size (%lld query rows)", op, b_total);
    LS_REQUIRE(b_total <= INT_MAX, "%s: %lld query rows exceed %d (int row indices)", op, b_total, INT_MAX);
    LS_REQUIRE(sum && n, "%s: null sum / n", op);
    LS_REQUIRE(origin && voxel && trunc, "%s: null origin / voxel / trunc", op);
    LS_REQUIRE(b_total == 0 || (B && phi && grad && state), "%s: null B / phi / grad / state with %lld query rows", op, b_total);
    LS_REQUIRE(counts && sum_phi2, "%s: null counts / sum_phi2", op);
    int rc = check_ranges(op, "problem", "b_off", P, b_off, b_total, INT_MAX);
    if (rc != LS_OK) return rc;
    std::vector<long long> host(2 * ((size_t)P + 1) + (size_t)P * SAMPLE_GRID_WORDS);
    double* grids = (double*)(host.data() + 2 * ((size_t)P + 1));           // 8-byte words both
    long long chunks = 0;
    for (int p = 0; p < P; ++p) {
        const int bad = fp::fuse_bad_grid(origin + (size_t)p * 3, voxel[p], trunc[p]);
        LS_REQUIRE(bad != 1, "%s: problem %d: origin must be finite, got (%g, %g, %g)", op, p, origin[p * 3], origin[p * 3 + 1], origin[p * 3 + 2]);
        LS_REQUIRE(bad != 2, "%s: problem %d: voxel must be finite and > 0, got %g", op, p, voxel[p]);
        LS_REQUIRE(bad != 3, "%s: problem %d: trunc must be finite and > 0, got %g", op, p, trunc[p]);
        const double toh = sample_trunc_over_h(voxel[p], trunc[p]);
        LS_REQUIRE(toh == toh, "%s: problem %d: trunc / voxel overflows float64 (trunc %g, voxel %g)", op, p, trunc[p], voxel[p]);
        double* gr = grids + (size_t)p * SAMPLE_GRID_WORDS;
        for (int a = 0; a < 3; ++a) gr[a] = origin[(size_t)p * 3 + a];
        gr[3] = voxel[p], gr[4] = trunc[p], gr[5] = toh;
        host[p] = b_off[p];
        host[(size_t)P + 1 + p] = chunks;
        chunks += sample_chunks(b_off[p + 1] - b_off[p]);
    }
    host[P] = b_off[P];
    host[2 * (size_t)P + 1] = chunks;
    if (icp) {
        LS_REQUIRE(icp->max_iter >= 0, "%s: max_iter must be >= 0, got %d", op, icp->max_iter);
        LS_REQUIRE(icp->max_iter < INT_MAX, "%s: max_iter %d: max_iter + 1 samples do not fit an int", op, icp->max_iter);
        LS_REQUIRE(std::isfinite(icp->rel_thr) && icp->rel_thr >= 0.0, "%s: rel_thr must be finite and >= 0, got %g", op, icp->rel_thr);
        LS_REQUIRE(icp->min_matched >= 3, "%s: min_matched must be >= 3 (a rotation needs three correspondences), got %d", op, icp->min_matched);
        LS_REQUIRE(icp->g_out && icp->stop && icp->iters, "%s: null g_out / stop / iters", op);
    }
    const size_t need = workspace_need(P, nx, ny, nz, b_total, icp != nullptr);
    if (!(workspace && workspace_bytes >= need)) {
        set_error("%s: workspace %zu < required %zu (ls_%s_workspace_bytes)", op, workspace ? workspace_bytes : (size_t)0, need, op);
        return LS_ERR_WORKSPACE;
    }
    const Ws w = layout(workspace, P, b_total, icp != nullptr);
    rc = upload_offsets(w.words, host, st);
    if (rc != LS_OK) return rc;
    SampleArgs G{};
    G.sum = sum, G.n = n;
    G.dims[0] = nx, G.dims[1] = ny, G.dims[2] = nz;
    G.voxels = (long long)nx * ny * nz;
    G.min_obs = min_obs, G.P = P;
    G.B = B;
    G.b_off = w.words, G.q_off = w.words + P + 1;
    G.grids = (const double*)(w.words + w.offs);
    G.phi = phi, G.grad = grad, G.state = state;
    G.part = w.part, G.part_cnt = w.part_cnt;
    const dim3 threads(SAMPLE_CHUNK);
    if (!icp) {
        G.g = g;
        if (chunks > 0) {
            hipLaunchKernelGGL(tsdf_sample_kernel<false>, dim3((unsigned)chunks), threads, 0, st, G);
            LS_TSDF_PASS("sample");
        }
    } else {
        G.g = w.gk, G.stop = icp->stop, G.mom = w.mom;
        hipLaunchKernelGGL(tsdf_icp_init_kernel, dim3(cdiv((long long)P * 12, 256)), dim3(256), 0, st, P, icp->g0, w.gk, w.e_prev, icp->stop, icp->iters);
        LS_TSDF_PASS("init");
        SolveArgs S{0, icp->max_iter, icp->min_matched, icp->rel_thr, G.q_off, G.grids, w.part_cnt, w.mom, w.gk, w.e_prev, icp->stop, icp->iters,
                    icp->g_out, icp->g_trace, icp->stat_trace};
        for (int k = 0; k <= icp->max_iter; ++k) {
            if (chunks > 0) {
                hipLaunchKernelGGL(tsdf_sample_kernel<true>, dim3((unsigned)chunks), threads, 0, st, G);
                LS_TSDF_PASS("sample");
            }
            S.k = k;
            hipLaunchKernelGGL(tsdf_icp_solve_kernel, dim3(P), dim3(kWave), 0, st, S);
            LS_TSDF_PASS("solve");
        }
    }
    hipLaunchKernelGGL(tsdf_final_kernel, dim3(P), dim3(256), 0, st, P, G.q_off, w.part, w.part_cnt, counts, sum_phi2);
    LS_TSDF_PASS("final");
    return LS_OK;
}
}  // namespace

extern "C" {

size_t ls_tsdf_sample_workspace_bytes(int nx, int ny, int nz, long long b) { return workspace_need(1, nx, ny, nz, b, false); }
size_t ls_tsdf_sample_batch_workspace_bytes(int P, int nx, int ny, int nz, long long b_total) { return workspace_need(P, nx, ny, nz, b_total, false); }
size_t ls_tsdf_icp_workspace_bytes(int nx, int ny, int nz, long long b) { return workspace_need(1, nx, ny, nz, b, true); }
size_t ls_tsdf_icp_batch_workspace_bytes(int P, int nx, int ny, int nz, long long b_total) { return workspace_need(P, nx, ny, nz, b_total, true); }

int ls_tsdf_sample_f32(const int32_t* sum, const int32_t* n, int nx, int ny, int nz, int min_obs, const double* origin, double voxel, double trunc,
                       const float* B, long long b, const float* g, double* phi, double* grad, uint8_t* state, long long* counts, double* sum_phi2,
                       void* workspace, size_t workspace_bytes, void* stream) {
    const long long b_off[2] = {0, b};
    return run("tsdf_sample", 1, sum, n, nx, ny, nz, min_obs, origin, &voxel, &trunc, B, b, b_off, g, nullptr, phi, grad, state, counts, sum_phi2,
               workspace, workspace_bytes, (hipStream_t)stream);
}

int ls_tsdf_sample_batch_f32(int P, const int32_t* sum, const int32_t* n, int nx, int ny, int nz, int min_obs, const double* origin,
                             const double* voxel, const double* trunc, const float* B, long long b_total, const long long* b_off, const float* g,
                             double* phi, double* grad, uint8_t* state, long long* counts, double* sum_phi2, void* workspace, size_t workspace_bytes,
                             void* stream) {
    return run("tsdf_sample_batch", P, sum, n, nx, ny, nz, min_obs, origin, voxel, trunc, B, b_total, b_off, g, nullptr, phi, grad, state, counts,
               sum_phi2, workspace, workspace_bytes, (hipStream_t)stream);
}

int ls_tsdf_icp_f32(const int32_t* sum, const int32_t* n, int nx, int ny, int nz, int min_obs, const double* origin, double voxel, double trunc,
                    const float* B, long long b, const float* g0, int max_iter, double rel_thr, int min_matched, float* g_out, int32_t* stop,
                    int32_t* iters, double* phi, double* grad, uint8_t* state, long long* counts, double* sum_phi2, float* g_trace,
                    double* stat_trace, void* workspace, size_t workspace_bytes, void* stream) {
    const long long b_off[2] = {0, b};
    const IcpCall I{g0, max_iter, rel_thr, min_matched, g_out, stop, iters, g_trace, stat_trace};
    return run("tsdf_icp", 1, sum, n, nx, ny, nz, min_obs, origin, &voxel, &trunc, B, b, b_off, nullptr, &I, phi, grad, state, counts, sum_phi2,
               workspace, workspace_bytes, (hipStream_t)stream);
}

int ls_tsdf_icp_batch_f32(int P, const int32_t* sum, const int32_t* n, int nx, int ny, int nz, int min_obs, const double* origin, const double* voxel,
                          const double* trunc, const float* B, long long b_total, const long long* b_off, const float* g0, int max_iter,
                          double rel_thr, int min_matched, float* g_out, int32_t* stop, int32_t* iters, double* phi, double* grad, uint8_t* state,
                          long long* counts, double* sum_phi2, float* g_trace, double* stat_trace, void* workspace, size_t workspace_bytes,
                          void* stream) {
    const IcpCall I{g0, max_iter, rel_thr, min_matched, g_out, stop, iters, g_trace, stat_trace};
    return run("tsdf_icp_batch", P, sum, n, nx, ny, nz, min_obs, origin, voxel, trunc, B, b_total, b_off, nullptr, &I, phi, grad, state, counts,
               sum_phi2, workspace, workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"
