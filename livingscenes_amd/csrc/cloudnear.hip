// cloudnear.hip -- scene memory: fixed-radius nearest neighbour between the cloud an instance keeps (A, the targets) and a posed observation of
// it (B, the queries), with the overlap statistics of the pair.  The definition is in include/livingscenes_hip.h (ls_cloud_nearest_f32) and,
// as NumPy, in tests/nearest_oracle.py; the pose, the cell (of edge r, for targets and queries alike), the table and its claim walk are
// those of cloud_grid.h.  What this file adds:
//   distance    d2 = ((dx dx + dy dy) + dz dz), dx = y_0 - A[j][0] ..., every operation rounded to fp32; r2 = r r rounded on the host
//   neighbour   of query i: among the targets j whose cell differs from the query's by at most 1 on every axis and with d2 <= r2, the least
//               under (d2, j); a target without a cell is never a neighbour, a query without one has none
// Method: a table of 2 a_p slots per problem; the atomic count of a slot hands every target of its cell a rank.  Count -> scan (ls_scan.h)
// -> fill puts the members of every cell back to back as (x, y, z, index).  One thread per query then walks the 27 cells around its own
// -- each by a probe walk that ends at the cell or at an empty slot -- and keeps the minimum under (d2, j) in registers: which slot a
// cell got and the order of its members depend on the race, the minimum does not.  The sum of the distances follows the per-problem rule of
// regmetrics.hip: a workgroup owns one chunk of QUERY_CHUNK queries of ONE problem, adds it in a fixed LDS tree and writes one float64
// partial; the last kernel adds a problem's partials in chunk order.  Integer atomics only, and only on the table: a problem's outputs are
// the same bits alone, in any batch and in any run.
// Three more operators on the same grid, all extensions beyond the released reference like the search itself.  The trimmed ICP
// (ls_cloud_icp_f32; tests/icp_oracle.py): the grid is built once over the memory, then every iteration repeats the search under the
// current pose -- search_chunk is one __device__ function for both -- with the float64 moments of the matched pairs per chunk, and one
// workgroup per problem adds the chunk records in order, applies the stop tests and solves the 3x3 Kabsch problem (svd3.h).  A stopped
// problem is frozen: its workgroups exit at once, so the launches depend on max_iter alone and nothing waits on the host or on another
// workgroup.  The normals of the kept cloud (ls_cloud_normals_f32; tests/normals_oracle.py): one thread per target walks the 27 cells
// around its own and adds INTEGER moments of the neighbours' offsets, then the covariance and its eigenvectors in float64.  And the ICP
// loop with the point-to-plane metric (ls_cloud_icp_plane_f32; tests/plane_icp_oracle.py): the search and the solve kernel are templates
// on the metric, which says what a match adds to its chunk's record and how g_{k+1} follows from the sums.
// A fourth, the projection of the kept cloud onto its local planes (ls_cloud_project_f32; tests/project_oracle.py): the neighbourhood,
// the moments and the eigen-decomposition of the normals -- local_plane is one __device__ function for both -- then in float64 the
// distance of the row to the plane through the centroid of its neighbours and the row moved onto it, from the input positions; the sum
// of the squared distances by the chunk rule of the search, over chunks of the kept rows.
// An operator on this grid is a kernel templated on the problem locator (OneNear / RaggedNear), a launch function after grid_launch, and
// an entry that describes its call (NearCall) and hands the launch to near_run: every check, size and upload of the entry path is there.
#include <climits>
#include <cmath>
#include <vector>

#include "ls_common.h"
#include "ls_ragged.h"
#include "ls_scan.h"
#include "svd3.h"

// the arithmetic of the definition as written: no contraction of a * b + c into an fma anywhere in this file
#pragma clang fp contract(off)
#include "cloud_grid.h"
#include "se3_gn.h"

namespace ls {
namespace cnr {
using namespace cloud;
using gn::plane_update;      // the solve and the retraction of the plane metric, and the wave tree of its moments: se3_gn.h, shared with
using gn::wave_tree_f64;     // tsdficp.hip

constexpr int QUERY_CHUNK = 256;              // queries per workgroup, one per thread: the chunk of the float64 sum

// ------------------------------------------------------------------------------------------------ which problem: one, or one of a ragged batch
struct NearRef {
    const float* B;        // the problem's queries
    long long a, b;        // its targets and queries
    const float* g;        // [3,4] or null
    float inv, r2;
    long long a0, b0;      // global index of its first target / first query; its table: 2 a slots from slot 2 a0
    long long q0, q1;      // its chunks of queries
};

struct OneNear {
    const float* B;
    long long a, b;
    const float* g;
    float inv, r2;
    __device__ int target_owner(long long) const { return 0; }
    __device__ int chunk_owner(long long) const { return 0; }
    __device__ NearRef problem(int) const { return {B, a, b, g, inv, r2, 0, 0, 0, (b + QUERY_CHUNK - 1) / QUERY_CHUNK}; }
};

enum { OFF_A = 0, OFF_B, OFF_Q, OFF_ARRAYS };   // the device copy of a batch's offsets: rows of A, rows of B, chunks of queries

struct RaggedNear {
    const float* B;
    const float* g;            // [P,3,4] or null
    const long long* offs;
    const float* inv;          // [P]
    const float* r2;           // [P]
    int P;
    __device__ const long long* off(int k) const { return offs + (size_t)k * (P + 1); }
    __device__ int target_owner(long long i) const { return owner(off(OFF_A), P, i); }
    __device__ int chunk_owner(long long c) const { return owner(off(OFF_Q), P, c); }
    __device__ NearRef problem(int p) const {
        const long long *ao = off(OFF_A), *bo = off(OFF_B), *qo = off(OFF_Q);
        return {B + bo[p] * 3, ao[p + 1] - ao[p], bo[p + 1] - bo[p], g ? g + (size_t)p * 12 : nullptr, inv[p], r2[p], ao[p], bo[p], qo[p], qo[p + 1]};
    }
};

// tcell [a_total,3]: the targets' cells (NO_CELL in [0]: none)
template <class Near>
__global__ __launch_bounds__(256) void tcell_kernel(Near L, const float* __restrict__ A, long long a_total, int* __restrict__ tcell) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a_total) return;
    const NearRef C = L.problem(L.target_owner(i));
    const float y[3] = {A[i * 3 + 0], A[i * 3 + 1], A[i * 3 + 2]};
    int c[3];
    cell_of(y, C.inv, c);
    for (int k = 0; k < 3; ++k) tcell[i * 3 + k] = c[k];
}

// the table of a problem: slot s holds the GLOBAL index of the target that claimed it for its cell (-1: free) and never changes again, so all
// targets of a cell meet in one slot; cnt[s] counts them and hands each its rank.  A problem has at most a_p cells for 2 a_p slots.
template <class Near>
__global__ __launch_bounds__(256) void claim_kernel(Near L, long long a_total, const int* __restrict__ tcell, int* __restrict__ table,
                                                    int* __restrict__ cnt, unsigned* __restrict__ slot_of, int* __restrict__ rank,
                                                    int* __restrict__ status) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a_total) return;
    const int c0 = tcell[i * 3 + 0], c1 = tcell[i * 3 + 1], c2 = tcell[i * 3 + 2];
    if (c0 == NO_CELL) {
        slot_of[i] = NO_SLOT;
        return;
    }
    const int p = L.target_owner(i);
    const NearRef C = L.problem(p);
    int occupant;
    const unsigned found = claim_slot(table, 2 * C.a0, 2 * C.a, tcell, c0, c1, c2, (int)i, occupant);
    slot_of[i] = found;
    if (found == NO_SLOT) status[p] = LS_ERR_WORKSPACE;
    else rank[i] = atomicAdd(&cnt[found], 1);
}

// slots[s] = (cell of the slot, first member): what a query's probe step reads in one load ([0] == NO_CELL: the slot is empty)
__global__ __launch_bounds__(256) void slot_kernel(long long n_slots, const int* __restrict__ table, const int* __restrict__ tcell,
                                                   const int* __restrict__ start, int4* __restrict__ slots) {
    const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
    if (s >= n_slots) return;
    const int rep = table[s];
    int4 v = {NO_CELL, 0, 0, 0};
    if (rep >= 0) v = {tcell[(long long)rep * 3 + 0], tcell[(long long)rep * 3 + 1], tcell[(long long)rep * 3 + 2], start[s]};
    slots[s] = v;
}

// members: the targets of every cell back to back as (x, y, z, global index), the order inside a cell as the ranks fell
__global__ __launch_bounds__(256) void fill_kernel(const float* __restrict__ A, long long a_total, const unsigned* __restrict__ slot_of,
                                                   const int* __restrict__ rank, const int* __restrict__ start, float4* __restrict__ members) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a_total) return;
    const unsigned s = slot_of[i];
    if (s == NO_SLOT) return;
    members[(long long)start[s] + rank[i]] = make_float4(A[i * 3 + 0], A[i * 3 + 1], A[i * 3 + 2], __int_as_float((int)i));
}

// the 27 cells around c, each by a probe walk that ends at the cell or at an empty slot: visit(member) for every target in them, in an order
// that depends on the race.  Written once, for the search, for the ICP and for the normals.
template <class Visit>
__device__ __forceinline__ void walk_cells(const NearRef& C, const int (&c)[3], const int4* __restrict__ slots, const int* __restrict__ cnt,
                                           const float4* __restrict__ members, Visit&& visit) {
    const long long t0 = 2 * C.a0, T = 2 * C.a;
    for (int k = 0; k < 27; ++k) {
        const int n0 = c[0] + k / 9 - 1, n1 = c[1] + (k / 3) % 3 - 1, n2 = c[2] + k % 3 - 1;   // |c| <= 2^30: no overflow
        long long s = first_slot(n0, n1, n2, T);
        for (long long step = 0; step < T; ++step) {
            const int4 sl = slots[t0 + s];
            if (sl.x == NO_CELL) break;                        // an empty slot ends the walk: the cell has no target
            if (sl.x == n0 && sl.y == n1 && sl.z == n2) {
                const float4* __restrict__ m = members + sl.w;
                const int count = cnt[t0 + s];
                for (int e = 0; e < count; ++e) visit(m[e]);
                break;
            }
            if (++s == T) s = 0;
        }
    }
}

// the neighbour of the query y of cell c: the minimum under (d2, j) over the 27 cells, with the global index j (INT_MAX: none) and the
// neighbour's coordinates
__device__ __forceinline__ void nearest_in_cells(const NearRef& C, const float (&y)[3], const int (&c)[3], const int4* __restrict__ slots,
                                                 const int* __restrict__ cnt, const float4* __restrict__ members, float& best, int& best_j,
                                                 float (&best_a)[3]) {
    walk_cells(C, c, slots, cnt, members, [&](const float4 t) {
        const float dx = y[0] - t.x, dy = y[1] - t.y, dz = y[2] - t.z;
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        const int j = __float_as_int(t.w);
        if (d2 <= C.r2 && (d2 < best || (d2 == best && j < best_j))) {
            best = d2;
            best_j = j;
            best_a[0] = t.x, best_a[1] = t.y, best_a[2] = t.z;
        }
    });
}

// one thread's query of problem C under the pose g: finite?, the posed row y as the search forms it, and its neighbour
__device__ __forceinline__ bool query_one(const NearRef& C, const float* __restrict__ g, long long qi, const int4* __restrict__ slots,
                                          const int* __restrict__ cnt, const float4* __restrict__ members, float (&x)[3], float (&y)[3],
                                          float& best, int& best_j, float (&best_a)[3]) {
    const float* __restrict__ row = C.B + qi * 3;
    x[0] = row[0], x[1] = row[1], x[2] = row[2];
    pose_row(g, x[0], x[1], x[2], y);
    int c[3];
    const bool finite = cell_of(y, C.inv, c);
    if (finite && C.a > 0) nearest_in_cells(C, y, c, slots, cnt, members, best, best_j, best_a);
    return finite;
}

// the float64 sum of a chunk, one value per thread, in the fixed LDS tree of the definition -> every thread
__device__ __forceinline__ double chunk_sum(double (&lds)[QUERY_CHUNK], double v) {
    lds[threadIdx.x] = v;
    __syncthreads();
    for (int o = QUERY_CHUNK / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) lds[threadIdx.x] += lds[threadIdx.x + o];
        __syncthreads();
    }
    return lds[0];
}

// The search of the chunk blockIdx.x -- QUERY_CHUNK queries of the one problem C, one thread per query, under the pose g -- by the whole
// workgroup: nn_idx / nn_d2 of the query, part[chunk] = the float64 sum of the chunk's nn_d2 in a fixed order, part_cnt[chunk] = (finite
// queries, queries with a neighbour).  Written once for the search and for every iteration of the ICP: the last search of a problem IS
// its final search.  What it leaves in its thread: best_j, the global index of the neighbour (the caller sets INT_MAX: none), the query's
// row x, the posed row y as the search formed it and the neighbour's coordinates a, untouched where the thread has no query
// -> the thread has a neighbour.  The caller's plain locals by reference and the caller's LDS array, not a struct by value and an array
// of its own: measured, the struct cost the point ICP's search 4 us of 308 per launch on small problems (docs/history.md, section 35).
__device__ __forceinline__ bool search_chunk(const NearRef& C, const float* __restrict__ g, const int4* __restrict__ slots,
                                             const int* __restrict__ cnt, const float4* __restrict__ members, int* __restrict__ nn_idx,
                                             float* __restrict__ nn_d2, double* __restrict__ part, int2* __restrict__ part_cnt,
                                             double (&lds)[QUERY_CHUNK], int& best_j, float (&x)[3], float (&y)[3], float (&a)[3]) {
    const long long qi = ((long long)blockIdx.x - C.q0) * QUERY_CHUNK + threadIdx.x;
    const bool live = qi < C.b;
    bool finite = false;
    float best = INFINITY;
    if (live) finite = query_one(C, g, qi, slots, cnt, members, x, y, best, best_j, a);
    const bool has = best_j != INT_MAX;
    if (live) {
        nn_idx[C.b0 + qi] = has ? (int)(best_j - C.a0) : -1;
        nn_d2[C.b0 + qi] = best;
    }
    const int n_finite = __syncthreads_count(finite), n_has = __syncthreads_count(has);
    const double sum = chunk_sum(lds, has ? (double)best : 0.0);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = sum;
        part_cnt[blockIdx.x] = make_int2(n_finite, n_has);
    }
    return has;
}

// workgroup = one chunk of queries under the problem's own pose; hit[j] = target j is somebody's neighbour
template <class Near>
__global__ __launch_bounds__(QUERY_CHUNK) void query_kernel(Near L, const int4* __restrict__ slots, const int* __restrict__ cnt,
                                                            const float4* __restrict__ members, unsigned char* __restrict__ hit,
                                                            int* __restrict__ nn_idx, float* __restrict__ nn_d2, double* __restrict__ part,
                                                            int2* __restrict__ part_cnt) {
    const NearRef C = L.problem(L.chunk_owner(blockIdx.x));
    __shared__ double lds[QUERY_CHUNK];
    int best_j = INT_MAX;
    float x[3], y[3], a[3];
    if (search_chunk(C, C.g, slots, cnt, members, nn_idx, nn_d2, part, part_cnt, lds, best_j, x, y, a))
        hit[best_j] = 1;                                               // every writer writes the same byte
}

// the totals of K counters over the 256 threads of a workgroup, v[k] of every thread -> lds[k][0]
template <int K>
__device__ __forceinline__ void count_tree(long long (&lds)[K][256], const long long (&v)[K]) {
    for (int k = 0; k < K; ++k) lds[k][threadIdx.x] = v[k];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o)
            for (int k = 0; k < K; ++k) lds[k][threadIdx.x] += lds[k][threadIdx.x + o];
        __syncthreads();
    }
}

// workgroup = one problem: counts (the integer partials and the hit flags, any order) and sum_d2 (the float64 partials in chunk order)
template <class Near>
__global__ __launch_bounds__(256) void final_kernel(Near L, const unsigned char* __restrict__ hit, const double* __restrict__ part,
                                                    const int2* __restrict__ part_cnt, const int* __restrict__ status,
                                                    long long* __restrict__ counts, double* __restrict__ sum_d2, int* __restrict__ status_out) {
    __shared__ long long lds[3][256];
    const int p = blockIdx.x;
    const NearRef C = L.problem(p);
    long long v[3] = {0, 0, 0};
    for (long long q = C.q0 + threadIdx.x; q < C.q1; q += 256) {
        v[0] += part_cnt[q].x;
        v[1] += part_cnt[q].y;
    }
    for (long long j = threadIdx.x; j < C.a; j += 256) v[2] += hit[C.a0 + j];
    count_tree(lds, v);
    if (threadIdx.x < 3) counts[(size_t)p * 3 + threadIdx.x] = lds[threadIdx.x][0];
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (long long q = C.q0; q < C.q1; ++q) s += part[q];
        sum_d2[p] = s;
        if (status_out) status_out[p] = status[p];
    }
}

// ------------------------------------------------------------------------------------------------ normals of the kept cloud (ls_cloud_normals_f32)
constexpr float MOMENT_SCALE = 32768.0f;      // 2^15: dx / r in units of 2^-15, |q| <= 2^15, so a sum of q_a q_b over < 2^31 neighbours stays below 2^61

// The local plane of the row y of cell c, for the normals and for the projection: the walk of the search with the query y and no pose,
// the neighbours' offsets as integers q = rint((dx inv) 2^15), their first and second moments in int64 -- the order of a cell's members
// depends on the race, an integer sum does not -- the covariance in float64 from the integers, its eigenvalues by Jacobi (svd3.h) and
// the validity rule of the definition.  Ten accumulators in registers, no LDS.  m = the neighbours (the caller sets 0) and s1 their
// first moments; where the row is valid also lam, V and the places lo / mid / hi of the least, middle and largest eigenvalue -> valid
__device__ __forceinline__ bool local_plane(const NearRef& C, const int (&c)[3], const float (&y)[3], const int4* __restrict__ slots,
                                            const int* __restrict__ cnt, const float4* __restrict__ members, int min_nbrs, int& m,
                                            long long (&s1)[3], double (&lam)[3], double (&V)[3][3], int& lo, int& mid, int& hi) {
    long long s2[6] = {0, 0, 0, 0, 0, 0};
    walk_cells(C, c, slots, cnt, members, [&](const float4 t) {
        const float dx = y[0] - t.x, dy = y[1] - t.y, dz = y[2] - t.z;
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        if (d2 <= C.r2) {
            const long long q0 = (int)rintf((dx * C.inv) * MOMENT_SCALE), q1 = (int)rintf((dy * C.inv) * MOMENT_SCALE),
                            q2 = (int)rintf((dz * C.inv) * MOMENT_SCALE);
            ++m;
            s1[0] += q0, s1[1] += q1, s1[2] += q2;
            s2[0] += q0 * q0, s2[1] += q0 * q1, s2[2] += q0 * q2, s2[3] += q1 * q1, s2[4] += q1 * q2, s2[5] += q2 * q2;
        }
    });
    if (m < min_nbrs || m <= 0) return false;
    const double dm = (double)m, d1[3] = {(double)s1[0], (double)s1[1], (double)s1[2]};
    const double Cv[6] = {(double)s2[0] - (d1[0] * d1[0]) / dm, (double)s2[1] - (d1[0] * d1[1]) / dm, (double)s2[2] - (d1[0] * d1[2]) / dm,
                          (double)s2[3] - (d1[1] * d1[1]) / dm, (double)s2[4] - (d1[1] * d1[2]) / dm, (double)s2[5] - (d1[2] * d1[2]) / dm};
    sym_eig3(Cv, lam, V);
    lo = 0, hi = 0;
    for (int k = 1; k < 3; ++k) {
        if (lam[k] < lam[lo]) lo = k;
        if (lam[k] > lam[hi]) hi = k;
    }
    if (hi == lo) hi = (lo + 1) % 3;                                    // three equal eigenvalues
    mid = 3 - lo - hi;
    return lam[hi] > 0.0 && lam[mid] > 0x1p-40 * lam[hi];
}

// One thread per target i that has a cell: its local plane, then the unit eigenvector of the least eigenvalue rounded to fp32 under the
// sign rule of the definition, and the surface variation.
template <class Near>
__global__ __launch_bounds__(256) void normals_kernel(Near L, const float* __restrict__ A, long long a_total, const int* __restrict__ tcell,
                                                      const int4* __restrict__ slots, const int* __restrict__ cnt,
                                                      const float4* __restrict__ members, int min_nbrs, float* __restrict__ normals,
                                                      int* __restrict__ nbr_cnt, float* __restrict__ variation) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a_total) return;
    const int c[3] = {tcell[i * 3 + 0], tcell[i * 3 + 1], tcell[i * 3 + 2]};
    int m = 0;
    float nrm[3] = {0.f, 0.f, 0.f}, var = 0.f;
    if (c[0] != NO_CELL) {
        const NearRef C = L.problem(L.target_owner(i));
        const float y[3] = {A[i * 3 + 0], A[i * 3 + 1], A[i * 3 + 2]};
        long long s1[3] = {0, 0, 0};
        double lam[3], V[3][3];
        int lo, mid, hi;
        if (local_plane(C, c, y, slots, cnt, members, min_nbrs, m, s1, lam, V, lo, mid, hi)) {
            const double len = sqrt((V[0][lo] * V[0][lo] + V[1][lo] * V[1][lo]) + V[2][lo] * V[2][lo]);
            for (int k = 0; k < 3; ++k) nrm[k] = (float)(V[k][lo] / len);
            int big = 0;                                               // the first component of largest magnitude is positive
            for (int k = 1; k < 3; ++k)
                if (fabsf(nrm[k]) > fabsf(nrm[big])) big = k;
            const bool flip = nrm[big] < 0.f;
            for (int k = 0; k < 3; ++k) nrm[k] = nrm[k] == 0.f ? 0.f : (flip ? -nrm[k] : nrm[k]);
            var = (float)(lam[lo] / ((lam[lo] + lam[mid]) + lam[hi]));
        }
    }
    for (int k = 0; k < 3; ++k) normals[i * 3 + k] = nrm[k];
    nbr_cnt[i] = m;
    variation[i] = var;
}

// workgroup = one problem: counts [2] = (rows with a cell: they are their own neighbour, rows with a normal), any order -- integers
template <class Near>
__global__ __launch_bounds__(256) void normals_final_kernel(Near L, const float* __restrict__ normals, const int* __restrict__ nbr_cnt,
                                                            const int* __restrict__ status, long long* __restrict__ counts,
                                                            int* __restrict__ status_out) {
    __shared__ long long lds[2][256];
    const int p = blockIdx.x;
    const NearRef C = L.problem(p);
    long long v[2] = {0, 0};
    for (long long j = C.a0 + threadIdx.x; j < C.a0 + C.a; j += 256) {
        v[0] += nbr_cnt[j] > 0;
        v[1] += normals[j * 3 + 0] != 0.f || normals[j * 3 + 1] != 0.f || normals[j * 3 + 2] != 0.f;
    }
    count_tree(lds, v);
    if (threadIdx.x < 2) counts[(size_t)p * 2 + threadIdx.x] = lds[threadIdx.x][0];
    if (threadIdx.x == 0 && status_out) status_out[p] = status[p];
}

// ------------------------------------------------------------------------------------------------ projection onto the local planes (ls_cloud_project_f32)
enum { PROJ_NO_CELL = 0, PROJ_NO_PLANE, PROJ_HELD, PROJ_MOVED, PROJ_STATES };

// workgroup = one chunk of QUERY_CHUNK rows of ONE problem's kept cloud (the locator's queries ARE its targets: b = a, b0 = a0), one
// thread per row: its local plane as the normals form it, then in float64 the unit normal before any fp32 rounding, the row minus the
// centroid of its neighbourhood from the integer moments, and s, its signed distance to the plane through the centroid.  Every row is
// projected from the INPUT positions and written to out_pts (a Jacobi step).  part[chunk] = the sum of s^2 over the chunk's moved rows.
template <class Near>
__global__ __launch_bounds__(QUERY_CHUNK) void project_kernel(Near L, const float* __restrict__ A, const int* __restrict__ tcell,
                                                              const int4* __restrict__ slots, const int* __restrict__ cnt,
                                                              const float4* __restrict__ members, int min_nbrs, double max_variation,
                                                              double max_shift, float* __restrict__ out_pts, int* __restrict__ state,
                                                              float* __restrict__ shift, double* __restrict__ part) {
    __shared__ double lds[QUERY_CHUNK];
    const NearRef C = L.problem(L.chunk_owner(blockIdx.x));
    const long long qi = ((long long)blockIdx.x - C.q0) * QUERY_CHUNK + threadIdx.x;
    double moved2 = 0.0;
    if (qi < C.a) {
        const long long i = C.a0 + qi;
        const int c[3] = {tcell[i * 3 + 0], tcell[i * 3 + 1], tcell[i * 3 + 2]};
        const float y[3] = {A[i * 3 + 0], A[i * 3 + 1], A[i * 3 + 2]};
        float out[3] = {y[0], y[1], y[2]}, sh = 0.f;
        int what = PROJ_NO_CELL;
        if (c[0] != NO_CELL) {
            int m = 0, lo, mid, hi;
            long long s1[3] = {0, 0, 0};
            double lam[3], V[3][3];
            what = PROJ_NO_PLANE;
            if (local_plane(C, c, y, slots, cnt, members, min_nbrs, m, s1, lam, V, lo, mid, hi)) {
                const double len = sqrt((V[0][lo] * V[0][lo] + V[1][lo] * V[1][lo]) + V[2][lo] * V[2][lo]);
                const double n[3] = {V[0][lo] / len, V[1][lo] / len, V[2][lo] / len};
                const double unit = 1.0 / ((double)C.inv * (double)MOMENT_SCALE), dm = (double)m;
                const double d[3] = {((double)s1[0] / dm) * unit, ((double)s1[1] / dm) * unit, ((double)s1[2] / dm) * unit};
                const double s = (d[0] * n[0] + d[1] * n[1]) + d[2] * n[2];
                const double var = lam[lo] / ((lam[lo] + lam[mid]) + lam[hi]);
                sh = (float)fabs(s);
                what = (var > max_variation || fabs(s) > max_shift) ? PROJ_HELD : PROJ_MOVED;
                if (what == PROJ_MOVED) {
                    for (int k = 0; k < 3; ++k) out[k] = (float)((double)y[k] - s * n[k]);
                    moved2 = s * s;
                }
            }
        }
        for (int k = 0; k < 3; ++k) out_pts[i * 3 + k] = out[k];
        state[i] = what;
        shift[i] = sh;
    }
    const double sum = chunk_sum(lds, moved2);
    if (threadIdx.x == 0) part[blockIdx.x] = sum;
}

// workgroup = one problem: counts [4] = the rows per state (integers, any order) and sum_shift2 (the float64 partials in chunk order)
template <class Near>
__global__ __launch_bounds__(256) void project_final_kernel(Near L, const int* __restrict__ state, const double* __restrict__ part,
                                                            const int* __restrict__ status, long long* __restrict__ counts,
                                                            double* __restrict__ sum_shift2, int* __restrict__ status_out) {
    __shared__ long long lds[PROJ_STATES][256];
    const int p = blockIdx.x;
    const NearRef C = L.problem(p);
    long long v[PROJ_STATES] = {0, 0, 0, 0};
    for (long long j = C.a0 + threadIdx.x; j < C.a0 + C.a; j += 256)
        for (int k = 0; k < PROJ_STATES; ++k) v[k] += state[j] == k;
    count_tree(lds, v);
    if (threadIdx.x < PROJ_STATES) counts[(size_t)p * PROJ_STATES + threadIdx.x] = lds[threadIdx.x][0];
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (long long q = C.q0; q < C.q1; ++q) s += part[q];
        sum_shift2[p] = s;
        if (status_out) status_out[p] = status[p];
    }
}

// ------------------------------------------------------------------------------------------------ trimmed ICP on the same grid (ls_cloud_icp_f32)
// The state of a problem between two launches: its pose g_k and E_{k-1} in the workspace, stop[p] (ICP_RUNNING until a stop test holds) and
// iters[p] in the caller's arrays.  A launch of iteration k touches the problems that still run and no other.
constexpr int ICP_RUNNING = -1;
// The two metrics of the loop.  A metric says what a matched query adds to the record of float64 moments of its chunk, and how g_{k+1}
// follows from the sums; the search, the chunk rule, the stop tests and the freezing are written once for both.
struct PointMetric {                          // ls_cloud_icp_f32: sum x [3], sum a [3], sum x a^T [9] -> Kabsch
    static constexpr bool PLANE = false;
    static constexpr int N_MOM = 15, N_STAT = 3;
};
struct PlaneMetric {                          // ls_cloud_icp_plane_f32: Q = sum rho^2, sum J rho [6], sum J J^T [21, the upper triangle by rows] -> Cholesky
    static constexpr bool PLANE = true;
    static constexpr int N_MOM = 28, N_STAT = 5;
};

__global__ __launch_bounds__(256) void icp_init_kernel(int P, const float* __restrict__ g0, float* __restrict__ gk, double* __restrict__ e_prev,
                                                       int* __restrict__ stop, int* __restrict__ iters) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P * 12) return;
    gk[i] = g0 ? g0[i] : ((i % 12) % 5 == 0 ? 1.0f : 0.0f);           // NULL: the identity as a matrix
    if (i % 12 == 0) {
        e_prev[i / 12] = 0.0;
        stop[i / 12] = ICP_RUNNING;
        iters[i / 12] = 0;
    }
}

// what a planar match adds: y the posed row as the search formed it, a its neighbour, n the neighbour's normal, all as float64; every
// product of two of them is exact in float64 (24 x 24 bits), the sums and the products with rho are rounded once each
__device__ __forceinline__ void plane_moments(bool planar, const float (&y)[3], const float (&a)[3], const float (&n)[3],
                                              double (&m)[PlaneMetric::N_MOM]) {
    double yd[3], ad[3], J[6];
    for (int r = 0; r < 3; ++r) yd[r] = planar ? (double)y[r] : 0.0, ad[r] = planar ? (double)a[r] : 0.0, J[r] = planar ? (double)n[r] : 0.0;
    const double rho = ((yd[0] - ad[0]) * J[0] + (yd[1] - ad[1]) * J[1]) + (yd[2] - ad[2]) * J[2];
    J[3] = yd[1] * J[2] - yd[2] * J[1];
    J[4] = yd[2] * J[0] - yd[0] * J[2];
    J[5] = yd[0] * J[1] - yd[1] * J[0];
    m[0] = rho * rho;
    for (int r = 0; r < 6; ++r) m[1 + r] = J[r] * rho;
    int e = 7;
    for (int r = 0; r < 6; ++r)
        for (int c = r; c < 6; ++c) m[e++] = J[r] * J[c];
}

// The search of iteration k: search_chunk under g_k, for the chunks of the problems that still run, and one record of N_MOM float64
// moments per chunk over the matched queries.  Point metric: the ORIGINAL row x of B and its neighbour a, products formed in float64 (exact:
// 24 x 24 bits).  Plane metric: a matched query gathers the normal row of its neighbour from N (packed like A); the match is planar iff
// that row is not zero, part_w[chunk] counts them.  The moments go through a fixed tree inside every wave and a fixed tree over the four
// waves: under 1 KB of LDS instead of 30 KB and more.
template <class Near, class Metric>
__global__ __launch_bounds__(QUERY_CHUNK) void icp_search_kernel(Near L, const int* __restrict__ stop, const float* __restrict__ gk,
                                                                 const int4* __restrict__ slots, const int* __restrict__ cnt,
                                                                 const float4* __restrict__ members, const float* __restrict__ N,
                                                                 int* __restrict__ nn_idx, float* __restrict__ nn_d2,
                                                                 double* __restrict__ part, int2* __restrict__ part_cnt,
                                                                 int* __restrict__ part_w, double* __restrict__ mom) {
    constexpr int N_MOM = Metric::N_MOM;
    __shared__ double lds[QUERY_CHUNK];
    __shared__ double wave_part[N_MOM][QUERY_CHUNK / kWave];
    const int p = L.chunk_owner(blockIdx.x);
    if (stop[p] != ICP_RUNNING) return;                                // the whole workgroup: a stopped problem is frozen
    const NearRef C = L.problem(p);
    int best_j = INT_MAX;
    float x[3] = {0.f, 0.f, 0.f}, y[3] = {0.f, 0.f, 0.f}, a[3] = {0.f, 0.f, 0.f};
    const bool has = search_chunk(C, gk + (size_t)p * 12, slots, cnt, members, nn_idx, nn_d2, part, part_cnt, lds, best_j, x, y, a);
    double m[N_MOM];
    if constexpr (Metric::PLANE) {
        float n[3] = {0.f, 0.f, 0.f};
        if (has)
            for (int r = 0; r < 3; ++r) n[r] = N[(long long)best_j * 3 + r];
        const bool planar = has && (n[0] != 0.f || n[1] != 0.f || n[2] != 0.f);
        const int n_planar = __syncthreads_count(planar);
        if (threadIdx.x == 0) part_w[blockIdx.x] = n_planar;
        plane_moments(planar, y, a, n, m);
    } else {
        for (int r = 0; r < 3; ++r) {
            m[r] = has ? (double)x[r] : 0.0;
            m[3 + r] = has ? (double)a[r] : 0.0;
        }
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) m[6 + r * 3 + c] = m[r] * m[3 + c];
    }
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    for (int e = 0; e < N_MOM; ++e) {
        const double v = wave_tree_f64(m[e]);
        if (lane == 0) wave_part[e][wave] = v;
    }
    __syncthreads();
    if (threadIdx.x < N_MOM) {
        const double* v = wave_part[threadIdx.x];
        mom[(size_t)blockIdx.x * N_MOM + threadIdx.x] = (v[0] + v[1]) + (v[2] + v[3]);
    }
}

// the Kabsch update of the point metric from the 15 sums over n matches: false = the solver reports anything but LS_KABSCH_OK
__device__ __forceinline__ bool point_update(const double* sums, long long n, float* g) {
    const double dn = (double)n;
    double H[9], mx[3], ma[3];
    float R[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) H[r * 3 + c] = sums[6 + r * 3 + c] - (sums[r] * sums[3 + c]) / dn;
    for (int r = 0; r < 3; ++r) mx[r] = sums[r] / dn, ma[r] = sums[3 + r] / dn;
    if (kabsch_rotation(H, R) != LS_KABSCH_OK) return false;
    for (int r = 0; r < 3; ++r) {
        const double Rm = ((double)R[r * 3 + 0] * mx[0] + (double)R[r * 3 + 1] * mx[1]) + (double)R[r * 3 + 2] * mx[2];
        for (int c = 0; c < 3; ++c) g[r * 4 + c] = R[r * 3 + c];
        g[r * 4 + 3] = (float)(ma[r] - Rm);
    }
    return true;
}

// workgroup (one wave) = one problem that still runs, after the search of iteration k: the chunk records added in chunk order (lane e the
// e-th float64 quantity, three lanes the counts), then one lane applies the stop tests of the definition or solves for g_{k+1}.  The plane
// metric counts w, the planar matches, where the point metric counts n, and its cost takes Q = sum rho^2 where that takes S.
template <class Near, class Metric>
__global__ __launch_bounds__(kWave) void icp_solve_kernel(Near L, int k, int max_iter, double rel_thr, int min_matched,
                                                          const double* __restrict__ part, const int2* __restrict__ part_cnt,
                                                          const int* __restrict__ part_w, const double* __restrict__ mom,
                                                          float* __restrict__ gk, double* __restrict__ e_prev, int* __restrict__ stop,
                                                          int* __restrict__ iters, float* __restrict__ g_out, long long* __restrict__ planar,
                                                          double* __restrict__ sum_rho2, float* __restrict__ g_trace,
                                                          double* __restrict__ stat_trace) {
    constexpr int N_MOM = Metric::N_MOM, N_STAT = Metric::N_STAT;
    static_assert(N_MOM + 4 <= kWave, "one lane per quantity");
    __shared__ double sums[N_MOM + 1];
    __shared__ long long cnts[3];
    const int p = blockIdx.x;
    if (stop[p] != ICP_RUNNING) return;
    const NearRef C = L.problem(p);
    const int e = threadIdx.x;
    if (e < N_MOM) {
        double s = 0.0;
        for (long long q = C.q0; q < C.q1; ++q) s += mom[(size_t)q * N_MOM + e];
        sums[e] = s;
    } else if (e == N_MOM) {
        double s = 0.0;
        for (long long q = C.q0; q < C.q1; ++q) s += part[q];         // the sum_d2 of final_kernel
        sums[N_MOM] = s;
    } else if (e < N_MOM + 3) {
        long long s = 0;
        for (long long q = C.q0; q < C.q1; ++q) s += e == N_MOM + 1 ? part_cnt[q].x : part_cnt[q].y;
        cnts[e - N_MOM - 1] = s;
    } else if (e == N_MOM + 3) {
        long long s = 0;
        if constexpr (Metric::PLANE)
            for (long long q = C.q0; q < C.q1; ++q) s += part_w[q];
        cnts[2] = s;
    }
    __syncthreads();
    if (e != 0) return;
    float* g = gk + (size_t)p * 12;
    const long long f = cnts[0], n = cnts[1], w = Metric::PLANE ? cnts[2] : n;
    const double S = sums[N_MOM], Q = Metric::PLANE ? sums[0] : S;
    const double E = f > 0 ? (Q + (double)(f - w) * (double)C.r2) / (double)f : 0.0;
    if (g_trace)
        for (int i = 0; i < 12; ++i) g_trace[((size_t)p * (max_iter + 1) + k) * 12 + i] = g[i];
    if (stat_trace) {
        double* st = stat_trace + ((size_t)p * (max_iter + 1) + k) * N_STAT;
        st[0] = (double)f, st[1] = (double)n, st[2] = S;
        if constexpr (Metric::PLANE) st[3] = (double)w, st[4] = Q;
    }
    int why = ICP_RUNNING;
    float g_next[12];
    for (int i = 0; i < 12; ++i) g_next[i] = g[i];
    if (w < min_matched) why = LS_ICP_STARVED;
    else if (k >= 1 && e_prev[p] - E <= rel_thr * e_prev[p]) why = LS_ICP_CONVERGED;
    else if (k == max_iter) why = LS_ICP_MAX_ITER;
    else {
        bool ok;
        if constexpr (Metric::PLANE) ok = plane_update(sums, g_next);
        else ok = point_update(sums, n, g_next);
        if (!ok) why = LS_ICP_DEGENERATE;
    }
    if (why != ICP_RUNNING) {
        stop[p] = why;
        iters[p] = k;
        for (int i = 0; i < 12; ++i) g_out[(size_t)p * 12 + i] = g[i];
        if constexpr (Metric::PLANE) planar[p] = w, sum_rho2[p] = Q;
        return;
    }
    for (int i = 0; i < 12; ++i) g[i] = g_next[i];
    e_prev[p] = E;
}

// after the loop: the targets that are a neighbour in the final search of their problem
template <class Near>
__global__ __launch_bounds__(QUERY_CHUNK) void icp_mark_kernel(Near L, const int* __restrict__ nn_idx, unsigned char* __restrict__ hit) {
    const NearRef C = L.problem(L.chunk_owner(blockIdx.x));
    const long long qi = ((long long)blockIdx.x - C.q0) * QUERY_CHUNK + threadIdx.x;
    if (qi >= C.b) return;
    const int j = nn_idx[C.b0 + qi];
    if (j >= 0) hit[C.a0 + j] = 1;
}

}  // namespace cnr
}  // namespace ls

using namespace ls;
using namespace ls::cnr;

namespace {
inline long long chunks_of(long long b) { return (b + QUERY_CHUNK - 1) / QUERY_CHUNK; }

struct Ws {
    long long* offs;          // a batch: the device copy of the offsets
    float* inv;               // a batch: [P]
    float* r2;                // a batch: [P]
    int* status;              // [P]
    long long* total;         // the scan's total: targets with a cell
    int* tcell;               // [a,3]
    int* table;               // [2 a]
    int* cnt;                 // [2 a]
    int* start;               // [2 a]
    int* blk;                 // the scan's block sums
    int4* slots;              // [2 a]
    unsigned* slot_of;        // [a]
    int* rank;                // [a]
    float4* members;          // [a]
    unsigned char* hit;       // [a]
    double* part;             // one per chunk of queries
    int2* part_cnt;           // one per chunk of queries
    float* gk;                // the ICP: [P,12] the pose of the current iteration
    double* e_prev;           // the ICP: [P] the cost of the previous iteration
    double* mom;              // the ICP: the metric's N_MOM per chunk of queries
    int* part_w;              // the plane ICP: one per chunk of queries
    size_t bytes;             // of the whole layout
};

// the layout depends on (P, a, b) alone (ws null: a sizing pass; n_offs = 0: a single problem); sum_p ceil(b_p / c) <= floor(b / c) + P.
// The ICP's pieces follow the search's, so its workspace is the search's and then its own state and one moment record per chunk (n_mom:
// the metric's N_MOM; 0: no ICP); the plane metric's count of planar matches per chunk comes last, so the point ICP's layout is what it was.
// row_chunks: an operator without queries (b = 0) whose workgroups own chunks of A's rows and leave one float64 each -- `part` holds
// those chunks and nothing else changes, so its workspace is the normals' plus 8 bytes per chunk of rows.
Ws layout(void* ws, size_t n_offs, int P, long long a, long long b, int n_mom = 0, bool row_chunks = false) {
    Arena ar(ws);
    Ws w;
    const size_t chunks = (size_t)(b / QUERY_CHUNK + P);
    w.offs = ar.take<long long>(n_offs);
    w.inv = ar.take<float>(n_offs ? (size_t)P : 0);
    w.r2 = ar.take<float>(n_offs ? (size_t)P : 0);
    w.status = ar.take<int>((size_t)P);
    w.total = ar.take<long long>(1);
    w.tcell = ar.take<int>((size_t)a * 3);
    w.table = ar.take<int>((size_t)a * 2);
    w.cnt = ar.take<int>((size_t)a * 2);
    w.start = ar.take<int>((size_t)a * 2);
    w.blk = ar.take<int>((size_t)scan_blocks(2 * a));
    w.slots = ar.take<int4>((size_t)a * 2);
    w.slot_of = ar.take<unsigned>((size_t)a);
    w.rank = ar.take<int>((size_t)a);
    w.members = ar.take<float4>((size_t)a);
    w.hit = ar.take<unsigned char>((size_t)a);
    w.part = ar.take<double>(row_chunks ? (size_t)(a / QUERY_CHUNK + P) : chunks);
    w.part_cnt = ar.take<int2>(chunks);
    w.gk = ar.take<float>(n_mom ? (size_t)P * 12 : 0);
    w.e_prev = ar.take<double>(n_mom ? (size_t)P : 0);
    w.mom = ar.take<double>(chunks * (size_t)n_mom);
    w.part_w = ar.take<int>(n_mom == PlaneMetric::N_MOM ? chunks : 0);
    w.bytes = ar.bytes();
    return w;
}

// the grid over the targets of P problems located by L: the table, the members of every cell back to back, the hit flags cleared
template <class Near>
int grid_launch(const Near& L, int P, const float* A, long long a, const Ws& w, hipStream_t st) {
    LS_HIP_CHECK(hipMemsetAsync(w.status, 0, (size_t)P * sizeof(int), st));               // LS_OK
    if (a > 0) {
        const int nb = cdiv(a, 256);
        LS_HIP_CHECK(hipMemsetAsync(w.table, 0xFF, (size_t)a * 2 * sizeof(int), st));     // -1: free
        LS_HIP_CHECK(hipMemsetAsync(w.cnt, 0, (size_t)a * 2 * sizeof(int), st));
        LS_HIP_CHECK(hipMemsetAsync(w.hit, 0, (size_t)a, st));
        hipLaunchKernelGGL(tcell_kernel<Near>, dim3(nb), dim3(256), 0, st, L, A, a, w.tcell);
        hipLaunchKernelGGL(claim_kernel<Near>, dim3(nb), dim3(256), 0, st, L, a, w.tcell, w.table, w.cnt, w.slot_of, w.rank, w.status);
        scan<int, int, false>(w.cnt, 2 * a, w.blk, w.start, w.total, st);
        hipLaunchKernelGGL(slot_kernel, dim3(cdiv(2 * a, 256)), dim3(256), 0, st, 2 * a, w.table, w.tcell, w.start, w.slots);
        hipLaunchKernelGGL(fill_kernel, dim3(nb), dim3(256), 0, st, A, a, w.slot_of, w.rank, w.start, w.members);
    }
    return LS_OK;
}

// the launch sequence: P problems located by L, a targets, b queries and `chunks` chunks of queries in all
template <class Near>
int nearest_launch(const Near& L, int P, const float* A, long long a, long long b, long long chunks, const Ws& w, int* nn_idx, float* nn_d2,
                   long long* counts, double* sum_d2, int* status_out, hipStream_t st) {
    const int rc = grid_launch(L, P, A, a, w, st);
    if (rc != LS_OK) return rc;
    if (chunks > 0)
        hipLaunchKernelGGL(query_kernel<Near>, dim3((unsigned)chunks), dim3(QUERY_CHUNK), 0, st, L, w.slots, w.cnt, w.members, w.hit, nn_idx, nn_d2,
                           w.part, w.part_cnt);
    hipLaunchKernelGGL(final_kernel<Near>, dim3(P), dim3(256), 0, st, L, w.hit, w.part, w.part_cnt, w.status, counts, sum_d2, status_out);
    LS_LAUNCH_CHECK();
    return LS_OK;
}

struct IcpArgs {
    int max_iter;
    double rel_thr;
    int min_matched;
    float* g_out;
    int* stop;
    int* iters;
    float* g_trace;
    double* stat_trace;
    const float* N = nullptr;          // the plane metric: the targets' normals, packed like A
    long long* planar = nullptr;       // the plane metric: [P] the planar matches of the final search
    double* sum_rho2 = nullptr;        // the plane metric: [P] their sum of rho^2
};

// the ICP's launch sequence: the grid once, then max_iter + 1 times (search, solve) -- the problems that have stopped exit at once -- then
// the hit flags and the counts of the final searches.  2 max_iter + 5 kernels after the grid build, whatever P and whenever problems stop.
template <class Metric, class Near>
int icp_launch(const Near& L, int P, const float* A, long long a, long long chunks, const float* g0, const IcpArgs& I, const Ws& w, int* nn_idx,
               float* nn_d2, long long* counts, double* sum_d2, int* status_out, hipStream_t st) {
    const int rc = grid_launch(L, P, A, a, w, st);
    if (rc != LS_OK) return rc;
    hipLaunchKernelGGL(icp_init_kernel, dim3(cdiv((long long)P * 12, 256)), dim3(256), 0, st, P, g0, w.gk, w.e_prev, I.stop, I.iters);
    for (int k = 0; k <= I.max_iter; ++k) {
        if (chunks > 0)
            hipLaunchKernelGGL((icp_search_kernel<Near, Metric>), dim3((unsigned)chunks), dim3(QUERY_CHUNK), 0, st, L, I.stop, w.gk, w.slots, w.cnt,
                               w.members, I.N, nn_idx, nn_d2, w.part, w.part_cnt, w.part_w, w.mom);
        hipLaunchKernelGGL((icp_solve_kernel<Near, Metric>), dim3(P), dim3(kWave), 0, st, L, k, I.max_iter, I.rel_thr, I.min_matched, w.part,
                           w.part_cnt, w.part_w, w.mom, w.gk, w.e_prev, I.stop, I.iters, I.g_out, I.planar, I.sum_rho2, I.g_trace, I.stat_trace);
    }
    if (chunks > 0) hipLaunchKernelGGL(icp_mark_kernel<Near>, dim3((unsigned)chunks), dim3(QUERY_CHUNK), 0, st, L, nn_idx, w.hit);
    hipLaunchKernelGGL(final_kernel<Near>, dim3(P), dim3(256), 0, st, L, w.hit, w.part, w.part_cnt, w.status, counts, sum_d2, status_out);
    LS_LAUNCH_CHECK();
    return LS_OK;
}

int check_icp(const char* op, const IcpArgs& I) {
    LS_REQUIRE(I.max_iter >= 0, "%s: max_iter must be >= 0, got %d", op, I.max_iter);
    LS_REQUIRE(I.max_iter < INT_MAX, "%s: max_iter %d: max_iter + 1 searches do not fit an int", op, I.max_iter);
    LS_REQUIRE(std::isfinite(I.rel_thr) && I.rel_thr >= 0.0, "%s: rel_thr must be finite and >= 0, got %g", op, I.rel_thr);
    LS_REQUIRE(I.min_matched >= 3, "%s: min_matched must be >= 3 (a rotation needs three correspondences), got %d", op, I.min_matched);
    LS_REQUIRE(I.g_out && I.stop && I.iters, "%s: null g_out / stop / iters", op);
    return LS_OK;
}

int check_plane(const char* op, long long a, const IcpArgs& I) {
    LS_REQUIRE(a == 0 || I.N, "%s: null N with %lld kept rows", op, a);
    LS_REQUIRE(I.planar && I.sum_rho2, "%s: null planar / sum_rho2", op);
    return LS_OK;
}

int check_normals(const char* op, long long a, const float* A, int min_nbrs, const float* normals, const int* nbr_cnt, const float* variation,
                  const long long* counts) {
    LS_REQUIRE(a >= 0, "%s: negative size (%lld kept rows)", op, a);
    LS_REQUIRE(a <= INT_MAX, "%s: %lld rows exceed %d (int row indices)", op, a, INT_MAX);
    LS_REQUIRE(a == 0 || (A && normals && nbr_cnt && variation), "%s: null A / normals / nbr_cnt / variation with %lld rows", op, a);
    LS_REQUIRE(counts, "%s: null counts", op);
    LS_REQUIRE(min_nbrs >= 1, "%s: min_nbrs must be >= 1, got %d", op, min_nbrs);
    return LS_OK;
}

// the normals' launch sequence: the grid, one thread per target, the counts -- 2 kernels after the grid build, whatever P
template <class Near>
int normals_launch(const Near& L, int P, const float* A, long long a, int min_nbrs, const Ws& w, float* normals, int* nbr_cnt, float* variation,
                   long long* counts, int* status_out, hipStream_t st) {
    const int rc = grid_launch(L, P, A, a, w, st);
    if (rc != LS_OK) return rc;
    if (a > 0)
        hipLaunchKernelGGL(normals_kernel<Near>, dim3(cdiv(a, 256)), dim3(256), 0, st, L, A, a, w.tcell, w.slots, w.cnt, w.members, min_nbrs, normals,
                           nbr_cnt, variation);
    hipLaunchKernelGGL(normals_final_kernel<Near>, dim3(P), dim3(256), 0, st, L, normals, nbr_cnt, w.status, counts, status_out);
    LS_LAUNCH_CHECK();
    return LS_OK;
}

struct ProjectArgs {
    int min_nbrs;
    float max_variation, max_shift;
    float* out_pts;
    int* state;
    float* shift;
    long long* counts;
    double* sum_shift2;
};

int check_project_sizes(const char* op, long long a, const float* A, const ProjectArgs& J) {
    LS_REQUIRE(a >= 0, "%s: negative size (%lld kept rows)", op, a);
    LS_REQUIRE(a <= INT_MAX, "%s: %lld rows exceed %d (int row indices)", op, a, INT_MAX);
    LS_REQUIRE(a == 0 || (A && J.out_pts && J.state && J.shift), "%s: null A / out_pts / state / shift with %lld rows", op, a);
    LS_REQUIRE(J.counts && J.sum_shift2, "%s: null counts / sum_shift2", op);
    LS_REQUIRE(a == 0 || (J.out_pts + a * 3 <= A || A + a * 3 <= J.out_pts),
               "%s: out_pts overlaps A: every row is projected from the input positions, so the operator cannot work in place", op);
    return LS_OK;
}

int check_project(const char* op, const ProjectArgs& J) {
    LS_REQUIRE(J.min_nbrs >= 1, "%s: min_nbrs must be >= 1, got %d", op, J.min_nbrs);
    LS_REQUIRE(J.max_variation >= 0.0f, "%s: max_variation must be >= 0 and not NaN (1/3 and above: no limit), got %g", op, (double)J.max_variation);
    LS_REQUIRE(J.max_shift >= 0.0f, "%s: max_shift must be >= 0 and not NaN (+inf: no limit), got %g", op, (double)J.max_shift);
    return LS_OK;
}

// the projection's launch sequence: the grid, one thread per row in chunks of one problem, the counts and sums -- 2 kernels after the
// grid build, whatever P
template <class Near>
int project_launch(const Near& L, int P, const float* A, long long a, long long chunks, const ProjectArgs& J, const Ws& w, int* status_out,
                   hipStream_t st) {
    const int rc = grid_launch(L, P, A, a, w, st);
    if (rc != LS_OK) return rc;
    if (chunks > 0)
        hipLaunchKernelGGL(project_kernel<Near>, dim3((unsigned)chunks), dim3(QUERY_CHUNK), 0, st, L, A, w.tcell, w.slots, w.cnt, w.members, J.min_nbrs,
                           (double)J.max_variation, (double)J.max_shift, J.out_pts, J.state, J.shift, w.part);
    hipLaunchKernelGGL(project_final_kernel<Near>, dim3(P), dim3(256), 0, st, L, J.state, w.part, w.status, J.counts, J.sum_shift2, status_out);
    LS_LAUNCH_CHECK();
    return LS_OK;
}

int check_common(const char* op, long long a, long long b, const float* A, const float* B, const int* nn_idx, const float* nn_d2,
                 const long long* counts, const double* sum_d2) {
    LS_REQUIRE(a >= 0 && b >= 0, "%s: negative size (%lld kept rows, %lld query rows)", op, a, b);
    LS_REQUIRE(a + b <= INT_MAX, "%s: %lld + %lld rows exceed %d (int row indices)", op, a, b, INT_MAX);
    LS_REQUIRE((a == 0 || A) && (b == 0 || B), "%s: null A / B with %lld and %lld rows", op, a, b);
    LS_REQUIRE(counts && sum_d2 && (b == 0 || (nn_idx && nn_d2)), "%s: null nn_idx / nn_d2 / counts / sum_d2", op);
    return LS_OK;
}

// One call of an operator on the grid, as its entry describes it: the single form or a ragged batch of P problems, a targets and b
// queries in all (an operator without queries: has_b false, b = 0), the radius of every problem.
struct NearCall {
    const char* op;
    bool batch;
    int P;                       // a batch: its problems
    const float* A;
    long long a;
    const long long* a_off;      // a batch: [P+1]
    bool has_b;
    const float* B;
    long long b;
    const long long* b_off;      // a batch with queries: [P+1]
    const float* g;              // the locator's pose: [3,4] / [P,3,4] or null
    const float* radius;         // a batch: [P]; the single form: the address of its one radius
    int n_mom;                   // the ICP: the metric's N_MOM; 0: no ICP
    bool row_chunks;             // no queries, but workgroups that own chunks of A's rows: the locator's queries are its targets (B = A, b = a)
    void* workspace;
    size_t workspace_bytes;
    void* stream;

    // the two forms an entry fills, every field by name; an operator without queries passes no B and clears has_b
    static NearCall one(const char* op, const float* A, long long a, const float* B, long long b, const float* g, const float* radius,
                        int n_mom, void* workspace, size_t workspace_bytes, void* stream) {
        NearCall c{};
        c.op = op, c.batch = false, c.P = 1;
        c.A = A, c.a = a, c.a_off = nullptr;
        c.has_b = true, c.B = B, c.b = b, c.b_off = nullptr;
        c.g = g, c.radius = radius, c.n_mom = n_mom, c.row_chunks = false;
        c.workspace = workspace, c.workspace_bytes = workspace_bytes, c.stream = stream;
        return c;
    }
    static NearCall ragged(const char* op, int P, const float* A, long long a_total, const long long* a_off, const float* B, long long b_total,
                           const long long* b_off, const float* g, const float* radius, int n_mom, void* workspace, size_t workspace_bytes,
                           void* stream) {
        NearCall c = one(op, A, a_total, B, b_total, g, radius, n_mom, workspace, workspace_bytes, stream);
        c.batch = true, c.P = P, c.a_off = a_off, c.b_off = b_off;
        return c;
    }
};

// every size query: 0 for sizes no call accepts
size_t near_bytes(bool batch, int P, long long a, long long b, int n_mom, bool row_chunks = false) {
    if ((batch && P < 1) || a < 0 || b < 0 || a + b > INT_MAX) return 0;
    return layout(nullptr, batch ? (size_t)OFF_ARRAYS * (P + 1) : 0, batch ? P : 1, a, b, n_mom, row_chunks).bytes;
}

// The entry path of every operator, all checks before the first HIP call and in one order: sizes() -- the operator's checks of its sizes
// and pointers -- the offsets of a batch, the radius terms and the chunks of every problem (the errors name the problem), checks() -- the
// operator's other arguments -- and the workspace; then the layout, for a batch the upload of what the locator reads, and
// launch(locator, P, layout, chunks, stream).  The single form uploads nothing and allocates nothing on the host.
template <class Sizes, class Checks, class Launch>
int near_run(const NearCall& c, Sizes&& sizes, Checks&& checks, Launch&& launch) {
    const char* op = c.op;
    LS_REQUIRE(!c.batch || c.P >= 1, "%s: P must be at least 1, got %d", op, c.P);
    const int P = c.batch ? c.P : 1;
    int rc = sizes();
    if (rc != LS_OK) return rc;
    if (c.batch) {
        rc = check_ranges(op, "problem", "a_off", P, c.a_off, c.a, INT_MAX);
        if (rc != LS_OK) return rc;
        if (c.has_b) rc = check_ranges(op, "problem", "b_off", P, c.b_off, c.b, INT_MAX);
        if (rc != LS_OK) return rc;
        LS_REQUIRE(c.radius, "%s: null radius", op);
    }
    std::vector<long long> q_off(c.batch ? P + 1 : 0, 0);               // a batch: the chunk offsets; without queries or row chunks also its b_off
    std::vector<float> terms(c.batch ? 2 * (size_t)P : 0);
    float one[2];
    float *inv = c.batch ? terms.data() : one, *r2 = inv + P;
    long long chunks = 0;
    for (int p = 0; p < P; ++p) {
        if (c.has_b) chunks += chunks_of(c.batch ? c.b_off[p + 1] - c.b_off[p] : c.b);
        if (c.row_chunks) chunks += chunks_of(c.batch ? c.a_off[p + 1] - c.a_off[p] : c.a);
        if (c.batch) q_off[p + 1] = chunks;
        rc = check_edge(op, p, "radius", "radius", c.radius[p], &inv[p], &r2[p]);
        if (rc != LS_OK) return rc;
    }
    rc = checks();
    if (rc != LS_OK) return rc;
    rc = check_workspace(op, c.workspace, c.workspace_bytes, near_bytes(c.batch, c.P, c.a, c.b, c.n_mom, c.row_chunks), c.batch ? P : 0, c.a,
                         c.has_b ? c.b : -1);
    if (rc != LS_OK) return rc;
    const Ws w = layout(c.workspace, c.batch ? (size_t)OFF_ARRAYS * (P + 1) : 0, P, c.a, c.b, c.n_mom, c.row_chunks);
    hipStream_t st = (hipStream_t)c.stream;
    const float* Q = c.row_chunks ? c.A : c.B;                          // the locator's queries
    if (!c.batch) return launch(OneNear{Q, c.a, c.row_chunks ? c.a : c.b, c.g, inv[0], r2[0]}, P, w, chunks, st);
    rc = upload_offsets(w.offs, pack_offsets(P, {c.a_off, c.has_b ? c.b_off : c.row_chunks ? c.a_off : q_off.data(), q_off.data()}), st);
    if (rc != LS_OK) return rc;
    LS_HIP_CHECK(hipMemcpyAsync(w.inv, inv, (size_t)P * sizeof(float), hipMemcpyHostToDevice, st));   // pageable: read when it returns
    LS_HIP_CHECK(hipMemcpyAsync(w.r2, r2, (size_t)P * sizeof(float), hipMemcpyHostToDevice, st));
    return launch(RaggedNear{Q, c.g, w.offs, w.inv, w.r2, P}, P, w, chunks, st);
}

const auto no_checks = [] { return LS_OK; };

// the entry of the search
int nearest_entry(const NearCall& c, int* nn_idx, float* nn_d2, long long* counts, double* sum_d2, int* status_out) {
    return near_run(
        c, [&] { return check_common(c.op, c.a, c.b, c.A, c.B, nn_idx, nn_d2, counts, sum_d2); }, no_checks,
        [&](const auto& L, int P, const Ws& w, long long chunks, hipStream_t st) {
            return nearest_launch(L, P, c.A, c.a, c.b, chunks, w, nn_idx, nn_d2, counts, sum_d2, status_out, st);
        });
}

// the entry of the ICP under either metric, from the pose g0 (the locator has none).  The plane metric's own pointers are checked with
// the sizes in the single form and after the radii in a batch.
template <class Metric>
int icp_entry(const NearCall& c, const float* g0, const IcpArgs& I, int* nn_idx, float* nn_d2, long long* counts, double* sum_d2, int* status_out) {
    const auto plane = [&] { return Metric::PLANE ? check_plane(c.op, c.a, I) : LS_OK; };
    return near_run(
        c,
        [&] {
            const int rc = check_common(c.op, c.a, c.b, c.A, c.B, nn_idx, nn_d2, counts, sum_d2);
            return rc != LS_OK || c.batch ? rc : plane();
        },
        [&] {
            const int rc = c.batch ? plane() : LS_OK;
            return rc != LS_OK ? rc : check_icp(c.op, I);
        },
        [&](const auto& L, int P, const Ws& w, long long chunks, hipStream_t st) {
            return icp_launch<Metric>(L, P, c.A, c.a, chunks, g0, I, w, nn_idx, nn_d2, counts, sum_d2, status_out, st);
        });
}

// the entry of the normals: no queries
int normals_entry(const NearCall& c, int min_nbrs, float* normals, int* nbr_cnt, float* variation, long long* counts, int* status_out) {
    return near_run(
        c, [&] { return check_normals(c.op, c.a, c.A, min_nbrs, normals, nbr_cnt, variation, counts); }, no_checks,
        [&](const auto& L, int P, const Ws& w, long long, hipStream_t st) {
            return normals_launch(L, P, c.A, c.a, min_nbrs, w, normals, nbr_cnt, variation, counts, status_out, st);
        });
}

// the entry of the projection: no queries, chunks of the kept rows
int project_entry(NearCall c, const ProjectArgs& J, int* status_out) {
    c.has_b = false, c.row_chunks = true;
    return near_run(
        c, [&] { return check_project_sizes(c.op, c.a, c.A, J); }, [&] { return check_project(c.op, J); },
        [&](const auto& L, int P, const Ws& w, long long chunks, hipStream_t st) {
            return project_launch(L, P, c.A, c.a, chunks, J, w, status_out, st);
        });
}
}  // namespace

extern "C" {

size_t ls_cloud_nearest_workspace_bytes(long long a, long long b) { return near_bytes(false, 1, a, b, 0); }
size_t ls_cloud_nearest_batch_workspace_bytes(int P, long long a_total, long long b_total) { return near_bytes(true, P, a_total, b_total, 0); }
size_t ls_cloud_icp_workspace_bytes(long long a, long long b) { return near_bytes(false, 1, a, b, PointMetric::N_MOM); }
size_t ls_cloud_icp_batch_workspace_bytes(int P, long long a_total, long long b_total) {
    return near_bytes(true, P, a_total, b_total, PointMetric::N_MOM);
}
size_t ls_cloud_icp_plane_workspace_bytes(long long a, long long b) { return near_bytes(false, 1, a, b, PlaneMetric::N_MOM); }
size_t ls_cloud_icp_plane_batch_workspace_bytes(int P, long long a_total, long long b_total) {
    return near_bytes(true, P, a_total, b_total, PlaneMetric::N_MOM);
}
size_t ls_cloud_normals_workspace_bytes(long long a) { return near_bytes(false, 1, a, 0, 0); }
size_t ls_cloud_normals_batch_workspace_bytes(int P, long long a_total) { return near_bytes(true, P, a_total, 0, 0); }

int ls_cloud_nearest_f32(const float* A, long long a, const float* B, long long b, const float* g, float radius, int32_t* nn_idx, float* nn_d2,
                         long long* counts, double* sum_d2, int* status_out, void* workspace, size_t workspace_bytes, void* stream) {
    const NearCall c = NearCall::one("cloud_nearest", A, a, B, b, g, &radius, 0, workspace, workspace_bytes, stream);
    return nearest_entry(c, nn_idx, nn_d2, counts, sum_d2, status_out);
}

int ls_cloud_nearest_batch_f32(int P, const float* A, long long a_total, const long long* a_off, const float* B, long long b_total,
                               const long long* b_off, const float* g, const float* radius, int32_t* nn_idx, float* nn_d2, long long* counts,
                               double* sum_d2, int* status_out, void* workspace, size_t workspace_bytes, void* stream) {
    const NearCall c = NearCall::ragged("cloud_nearest_batch", P, A, a_total, a_off, B, b_total, b_off, g, radius, 0, workspace, workspace_bytes, stream);
    return nearest_entry(c, nn_idx, nn_d2, counts, sum_d2, status_out);
}

int ls_cloud_icp_f32(const float* A, long long a, const float* B, long long b, const float* g0, float radius, int max_iter, double rel_thr,
                     int min_matched, float* g_out, int32_t* stop, int32_t* iters, int32_t* nn_idx, float* nn_d2, long long* counts, double* sum_d2,
                     int* status_out, float* g_trace, double* stat_trace, void* workspace, size_t workspace_bytes, void* stream) {
    const NearCall c = NearCall::one("cloud_icp", A, a, B, b, nullptr, &radius, PointMetric::N_MOM, workspace, workspace_bytes, stream);
    const IcpArgs I{max_iter, rel_thr, min_matched, g_out, stop, iters, g_trace, stat_trace};
    return icp_entry<PointMetric>(c, g0, I, nn_idx, nn_d2, counts, sum_d2, status_out);
}

int ls_cloud_icp_batch_f32(int P, const float* A, long long a_total, const long long* a_off, const float* B, long long b_total,
                           const long long* b_off, const float* g0, const float* radius, int max_iter, double rel_thr, int min_matched,
                           float* g_out, int32_t* stop, int32_t* iters, int32_t* nn_idx, float* nn_d2, long long* counts, double* sum_d2,
                           int* status_out, float* g_trace, double* stat_trace, void* workspace, size_t workspace_bytes, void* stream) {
    const NearCall c = NearCall::ragged("cloud_icp_batch", P, A, a_total, a_off, B, b_total, b_off, nullptr, radius, PointMetric::N_MOM, workspace,
                                        workspace_bytes, stream);
    const IcpArgs I{max_iter, rel_thr, min_matched, g_out, stop, iters, g_trace, stat_trace};
    return icp_entry<PointMetric>(c, g0, I, nn_idx, nn_d2, counts, sum_d2, status_out);
}

int ls_cloud_icp_plane_f32(const float* A, const float* N, long long a, const float* B, long long b, const float* g0, float radius, int max_iter,
                           double rel_thr, int min_matched, float* g_out, int32_t* stop, int32_t* iters, int32_t* nn_idx, float* nn_d2,
                           long long* counts, double* sum_d2, long long* planar, double* sum_rho2, int* status_out, float* g_trace,
                           double* stat_trace, void* workspace, size_t workspace_bytes, void* stream) {
    const NearCall c = NearCall::one("cloud_icp_plane", A, a, B, b, nullptr, &radius, PlaneMetric::N_MOM, workspace, workspace_bytes, stream);
    const IcpArgs I{max_iter, rel_thr, min_matched, g_out, stop, iters, g_trace, stat_trace, N, planar, sum_rho2};
    return icp_entry<PlaneMetric>(c, g0, I, nn_idx, nn_d2, counts, sum_d2, status_out);
}

int ls_cloud_icp_plane_batch_f32(int P, const float* A, const float* N, long long a_total, const long long* a_off, const float* B,
                                 long long b_total, const long long* b_off, const float* g0, const float* radius, int max_iter, double rel_thr,
                                 int min_matched, float* g_out, int32_t* stop, int32_t* iters, int32_t* nn_idx, float* nn_d2, long long* counts,
                                 double* sum_d2, long long* planar, double* sum_rho2, int* status_out, float* g_trace, double* stat_trace,
                                 void* workspace, size_t workspace_bytes, void* stream) {
    const NearCall c = NearCall::ragged("cloud_icp_plane_batch", P, A, a_total, a_off, B, b_total, b_off, nullptr, radius, PlaneMetric::N_MOM,
                                        workspace, workspace_bytes, stream);
    const IcpArgs I{max_iter, rel_thr, min_matched, g_out, stop, iters, g_trace, stat_trace, N, planar, sum_rho2};
    return icp_entry<PlaneMetric>(c, g0, I, nn_idx, nn_d2, counts, sum_d2, status_out);
}

int ls_cloud_normals_f32(const float* A, long long a, float radius, int min_nbrs, float* normals, int32_t* nbr_cnt, float* variation,
                         long long* counts, int* status_out, void* workspace, size_t workspace_bytes, void* stream) {
    NearCall c = NearCall::one("cloud_normals", A, a, nullptr, 0, nullptr, &radius, 0, workspace, workspace_bytes, stream);
    c.has_b = false;
    return normals_entry(c, min_nbrs, normals, nbr_cnt, variation, counts, status_out);
}

int ls_cloud_normals_batch_f32(int P, const float* A, long long a_total, const long long* a_off, const float* radius, int min_nbrs,
                               float* normals, int32_t* nbr_cnt, float* variation, long long* counts, int* status_out, void* workspace,
                               size_t workspace_bytes, void* stream) {
    NearCall c = NearCall::ragged("cloud_normals_batch", P, A, a_total, a_off, nullptr, 0, nullptr, nullptr, radius, 0, workspace, workspace_bytes, stream);
    c.has_b = false;
    return normals_entry(c, min_nbrs, normals, nbr_cnt, variation, counts, status_out);
}

size_t ls_cloud_project_workspace_bytes(long long a) { return near_bytes(false, 1, a, 0, 0, true); }
size_t ls_cloud_project_batch_workspace_bytes(int P, long long a_total) { return near_bytes(true, P, a_total, 0, 0, true); }

int ls_cloud_project_f32(const float* A, long long a, float radius, int min_nbrs, float max_variation, float max_shift, float* out_pts,
                         int32_t* state, float* shift, long long* counts, double* sum_shift2, int* status_out, void* workspace,
                         size_t workspace_bytes, void* stream) {
    const NearCall c = NearCall::one("cloud_project", A, a, nullptr, 0, nullptr, &radius, 0, workspace, workspace_bytes, stream);
    return project_entry(c, ProjectArgs{min_nbrs, max_variation, max_shift, out_pts, state, shift, counts, sum_shift2}, status_out);
}

int ls_cloud_project_batch_f32(int P, const float* A, long long a_total, const long long* a_off, const float* radius, int min_nbrs,
                               float max_variation, float max_shift, float* out_pts, int32_t* state, float* shift, long long* counts,
                               double* sum_shift2, int* status_out, void* workspace, size_t workspace_bytes, void* stream) {
    const NearCall c = NearCall::ragged("cloud_project_batch", P, A, a_total, a_off, nullptr, 0, nullptr, nullptr, radius, 0, workspace,
                                        workspace_bytes, stream);
    return project_entry(c, ProjectArgs{min_nbrs, max_variation, max_shift, out_pts, state, shift, counts, sum_shift2}, status_out);
}

}  // extern "C"
