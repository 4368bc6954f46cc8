// tsdfprior.hip -- scene memory: the shape prior's field as VOTES in the fused state of an instance (depthfuse.hip: sum, n).  The
// lattice samples the cameras left short of `weight` observations become query rows for the decoder; its values come back as integer
// votes of the missing weight into a SECOND state of the same format, so the mesh, raycast and sample operators read the completed
// state unchanged.  The observed state is never written.  The definitions are in include/livingscenes_hip.h (ls_tsdf_prior_rows_f32,
// ls_tsdf_prior_vote_f32) and, as NumPy, in tests/tsdf_prior_oracle.py; the arithmetic of a sample is tsdfprior_plan.h, which
// tests/tools/tsdfprior_plan_run.cpp runs on the host.  What this file adds:
//   classify   a workgroup owns one block of PRIOR_BLOCK = 4096 consecutive samples of ONE problem (blockIdx.y), a thread every 256th
//              of them: consecutive k on consecutive lanes, the 16 int32 loads of a thread issued before the first use.  The
//              eligibility of 64 consecutive samples is one ballot, stored as the mask word of those samples; the popcounts are summed
//              per workgroup into the block's count.
//   scan       ONE workgroup per call: scan_top_block (ls_scan.h) over the P * nblk block counts, in place -- the rows of a batch are
//              one packed list, problems in order -- then the row offset of every problem and its counts.
//   emit       workgroup = block: the exclusive prefix of the popcounts of its 64 mask words (one wave), then every set bit writes its
//              row at block offset + word prefix + popcount of the lower lanes.  The state is not read again.
//   vote       workgroup = block, ONE pass over the whole volume: it forms the ballots of its samples again from n (which it reads
//              anyway), finds the row of an eligible sample as emit does, and writes (sum', n') of EVERY sample.  The voted / skipped
//              counts are two integer atomics per workgroup.
// Launches: rows: the copy of the host grids into the workspace and 2 kernels (sizing) or 3, whatever P; a vote: the copy and 3
// kernels (classify, scan, vote).  No host synchronisation, no allocation, no floating-point atomics, no compact list;
// hipGetLastError() after every launch, the pass named.  The single entries are the batch of one problem.
#include <climits>
#include <cmath>
#include <vector>

#include "ls_common.h"
#include "ls_ragged.h"
#include "ls_scan.h"
#include "ls_workspace.h"

// the arithmetic of the definition as written: no contraction of a * b + c into an fma anywhere in this file
#pragma clang fp contract(off)
#include "tsdfprior_plan.h"

namespace ls {
namespace tpk {
using namespace tp;

constexpr int ITEMS = PRIOR_BLOCK / PRIOR_THREADS;
constexpr int WAVES = PRIOR_THREADS / kWave;
static_assert(PRIOR_THREADS == 4 * kWave && PRIOR_WORD == kWave && PRIOR_BLOCK == PRIOR_THREADS * ITEMS && ITEMS * WAVES == PRIOR_BLOCK_WORDS,
              "a block: 16 ballots of each of four waves");
static_assert(PRIOR_BLOCK_WORDS == kWave, "the word prefix of a block is one wave");
static_assert(sizeof(u64) == 8 && sizeof(double) == 8 && sizeof(long long) == 8, "the uploaded words");

struct PriorArgs {
    const int* sum;                // [P,nx,ny,nz], the vote only
    const int* n;                  // [P,nx,ny,nz]
    int dims[3];
    long long voxels;              // nx ny nz
    int w0, nblk, P;
    const double* grids;           // [P,6]: origin, voxel, trunc, s, in the workspace
    long long* blk;                // [P,nblk]: eligible samples per block, then their exclusive scan over the whole call
    u64* masks;                    // [P,nblk,PRIOR_BLOCK_WORDS]
    long long* row_off;            // [P+1] or null (the vote)
    long long* counts;             // [P,4] or null
    float* points;                 // [R,3]
    int* row_inst;                 // [R]
    int* row_index;                // [R]
    long long cap_rows;
    const float* values;           // [R]
    long long rows;
    int* sum_out;                  // [P,nx,ny,nz]
    int* n_out;
};

// pass 1: workgroup = block blockIdx.x of problem blockIdx.y
__global__ __launch_bounds__(PRIOR_THREADS) void tsdf_prior_classify_kernel(PriorArgs G) {
    __shared__ int red[WAVES];
    const int p = blockIdx.y;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int* __restrict__ n = G.n + (size_t)p * G.voxels;
    const long long first = (long long)blockIdx.x * PRIOR_BLOCK + threadIdx.x;
    int c[ITEMS];
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {                                  // 16 loads in flight before the first use
        const long long at = first + (long long)it * PRIOR_THREADS;
        c[it] = at < G.voxels ? n[at] : INT_MAX;                          // never eligible: w0 <= 65535
    }
    u64* words = G.masks + ((size_t)p * G.nblk + blockIdx.x) * PRIOR_BLOCK_WORDS;
    int acc = 0;
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
        const u64 m = __ballot(prior_weight(G.w0, c[it]) > 0);
        if (lane == 0) words[it * WAVES + wave] = m;                      // word (it * 4 + wave) of the block: samples in linear order
        acc += __popcll(m);
    }
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) G.blk[(size_t)p * G.nblk + blockIdx.x] = (long long)((red[0] + red[1]) + (red[2] + red[3]));
}

// pass 2: one workgroup: the exclusive scan of every block count of the call in place, the row offsets, the counts
__global__ __launch_bounds__(1024) void tsdf_prior_scan_kernel(PriorArgs G) {
    const long long total = scan_top_block<long long>(G.blk, G.P * G.nblk);
    __syncthreads();                                                      // the scanned counts of the other threads
    for (int p = threadIdx.x; p < G.P; p += 1024) {
        const long long own = G.blk[(size_t)p * G.nblk];
        const long long next = p + 1 < G.P ? G.blk[(size_t)(p + 1) * G.nblk] : total;
        if (G.row_off) G.row_off[p] = own;
        if (G.counts) {
            long long* cnt = G.counts + (size_t)p * PRIOR_FIELDS;
            cnt[PRIOR_ELIGIBLE] = next - own, cnt[PRIOR_VOTED] = 0, cnt[PRIOR_SKIPPED] = 0, cnt[PRIOR_UNTOUCHED] = G.voxels - (next - own);
        }
    }
    if (threadIdx.x == 0 && G.row_off) G.row_off[G.P] = total;
}

// pre[0 .. 64): the counts of a block's words -> their exclusive prefix, by the first wave.  Every thread of the workgroup calls it,
// after a barrier behind the writes of pre.
__device__ __forceinline__ void word_prefix(int* pre) {
    if (threadIdx.x < kWave) {
        const int c = pre[threadIdx.x];
        int v = c;
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) {
            const int a = __shfl_up(v, o, kWave);
            if ((int)threadIdx.x >= o) v += a;
        }
        pre[threadIdx.x] = v - c;
    }
    __syncthreads();
}

// pass 3 of the rows: workgroup = block blockIdx.x of problem blockIdx.y
__global__ __launch_bounds__(PRIOR_THREADS) void tsdf_prior_emit_kernel(PriorArgs G) {
    __shared__ u64 word[PRIOR_BLOCK_WORDS];
    __shared__ int pre[PRIOR_BLOCK_WORDS];
    const int p = blockIdx.y;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    if (threadIdx.x < PRIOR_BLOCK_WORDS) {
        const u64 m = G.masks[((size_t)p * G.nblk + blockIdx.x) * PRIOR_BLOCK_WORDS + threadIdx.x];
        word[threadIdx.x] = m;
        pre[threadIdx.x] = __popcll(m);
    }
    __syncthreads();
    word_prefix(pre);
    const long long base = G.blk[(size_t)p * G.nblk + blockIdx.x];
    const double* grid = G.grids + (size_t)p * PRIOR_GRID_WORDS;
#pragma unroll 4
    for (int it = 0; it < ITEMS; ++it) {
        const int wd = it * WAVES + wave;
        const u64 bits = word[wd];
        if (!((bits >> lane) & 1ull)) continue;
        const long long row = base + pre[wd] + __popcll(bits & ((1ull << lane) - 1ull));
        const long long at = (long long)blockIdx.x * PRIOR_BLOCK + (long long)wd * PRIOR_WORD + lane;
        if (row >= G.cap_rows || at >= G.voxels) continue;                // never, unless the state changed behind the sizing call
        float point[3];
        prior_row(at, G.dims, grid, grid[3], point);
        for (int a = 0; a < 3; ++a) G.points[(size_t)row * 3 + a] = point[a];
        G.row_inst[row] = p;
        G.row_index[row] = (int)at;
    }
}

// pass 3 of the vote: workgroup = block blockIdx.x of problem blockIdx.y; every sample of the volume is written
__global__ __launch_bounds__(PRIOR_THREADS) void tsdf_prior_vote_kernel(PriorArgs G) {
    __shared__ int pre[PRIOR_BLOCK_WORDS];
    __shared__ int tally[WAVES][2];
    const int p = blockIdx.y;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const size_t vol = (size_t)p * G.voxels;
    const int* __restrict__ sum = G.sum + vol;
    const int* __restrict__ n = G.n + vol;
    const long long first = (long long)blockIdx.x * PRIOR_BLOCK + threadIdx.x;
    int s[ITEMS], c[ITEMS];
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {                                  // 32 loads in flight before the first use
        const long long at = first + (long long)it * PRIOR_THREADS;
        const bool in = at < G.voxels;
        s[it] = in ? sum[at] : 0;
        c[it] = in ? n[at] : INT_MAX;
    }
    u64 mine[ITEMS];
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
        mine[it] = __ballot(prior_weight(G.w0, c[it]) > 0);
        if (lane == 0) pre[it * WAVES + wave] = __popcll(mine[it]);
    }
    __syncthreads();
    word_prefix(pre);
    const long long base = G.blk[(size_t)p * G.nblk + blockIdx.x];
    const double* grid = G.grids + (size_t)p * PRIOR_GRID_WORDS;
    const double trunc = grid[4], scale = grid[5];
    int cast = 0, skipped = 0;
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
        const long long at = first + (long long)it * PRIOR_THREADS;
        float f = NAN;                                                    // a row past the values casts no vote
        if ((mine[it] >> lane) & 1ull) {
            const long long row = base + pre[it * WAVES + wave] + __popcll(mine[it] & ((1ull << lane) - 1ull));
            if (row < G.rows) f = G.values[row];
        }
        int so, no;
        const int did = prior_vote(s[it], c[it], G.w0, scale, trunc, f, &so, &no);
        if (at < G.voxels) G.sum_out[vol + at] = so, G.n_out[vol + at] = no;
        cast += __popcll(__ballot(did == VOTE_CAST));
        skipped += __popcll(__ballot(did == VOTE_SKIPPED));
    }
    if (lane == 0) tally[wave][0] = cast, tally[wave][1] = skipped;
    __syncthreads();
    if (threadIdx.x < 2) {
        const int t = (tally[0][threadIdx.x] + tally[1][threadIdx.x]) + (tally[2][threadIdx.x] + tally[3][threadIdx.x]);
        if (t) atomicAdd((u64*)(G.counts + (size_t)p * PRIOR_FIELDS + (threadIdx.x == 0 ? PRIOR_VOTED : PRIOR_SKIPPED)), (u64)t);
    }
}

}  // namespace tpk
}  // namespace ls

using namespace ls;
using namespace ls::tpk;

namespace {
struct Ws {
    double* grids;
    long long* blk;
    u64* masks;
    int nblk;
    size_t bytes;
};

// the one layout: the pieces of tsdfprior_plan.h from one Arena (ws null: a sizing pass)
Ws layout(void* ws, int P, int nx, int ny, int nz) {
    const PriorPieces c = prior_pieces(P, nx, ny, nz);
    Arena ar(ws);
    Ws w;
    w.grids = ar.take<double>(c.grids);
    w.blk = ar.take<long long>(c.blocks);
    w.masks = ar.take<u64>(c.masks);
    w.nblk = (int)c.nblk;
    w.bytes = ar.bytes();
    return w;
}

size_t workspace_need(int P, int nx, int ny, int nz) {
    if (!fp::fuse_sizes_ok(P, nx, ny, nz) || prior_bad_sizes(P, nx, ny, nz) != 0) return 0;
    return layout(nullptr, P, nx, ny, nz).bytes;
}

#define LS_PRIOR_PASS(name)                                                                                  \
    do {                                                                                                     \
        hipError_t _e = hipGetLastError();                                                                   \
        if (_e != hipSuccess) {                                                                              \
            ls::set_error("%s: the %s pass failed to launch: %s (%s:%d)", op, name, hipGetErrorString(_e), __FILE__, __LINE__); \
            return LS_ERR_HIP;                                                                               \
        }                                                                                                    \
    } while (0)

// What both entries decide on the host, then the copy of the host grids and the passes.  vote: sum, trunc, s, values, sum_out and n_out
// are the vote's, the rest the rows'; the workspace query is the rows' for both.
int prior_run(const char* op, const char* query, bool vote, int P, const int32_t* sum, const int32_t* n, int nx, int ny, int nz, int weight,
              const double* origin, const double* voxel, const double* s, const double* trunc, float* points, int32_t* row_inst, int32_t* row_index,
              long long cap_rows, long long* row_off, const float* values, long long rows, int32_t* sum_out, int32_t* n_out, long long* counts,
              void* workspace, size_t workspace_bytes, hipStream_t st) {
    LS_REQUIRE(P >= 1, "%s: P must be at least 1, got %d", op, P);
    LS_REQUIRE(nx >= 1 && ny >= 1 && nz >= 1, "%s: dims must be at least 1, got %d x %d x %d", op, nx, ny, nz);
    LS_REQUIRE(fp::fuse_sizes_ok(P, nx, ny, nz), "%s: P * nx * ny * nz = %d * %d * %d * %d reaches 2^31 (int32 state indices)", op, P, nx, ny, nz);
    const int bad = prior_bad_sizes(P, nx, ny, nz);
    LS_REQUIRE(bad != 1, "%s: nx * ny * nz = %d * %d * %d exceeds %d blocks of %d samples (the scan limit of the draw)", op, nx, ny, nz,
               PRIOR_MAX_BLOCKS, PRIOR_BLOCK);
    LS_REQUIRE(bad != 2, "%s: P = %d outside 1..%d", op, P, PRIOR_MAX_BATCH);
    LS_REQUIRE(prior_bad_weight(weight) == 0, "%s: weight must be in 1..%d (the votes the prior tops a sample up to), got %d", op, PRIOR_MAX_WEIGHT,
               weight);
    if (vote) {
        LS_REQUIRE(sum && n, "%s: null sum / n", op);
        LS_REQUIRE(s && trunc, "%s: null s / trunc", op);
        LS_REQUIRE(rows >= 0, "%s: negative row count %lld", op, rows);
        LS_REQUIRE(values || rows == 0, "%s: null values", op);
        LS_REQUIRE(sum_out && n_out, "%s: null sum_out / n_out", op);
        LS_REQUIRE(sum_out != sum && n_out != n && sum_out != n && n_out != sum, "%s: the completed state is a separate pair: the observed state is read only", op);
        LS_REQUIRE(counts, "%s: null counts", op);
    } else {
        LS_REQUIRE(n, "%s: null n", op);
        LS_REQUIRE(origin && voxel, "%s: null origin / voxel", op);
        LS_REQUIRE(cap_rows >= 0, "%s: negative capacity %lld", op, cap_rows);
        LS_REQUIRE((points != nullptr) == (row_inst != nullptr) && (points != nullptr) == (row_index != nullptr),
                   "%s: points, row_inst and row_index come together (all null: a sizing call)", op);
        LS_REQUIRE(row_off, "%s: null row_off", op);
    }
    std::vector<long long> host((size_t)P * PRIOR_GRID_WORDS);
    double* grids = (double*)host.data();                                    // 8-byte words both
    const double zero[3] = {0.0, 0.0, 0.0};
    for (int p = 0; p < P; ++p) {
        double* gr = grids + (size_t)p * PRIOR_GRID_WORDS;
        for (int a = 0; a < PRIOR_GRID_WORDS; ++a) gr[a] = 0.0;
        if (vote) {
            LS_REQUIRE(prior_bad_scale(s[p]) == 0, "%s: problem %d: s must be finite and > 0, got %g", op, p, s[p]);
            LS_REQUIRE(fp::fuse_bad_grid(zero, 1.0, trunc[p]) == 0, "%s: problem %d: trunc must be finite and > 0, got %g", op, p, trunc[p]);
            gr[4] = trunc[p], gr[5] = s[p];
        } else {
            const int g = fp::fuse_bad_grid(origin + (size_t)p * 3, voxel[p], 1.0);
            LS_REQUIRE(g != 1, "%s: problem %d: origin must be finite, got (%g, %g, %g)", op, p, origin[p * 3], origin[p * 3 + 1], origin[p * 3 + 2]);
            LS_REQUIRE(g != 2, "%s: problem %d: voxel must be finite and > 0, got %g", op, p, voxel[p]);
            for (int a = 0; a < 3; ++a) gr[a] = origin[(size_t)p * 3 + a];
            gr[3] = voxel[p];
        }
    }
    const size_t need = workspace_need(P, nx, ny, nz);
    if (!(workspace && workspace_bytes >= need)) {
        set_error("%s: workspace %zu < required %zu (%s)", op, workspace ? workspace_bytes : (size_t)0, need, query);
        return LS_ERR_WORKSPACE;
    }
    const Ws w = layout(workspace, P, nx, ny, nz);
    int rc = upload_offsets((long long*)w.grids, host, st);
    if (rc != LS_OK) return rc;
    PriorArgs G{};
    G.sum = sum, G.n = n;
    G.dims[0] = nx, G.dims[1] = ny, G.dims[2] = nz;
    G.voxels = (long long)nx * ny * nz;
    G.w0 = weight, G.nblk = w.nblk, G.P = P;
    G.grids = w.grids, G.blk = w.blk, G.masks = w.masks;
    G.row_off = row_off, G.counts = counts;
    G.points = points, G.row_inst = row_inst, G.row_index = row_index, G.cap_rows = cap_rows;
    G.values = values, G.rows = rows, G.sum_out = sum_out, G.n_out = n_out;
    const dim3 grid((unsigned)w.nblk, (unsigned)P);
    hipLaunchKernelGGL(tsdf_prior_classify_kernel, grid, dim3(PRIOR_THREADS), 0, st, G);
    LS_PRIOR_PASS("classify");
    hipLaunchKernelGGL(tsdf_prior_scan_kernel, dim3(1), dim3(1024), 0, st, G);
    LS_PRIOR_PASS("scan");
    if (vote) {
        hipLaunchKernelGGL(tsdf_prior_vote_kernel, grid, dim3(PRIOR_THREADS), 0, st, G);
        LS_PRIOR_PASS("vote");
    } else if (points && cap_rows > 0) {
        hipLaunchKernelGGL(tsdf_prior_emit_kernel, grid, dim3(PRIOR_THREADS), 0, st, G);
        LS_PRIOR_PASS("emit");
    }
    return LS_OK;
}
}  // namespace

extern "C" {

size_t ls_tsdf_prior_rows_workspace_bytes(int nx, int ny, int nz) { return workspace_need(1, nx, ny, nz); }
size_t ls_tsdf_prior_rows_batch_workspace_bytes(int P, int nx, int ny, int nz) { return workspace_need(P, nx, ny, nz); }

int ls_tsdf_prior_rows_f32(const int32_t* n, int nx, int ny, int nz, int weight, const double* origin, double voxel, float* points, int32_t* row_inst,
                           int32_t* row_index, long long cap_rows, long long* row_off, long long* counts, void* workspace, size_t workspace_bytes,
                           void* stream) {
    return prior_run("tsdf_prior_rows", "ls_tsdf_prior_rows_workspace_bytes", false, 1, nullptr, n, nx, ny, nz, weight, origin, &voxel, nullptr, nullptr,
                     points, row_inst, row_index, cap_rows, row_off, nullptr, 0, nullptr, nullptr, counts, workspace, workspace_bytes, (hipStream_t)stream);
}

int ls_tsdf_prior_rows_batch_f32(int P, const int32_t* n, int nx, int ny, int nz, int weight, const double* origin, const double* voxel, float* points,
                                 int32_t* row_inst, int32_t* row_index, long long cap_rows, long long* row_off, long long* counts, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    return prior_run("tsdf_prior_rows_batch", "ls_tsdf_prior_rows_batch_workspace_bytes", false, P, nullptr, n, nx, ny, nz, weight, origin, voxel, nullptr,
                     nullptr, points, row_inst, row_index, cap_rows, row_off, nullptr, 0, nullptr, nullptr, counts, workspace, workspace_bytes,
                     (hipStream_t)stream);
}

int ls_tsdf_prior_vote_f32(const int32_t* sum, const int32_t* n, int nx, int ny, int nz, int weight, double s, double trunc, const float* values,
                           long long rows, int32_t* sum_out, int32_t* n_out, long long* counts, void* workspace, size_t workspace_bytes, void* stream) {
    return prior_run("tsdf_prior_vote", "ls_tsdf_prior_rows_workspace_bytes", true, 1, sum, n, nx, ny, nz, weight, nullptr, nullptr, &s, &trunc, nullptr,
                     nullptr, nullptr, 0, nullptr, values, rows, sum_out, n_out, counts, workspace, workspace_bytes, (hipStream_t)stream);
}

int ls_tsdf_prior_vote_batch_f32(int P, const int32_t* sum, const int32_t* n, int nx, int ny, int nz, int weight, const double* s, const double* trunc,
                                 const float* values, long long rows, int32_t* sum_out, int32_t* n_out, long long* counts, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    return prior_run("tsdf_prior_vote_batch", "ls_tsdf_prior_rows_batch_workspace_bytes", true, P, sum, n, nx, ny, nz, weight, nullptr, nullptr, s, trunc,
                     nullptr, nullptr, nullptr, 0, nullptr, values, rows, sum_out, n_out, counts, workspace, workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"
