// tsdffit.hip -- scene memory: the fused state of an instance (depthfuse.hip: sum, n) as a TRAINING SIGNAL for its latent code.  A
// deterministic draw of a fixed number of band and free-space lattice samples out of the state, and the loss that holds the decoder to
// them: equality inside the band, a one-sided hinge in observed free space.  The definitions are in include/livingscenes_hip.h
// (ls_tsdf_draw_f32, ls_tsdf_fit_loss_f64) and, as NumPy, in tests/tsdf_fit_oracle.py; the arithmetic of a column is tsdffit_plan.h,
// which tests/tools/tsdffit_plan_run.cpp runs on the host.  What this file adds:
//   classify   a workgroup owns one block of DRAW_BLOCK = 4096 consecutive samples of ONE problem (blockIdx.y), a thread every 256th of
//              them: consecutive k on consecutive lanes, the 32 int32 loads of a thread issued before the first use.  The kind of 64
//              consecutive samples becomes two ballots, stored as the mask words (band, free) of those samples; their popcounts are
//              summed per workgroup into one packed count (band << 32 | free).
//   scan       one workgroup per problem: scan_top_block (ls_scan.h) over the problem's packed block counts, in place; the totals are
//              the lengths of the two lists and the counts of the call.
//   resolve    one thread per column: its stratum's rank (draw_rank), the block by a binary search over the scanned counts, the word by
//              the popcounts of the block's 64 mask words, the bit inside the word; then the column of that sample (draw_column).
//              The ranks are resolved by SEARCH: no compact list is written (it would cost 4 bytes per sample of stores beside the 8
//              bytes per sample that must be read; the masks cost 1/4 byte).
//   loss       one launch: workgroup (c, p) owns chunk c of SAMPLE_CHUNK columns of problem p -- it counts the problem's non-PAD
//              columns itself and writes its columns' gradient; the workgroup of chunk 0 also forms every chunk record of its problem,
//              in chunk order, by the tree of tsdficp.hip (wave shuffles and four LDS words), and adds them from 0.0: the loss and the
//              best-loss bookkeeping of ls_mse_f32.  The order is fixed, so there is no second stage and no atomic.
// Launches: a draw: the copy of the host arrays into the workspace and 3 kernels, whatever P; a loss: 1 kernel.  No host synchronisation,
// no allocation, no atomics; hipGetLastError() after every launch, the pass named.  The single draw is the batch of one problem.
#include <climits>
#include <cmath>
#include <vector>

#include "ls_common.h"
#include "ls_ragged.h"
#include "ls_scan.h"
#include "ls_workspace.h"

// the arithmetic of the definition as written: no contraction of a * b + c into an fma anywhere in this file
#pragma clang fp contract(off)
#include "se3_gn.h"
#include "tsdffit_plan.h"

namespace ls {
namespace tfk {
using namespace tf;
using ts::SAMPLE_CHUNK;
using ts::SAMPLE_WAVE;

static_assert(SAMPLE_CHUNK == 4 * kWave && SAMPLE_WAVE == kWave, "the chunk rule: four waves of 64");
static_assert(DRAW_THREADS == 4 * kWave && DRAW_WORD == kWave && DRAW_BLOCK == DRAW_THREADS * 16, "a block: 16 ballots of each of four waves");
static_assert(DRAW_MAX_BLOCKS == SCAN_MAX_BLOCKS, "the scan of a problem's blocks is the top-level scan of ls_scan.h");
static_assert(sizeof(u64) == 8 && sizeof(double) == 8, "the uploaded words");

struct DrawArgs {
    const int* sum;                // [P,nx,ny,nz]
    const int* n;                  // [P,nx,ny,nz]
    int dims[3];
    long long voxels;              // nx ny nz
    int min_obs, nblk;
    long long n_band, n_free;
    const u64* seeds;              // [P], in the workspace
    const double* grids;           // [P,5]: origin, voxel, trunc, in the workspace
    u64* blk;                      // [P,nblk]: packed counts (band << 32 | free), then their exclusive scan
    u64* totals;                   // [P]
    u64* masks;                    // [P,nblk,DRAW_BLOCK_WORDS,2]
    float* points;                 // [P,N,3]
    double* target;                // [P,N]
    unsigned char* kind;           // [P,N]
    int* index;                    // [P,N]
    long long* counts;             // [P,3]
};

// pass 1: workgroup = block blockIdx.x of problem blockIdx.y
__global__ __launch_bounds__(DRAW_THREADS) void tsdf_draw_classify_kernel(DrawArgs G) {
    __shared__ u64 red[DRAW_THREADS / kWave];
    const int p = blockIdx.y;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int* __restrict__ sum = G.sum + (size_t)p * G.voxels;
    const int* __restrict__ n = G.n + (size_t)p * G.voxels;
    const long long first = (long long)blockIdx.x * DRAW_BLOCK + threadIdx.x;
    constexpr int ITEMS = DRAW_BLOCK / DRAW_THREADS;
    int s[ITEMS], c[ITEMS];
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {                                  // 32 loads in flight before the first use
        const long long at = first + (long long)it * DRAW_THREADS;
        const bool in = at < G.voxels;
        s[it] = in ? sum[at] : 0;
        c[it] = in ? n[at] : INT_MIN;                                     // never eligible: min_obs >= 1
    }
    u64* words = G.masks + ((size_t)p * G.nblk + blockIdx.x) * (DRAW_BLOCK_WORDS * 2);
    u64 acc = 0;
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
        const int kind = draw_kind(s[it], c[it], G.min_obs);
        const u64 mb = __ballot(kind == FIT_BAND), mf = __ballot(kind == FIT_FREE);
        if (lane == 0) {
            words[(it * (DRAW_THREADS / kWave) + wave) * 2] = mb;         // word (it * 4 + wave) of the block: samples in linear order
            words[(it * (DRAW_THREADS / kWave) + wave) * 2 + 1] = mf;
        }
        acc += ((u64)__popcll(mb) << 32) | (u64)__popcll(mf);             // at most 4096 per field in a workgroup: no field carries
    }
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) G.blk[(size_t)p * G.nblk + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// pass 2: workgroup = one problem: the exclusive scan of its block counts in place (both fields at once: a list is shorter than 2^31),
// the totals, the counts
__global__ __launch_bounds__(1024) void tsdf_draw_scan_kernel(DrawArgs G) {
    const int p = blockIdx.x;
    const u64 total = scan_top_block<u64>(G.blk + (size_t)p * G.nblk, G.nblk);
    if (threadIdx.x == 1023) {
        G.totals[p] = total;
        const long long band = (long long)(total >> 32), free_ = (long long)(total & 0xFFFFFFFFull);
        long long* cnt = G.counts + (size_t)p * DRAW_FIELDS;
        cnt[DRAW_ELIGIBLE] = band + free_, cnt[DRAW_BAND] = band, cnt[DRAW_FREE] = free_;
    }
}

// pass 3: one thread per column of problem blockIdx.y
__global__ __launch_bounds__(256) void tsdf_draw_resolve_kernel(DrawArgs G) {
    const long long N = G.n_band + G.n_free;
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c >= N) return;
    const int p = blockIdx.y;
    const u64 total = G.totals[p];
    long long j;
    const int kind = draw_column_kind(c, G.n_band, &j);
    const int shift = kind == FIT_BAND ? 32 : 0;
    const long long L = (long long)((total >> shift) & 0xFFFFFFFFull);
    const long long T = draw_take(L, kind == FIT_BAND ? G.n_band : G.n_free);
    long long index = -1;
    int s = 0, n = 0;
    if (j < T) {
        const long long rank = draw_rank(draw_key(G.seeds[p], kind), j, L, T);
        const u64* __restrict__ blk = G.blk + (size_t)p * G.nblk;
        int lo = 0, hi = G.nblk - 1;                                      // the last block whose prefix is <= rank: it holds the rank (rank < L)
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if ((long long)((blk[mid] >> shift) & 0xFFFFFFFFull) <= rank) lo = mid;
            else hi = mid - 1;
        }
        int r = (int)(rank - (long long)((blk[lo] >> shift) & 0xFFFFFFFFull));
        const u64* __restrict__ words = G.masks + ((size_t)p * G.nblk + lo) * (DRAW_BLOCK_WORDS * 2) + (kind == FIT_FREE ? 1 : 0);
        int w = 0;
        u64 bits = 0;
        for (; w < DRAW_BLOCK_WORDS; ++w) {
            bits = words[2 * w];
            const int have = __popcll(bits);
            if (r < have) break;
            r -= have;
        }
        if (w < DRAW_BLOCK_WORDS) {                                       // always: the block's count says so
            for (int i = 0; i < r; ++i) bits &= bits - 1;                 // drop the r lowest set bits
            const long long at = (long long)lo * DRAW_BLOCK + (long long)w * DRAW_WORD + (long long)(__ffsll((unsigned long long)bits) - 1);
            if (at < G.voxels) {
                index = at;
                s = G.sum[(size_t)p * G.voxels + at];
                n = G.n[(size_t)p * G.voxels + at];
            }
        }
    }
    const double* grid = G.grids + (size_t)p * DRAW_GRID_WORDS;
    float point[3];
    double target;
    unsigned char kd;
    int idx;
    draw_column(index, s, n, G.min_obs, G.dims, grid, grid[3], grid[4], point, &target, &kd, &idx);
    const size_t o = (size_t)p * (size_t)N + (size_t)c;
    for (int a = 0; a < 3; ++a) G.points[o * 3 + a] = point[a];
    G.target[o] = target;
    G.kind[o] = kd;
    G.index[o] = idx;
}

// the sum of a chunk, one value per thread: the fixed tree inside each wave, then the fixed tree over the four waves -> every thread.
// Every thread of the workgroup calls it.  The tree of tsdficp.hip.
__device__ __forceinline__ double chunk_tree(double (&wave_part)[SAMPLE_CHUNK / kWave], double v) {
    const double s = gn::wave_tree_f64(v);
    __syncthreads();                                                      // the previous use of wave_part has been read
    if ((threadIdx.x & (kWave - 1)) == 0) wave_part[threadIdx.x / kWave] = s;
    __syncthreads();
    return (wave_part[0] + wave_part[1]) + (wave_part[2] + wave_part[3]);
}

struct LossArgs {
    const float* sdf;              // [P,N]
    const float* s;                // [P]
    const double* trunc;           // [P]
    const double* target;          // [P,N]
    const unsigned char* kind;     // [P,N]
    int N;
    double* loss;                  // [P]
    float* grad;                   // [P,N]
    double* min_loss;              // [P] or null
    int* improved;                 // [P] or null
};

// workgroup = chunk blockIdx.x of problem blockIdx.y
__global__ __launch_bounds__(SAMPLE_CHUNK) void tsdf_fit_loss_kernel(LossArgs A) {
    __shared__ double wave_part[SAMPLE_CHUNK / kWave];
    __shared__ int wave_cnt[SAMPLE_CHUNK / kWave];
    const int p = blockIdx.y;
    const size_t row = (size_t)p * (size_t)A.N;
    const unsigned char* __restrict__ kind = A.kind + row;
    int mine = 0;
    for (int i = threadIdx.x; i < A.N; i += SAMPLE_CHUNK) mine += kind[i] != FIT_PAD;
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) mine += __shfl_xor(mine, o, kWave);
    if ((threadIdx.x & (kWave - 1)) == 0) wave_cnt[threadIdx.x / kWave] = mine;
    __syncthreads();
    const long long m = (long long)wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
    const float s = A.s[p];
    const double trunc = A.trunc[p];
    const int i = blockIdx.x * SAMPLE_CHUNK + threadIdx.x;
    if (i < A.N) A.grad[row + i] = fit_grad(fit_error(kind[i], A.sdf[row + i], s, trunc, A.target[row + i]), m);
    if (blockIdx.x != 0) return;                                          // the whole workgroup
    double total = 0.0;
    for (int c0 = 0; c0 < A.N; c0 += SAMPLE_CHUNK) {                      // the chunk records in chunk order, from 0.0
        const int q = c0 + threadIdx.x;
        const double e = q < A.N ? fit_error(kind[q], A.sdf[row + q], s, trunc, A.target[row + q]) : 0.0;
        total += chunk_tree(wave_part, e * e);
    }
    if (threadIdx.x == 0) {
        const double l = fit_loss(total, m);
        A.loss[p] = l;
        if (A.min_loss && l < A.min_loss[p]) {
            A.min_loss[p] = l;
            if (A.improved) A.improved[p] = 1;
        }
    }
}

}  // namespace tfk
}  // namespace ls

using namespace ls;
using namespace ls::tfk;

namespace {
struct Ws {
    u64* words;           // the seeds [P], then the grids [P,5] as float64
    u64* blk;
    u64* totals;
    u64* masks;
    int nblk;
    size_t bytes;
};

// the one layout: the pieces of tsdffit_plan.h from one Arena (ws null: a sizing pass)
Ws layout(void* ws, int P, int nx, int ny, int nz) {
    const DrawPieces c = draw_pieces(P, nx, ny, nz);
    Arena ar(ws);
    Ws w;
    w.words = ar.take<u64>(c.words);
    w.blk = ar.take<u64>(c.blocks);
    w.totals = ar.take<u64>(c.totals);
    w.masks = ar.take<u64>(c.masks);
    w.nblk = (int)c.nblk;
    w.bytes = ar.bytes();
    return w;
}

size_t workspace_need(int P, int nx, int ny, int nz) {
    if (!fp::fuse_sizes_ok(P, nx, ny, nz) || draw_bad_sizes(P, nx, ny, nz, 1, 0) != 0) return 0;
    return layout(nullptr, P, nx, ny, nz).bytes;
}

#define LS_FIT_PASS(name)                                                                                    \
    do {                                                                                                     \
        hipError_t _e = hipGetLastError();                                                                   \
        if (_e != hipSuccess) {                                                                              \
            ls::set_error("%s: the %s pass failed to launch: %s (%s:%d)", op, name, hipGetErrorString(_e), __FILE__, __LINE__); \
            return LS_ERR_HIP;                                                                               \
        }                                                                                                    \
    } while (0)

// everything the host decides, then the copy of the host arrays and the passes
int draw_run(const char* op, int P, const int32_t* sum, const int32_t* n, int nx, int ny, int nz, int min_obs, const double* origin, const double* voxel,
             const double* trunc, long long n_band, long long n_free, const unsigned long long* seeds, float* points, double* target, uint8_t* kind,
             int32_t* index, long long* counts, void* workspace, size_t workspace_bytes, hipStream_t st) {
    LS_REQUIRE(P >= 1, "%s: P must be at least 1, got %d", op, P);
    LS_REQUIRE(nx >= 1 && ny >= 1 && nz >= 1, "%s: dims must be at least 1, got %d x %d x %d", op, nx, ny, nz);
    LS_REQUIRE(fp::fuse_sizes_ok(P, nx, ny, nz), "%s: P * nx * ny * nz = %d * %d * %d * %d reaches 2^31 (int32 state indices)", op, P, nx, ny, nz);
    const int bad = draw_bad_sizes(P, nx, ny, nz, n_band, n_free);
    LS_REQUIRE(bad != 1, "%s: nx * ny * nz = %d * %d * %d exceeds %d blocks of %d samples (the scan of a problem's block counts is one workgroup)", op,
               nx, ny, nz, DRAW_MAX_BLOCKS, DRAW_BLOCK);
    LS_REQUIRE(min_obs >= 1, "%s: min_obs must be >= 1 (a sample never observed has no distance), got %d", op, min_obs);
    LS_REQUIRE(bad != 2, "%s: negative quota (n_band = %lld, n_free = %lld)", op, n_band, n_free);
    LS_REQUIRE(bad != 3, "%s: n_band + n_free must be at least 1 (no column to draw)", op);
    LS_REQUIRE(bad != 4, "%s: P * (n_band + n_free) = %d * (%lld + %lld) reaches 2^31 (int column indices)", op, P, n_band, n_free);
    LS_REQUIRE(bad != 5, "%s: P = %d outside 1..%d", op, P, DRAW_MAX_BATCH);
    LS_REQUIRE(sum && n, "%s: null sum / n", op);
    LS_REQUIRE(origin && voxel && trunc, "%s: null origin / voxel / trunc", op);
    LS_REQUIRE(seeds, "%s: null seeds", op);
    LS_REQUIRE(points && target && kind && index, "%s: null points / target / kind / index", op);
    LS_REQUIRE(counts, "%s: null counts", op);
    std::vector<long long> host((size_t)P * (1 + DRAW_GRID_WORDS));
    double* grids = (double*)(host.data() + P);                              // 8-byte words both
    for (int p = 0; p < P; ++p) {
        const int g = fp::fuse_bad_grid(origin + (size_t)p * 3, voxel[p], trunc[p]);
        LS_REQUIRE(g != 1, "%s: problem %d: origin must be finite, got (%g, %g, %g)", op, p, origin[p * 3], origin[p * 3 + 1], origin[p * 3 + 2]);
        LS_REQUIRE(g != 2, "%s: problem %d: voxel must be finite and > 0, got %g", op, p, voxel[p]);
        LS_REQUIRE(g != 3, "%s: problem %d: trunc must be finite and > 0, got %g", op, p, trunc[p]);
        host[p] = (long long)seeds[p];
        double* gr = grids + (size_t)p * DRAW_GRID_WORDS;
        for (int a = 0; a < 3; ++a) gr[a] = origin[(size_t)p * 3 + a];
        gr[3] = voxel[p], gr[4] = trunc[p];
    }
    const size_t need = workspace_need(P, nx, ny, nz);
    if (!(workspace && workspace_bytes >= need)) {
        set_error("%s: workspace %zu < required %zu (ls_%s_workspace_bytes)", op, workspace ? workspace_bytes : (size_t)0, need, op);
        return LS_ERR_WORKSPACE;
    }
    const Ws w = layout(workspace, P, nx, ny, nz);
    int rc = upload_offsets((long long*)w.words, host, st);
    if (rc != LS_OK) return rc;
    DrawArgs G{};
    G.sum = sum, G.n = n;
    G.dims[0] = nx, G.dims[1] = ny, G.dims[2] = nz;
    G.voxels = (long long)nx * ny * nz;
    G.min_obs = min_obs, G.nblk = w.nblk;
    G.n_band = n_band, G.n_free = n_free;
    G.seeds = w.words;
    G.grids = (const double*)(w.words + P);
    G.blk = w.blk, G.totals = w.totals, G.masks = w.masks;
    G.points = points, G.target = target, G.kind = kind, G.index = index, G.counts = counts;
    hipLaunchKernelGGL(tsdf_draw_classify_kernel, dim3((unsigned)w.nblk, (unsigned)P), dim3(DRAW_THREADS), 0, st, G);
    LS_FIT_PASS("classify");
    hipLaunchKernelGGL(tsdf_draw_scan_kernel, dim3((unsigned)P), dim3(1024), 0, st, G);
    LS_FIT_PASS("scan");
    hipLaunchKernelGGL(tsdf_draw_resolve_kernel, dim3((unsigned)cdiv(n_band + n_free, 256), (unsigned)P), dim3(256), 0, st, G);
    LS_FIT_PASS("resolve");
    return LS_OK;
}
}  // namespace

extern "C" {

size_t ls_tsdf_draw_workspace_bytes(int nx, int ny, int nz) { return workspace_need(1, nx, ny, nz); }
size_t ls_tsdf_draw_batch_workspace_bytes(int P, int nx, int ny, int nz) { return workspace_need(P, nx, ny, nz); }

int ls_tsdf_draw_f32(const int32_t* sum, const int32_t* n, int nx, int ny, int nz, int min_obs, const double* origin, double voxel, double trunc,
                     long long n_band, long long n_free, unsigned long long seed, float* points, double* target, uint8_t* kind, int32_t* index, long long* counts,
                     void* workspace, size_t workspace_bytes, void* stream) {
    return draw_run("tsdf_draw", 1, sum, n, nx, ny, nz, min_obs, origin, &voxel, &trunc, n_band, n_free, &seed, points, target, kind, index, counts,
                    workspace, workspace_bytes, (hipStream_t)stream);
}

int ls_tsdf_draw_batch_f32(int P, const int32_t* sum, const int32_t* n, int nx, int ny, int nz, int min_obs, const double* origin, const double* voxel,
                           const double* trunc, long long n_band, long long n_free, const unsigned long long* seeds, float* points, double* target, uint8_t* kind,
                           int32_t* index, long long* counts, void* workspace, size_t workspace_bytes, void* stream) {
    return draw_run("tsdf_draw_batch", P, sum, n, nx, ny, nz, min_obs, origin, voxel, trunc, n_band, n_free, seeds, points, target, kind, index, counts,
                    workspace, workspace_bytes, (hipStream_t)stream);
}

int ls_tsdf_fit_loss_f64(const float* sdf, const float* s, const double* trunc, const double* target, const uint8_t* kind, int P, int N, double* loss,
                         float* grad, double* min_loss, int32_t* improved, void* stream) {
    const char* op = "tsdf_fit_loss";
    LS_REQUIRE(P >= 1 && N >= 1, "%s: P and N must be at least 1, got P = %d, N = %d", op, P, N);
    LS_REQUIRE((long long)P * (long long)N < (1ll << 31), "%s: P * N = %d * %d reaches 2^31 (int column indices)", op, P, N);
    LS_REQUIRE(P <= DRAW_MAX_BATCH, "%s: P = %d outside 1..%d", op, P, DRAW_MAX_BATCH);
    LS_REQUIRE(sdf && s && trunc && target && kind, "%s: null sdf / s / trunc / target / kind", op);
    LS_REQUIRE(loss && grad, "%s: null loss / grad", op);
    LossArgs A{sdf, s, trunc, target, kind, N, loss, grad, min_loss, improved};
    hipLaunchKernelGGL(tsdf_fit_loss_kernel, dim3((unsigned)cdiv(N, SAMPLE_CHUNK), (unsigned)P), dim3(SAMPLE_CHUNK), 0, (hipStream_t)stream, A);
    LS_FIT_PASS("loss");
    return LS_OK;
}

}  // extern "C"
