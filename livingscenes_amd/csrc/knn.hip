// knn.hip -- feature-space K-nearest-neighbour graph build (K <= 16), bit-exact w.r.t. oracle/ls_oracle.c.
//
// Replaces pytorch3d.ops.knn_points as called at
//   /root/reference/lib_shape_prior/core/lib/vec_sim3/vec_dgcnn_atten.py:139-141
//
// Data layout (HBM): features [B, N, 3, C] fp32 ("x-major rows").  Canonical distance
//   d(q,s) = sum_{c=0..C-1} sum_{x=0..2} (q[x][c]-s[x][c])^2   accumulated sequentially in that order
// (the reference flattens [B,C,3,N] -> [B,3C,N], so j = c*3+x), each term rounded per the FMA flag.
//
// This file: the all-VALU tile kernel (knn_kernel + knn_merge_kernel) and the family's host side: knn_dispatch = check, traits, plan, knn_run.  WHICH kernel
// of this file, knn_mfma.hip or knn_xyz.hip runs, on what grid and with how many candidate splits, is decided in knn_plan.h and nowhere else.
// Kernel shape (wave64, 256 threads = 4 waves per workgroup):
//   * a workgroup owns 64 queries of one instance and streams the instance's candidates in tiles of 64;
//   * both tiles are staged through LDS in channel chunks of CC (32 channels = 96 dims), rows padded to
//     100 floats so the 16-lane groups of ds_read_b128 hit 16 distinct 16-B bank slots (row stride/4 odd);
//   * each thread owns a 4x4 (query x candidate) register micro-tile: 24 ds_read_b128 feed 192 pair-dims;
//   * the 64x64 distance tile goes back to LDS and each wave merges 16 query rows into per-query sorted
//     top-K lists that live in the 16 lanes of a DPP row (4 queries per VGPR pair): every lane filters 4
//     candidates against its row's K-th entry under the lexicographic (dist, idx) order; survivors are
//     inserted one per row per step with two ballots + one DPP row_shr:1 -- four queries advance per wave
//     instruction, no LDS traffic besides the tile read, no divergence beyond a wave-uniform loop.
//   * blockIdx is remapped so that the tiles of one instance run on one XCD and share its L2.
// Roofline: VALU-bound (3 VALU ops per pair-dim without FMA, 2 with): algorithmic bytes per instance-layer
// are (Nd+Ns)*3C*4 + Nd*K*4, three orders of magnitude below the VALU time.
#include "knn_common.h"
#include "ls_launch.h"

namespace ls {

// CC = channels per LDS chunk (32)
template <int CC, bool FMA>
__global__ __launch_bounds__(256, 3) void knn_kernel(const float* __restrict__ dstf, const float* __restrict__ srcf,
                                                  const int32_t* __restrict__ dst_rows, int Nd, int dst_n, int Ns, int C,
                                                  int K, int32_t* __restrict__ idx_out, float* __restrict__ dist_out,
                                                  int qtiles, int splits, int tiles_per_split, u64* __restrict__ partial,
                                                  const int32_t* __restrict__ seed_idx, int seed_n, int seed_by_row) {
    constexpr int ROW = 3 * CC + 4;       // floats per staged row (ROW/4 odd: conflict-free ds_read_b128)
    constexpr int PR = 2 * 3 * CC + 4;    // floats per candidate-PAIR row (PR/4 odd)
    constexpr int LC_FLOATS = KNN_TS * ROW;
    static_assert(LC_FLOATS >= KNN_TQ * KNN_LD && LC_FLOATS >= KNN_TS / 2 * PR, "the candidate chunk's LDS also holds the distance tile");
    __shared__ __attribute__((aligned(16))) float lq[KNN_TQ * ROW];
    __shared__ __attribute__((aligned(16))) float lc[LC_FLOATS];   // candidate chunk; re-used as the 64x64 distance tile
    __shared__ int lqrow[KNN_TQ];
    float* ldist = lc;

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int logical = xcd_remap(blockIdx.x, gridDim.x);
    const int sp = logical % splits;                 // candidate range of this workgroup (split-S for under-filled grids)
    const int b = (logical / splits) / qtiles, qt = (logical / splits) % qtiles;
    const int q0 = qt * KNN_TQ;
    const int s_begin = sp * tiles_per_split * KNN_TS;
    const int s_end = min(Ns, s_begin + tiles_per_split * KNN_TS);
    const size_t row_f = (size_t)3 * C;
    const float* dbase = dstf + (size_t)b * dst_n * row_f;
    const float* sbase = srcf + (size_t)b * Ns * row_f;

    if (tid < KNN_TQ) {
        int q = q0 + tid;
        int r = -1;
        if (q < Nd) r = dst_rows ? dst_rows[(size_t)b * Nd + q] : q;
        lqrow[tid] = r;
    }
    __syncthreads();

    const int tx = tid & 15, ty = tid >> 4;  // candidates tx+16j, queries ty*4+i

    // per-wave top-K lists: group g, row r = lane>>4 -> query wave*16 + g*4 + r, entry e = lane&15 of its sorted key
    // list; rkey = the row's current K-th key replicated over the row (the admission threshold); ~0 = empty slot
    u64 lk[4], rkey[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { lk[i] = ~0ull; rkey[i] = ~0ull; }

    const int nchunks = C / CC;
    const bool q_once = nchunks == 1;  // single chunk: the query tile is loop invariant, stage it once

    Stager<CC> sq, sc;  // register staging buffers (next chunk in flight under the current compute)
    sq.load(dbase, lqrow, 0, 0, row_f, C, 0, tid);
    sc.load(sbase, nullptr, s_begin, Ns, row_f, C, 0, tid);
    if (q_once) { sq.store(lq, ROW, tid); }
    // optional hints (e.g. the previous layer's neighbour list of the same point): start the lists from their exact
    // canonical distances so that the admission threshold is near-final from the first tile.  Only split 0 is seeded (the
    // merge kernel drops duplicates); the result does not depend on the hints.
    const bool seeded = seed_idx != nullptr && sp == 0;
    if (seeded) {
        u64* lseed = reinterpret_cast<u64*>(lc);  // 8 KB, lc is not in use before the first tile is stored
        compute_seed_keys<FMA>(lseed, seed_idx, seed_n, seed_by_row != 0, dbase, sbase, lqrow, b, q0, Ns, C, tid);
        __syncthreads();
        seed_lists(lseed, lk, rkey, K, wave, lane);
    }

    for (int s0 = s_begin; s0 < s_end; s0 += KNN_TS) {
        f32x2_t acc2[4][2];     // [query][candidate pair] x (even, odd candidate)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc2[i][j] = f32x2_t{0.0f, 0.0f};

        for (int ch = 0; ch < nchunks; ++ch) {
            __syncthreads();  // previous chunk's compute / previous tile's selection done with lq, lc
            if (!q_once) sq.store(lq, ROW, tid);
            sc.store_pairs(lc, PR, tid);
            __syncthreads();
            // prefetch the next chunk (or the next tile's first chunk) into registers
            {
                int nch = ch + 1, ns0 = s0;
                if (nch == nchunks) { nch = 0; ns0 = s0 + KNN_TS; }
                if (ns0 < s_end) {
                    if (!q_once) sq.load(dbase, lqrow, 0, 0, row_f, C, nch * CC, tid);
                    sc.load(sbase, nullptr, ns0, Ns, row_f, C, nch * CC, tid);
                }
            }
#pragma unroll 1
            for (int d4 = 0; d4 < 3 * CC; d4 += 4) {
                float4 qv[4];
                f32x2_t cp[2][4];  // [candidate pair][dim] = (c_{2pm}.d, c_{2pm+1}.d)
#pragma unroll
                for (int i = 0; i < 4; ++i) qv[i] = *reinterpret_cast<const float4*>(&lq[(ty * 4 + i) * ROW + d4]);
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) {
                    const float4 lo = *reinterpret_cast<const float4*>(&lc[(tx + 16 * jj) * PR + d4 * 2]);
                    const float4 hi = *reinterpret_cast<const float4*>(&lc[(tx + 16 * jj) * PR + d4 * 2 + 4]);
                    cp[jj][0] = f32x2_t{lo.x, lo.y}; cp[jj][1] = f32x2_t{lo.z, lo.w};
                    cp[jj][2] = f32x2_t{hi.x, hi.y}; cp[jj][3] = f32x2_t{hi.z, hi.w};
                }
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int jj = 0; jj < 2; ++jj) {
                        f32x2_t a = acc2[i][jj];  // canonical order j = c*3+x == LDS dim order
                        a = accq2<FMA>(a, qv[i].x, cp[jj][0]); a = accq2<FMA>(a, qv[i].y, cp[jj][1]);
                        a = accq2<FMA>(a, qv[i].z, cp[jj][2]); a = accq2<FMA>(a, qv[i].w, cp[jj][3]);
                        acc2[i][jj] = a;
                    }
            }
        }
        __syncthreads();  // everyone is done reading lc before it becomes the distance tile
        // distance tile -> LDS, candidate c of a query row stored at slot (c & 15) * 4 + (c >> 4) (what a selection lane
        // reads with one ds_read_b128).  A thread owns candidates c = 2*tx + 32*jj + h (pair-interleaved).
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) {
                const int c0 = 2 * tx + 32 * jj;
                ldist[(ty * 4 + i) * KNN_LD + (c0 & 15) * 4 + (c0 >> 4)] = acc2[i][jj].x;
                ldist[(ty * 4 + i) * KNN_LD + ((c0 + 1) & 15) * 4 + ((c0 + 1) >> 4)] = acc2[i][jj].y;
            }
        __syncthreads();

        if (seeded) select_tile<true>(ldist, lk, rkey, s0, Ns, K, wave, lane);
        else select_tile<false>(ldist, lk, rkey, s0, Ns, K, wave, lane);
    }
    write_lists(lk, b, q0, Nd, K, wave, lane, splits, sp, partial, idx_out, dist_out);
}

// merge the per-split sorted key lists of every query: one 16-lane row per query, same insertion step as above
__global__ __launch_bounds__(256) void knn_merge_kernel(const u64* __restrict__ partial, int total_q, int splits, int K,
                                                        int32_t* __restrict__ idx_out, float* __restrict__ dist_out) {
    const int lane = threadIdx.x & 63, e16 = lane & 15, rowbase = lane & 48;
    const int q = (blockIdx.x * 256 + threadIdx.x) >> 4;
    const bool live = q < total_q;
    const u64* pq = partial + (size_t)(live ? q : 0) * splits * 16;
    u64 lkey = live ? pq[e16] : ~0ull;                       // split 0 is already sorted
    u64 kk = bperm64(rowbase + K - 1, lkey);
    for (int s = 1; s < splits; ++s)   // (DEDUP: the seeded split 0 may already hold a candidate of another split's range)
        merge_keys<true>(live ? pq[s * 16 + e16] : ~0ull, ~0ull, ~0ull, ~0ull, lkey, kk, K, lane);
    if (live && e16 < K) {
        const size_t o = (size_t)q * K + e16;
        const unsigned hi = (unsigned)(lkey >> 32), lo = (unsigned)lkey;
        idx_out[o] = hi == 0xFFFFFFFFu ? -1 : (int)lo;
        if (dist_out) dist_out[o] = hi == 0xFFFFFFFFu ? INFINITY : __uint_as_float(hi);
    }
}

// TILE: the tile kernel on the plan's grid, then the merge over the splits' lists
static int knn_tile_run(const Knn& k, const KnnPlan& p, hipStream_t st) {
    hipLaunchKernelGGL((k.fma ? knn_kernel<32, true> : knn_kernel<32, false>), dim3(p.grid), dim3(p.block), 0, st, k.dst, k.src, k.dst_rows, k.Nd, k.dst_n, k.Ns, k.C,
                       k.K, k.idx_out, k.dist_out, p.qtiles, p.splits, p.tiles_per_split, (u64*)k.scratch, k.seed_idx, k.seed_n, k.seed_by_row);
    LS_LAUNCH_CHECK();
    if (p.merge_grid) {
        hipLaunchKernelGGL(knn_merge_kernel, dim3(p.merge_grid), dim3(256), 0, st, (const u64*)k.scratch, k.B * k.Nd, p.splits, k.K, k.idx_out, k.dist_out);
        LS_LAUNCH_CHECK();
    }
    return LS_OK;
}

// launch what the plan names
static int knn_run(const KnnPlan& p, const Knn& k, hipStream_t st) {
    switch (p.kernel) {
    case KnnKernel::XYZ_SINGLE: case KnnKernel::XYZ_CHUNKED: return knn_xyz_run(k, p, st);
    case KnnKernel::SMALL: return knn_small_run(k, p, st);
    case KnnKernel::TILE: return knn_tile_run(k, p, st);
    default: return knn_fused_run(k, p, st);
    }
}

size_t knn_scratch_bytes(int B, int Nd, int dst_n, int Ns, int C, unsigned flags) {
    return knn_plan(knn_traits(false, B, Nd, dst_n, Ns, C, KNN_MAXK, flags, false, true)).scratch_bytes;
}

// what the family serves: asked first by knn_dispatch, and by ls_knn_f32 in front of its workspace check (a call refused here is refused for this reason)
static int knn_check(int B, int Nd, int dst_n, int Ns, int C, int K) {
    LS_REQUIRE(B > 0 && Nd > 0 && Ns > 0 && dst_n > 0, "knn: empty problem (B=%d Nd=%d Ns=%d)", B, Nd, Ns);
    LS_REQUIRE(K >= 1 && K <= KNN_MAXK, "knn: K=%d unsupported (1..16)", K);
    LS_REQUIRE(C == 1 || C % 32 == 0, "knn: C=%d must be 1 or a multiple of 32", C);
    return LS_OK;
}

int knn_dispatch(const float* dst, const float* src, const int32_t* dst_rows, int B, int Nd, int dst_n, int Ns, int C,
                 int K, unsigned flags, int32_t* idx_out, float* dist_out, void* scratch, const int32_t* seed_idx, int seed_n,
                 int seed_by_row, hipStream_t st) {
    if (const int rc = knn_check(B, Nd, dst_n, Ns, C, K)) return rc;
    Knn k;
    k.dst = dst; k.src = src; k.dst_rows = dst_rows;
    k.B = B; k.Nd = Nd; k.dst_n = dst_n; k.Ns = Ns; k.C = C; k.K = K; k.fma = (flags & LS_FLAG_CONTRACT_FMA) != 0;
    k.idx_out = idx_out; k.dist_out = dist_out; k.scratch = scratch;
    k.seed_idx = seed_idx; k.seed_n = seed_n; k.seed_by_row = seed_by_row;
    return knn_run(knn_plan(knn_traits(dst == src, B, Nd, dst_n, Ns, C, K, flags, seed_idx != nullptr, scratch != nullptr)), k, st);
}

}  // namespace ls

using namespace ls;
extern "C" {
size_t ls_knn_workspace_bytes(int B, int Nd, int dst_n, int Ns, int C, int /*seeded*/, unsigned flags) {   // (hints never changed the size)
    if (B <= 0 || Nd <= 0 || Ns <= 0 || dst_n <= 0) return 0;
    return knn_scratch_bytes(B, Nd, dst_n, Ns, C, flags);
}
int ls_knn_f32(const float* dst, const float* src, const int32_t* dst_rows, const int32_t* seed_idx, int B, int Nd, int dst_n, int Ns,
               int C, int K, unsigned flags, int32_t* idx_out, float* dist_out, void* workspace, size_t workspace_bytes, void* stream) {
    if (const int rc = knn_check(B, Nd, dst_n, Ns, C, K)) return rc;
    const size_t sb = knn_scratch_bytes(B, Nd, dst_n, Ns, C, flags);
    if (sb > workspace_bytes || (sb && !workspace)) {
        set_error("knn: workspace %zu < required %zu (ls_knn_workspace_bytes)", workspace_bytes, sb);
        return LS_ERR_WORKSPACE;
    }
    return knn_dispatch(dst, src, dst_rows, B, Nd, dst_n, Ns, C, K, flags, idx_out, dist_out, workspace, seed_idx, Nd, 0, (hipStream_t)stream);
}
}  // extern "C"
