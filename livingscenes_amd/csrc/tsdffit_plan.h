// tsdffit_plan.h -- the fused state of the scene memory (depthfuse.hip: sum, n) as a TRAINING SIGNAL for the latent codes, the one
// statement of it: the kind of a lattice sample (band / observed free space), the deterministic stratified draw of a fixed number of
// samples of each kind, what a drawn column holds, the error and the gradient of the fit loss, what a call accepts and the pieces of the
// workspace.  Pure functions: no HIP, no global state.  The kernels of tsdffit.hip are loops around draw_kind, draw_rank, draw_column and
// fit_error; a plain C++17 compiler accepts the file, and tests/test_tsdf_fit_cpu.py replays it (tests/tools/tsdffit_plan_run.cpp)
// against the NumPy twin of the definition (tests/tsdf_fit_oracle.py; the definition itself: include/livingscenes_hip.h,
// ls_tsdf_draw_f32 / ls_tsdf_fit_loss_f64).  Everything is integer or float64 and no a * b + c is contracted into an fma: clang is told
// here, any other compiler by -ffp-contract=off.
//
// THIS BUILD'S DEFINITION, pinned by no test of the reference: the decoder's value times the instance's scale s is a metric distance.
// It follows the reference's training loss, which compares the decoder's output with distances in the normalised frame; so a metric
// target enters the loss as target / s, and the reference's point loss MSE(sdf, 0) is the special case target = 0.
#pragma once
#include <cmath>
#include <cstddef>

#include "tsdfsample_plan.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace ls {
namespace tf {

using cp::finite64;
typedef unsigned long long u64;

enum { FIT_PAD = 0, FIT_BAND, FIT_FREE, FIT_KINDS };                      // the kind of a column, by value; 0 also: a sample not eligible
enum { DRAW_ELIGIBLE = 0, DRAW_BAND, DRAW_FREE, DRAW_FIELDS };            // counts[p]
constexpr int DRAW_THREADS = 256;         // threads of a classify workgroup
constexpr int DRAW_WORD = 64;             // samples per mask word: one ballot of a wave, bit l = the l-th sample of the word
constexpr int DRAW_BLOCK_WORDS = 64;      // mask words per block
constexpr int DRAW_BLOCK = DRAW_WORD * DRAW_BLOCK_WORDS;   // 4096 consecutive samples of ONE problem per classify workgroup: a block
constexpr int DRAW_MAX_BLOCKS = 4096;     // blocks per problem: the top-level scan of ls_scan.h (SCAN_MAX_BLOCKS), so nx ny nz <= 2^24
constexpr int DRAW_MAX_BATCH = 65535;    // problems per call: the problem is blockIdx.y
constexpr int DRAW_GRID_WORDS = 5;        // origin[3], voxel, trunc of one problem
constexpr u64 DRAW_GOLDEN = 0x9E3779B97F4A7C15ull;

// the finaliser of splitmix64: the text of mix64 (ls_common.h), which a header without HIP cannot include
LS_CP_HD u64 draw_mix64(u64 z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// Eligible iff n >= min_obs.  FREE iff sum == n * FUSE_SCALE: every view that looked saw the sample at or beyond +trunc (the projective
// distance is clamped on that side only).  Every other eligible sample is BAND: fuse_distance never records less than -1 (an occluded
// sample is skipped), so D = -1 is an exact value.  Integer comparisons only.
LS_CP_HD int draw_kind(int sum, int n, int min_obs) {
    if (n < min_obs) return FIT_PAD;
    return (long long)sum == (long long)n * (long long)fp::FUSE_SCALE ? FIT_FREE : FIT_BAND;
}

// the stream of one (problem, kind): key = mix64(seed + kind * golden), r_j = the top 32 bits of mix64(key + (j + 1) * golden)
LS_CP_HD u64 draw_key(u64 seed, int kind) { return draw_mix64(seed + (u64)kind * DRAW_GOLDEN); }
LS_CP_HD u64 draw_uniform32(u64 key, long long j) { return draw_mix64(key + ((u64)j + 1ull) * DRAW_GOLDEN) >> 32; }

// a quota m out of a list of length L takes T = min(L, m), one per stratum
LS_CP_HD long long draw_take(long long L, long long m) { return L < m ? L : m; }

// The list rank stratum j < T of a list of length L < 2^31 takes: stratum j is the ranks [floor(j L / T), floor((j + 1) L / T)), of
// width w >= 1; the rank is its first plus (r_j * w) >> 32.  64-bit unsigned arithmetic: j L < 2^62, r_j w < 2^63.  The ranks are
// distinct and ascending, and with T = L every stratum has width 1: the whole list.
LS_CP_HD long long draw_rank(u64 key, long long j, long long L, long long T) {
    const u64 lo = ((u64)j * (u64)L) / (u64)T, hi = (((u64)j + 1ull) * (u64)L) / (u64)T;
    return (long long)(lo + ((draw_uniform32(key, j) * (hi - lo)) >> 32));
}

// where column c of [0, n_band + n_free) stands: its kind and its stratum
LS_CP_HD int draw_column_kind(long long c, long long n_band, long long* j) {
    *j = c < n_band ? c : c - n_band;
    return c < n_band ? FIT_BAND : FIT_FREE;
}

// What a column holds.  index >= 0: the lattice sample with that linear index (k fastest) and state (sum, n), which is eligible:
// the float64 fuse_position of each axis rounded once to fp32, target = trunc * fuse_value(sum, n) in metres, its kind.  index < 0: a
// PAD -- the position of lattice sample 0, target 0, index -1.
LS_CP_HD void draw_column(long long index, int sum, int n, int min_obs, const int (&dims)[3], const double* origin, double voxel, double trunc,
                          float (&point)[3], double* target, unsigned char* kind, int* index_out) {
    int ijk[3] = {0, 0, 0};
    *target = 0.0, *kind = (unsigned char)FIT_PAD, *index_out = -1;
    if (index >= 0) {
        ijk[2] = (int)(index % dims[2]);
        ijk[1] = (int)((index / dims[2]) % dims[1]);
        ijk[0] = (int)((index / dims[2]) / dims[1]);
        bool valid;
        *target = trunc * fp::fuse_value(sum, n, min_obs, &valid);
        *kind = (unsigned char)draw_kind(sum, n, min_obs);
        *index_out = (int)index;
    }
    for (int a = 0; a < 3; ++a) point[a] = (float)fp::fuse_position(origin[a], voxel, ijk[a]);
}

// The error of one column in the decoder's units, u = (double)sdf: BAND e = u - target / s; FREE e = min(u - trunc / s, 0) -- a
// one-sided hinge: observed free space only says "at least trunc in front of every surface that saw it"; PAD e = 0.  No weight between
// the kinds (the quotas set the balance), no clamp of the band error, and s is not optimised.
LS_CP_HD double fit_error(int kind, float sdf, float s, double trunc, double target) {
    const double u = (double)sdf;
    if (kind == FIT_BAND) return u - target / (double)s;
    if (kind == FIT_FREE) {
        const double e = u - trunc / (double)s;
        return e < 0.0 ? e : 0.0;
    }
    return 0.0;
}

// grad = (float)(2 e / m) over the m non-PAD columns of the problem, 0 where m = 0; loss = (sum of e^2 by the chunk rule) / m, 0.0 where m = 0
LS_CP_HD float fit_grad(double e, long long m) { return m > 0 ? (float)(2.0 * e / (double)m) : 0.0f; }
LS_CP_HD double fit_loss(double sum_e2, long long m) { return m > 0 ? sum_e2 / (double)m : 0.0; }

LS_CP_HD long long draw_blocks(long long voxels) { return (voxels + DRAW_BLOCK - 1) / DRAW_BLOCK; }

// the sizes a draw accepts beyond fuse_sizes_ok -> 0, or 1: nx ny nz above DRAW_MAX_BLOCKS blocks of DRAW_BLOCK samples (the scan of
// a problem's block counts is one workgroup of ls_scan.h), 2: a negative quota, 3: no column, 4: P (n_band + n_free) reaches 2^31,
// 5: P above DRAW_MAX_BATCH
LS_CP_HD int draw_bad_sizes(int P, int nx, int ny, int nz, long long n_band, long long n_free) {
    if (draw_blocks((long long)nx * ny * nz) > DRAW_MAX_BLOCKS) return 1;
    if (n_band < 0 || n_free < 0) return 2;
    if (n_band + n_free < 1) return 3;
    const long long lim = 1ll << 31;
    if (n_band >= lim || n_free >= lim || (n_band + n_free) * (long long)P >= lim) return 4;
    if (P > DRAW_MAX_BATCH) return 5;
    return 0;
}

// The pieces of the workspace.  words: the P seeds as uint64, then P grids of DRAW_GRID_WORDS float64 -- one upload; per block of a
// problem one packed count (band << 32 | free), scanned in place, and per problem the packed total; per 64 samples two mask words
// (band, free): 1/4 byte per sample.  No compact list is materialised.
struct DrawPieces { size_t words, blocks, totals, masks; long long nblk; };
LS_CP_HD DrawPieces draw_pieces(int P, int nx, int ny, int nz) {
    DrawPieces c;
    c.nblk = draw_blocks((long long)nx * ny * nz);
    c.words = (size_t)P * (1 + DRAW_GRID_WORDS);
    c.blocks = (size_t)P * (size_t)c.nblk;
    c.totals = (size_t)P;
    c.masks = c.blocks * DRAW_BLOCK_WORDS * 2;
    return c;
}

}  // namespace tf
}  // namespace ls
