// tsdfprior_plan.h -- the shape prior's field as VOTES in the fused state of the scene memory (depthfuse.hip: sum, n), the one statement
// of it: the weight the prior has at a lattice sample, the query row of an eligible sample, the quantised vote of the decoder's value,
// the integer update into the completed state, what a call accepts and the pieces of the workspace.  Pure functions: no HIP, no global
// state.  The kernels of tsdfprior.hip are loops around prior_weight, prior_row and prior_vote; a plain C++17 compiler accepts the
// file, and tests/test_tsdf_prior_cpu.py replays it (tests/tools/tsdfprior_plan_run.cpp) against the NumPy twin of the definition
// (tests/tsdf_prior_oracle.py; the definition itself: include/livingscenes_hip.h, ls_tsdf_prior_rows_f32 / ls_tsdf_prior_vote_f32).
// Everything is integer or float64 and no a * b + c is contracted into an fma: clang is told here, any other compiler by
// -ffp-contract=off.
//
// THE CONVENTION OF tsdffit_plan.h HOLDS: the decoder's value times the instance's scale s is a metric distance, with the sign of the
// fused distance (positive in front of the surface).
#pragma once
#include <cmath>
#include <cstddef>

#include "fuse_plan.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace ls {
namespace tp {

using cp::finite64;
typedef unsigned long long u64;

enum { PRIOR_ELIGIBLE = 0, PRIOR_VOTED, PRIOR_SKIPPED, PRIOR_UNTOUCHED, PRIOR_FIELDS };   // counts[p]
enum { VOTE_UNTOUCHED = 0, VOTE_CAST, VOTE_SKIPPED };                     // what prior_vote did with a sample, by value
constexpr int PRIOR_THREADS = 256;        // threads of a workgroup of every pass
constexpr int PRIOR_WORD = 64;            // samples per ballot word: one ballot of a wave, bit l = the l-th sample of the word
constexpr int PRIOR_BLOCK_WORDS = 64;     // ballot words per block
constexpr int PRIOR_BLOCK = PRIOR_WORD * PRIOR_BLOCK_WORDS;   // 4096 consecutive samples of ONE problem per workgroup: a block
constexpr int PRIOR_MAX_BLOCKS = 4096;    // blocks per problem, so nx ny nz <= 2^24: the scan limit of tsdffit_plan.h
constexpr int PRIOR_MAX_BATCH = 65535;    // problems per call: the problem is blockIdx.y
constexpr int PRIOR_MAX_WEIGHT = fp::FUSE_MAX_OBS;
constexpr int PRIOR_GRID_WORDS = 6;       // origin[3], voxel, trunc, s of one problem

// step 1: the prior tops a sample up to w0 votes and fades out as observations arrive; > 0: the sample is eligible
LS_CP_HD long long prior_weight(int w0, int n) {
    const long long w = (long long)w0 - (long long)n;
    return w > 0 ? w : 0;
}

// step 2: the query row of the sample with linear index i (k fastest): the float64 fuse_position of each axis rounded once to fp32
LS_CP_HD void prior_row(long long index, const int (&dims)[3], const double* origin, double voxel, float (&point)[3]) {
    const int ijk[3] = {(int)((index / dims[2]) / dims[1]), (int)((index / dims[2]) % dims[1]), (int)(index % dims[2])};
    for (int a = 0; a < 3; ++a) point[a] = (float)fp::fuse_position(origin[a], voxel, ijk[a]);
}

// step 3, first half: d = s f as a metric distance, t = d / trunc clamped to [-1, 1], q = floor(t * 16384 + 0.5).  f is not NaN.
LS_CP_HD int prior_quantise(double s, float f, double trunc) {
    const double d = s * (double)f;
    double t = d / trunc;
    t = t < -1.0 ? -1.0 : (t > 1.0 ? 1.0 : t);
    return (int)floor(t * (double)fp::FUSE_SCALE + 0.5);
}

// steps 1, 3 and 4 for one sample: (sum, n) -> (*sum_out, *n_out); f is read only where the sample is eligible.  A NaN casts no
// vote.  The sums are formed in 64 bits: a state that honours |sum| <= n * 16384, n <= 65535 never leaves int32.
LS_CP_HD int prior_vote(int sum, int n, int w0, double s, double trunc, float f, int* sum_out, int* n_out) {
    *sum_out = sum, *n_out = n;
    const long long w = prior_weight(w0, n);
    if (w == 0) return VOTE_UNTOUCHED;
    if (f != f) return VOTE_SKIPPED;
    *sum_out = (int)((long long)sum + w * (long long)prior_quantise(s, f, trunc));
    *n_out = (int)((long long)n + w);
    return VOTE_CAST;
}

LS_CP_HD long long prior_blocks(long long voxels) { return (voxels + PRIOR_BLOCK - 1) / PRIOR_BLOCK; }

// the sizes a call accepts beyond fuse_sizes_ok -> 0, or 1: nx ny nz above PRIOR_MAX_BLOCKS blocks of PRIOR_BLOCK samples, 2: P above
// PRIOR_MAX_BATCH
LS_CP_HD int prior_bad_sizes(int P, int nx, int ny, int nz) {
    if (prior_blocks((long long)nx * ny * nz) > PRIOR_MAX_BLOCKS) return 1;
    if (P > PRIOR_MAX_BATCH) return 2;
    return 0;
}

// the scalars of a call: the prior weight in 1 .. 65535 -> 0 or 1; the scale of one problem finite and > 0 -> 0 or 1
LS_CP_HD int prior_bad_weight(int w0) { return (w0 >= 1 && w0 <= PRIOR_MAX_WEIGHT) ? 0 : 1; }
LS_CP_HD int prior_bad_scale(double s) { return (finite64(s) && s > 0.0) ? 0 : 1; }

// The pieces of the workspace, in 8-byte words.  grids: P records of PRIOR_GRID_WORDS float64 -- one upload; per block of a problem
// one count of eligible samples, ALL P nblk of them scanned in place by the one scan of a call (the rows of a batch are one packed list,
// problems in order); per 64 samples one ballot word: 1/8 byte per sample.  No compact list is materialised.
struct PriorPieces { size_t grids, blocks, masks; long long nblk; };
LS_CP_HD PriorPieces prior_pieces(int P, int nx, int ny, int nz) {
    PriorPieces c;
    c.nblk = prior_blocks((long long)nx * ny * nz);
    c.grids = (size_t)P * PRIOR_GRID_WORDS;
    c.blocks = (size_t)P * (size_t)c.nblk;
    c.masks = c.blocks * PRIOR_BLOCK_WORDS;
    return c;
}

}  // namespace tp
}  // namespace ls
