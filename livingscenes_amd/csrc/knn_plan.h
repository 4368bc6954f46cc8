// knn_plan.h -- what one k-NN build launches: which kernel of knn.hip / knn_mfma.hip / knn_xyz.hip on what grid, with which preparation and merge
// launches around it, how its scratch is laid out and how many bytes a caller has to bring.  The one statement of that choice, as a pure host
// function: no HIP, no global state.  knn_dispatch (knn.hip) builds the traits, asks here and calls knn_run, which launches what the plan names;
// the sizing query and the encoder (model.hip) read the same plan.  Every path is bit-exact against oracle/ls_oracle.c, so a changed choice shows
// only as a changed speed.  Compiles with a plain C++17 compiler: tests/test_knn_plan_cpu.py replays it against the launches recorded in
// tests/golden/knn_launches.json.
#pragma once
#include <cstddef>

namespace ls {

constexpr int KNN_MAXK = 16;
constexpr int KNN_TQ = 64, KNN_TS = 64;        // tile kernel (knn.hip): queries per workgroup, candidates per tile
constexpr int KF_QT = 32, KF_WAVES = 8;        // fused kernel (knn_mfma.hip): queries per workgroup (one 32-row MFMA operand), waves per workgroup
constexpr int KF_MAXNS = KF_WAVES * 4 * 32;    // ... its largest padded candidate set: four 32-candidate tiles per wave
constexpr int KX_CH = 1024;                    // raw-cloud kernel (knn_xyz.hip): candidates per chunk (16 per lane)
constexpr int KSM_Q = 8;                       // small kernel (knn_xyz.hip): queries per workgroup

// everything the choice depends on, and nothing else
struct KnnTraits {
    int B = 0, Nd = 0, dst_n = 0, Ns = 0, C = 0, K = 0;   // Nd queries out of a destination set of dst_n rows, Ns candidates, rows of 3 C floats
    bool fma = false;          // LS_FLAG_CONTRACT_FMA: which instantiation, never which kernel
    bool valu_only = false;    // LS_FLAG_KNN_VALU_ONLY
    bool seeded = false;       // the caller brings hints (the tile kernel starts its lists from them, the fused kernel ignores them)
    bool self = false;         // the destination set is the candidate set (dst == src)
    bool has_scratch = false;  // the caller brings scratch (of scratch_bytes)
};

// one enumerator per kernel instantiation that can be launched, FMA aside (knn_run switches on it)
enum class KnnKernel {
    XYZ_SINGLE, XYZ_CHUNKED,                  // knn_xyz_kernel<FMA, SINGLE>: raw clouds, the candidates in one chunk of KX_CH | several
    SMALL,                                    // knn_small_kernel<FMA>
    TILE,                                     // knn_kernel<32, FMA>, then knn_merge_kernel where the candidates were split
    FUSED_32_T1, FUSED_32_T2, FUSED_32_T4,    // knn_fused_kernel<CC, FMA, TPW> after knn_prep_f16_tile_kernel<6, 3> (C = 32) ...
    FUSED_64_T1, FUSED_64_T2, FUSED_64_T4     // ... or <12, 4> (C = 64) on the candidate set and (not self) on the destination set
};

// the fused kernel's scratch as byte offsets: per-query exact-phase counters (first: knn_sweep_stats_launch finds them whatever the rest looks
// like) | squared row norms (src, dst) | inverse row scales (src, dst) | f16 images (src, dst); self: the dst pieces are the src pieces
struct KnnFusedLayout { size_t cnt = 0, nsrc = 0, ndst = 0, isrc = 0, idst = 0, sq = 0, dq = 0, bytes = 0; };

struct KnnPlan {
    KnnKernel kernel = KnnKernel::TILE;
    unsigned grid = 0, block = 256;            // the main launch
    int qpw = 0, qblocks = 0;                  // raw cloud: queries per wave, query blocks per instance (small: qblocks alone)
    int qtiles = 0;                            // tile, fused: query tiles per instance
    int splits = 1, tiles_per_split = 0;       // tile: candidate ranges per query tile, candidate tiles per range
    unsigned merge_grid = 0;                   // tile: the merge launch over the ranges' lists (workgroups of 256); 0: none
    int ns_pad = 0, dst_npad = 0, tpw = 0;     // fused: the sets padded to 32 rows, candidate tiles per wave (the TPW instantiated: 1, 2, 4)
    unsigned prep_grid[2] = {0, 0}, prep_block = 0;   // fused: the image launches on the candidate set and on the destination set (0 when self)
    KnnFusedLayout fl;                         // fused
    bool stats = false;                        // the call leaves exact-phase counters at the start of the scratch (knn_sweep_stats_launch)
    size_t scratch_bytes = 0;                  // what a caller has to bring for these sizes and flags: the same with and without hints or scratch
};

inline int knn_cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }
inline int knn_pad32(int n) { return (n + 31) & ~31; }

inline KnnFusedLayout knn_fused_layout(int B, int Nd, int dst_n, int Ns, int C, bool self) {
    KnnFusedLayout l;
    size_t end = 0;
    auto take = [&end](size_t bytes) { const size_t o = (end + 255) & ~(size_t)255; end = o + bytes; return o; };   // pieces on 256-byte multiples (ls_workspace.h)
    const size_t D = 3 * (size_t)C;
    l.cnt = take((size_t)B * Nd * 4);
    l.nsrc = take((size_t)B * Ns * 4);
    l.ndst = self ? l.nsrc : take((size_t)B * dst_n * 4);
    l.isrc = take((size_t)B * Ns * 4);
    l.idst = self ? l.isrc : take((size_t)B * dst_n * 4);
    l.sq = take((size_t)B * knn_pad32(Ns) * D * 2);
    l.dq = self ? l.sq : take((size_t)B * knn_pad32(dst_n) * D * 2);
    l.bytes = (end + 255) & ~(size_t)255;
    return l;
}

inline KnnPlan knn_plan(const KnnTraits& t) {
    KnnPlan p;
    const int B = t.B, Nd = t.Nd, Ns = t.Ns, C = t.C;
    // the fused kernel serves rows of 32 / 64 channels and at most KF_MAXNS padded candidates
    const bool fused_shape = (C == 32 || C == 64) && !t.valu_only && Ns >= 1 && knn_pad32(Ns) <= KF_MAXNS;
    // candidate splits the tile kernel asks for: fill the chip when the (instance x query-tile) grid is small
    const int qtiles = knn_cdiv(Nd, KNN_TQ), ctiles = knn_cdiv(Ns, KNN_TS);
    const int blocks = B * qtiles;
    int ask = 1;
    if (blocks < 512 && ctiles >= 2) {   // (>= 2 workgroups per CU of the chip this was tuned on: splitting would only add merge work and un-seeded splits)
        // one workgroup per CU is the target: every split re-stages the 64 x 3C query tile and only split 0 is seeded, so at the
        // layer-4 shape (128 x 512, D = 192) 2 splits run in 0.14 ms where 8 splits (1024 workgroups) took 0.23 ms and 1 split 0.19 ms
        ask = knn_cdiv(256, blocks);     // (1 from 256 workgroups on)
        if (ask > ctiles) ask = ctiles;
        if (ask > 16) ask = 16;
    }
    // Scratch: sized by the shape and the flags alone, hints or not.  A fused shape is sized for two sets of their own even where the call is self or
    // has 32 queries or fewer and no hints (the small kernel, which uses none); every other shape for the lists of the splits asked, whichever kernel runs.
    p.scratch_bytes = fused_shape ? knn_fused_layout(B, Nd, t.dst_n, Ns, C, false).bytes : (ask > 1 ? (size_t)B * Nd * ask * 16 * sizeof(unsigned long long) : 0);

    // A call without scratch never takes the fused kernel.  With 32 queries or fewer an un-seeded call takes the small kernel below, a seeded
    // one the fused kernel all the same (which ignores the hints).
    if (t.has_scratch && fused_shape && (t.seeded || Nd > 32)) {
        p.ns_pad = knn_pad32(Ns); p.dst_npad = knn_pad32(t.dst_n);
        const int need = knn_cdiv(p.ns_pad / 32, KF_WAVES);    // candidate tiles per wave; three run as four
        p.tpw = need <= 1 ? 1 : need == 2 ? 2 : 4;
        p.kernel = (KnnKernel)((int)(C == 32 ? KnnKernel::FUSED_32_T1 : KnnKernel::FUSED_64_T1) + (p.tpw == 1 ? 0 : p.tpw == 2 ? 1 : 2));
        p.qtiles = knn_cdiv(Nd, KF_QT);
        p.grid = (unsigned)(B * p.qtiles); p.block = 64 * KF_WAVES;
        p.prep_block = C == 32 ? 192 : 256;                    // a workgroup per 32-row tile, KK / WPT k-steps per wave (<6, 3>, <12, 4>)
        p.prep_grid[0] = (unsigned)(B * (p.ns_pad / 32));
        p.prep_grid[1] = t.self ? 0 : (unsigned)(B * (p.dst_npad / 32));
        p.fl = knn_fused_layout(B, Nd, t.dst_n, Ns, C, t.self);
        p.stats = true;
        return p;
    }
    if (C == 1) {   // raw clouds: a wave per query
        // queries per wave: 16 amortises the candidate registers; fewer when the launch would not fill the 256 CUs
        for (p.qpw = 16; p.qpw > 1 && (long long)B * knn_cdiv(Nd, 4 * p.qpw) < 1024;) p.qpw >>= 1;
        p.kernel = Ns <= KX_CH ? KnnKernel::XYZ_SINGLE : KnnKernel::XYZ_CHUNKED;
        p.qblocks = knn_cdiv(Nd, 4 * p.qpw);
        p.grid = (unsigned)(B * p.qblocks);
        return p;
    }
    if (Nd <= 32) {   // few queries per instance (encoder layers 5, 6): one pair per thread on whole rows instead of 64 x 64 tiles
        p.kernel = KnnKernel::SMALL;
        p.qblocks = knn_cdiv(Nd, KSM_Q);
        p.grid = (unsigned)(B * p.qblocks);
        return p;
    }
    // the tile kernel; a call without scratch never splits.  The splits asked only bound the tiles per split: 17 tiles in 16 splits are 9 splits of 2.
    p.kernel = KnnKernel::TILE;
    p.qtiles = qtiles;
    p.tiles_per_split = knn_cdiv(ctiles, t.has_scratch ? ask : 1);
    p.splits = knn_cdiv(ctiles, p.tiles_per_split);
    p.grid = (unsigned)(B * qtiles * p.splits);
    p.merge_grid = p.splits > 1 ? (unsigned)knn_cdiv((long long)B * Nd, 16) : 0;   // a 16-lane row per query
    return p;
}

}  // namespace ls
