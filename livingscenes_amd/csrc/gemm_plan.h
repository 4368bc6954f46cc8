// gemm_plan.h -- which GEMM kernel runs a problem, on what grid: the dispatch policy of gemm.hip as a pure host function.  No HIP, no global
// state (the arithmetic mode is an input): gemm_run / gemm_vn_run (gemm.hip) build the traits, ask here and launch; callers that must know what
// a launch will do (split-K slabs to size, row maxima written or not, column sums honoured or not) ask the same function.  Compiles with a
// plain C++17 compiler: tests/test_gemm_plan_cpu.py replays it against the launches recorded in tests/golden/gemm_launches.json.
#pragma once
#include <algorithm>
#include <cstddef>

namespace ls {

// everything the choice depends on, and nothing else
struct GemmTraits {
    int M = 0, N = 0, K = 0, lda = 0, ldw = 0;
    int mode = 0;                    // gemm_mode(): 0 = two f16 pieces, 1 = three bf16 pieces (LS_GEMM_MODE=bf16x3), 2 = exact fp32 (LS_GEMM_MODE=fp32)
    int pieces = 3;                  // 3 = the mode's default product, 2 = two bf16 pieces (the decoder's opt-in throughput mode)
    bool gather = false;             // A rows through an index (a_rows)
    bool masked = false;             // out = (mask > 0) ? A W^T : 0
    bool may_split = false;          // a scratch buffer for split-K slabs was given
    bool latency = false;            // a handful of tiles by construction: the caller asks for the short-slab fp32 kernel
    bool has_planes = false;         // GemmAux::w_planes && GemmAux::w_rowmax
    bool wants_out_rowmax = false;   // GemmAux::out_rowmax
    // the VN form (gemm_vn_plan): out [M = B * npts * 3, C]
    int C = 0, npts = 0, a_parts = 0;
    bool has_G_or_cs = false, has_a_rowmax = false, has_w_rowmax = false;
};

// one enumerator per kernel instantiation that can be launched (gemm_run indexes its kernel tables by the order inside a family)
enum class GemmKernel {
    NONE,                                                          // gemm_vn_plan: shape / mode not supported
    F32_EXACT, F32_BF16X3, F32_BF16X2, F32_F16X2,                  // gemm_f32_kernel<false>, <true>, <true, 2>, <true, 22>
    H2, H2_PLANES, H2_ANYK,                                        // gemm_h2_kernel<true, false>, <true, true>, <false, false>
    W2, W2_MASKED, W2_PLANES, W2_MASKED_PLANES,                    // gemm_w2_kernel<MASKED, WPL>
    SMALLK32, SMALLK32_GATHER,                                     // gemm_smallk_kernel<32, GATHER>
    H2_SMALLK32_GATHER, H2_SMALLK32, H2_SMALLK64_GATHER, H2_SMALLK64,   // gemm_h2_smallk_kernel<KK, GATHER>
    VN_DIRECT, VN_DIRECT_ONEPART, VN_SMALLK32, VN_SMALLK64, VN, VN_ANYK  // gemm_vn_direct_kernel<64, ONEPART>, gemm_vn_smallk_kernel<KK>, gemm_vn_kernel<KAL>
};

struct GemmPlan {
    GemmKernel kernel = GemmKernel::NONE;
    unsigned grid_x = 0, grid_y = 1, block = 256;
    size_t lds = 0;                  // dynamic LDS bytes
    int nsplit = 1;                  // K slices asked for; > 1: partial slabs in the scratch + gemm_splitk_reduce_kernel on reduce_grid workgroups
    int ns = 1;                      // slices launched (grid_y): cdiv(K, kchunk) <= nsplit
    int kchunk = 0;                  // k per slice (K when the launch does not split)
    unsigned reduce_grid = 0;
    int tm = 0, tn = 0;              // tiles of the kernel's own shape: 128 x 128, the wide kernel 256 x 256, the VN kernels 120 x 64
    int per_n = 0;                   // persistent kernels: workgroups per N-tile; the streaming VN kernel: workgroups per instance (wpi)
    size_t scratch_floats = 0;       // split-K slabs: nsplit * M * N
    bool writes_out_rowmax = true;   // a split launch writes no GemmAux::out_rowmax
    bool honours_cs = false;         // VN form: GemmAux::cs is read (the streaming kernel only)
};

constexpr int GEMM_TILE = 128, GEMM_FP32_SLAB = 16, GEMM_SPLIT_SLAB = 32;   // gemm.hip: GM = GN, GK, and the 32-k slabs of the split kernels
inline int gemm_cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

// Under-filled grids with a long K loop (the per-instance "mean" rows of the residual global conv: M = 3B rows against
// K = C up to 512; conv_c) are pure latency: 32 workgroups x 16 dependent k-steps = 44 us for 0.2 GFLOP.  They are split
// along K into slices written as partial slabs and combined by a second launch.
inline int gemm_choose_splits(int M, int N, int K) {
    const int tiles = gemm_cdiv(M, GEMM_TILE) * gemm_cdiv(N, GEMM_TILE);
    if (tiles >= 192 || K < 128 || N % 4 != 0) return 1;
    int s2 = 512 / tiles;
    if (s2 > K / 32) s2 = K / 32;
    return s2 < 2 ? 1 : s2;
}
// the kernels that read planes: gemm_h2_kernel<true, true>, gemm_w2_kernel<., true>.  Measured: -5 % at
// the decoder shape (992 -> 941 us wide, 1198 -> 1128 us narrow), neutral at K = 512, +8 .. 15 % on the K = 128 / 256 tables: K >= 512 only
inline bool gemm_w_planes_useful(int K) { return K >= 512 && K % 32 == 0; }

inline GemmPlan gemm_plan(const GemmTraits& t) {
    const int M = t.M, N = t.N, K = t.K;
    GemmPlan p;
    const int tm = p.tm = gemm_cdiv(M, GEMM_TILE), tn = p.tn = gemm_cdiv(N, GEMM_TILE);
    p.kchunk = K;
    const bool split_on = t.mode != 2;      // LS_GEMM_MODE=fp32: exact fp32 FMA chains on v_mfma_f32_32x32x2_f32
    // (fp32 mode only: with three-piece bf16 products the tiled kernel below is faster on the K = 32 tables too -- 27.8 / 42.8 /
    // 34.5 us vs 28.8 / 47.2 / 38.8 us for the three layer-1/2 shapes -- and the arithmetic then depends on nothing but K)
    if (K == 32 && tm >= 16 && !split_on) {
        // persistent small-K kernel: ~3 resident workgroups per CU, spread evenly over the N-tiles.  (The K = 64 instantiation
        // needs 70 KB of LDS -> 2 workgroups per CU and measured SLOWER than the tiled kernel: 138 vs 110 us at the layer-3 shape.)
        // (odd: taken before every other rule -- a scratch, a mask or an out_rowmax given with such a problem is not looked at)
        p.per_n = std::min(gemm_cdiv(768, tn), tm);
        p.kernel = t.gather ? GemmKernel::SMALLK32_GATHER : GemmKernel::SMALLK32;
        p.grid_x = (unsigned)(tn * p.per_n);
        return p;
    }
    // The arithmetic must not depend on M (a decode of one instance's points has to equal the same rows inside a batched decode),
    // so the choice is the CALLER's: latency = a handful of tiles by construction (the per-instance mean rows of the global
    // conv, M = 3B), where the fp32 kernel's shorter slab (16 k, no split arithmetic before the first MFMA) wins: 44 vs 112 us
    // at M = 192, N = 1024, K = 512
    const bool split = split_on && !t.latency;
    // how an fp32 product is formed on the 16-bit matrix cores: 22 = two f16 pieces (three MFMAs per 16 k, the
    // default), 3 = three bf16 pieces (six MFMAs, any fp32 range: LS_GEMM_MODE=bf16x3), 2 = two bf16 pieces (opt-in decode mode)
    const int pieces = t.pieces == 3 ? (t.mode == 1 ? 3 : 22) : t.pieces;
    const bool wpl = t.has_planes && K % 32 == 0 && K > 64;   // planes only where a kernel reads them
    const GemmKernel h2 = K <= 64 ? GemmKernel::F32_F16X2 : (K % 32 == 0 ? (wpl ? GemmKernel::H2_PLANES : GemmKernel::H2) : GemmKernel::H2_ANYK);
    p.nsplit = (t.may_split && !t.masked) ? gemm_choose_splits(M, N, K) : 1;
    if (p.nsplit > 1) {
        const int kq = split ? GEMM_SPLIT_SLAB : GEMM_FP32_SLAB;
        p.kchunk = gemm_cdiv(gemm_cdiv(K, p.nsplit), kq) * kq;
        p.ns = gemm_cdiv(K, p.kchunk);
        // (odd: a split launch asked for with pieces == 2 runs the three-piece kernel)
        p.kernel = !split ? GemmKernel::F32_EXACT : (pieces == 22 ? h2 : GemmKernel::F32_BF16X3);
        p.grid_x = (unsigned)(tm * tn);
        p.grid_y = (unsigned)p.ns;
        p.reduce_grid = (unsigned)gemm_cdiv((long long)M * (N / 4), 256);
        p.scratch_floats = (size_t)p.nsplit * M * N;
        p.writes_out_rowmax = false;
        return p;
    }
    // 256 x 256 tiles once they fill the chip (same arithmetic, bit-identical results).  Measured: the wide kernel wins when its grid fills whole
    // rounds of the 256 CUs (one workgroup per CU): 480 tiles 88 -> 73 us, 768 tiles 355 -> 280 us, 3072 tiles 1186 -> 1002 us; ties at 384 tiles, loses below one round
    const long long wtiles = (long long)gemm_cdiv(M, 256) * gemm_cdiv(N, 256);
    const bool wide_on = wtiles >= 1024 || (wtiles >= 256 && wtiles * 100 >= 85 * 256 * gemm_cdiv(wtiles, 256));
    if (split && pieces == 22 && tm >= 16 && !t.masked && (K == 32 || K == 64) && !t.wants_out_rowmax) {
        p.per_n = std::min(gemm_cdiv(512, tn), tm);   // resident workgroups per CU x 256, spread evenly over the N-tiles
        p.kernel = K == 32 ? (t.gather ? GemmKernel::H2_SMALLK32_GATHER : GemmKernel::H2_SMALLK32)
                           : (t.gather ? GemmKernel::H2_SMALLK64_GATHER : GemmKernel::H2_SMALLK64);
        p.grid_x = (unsigned)(tn * p.per_n);
    } else if (split && pieces == 22 && wide_on && !t.gather && K % 32 == 0 && K >= 128 && (unsigned long long)M * t.lda < (1ull << 30) &&
               (unsigned long long)N * std::max(t.ldw, K) < (1ull << 30)) {   // (the wide kernel addresses its operands by 32-bit byte offsets)
        p.tm = gemm_cdiv(M, 256);
        p.tn = gemm_cdiv(N, 256);
        p.lds = 2 * 4 * 256 * 64 + 512 * sizeof(float);
        p.kernel = t.masked ? (wpl ? GemmKernel::W2_MASKED_PLANES : GemmKernel::W2_MASKED) : (wpl ? GemmKernel::W2_PLANES : GemmKernel::W2);
        p.grid_x = (unsigned)(p.tm * p.tn);
        p.block = 512;
    } else {
        p.kernel = !split ? GemmKernel::F32_EXACT : (pieces == 22 ? h2 : (pieces == 2 ? GemmKernel::F32_BF16X2 : GemmKernel::F32_BF16X3));
        p.grid_x = (unsigned)(tm * tn);
    }
    return p;
}
// split-K slabs (floats) of an M x N x K problem launched with a scratch buffer; 0: it does not split
inline size_t gemm_scratch_floats(int M, int N, int K) {
    GemmTraits t;
    t.M = M; t.N = N; t.K = K; t.lda = t.ldw = K; t.may_split = true;
    t.mode = 0;   // (the slab count does not depend on the arithmetic; mode 2's persistent K = 32 kernel sits below the K >= 128 of a split)
    return gemm_plan(t).scratch_floats;
}

// out [M = B * npts * 3, C] = VN-act(A W[0:C]^T + G lin part, A W[C:2C]^T + G dir part): see gemm_vn_kernel.  NONE = shape / mode not
// supported (the caller runs GEMM + vn_act_rows instead): the fused kernels exist for mode 0 only
inline GemmPlan gemm_vn_plan(const GemmTraits& t) {
    const int M = t.M, C = t.C, K = t.K;
    GemmPlan p;
    if (!(t.mode == 0 && C % 64 == 0 && K % 4 == 0 && K >= 32 && M % 3 == 0)) return p;
    const int tm = p.tm = gemm_cdiv(M, 120), tn = p.tn = C / 64;
    p.kchunk = K;
    p.writes_out_rowmax = true;
    // the streaming kernel (gemm_vn_direct_kernel): 64 channels, the producer's row maxima, whole 8-point tiles, at least 24 of them
    const bool streams = K == 64 && C == 64 && t.lda == K && t.npts % 8 == 0 && t.has_a_rowmax && t.a_parts > 0 && t.has_w_rowmax && M >= 24 * 64;
    if (streams && t.has_G_or_cs) {
        const int B = M / (3 * t.npts), tiles_inst = t.npts / 8;
        p.per_n = std::max(1, std::min(gemm_cdiv(512, B), gemm_cdiv(tiles_inst, 2)));   // ~512 workgroups (two per CU), every one inside one instance
        p.kernel = t.a_parts == 1 ? GemmKernel::VN_DIRECT_ONEPART : GemmKernel::VN_DIRECT;
        p.grid_x = (unsigned)(B * p.per_n);
        p.honours_cs = true;
    } else if ((K == 32 || K == 64) && tm >= 16 && t.lda == K) {
        p.per_n = std::min(gemm_cdiv(512, tn), tm);   // resident workgroups per CU x 256
        p.kernel = K == 32 ? GemmKernel::VN_SMALLK32 : GemmKernel::VN_SMALLK64;
        p.grid_x = (unsigned)(tn * p.per_n);
    } else {
        p.kernel = K % 32 == 0 ? GemmKernel::VN : GemmKernel::VN_ANYK;
        p.grid_x = (unsigned)(tm * tn);
    }
    return p;
}

}  // namespace ls
