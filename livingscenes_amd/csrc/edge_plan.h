// edge_plan.h -- what one edge-conv layer (i >= 1) of the encoder launches: which gather kernel on what grid, how its table area is laid out and
// formed, which side products the kernel emits.  The one statement of that choice, as a pure host function: no HIP, no global state (the
// arithmetic mode is an input).  model.hip builds the traits, asks here, forms the tables (edge_tables_run) and calls edge_run (edge.hip), which
// launches what the plan names; the encoder reads the side products off the same plan.  Compiles with a plain C++17 compiler:
// tests/test_edge_plan_cpu.py replays it against the launches recorded in tests/golden/edge_launches.json.
#pragma once
#include <cstddef>

namespace ls {

// everything the choice depends on, and nothing else
struct EdgeTraits {
    bool attn = false;               // attention layer (i >= atten_start_layer), else mean-pool
    int Cin = 0, Co = 0, head_c = 0;
    int B = 0, Ns = 0, Nd = 0;
    bool has_rows = false;           // the destination points are rows of the source points selected by FPS (a down-sampling layer)
    int mode = 0;                    // gemm_mode(), as GemmTraits::mode
    // LS_OPT_EDGE_FUSE_Q: destination side of attention layers 2 - 4 inside the edge kernel; LS_OPT_EDGE_FUSE_T: table-free 32-point attention layers
    bool fuse_q = true, fuse_t = true;
    bool has_wq = false, has_wt = false;             // the handle holds the layer's destination-side (edge_attn_fq_shape) / table-free (edge_ft_shape) weight planes
    // the caller has a buffer for the row maxima of the output (a residual global conv follows) / for its partial column sums (... and LS_OPT_GLOB_FUSE != 0)
    bool want_rowmax = false, want_colsum = false;
};

// one enumerator per kernel instantiation that can be launched (edge_run switches on it; the mean-pool kernels come first); FT_*: edge_ft_qk_kernel + edge_ft_norms_kernel +
// edge_ft_v_kernel<CIN, NS, HG> of edge_fused.hip, after edge_ft_prep_a_kernel<CIN / 16> where the table GEMM was
enum class EdgeKernel {
    POOL, POOL_V4_8, POOL_V4_16,                               // edge_pool_kernel, edge_pool_v4_kernel<LPP>
    ATTN, ATTN_V4_16, ATTN_V4_32, ATTN_V4_64, ATTN_V4_64X2,    // edge_attn_kernel, edge_attn_v4_kernel<16, 1>, <32, 1>, <64, 1>, <64, 2>
    ATTN_FQ_16_32, ATTN_FQ_16_64, ATTN_FQ_32_64,               // edge_attn_fq_kernel<LPP, CIN>
    FT_128, FT_256                                             // <128, 128, 1> (released layer 5), <256, 32, 2> (layer 6)
};

// the table-free path's scratch inside the layer's table area, as byte offsets: A planes (rows of Cin / 4 uint4) + exponents of the source rows
// (p) and of the selected destination rows (q: the same pieces when the layer does not down-sample), raw scores, partial norms, the summed norms
struct EdgeFtLayout { size_t a_p = 0, ae_p = 0, a_q = 0, ae_q = 0, scores = 0, sskp = 0, ssqp = 0, invk = 0, invq = 0, bytes = 0; };

struct EdgePlan {
    EdgeKernel kernel = EdgeKernel::POOL;
    unsigned grid = 0, block = 256;  // the gather launch; FT_*: of the q/k and the v launch (the norms launch between them: B workgroups)
    size_t lds = 0;                  // dynamic LDS bytes
    unsigned prep_grid[2] = {0, 0};  // FT_*: the operand-image launches on the source rows and (has_rows) on the selected rows
    // the table side: n_gemm GEMMs against the layer's weight rows, the first gemm_n[0] rows on all source points into the area's start, the
    // next gemm_n[1] on the selected points at q_off; 0: no table, the operand-image launches instead
    int n_gemm = 0, gemm_n[2] = {0, 0};
    int ldp = 0, ldq = 0, NQ = 0, qvr = 0;   // how the gather kernel reads them: leading dimensions of the neighbour / destination side, the
                                             // destination side's rows per instance, and whether it is indexed by source row (1) or by point (0)
    size_t q_off = 0;                // floats from the area's start to the destination side
    size_t table_floats = 0;         // the area (edge_table_floats)
    EdgeFtLayout ft;                 // FT_*
    int rowmax_parts = 0;            // row maxima of the output, this many per row; 0: none written
    int cs_rows = 0;                 // partial column sums [B][cs_rows][3][Co]; 0: none written
};

constexpr int EDGE_K = 16, EDGE_FT_ND = 32;   // neighbours per point (edge.hip: EK, edge_fused.hip: FK); destination points of the table-free kernels (FND)
inline unsigned edge_cdiv(long long a, long long b) { return (unsigned)((a + b - 1) / b); }

// can this layer shape ever take the table-free path (edge_fused.hip has kernels for it)?  ls_model_create allocates wt_planes by it
inline bool edge_ft_shape(int Co, int Cin, int head_c) { return head_c == 16 && ((Cin == 128 && Co % 16 == 0) || (Cin == 256 && Co % 32 == 0)); }
// ... the fused destination side (edge_attn_fq_kernel)?  wq_planes
inline bool edge_attn_fq_shape(int Co, int Cin, int head_c) { return head_c == 16 && ((Co == 64 && (Cin == 32 || Cin == 64)) || (Co == 128 && Cin == 64)); }
inline int edge_ft_heads_per_group(int Cin) { return Cin == 256 ? 2 : 1; }
// row maxima per row from the table-free path: one per head group (make_plan sizes its buffers by it where edge_ft_shape holds)
inline int edge_ft_rowmax_parts(int Co, int Cin) { return Co / 16 / edge_ft_heads_per_group(Cin); }
// the fused and the float4 pool kernel address the neighbour-side table by 32-bit byte offsets formed with a 24-bit multiply, and pack
// neighbour indices two per register
inline bool edge_off32_fits(int B, int Ns, int ldt) {
    return (unsigned long long)B * Ns * 3ull * ldt * 4ull < (1ull << 32) && (unsigned long long)B * Ns < (1ull << 24) && 3ull * ldt * 4ull < (1ull << 24) &&
           Ns < 65536;
}
// floats of the per-point table(s): one combined table over the source points, or (destination points selected by FPS rows) a neighbour-side
// table on the source points + a destination-side table on the selected points
inline size_t edge_table_floats(bool attn, int Co, int B, int Ns, int Nd, bool has_rows) {
    const size_t nc = (size_t)(attn ? 10 : 4) * Co, pc = (size_t)(attn ? 4 : 2) * Co;
    return has_rows ? (size_t)B * 3 * ((size_t)Ns * pc + (size_t)Nd * (nc - pc)) : (size_t)B * Ns * 3 * nc;
}
inline EdgeFtLayout edge_ft_layout(int B, int Ns, int Nd, int Cin, int Co, bool has_rows) {
    const size_t rp = (size_t)B * Ns * 3, rq = (size_t)B * Nd * 3, H = Co / 16;
    EdgeFtLayout l;
    size_t end = 0;
    auto take = [&end](size_t bytes) { const size_t o = (end + 255) & ~(size_t)255; end = o + bytes; return o; };   // pieces on 256-byte multiples (ls_workspace.h)
    l.a_p = take(rp * Cin / 4 * 16);
    l.ae_p = take(rp * 4);
    l.a_q = has_rows ? take(rq * Cin / 4 * 16) : l.a_p;
    l.ae_q = has_rows ? take(rq * 4) : l.ae_p;
    l.scores = take((size_t)B * H * Nd * EDGE_K * 4);
    l.sskp = take((size_t)B * H * Nd * EDGE_K * 4);
    l.ssqp = take((size_t)B * H * Nd * 4);
    l.invk = take((size_t)B * Nd * EDGE_K * 4);
    l.invq = take((size_t)B * Nd * 4);
    l.bytes = (end + 255) & ~(size_t)255;
    return l;
}

inline EdgePlan edge_plan(const EdgeTraits& t) {
    EdgePlan p;
    const int Co = t.Co, Cin = t.Cin, B = t.B, Ns = t.Ns, Nd = t.Nd;
    const int nc = (t.attn ? 10 : 4) * Co, pc = (t.attn ? 4 : 2) * Co;
    const long long total = (long long)B * Nd;
    p.table_floats = edge_table_floats(t.attn, Co, B, Ns, Nd, t.has_rows);
    // points per workgroup of the fused and the float4-lane attention kernels of Co = 64 / 128 = points per row of column sums (0: none)
    const int pw = Co == 64 ? 16 : Co == 128 ? 8 : 0;
    // The fused paths form their products from f16 pieces like the default GEMM mode; under LS_GEMM_MODE=bf16x3 / fp32 (any fp32 range, or the
    // fp32-MFMA kernels) the table path is kept so that every product of the layer is formed the same way.
    const bool f16 = t.mode == 0;
    // table-free: 32 destination points of 128 sources through rows (released layer 5) or of 32 sources (layer 6), and the scratch fits the area
    if (t.attn && t.fuse_t && f16 && t.has_wt && edge_ft_shape(Co, Cin, t.head_c) && Nd == EDGE_FT_ND &&
        ((Cin == 128 && Ns == 128 && t.has_rows) || (Cin == 256 && Ns == 32 && !t.has_rows))) {
        p.ft = edge_ft_layout(B, Ns, Nd, Cin, Co, t.has_rows);
        if (p.ft.bytes <= p.table_floats * sizeof(float)) {
            p.kernel = Cin == 128 ? EdgeKernel::FT_128 : EdgeKernel::FT_256;
            p.grid = (unsigned)(edge_ft_rowmax_parts(Co, Cin) * B);   // a workgroup per head group and instance
            p.prep_grid[0] = (unsigned)(B * Ns * 3 / 32);
            p.prep_grid[1] = t.has_rows ? (unsigned)(B * Nd * 3 / 32) : 0;
            p.rowmax_parts = t.want_rowmax ? edge_ft_rowmax_parts(Co, Cin) : 0;
            p.cs_rows = t.want_colsum ? 1 : 0;
            return p;
        }
    }
    p.ldp = pc;
    // attention layers 2 - 4, destination side inside the edge kernel: only the neighbour-side table.  (A batch whose table reaches 4 GB takes the table path.)
    if (t.attn && t.fuse_q && f16 && t.has_wq && edge_attn_fq_shape(Co, Cin, t.head_c) && edge_off32_fits(B, Ns, pc)) {
        p.kernel = Co == 128 ? EdgeKernel::ATTN_FQ_32_64 : (Cin == 32 ? EdgeKernel::ATTN_FQ_16_32 : EdgeKernel::ATTN_FQ_16_64);
        p.grid = edge_cdiv(total, pw);
        p.n_gemm = 1; p.gemm_n[0] = pc;
        p.rowmax_parts = t.want_rowmax ? 1 : 0;
        p.cs_rows = t.want_colsum && Nd % pw == 0 ? Nd / pw : 0;
        return p;
    }
    if (t.has_rows) { p.n_gemm = 2; p.gemm_n[0] = pc; p.gemm_n[1] = nc - pc; p.q_off = (size_t)B * Ns * 3 * pc; p.ldq = nc - pc; p.NQ = Nd; p.qvr = 0; }
    else { p.n_gemm = 1; p.gemm_n[0] = nc; p.q_off = (size_t)pc; p.ldp = p.ldq = nc; p.NQ = Ns; p.qvr = 1; }
    const bool v4 = p.ldp % 4 == 0 && p.ldq % 4 == 0;   // 16-byte-aligned table rows: the float4-lane kernels
    if (t.attn) {
        if (v4 && (Co == 64 || Co == 128 || Co == 256 || Co == 512)) {
            const int lpp = Co == 64 ? 16 : Co == 128 ? 32 : 64;   // lanes per point
            p.kernel = Co == 64 ? EdgeKernel::ATTN_V4_16 : Co == 128 ? EdgeKernel::ATTN_V4_32 : Co == 256 ? EdgeKernel::ATTN_V4_64 : EdgeKernel::ATTN_V4_64X2;
            p.grid = edge_cdiv(total, 4 * (64 / lpp));
            p.rowmax_parts = t.want_rowmax ? 1 : 0;
            p.cs_rows = t.want_colsum && pw > 0 && Nd % pw == 0 ? Nd / pw : 0;   // (Co = 64 / 128 share the fused kernel's point map)
        } else {   // the generic kernel: no row maxima, no column sums
            p.kernel = EdgeKernel::ATTN;
            p.grid = edge_cdiv(total, 4);
            p.lds = (size_t)4 * (3 * Co + 2 * (Co / 16) * EDGE_K) * sizeof(float);
        }
        return p;
    }
    const bool pv4 = v4 && (Co == 32 || Co == 64) && edge_off32_fits(B, Ns, p.ldp);
    p.kernel = pv4 ? (Co == 32 ? EdgeKernel::POOL_V4_8 : EdgeKernel::POOL_V4_16) : EdgeKernel::POOL;
    p.grid = edge_cdiv(total, pv4 ? (Co == 32 ? 32 : 16) : (Co <= 32 ? 8 : 4));   // points per workgroup
    return p;
}

}  // namespace ls
