// model.hip -- the model's part of the C ABI: version / error / device count, the model handle and its options, the per-layer operator exports, profiling
// and the two composite hot-path entry points (ls_encode = Shape_Prior.encode, ls_sdf_decode = FieldWrapper.forward).  Leaf operators are exported at the
// end of the file that holds their kernels; what this file calls in other translation units is declared in ls_launch.h.  Host code only enqueues work on
// the caller's stream (plus one library-owned side stream for the FPS chain); it never synchronises the device.
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "ls_launch.h"

namespace ls {

static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

}  // namespace ls

using namespace ls;

struct ProfRec { int kind, layer; hipEvent_t a, b; };

struct ls_model {
    ls_model_desc d;
    float* blob = nullptr;
    void* wt_planes[LS_MAX_LAYERS] = {};   // attention layers whose input has 128 / 256 channels (released layers 5, 6): ALL table weights as per-head f16
                                           // MFMA fragment tiles (edge_fused.hip); used when the call's point counts fit the fused kernels
    void* wq_planes[LS_MAX_LAYERS] = {};   // attention layers 2 - 4: destination-side weights as f16 MFMA fragments (edge.hip, edge_attn_fq_kernel)
    bool fuse_q = true;                    // LS_OPT_EDGE_FUSE_Q: destination side of attention layers 2 - 4 inside the edge kernel (edge.hip: edge_attn_fq_kernel)
    bool fuse_t = true;                    // LS_OPT_EDGE_FUSE_T: table-free 32-point attention layers (edge_fused.hip)
    int glob_fuse = 1;                     // LS_OPT_GLOB_FUSE (0 / 1 / 2; 2 = 1 + the operator export ls_vn_lna_f32 chains exact row maxima like the encoder's producers do): residual global conv as mean + GEMV launch and GEMM + VN activation in one kernel (gemm.hip: gemm_vn_kernel)
    int debug_edge = 0;                    // LS_OPT_DEBUG_EDGE: ls_vn_edgeconv_* runs 0 = table GEMM + edge kernel, 1 = the table GEMM only, 2 = the edge kernel only on the
                                           // tables already in the workspace (per-operator counter passes: scripts/pmc_ops.py)
    float* dec_wt = nullptr;            // transposed decoder weights [kin_l][out_l], built by the first backward call
    size_t dec_wt_off[12] = {};
    // max|row| of every weight matrix a GEMM reads (gemm.hip, GemmAux::w_rowmax): saves the kernels their pre-pass over W
    struct WMax { const float* base; size_t rows; int K; const float* wmax; const char* planes; };   // planes: pre-split rows (GemmAux::w_planes) or null
    std::vector<WMax> wreg;
    float* wmax_pool = nullptr;         // blob matrices (ls_model_create)
    float* wmax_pool_t = nullptr;       // transposed decoder weights (first backward call)
    char* wplanes_pool = nullptr;       // pre-split f16 pieces of the K >= 128 matrices of the blob
    char* wplanes_pool_t = nullptr;     // ... of the transposed decoder weights
    hipStream_t side = nullptr;    // FPS chain
    hipStream_t side2 = nullptr;   // per-layer table GEMMs, concurrent with the k-NN of the same layer
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    hipEvent_t ev_fps[LS_MAX_LAYERS] = {};   // one per FPS level: a down-sampling layer waits for ITS level only (round 3: waiting for the whole chain
                                             // kept layer 2 idle for ~100 us while levels 1 and 2 were still running)
    hipEvent_t ev_feat[LS_MAX_LAYERS] = {}, ev_tab[LS_MAX_LAYERS] = {};
    bool train_splitk = true;      // ls_model_set_option(LS_OPT_SDF_TRAIN_SPLITK): split-K in the decoder's TRAINING-path GEMMs (under-filled
                                   // M = 1024 problems: 2.43 -> 1.6 ms per step); off = a row's result never depends on the batch it rides in
    bool sdf_bf16x2 = false;       // LS_SDF_BF16X2=1: decoder GEMMs with two-piece bf16 products (2^-16 per product, ~1.7x; opt-in)
    // captured launch sequences of ls_encode, one per (workspace, B, N, mode): OPT-IN (LS_ENCODE_GRAPH=1 / ls_model_set_option).
    // Measured on MI355X / ROCm 7.2 (round 2, bench.py, B = 64): replaying the ~170-node graph costs the host MORE than enqueueing
    // the kernels directly -- one step in flight 22.2k obj/s (2.53 ms of host time per step) vs 29.6k (1.98 ms) direct; eight steps in
    // flight 38.1k vs 39.4k -- so the direct path stays the default.
    struct EncGraph { void* ws; size_t ws_bytes; int B, N, pre; unsigned flags; hipStream_t st; hipGraph_t graph; hipGraphExec_t exec; };
    std::vector<EncGraph> graphs;
    bool use_graph = false;
    bool graph_broken = false;     // a capture / instantiate failed once on this handle: stay on the direct path
    int debug_layers = -1;         // LS_DEBUG_LAYERS=n: ls_encode stops after n layers (outputs undefined) and prints the workspace plan:
                                   // race hunting by comparing workspaces (scripts/diag/)
    bool fps_side = true;          // LS_FPS_SIDE=0 runs the FPS chain on the caller's stream (A/B timing, race hunting)
    bool overlap_gemm = true;      // LS_GEMM_OVERLAP=0 serialises the table GEMMs on the caller's stream (A/B timing)
    bool profiling = false;
    std::vector<ProfRec> prof;          // pending (un-collected) event pairs
    std::vector<hipEvent_t> ev_pool;    // recycled events
    unsigned long long* knn_stats = nullptr;   // device [LS_MAX_LAYERS][2]: exact-phase statistics of the sweep-path k-NN layers, filled by profiled ls_encode calls only
    float prof_ms[LS_K_COUNT][16];
    int prof_n[LS_K_COUNT][16];
    std::vector<hipStream_t> prof_streams;
};

// RAII bracket: records an event pair around one launch when profiling is on
struct ProfScope {
    ls_model* m; hipStream_t st; ProfRec r; bool on;
    ProfScope(ls_model* m_, int kind, int layer, hipStream_t st_) : m(m_), st(st_), on(m_ && m_->profiling) {
        if (!on) return;
        auto get = [&]() { hipEvent_t e; if (!m->ev_pool.empty()) { e = m->ev_pool.back(); m->ev_pool.pop_back(); } else (void)hipEventCreate(&e); return e; };
        r.kind = kind; r.layer = layer < 16 ? layer : 15; r.a = get(); r.b = get();
        (void)hipEventRecord(r.a, st);
    }
    ~ProfScope() {
        if (!on) return;
        (void)hipEventRecord(r.b, st);
        m->prof.push_back(r);
        bool seen = false;
        for (auto s : m->prof_streams) seen |= (s == st);
        if (!seen) m->prof_streams.push_back(st);
    }
};
#define PROF(kind, layer, st) ProfScope _ps_##__LINE__(m, kind, layer, st)

static inline int pad4(int cols) { return (cols + 3) / 4 * 4; }   // a matrix's columns as whole float4s

// a layer's widths: input channels and table columns (mean-pool: 2 Co neighbour-side + 2 Co destination-side, attention: 4 Co + 6 Co); output channels: d.feat_dim[i]
static inline int layer_cin(const ls_model_desc& d, int i) { return i == 0 ? 1 : d.feat_dim[i - 1]; }
static inline int layer_ncols(const ls_model_desc& d, int i) { return i == 0 ? 0 : (i >= d.atten_start_layer ? 10 : 4) * d.feat_dim[i]; }

// ------------------------------------------------------------------------------------------------ plan
struct EncPlan {
    int L = 0;
    int Ns[LS_MAX_LAYERS], Nd[LS_MAX_LAYERS], level[LS_MAX_LAYERS];
    int nlevels = 0, levelN[LS_MAX_LAYERS + 1];
    int NP = 0, Cdp = 0;
    // workspace offsets (bytes)
    size_t o_pts[LS_MAX_LAYERS + 1], o_fps[LS_MAX_LAYERS + 1], o_centroid, o_scale0, o_pro, o_knn, o_knn2, o_knns, o_fA, o_fB, o_msg, o_T, o_TG, o_g, o_G, o_Tc, o_gws, o_xin, o_out, o_rm_msg, o_rm_out[2], o_cs, o_fpsws, fpsws_bytes, total;
};

static int make_plan(const ls_model_desc& d, int B, int N, EncPlan& p) {
    LS_REQUIRE(d.num_layers >= 2 && d.num_layers <= LS_MAX_LAYERS, "encoder: num_layers=%d unsupported", d.num_layers);
    p.L = d.num_layers;
    int cur = N;
    p.nlevels = 0;
    p.levelN[0] = N;
    size_t maxF = 0, maxT = 0, maxTG = 0, maxC = 0, maxKnn = 0, maxKs = 0, maxGws = 0, maxRm = 0, maxCs = 0;
    for (int i = 0; i < p.L; ++i) {
        p.Ns[i] = cur;
        const int f = d.down_factor[i] > 1 ? d.down_factor[i] : 1;
        p.level[i] = -1;
        if (f > 1) {
            LS_REQUIRE(i > 0, "encoder: down-sampling at layer 0 unsupported");
            p.level[i] = p.nlevels;
            p.nlevels++;
            cur = cur / f;
            p.levelN[p.nlevels] = cur;
        }
        p.Nd[i] = cur;
        LS_REQUIRE(cur >= 1, "encoder: N=%d too small for the down-sampling schedule", N);
        // a layer with fewer source points than neighbours would hand -1 padded lists to the gather kernels (and the reference's
        // behaviour there is pytorch3d's padding convention, unpinned): refuse instead of reading out of bounds
        LS_REQUIRE(p.Ns[i] >= d.num_knn, "encoder: layer %d has %d source points < num_knn=%d (N=%d too small for the schedule)", i,
                   p.Ns[i], d.num_knn, N);
        const int Cin = layer_cin(d, i), Co = d.feat_dim[i];
        const bool attn = i >= d.atten_start_layer;
        LS_REQUIRE(Co % 16 == 0, "encoder: feat_dim[%d]=%d must be a multiple of 16", i, Co);
        if (i > 0) LS_REQUIRE(Cin % 32 == 0, "encoder: feat_dim[%d]=%d must be a multiple of 32 (k-NN chunking)", i - 1, Cin);
        maxF = std::max(maxF, (size_t)p.Nd[i] * 3 * Co);
        if (i > 0) maxT = std::max(maxT, edge_table_floats(attn, Co, 1, p.Ns[i], p.Nd[i], f > 1));   // per instance
        maxTG = std::max(maxTG, (size_t)p.Nd[i] * 3 * 2 * Co);
        maxC = std::max(maxC, (size_t)Co);
        // row maxima of a layer's message / output: one part per 32 channels + 1, or -- where the table-free path of the 32-point layers may run
        // (edge_fused.hip) -- one per head group; sized per LAYER (round 4 sized Nd and the parts by separate maxima, which only held because
        // the released schedule has wide early layers: ADVICE r4)
        if (i >= d.res_global_start_layer) {
            size_t parts = (size_t)Co / 32 + 1;
            if (i > 0 && attn && edge_ft_shape(Co, Cin, d.atten_head_c)) parts = std::max(parts, (size_t)edge_ft_rowmax_parts(Co, Cin));
            maxRm = std::max(maxRm, (size_t)p.Nd[i] * parts);
            // partial column sums of the message from the attention kernel that wrote it (global_conv): at most one row per 8 points
            maxCs = std::max(maxCs, (size_t)(p.Nd[i] / 8 + 1) * 3 * Co);
        }
        // split-K slabs of the under-filled GEMMs (residual global conv: per-point part and per-instance mean part)
        maxGws = std::max(maxGws, std::max(gemm_scratch_floats(B * p.Nd[i] * 3, 2 * Co, Co), gemm_scratch_floats(B * 3, 4 * Co, Co)));
        maxKnn = std::max(maxKnn, (size_t)p.Nd[i] * 16);
        maxKs = std::max(maxKs, knn_scratch_bytes(B, p.Nd[i], p.Ns[i], p.Ns[i], Cin, 0u));
    }
    LS_REQUIRE(d.num_knn == 16, "encoder: num_knn=%d unsupported (16)", d.num_knn);
    LS_REQUIRE(p.Ns[p.L - 1] >= 1, "encoder: bad schedule");
    p.NP = cur;
    p.Cdp = pad4(d.c_dim + 1);
    Arena a(nullptr);   // the plan stores offsets: encode_enqueue adds the workspace
    for (int l = 0; l <= p.nlevels; ++l) {
        p.o_pts[l] = a.take_bytes((size_t)B * p.levelN[l] * 3 * 4);
        p.o_fps[l] = a.take_bytes((size_t)B * p.levelN[l] * 4);
    }
    p.o_centroid = a.take_bytes((size_t)B * 3 * 4);
    p.o_scale0 = a.take_bytes((size_t)B * 4);
    p.o_pro = a.take_bytes(prologue_scratch_floats(B) * 4);
    p.o_knn = a.take_bytes((size_t)B * maxKnn * 4);
    p.o_knn2 = a.take_bytes((size_t)B * maxKnn * 4);
    p.o_knns = a.take_bytes(maxKs + 256);
    p.o_fA = a.take_bytes((size_t)B * maxF * 4);
    p.o_fB = a.take_bytes((size_t)B * maxF * 4);
    p.o_msg = a.take_bytes((size_t)B * maxF * 4);
    p.o_T = a.take_bytes((size_t)B * maxT * 4);
    p.o_TG = a.take_bytes((size_t)B * maxTG * 4);
    p.o_g = a.take_bytes((size_t)B * 3 * maxC * 4);
    p.o_G = a.take_bytes((size_t)B * 3 * 4 * maxC * 4);
    p.o_Tc = a.take_bytes((size_t)B * p.NP * 3 * p.Cdp * 4);
    maxGws = std::max(maxGws, gemm_scratch_floats(B * p.NP * 3, p.Cdp, d.feat_dim[p.L - 1]));
    p.o_gws = a.take_bytes(maxGws * 4 + 256);
    // row maxima of the messages / layer outputs, chained into the GEMMs that read them (gemm.hip, GemmAux)
    p.o_rm_msg = a.take_bytes((size_t)B * maxRm * 3 * 4);      // maxRm = max over the layers of Nd x parts (above)
    p.o_rm_out[0] = a.take_bytes((size_t)B * maxRm * 3 * 4);
    p.o_rm_out[1] = a.take_bytes((size_t)B * maxRm * 3 * 4);
    p.o_cs = a.take_bytes((size_t)B * maxCs * 4);
    // FPS scratch of the encoder's own down-sampling chain (fps.hip: exact bucket pruning for 8 193 .. 65 536 source points; 0 bytes below that).  The
    // levels run one after the other on one stream and share it.  (the chain passed no workspace, so an encode with N > 8192 failed in the
    // MIDDLE of the enqueue, after the side stream had forked.)
    p.fpsws_bytes = 0;
    for (int l = 0; l < p.nlevels; ++l) {
        LS_REQUIRE(p.levelN[l] <= 65536, "encoder: %d points at down-sampling level %d (FPS handles at most 65536)", p.levelN[l], l);
        p.fpsws_bytes = std::max(p.fpsws_bytes, fps_scratch_bytes_per_cloud(p.levelN[l]) * (size_t)B);
    }
    p.o_fpsws = a.take_bytes(p.fpsws_bytes);
    // staging of the captured-graph path: the graph reads x from / writes the codes to FIXED addresses inside the workspace
    p.o_xin = a.take_bytes((size_t)B * 3 * N * 4);
    p.o_out = a.take_bytes((size_t)B * (4 * (size_t)d.c_dim + 4) * 4);
    p.total = a.bytes();
    return LS_OK;
}

static int dec_out(const ls_model_desc& d, int l);
// ------------------------------------------------------------------------------------------------ weight row maxima
// rows [W, W + N*K) of a registered matrix with the same K -> their maxima; nullptr = not registered (the GEMM then scans W itself)
static const float* wmax_for(const ls_model* m, const float* W, int N, int K, const void** planes = nullptr) {
    for (const auto& e : m->wreg) {
        if (e.K != K || W < e.base) continue;
        const size_t off = (size_t)(W - e.base);
        if (off % K == 0 && off / K + (size_t)N <= e.rows) {
            if (planes) *planes = e.planes ? e.planes + gemm_w_planes_bytes(off / K, K) : nullptr;
            return e.wmax + off / K;
        }
    }
    return nullptr;
}
static GemmAux aux_w(const ls_model* m, const float* W, int N, int K) {
    GemmAux a;
    a.w_rowmax = wmax_for(m, W, N, K, &a.w_planes);
    return a;
}
struct WSpec { const float* base; size_t rows; int K; };
static int wmax_register(ls_model* m, const std::vector<WSpec>& specs, float** pool, char** planes_pool, hipStream_t st) {
    size_t total = 0, pbytes = 0;
    for (const auto& sp : specs) {
        total += sp.rows;
        if (gemm_w_planes_useful(sp.K)) pbytes += gemm_w_planes_bytes(sp.rows, sp.K);
    }
    if (!total) return LS_OK;
    LS_HIP_CHECK(hipMalloc((void**)pool, total * sizeof(float)));
    if (pbytes) LS_HIP_CHECK(hipMalloc((void**)planes_pool, pbytes));
    size_t off = 0, poff = 0;
    for (const auto& sp : specs) {
        int rc = gemm_rowmax_launch(sp.base, (int)sp.rows, sp.K, sp.K, *pool + off, st);
        if (rc != LS_OK) return rc;
        const char* planes = nullptr;
        if (gemm_w_planes_useful(sp.K)) {
            planes = *planes_pool + poff;
            rc = gemm_presplit_w_launch(sp.base, (int)sp.rows, sp.K, sp.K, *pool + off, *planes_pool + poff, st);
            if (rc != LS_OK) return rc;
            poff += gemm_w_planes_bytes(sp.rows, sp.K);
        }
        m->wreg.push_back({sp.base, sp.rows, sp.K, *pool + off, planes});
        off += sp.rows;
    }
    return LS_OK;
}

// ------------------------------------------------------------------------------------------------ layer pieces
// (shared by ls_encode and the per-operator exports ls_vn_edgeconv_* / ls_vn_lna_f32 / ls_encoder_tail_f32)
// what edge-conv layer i >= 1 of a call launches (edge_plan.h: the one statement of the choice).  glob: a residual global conv follows, which
// takes the row maxima and (LS_OPT_GLOB_FUSE) the partial column sums of the message from the kernel that wrote it
static EdgePlan layer_edge_plan(const ls_model* m, int i, int B, int Ns, int Nd, bool has_rows, bool glob) {
    const ls_model_desc& d = m->d;
    EdgeTraits t;
    t.attn = i >= d.atten_start_layer; t.Cin = layer_cin(d, i); t.Co = d.feat_dim[i]; t.head_c = d.atten_head_c;
    t.B = B; t.Ns = Ns; t.Nd = Nd; t.has_rows = has_rows;
    t.mode = gemm_mode();
    t.fuse_q = m->fuse_q; t.fuse_t = m->fuse_t; t.has_wq = m->wq_planes[i] != nullptr; t.has_wt = m->wt_planes[i] != nullptr;
    t.want_rowmax = glob; t.want_colsum = glob && m->glob_fuse;
    return edge_plan(t);
}
// the table side of the plan: the folded VN-Linear contraction of layer i >= 1 (edge.hip header), cur [B,Ns,3,Cin] -> table(s) in T
// a_rowmax (nullable) [B*Ns*3][a_parts]: row maxima of `cur` from the kernel that wrote it (GemmAux)
static int edge_tables_run(ls_model* m, int i, const EdgePlan& ep, const float* cur, const int32_t* dst_rows, int B, int Ns, int Nd, float* T, hipStream_t gs,
                           const float* a_rowmax = nullptr, int a_parts = 0) {
    const ls_model_desc& d = m->d;
    const int Cin = layer_cin(d, i);
    const float* W = m->blob + d.off_edge[i];
    PROF(LS_K_GEMM_EDGE, i, gs);
    // 32-point attention layers (edge_fused.hip): no table -- only the operand image of the feature rows (f16 fragment planes) is formed here
    if (ep.n_gemm == 0) return edge_ft_prep_launch(cur, dst_rows, Ns, Nd, T, ep, gs);
    Gemm g;   // the neighbour-side (P) columns, or the combined table, on all source points
    g.A = cur; g.lda = Cin; g.W = W; g.ldw = Cin; g.out = T; g.M = B * Ns * 3; g.K = Cin;
    g.N = g.ldc = ep.gemm_n[0];
    g.aux = aux_w(m, W, layer_ncols(d, i), Cin);
    g.aux.a_rowmax = a_rowmax; g.aux.a_parts = a_parts;
    int rc = gemm_run(g, gs);
    if (ep.n_gemm == 1 || rc != LS_OK) return rc;
    // down-sampled layer: the destination-side (Q) table only on the FPS-selected destination points -- the following rows of the same matrix
    const int pc = ep.gemm_n[0];
    g.W = W + (size_t)pc * Cin; g.out = T + ep.q_off; g.M = B * Nd * 3; g.N = g.ldc = ep.gemm_n[1];
    g.a_rows = dst_rows; g.gNd = Nd; g.gNs = Ns;
    if (g.aux.w_rowmax) g.aux.w_rowmax += pc;
    if (g.aux.w_planes) g.aux.w_planes = static_cast<const char*>(g.aux.w_planes) + gemm_w_planes_bytes((size_t)pc, Cin);
    return gemm_run(g, gs);
}
// gather + VN activation + mean-pool | attention of layer i >= 1 over the tables; rowmax / colsum: where the plan's side products go
static int edge_layer_run(ls_model* m, int i, const EdgePlan& ep, const float* T, const float* cur, const int32_t* knn, const int32_t* dst_rows, int B, int Ns,
                          int Nd, float* out, hipStream_t st, float* rowmax = nullptr, float* colsum = nullptr) {
    const ls_model_desc& d = m->d;
    Edge e;
    e.T = T; e.cur = cur; e.planes = ep.n_gemm == 0 ? m->wt_planes[i] : m->wq_planes[i]; e.knn = knn; e.dst_rows = dst_rows;
    e.B = B; e.Ns = Ns; e.Nd = Nd; e.Cin = layer_cin(d, i); e.Co = d.feat_dim[i]; e.head_c = d.atten_head_c; e.neg_slope = d.neg_slope;
    e.out = out; e.rowmax = rowmax; e.colsum = colsum;
    PROF(i >= d.atten_start_layer ? LS_K_EDGE_ATTN : LS_K_EDGE_POOL, i, st);
    return edge_run(e, ep, st);
}
// residual global conv of layer i (vec_dgcnn_atten.py:222-225): out = VecLNA_G(cat(msg, mean_n msg))
static size_t global_conv_gws_floats(const ls_model_desc& d, int i, int B, int Nd) {
    const int Co = d.feat_dim[i];
    return std::max(gemm_scratch_floats(B * Nd * 3, 2 * Co, Co), gemm_scratch_floats(B * 3, 4 * Co, Co));
}
// rm_msg (nullable) [B*Nd*3]: row maxima of msg from the kernel that wrote it; rm_out (nullable) [B*Nd*3][Co/32]: receives those of `out`
// (*rm_written: whether the path taken wrote them) -- gemm.hip, GemmAux
static int global_conv(ls_model* m, int i, const float* msg, int B, int Nd, float* g, float* G, float* TG, float* gws, float* out, hipStream_t st,
                       const float* rm_msg = nullptr, float* rm_out = nullptr, bool* rm_written = nullptr, int rm_msg_parts = 1, const float* cs = nullptr,
                       int cs_rows = 0) {
    // cs (nullable) [B][cs_rows][3][Co]: partial column sums of msg from the kernel that wrote it (edge_plan.h: cs_rows): the mean is finished from them
    const ls_model_desc& d = m->d;
    const int Co = d.feat_dim[i];
    const float* Wg = m->blob + d.off_glob[i];
    if (rm_written) *rm_written = false;
    int rc;
    GemmVn v;   // the conv as ONE launch: the per-point contraction + the VN activation (gemm.hip: gemm_vn_kernel / gemm_vn_smallk_kernel / gemm_vn_direct_kernel)
    v.A = msg; v.lda = Co; v.W = Wg; v.ldw = Co; v.G = G; v.ldg = 4 * Co; v.out = out; v.M = B * Nd * 3; v.C = Co; v.K = Co; v.npts = Nd;
    v.oms = 1.0f - d.neg_slope;
    v.aux = aux_w(m, Wg, 2 * Co, Co);
    v.aux.a_rowmax = rm_msg; v.aux.a_parts = rm_msg ? rm_msg_parts : 0;
    v.aux.out_rowmax = rm_out;
    if (cs && cs_rows > 0 && cs_rows <= 32) { v.aux.cs = cs; v.aux.cs_rows = cs_rows; }
    const GemmPlan vp = gemm_vn_plan(gemm_traits(v));
    if (m->glob_fuse && vp.kernel != GemmKernel::NONE) {
        // 64-channel layers with the producer's column sums: the streaming kernel finishes the mean and its contraction itself -- no mean launch
        if (!(v.aux.cs && vp.honours_cs)) {
            // per-instance part: mean over the points and its contraction with the W_b / Wd W_b rows in ONE launch (pointwise.hip) ...
            v.aux.cs = nullptr; v.aux.cs_rows = 0;
            PROF(LS_K_MEAN, i, st);
            rc = (cs && cs_rows > 0) ? glob_mean_gemv_launch(cs, B, cs_rows, Co, Wg, 2 * Co, 2 * Co, G, 4 * Co, st, Nd)
                                     : glob_mean_gemv_launch(msg, B, Nd, Co, Wg, 2 * Co, 2 * Co, G, 4 * Co, st);
            if (rc != LS_OK) return rc;
        }
        // ... then the per-point launch
        PROF(LS_K_GEMM_GLOB, i, st);
        if (rm_written) *rm_written = rm_out != nullptr;
        return gemm_vn_run(v, st);
    }
    { PROF(LS_K_MEAN, i, st); rc = mean_points_launch(msg, B, Nd, Co, g, st); }
    if (rc != LS_OK) return rc;
    {
        PROF(LS_K_GEMM_GLOB, i, st);
        Gemm pt;   // per point: msg against the W_a / Wd W_a rows
        pt.A = msg; pt.lda = Co; pt.W = Wg; pt.ldw = Co; pt.out = TG; pt.ldc = 2 * Co; pt.M = B * Nd * 3; pt.N = 2 * Co; pt.K = Co; pt.scratch = gws;
        pt.aux = v.aux;
        pt.aux.out_rowmax = nullptr; pt.aux.cs = nullptr; pt.aux.cs_rows = 0;
        rc = gemm_run(pt, st);
        Gemm pi;   // per instance: the mean rows against all four row groups -- a handful of tiles by construction
        pi.A = g; pi.lda = Co; pi.W = Wg; pi.ldw = Co; pi.out = G; pi.ldc = 4 * Co; pi.M = B * 3; pi.N = 4 * Co; pi.K = Co; pi.scratch = gws; pi.latency = true;
        if (rc == LS_OK) rc = gemm_run(pi, st);
    }
    if (rc != LS_OK) return rc;
    PROF(LS_K_VN_ACT, i, st);
    return vn_act_rows_launch(TG, 2 * Co, G, 4 * Co, B, Nd, Co, d.neg_slope, out, st);
}
// conv_c + pooling + heads (vec_dgcnn_atten.py:231-250) + the encode epilogue (model_utils.py:182-195)
static int encoder_tail(ls_model* m, const float* cur, int B, int NP, float* Tc, float* gws, const float* centroid, const float* scale0,
                        float* z_so3, float* z_inv, float* s_out, float* t_out, hipStream_t st, const float* rm_cur = nullptr, int rm_parts = 0) {
    const ls_model_desc& d = m->d;
    const int Cl = d.feat_dim[d.num_layers - 1], Cdp = pad4(d.c_dim + 1);
    const float* W = m->blob;
    int rc = tail_check(d.c_dim);   // a refusal of tail_launch must not leave conv_c enqueued behind it
    if (rc != LS_OK) return rc;
    { PROF(LS_K_GEMM_TAIL, 0, st);
      Gemm g;
      g.A = cur; g.lda = Cl; g.W = W + d.off_convc; g.ldw = Cl; g.out = Tc; g.ldc = Cdp; g.M = B * NP * 3; g.N = Cdp; g.K = Cl; g.scratch = gws;
      g.aux = aux_w(m, g.W, Cdp, Cl);
      g.aux.a_rowmax = rm_cur; g.aux.a_parts = rm_parts;
      rc = gemm_run(g, st); }
    if (rc != LS_OK) return rc;
    PROF(LS_K_TAIL, 0, st);
    return tail_launch(Tc, Cdp, B, NP, d.c_dim, W + d.off_inv_t, W + d.off_c_fc0_t, W + d.off_c_misc, d.neg_slope, d.scale_factor,
                       d.center_pred, d.center_pred_scale, centroid, scale0, z_so3, z_inv, s_out, t_out, st);
}

extern "C" {

int ls_version(void) { return LS_ABI_VERSION; }
const char* ls_last_error(void) { return g_err; }

int ls_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { set_error("hipGetDeviceCount: %s", hipGetErrorString(e)); return LS_ERR_NO_DEVICE; }
    return n;
}

// ------------------------------------------------------------------------------------------------ model
int ls_model_create(const ls_model_desc* desc, const float* blob_host, ls_model_t** out) {
    LS_REQUIRE(desc && blob_host && out, "model_create: null argument");
    LS_REQUIRE(desc->blob_floats > 0, "model_create: empty blob");
    LS_REQUIRE(desc->dec_input == LS_DEC_INNER || desc->dec_input == LS_DEC_XYZ, "model_create: unknown dec_input %d", desc->dec_input);
    ls_model* m = new ls_model();
    m->d = *desc;
    if (const char* ev = getenv("LS_ENCODE_GRAPH")) m->use_graph = atoi(ev) != 0;
    if (const char* ev = getenv("LS_SDF_BF16X2")) m->sdf_bf16x2 = atoi(ev) != 0;
#ifdef LS_DEV_KNOBS   // race hunting (scripts/diag), only in a library built with -DLS_DEV_KNOBS
    if (const char* ev = getenv("LS_FPS_SIDE")) m->fps_side = atoi(ev) != 0;
    if (const char* ev = getenv("LS_DEBUG_LAYERS")) m->debug_layers = atoi(ev);
#endif
    hipError_t e = hipMalloc((void**)&m->blob, (size_t)desc->blob_floats * sizeof(float));
    if (e != hipSuccess) { delete m; set_error("hipMalloc(model blob): %s", hipGetErrorString(e)); return LS_ERR_HIP; }
    e = hipMemcpy(m->blob, blob_host, (size_t)desc->blob_floats * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&m->side, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&m->side2, hipStreamNonBlocking);
    for (int i = 0; i < LS_MAX_LAYERS && e == hipSuccess; ++i) {
        e = hipEventCreateWithFlags(&m->ev_feat[i], hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&m->ev_fps[i], hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&m->ev_tab[i], hipEventDisableTiming);
    }
    if (e == hipSuccess) e = hipEventCreateWithFlags(&m->ev_fork, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&m->ev_join, hipEventDisableTiming);
    if (e == hipSuccess) e = hipMalloc((void**)&m->knn_stats, sizeof(unsigned long long) * 2 * LS_MAX_LAYERS);
    if (e == hipSuccess) e = hipMemset(m->knn_stats, 0, sizeof(unsigned long long) * 2 * LS_MAX_LAYERS);
    if (e != hipSuccess) { set_error("model_create: %s", hipGetErrorString(e)); ls_model_destroy(m); return LS_ERR_HIP; }
    for (int i = desc->atten_start_layer; i < desc->num_layers && i >= 1; ++i) {   // attention layers: weight planes for the shapes the fused kernels serve (edge_plan.h)
        const int Co = desc->feat_dim[i], Cin = layer_cin(*desc, i);
        const float* W = m->blob + desc->off_edge[i];
        int rc = LS_OK;
        if (edge_ft_shape(Co, Cin, desc->atten_head_c)) {   // table-free 32-point layers (edge_fused.hip)
            e = hipMalloc(&m->wt_planes[i], edge_ft_w_bytes(Co, Cin));
            if (e == hipSuccess) rc = edge_ft_presplit_w_launch(W, Co, Cin, m->wt_planes[i], nullptr);
        }
        if (e == hipSuccess && rc == LS_OK && edge_attn_fq_shape(Co, Cin, desc->atten_head_c)) {   // destination side inside the edge kernel (edge.hip)
            e = hipMalloc(&m->wq_planes[i], edge_wq_planes_bytes(Co, Cin));
            if (e == hipSuccess) rc = edge_presplit_wq_launch(W + (size_t)4 * Co * Cin, Co, Cin, m->wq_planes[i], nullptr);   // (its rows follow the 4 Co neighbour-side rows)
        }
        if (e != hipSuccess) { set_error("model_create: %s", hipGetErrorString(e)); ls_model_destroy(m); return LS_ERR_HIP; }
        if (rc != LS_OK || hipDeviceSynchronize() != hipSuccess) { ls_model_destroy(m); return LS_ERR_HIP; }
    }
    {   // row maxima of every matrix the GEMMs read (GemmAux::w_rowmax)
        std::vector<WSpec> specs;
        const ls_model_desc& d = *desc;
        for (int i = 1; i < d.num_layers; ++i) specs.push_back({m->blob + d.off_edge[i], (size_t)layer_ncols(d, i), layer_cin(d, i)});
        for (int i = d.res_global_start_layer; i < d.num_layers; ++i)
            if (i >= 0) specs.push_back({m->blob + d.off_glob[i], (size_t)4 * d.feat_dim[i], d.feat_dim[i]});
        if (d.num_layers >= 1) specs.push_back({m->blob + d.off_convc, (size_t)pad4(d.c_dim + 1), d.feat_dim[d.num_layers - 1]});
        if (d.dec_num_linear >= 3) {
            int kin = d.dec_width;
            for (int l = 1; l < d.dec_num_linear - 1; ++l) {
                const int outw = dec_out(d, l);
                specs.push_back({m->blob + d.off_dec_w[l], (size_t)outw, kin});
                kin = outw;
            }
            specs.push_back({m->blob + d.off_dec_w[d.dec_num_linear - 1], 1, kin});
        }
        const int rc = wmax_register(m, specs, &m->wmax_pool, &m->wplanes_pool, nullptr);
        if (rc != LS_OK || hipDeviceSynchronize() != hipSuccess) { ls_model_destroy(m); return LS_ERR_HIP; }
    }
    *out = m;
    return LS_OK;
}

void ls_model_destroy(ls_model_t* m) {
    if (!m) return;
    if (m->blob) (void)hipFree(m->blob);
    if (m->dec_wt) (void)hipFree(m->dec_wt);
    if (m->wmax_pool) (void)hipFree(m->wmax_pool);
    if (m->wmax_pool_t) (void)hipFree(m->wmax_pool_t);
    if (m->wplanes_pool) (void)hipFree(m->wplanes_pool);
    if (m->wplanes_pool_t) (void)hipFree(m->wplanes_pool_t);
    for (int i = 0; i < LS_MAX_LAYERS; ++i) {
        if (m->wq_planes[i]) (void)hipFree(m->wq_planes[i]);
        if (m->wt_planes[i]) (void)hipFree(m->wt_planes[i]);
    }
    if (m->side) (void)hipStreamDestroy(m->side);
    if (m->side2) (void)hipStreamDestroy(m->side2);
    for (int i = 0; i < LS_MAX_LAYERS; ++i) {
        if (m->ev_feat[i]) (void)hipEventDestroy(m->ev_feat[i]);
        if (m->ev_fps[i]) (void)hipEventDestroy(m->ev_fps[i]);
        if (m->ev_tab[i]) (void)hipEventDestroy(m->ev_tab[i]);
    }
    if (m->ev_fork) (void)hipEventDestroy(m->ev_fork);
    if (m->ev_join) (void)hipEventDestroy(m->ev_join);
    if (m->knn_stats) (void)hipFree(m->knn_stats);
    for (auto& g : m->graphs) { (void)hipGraphExecDestroy(g.exec); (void)hipGraphDestroy(g.graph); }
    for (auto& r : m->prof) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    for (auto e : m->ev_pool) (void)hipEventDestroy(e);
    delete m;
}

// captured launch sequences are keyed on (workspace, B, N, mode, stream) only: an option that selects kernels must drop them, or a replay would
// run the launch sequence of the OLD setting
static void drop_graphs(ls_model* m) {
    for (auto& g : m->graphs) { (void)hipGraphExecDestroy(g.exec); (void)hipGraphDestroy(g.graph); }
    m->graphs.clear();
}

int ls_model_set_option(ls_model_t* m, int option, int value) {
    LS_REQUIRE(m, "model_set_option: null model");
    switch (option) {
        case LS_OPT_SDF_TRAIN_SPLITK: m->train_splitk = value != 0; return LS_OK;
        case LS_OPT_SDF_BF16X2: m->sdf_bf16x2 = value != 0; return LS_OK;
        case LS_OPT_ENCODE_GRAPH: m->use_graph = value != 0; return LS_OK;
        case LS_OPT_EDGE_FUSE_Q: m->fuse_q = value != 0; drop_graphs(m); return LS_OK;
        case LS_OPT_EDGE_FUSE_T: m->fuse_t = value != 0; drop_graphs(m); return LS_OK;
        case LS_OPT_GLOB_FUSE: LS_REQUIRE(value >= 0 && value <= 2, "model_set_option: LS_OPT_GLOB_FUSE takes 0, 1 or 2"); m->glob_fuse = value; drop_graphs(m); return LS_OK;
        case LS_OPT_DEBUG_EDGE: LS_REQUIRE(value >= 0 && value <= 2, "model_set_option: LS_OPT_DEBUG_EDGE takes 0, 1 or 2"); m->debug_edge = value; drop_graphs(m); return LS_OK;
        case LS_OPT_GEMM_OVERLAP: m->overlap_gemm = value != 0; drop_graphs(m); return LS_OK;
        default: set_error("model_set_option: unknown option %d", option); return LS_ERR_INVALID;
    }
}

int ls_model_get_option(const ls_model_t* m, int option, int* value) {
    LS_REQUIRE(m && value, "model_get_option: null argument");
    switch (option) {
        case LS_OPT_SDF_TRAIN_SPLITK: *value = m->train_splitk ? 1 : 0; return LS_OK;
        case LS_OPT_SDF_BF16X2: *value = m->sdf_bf16x2 ? 1 : 0; return LS_OK;
        case LS_OPT_ENCODE_GRAPH: *value = m->use_graph ? 1 : 0; return LS_OK;
        case LS_OPT_EDGE_FUSE_Q: *value = m->fuse_q ? 1 : 0; return LS_OK;
        case LS_OPT_EDGE_FUSE_T: *value = m->fuse_t ? 1 : 0; return LS_OK;
        case LS_OPT_GLOB_FUSE: *value = m->glob_fuse; return LS_OK;
        case LS_OPT_DEBUG_EDGE: *value = m->debug_edge; return LS_OK;
        case LS_OPT_GEMM_OVERLAP: *value = m->overlap_gemm ? 1 : 0; return LS_OK;
        default: set_error("model_get_option: unknown option %d", option); return LS_ERR_INVALID;
    }
}

size_t ls_encoder_workspace_bytes(const ls_model_t* m, int B, int N) {
    if (!m || B <= 0) return 0;   // (B = 0 would reach the split-K choice with an empty GEMM: a division by zero)
    EncPlan p;
    if (make_plan(m->d, B, N, p) != LS_OK) return 0;
    return p.total;
}

}  // extern "C"

// the launch sequence of Shape_Prior.encode on `st` (+ the handle's side streams, forked from and joined back into `st`)
static int encode_enqueue(ls_model_t* m, const EncPlan& p, const float* x, int B, int N, int pre_normalised, unsigned flags, float* z_so3,
                          float* z_inv, float* s_out, float* t_out, int32_t* trace_knn, int32_t* trace_fps, void* workspace, hipStream_t st) {
    const ls_model_desc& d = m->d;
    int rc = LS_OK;
    char* ws = (char*)workspace;
    auto F = [&](size_t o) { return (float*)(ws + o); };
    auto I = [&](size_t o) { return (int32_t*)(ws + o); };
    const float* W = m->blob;
    float* pts0 = F(p.o_pts[0]);
    float* centroid = F(p.o_centroid);
    float* scale0 = F(p.o_scale0);

    {
        PROF(LS_K_PROLOGUE, 0, st);
        if (pre_normalised) rc = transpose_cloud_launch(x, B, N, pts0, st);
        else rc = prologue_launch(x, B, N, pts0, centroid, scale0, F(p.o_pro), st);
    }
    if (rc != LS_OK) return rc;
    // ---- FPS chain on the side stream: depends on xyz only, overlaps with layers 0..first down-sample
    hipStream_t fs = m->fps_side ? m->side : st;
    if (p.nlevels > 0) {
        if (m->fps_side) {
            LS_HIP_CHECK(hipEventRecord(m->ev_fork, st));
            LS_HIP_CHECK(hipStreamWaitEvent(fs, m->ev_fork, 0));
        }
        size_t toff = 0;
        for (int l = 0; l < p.nlevels; ++l) {
            int32_t* idx = trace_fps ? trace_fps + toff : I(p.o_fps[l + 1]);
            toff += (size_t)B * p.levelN[l + 1];
            {
                PROF(LS_K_FPS, l, fs);
                rc = fps_dispatch(F(p.o_pts[l]), nullptr, B, p.levelN[l], p.levelN[l + 1], flags, idx, F(p.o_pts[l + 1]),
                                  p.fpsws_bytes ? (void*)(ws + p.o_fpsws) : nullptr, p.fpsws_bytes, fs);
            }
            if (rc != LS_OK) return rc;
            if (m->fps_side) LS_HIP_CHECK(hipEventRecord(m->ev_fps[l], fs));
        }
        if (m->fps_side) LS_HIP_CHECK(hipEventRecord(m->ev_join, fs));
    }

    float* cur = F(p.o_fA);
    float* nxt = F(p.o_fB);
    float* msg = F(p.o_msg);
    float* T = F(p.o_T);
    bool joined = false;
    size_t knn_off = 0, fps_off = 0;
    const float* cur_rm = nullptr;        // row maxima of `cur` ([rows][cur_rm_parts]) when the kernel that wrote it emitted them (GemmAux)
    int cur_rm_parts = 0;
    for (int i = 0; i < p.L; ++i) {
        if (i == m->debug_layers) {
            static bool printed = false;
            if (!printed) {
                printed = true;
                fprintf(stderr, "LS_PLAN knn=%zu knn2=%zu knns=%zu fA=%zu fB=%zu msg=%zu T=%zu TG=%zu g=%zu G=%zu Tc=%zu gws=%zu total=%zu\n",
                        p.o_knn, p.o_knn2, p.o_knns, p.o_fA, p.o_fB, p.o_msg, p.o_T, p.o_TG, p.o_g, p.o_G, p.o_Tc, p.o_gws, p.total);
            }
            if (p.nlevels > 0 && !joined && m->fps_side) LS_HIP_CHECK(hipStreamWaitEvent(st, m->ev_join, 0));
            return LS_OK;
        }
        const int Ns = p.Ns[i], Nd = p.Nd[i], Co = d.feat_dim[i];
        const int32_t* dst_rows = nullptr;
        if (p.level[i] >= 0) {
            if (m->fps_side) LS_HIP_CHECK(hipStreamWaitEvent(st, m->ev_fps[p.level[i]], 0));   // this layer's level only
            joined = p.level[i] == p.nlevels - 1;                                            // the last level joins the whole side chain
            dst_rows = trace_fps ? trace_fps + fps_off : I(p.o_fps[p.level[i] + 1]);
            fps_off += (size_t)B * Nd;
        }
        int32_t* knn = trace_knn ? trace_knn + knn_off : I((i & 1) ? p.o_knn2 : p.o_knn);  // ping-pong: layer i+1 is seeded by layer i
        knn_off += (size_t)B * Nd * 16;
        const bool attn = i >= d.atten_start_layer;
        const bool glob = i >= d.res_global_start_layer;
        float* mp = glob ? msg : nxt;
        int msg_rm_parts = 0, msg_cs_rows = 0;   // side products of the kernel that wrote the message (0: none)
        if (i == 0) {
            { PROF(LS_K_KNN, i, st); rc = knn_dispatch(pts0, pts0, nullptr, B, Nd, Ns, Ns, 1, 16, flags, knn, nullptr, ws + p.o_knns, nullptr, 0, 0, st); }
            if (rc != LS_OK) return rc;
            LS_REQUIRE(!attn, "encoder: attention at layer 0 unsupported (atten_start_layer >= 1)");
            { PROF(LS_K_EDGE_L0, i, st); rc = edge_l0_launch(pts0, knn, W + d.off_l0, B, Ns, Co, d.neg_slope, mp, st); }
            if (rc != LS_OK) return rc;
        } else {
            const int Cin = layer_cin(d, i);
            const EdgePlan ep = layer_edge_plan(m, i, B, Ns, Nd, dst_rows != nullptr, glob);
            // fork: the table GEMM(s) depend only on the layer input, like the k-NN -> run them on side2 (matrix cores /
            // HBM writes) concurrently with the VALU-bound k-NN on the caller's stream; join before the edge kernel.
            hipStream_t gs = m->overlap_gemm ? m->side2 : st;
            if (m->overlap_gemm) {
                LS_HIP_CHECK(hipEventRecord(m->ev_feat[i], st));
                LS_HIP_CHECK(hipStreamWaitEvent(gs, m->ev_feat[i], 0));
            }
            rc = edge_tables_run(m, i, ep, cur, dst_rows, B, Ns, Nd, T, gs, cur_rm, cur_rm_parts);
            if (rc != LS_OK) return rc;
            if (m->overlap_gemm) LS_HIP_CHECK(hipEventRecord(m->ev_tab[i], gs));
            {   // (no hints: the fused k-NN kernel derives its thresholds from its own sweep -- knn_mfma.hip)
                PROF(LS_K_KNN, i, st);
                rc = knn_dispatch(cur, cur, dst_rows, B, Nd, Ns, Ns, Cin, 16, flags, knn, nullptr, ws + p.o_knns, nullptr, 0, 0, st);
            }
            if (rc != LS_OK) return rc;
            if (m->profiling && m->knn_stats && knn_plan(knn_traits(true, B, Nd, Ns, Ns, Cin, 16, flags, false, true)).stats) {   // (the plan of the call above)
                // (outside the launch's event bracket) how many candidates got a canonical distance: ls_profile_knn_stats
                rc = knn_sweep_stats_launch(ws + p.o_knns, B, Nd, m->knn_stats + 2 * i, st);
                if (rc != LS_OK) return rc;
            }
            if (m->overlap_gemm) LS_HIP_CHECK(hipStreamWaitEvent(st, m->ev_tab[i], 0));
            rc = edge_layer_run(m, i, ep, T, cur, knn, dst_rows, B, Ns, Nd, mp, st, F(p.o_rm_msg), F(p.o_cs));
            if (rc != LS_OK) return rc;
            msg_rm_parts = ep.rowmax_parts; msg_cs_rows = ep.cs_rows;
        }
        cur_rm = nullptr; cur_rm_parts = 0;
        if (glob) {
            bool out_rm = false;
            rc = global_conv(m, i, msg, B, Nd, F(p.o_g), F(p.o_G), F(p.o_TG), F(p.o_gws), nxt, st, msg_rm_parts ? F(p.o_rm_msg) : nullptr,
                             F(p.o_rm_out[i & 1]), &out_rm, msg_rm_parts, F(p.o_cs), msg_cs_rows);
            if (rc != LS_OK) return rc;
            if (out_rm) { cur_rm = F(p.o_rm_out[i & 1]); cur_rm_parts = Co / 32; }
        }
        std::swap(cur, nxt);
    }
    if (p.nlevels > 0 && !joined && m->fps_side) LS_HIP_CHECK(hipStreamWaitEvent(st, m->ev_join, 0));

    // ---- tail
    return encoder_tail(m, cur, B, p.NP, F(p.o_Tc), F(p.o_gws), pre_normalised ? nullptr : centroid, pre_normalised ? nullptr : scale0,
                        z_so3, z_inv, s_out, t_out, st, cur_rm, cur_rm_parts);
}


// One encode = ~170 kernel launches, 1.35 ms of host time per 64-instance step in round 1 (the GPU needs 1.6 ms).  The launch
// sequence depends only on (B, N, flags, workspace), so it is CAPTURED once per such key into a hipGraph (stream capture incl. the
// fork / join onto the handle's side streams) and replayed: a call is then one D2D copy of x into the workspace, one graph launch
// and one tiny kernel that scatters the packed codes to the caller's output tensors (the graph itself only ever touches fixed
// addresses inside the caller's workspace, so the caller's x / output pointers may change freely between calls).
static int encode_graphed(ls_model_t* m, const EncPlan& p, const float* x, int B, int N, int pre_normalised, unsigned flags, float* z_so3,
                          float* z_inv, float* s_out, float* t_out, void* workspace, size_t workspace_bytes, hipStream_t st) {
    char* ws = (char*)workspace;
    float* xin = (float*)(ws + p.o_xin);
    float* packed = (float*)(ws + p.o_out);
    const int c = m->d.c_dim;
    float* g_zso3 = packed;
    float* g_zinv = g_zso3 + (size_t)B * c * 3;
    float* g_s = g_zinv + (size_t)B * c;
    float* g_t = g_s + B;
    ls_model::EncGraph* hit = nullptr;
    for (auto& g : m->graphs)
        if (g.ws == workspace && g.ws_bytes == workspace_bytes && g.B == B && g.N == N && g.pre == pre_normalised && g.flags == flags && g.st == st) hit = &g;
    if (!hit) {
        hipGraph_t graph = nullptr;
        hipGraphExec_t exec = nullptr;
        hipError_t e = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal);
        if (e != hipSuccess) { (void)hipGetLastError(); m->graph_broken = true; return 1; }
        const int rc = encode_enqueue(m, p, xin, B, N, pre_normalised, flags, g_zso3, g_zinv, g_s, g_t, nullptr, nullptr, workspace, st);
        e = hipStreamEndCapture(st, &graph);
        if (rc != LS_OK || e != hipSuccess || !graph) { (void)hipGetLastError(); if (graph) (void)hipGraphDestroy(graph); m->graph_broken = true; return rc != LS_OK ? rc : 1; }
        e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
        if (e != hipSuccess) { (void)hipGetLastError(); (void)hipGraphDestroy(graph); m->graph_broken = true; return 1; }
        if (m->graphs.size() >= 8) {   // a handle serves a few shapes; drop the oldest beyond that
            (void)hipGraphExecDestroy(m->graphs.front().exec);
            (void)hipGraphDestroy(m->graphs.front().graph);
            m->graphs.erase(m->graphs.begin());
        }
        m->graphs.push_back(ls_model::EncGraph{workspace, workspace_bytes, B, N, pre_normalised, flags, st, graph, exec});
        hit = &m->graphs.back();
    }
    LS_HIP_CHECK(hipMemcpyAsync(xin, x, (size_t)B * 3 * N * sizeof(float), hipMemcpyDeviceToDevice, st));
    LS_HIP_CHECK(hipGraphLaunch(hit->exec, st));
    return scatter_codes_launch(packed, B, c, z_so3, z_inv, s_out, t_out, st);
}

extern "C" {

int ls_encode(ls_model_t* m, const float* x, int B, int N, int pre_normalised, unsigned flags, float* z_so3, float* z_inv,
              float* s_out, float* t_out, int32_t* trace_knn, int32_t* trace_fps, void* workspace, size_t workspace_bytes,
              void* stream) {
    LS_REQUIRE(m && x && z_so3 && z_inv && s_out && t_out && workspace, "encode: null argument");
    LS_REQUIRE(B > 0 && N >= 16, "encode: need B>0, N>=16 (B=%d N=%d)", B, N);
    EncPlan p;
    int rc = make_plan(m->d, B, N, p);
    if (rc != LS_OK) return rc;
    if (workspace_bytes < p.total) { set_error("encode: workspace %zu < required %zu", workspace_bytes, p.total); return LS_ERR_WORKSPACE; }
    hipStream_t st = (hipStream_t)stream;
    // the captured path: not while per-launch profiling events or the index traces are requested (tests / bench's profiled pass), not
    // on the legacy NULL stream (it cannot be captured), and not with the debugging knobs
    if (m->use_graph && !m->graph_broken && !m->profiling && !trace_knn && !trace_fps && st != nullptr && m->debug_layers < 0) {
        rc = encode_graphed(m, p, x, B, N, pre_normalised, flags, z_so3, z_inv, s_out, t_out, workspace, workspace_bytes, st);
        if (rc <= 0) return rc;    // 0 = done, < 0 = error; 1 = capture unavailable on this runtime: fall through to the direct path
    }
    return encode_enqueue(m, p, x, B, N, pre_normalised, flags, z_so3, z_inv, s_out, t_out, trace_knn, trace_fps, workspace, st);
}

// ------------------------------------------------------------------------------------------------ per-operator exports
static int check_layer(const ls_model_t* m, int layer, bool want_attn, const char* who) {
    LS_REQUIRE(m, "%s: null model", who);
    LS_REQUIRE(layer >= 0 && layer < m->d.num_layers, "%s: layer %d out of range", who, layer);
    LS_REQUIRE((layer >= m->d.atten_start_layer) == want_attn, "%s: layer %d is %s layer", who, layer, want_attn ? "a mean-pool" : "an attention");
    return LS_OK;
}
// the workspace of an exported edge-conv layer is one piece: its table area (+ 4 floats the size has always counted)
size_t ls_vn_edgeconv_workspace_bytes(const ls_model_t* m, int layer, int B, int Ns, int Nd, int has_dst_rows) {
    if (!m || layer < 0 || layer >= m->d.num_layers || B <= 0) return 0;
    Arena a(nullptr);
    a.take<float>((layer == 0 ? 0 : edge_table_floats(layer >= m->d.atten_start_layer, m->d.feat_dim[layer], B, Ns, Nd, has_dst_rows != 0)) + 4);
    return a.bytes();
}
static int edgeconv_export(ls_model_t* m, int layer, const float* src_f, const int32_t* knn, const int32_t* dst_rows, int B, int Ns, int Nd,
                           float* out, void* workspace, size_t workspace_bytes, hipStream_t st, const char* who) {
    LS_REQUIRE(src_f && knn && out, "%s: null argument", who);
    LS_REQUIRE(B > 0 && Ns >= m->d.num_knn && Nd > 0 && (dst_rows || Nd == Ns), "%s: bad sizes (B=%d Ns=%d Nd=%d)", who, B, Ns, Nd);
    LS_REQUIRE(m->d.num_knn == 16, "%s: num_knn=%d unsupported (16)", who, m->d.num_knn);
    if (layer == 0) {
        LS_REQUIRE(!dst_rows, "%s: layer 0 does not down-sample", who);
        PROF(LS_K_EDGE_L0, 0, st);
        return edge_l0_launch(src_f, knn, m->blob + m->d.off_l0, B, Ns, m->d.feat_dim[0], m->d.neg_slope, out, st);
    }
    const size_t need = ls_vn_edgeconv_workspace_bytes(m, layer, B, Ns, Nd, dst_rows != nullptr);
    if (!workspace || workspace_bytes < need) { set_error("%s: workspace %zu < required %zu", who, workspace_bytes, need); return LS_ERR_WORKSPACE; }
    const EdgePlan ep = layer_edge_plan(m, layer, B, Ns, Nd, dst_rows != nullptr, false);
    // LS_OPT_DEBUG_EDGE = 2: the tables are already in the workspace; 1: the tables only
    const int rc = m->debug_edge == 2 ? LS_OK : edge_tables_run(m, layer, ep, src_f, dst_rows, B, Ns, Nd, (float*)workspace, st);
    if (rc != LS_OK || m->debug_edge == 1) return rc;
    return edge_layer_run(m, layer, ep, (const float*)workspace, src_f, knn, dst_rows, B, Ns, Nd, out, st);
}
int ls_vn_edgeconv_pool_f32(ls_model_t* m, int layer, const float* src_f, const int32_t* knn, const int32_t* dst_rows, int B, int Ns, int Nd,
                            float* out, void* workspace, size_t workspace_bytes, void* stream) {
    int rc = check_layer(m, layer, false, "vn_edgeconv_pool");
    if (rc != LS_OK) return rc;
    return edgeconv_export(m, layer, src_f, knn, dst_rows, B, Ns, Nd, out, workspace, workspace_bytes, (hipStream_t)stream, "vn_edgeconv_pool");
}
int ls_vn_edgeconv_attn_f32(ls_model_t* m, int layer, const float* src_f, const int32_t* knn, const int32_t* dst_rows, int B, int Ns, int Nd,
                            float* out, void* workspace, size_t workspace_bytes, void* stream) {
    int rc = check_layer(m, layer, true, "vn_edgeconv_attn");
    if (rc != LS_OK) return rc;
    return edgeconv_export(m, layer, src_f, knn, dst_rows, B, Ns, Nd, out, workspace, workspace_bytes, (hipStream_t)stream, "vn_edgeconv_attn");
}

struct LnaPlan { float *g, *G, *TG, *gws, *rm; size_t total; };
static LnaPlan lna_plan(const ls_model_desc& d, void* workspace, int layer, int B, int N) {   // a null workspace: a sizing pass
    const size_t Co = (size_t)d.feat_dim[layer];
    LnaPlan q{};
    Arena a(workspace);
    q.g = a.take<float>((size_t)B * 3 * Co);
    q.G = a.take<float>((size_t)B * 3 * 4 * Co);
    q.TG = a.take<float>((size_t)B * N * 3 * 2 * Co);
    q.gws = a.take<float>(global_conv_gws_floats(d, layer, B, N) + 64);   // split-K slabs and their 256-byte tail
    q.rm = a.take<float>((size_t)B * N * 3);
    q.total = a.bytes();
    return q;
}
size_t ls_vn_lna_workspace_bytes(const ls_model_t* m, int layer, int B, int N) {
    if (!m || layer < m->d.res_global_start_layer || layer >= m->d.num_layers || B <= 0 || N <= 0) return 0;
    return lna_plan(m->d, nullptr, layer, B, N).total;
}
int ls_vn_lna_f32(ls_model_t* m, int layer, const float* f, int B, int N, float* out, void* workspace, size_t workspace_bytes, void* stream) {
    LS_REQUIRE(m && f && out && workspace, "vn_lna: null argument");
    LS_REQUIRE(layer >= m->d.res_global_start_layer && layer < m->d.num_layers, "vn_lna: layer %d has no residual global conv", layer);
    LS_REQUIRE(B > 0 && N > 0, "vn_lna: empty problem");
    const LnaPlan q = lna_plan(m->d, workspace, layer, B, N);
    if (workspace_bytes < q.total) { set_error("vn_lna: workspace %zu < required %zu", workspace_bytes, q.total); return LS_ERR_WORKSPACE; }
    const float* rm = nullptr;
    if (m->glob_fuse == 2) {   // the message's exact row maxima, as the encoder's attention kernels hand them over (GemmAux::a_rowmax)
        const int Co = m->d.feat_dim[layer];
        const int rc = gemm_rowmax_launch(f, B * N * 3, Co, Co, q.rm, (hipStream_t)stream);
        if (rc != LS_OK) return rc;
        rm = q.rm;
    }
    return global_conv(m, layer, f, B, N, q.g, q.G, q.TG, q.gws, out, (hipStream_t)stream, rm);
}
int ls_vn_lna_ex_f32(ls_model_t* m, int layer, const float* f, int B, int N, const float* a_rowmax, int a_parts, float* out_rowmax, int* rowmax_written,
                     float* out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!a_rowmax && !out_rowmax) {
        if (rowmax_written) *rowmax_written = 0;
        return ls_vn_lna_f32(m, layer, f, B, N, out, workspace, workspace_bytes, stream);
    }
    LS_REQUIRE(m && f && out && workspace, "vn_lna_ex: null argument");
    LS_REQUIRE(layer >= m->d.res_global_start_layer && layer < m->d.num_layers, "vn_lna_ex: layer %d has no residual global conv", layer);
    LS_REQUIRE(B > 0 && N > 0, "vn_lna_ex: empty problem");
    LS_REQUIRE(!a_rowmax || a_parts >= 1, "vn_lna_ex: a_rowmax needs a_parts >= 1");
    const LnaPlan q = lna_plan(m->d, workspace, layer, B, N);
    if (workspace_bytes < q.total) { set_error("vn_lna_ex: workspace %zu < required %zu", workspace_bytes, q.total); return LS_ERR_WORKSPACE; }
    bool written = false;
    const int rc = global_conv(m, layer, f, B, N, q.g, q.G, q.TG, q.gws, out, (hipStream_t)stream, a_rowmax, out_rowmax, &written, a_rowmax ? a_parts : 1);
    if (rowmax_written) *rowmax_written = written;
    return rc;
}

// the workspace of the exported tail: conv_c's output, then the split-K slabs of that GEMM and their 256-byte tail.  A null workspace: a
// sizing pass.  The size has always ended with that tail, unpadded.
struct TailWs { float *Tc, *gws; size_t bytes; };
static TailWs tail_ws_layout(const ls_model_desc& d, void* workspace, int B, int NP) {
    const int Cl = d.feat_dim[d.num_layers - 1], Cdp = pad4(d.c_dim + 1);
    Arena a(workspace);
    TailWs w;
    w.Tc = a.take<float>((size_t)B * NP * 3 * Cdp);
    w.gws = a.take<float>(gemm_scratch_floats(B * NP * 3, Cdp, Cl) + 64);
    w.bytes = a.bytes_unpadded();
    return w;
}
size_t ls_encoder_tail_workspace_bytes(const ls_model_t* m, int B, int NP) {
    return (!m || B <= 0 || NP <= 0) ? 0 : tail_ws_layout(m->d, nullptr, B, NP).bytes;
}
int ls_encoder_tail_f32(ls_model_t* m, const float* f, const float* centroid, const float* scale0, int B, int NP, float* z_so3, float* z_inv,
                        float* s, float* t, void* workspace, size_t workspace_bytes, void* stream) {
    LS_REQUIRE(m && f && z_so3 && z_inv && s && t && workspace, "encoder_tail: null argument");
    LS_REQUIRE(B > 0 && NP > 0, "encoder_tail: empty problem");
    LS_REQUIRE((centroid == nullptr) == (scale0 == nullptr), "encoder_tail: centroid and scale0 go together");
    const TailWs w = tail_ws_layout(m->d, workspace, B, NP);
    if (workspace_bytes < w.bytes) { set_error("encoder_tail: workspace %zu < required %zu", workspace_bytes, w.bytes); return LS_ERR_WORKSPACE; }
    return encoder_tail(m, f, B, NP, w.Tc, w.gws, centroid, scale0, z_so3, z_inv, s, t, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------------ SDF decode
static bool dec_xyz(const ls_model_desc& d) { return d.dec_input == LS_DEC_XYZ; }
// width of the decoder input u: [z_inv | <q, z_so3> | |q|] (LS_DEC_INNER) or [z_inv | query] (LS_DEC_XYZ)
static int dec_in_width(const ls_model_desc& d) { return dec_xyz(d) ? d.c_dim + 3 : 2 * d.c_dim + 1; }
static int dec_out(const ls_model_desc& d, int l) {  // padded output width of linear layer l
    const int nl = d.dec_num_linear;
    if (l == nl - 1) return 1;
    if (d.dec_latent_in >= 0 && l + 1 == d.dec_latent_in) return pad4(d.dec_width - dec_in_width(d));
    return d.dec_width;
}
// the per-instance table of the code-fed layer l that multiplies the query (sdf_prep_launch's so3_t argument)
static const float* dec_q_table(const ls_model_t* m, int l) {
    return m->blob + (dec_xyz(m->d) ? m->d.off_dec_xyz_t[l] : m->d.off_dec_so3_t[l]);
}

// split-K scratch (floats) that covers every GEMM of the decoder forward and backward at `rows` query rows
static int sdf_rm_parts(int w) { return std::max(sdf_affine_rowmax_parts(w), gemm_rowmax_parts(w)); }
static size_t sdf_gemm_scratch(const ls_model_desc& d, long long rows) {
    size_t mx = 0;
    int kin = d.dec_width;
    for (int l = 1; l < d.dec_num_linear - 1; ++l) {
        const int outw = dec_out(d, l);
        mx = std::max(mx, gemm_scratch_floats((int)rows, outw, kin));   // forward: [rows,kin] x [outw,kin]^T
        mx = std::max(mx, gemm_scratch_floats((int)rows, kin, outw));   // backward: [rows,outw] x [kin,outw]^T
        kin = outw;
    }
    return mx;
}

struct SdfBuffers {
    float *A0, *A4, *b0, *b4;
    float* h[12];       // output of linear layer l (post-ReLU); inference: two ping-pong buffers
    float *dzA, *dzB, *dA0, *dA4, *db0, *db4, *dQ;
    float* gws;         // split-K scratch for the under-filled GEMMs (NULL when the grid is large enough)
    float* rm[2];       // row maxima of the activations / gradients, ping-pong: [rows][sdf_rm_parts(w)] (GemmAux)
    size_t bytes;       // of the whole layout
};
// The one statement of the decoder's workspace layout: B instances, `rows` query rows in all (B * M, or R of the ragged form).
// A null `workspace` is a sizing pass: the byte total and null pointers.  train: every layer's activations are kept for the backward pass, plus its scratch.
static SdfBuffers sdf_buffers(const ls_model_desc& d, void* workspace, int B, long long rows, bool train, bool allow_splitk = true) {
    SdfBuffers sb{};
    const int w = d.dec_width, nl = d.dec_num_linear;
    const size_t R = (size_t)rows;
    Arena a(workspace);
    sb.A0 = a.take<float>((size_t)B * w * 4);
    sb.A4 = a.take<float>((size_t)B * w * 4);
    sb.b0 = a.take<float>((size_t)B * w);
    sb.b4 = a.take<float>((size_t)B * w);
    if (!train) {
        float* hA = a.take<float>(R * w);
        float* hB = a.take<float>(R * w);
        for (int l = 0; l < nl - 1; ++l) sb.h[l] = (l & 1) ? hB : hA;
        // inference never splits K: a query's SDF must not depend on how many other queries share the call (MISE evaluates
        // the same lattice point in calls of very different sizes; split-K changes the fp32 summation order)
        sb.gws = nullptr;
    } else {
        for (int l = 0; l < nl - 1; ++l) sb.h[l] = a.take<float>(R * w);
        sb.dzA = a.take<float>(R * w);
        sb.dzB = a.take<float>(R * w);
        sb.dA0 = a.take<float>((size_t)B * w * 4);
        sb.dA4 = a.take<float>((size_t)B * w * 4);
        sb.db0 = a.take<float>((size_t)B * w);
        sb.db4 = a.take<float>((size_t)B * w);
        sb.dQ = a.take<float>(R * 4);
        // split-K slabs (small M only) and their 256-byte tail; the tail is reserved even where no GEMM splits (the size always counted it)
        const size_t scratch = sdf_gemm_scratch(d, rows);
        float* gws = a.take<float>(scratch + 64);
        sb.gws = scratch && allow_splitk ? gws : nullptr;
    }
    sb.rm[0] = a.take<float>(R * sdf_rm_parts(w));
    sb.rm[1] = a.take<float>(R * sdf_rm_parts(w));
    sb.bytes = a.bytes();
    return sb;
}
static size_t sdf_bytes(const ls_model_t* m, int B, long long rows, bool train) {
    return m && m->d.dec_num_linear > 0 ? sdf_buffers(m->d, nullptr, B, rows, train).bytes : 0;
}
size_t ls_sdf_workspace_bytes(const ls_model_t* m, int B, int M) { return sdf_bytes(m, B, (long long)B * M, false); }
// Ragged batch: R query rows of B instances packed back to back (rows of one instance contiguous), row_inst[r] = instance of row r.
size_t ls_sdf_rows_workspace_bytes(const ls_model_t* m, int B, long long R) { return sdf_bytes(m, B, R, false); }
size_t ls_sdf_train_workspace_bytes(const ls_model_t* m, int B, int M) { return sdf_bytes(m, B, (long long)B * M, true); }

// Operand range of the decoder's GEMMs (gemm.hip, GemmAux): every kernel that writes an activation (forward) or a gradient (backward) also
// writes its row maxima, and the GEMM that reads it takes them instead of scanning its A rows; the weights carry theirs from ls_model_create.
// The maxima ping-pong between two buffers; the chain is off in the sdf_bf16x2 mode.
struct RowMaxChain {
    float* const* rm;
    bool on;
    int cur = 1, parts = 0;   // rm[cur] holds the maxima of the current operand, `parts` per row, when `have`
    bool have = false;
    // the GEMM about to be launched reads the current operand
    void operand(GemmAux& ax) const { ax.a_rowmax = have ? rm[cur] : nullptr; ax.a_parts = have ? parts : 0; }
    // the launch that produces the next operand writes its maxima, n per row, to the returned buffer (NULL: chain off)
    float* emit(int n) {
        if (!on) return nullptr;
        cur ^= 1; parts = n; have = true;
        return rm[cur];
    }
    // ... or writes none (a split-K launch)
    void emit_none() { have = false; }
};

// row_inst == nullptr: B instances x rows / B rows each; else row r belongs to instance row_inst[r]
static int sdf_forward(ls_model_t* m, const SdfBuffers& sb, const float* query, const float* z_so3, const float* z_inv, const float* s,
                       const float* t, int B, long long rows, float* sdf, hipStream_t st, const int32_t* row_inst = nullptr) {
    const ls_model_desc& d = m->d;
    const int w = d.dec_width, L = d.c_dim, nl = d.dec_num_linear, li = d.dec_latent_in;
    const bool xyz = dec_xyz(d);   // LS_DEC_XYZ: z_so3, s and t are not read
    const float* W = m->blob;
    int rc;
    {
        PROF(LS_K_SDF_PREP, 0, st);
        rc = sdf_prep_launch(W + d.off_dec_inv_t[0], dec_q_table(m, 0), W + d.off_dec_len[0], W + d.off_dec_b[0], z_so3,
                             z_inv, B, L, w, sb.A0, sb.b0, xyz, st);
        if (rc == LS_OK && li >= 0)
            rc = sdf_prep_launch(W + d.off_dec_inv_t[li], dec_q_table(m, li), W + d.off_dec_len[li], W + d.off_dec_b[li],
                                 z_so3, z_inv, B, L, w, sb.A4, sb.b4, xyz, st);
    }
    if (rc != LS_OK) return rc;
    // layer 0: pure affine in (q, |q|) (LS_DEC_XYZ: in the raw query)
    RowMaxChain rmc{sb.rm, !m->sdf_bf16x2};
    { PROF(LS_K_SDF_AFFINE, 0, st);
      rc = sdf_affine_launch(query, row_inst, s, t, sb.A0, sb.b0, B, rows, w, w, 0, sb.h[0], xyz, st, rmc.emit(sdf_affine_rowmax_parts(w))); }
    if (rc != LS_OK) return rc;
    // opt-in two-piece products (decoder throughput mode); a launch that may split K keeps the default product
    const bool two_piece = m->sdf_bf16x2 && !sb.gws;
    int kin = w;
    for (int l = 1; l < nl - 1; ++l) {
        const int outw = dec_out(d, l);
        const float* cur = sb.h[l - 1];
        float* nxt = sb.h[l];
        Gemm g;
        g.A = cur; g.lda = w; g.W = W + d.off_dec_w[l]; g.ldw = kin; g.out = nxt; g.ldc = w; g.M = (int)rows; g.N = outw; g.K = kin; g.scratch = sb.gws;
        if (two_piece) g.pieces = 2;   // (takes no operand ranges or planes)
        else { g.aux = aux_w(m, g.W, outw, kin); rmc.operand(g.aux); }
        if (l == li) {
            { PROF(LS_K_GEMM_SDF, l, st);
              rc = gemm_run(g, st); }
            if (rc != LS_OK) return rc;
            PROF(LS_K_SDF_AFFINE, l, st);
            rc = sdf_affine_launch(query, row_inst, s, t, sb.A4, sb.b4, B, rows, w, w, 1, nxt, xyz, st, rmc.emit(sdf_affine_rowmax_parts(w)));
        } else {
            PROF(LS_K_GEMM_SDF, l, st);
            g.bias = W + d.off_dec_b[l]; g.relu = 1;
            if (!gemm_plan(gemm_traits(g)).writes_out_rowmax) rmc.emit_none();
            else g.aux.out_rowmax = rmc.emit(gemm_rowmax_parts(outw));
            rc = gemm_run(g, st);
        }
        if (rc != LS_OK) return rc;
        kin = outw;
    }
    PROF(LS_K_SDF_OUT, nl - 1, st);
    return sdf_out_launch(sb.h[nl - 2], w, kin, W + d.off_dec_w[nl - 1], W + d.off_dec_b[nl - 1], rows, sdf, st);
}

// The checks the decoder's entry points share; `op` names the operator in the messages.  args: the handle and the operator's pointers are
// there (LS_DEC_XYZ reads no z_so3, s or t).  n: rows per instance, or all R rows of the ragged form.
static int sdf_entry(const ls_model_t* m, const char* op, bool args, int B, long long n, bool ragged, bool train, size_t workspace_bytes) {
    LS_REQUIRE(args, "%s: null argument", op);
    LS_REQUIRE(m->d.dec_num_linear >= 3, "%s: model has no decoder packed", op);
    if (ragged) LS_REQUIRE(B > 0 && n > 0 && n < (1ll << 31), "%s: empty or oversized problem", op);
    else LS_REQUIRE(B > 0 && n > 0, "%s: empty problem", op);
    // the GEMMs and their split-K sizing take the row count as an int (Gemm::M, gemm_scratch_floats): said here, before anything is sized
    if (!ragged) LS_REQUIRE((long long)B * n < (1ll << 31), "%s: B=%d x M=%lld rows too many for one call (< 2^31): split the queries", op, B, n);
    const size_t need = sdf_bytes(m, B, ragged ? n : B * n, train);
    if (workspace_bytes < need) { set_error("%s: workspace %zu < required %zu", op, workspace_bytes, need); return LS_ERR_WORKSPACE; }
    return LS_OK;
}

int ls_sdf_decode(ls_model_t* m, const float* query, const float* z_so3, const float* z_inv, const float* s, const float* t,
                  int B, int M, float* sdf, void* workspace, size_t workspace_bytes, void* stream) {
    const int rc = sdf_entry(m, "sdf_decode", m && query && z_inv && sdf && workspace && (dec_xyz(m->d) || (z_so3 && s && t)), B, M, false, false,
                             workspace_bytes);
    if (rc != LS_OK) return rc;
    const long long rows = (long long)B * M;
    return sdf_forward(m, sdf_buffers(m->d, workspace, B, rows, false), query, z_so3, z_inv, s, t, B, rows, sdf, (hipStream_t)stream);
}

// Workspace: ls_sdf_rows_workspace_bytes(m, B, R).
int ls_sdf_decode_rows(ls_model_t* m, const float* query, const int32_t* row_inst, const float* z_so3, const float* z_inv, const float* s,
                       const float* t, int B, long long R, float* sdf, void* workspace, size_t workspace_bytes, void* stream) {
    const int rc = sdf_entry(m, "sdf_decode_rows", m && query && row_inst && z_inv && sdf && workspace && (dec_xyz(m->d) || (z_so3 && s && t)), B, R,
                             true, false, workspace_bytes);
    if (rc != LS_OK) return rc;
    return sdf_forward(m, sdf_buffers(m->d, workspace, B, R, false), query, z_so3, z_inv, s, t, B, R, sdf, (hipStream_t)stream, row_inst);
}

// forward that keeps every layer's activations in `workspace` for ls_sdf_backward
int ls_sdf_decode_train(ls_model_t* m, const float* query, const float* z_so3, const float* z_inv, const float* s, const float* t,
                        int B, int M, float* sdf, void* workspace, size_t workspace_bytes, void* stream) {
    const int rc = sdf_entry(m, "sdf_decode_train", m && query && z_inv && sdf && workspace && (dec_xyz(m->d) || (z_so3 && s && t)), B, M, false, true,
                             workspace_bytes);
    if (rc != LS_OK) return rc;
    const long long rows = (long long)B * M;
    return sdf_forward(m, sdf_buffers(m->d, workspace, B, rows, true, m->train_splitk), query, z_so3, z_inv, s, t, B, rows, sdf, (hipStream_t)stream);
}

static int build_dec_wt(ls_model_t* m, hipStream_t st) {   // transposed main weights of layers 1 .. nl-2
    if (m->dec_wt) return LS_OK;
    const ls_model_desc& d = m->d;
    const int nl = d.dec_num_linear, w = d.dec_width;
    size_t total = 0;
    int kin = w;
    for (int l = 1; l < nl - 1; ++l) { const int outw = dec_out(d, l); m->dec_wt_off[l] = total; total += (size_t)kin * outw; kin = outw; }
    LS_HIP_CHECK(hipMalloc((void**)&m->dec_wt, total * sizeof(float)));
    kin = w;
    for (int l = 1; l < nl - 1; ++l) {
        const int outw = dec_out(d, l);
        int rc = transpose_launch(m->blob + d.off_dec_w[l], outw, kin, m->dec_wt + m->dec_wt_off[l], st);   // W [out][kin] -> [kin][out]
        if (rc != LS_OK) return rc;
        kin = outw;
    }
    std::vector<WSpec> specs;
    kin = w;
    for (int l = 1; l < nl - 1; ++l) { const int outw = dec_out(d, l); specs.push_back({m->dec_wt + m->dec_wt_off[l], (size_t)kin, outw}); kin = outw; }
    return wmax_register(m, specs, &m->wmax_pool_t, &m->wplanes_pool_t, st);
}

// Gradients of sum(grad_sdf * sdf) w.r.t. the code and the query points, after ls_sdf_decode_train on the SAME arguments and
// workspace.  grad_query is optional; grad_z_so3 / grad_z_inv may be omitted TOGETHER (pose refinement with a fixed code).
// LS_DEC_XYZ: z_so3, s, t are not read and each of grad_z_so3, grad_s, grad_t may be NULL; where given they are set to exact zeros
// (the SDF does not depend on them); need_code follows grad_z_inv alone.
int ls_sdf_backward(ls_model_t* m, const float* query, const float* z_so3, const float* z_inv, const float* s, const float* t, int B,
                    int M, const float* sdf, const float* grad_sdf, void* workspace, size_t workspace_bytes, float* grad_query,
                    float* grad_z_so3, float* grad_z_inv, float* grad_s, float* grad_t, void* stream) {
    int rc = sdf_entry(m, "sdf_backward",
                       m && query && z_inv && sdf && grad_sdf && workspace && (dec_xyz(m->d) || (z_so3 && s && t && grad_s && grad_t)), B, M, false, true,
                       workspace_bytes);
    if (rc != LS_OK) return rc;
    const ls_model_desc& d = m->d;
    const bool xyz = dec_xyz(d);
    LS_REQUIRE(xyz || (grad_z_so3 != nullptr) == (grad_z_inv != nullptr), "sdf_backward: grad_z_so3 and grad_z_inv are given or omitted together");
    const bool need_code = grad_z_inv != nullptr;   // a pose refinement with a fixed code skips the code-gradient reductions
    hipStream_t st = (hipStream_t)stream;
    if (xyz) {   // the invariant decoder does not read z_so3, s or t: their gradients are exact zeros
        if (grad_z_so3) LS_HIP_CHECK(hipMemsetAsync(grad_z_so3, 0, (size_t)B * d.c_dim * 3 * sizeof(float), st));
        if (grad_s) LS_HIP_CHECK(hipMemsetAsync(grad_s, 0, (size_t)B * sizeof(float), st));
        if (grad_t) LS_HIP_CHECK(hipMemsetAsync(grad_t, 0, (size_t)B * 3 * sizeof(float), st));
    }
    rc = build_dec_wt(m, st);
    if (rc != LS_OK) return rc;
    const long long rows = (long long)B * M;
    const SdfBuffers sb = sdf_buffers(d, workspace, B, rows, true, m->train_splitk);
    const int w = d.dec_width, L = d.c_dim, nl = d.dec_num_linear, li = d.dec_latent_in;
    const float* W = m->blob;
    // widths: out_w[l] = padded output width of layer l
    int outw[12];
    for (int l = 0; l < nl; ++l) outw[l] = l == 0 ? w : dec_out(d, l);
    float* dz = sb.dzA;     // dz_l: gradient w.r.t. the pre-activation of layer l, row stride w
    float* other = sb.dzB;
    // last layer: dz_{nl-2}
    // dz carries its row maxima (here: an upper bound, one per row) from kernel to kernel like the activations of the forward pass
    RowMaxChain rmc{sb.rm, !m->sdf_bf16x2};
    const float* w8max = wmax_for(m, W + d.off_dec_w[nl - 1], 1, outw[nl - 2]);
    rc = sdf_out_bwd_launch(grad_sdf, sdf, W + d.off_dec_w[nl - 1], sb.h[nl - 2], w, outw[nl - 2], rows, dz, st, rmc.emit(1), w8max);
    if (!w8max) rmc.emit_none();   // (the launch writes no bound without the weight's maximum)
    if (rc != LS_OK) return rc;
    bool dq_started = false;
    for (int l = nl - 2; l >= 1; --l) {
        const int kin = outw[l - 1];          // input width of layer l (= padded output width of layer l-1)
        if (l == li) {
            rc = sdf_affine_bwd_launch(query, s, t, dz, sb.A4, B, M, w, w, dq_started ? 1 : 0, sb.dA4, sb.db4, sb.dQ, need_code, xyz, st);
            if (rc != LS_OK) return rc;
            dq_started = true;
        }
        // dh_{l-1} [rows, kin] = dz_l [rows, out_l] . W_l [out_l][kin]  ==  dz_l . (Wt_l [kin][out_l])^T
        // the ReLU derivative [h_{l-1} > 0] is applied in the GEMM's store when the launch does not split K (h and dh share the row stride w)
        const bool fuse_mask = !sb.gws && kin % 4 == 0;
        Gemm g;
        g.A = dz; g.lda = w; g.W = m->dec_wt + m->dec_wt_off[l]; g.ldw = outw[l]; g.out = other; g.ldc = w; g.M = (int)rows; g.N = kin; g.K = outw[l];
        g.aux = aux_w(m, g.W, kin, outw[l]);
        rmc.operand(g.aux);
        if (fuse_mask) {
            g.mask = sb.h[l - 1];
            if (m->sdf_bf16x2) g.pieces = 2;
            g.aux.out_rowmax = rmc.emit(gemm_rowmax_parts(kin));   // after the mask
            rc = gemm_run(g, st);
        } else {
            // (an un-masked, possibly split-K launch: its maxima would still bound the masked values, but a split launch writes none)
            g.scratch = sb.gws;
            if (!gemm_plan(gemm_traits(g)).writes_out_rowmax) rmc.emit_none();
            else g.aux.out_rowmax = rmc.emit(gemm_rowmax_parts(kin));
            rc = gemm_run(g, st);
            if (rc != LS_OK) return rc;
            rc = relu_mask_launch(other, sb.h[l - 1], rows, kin, w, st);
        }
        if (rc != LS_OK) return rc;
        std::swap(dz, other);
    }
    rc = sdf_affine_bwd_launch(query, s, t, dz, sb.A0, B, M, w, w, dq_started ? 1 : 0, sb.dA0, sb.db0, sb.dQ, need_code, xyz, st);
    if (rc != LS_OK) return rc;
    if (need_code) rc = sdf_code_grad_launch(xyz ? nullptr : W + d.off_dec_so3_t[0], W + d.off_dec_inv_t[0], sb.dA0, sb.db0,
                                             li >= 0 && !xyz ? W + d.off_dec_so3_t[li] : nullptr, li >= 0 ? W + d.off_dec_inv_t[li] : nullptr,
                                             sb.dA4, sb.db4, B, L, w, grad_z_so3, grad_z_inv, xyz, st);
    if (rc != LS_OK) return rc;
    return sdf_query_grad_launch(query, s, t, sb.dQ, B, M, grad_query, grad_t, grad_s, xyz, st);
}

// ------------------------------------------------------------------------------------------------ profiling
static void prof_collect(ls_model* m) {
    for (auto s : m->prof_streams) (void)hipStreamSynchronize(s);
    for (auto& r : m->prof) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) { m->prof_ms[r.kind][r.layer] += ms; m->prof_n[r.kind][r.layer] += 1; }
        m->ev_pool.push_back(r.a);
        m->ev_pool.push_back(r.b);
    }
    m->prof.clear();
}

int ls_profile_begin(ls_model_t* m) {
    LS_REQUIRE(m, "profile_begin: null model");
    prof_collect(m);
    memset(m->prof_ms, 0, sizeof(m->prof_ms));
    memset(m->prof_n, 0, sizeof(m->prof_n));
    if (m->knn_stats) LS_HIP_CHECK(hipMemset(m->knn_stats, 0, sizeof(unsigned long long) * 2 * LS_MAX_LAYERS));
    m->profiling = true;
    return LS_OK;
}

int ls_profile_knn_stats(ls_model_t* m, unsigned long long* out_host, int max_layers) {
    LS_REQUIRE(m && out_host && max_layers >= 1, "profile_knn_stats: null argument");
    LS_REQUIRE(m->knn_stats, "profile_knn_stats: the handle has no statistics buffer");
    for (auto s : m->prof_streams) (void)hipStreamSynchronize(s);
    unsigned long long h[2 * LS_MAX_LAYERS];
    LS_HIP_CHECK(hipMemcpy(h, m->knn_stats, sizeof(h), hipMemcpyDeviceToHost));
    for (int i = 0; i < std::min(max_layers, (int)LS_MAX_LAYERS); ++i) { out_host[2 * i] = h[2 * i]; out_host[2 * i + 1] = h[2 * i + 1]; }
    return LS_OK;
}

int ls_profile_end(ls_model_t* m, ls_profile_entry* out, int max_entries, int* n_out) {
    LS_REQUIRE(m && out && n_out, "profile_end: null argument");
    prof_collect(m);
    m->profiling = false;
    int n = 0;
    for (int k = 0; k < LS_K_COUNT; ++k)
        for (int l = 0; l < 16; ++l)
            if (m->prof_n[k][l] > 0 && n < max_entries) {
                out[n].kind = k; out[n].layer = l; out[n].launches = m->prof_n[k][l]; out[n].total_ms = m->prof_ms[k][l];
                ++n;
            }
    *n_out = n;
    return LS_OK;
}

}  // extern "C"
