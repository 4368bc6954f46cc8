// ls_launch.h -- the library's only internal interface: every host function that one translation unit defines and another calls, declared
// once, with its default arguments.  Included by the file that defines a function and by every file that calls it, so a definition that
// drifts from its declaration fails where it is made.  (The k-NN files' own cross-calls are in knn_common.h; set_error is in ls_common.h.)
#pragma once
#include "ls_common.h"
#include "gemm_plan.h"
#include "edge_plan.h"
#include "knn_plan.h"

namespace ls {

// ---- knn.hip
int knn_dispatch(const float* dst, const float* src, const int32_t* dst_rows, int B, int Nd, int dst_n, int Ns, int C, int K, unsigned flags, int32_t* idx_out,
                 float* dist_out, void* scratch, const int32_t* seed_idx, int seed_n, int seed_by_row, hipStream_t st);
size_t knn_scratch_bytes(int B, int Nd, int dst_n, int Ns, int C, unsigned flags);
// (knn_plan.h: the kernel choice) the traits of a knn_dispatch call with these arguments; self: dst == src
inline KnnTraits knn_traits(bool self, int B, int Nd, int dst_n, int Ns, int C, int K, unsigned flags, bool seeded, bool has_scratch) {
    KnnTraits t;
    t.B = B; t.Nd = Nd; t.dst_n = dst_n; t.Ns = Ns; t.C = C; t.K = K;
    t.fma = (flags & LS_FLAG_CONTRACT_FMA) != 0;
    t.valu_only = (flags & LS_FLAG_KNN_VALU_ONLY) != 0;
    t.seeded = seeded; t.self = self; t.has_scratch = has_scratch;
    return t;
}
// ---- knn_mfma.hip
// the exact-phase counters of the last call on `scratch` whose plan says stats, added to out[0..1]
int knn_sweep_stats_launch(const void* scratch, int B, int Nd, unsigned long long* out, hipStream_t st);
// ---- fps.hip
int fps_dispatch(const float* pts, const int32_t* lengths, int B, int N, int K, unsigned flags, int32_t* idx_out, float* pts_out, void* ws, size_t ws_bytes,
                 hipStream_t st);
size_t fps_scratch_bytes_per_cloud(int N);
// ---- gemm.hip
// (gemm_plan.h: the kernel choice -- gemm_plan, gemm_vn_plan -- and its queries gemm_scratch_floats, gemm_w_planes_useful)
int gemm_mode();
// out [M, N] = act(A [M, K] W [N, K]^T + bias)
struct Gemm {
    const float* A = nullptr; int lda = 0;
    const float* W = nullptr; int ldw = 0;
    const float* bias = nullptr;
    float* out = nullptr; int ldc = 0;
    int M = 0, N = 0, K = 0, relu = 0;
    const int32_t* a_rows = nullptr; int gNd = 0, gNs = 0;   // gather: row r of A is row a_rows[r] of its instance (gNd rows of gNs)
    float* scratch = nullptr;      // gemm_scratch_floats(M, N, K) floats: the launch may split K
    bool latency = false;          // a handful of tiles by construction: the short-slab fp32 kernel (gemm_plan.h)
    int pieces = 3;                // 2: two-piece bf16 products (the decoder's opt-in throughput mode)
    const float* mask = nullptr;   // laid out like `out`: out = (mask > 0) ? A W^T : 0; never splits K
    GemmAux aux;
};
// out [M = B * npts * 3, C] = VN-act(A W[0:C]^T + G lin part, A W[C:2C]^T + G dir part), oms = 1 - negative slope
struct GemmVn {
    const float* A = nullptr; int lda = 0;
    const float* W = nullptr; int ldw = 0;
    const float* G = nullptr; int ldg = 0;
    float* out = nullptr;
    int M = 0, C = 0, K = 0, npts = 0;
    float oms = 0.f;
    GemmAux aux;
};
GemmTraits gemm_traits(const Gemm& g);
GemmTraits gemm_traits(const GemmVn& g);
int gemm_run(const Gemm& g, hipStream_t st);
int gemm_vn_run(const GemmVn& g, hipStream_t st);   // gemm_vn_plan(gemm_traits(g)).kernel == NONE is an error: the caller runs GEMM + vn_act_rows
int gemm_rowmax_launch(const float* W, int rows, int K, int ldw, float* out, hipStream_t st);
int gemm_rowmax_parts(int N);
size_t gemm_w_planes_bytes(size_t rows, int K);
int gemm_presplit_w_launch(const float* W, int rows, int K, int ldw, const float* rowmax, void* planes, hipStream_t st);
// ---- edge.hip
int edge_l0_launch(const float* pts, const int32_t* knn, const float* w0, int B, int N, int Co, float neg_slope, float* out, hipStream_t st);
// layer i >= 1 over its table area, launched as edge_plan (edge_plan.h) says; rowmax [B*Nd*3][rowmax_parts] and colsum [B][cs_rows][3][Co] are
// written where the plan says so
struct Edge {
    const float* T = nullptr;            // the table area, formed as the same plan says (the table-free path's scratch)
    const float* cur = nullptr;          // the layer's input [B, Ns, 3, Cin]: the fused destination side reads it
    const void* planes = nullptr;        // wq_planes (ATTN_FQ_*) / wt_planes (FT_*) of the layer
    const int32_t *knn = nullptr, *dst_rows = nullptr;
    int B = 0, Ns = 0, Nd = 0, Cin = 0, Co = 0, head_c = 0;
    float neg_slope = 0.f;
    float *out = nullptr, *rowmax = nullptr, *colsum = nullptr;
};
int edge_run(const Edge& e, const EdgePlan& p, hipStream_t st);
size_t edge_wq_planes_bytes(int Co, int Cin);
int edge_presplit_wq_launch(const float* Wq, int Co, int Cin, void* planes, hipStream_t st);
// ---- edge_fused.hip: attention layers with 32 destination points (released layers 5 / 6) -- table slices formed and consumed in LDS
size_t edge_ft_w_bytes(int Co, int Cin);
int edge_ft_presplit_w_launch(const float* W, int Co, int Cin, void* planes, hipStream_t st);
int edge_ft_prep_launch(const float* cur, const int32_t* dst_rows, int Ns, int Nd, void* scratch, const EdgePlan& p, hipStream_t st);
int edge_ft_attn_launch(const Edge& e, const EdgePlan& p, hipStream_t st);
// ---- pointwise.hip
int prologue_launch(const float* x, int B, int N, float* pts, float* centroid, float* scale0, float* unused, hipStream_t st);
size_t prologue_scratch_floats(int B);
int transpose_cloud_launch(const float* x, int B, int N, float* pts, hipStream_t st);
int mean_points_launch(const float* f, int B, int N, int C, float* out, hipStream_t st);
int glob_mean_gemv_launch(const float* f, int B, int N, int C, const float* W, int col0, int ncols, float* G, int ldg, hipStream_t st, int npoints = 0);
int vn_act_rows_launch(const float* T, int ldt, const float* G, int ldg, int B, int N, int C, float neg_slope, float* out, hipStream_t st);
int tail_check(int Cd);   // what tail_launch serves (its own first line): asked before anything that feeds it is enqueued
int tail_launch(const float* Tc, int ldc, int B, int NP, int Cd, const float* inv_t, const float* fc0_t, const float* misc, float neg_slope, float scale_factor,
                int center_pred, int center_scale, const float* centroid, const float* scale0, float* z_so3, float* z_inv, float* s_out, float* t_out,
                hipStream_t st);
int scatter_codes_launch(const float* packed, int B, int c, float* z_so3, float* z_inv, float* s, float* t, hipStream_t st);
// ---- sdf.hip
int sdf_prep_launch(const float* inv_t, const float* so3_t, const float* wlen, const float* bias, const float* z_so3, const float* z_inv, int B, int L, int out_dim,
                    float* A, float* beff, bool xyz, hipStream_t st);
int sdf_affine_launch(const float* query, const int32_t* row_inst, const float* s, const float* t, const float* A, const float* beff, int B, long long rows,
                      int out_dim, int ldh, int accumulate, float* h, bool xyz, hipStream_t st, float* rowmax = nullptr);
int sdf_affine_rowmax_parts(int out_dim);
int sdf_out_launch(const float* h, int ldh, int width, const float* w, const float* bias, long long rows, float* sdf, hipStream_t st);
int sdf_out_bwd_launch(const float* g, const float* sdf, const float* w, const float* h, int ldh, int width, long long rows, float* dz, hipStream_t st,
                       float* rowmax = nullptr, const float* wmax = nullptr);
int relu_mask_launch(float* dh, const float* h, long long rows, int cols, int ld, hipStream_t st);
int sdf_affine_bwd_launch(const float* query, const float* s, const float* t, const float* dz, const float* A, int B, int M, int out_dim, int ldh, int accumulate,
                          float* dA, float* dbeff, float* dQ, bool need_code, bool xyz, hipStream_t st);
int sdf_code_grad_launch(const float* so3_t0, const float* inv_t0, const float* dA0, const float* db0, const float* so3_t1, const float* inv_t1, const float* dA1,
                         const float* db1, int B, int L, int out_dim, float* g_so3, float* g_inv, bool xyz, hipStream_t st);
int sdf_query_grad_launch(const float* query, const float* s, const float* t, const float* dQ, int B, int M, float* g_query, float* g_t, float* g_s, bool xyz,
                          hipStream_t st);
int transpose_launch(const float* W, int rows, int cols, float* Wt, hipStream_t st);

}  // namespace ls
