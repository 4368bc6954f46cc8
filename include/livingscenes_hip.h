/*
 * livingscenes_hip.h -- C ABI of liblivingscenes_hip.so (MI355X / gfx950 only).
 *
 * The reference (GradientSpaces/LivingScenes) is pure Python/PyTorch: it has no FFI of its own.  The
 * boundary below is what a maintainer binds (ctypes) to replace the ATen /
 * pytorch3d kernels behind the reference's Python call surface for the per-instance inference path.
 * Every entry point cites the reference interface it replaces (paths relative to the reference root).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name ends in _host; the caller (PyTorch) owns all
 *     input / output / workspace buffers; the library never frees or retains caller memory and never
 *     allocates device memory behind an operator call: every op that needs scratch takes
 *     (workspace, workspace_bytes) sized by its ls_<op>_workspace_bytes() query.  The only library-owned
 *     device allocations are the packed weights of an ls_model_t (and, on the first ls_sdf_backward of a
 *     model, their transposed copy), freed by ls_model_destroy.
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it, nothing synchronises
 *     the device.  (ls_encoder_forward additionally forks onto a library-owned side stream and joins
 *     back with events; the join happens before it returns control of `stream`'s tail.)
 *   - return value: 0 on success, negative ls_status on failure; text via ls_last_error() (thread-local).
 *   - feature tensors use the library's point-major layout [B, N, 3, C] ("x-major rows": a point is
 *     three rows of C contiguous floats).  The reference layout is [B, C, 3, N]; the Python shim
 *     converts at the API edge only (inputs x[B,3,N], outputs z_so3[B,C,3] keep the reference layout).
 *   - all floating point is IEEE fp32 (the reference runs fp32: configs/room4cates.yaml:15).
 */
#ifndef LIVINGSCENES_HIP_H
#define LIVINGSCENES_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    LS_OK = 0,
    LS_ERR_INVALID = -1,     /* bad argument / unsupported shape */
    LS_ERR_HIP = -2,         /* a HIP runtime call failed */
    LS_ERR_WORKSPACE = -3,   /* workspace too small */
    LS_ERR_NO_DEVICE = -4
} ls_status;

/* flags for the integer-exact ops: how `dist += diff*diff` is rounded (oracle/ls_oracle.c header) */
#define LS_FLAG_CONTRACT_FMA 1u /* d = fmaf(diff,diff,d); default (0) = separately rounded mul, add */
#define LS_FLAG_KNN_MFMA_FILTER 2u /* k-NN: accepted for compatibility, no effect: the MFMA sweep kernel (knn_mfma.hip) is the
                                     default wherever it applies (seed_idx given, C == 32 or 64); result is bit-identical */
#define LS_FLAG_KNN_VALU_ONLY 4u   /* k-NN: force the all-VALU kernel (knn.hip) even where the MFMA sweep applies (A/B work) */

#define LS_FLAG_KABSCH_RAW_WEIGHTS 8u /* Kabsch: `weights` are final (the caller applied pose_estimation.py:52-66 itself); no normalisation */

/* per-problem status written to ls_kabsch_batched_f32's flags_out */
#define LS_KABSCH_OK 0         /* covariance of rank >= 2: unique rotation */
#define LS_KABSCH_RANK1 1      /* rank 1: smallest rotation of the least-squares family (torch.svd also succeeds here) */
#define LS_KABSCH_RANK0 2      /* zero covariance: identity rotation, t = mu2 - mu1 */
#define LS_KABSCH_NONFINITE 3  /* NaN / Inf input: identity, zero t -- the reference's SVD-exception branch, flag = True */

#define LS_MAX_LAYERS 8

/* version of this C ABI: bumped whenever a signature or struct layout changes incompatibly (101: double-precision Adam hyper-parameters in
 * ls_adam_group / ls_adam_step_f32 / ls_se3_adam_step_f32, option 4 (LDS-staged attention); 102: LS_OPT_EDGE_FUSE_Q / _T, LS_OPT_GLOB_FUSE, LS_OPT_DEBUG_EDGE; the
 * library reads no development switches from the environment any more; 104: option 4 retired with the staged attention path, refused like
 * any unknown option; 105: the mesh metrics ls_mesh_contains_f64 / ls_mesh_distance_f64 / ls_mesh_sample_f64; 106: ls_model_desc.dec_input and
 * off_dec_xyz_t, the invariant decoder_type "deepsdf"; 107: the ragged multi-mesh metrics ls_mesh_contains_batch_f64 /
 * ls_mesh_distance_batch_f64 / ls_mesh_sample_batch_f64; symbols added since -- ls_reg_metrics_batch, ls_mesh_cluster_f64 / ls_mesh_cluster_batch_f64,
 * ls_cloud_merge_f32 / ls_cloud_merge_batch_f32, ls_cloud_nearest_f32 / ls_cloud_nearest_batch_f32, ls_cloud_icp_f32 / ls_cloud_icp_batch_f32,
 * ls_cloud_normals_f32 / ls_cloud_normals_batch_f32, ls_cloud_icp_plane_f32 / ls_cloud_icp_plane_batch_f32, ls_cloud_project_f32 / ls_cloud_project_batch_f32,
 * ls_mesh_render_depth_f64 / ls_mesh_render_depth_batch_f64, ls_depth_points_f32, ls_cloud_carve_f32 / ls_cloud_carve_batch_f32,
 * ls_depth_fuse_f32 / ls_depth_fuse_batch_f32, ls_tsdf_volume_f64, ls_tsdf_mesh_f64 / ls_tsdf_mesh_batch_f64,
 * ls_tsdf_sample_f32 / ls_tsdf_sample_batch_f32, ls_tsdf_icp_f32 / ls_tsdf_icp_batch_f32,
 * ls_tsdf_draw_f32 / ls_tsdf_draw_batch_f32, ls_tsdf_fit_loss_f64,
 * ls_tsdf_raycast_f64 / ls_tsdf_raycast_batch_f64, ls_depth_compare_f32,
 * ls_depth_normals_f32, ls_depth_fuse_weighted_f32 / ls_depth_fuse_weighted_batch_f32,
 * ls_tsdf_prior_rows_f32 / ls_tsdf_prior_rows_batch_f32, ls_tsdf_prior_vote_f32 / ls_tsdf_prior_vote_batch_f32 -- change no existing layout and keep 107).  ls_version() returns the value the LIBRARY was built with; a
 * binding compares it with the header it was written against and refuses a mismatch (livingscenes_amd/_lib.py: load). */
#define LS_ABI_VERSION 107
int ls_version(void);
const char* ls_last_error(void);
/* number of HIP devices visible, or a negative ls_status */
int ls_device_count(void);

/* ------------------------------------------------------------------------------------------------
 * Leaf operators
 * ---------------------------------------------------------------------------------------------- */

/* pytorch3d.ops.knn_points(dst, src, K, return_nn=...) as called at
 * lib_shape_prior/core/lib/vec_sim3/vec_dgcnn_atten.py:139-141 (feature-space dynamic graph).
 *   src      [B, Ns, 3, C]   candidate features
 *   dst      [B, Nd', 3, C]  query features; if dst_rows != NULL the query n of instance b is row
 *                            dst_rows[b*Nd + n] of `dst` (which then has Nd' = dst_n rows per instance)
 *   idx_out  [B, Nd, K] int32, ascending (dist, index); -1 padded when Ns < K
 *   dist_out [B, Nd, K] or NULL
 *   seed_idx [B, Nd, 16] int32 or NULL: optional HINTS, any candidate indices per query (-1 = none), e.g. the
 *            neighbour list of the same point in the previous encoder layer.  Their exact distances initialise
 *            the top-K lists (tighter admission threshold, fewer insertions); the RESULT DOES NOT DEPEND on them.
 * Distance = sum_j (a_j-b_j)^2, j = c*3+x ascending, fp32, rounding per `flags`.  K <= 16.
 * C must be 1 or a multiple of 32.  Kernel choice (never visible in the result): C == 1 -> wave-per-query kernel
 * (knn_xyz.hip); seed_idx given and C in {32, 64} -> seed / matrix-core sweep / finish (knn_mfma.hip; the sweep filters with
 * bf16 MFMA on centred rows for Ns <= 2048, fp32 MFMA above); Nd <= 32 -> small-problem kernel; otherwise the tiled all-VALU
 * kernel (knn.hip).  workspace: ls_knn_workspace_bytes(..., seeded = seed_idx != NULL, flags) bytes (0 for some shapes: then
 * workspace may be NULL). */
size_t ls_knn_workspace_bytes(int B, int Nd, int dst_n, int Ns, int C, int seeded, unsigned flags);
int ls_knn_f32(const float* dst, const float* src, const int32_t* dst_rows, const int32_t* seed_idx, int B, int Nd,
               int dst_n, int Ns, int C, int K, unsigned flags, int32_t* idx_out, float* dist_out, void* workspace,
               size_t workspace_bytes, void* stream);

/* pytorch3d.ops.sample_farthest_points(points, K=..., random_start_point=False) as called at
 * vec_dgcnn_atten.py:169, model_utils.py:205, lib_more/more_solver.py:107-108.
 *   pts [B, N, 3]; lengths [B] or NULL; idx_out [B, K] int32 (-1 padded when K > length);
 *   pts_out [B, K, 3] or NULL (gathered points).  Start index 0, running min, first arg-max.
 * workspace: ls_fps_workspace_bytes(B, N, K) bytes -- non-zero only for raw clouds of more than 8 192 points, where it holds the
 * bucketed copy of the clouds the pruned scan works on (fps.hip); NULL / too small there = the un-pruned scan (same result, ~6x slower). */
size_t ls_fps_workspace_bytes(int B, int N, int K);
int ls_fps_f32(const float* pts, const int32_t* lengths, int B, int N, int K, unsigned flags, int32_t* idx_out,
               float* pts_out, void* workspace, size_t workspace_bytes, void* stream);

/* out[M,N] = act(A[M,K] * W[N,K]^T + bias[N]) -- the VecLinear channel contraction
 * (vec_layers.py:121-136, F.linear at :134) on x-major rows, and the DeepSDF linears
 * (lib_shape_prior/core/lib/implicit_func/deepsdf_decoder.py:98-121).  fp32 in, fp32 out; the products run on the f16
 * matrix cores as TWO-PIECE splits (a = h + l, h = f16(a), l = f16(a - h): 2^-22 |a|; three v_mfma_f32_32x32x16_f16 per 16 k into
 * one fp32 accumulator): measured against fp64 this is as accurate as an fp32 FMA chain (the fp32 accumulation error dominates
 * both) and exact on integer-valued operands below 2^22.
 * RANGE: any finite fp32 operands.  Every row of A and every row of W is multiplied by its own exact power of two before the split
 * (row maximum -> [2^14, 2^15)) and the accumulators by the inverse afterwards, so the f16 window follows each row: elements down to
 * 2^-17 of their row's maximum keep the full 22 bits, smaller ones an absolute error of at most 2^-39 of the row maximum (2^-15 of
 * the fp32 rounding of the row's largest term), nothing overflows; rows that hold
 * Inf / NaN give non-finite results in that row only.  A row's result depends on that row of A and on W only -- not on the other rows of
 * the call -- as long as the launch does not split K (split-K: M * N < 192 tiles of 128 x 128 and K >= 128 and a workspace is given;
 * it changes the fp32 summation order with M; ls_gemm_f32_ex with workspace = NULL never splits).
 * LS_GEMM_MODE=bf16x3 in the environment selects three-piece bf16 splits instead (six v_mfma_f32_32x32x16_bf16 per 16 k, ~1.5x the
 * time); LS_GEMM_MODE=fp32 the fp32-MFMA kernel (v_mfma_f32_32x32x2_f32, exact fp32 FMA chains).
 * K % 4 == 0, lda/ldw/ldc % 4 == 0; bias may be NULL; relu in {0,1}.  workspace: ls_gemm_workspace_bytes(M, N, K) bytes
 * (split-K slabs of under-filled long-K problems; 0 -> may be NULL). */
size_t ls_gemm_workspace_bytes(int M, int N, int K);
int ls_gemm_f32(const float* A, int lda, const float* W, int ldw, const float* bias, float* out, int ldc, int M,
                int N, int K, int relu, void* workspace, size_t workspace_bytes, void* stream);
/* The same GEMM for callers that chain several of them (an MLP): the row maxima the range scaling needs can be handed over instead
 * of being re-derived by a pre-pass over the operands (which costs ~30 % at K >= 128):
 *   a_rowmax [M][a_parts] or NULL: max over the parts >= max|A[row, :]| (any upper bound serves; a factor of two of slack costs one
 *                                  bit at the bottom of the 17-binade window);   w_rowmax [N] or NULL: likewise for W (ls_rowmax_f32 once
 *                                  per weight matrix);
 *   out_rowmax [M][ls_gemm_rowmax_parts(N)] or NULL: receives max|out[row, 64-column block]| -- the next layer's a_rowmax.  Not
 *                                  written by a launch that splits K: pass workspace = NULL when chaining.
 * Results are bit-identical to ls_gemm_f32 whenever the maxima handed over are the exact ones. */
int ls_gemm_rowmax_parts(int N);
int ls_gemm_f32_ex(const float* A, int lda, const float* W, int ldw, const float* bias, float* out, int ldc, int M, int N, int K,
                   int relu, const float* a_rowmax, int a_parts, const float* w_rowmax, float* out_rowmax, void* workspace,
                   size_t workspace_bytes, void* stream);
/* out[r] = max_k |X[r * ld + k]|, k < K  (X [rows, K]) */
int ls_rowmax_f32(const float* X, int rows, int K, int ld, float* out, void* stream);
/* A weight matrix that many GEMMs read can be split ONCE: planes = both f16 pieces of its range-scaled rows (4 * N * K bytes; row n =
 * K / 32 lines of [hi: 32 f16 | lo: 32 f16] of s_n W[n, :], s_n the power of two of w_rowmax[n], which must be the same array later
 * calls pass).  The
 * K >= 512 kernels then stage W with 16-byte copies instead of re-splitting it in every workgroup (decoder shape: -5 % time).
 * ls_gemm_w_planes_bytes = 0 -> no kernel reads planes at this K (K < 512 or K % 32 != 0): use ls_gemm_f32_ex.
 * ls_gemm_f32_planes: ls_gemm_f32_ex with the planes (W itself is still passed: same result, bit for bit, as without them);
 * never splits K.  F.linear of the reference (vec_layers.py:134, deepsdf_decoder.py:98-121) with a fixed weight. */
size_t ls_gemm_w_planes_bytes(int N, int K);
int ls_gemm_presplit_w_f32(const float* W, int ldw, int N, int K, const float* w_rowmax, void* planes, size_t planes_bytes, void* stream);
int ls_gemm_f32_planes(const float* A, int lda, const float* W, int ldw, const void* w_planes, const float* bias, float* out, int ldc,
                       int M, int N, int K, int relu, const float* a_rowmax, int a_parts, const float* w_rowmax, float* out_rowmax,
                       void* stream);

/* Shape_Prior.encode prologue, model_utils.py:166-177: centroid, scale_0 = mean of the 5 largest
 * entries of the N x N distance matrix, normalised cloud.
 *   x [B,3,N] (reference layout) -> pts_out [B,N,3], centroid_out [B,3], scale0_out [B] */
int ls_encode_prologue_f32(const float* x, int B, int N, float* pts_out, float* centroid_out, float* scale0_out,
                           void* stream);

/* sequential_matcher's score matrix, lib_more/matcher_new.py:110-120:
 * S = normalize(m0) @ normalize(m1)^T.   m0 [n,D], m1 [m,D] -> S [n,m];  workspace: (n + m) floats (the inverse row norms) */
size_t ls_cosine_scores_workspace_bytes(int n, int m);
int ls_cosine_scores_f32(const float* m0, const float* m1, int n, int m, int D, float* scores, void* workspace,
                         size_t workspace_bytes, void* stream);

/* The greedy assignment loop shared by sequential / sim3_seq / eq_seq matchers
 * (matcher_new.py:121-136, :166-181, :212-227): repeat min(n,m) times { S /= (max(S)+1e-5); take the
 * first row-major arg-max; record; delete row and column }.  `scores` [n,m] is DESTROYED.
 * matches0 [n], matches1 [m] int64, -1 = unmatched. */
int ls_greedy_match_f32(float* scores, int n, int m, int64_t* matches0, int64_t* matches1, void* stream);

/* nn_matcher after its score matrix, lib_more/matcher_new.py:89-98 (find_nn :73-83 without thresholds, mutual_check :100-105 twice):
 * matches0[i] = argmax_j S[i][j] if argmax_i S[i][that j] == i else -1; matches1 = mutual_check(argmax over rows, matches0).
 * First maximum on ties.  scores [n,m] (read only) -> matches0 [n], matches1 [m] int64.  One launch, one workgroup (LDS: about 190 x 190 at most). */
int ls_nn_match_f32(const float* scores, int n, int m, int64_t* matches0, int64_t* matches1, void* stream);

/* sinkhorn_matcher after its score matrix, matcher_new.py:49-71: couplings = [[S / score_divisor, alpha], [alpha, alpha]], `iters` log-space Sinkhorn
 * iterations (log_optimal_transport :20-40 with log_sinkhorn_iterations above it), arg-maxes of the inner block of Z, mutual checks, and
 * exp(max0) > match_threshold (:58-66).  The reference calls it with score_divisor = desc_dim ** 0.5, alpha = 1, iters = 100, threshold 0.
 * scores [n,m] (read only) -> matches0 [n], matches1 [m] int64, -1 = unmatched.  One launch, one workgroup. */
int ls_sinkhorn_match_f32(const float* scores, int n, int m, float score_divisor, float alpha, int iters, float match_threshold,
                          int64_t* matches0, int64_t* matches1, void* stream);

/* kabsch_transformation_estimation(x1, x2, weights, normalize_w=True, eps=1e-7),
 * lib_more/pose_estimation.py:29-102 (+ transformation_residuals :105-121).
 *   x1,x2 [b,n,3]; weights [b,n] or NULL (ones); flags: 0 = weights are normalised as :52-54 does, LS_FLAG_KABSCH_RAW_WEIGHTS =
 *   used as given (normalize_w=False, or the caller applied best_k / w_threshold of :58-66 to the normalised weights);
 *   R [b,3,3], t [b,3] (the reference's [b,3,1]), res [b,n] or NULL, flags_out [b] int32 or NULL = LS_KABSCH_* status
 *   (only LS_KABSCH_NONFINITE corresponds to the reference's SVD-failure branch at :79-88). */
int ls_kabsch_batched_f32(const float* x1, const float* x2, const float* weights, int b, int n, unsigned flags, float* R,
                          float* t, float* res, int32_t* flags_out, void* stream);
/* The same fit on More_Solver's pseudo-points (more_solver.py:114-116: kabsch(code1.z_so3 + code1.t, code2.z_so3 + code2.t)) with the
 * element-wise work around it inside the launch: set i of side k is x_k[i] + off_k[i] (off_k [*,3] or NULL), problem p reads set
 * sel_k[p] of side k (sel_k [b] int64 or NULL = p; a negative entry -- an unmatched row of matches0 -- reads set 0, as
 * matches0.clamp(min=0) does).  Unit weights.  Bit-identical to ls_kabsch_batched_f32 on the materialised sums. */
int ls_kabsch_codes_f32(const float* x1, const float* off1, const int64_t* sel1, const float* x2, const float* off2, const int64_t* sel2, int b,
                        int n, float* R, float* t, float* res, int32_t* flags_out, void* stream);

/* mean Kabsch residual of every (src i, tgt j) pair of equivariant codes: res_mat of
 * matcher_new.py:150-156 / :196-202.   src [n,P,3], tgt [m,P,3] -> res [n,m] */
int ls_kabsch_residual_matrix_f32(const float* src, const float* tgt, int n, int m, int P, float* res, void* stream);

/* ---- Ragged batches of matching problems: P problems per call, stored back to back (the convention of ls_mesh_*_batch_f64).
 * Problem p owns the source rows [src_off[p], src_off[p+1]) and the target rows [tgt_off[p], tgt_off[p+1]) of the packed arrays; its
 * score (residual) block is row-major n_p x m_p and starts at entry sum_{q<p} n_q m_q of the packed `scores` (`res`); matches0 [n_total]
 * and matches1 [m_total] hold indices LOCAL to the problem, -1 = unmatched.  src_off / tgt_off: HOST int64 arrays of P + 1 entries (P >= 1),
 * starting at 0, never decreasing, ending at n_total / m_total: checked, with errors that name the problem, and copied into the workspace
 * on the stream.  A problem with n_p == 0 or m_p == 0 is allowed: it reads nothing, owns no scores, and every match of its non-empty side
 * is -1 (the single ops refuse empty problems).  FOR EVERY PROBLEM EVERY OUTPUT IS BIT-IDENTICAL TO THE SINGLE OP ON THAT PROBLEM ALONE:
 * the same kernels, each problem with the launch choices the single op makes for its size.  The number of kernel launches does not depend
 * on P; no host synchronisation, no allocation.  *_batch_workspace_bytes: 0 for P <= 0 or a negative total; a missing or short workspace
 * is LS_ERR_WORKSPACE. */
/* ls_cosine_scores_f32 (matcher_new.py:110-120) per problem: m0 [n_total,D], m1 [m_total,D] -> packed scores.  1 launch, or 2 when a problem
 * has more than 4096 entries (the single op's two forms: each problem's entries are formed the way the single op forms them). */
size_t ls_cosine_scores_batch_workspace_bytes(int P, long long n_total, long long m_total);
int ls_cosine_scores_batch_f32(int P, const float* m0, long long n_total, const long long* src_off, const float* m1, long long m_total,
                               const long long* tgt_off, int D, float* scores, void* workspace, size_t workspace_bytes, void* stream);
/* ls_greedy_match_f32 (matcher_new.py:121-136, :166-181, :212-227) per problem; the packed `scores` are DESTROYED.  One workgroup per problem,
 * at most one launch per kernel class (n_p m_p <= 64 | <= 1024 | larger): every problem runs the kernel the single op gives it. */
size_t ls_greedy_match_batch_workspace_bytes(int P, long long n_total, long long m_total);
int ls_greedy_match_batch_f32(int P, float* scores, long long n_total, const long long* src_off, long long m_total, const long long* tgt_off,
                              int64_t* matches0, int64_t* matches1, void* workspace, size_t workspace_bytes, void* stream);
/* ls_nn_match_f32 (matcher_new.py:89-98, find_nn :73-83, mutual_check :100-105) per problem: one launch, one workgroup per problem, the LDS
 * of the largest problem (a problem beyond the single op's limit is refused, and named, before anything is enqueued). */
size_t ls_nn_match_batch_workspace_bytes(int P, long long n_total, long long m_total);
int ls_nn_match_batch_f32(int P, const float* scores, long long n_total, const long long* src_off, long long m_total, const long long* tgt_off,
                          int64_t* matches0, int64_t* matches1, void* workspace, size_t workspace_bytes, void* stream);
/* ls_sinkhorn_match_f32 (matcher_new.py:49-71, log_optimal_transport :20-40) per problem; score_divisor, alpha, iters and match_threshold
 * hold for the whole batch.  One launch, as ls_nn_match_batch_f32. */
size_t ls_sinkhorn_match_batch_workspace_bytes(int P, long long n_total, long long m_total);
int ls_sinkhorn_match_batch_f32(int P, const float* scores, long long n_total, const long long* src_off, long long m_total, const long long* tgt_off,
                                float score_divisor, float alpha, int iters, float match_threshold, int64_t* matches0, int64_t* matches1,
                                void* workspace, size_t workspace_bytes, void* stream);
/* ls_kabsch_residual_matrix_f32 (res_mat of matcher_new.py:150-156 / :196-202) per problem: src [n_total,C,3], tgt [m_total,C,3] (C pseudo-points
 * per code) -> packed res.  One launch, one wave per (i, j) pair. */
size_t ls_kabsch_residual_matrix_batch_workspace_bytes(int P, long long n_total, long long m_total);
int ls_kabsch_residual_matrix_batch_f32(int P, const float* src, long long n_total, const long long* src_off, const float* tgt, long long m_total,
                                        const long long* tgt_off, int C, float* res, void* workspace, size_t workspace_bytes, void* stream);

/* pytorch3d.ops.iterative_closest_point(X, Y, init_transform=SimilarityTransform(R0,T0,1)) with default
 * arguments (100 iterations, relative_rmse_thr 1e-6), as called at lib_more/more_solver.py:182-187.
 * Row-vector convention Xt = X R + T.  X [b,n,3], Y [b,m,3], R0 [b,3,3], T0 [b,3] ->
 * R [b,3,3], T [b,3], rmse [b], iters_out [1] int32.  workspace >= ls_icp_workspace_bytes(b,n). */
size_t ls_icp_workspace_bytes(int b, int n);
int ls_icp_f32(const float* X, const float* Y, const float* R0, const float* T0, int b, int n, int m, int max_iter,
               float rel_rmse_thr, unsigned flags, float* R, float* T, float* rmse, int32_t* iters_out,
               void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Model handle (packed device-resident weights: the library's only device allocation)
 * ---------------------------------------------------------------------------------------------- */
typedef struct ls_model ls_model_t;

typedef struct {
    /* encoder: VecDGCNN_att.__init__ arguments, vec_dgcnn_atten.py:23-45 */
    int32_t num_layers;
    int32_t feat_dim[LS_MAX_LAYERS];
    int32_t down_factor[LS_MAX_LAYERS]; /* 1 = no down-sampling before this layer */
    int32_t atten_start_layer;
    int32_t atten_head_c;
    int32_t res_global_start_layer;     /* >= num_layers disables the residual global conv */
    int32_t num_knn;
    int32_t c_dim;
    int32_t center_pred;
    int32_t center_pred_scale;
    float scale_factor;
    float neg_slope;
    /* decoder: DeepSDF_Decoder (deepsdf_decoder.py:12-57) behind FieldWrapper (model_utils.py:236-251) */
    int32_t dec_num_linear;             /* number of linear layers (9), 0 = no decoder packed */
    int32_t dec_width;                  /* hidden width (768 released, 512 invariant ablation) */
    int32_t dec_latent_in;              /* layer that re-concatenates the input (4), -1 = none */
    int32_t dec_input;                  /* LS_DEC_INNER / LS_DEC_XYZ: what the code-fed layers read (below) */
    /* offsets (in floats) into the packed blob; layouts documented in livingscenes_amd/packing.py */
    int64_t off_l0;                     /* [6][feat_dim[0]] layer-0 folded rows */
    int64_t off_edge[LS_MAX_LAYERS];    /* layer i>=1: [ncols_i][feat_dim[i-1]] folded per-point weights */
    int64_t off_glob[LS_MAX_LAYERS];    /* layer i>=g0: [4*C][C] = {Wa;Wd*Wa;Wb;Wd*Wb} */
    int64_t off_convc;                  /* [c_dim+1 (padded to 4)][feat_dim[-1]] */
    int64_t off_inv_t;                  /* fc_inv^T [c_dim][c_dim] */
    int64_t off_c_fc0_t;                /* fc_center.fc0 {lin;dir*lin}^T : [c_dim][2*h] */
    int64_t off_c_misc;                 /* lin1 [h], shortcut [c_dim], act2 dir scalar [1] */
    int64_t off_dec_w[12];              /* decoder layer l: folded main weight [out_l][kin_l] */
    int64_t off_dec_b[12];              /* decoder bias [out_l] */
    int64_t off_dec_inv_t[12];          /* layers fed by the code (0 and latent_in): Wa^T [latent][out] */
    int64_t off_dec_so3_t[12];          /*   "    Wb^T [latent][out] */
    int64_t off_dec_len[12];            /*   "    w_len [out] */
    int64_t off_dec_xyz_t[12];          /*   "    LS_DEC_XYZ only: W_xyz^T [3][out] (the columns that multiply the raw query) */
    int64_t blob_floats;
} ls_model_desc;

/* ls_model_desc.dec_input: the decoder's input u per query, and what the code-fed layers (0 and latent_in) fold per instance
 *   LS_DEC_INNER  decoder_type "inner_deepsdf" (released): u = [z_inv | <q, z_so3_c>_c | |q|], q = (query - t) / s, width 2 c_dim + 1;
 *                 off_dec_inv_t / off_dec_so3_t / off_dec_len hold the three column blocks of W
 *   LS_DEC_XYZ    decoder_type "deepsdf" (invariant ablation): u = [z_inv | query], the RAW query, width c_dim + 3;
 *                 off_dec_inv_t / off_dec_xyz_t hold the two column blocks; off_dec_so3_t / off_dec_len are unused.
 *                 The SDF then does not depend on z_so3, s or t: the ls_sdf_* calls ignore them (they may be NULL), and ls_sdf_backward
 *                 writes exact zeros to grad_z_so3, grad_s and grad_t where they are given (each may be NULL) */
#define LS_DEC_INNER 0
#define LS_DEC_XYZ 1
int ls_model_create(const ls_model_desc* desc_host, const float* blob_host, ls_model_t** out);
void ls_model_destroy(ls_model_t* m);
/* per-handle switches (defaults in brackets) */
#define LS_OPT_SDF_TRAIN_SPLITK 1 /* [1] split-K in the GEMMs of ls_sdf_decode_train / ls_sdf_backward when the problem under-fills the chip
                                     (one 1024-point cloud); 0 = never: a row's values do not depend on the size of the call (batched == per pair) */
#define LS_OPT_SDF_BF16X2 2       /* [0, or LS_SDF_BF16X2 in the environment] decoder products as two-piece bf16 splits (2^-16 per product, ~1.5x) */
#define LS_OPT_ENCODE_GRAPH 3     /* [0, or LS_ENCODE_GRAPH in the environment] ls_encode replays a captured hipGraph of its ~170 launches (one per
                                     (workspace, B, N, flags, stream); needs a non-NULL stream; profiled / traced calls always enqueue directly).
                                     Off by default: on ROCm 7.2 the replay measured slower than direct enqueue (22.2k vs 29.6k obj/s, one step in flight) */
#define LS_OPT_EDGE_FUSE_Q 5      /* [1] attention layers 2 - 4: the destination-side column groups computed inside the edge kernel (edge.hip: edge_attn_fq_kernel);
                                     0 = as table columns written by the table GEMM (the general path; also taken under LS_GEMM_MODE=bf16x3 / fp32) */
#define LS_OPT_EDGE_FUSE_T 6      /* [1] the 32-point attention layers (released layers 5, 6) without a table (edge_fused.hip); 0 = table GEMM + edge kernel */
#define LS_OPT_GLOB_FUSE 7        /* [1] residual global conv as one mean + GEMV launch and one GEMM + VN-activation launch (gemm.hip: gemm_vn_kernel);
                                     0 = mean, GEMM -> table, per-instance GEMM, VN activation as separate launches (same products in the same order);
                                     2 = as 1, and the operator export ls_vn_lna_f32 first takes the exact row maxima of its input, as the encoder's attention
                                     kernels hand them to this conv (layers of 64 channels then run gemm_vn_direct_kernel: bit-identical, tests/) */
#define LS_OPT_DEBUG_EDGE 8       /* [0] ls_vn_edgeconv_*: 1 = run the table GEMM only, 2 = run the edge kernel only on the tables already in the workspace
                                     (per-operator counter passes: scripts/pmc_ops.py); 0 = both */
#define LS_OPT_GEMM_OVERLAP 9     /* [1] ls_encode runs a layer's table GEMM on a side stream beside its k-NN build (+5 % with one call in flight); 0 = on the caller's
                                     stream (better once several ls_encode calls overlap on different streams: bench.py turns it off, -3.5 % otherwise) */
int ls_model_set_option(ls_model_t* m, int option, int value);
/* the handle's CURRENT value of an option (what ls_model_create read from the environment, or the last ls_model_set_option): the only
 * way a caller can change an option temporarily and put back exactly what was there */
int ls_model_get_option(const ls_model_t* m, int option, int* value);

/* ------------------------------------------------------------------------------------------------
 * Composite hot path
 * ---------------------------------------------------------------------------------------------- */

/* Shape_Prior.encode(x), model_utils.py:165-197, = prologue + VecDGCNN_att.forward
 * (vec_dgcnn_atten.py:177-252) + epilogue (t = center + centroid, s = scale_0 * pred_scale).
 *   x [B,3,N] -> z_so3 [B,c_dim,3], z_inv [B,c_dim], s [B], t [B,3]
 * Host cost: ~170 launches (0.7 ms of host time per 64-instance call).  With LS_OPT_ENCODE_GRAPH the sequence is captured into a hipGraph
 * on first use per (workspace, B, N, flags, stream) and replayed afterwards (x and the outputs may move between calls).
 * trace_knn / trace_fps (nullable): per-layer k-NN / FPS indices for the parity tests, packed
 * back to back: knn layer i at offset sum_{j<i} B*Nd_j*K (int32), fps level l at sum B*Nd_l.
 * If pre_normalised != 0, x is taken as already centred/scaled (prologue skipped, centroid 0, scale_0 1):
 * this is VecDGCNN_att.forward alone and the outputs are (center, scale, z_so3, z_inv). */
size_t ls_encoder_workspace_bytes(const ls_model_t* m, int B, int N);
int ls_encode(ls_model_t* m, const float* x, int B, int N, int pre_normalised, unsigned flags, float* z_so3,
              float* z_inv, float* s, float* t, int32_t* trace_knn, int32_t* trace_fps, void* workspace,
              size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The encoder's layer operators on their own (the same code ls_encode runs), for callers that drive the layer loop
 * themselves and for isolated parity tests.  Features are [B, N, 3, C] rows; `layer` selects the weights.
 * ---------------------------------------------------------------------------------------------- */

/* One edge-conv layer of VecDGCNN_att.forward WITHOUT its residual global conv: get_graph_feature (vec_dgcnn_atten.py:124-161:
 * cat(nbr - ctr, ctr); + the cross-product channel at layer 0) -> V_list[layer] VecLNA (vec_layers.py:523-534) -> mean over the
 * 16 neighbours (:202-204, layers < atten_start_layer: ls_vn_edgeconv_pool_f32), or K / Q / V VecLNAs + channel_equi_vec_normalize
 * (vec_layers.py:24-31) + per-head soft-max attention (:205-219, ls_vn_edgeconv_attn_f32).
 *   src_f [B,Ns,3,C_in] (layer 0: the normalised cloud [B,Ns,3]); knn [B,Nd,16] int32 indices into the Ns source points;
 *   dst_rows [B,Nd] int32 or NULL: the FPS selection when the layer down-samples (destination point n = source row dst_rows[n]),
 *   NULL requires Nd == Ns;  out [B,Nd,3,C_out].  workspace holds the folded per-point tables (edge.hip header). */
size_t ls_vn_edgeconv_workspace_bytes(const ls_model_t* m, int layer, int B, int Ns, int Nd, int has_dst_rows);
int ls_vn_edgeconv_pool_f32(ls_model_t* m, int layer, const float* src_f, const int32_t* knn, const int32_t* dst_rows, int B,
                            int Ns, int Nd, float* out, void* workspace, size_t workspace_bytes, void* stream);
int ls_vn_edgeconv_attn_f32(ls_model_t* m, int layer, const float* src_f, const int32_t* knn, const int32_t* dst_rows, int B,
                            int Ns, int Nd, float* out, void* workspace, size_t workspace_bytes, void* stream);

/* The residual global conv of layer `layer` >= res_global_start_layer (vec_dgcnn_atten.py:222-225):
 * out = VecLinearNormalizeActivate_G(cat(f, mean_n f))  (vec_layers.py:523-534 = VecLinear :121-136 + VecActivation :241-268).
 *   f [B,N,3,C] -> out [B,N,3,C] */
size_t ls_vn_lna_workspace_bytes(const ls_model_t* m, int layer, int B, int N);
int ls_vn_lna_f32(ls_model_t* m, int layer, const float* f, int B, int N, float* out, void* workspace, size_t workspace_bytes,
                  void* stream);
/* ls_vn_lna_f32 with the side products the encoder passes between its layers (same workspace):
 *   a_rowmax [B*N*3][a_parts] or NULL: max over the parts bounds max|f[row, :]|, as the kernel that wrote f would hand it over
 *     (NULL: as ls_vn_lna_f32);  out_rowmax [B*N*3][C/32] or NULL: receives max|out[row, 32 q .. 32 q + 31]| where the one-launch
 *     form of the conv runs; *rowmax_written (nullable) says whether it did. */
int ls_vn_lna_ex_f32(ls_model_t* m, int layer, const float* f, int B, int N, const float* a_rowmax, int a_parts, float* out_rowmax,
                     int* rowmax_written, float* out, void* workspace, size_t workspace_bytes, void* stream);
/* The per-instance half of that conv alone: G[b][x][col0 + j] = < mean f[b][.][x][:], W[col0 + j][:] >, j < ncols.
 *   f [B,N,3,C], W [>= col0 + ncols rows][C], G [B*3][ldg]; C % 4 == 0.  npoints == 0: the mean of the N rows;  npoints > 0: f holds N
 *   rows of partial column sums over npoints points per instance, the mean is their sum / npoints. */
int ls_glob_mean_gemv_f32(const float* f, int B, int N, int C, const float* W, int col0, int ncols, float* G, int ldg, int npoints,
                          void* stream);

/* The encoder's heads (vec_dgcnn_atten.py:231-250): conv_c VecLNA (shared direction) -> mean over the NP points -> z_so3 =
 * channel_equi_vec_normalize, scale = mean_c |x_c| * scale_factor, z_inv = <cevn(fc_inv x), z_so3>, center = VecResBlock
 * (vec_layers.py:631-651) * scale_factor; then Shape_Prior.encode's epilogue (model_utils.py:182-185) when centroid / scale0
 * are given: t = center + centroid, s = scale0 * scale (both NULL: t = center, s = scale).
 *   f [B,NP,3,C_last] -> z_so3 [B,c_dim,3], z_inv [B,c_dim], s [B], t [B,3] */
size_t ls_encoder_tail_workspace_bytes(const ls_model_t* m, int B, int NP);
int ls_encoder_tail_f32(ls_model_t* m, const float* f, const float* centroid, const float* scale0, int B, int NP, float* z_so3,
                        float* z_inv, float* s, float* t, void* workspace, size_t workspace_bytes, void* stream);

/* FieldWrapper.forward(query, None, code, return_sdf=True), decoder_type "inner_deepsdf":
 * model_utils.py:230-263 + DeepSDF_Decoder.forward, deepsdf_decoder.py:78-123.
 *   query [B,M,3], z_so3 [B,c,3], z_inv [B,c], s [B], t [B,3] -> sdf [B,M]
 * B * M < 2^31 rows per call (here and in ls_sdf_decode_train / ls_sdf_backward): more is refused before anything is sized or enqueued. */
size_t ls_sdf_workspace_bytes(const ls_model_t* m, int B, int M);
int ls_sdf_decode(ls_model_t* m, const float* query, const float* z_so3, const float* z_inv, const float* s,
                  const float* t, int B, int M, float* sdf, void* workspace, size_t workspace_bytes, void* stream);

/* Ragged form of ls_sdf_decode: R query rows of B instances packed back to back (rows of one instance contiguous), row_inst [R]
 * int32 = instance of each row.  Used by the batched MISE rounds, where every instance asks for a different number of points
 * (the reference evaluates one instance at a time, occnet_utils/mesh_extractor2.py:116-131).  sdf [R]. */
size_t ls_sdf_rows_workspace_bytes(const ls_model_t* m, int B, long long R);
int ls_sdf_decode_rows(ls_model_t* m, const float* query, const int32_t* row_inst, const float* z_so3, const float* z_inv,
                       const float* s, const float* t, int B, long long R, float* sdf, void* workspace, size_t workspace_bytes,
                       void* stream);

/* SURVEY.md 8 (f-1), the autograd half: what `loss.backward()` computes in More_Solver._optimize_code
 * (lib_more/more_solver.py:191-228) through FieldWrapper.forward (model_utils.py:230-263) and DeepSDF_Decoder.forward
 * (deepsdf_decoder.py:78-123).  ls_sdf_decode_train = ls_sdf_decode keeping every layer's activations in `workspace`
 * (ls_sdf_train_workspace_bytes); ls_sdf_backward, called with the SAME arguments and workspace, returns the gradients of
 * sum(grad_sdf * sdf):  grad_query [B,M,3] (nullable), grad_z_so3 [B,c,3], grad_z_inv [B,c] (nullable TOGETHER: a pose refinement
 * with a fixed code -- more_solver.py:137-173 -- skips the code-gradient reductions), grad_s [B], grad_t [B,3]. */
size_t ls_sdf_train_workspace_bytes(const ls_model_t* m, int B, int M);
int ls_sdf_decode_train(ls_model_t* m, const float* query, const float* z_so3, const float* z_inv, const float* s,
                        const float* t, int B, int M, float* sdf, void* workspace, size_t workspace_bytes, void* stream);
int ls_sdf_backward(ls_model_t* m, const float* query, const float* z_so3, const float* z_inv, const float* s, const float* t,
                    int B, int M, const float* sdf, const float* grad_sdf, void* workspace, size_t workspace_bytes,
                    float* grad_query, float* grad_z_so3, float* grad_z_inv, float* grad_s, float* grad_t, void* stream);

/* SURVEY.md 8 (f-1), registration half: the log-domain softmin of entropic OT with cost |x-y|^2/2, the primitive of
 * geomloss.SamplesLoss('sinkhorn', p=2) as used at lib_more/more_solver.py:146,158 (geomloss itself is absent: the
 * epsilon-scaling loop around this primitive, livingscenes_amd/sinkhorn.py, is restated from memory -- parity unpinned):
 *   out[i] = -eps log sum_j exp(h[j] - |x_i - y_j|^2 / (2 eps));  grad_x[i] (nullable) = d out[i] / d x_i
 * x [N,3], y [M,3], h [M] (log-weight + potential / eps). */
int ls_sinkhorn_softmin_f32(const float* x, const float* y, const float* h, int N, int M, float eps, float* out, float* grad_x,
                            void* stream);

/* SURVEY.md 8 (f-1), registration half, BATCHED over P pairs (csrc/optim.hip): the device side of one step of
 * More_Solver._solve_pairwise_registration(optim=True) (lib_more/more_solver.py:118-189) for P pairs in lock-step.
 *   ls_se3_transform_f32         query[p] = g[p] . src[p]       g [P,3,4] (R | t), src / query [P,N,3]                  (:149)
 *   ls_smooth_l1_f32             loss[p] (+)= mean_i SmoothL1(sdf[p,i], 0);  grad_sdf[p,i] = d loss[p] / d sdf[p,i]       (:152-156)
 *   ls_sinkhorn_softmin_batched_f32   ls_sinkhorn_softmin_f32 with a pair index: out[p,i] = -eps_p log sum_j exp(logw + pot_y[p,j] / eps_p
 *                                - |x_i - y_j|^2 / (2 eps_p)) (averaged with prev[p,i] if `average`); eps_p <= 0: out = prev (schedule
 *                                of that pair has ended); grad_x optional; out must not alias prev                           (:146,158)
 *   ls_se3_adam_step_f32         tangent gradient (sum G, sum query x G) -> Adam moments m1 / m2 [P,6] -> g <- exp(-step) g; best-loss
 *                                snapshot best_g / min_loss (after the step, as the reference); geodesic angle to init_R [P,3,3] above
 *                                stop_angle -> active[p] = 0 (frozen from then on); query <- g . src for the next step             (:160-173)
 * torchlie / geomloss / roma are absent: retraction and Sinkhorn loop are this build's definitions (PARITY UNPINNED). */
int ls_se3_transform_f32(const float* g, const float* src, int P, int N, float* query, void* stream);
int ls_smooth_l1_f32(const float* sdf, int P, int N, int accumulate, float* loss, float* grad_sdf, void* stream);
int ls_sinkhorn_softmin_batched_f32(const float* x, const float* y, const float* pot_y, float logw, const float* eps, const float* prev,
                                    int average, int P, int N, int M, float* out, float* grad_x, void* stream);
/* Up to four independent batched softmins in one launch (the four potentials of one symmetric Sinkhorn iteration): the same
 * arithmetic as ls_sinkhorn_softmin_batched_f32 without the gradient, problem i on x [P,N,3], y [P,M,3], pot_y [P,M] or NULL. */
typedef struct ls_softmin_problem {
    const float* x;
    const float* y;
    const float* pot_y;
    const float* prev;
    float* out;
    float logw;
    int N, M;
} ls_softmin_problem;
int ls_sinkhorn_softmin_multi_f32(const ls_softmin_problem* problems, int count, const float* eps, int average, int P, void* stream);
/* More_Solver._optimize_code's loss and optimizer on the device (more_solver.py:199-221: MSELoss(sdf, 0), torch.optim.Adam with three
 * parameter groups -- z_inv 1e-5, t 1e-4, z_so3 5e-4 -- MultiStepLR([160]), best-loss bookkeeping):
 *   ls_mse_f32: loss[p] = mean_i sdf[p,i]^2, grad_sdf[p,i] = 2 sdf[p,i] / N; min_loss / improved (nullable, [P]): if loss[p] <
 *               min_loss[p] then min_loss[p] = loss[p], improved[p] = 1 (:219-221);
 *   ls_adam_step_f32: one Adam step (no weight decay, no amsgrad, torch's operation order) on up to four tensors, each with its own
 *               learning rate; step = 0-based step count (bias corrections use step + 1). */
typedef struct ls_adam_group {
    float* param;
    const float* grad;
    float* m;
    float* v;
    long long n;
    double lr;
} ls_adam_group;
int ls_mse_f32(const float* sdf, int P, int N, float* loss, float* grad_sdf, float* min_loss, int32_t* improved, void* stream);
/* betas, eps and learning rates are DOUBLES (torch.optim.Adam's Python floats): 1 - beta, 1 - beta^t, lr / (1 - beta1^t), sqrt(1 - beta2^t) are formed
 * in double on the host and rounded to fp32 once, as torch hands them to its kernels */
int ls_adam_step_f32(const ls_adam_group* groups, int count, double beta1, double beta2, double adam_eps, int step, void* stream);
int ls_se3_adam_step_f32(const float* src, const float* grad_query, const float* loss, int P, int N, double lr, double beta1, double beta2,
                         double adam_eps, int step, float stop_angle, float* g, float* m1, float* m2, float* min_loss, float* best_g,
                         const float* init_R, int32_t* active, float* query, void* stream);

/* ------------------------------------------------------------------------------------------------
 * SURVEY.md 8 (f-2), first half: the MISE octree that decides WHICH lattice points of the (R+1)^3 grid the decoder has to
 * evaluate (R = resolution_0 << depth) and assembles the dense value grid -- class MISE of
 * occnet_utils/utils/libmise/mise.pyx, driven by the loop of occnet_utils/mesh_extractor2.py:116-131:
 *     init;  loop { query -> n points; if n == 0 break; values = decoder(points); update(points, values) };  to_dense
 * `state` is caller-allocated device memory of ls_mise_state_bytes(); lattice index = (x*(R+1) + y)*(R+1) + z.
 * (Marching cubes -- libmcubes -- follows below: ls_marching_cubes_*.)
 * ---------------------------------------------------------------------------------------------- */
size_t ls_mise_state_bytes(int resolution_0, int depth);
long long ls_mise_lattice_points(int resolution_0, int depth);   /* (R+1)^3: upper bound for a query */
/* MISE.__cinit__, mise.pyx:43-85 */
int ls_mise_init(void* state, size_t state_bytes, int resolution_0, int depth, void* stream);
/* MISE.query, mise.pyx:104-126 (+ the coordinate normalisation of mesh_extractor2.py:122-124, box_size = 1 + padding):
 * unknown points in ascending lattice order -> idx_out [cap] int32, pts_out [cap,3]; *count_out (DEVICE int32) = number of
 * unknown points (nothing is written past cap). */
int ls_mise_query(void* state, int resolution_0, int depth, float box_size, int32_t* idx_out, float* pts_out, int cap,
                  int32_t* count_out, void* stream);
/* MISE.update, mise.pyx:87-102 + subdivide_voxels :188-236; threshold = logit of the occupancy threshold (double, as the reference) */
int ls_mise_update(void* state, int resolution_0, int depth, double threshold, const int32_t* idx, const float* values, int n,
                   void* stream);
/* MISE.to_dense, mise.pyx:128-165 -> grid_out [(R+1)^3] float32 (the reference's float64 grid holds float32 values) */
int ls_mise_to_dense(void* state, int resolution_0, int depth, float* grid_out, void* stream);

/* B octrees per launch.  All octrees of a batch share (resolution_0, depth, threshold).  A batch state is B single states back to back,
 * stride ls_mise_state_bytes() (a multiple of 256), followed by the block sums of the batched query: slice b of a batch state is a valid
 * state for the single ops above, and ls_mise_batch_state_bytes() = B * ls_mise_state_bytes() + that tail (0 for arguments the batch ops
 * refuse).  Every batch op is the single op on every slice, bit for bit, in a number of launches that does not depend on B.
 * Limits: 1 <= B <= 65535 (the octree is a grid dimension of the launch) and B * (R+1)^3 < 2^31 (packed rows are counted in int32). */
size_t ls_mise_batch_state_bytes(int B, int resolution_0, int depth);
int ls_mise_init_batch(void* state, size_t state_bytes, int B, int resolution_0, int depth, void* stream);
/* The unknown points of octree 0 first, in ascending lattice index, then those of octree 1, ...: idx_out [cap] int32 = lattice index within
 * the octree, inst_out [cap] int32 = the octree (exactly the row_inst of ls_sdf_decode_rows), pts_out [cap,3] float32 by the formula of
 * ls_mise_query.  off_out (DEVICE long long [B+1]): off_out[b] = first row of octree b, off_out[B] = the total -- always the full counts;
 * nothing is written at or past row cap.  An octree without unknown points has an empty slice. */
int ls_mise_query_batch(void* state, int B, int resolution_0, int depth, float box_size, int32_t* idx_out, int32_t* inst_out,
                        float* pts_out, long long cap, long long* off_out, void* stream);
/* values[i] belongs to lattice point idx[i] of octree inst[i] (a row naming no octree or no lattice point is dropped); then clear / mark /
 * subdivide for every octree.  Per octree the result equals driving it alone through the loop above: an octree whose query came back empty
 * is at a fixed point of the update (its last update subdivided nothing, so marking again reproduces the same marks). */
int ls_mise_update_batch(void* state, int B, int resolution_0, int depth, double threshold, const int32_t* idx, const int32_t* inst,
                         const float* values, long long n, void* stream);
/* grid_out [B, R+1, R+1, R+1] float32 */
int ls_mise_to_dense_batch(void* state, int B, int resolution_0, int depth, float* grid_out, void* stream);

/* SURVEY.md 8 (f-2), second half: libmcubes.marching_cubes(volume, isovalue) as called by Generator3D.extract_mesh
 * (occnet_utils/mesh_extractor2.py:161-176; occnet_utils/utils/libmcubes/marchingcubes.h:23-196, marchingcubes.cpp:290-326,
 * pywrapper.cpp:90-108): volume [nx,ny,nz] float64 -> vertices [nv,3] float64 (with the library's +0.5 offset) and faces
 * [nf,3] int64, in the reference's vertex and face ORDER.  counts_out = DEVICE long long[2] {nv, nf}; call once with
 * vertices = faces = NULL to size the outputs (nothing past cap_v vertices / cap_f faces is written).  isovalue: the
 * reference narrows it to float (mcubes.pyx:22) -- pass the narrowed value. */
size_t ls_mcubes_workspace_bytes(int nx, int ny, int nz);
int ls_marching_cubes_f64(const double* volume, int nx, int ny, int nz, double isovalue, double* vertices, long long cap_v,
                          long long* faces, long long cap_f, long long* counts_out, void* workspace, size_t workspace_bytes,
                          void* stream);
/* B volumes of one shape per launch: volumes [B,nx,ny,nz] float64.  Vertices and faces are packed mesh after mesh, in the reference's order
 * inside each mesh, and face indices count from the mesh's own first vertex: slice b of the output is bit-identical to
 * ls_marching_cubes_f64 on volume b.  off_out (DEVICE long long [2][B+1]): [0][b] = first vertex of mesh b, [1][b] = its first face,
 * [.][B] = the totals -- always the full counts.  Sizing as above: a call with vertices = faces = NULL only fills off_out (read it once
 * per batch); nothing at or past cap_v vertices / cap_f faces of the packed outputs is written.
 * Limits: 1 <= B <= 65535, and the vertex / face-index bases stay int and share one 64-bit word while they are summed:
 * 15 * B * nx*ny*nz < 2^31 (a cube makes at most 15 face indices, a mesh at most 3 vertices per sample; this implies
 * 3 * B * ncubes < 2^31).  ls_mcubes_batch_workspace_bytes is 0 for arguments the op refuses. */
size_t ls_mcubes_batch_workspace_bytes(int B, int nx, int ny, int nz);
int ls_marching_cubes_batch_f64(const double* volumes, int B, int nx, int ny, int nz, double isovalue, double* vertices, long long cap_v,
                                long long* faces, long long cap_f, long long* off_out, void* workspace, size_t workspace_bytes,
                                void* stream);

/* libsimplify.simplify_mesh(mesh, f_target, agressiveness) as called by Generator3D.extract_mesh with (mesh, simplify_nfaces, 5.0)
 * (occnet_utils/mesh_extractor2.py:205-208; occnet_utils/utils/libsimplify/__init__.py:7-17, simplify_mesh.pyx:34-88,
 * Simplify.h:345-445): quadric-error edge-collapse decimation down to `target_faces` triangles.  A sequential greedy algorithm the
 * reference runs on the CPU too: HOST arrays in and out.  vertices [nv,3] float64, faces [nf,3] int64 -> vertices_out (room for
 * nv rows), faces_out (room for nf rows), counts_out {nv', nf'}; vertices, faces and their ORDER are bit-identical to the reference.
 * initial_border: the value Vertex::border holds while the INITIAL edge costs are computed -- the reference never initialises it
 * (simplify_mesh.pyx:42 copies an uninitialised temporary; Simplify.h resets it only after the costs, :683): 1 = what every build of
 * the reference made here reads (non-zero: initial costs from the best of a, b, midpoint) and what the fixtures pin; 0 = as published. */
int ls_simplify_mesh_f64_host(const double* vertices_host, long long nv, const long long* faces_host, long long nf, int target_faces,
                              double aggressiveness, int initial_border, double* vertices_out_host, long long* faces_out_host,
                              long long* counts_out_host);

/* ------------------------------------------------------------------------------------------------
 * Reconstruction metrics of the reference's evaluate.py (csrc/meshmetrics.hip) on ONE triangle mesh: vertices [nv,3] float64, faces [nf,3]
 * int32 (indices in [0, nv)), points [n,3] float64.  nf == 0 is an empty mesh: it contains nothing and is infinitely far away.
 * Data-dependent sizes follow ls_marching_cubes_f64: the binned ops list every triangle in the cells of a grid; a call with entries == NULL
 * writes the number of entries to the DEVICE long long count_out and stops (points and outputs are not read); the caller allocates
 * entries [count] int32 and repeats the call with cap_entries >= count (with a smaller cap the outputs are undefined; nothing at or past
 * cap_entries is written).  workspace: the ls_*_workspace_bytes query of the op (a bound computable from the dimensions).
 * ---------------------------------------------------------------------------------------------- */

/* libmesh.check_mesh_contains(mesh, points, hash_resolution) (lib_shape_prior/core/models/utils/occnet_utils/utils/libmesh/inside_mesh.py:5-154,
 * triangle_hash.pyx), as called by evaluate.py:45 compute_volumetric_iou: inside_out [n] uint8 (0 / 1), BIT-IDENTICAL to the reference
 * (same float64 operations in the same order, same 2-D hash of hash_resolution^2 cells).  2 <= hash_resolution <= 4096. */
size_t ls_mesh_contains_workspace_bytes(int nf, int hash_resolution);
int ls_mesh_contains_f64(const double* vertices, int nv, const int32_t* faces, int nf, const double* points, long long n, int hash_resolution,
                         uint8_t* inside_out, int32_t* entries, long long cap_entries, long long* count_out, void* workspace,
                         size_t workspace_bytes, void* stream);

/* |pcu.signed_distance_to_mesh(points, V, F)| under a cap, for evaluate.py:100-106 compute_sdf_recall (which only tests |sdf| < thres):
 * dist_out [n] float64 = the distance from point i to the closest point of any triangle (Ericson, Real-Time Collision Detection 5.1.5;
 * triangles of zero area as their edges) when it is < max_dist, +inf otherwise.  max_dist > 0 and finite. */
size_t ls_mesh_distance_workspace_bytes(int nf);
int ls_mesh_distance_f64(const double* vertices, int nv, const int32_t* faces, int nf, const double* points, long long n, double max_dist,
                         double* dist_out, int32_t* entries, long long cap_entries, long long* count_out, void* workspace,
                         size_t workspace_bytes, void* stream);

/* trimesh.sample.sample_surface(mesh, count) as called at evaluate.py:25 compute_chamfer_distance: face = first index whose cumulative area
 * (a device scan: rounding differs from numpy's sequential cumsum) reaches u0 * total, (r1, r2) folded into the triangle when r1 + r2 > 1,
 * p = v0 + (r1 (v1 - v0) + r2 (v2 - v0)).  The uniforms are reproducible where trimesh's are not: u = (splitmix64(key + (j + 1) * 0x9E3779B97F4A7C15)
 * >> 11) * 2^-53 with key = splitmix64(seed + 0x9E3779B97F4A7C15) and j = 3 i + {0, 1, 2} for (u0, r1, r2) of sample i.
 * points_out [count,3] float64, face_out [count] int64 or NULL.  nf > 0, count > 0. */
size_t ls_mesh_sample_workspace_bytes(int nf);
int ls_mesh_sample_f64(const double* vertices, int nv, const int32_t* faces, int nf, long long count, unsigned long long seed,
                       double* points_out, int64_t* face_out, void* workspace, size_t workspace_bytes, void* stream);

/* The three metrics on M meshes per call (ragged batches).  The meshes are stored back to back: mesh m owns vertices
 * [vert_off[m], vert_off[m+1]), faces [face_off[m], face_off[m+1]) -- indices LOCAL to the mesh -- and points (samples: count_off)
 * [pt_off[m], pt_off[m+1]).  The offsets are HOST int64 arrays of M + 1 entries starting at 0, never decreasing and ending at the totals
 * (nv_total, nf_total, n_total / count_total); the entry checks them, and every argument check of the single-mesh op, per mesh (the error
 * names the mesh), and copies them into its workspace on the stream.  hash_resolution and max_dist hold for the whole batch.  For every
 * mesh the result is BIT-IDENTICAL to the single-mesh op on that mesh alone (an empty mesh contains nothing and is infinitely far away).
 * The number of launches does not depend on M.  The binned ops follow the single ops' sizing convention with ONE entry count for the whole
 * batch.  Workspace: contains holds hash_resolution^2 cells per mesh; distance gives mesh m a grid of at most a^3 cells, a = the largest
 * integer <= 128 with a^3 <= 8 nf_m (at least 1), so at most 8 nf_total + M cells in all.  The sampler takes M seeds (device), zero
 * samples for a mesh are allowed (a mesh with faces is then not scanned), samples of an empty mesh are refused; face_out is local to the
 * mesh.  The *_workspace_bytes helpers return 0 for invalid arguments. */
size_t ls_mesh_contains_batch_workspace_bytes(int M, long long nf_total, int hash_resolution);
int ls_mesh_contains_batch_f64(int M, const double* vertices, long long nv_total, const long long* vert_off, const int32_t* faces, long long nf_total,
                               const long long* face_off, const double* points, long long n_total, const long long* pt_off, int hash_resolution,
                               uint8_t* inside_out, int32_t* entries, long long cap_entries, long long* count_out, void* workspace,
                               size_t workspace_bytes, void* stream);
size_t ls_mesh_distance_batch_workspace_bytes(int M, long long nf_total);
int ls_mesh_distance_batch_f64(int M, const double* vertices, long long nv_total, const long long* vert_off, const int32_t* faces, long long nf_total,
                               const long long* face_off, const double* points, long long n_total, const long long* pt_off, double max_dist,
                               double* dist_out, int32_t* entries, long long cap_entries, long long* count_out, void* workspace,
                               size_t workspace_bytes, void* stream);
size_t ls_mesh_sample_batch_workspace_bytes(int M, long long nf_total);
int ls_mesh_sample_batch_f64(int M, const double* vertices, long long nv_total, const long long* vert_off, const int32_t* faces, long long nf_total,
                             const long long* face_off, long long count_total, const long long* count_off, const unsigned long long* seeds,
                             double* points_out, int64_t* face_out, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Depth views of triangle meshes and their back-projection (csrc/meshrender.hip, csrc/render_plan.h): the device counterpart of the
 * reference's utils/render.py (render_depth / pointcloud), which renders with pyrender's OpenGL rasteriser.  PARITY WITH THAT RASTERISER
 * IS NOT PINNED (pyrender is not available to the tests); the semantics are defined here and tests/render_oracle.py is the same text as
 * NumPy, which the kernels reproduce bit for bit.  Everything is float64 unless stated, no contraction anywhere.
 * Per view: world_to_cam E [3,4] (camera: x right, y down, z forward), intrinsics (fx, fy, cx, cy); per call H, W, znear > 0.
 * Per (view, face), corners i = 0, 1, 2 at (x, y, z):
 *   1. c_i = ((E[:,0] x + E[:,1] y) + E[:,2] z) + E[:,3]
 *   2. near test: the face is dropped for the view if any c_i.z < znear or is not finite (no clipping)                    -> counts[2]
 *   3. u_i = fx (c_i.x / c_i.z) + cx, v_i = fy (c_i.y / c_i.z) + cy
 *   4. snap to 1/256 pixel: xs_i = (int64) floor(u_i 256 + 0.5), ys_i likewise; the face is dropped if a value is not finite or exceeds
 *      2^24 in magnitude (every edge function then stays below 2^53)                                                    -> counts[3]
 *   5. pixel box px in [ceil(min xs / 256), floor(max xs / 256)] clipped to [0, W-1], py likewise (floor / ceil division of negative
 *      integers included); a face that got here with A != 0 (below; A is the same at every pixel) is counted             -> counts[1]
 *   6. at pixel (px, py): X = 256 px, Y = 256 py (the ray goes through the INTEGER pixel coordinate, so ls_depth_points_f32 is the exact
 *      inverse); edge(i,j) = (xs_j - xs_i)(Y - ys_i) - (ys_j - ys_i)(X - xs_i) in int64; e0 = edge(1,2), e1 = edge(2,0), e2 = edge(0,1),
 *      A = e0 + e1 + e2.  Covered iff A != 0 and (all three >= 0 or all three <= 0): no back-face culling, inclusive edges -- integer edge
 *      functions are exactly antisymmetric, so both faces at a shared edge cover its pixels and there are no cracks.
 *      z = A / ((e0 iz_0 + e1 iz_1) + e2 iz_2) with iz_i = 1.0 / c_i.z (perspective-correct), d = (float) z.
 *   7. the pixel's winner is the minimum of the key (bits of d as uint32) << 32 | face index (local to the mesh): nearest depth, on equal
 *      fp32 depth the lower face index.
 * Outputs (DEVICE): depth_out [views,H,W] fp32 (0: nothing hit, pyrender's convention), face_out [views,H,W] int32 (-1: none), counts_out
 * [views,4] = pixels hit, faces counted at step 5, faces dropped at the near test, faces dropped at the snap; status_out [1] = LS_OK, or
 * LS_ERR_INVALID when a face names a vertex outside its mesh (the images are then unspecified; the binding raises).
 * vertices [nv,3] float64, faces [nf,3] int32, world_to_cam [views,3,4] and intrinsics [views,4] float64, all DEVICE.  nf = 0 and
 * n_views = 0 are allowed.  views H W < 2^31 and views nf < 2^31, znear finite and > 0: refused on the host otherwise.
 * Launches: three memsets (the key image, the counts, the status), the rasteriser -- one thread per (view, face) does steps 1 - 5 and walks
 * a box of at most RENDER_SMALL_BOX pixels itself; the larger boxes of a wave are walked by its 64 lanes together --, the strip pass -- in a
 * call with few items the large boxes are walked there instead, one wave per (64 items, strip of the image); otherwise one idle workgroup
 * -- and the resolve pass.  Their number depends on nothing.  No host synchronisation, no allocation; the only atomics are atomicMin on the 64-bit key and one
 * integer add per wave, view and counter: every output is the same bits in any run.  The workspace is the key image: 8 views H W bytes. */
size_t ls_mesh_render_depth_workspace_bytes(int n_views, int height, int width);
int ls_mesh_render_depth_f64(const double* vertices, int nv, const int32_t* faces, int nf, int n_views, const double* world_to_cam,
                             const double* intrinsics, int height, int width, double znear, float* depth_out, int32_t* face_out,
                             long long* counts_out, int* status_out, void* workspace, size_t workspace_bytes, void* stream);
/* M meshes stored back to back as in ls_mesh_contains_batch_f64 (vert_off / face_off: HOST int64 [M+1], faces local to their mesh), mesh m
 * rendered into the views [view_off[m], view_off[m+1]) (HOST int64 [M+1]) of the views_total images; one H x W and one znear per call.  The
 * offsets are checked on the host before the first HIP call and copied to the workspace.  A mesh with no views and a mesh with no faces
 * are allowed (its views come out empty).  Every image is BIT-IDENTICAL to ls_mesh_render_depth_f64 on that mesh alone, and the number of
 * launches does not depend on M.  The workspace depends on (M, views_total, H, W) alone: the key image and the offsets. */
size_t ls_mesh_render_depth_batch_workspace_bytes(int M, long long views_total, int height, int width);
int ls_mesh_render_depth_batch_f64(int M, const double* vertices, long long nv_total, const long long* vert_off, const int32_t* faces,
                                   long long nf_total, const long long* face_off, long long views_total, const long long* view_off,
                                   const double* world_to_cam, const double* intrinsics, int height, int width, double znear, float* depth_out,
                                   int32_t* face_out, long long* counts_out, int* status_out, void* workspace, size_t workspace_bytes,
                                   void* stream);
/* The back-projection of `views` depth maps (the reference's pointcloud plus the move to another frame): depth [views,H,W] fp32,
 * intrinsics [views,4] float64, cam_to_world M [views,3,4] float64 or NULL (the camera frame), all DEVICE.  Per view, every pixel with
 * d > 0 in ascending py W + px (the order of np.where):
 *   xc = ((px - cx) / fx) d, yc = ((py - cy) / fy) d, zc = d;  p = ((M[:,0] xc + M[:,1] yc) + M[:,2] zc) + M[:,3], rounded to fp32
 * pts_out [views H W,3] fp32 and pix_out [views H W] int32 (the pixel index py W + px) are sized by the caller for every pixel; the rows
 * of view v are [off_out[v], off_out[v+1]), off_out [views+1] int64 DEVICE.  Flag, two-level scan, scatter: 6 launches, no host
 * synchronisation, no atomics.  views H W is at most 2^24 (the scan's reach). */
size_t ls_depth_points_workspace_bytes(long long views, int height, int width);
int ls_depth_points_f32(const float* depth, long long views, int height, int width, const double* intrinsics, const double* cam_to_world,
                        float* pts_out, int32_t* pix_out, long long* off_out, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Decimation on the device (csrc/meshcluster.hip): vertex clustering on a uniform grid with quadric-optimal representatives (Lindstrom
 * 2000, regularised solve).  A SECOND decimator beside ls_simplify_mesh_f64_host, chosen explicitly: data-parallel and deterministic, it
 * does not reproduce the reference's edge collapse.  vertices [nv,3] float64, faces [nf,3] int64 (local to the mesh), all on the device.
 * Non-finite coordinates are not supported (every index stays in range, the output is unspecified).  Per mesh, in float64 and without
 * contraction, with the sums taken in the stated order (tests/cluster_oracle.py is the same text as NumPy):
 *   1. nf <= f_target (an empty mesh included): the output is the input unchanged, r = 0.
 *   2. grid: lo = per-axis minimum over ALL vertices, ext = the largest axis extent (1 if it is 0); at resolution r, h = ext / r, the cell
 *      of v is c_a = min(r - 1, (int)floor((v_a - lo_a) / h)) per axis, key = (c_x r + c_y) r + c_z.
 *   3. resolution: n_keep(r) = faces whose three corners have three different keys.  lo = 1, hi = r_max; while lo < hi: mid = (lo + hi + 1) / 2,
 *      n_keep(mid) <= f_target ? lo = mid : hi = mid - 1.  r* = lo -- defined by this procedure, monotonicity of n_keep is not assumed.
 *   4. faces at r*: faces with two equal corner keys are dropped; the others are grouped by their UNORDERED key triple; a group with an even
 *      number of members is dropped, one with an odd number keeps its member of lowest input index.  Output faces keep ascending input
 *      order and their corner order.  (The map is simplicial, so cancelling in pairs keeps a surface closed mod 2 closed mod 2: ray-parity
 *      tests such as ls_mesh_contains_f64 keep working.)
 *   5. vertices: the output cells are those named by an output face, in ascending key order; a face's indices are the ranks of its cells.
 *      xbar = the mean of all input vertices of the cell, summed in ascending vertex index.  The quadric about xbar runs over every corner
 *      of every INPUT face (dropped ones included) whose key is the cell, in ascending (face, corner): n = (p1 - p0) x (p2 - p0), a = |n|,
 *      skipped if a = 0, nh = n / a, A += a nh nh^T, g += a (nh . (p0 - xbar)) nh.  (A + 1e-3 tr(A) I) delta = g (delta = 0 if tr(A) = 0);
 *      x = xbar + delta clamped per axis to the cell's box [lo_a + c_a h, lo_a + (c_a + 1) h].
 * No floating-point atomics: a mesh's output bits are the same alone, in any batch and in any run.
 * Limitation: two sheets closer than one cell map to the same triangles and cancel, so a thin part (a chair leg) can vanish where the edge
 * collapse keeps it -- which is why this decimator is never a default.
 * Conventions of ls_marching_cubes_f64: counts_out = DEVICE long long[2] {nv', nf'}, always the full counts; a call with vertices_out =
 * faces_out = NULL (both or neither) writes only the counts and r_out; nothing at or past cap_v vertices / cap_f faces is written.  Caps
 * that are too small are an error: where the host can tell (a mesh under the target is copied) the call is refused, otherwise the mesh's
 * r_out is LS_ERR_INVALID.  r_out (DEVICE int, nullable here): r*, 0 for a copied mesh, or a negative ls_status for the mesh:
 * LS_ERR_INVALID (a face index outside [0, nv) -- such faces are ignored -- or the caps), LS_ERR_WORKSPACE (the triple hash overflowed;
 * it holds 2 f_target + 1 slots for at most f_target triples and its probe walk is bounded by the table, so this reports a defect, it
 * never spins).  1 <= f_target, 1 <= r_max <= 256, nv + 3 nf <= INT_MAX.  The workspace is the caller's (the cell bitmap alone is
 * r_max^3 bits per mesh: 2 MB at 256); everything is enqueued on the stream, and arguments are checked before the first launch. */
size_t ls_mesh_cluster_workspace_bytes(long long nv, long long nf, int r_max);
int ls_mesh_cluster_f64(const double* vertices, long long nv, const long long* faces, long long nf, int f_target, int r_max, double* vertices_out,
                        long long cap_v, long long* faces_out, long long cap_f, long long* counts_out, int* r_out, void* workspace,
                        size_t workspace_bytes, void* stream);
/* M >= 1 meshes per call, stored back to back as for the mesh metrics (HOST int64 offsets of M + 1 entries, checked here -- the error names
 * the mesh -- and copied into the workspace on the stream); f_target and r_max hold for every mesh.  The outputs are packed mesh after mesh
 * with face indices local to each mesh; off_out (DEVICE long long [2][M+1]): [0][m] = first output vertex of mesh m, [1][m] = its first
 * face, [.][M] = the totals, always the full counts; r_out DEVICE int [M].  Every mesh is BIT-IDENTICAL to ls_mesh_cluster_f64 on that
 * mesh alone, and the number of launches does not depend on M.  ls_mesh_cluster_batch_workspace_bytes is 0 for arguments the op refuses. */
size_t ls_mesh_cluster_batch_workspace_bytes(int M, long long nv_total, long long nf_total, int r_max);
int ls_mesh_cluster_batch_f64(int M, const double* vertices, long long nv_total, const long long* vert_off, const long long* faces, long long nf_total,
                              const long long* face_off, int f_target, int r_max, double* vertices_out, long long cap_v, long long* faces_out,
                              long long cap_f, long long* off_out, int* r_out, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Scene memory (csrc/cloudmerge.hip): the cloud an instance keeps, merged with a registered new observation of it on a voxel grid.  AN
 * EXTENSION BEYOND THE RELEASED REFERENCE: its README promises "a joint optimization algorithm that facilitates the accumulation of point
 * clouds originating from the same instance", but more_solver.py:246-299 (_solve_end2end) matches and registers one (reference, rescan)
 * pair and stops -- nothing carries an instance's points from one rescan to the next.  This is the step in between: pose-aligned merging
 * with a bound on the growth (one point per voxel).  Definition, per problem (tests/merge_oracle.py is the same text as NumPy):
 *   inputs      A [a,3] fp32 the kept cloud, B [b,3] fp32 the new observation, g [3,4] fp32 (R | t) taking B into A's frame (NULL: the
 *               identity, and then B is used bit for bit), h > 0 the voxel edge.  All DEVICE pointers except h.  a = 0 and b = 0 are allowed.
 *   candidates  in this order: the rows of A as given, then the rows of B transformed, y_a = ((R_a0 x_0 + R_a1 x_1) + R_a2 x_2) + t_a with
 *               every product and every sum rounded to fp32 in that order (no fma).
 *   cell        inv = (float)1 / (float)h, formed once on the host; c_a = floorf(y_a * inv) clamped to [-2^30, 2^30] and cast to int32 -- a
 *               multiplication, not a division, in the kernel.  h and inv must be finite and positive.
 *   non-finite  a candidate with a non-finite coordinate (after the transform) has no cell and is never kept.
 *   keep        candidate i is kept iff no candidate j < i of the same problem has the same cell triple.  So points already in the
 *               memory win over new ones, a cloud that is itself the output of a merge at the same h is kept whole, and
 *               merge(merge(A, B), {}) == merge(A, B).
 * Outputs, sized BY THE CALLER at the upper bound a + b rows (no sizing pass, no host synchronisation, no allocation): out_pts [.,3] the
 * kept candidates in ascending candidate order (rows of A: the input bits; rows of B: the transformed point), out_src int32 their
 * candidate index in [0, a + b) (>= a: it came from B), out_off DEVICE long long [2] = {0, n_out}.  status_out (DEVICE int, nullable):
 * LS_OK, or LS_ERR_WORKSPACE if the cell table overflowed -- it holds 2 (a + b) slots for at most a + b cells and its probe walk is bounded
 * by the table, so this reports a defect, it never spins.  a + b <= INT_MAX.  Integer atomics only: the output does not depend on the run. */
size_t ls_cloud_merge_workspace_bytes(long long a, long long b);
int ls_cloud_merge_f32(const float* A, long long a, const float* B, long long b, const float* g, float voxel, float* out_pts, int32_t* out_src,
                       long long* out_off, int* status_out, void* workspace, size_t workspace_bytes, void* stream);
/* P >= 1 problems per call: A [a_total,3] and B [b_total,3] hold the problems' rows back to back, a_off / b_off (HOST int64, P + 1 entries)
 * and voxel (HOST float, P entries) are checked here -- starting at 0, never decreasing, ending at the totals, h finite and > 0; the error
 * names the problem -- and copied into the workspace on the stream; g [P,3,4] DEVICE or NULL (identity for every problem).  The outputs
 * are packed problem after problem: out_off DEVICE long long [P+1], out_src local to its problem, status_out DEVICE int [P] (nullable).
 * a_total + b_total <= INT_MAX.  Every output of every problem is BIT-IDENTICAL to ls_cloud_merge_f32 on that problem alone, in any batch
 * composition and in any run, and the number of launches does not depend on P.  The workspace queries return 0 for sizes the op refuses. */
size_t ls_cloud_merge_batch_workspace_bytes(int P, long long a_total, long long b_total);
int ls_cloud_merge_batch_f32(int P, const float* A, long long a_total, const long long* a_off, const float* B, long long b_total,
                             const long long* b_off, const float* g, const float* voxel, float* out_pts, int32_t* out_src, long long* out_off,
                             int* status_out, void* workspace, size_t workspace_bytes, void* stream);

/* Scene memory, the question before a merge (csrc/cloudnear.hip): does a registered observation lie on what the memory holds?  Fixed-radius
 * nearest neighbour between a kept cloud and a posed observation, with the overlap statistics of the pair.  AN EXTENSION BEYOND THE
 * RELEASED REFERENCE, like the merge: the reference has no such step.  Definition, per problem (tests/nearest_oracle.py is the same text as
 * NumPy):
 *   inputs      A [a,3] fp32 the kept cloud (targets), B [b,3] fp32 the observation (queries), g [3,4] fp32 (R | t) taking B into A's frame
 *               (NULL: the identity, and then B is used bit for bit), r > 0 the radius.  All DEVICE pointers except r.  a = 0 and b = 0 are
 *               allowed.
 *   queries     y_a = ((R_a0 x_0 + R_a1 x_1) + R_a2 x_2) + t_a, the expression and rounding of ls_cloud_merge_f32: every product and every
 *               sum rounded to fp32 in that order (no fma).
 *   cells       of edge r, by the merge's rule for targets and queries alike: inv = (float)1 / r, formed once on the host; c_a =
 *               floorf(x_a * inv) clamped to [-2^30, 2^30] and cast to int32.  A row with a non-finite coordinate has no cell: such a
 *               target is never a neighbour, such a query has no neighbour.  r, inv and r2 must be finite and positive.
 *   distance    d2(i,j) = ((dx dx + dy dy) + dz dz) with dx = y_0 - A[j][0] and so on, every operation rounded to fp32 in that order;
 *               r2 = r r rounded to fp32 on the host.
 *   neighbour   of query i: among the targets j whose cell differs from the query's cell by at most 1 on every axis and whose
 *               d2(i,j) <= r2, the one that is least under the order (d2, j): ties go to the lowest index.
 * The cell condition is PART OF THE DEFINITION, not an approximation of it: it makes the 27-cell search exact, and differs from the pure
 * radius test only where a coordinate difference lies within rounding of r (r = 0.25, target (-1e-30, 0, 0), query (0.25, 0, 0):
 * d2 == r2 == 0.0625, the cells are -1 and 1, the query has no neighbour).
 * Outputs: nn_idx int32 [b] the neighbour's row in A, local to the problem (-1: none); nn_d2 float [b] its d2 (+inf: none); counts
 * long long [3] = (finite queries, queries with a neighbour, targets that are the neighbour of at least one query); sum_d2 double [1] the
 * float64 sum of the nn_d2 of the queries that have a neighbour, by the per-problem rule of ls_reg_metrics_batch: chunks of 256 queries of
 * the problem, each added in a fixed order, the partials added in chunk order -- no floating-point atomics.  status_out (DEVICE int,
 * nullable): LS_OK, or LS_ERR_WORKSPACE if the cell table overflowed -- it holds 2 a slots for at most a cells and its probe walks are
 * bounded by the table, so this reports a defect, it never spins.  a + b <= INT_MAX.  No host synchronisation, no allocation; the
 * workspace is the caller's (ls_cloud_nearest_workspace_bytes: at most 96 bytes per target row and 1 byte per 16 query rows, plus the
 * alignment of its pieces).  Integer atomics only: every output is the same bits in any run. */
size_t ls_cloud_nearest_workspace_bytes(long long a, long long b);
int ls_cloud_nearest_f32(const float* A, long long a, const float* B, long long b, const float* g, float radius, int32_t* nn_idx, float* nn_d2,
                         long long* counts, double* sum_d2, int* status_out, void* workspace, size_t workspace_bytes, void* stream);
/* P >= 1 problems per call, with the conventions of ls_cloud_merge_batch_f32: A [a_total,3] and B [b_total,3] hold the problems' rows back
 * to back, a_off / b_off (HOST int64, P + 1 entries) and radius (HOST float, P entries) are checked here before the first HIP call -- the
 * error names the problem -- and copied into the workspace on the stream; g [P,3,4] DEVICE or NULL.  nn_idx / nn_d2 [b_total] are packed
 * problem after problem (nn_idx local to its problem), counts DEVICE long long [P,3], sum_d2 DEVICE double [P], status_out DEVICE int [P]
 * (nullable).  a_total + b_total <= INT_MAX.  Every output of every problem is BIT-IDENTICAL to ls_cloud_nearest_f32 on that problem
 * alone, in any batch composition and in any run, and the number of launches does not depend on P.  The workspace queries return 0 for
 * sizes the op refuses. */
size_t ls_cloud_nearest_batch_workspace_bytes(int P, long long a_total, long long b_total);
int ls_cloud_nearest_batch_f32(int P, const float* A, long long a_total, const long long* a_off, const float* B, long long b_total,
                               const long long* b_off, const float* g, const float* radius, int32_t* nn_idx, float* nn_d2, long long* counts,
                               double* sum_d2, int* status_out, void* workspace, size_t workspace_bytes, void* stream);

/* Scene memory, the pose both of the above trust (csrc/cloudnear.hip): trimmed ICP of an observation onto the kept cloud, on the search's
 * grid and at full resolution.  AN EXTENSION BEYOND THE RELEASED REFERENCE, like the merge and the search: the reference registers two
 * 1 024-point samples (pytorch3d's ICP, every source point paired with its nearest target) and has no memory to register against.  Here
 * the observation B moves onto the complete kept cloud A, and only correspondences within r count, so the part of A the view does not see
 * pulls on nothing.  Definition, per problem (tests/icp_oracle.py is the same text as NumPy), with the conventions of ls_cloud_nearest_f32:
 *   inputs      A [a,3] fp32 (targets), B [b,3] fp32 (queries), g0 [3,4] fp32 taking B into A's frame (NULL: the identity MATRIX, which
 *               goes through the query expression like any other pose), r > 0; host scalars max_iter >= 0, rel_thr >= 0 finite (double),
 *               min_matched >= 3.  g_0 = g0, and for k = 0, 1, ...:
 *   search      exactly ls_cloud_nearest_f32(A, B, g_k, r): the same query expression and rounding, cells of edge r, d2 and neighbour
 *               under (d2, j).  f_k = finite queries, n_k = matched queries, S_k = the float64 sum of the matched nn_d2 by the chunk rule
 *               of the search (256 queries per chunk in a fixed tree, partials in chunk order).
 *   cost        E_k = (S_k + (f_k - n_k) (double)r2) / f_k in float64 in that order; f_k = 0: E_k = 0.  This is the truncated quadratic
 *               sum_i min(d_i^2, r^2) / f.  The neighbours within r are exact (any target within r lies within one cell per axis), so
 *               neither the assignment nor the Kabsch step can raise it, although the matched set changes -- which the rmse of the matched
 *               points alone does not promise: it can rise when more points match.
 *   stop tests  in this order, each with g_out = g_k and iters = k: n_k < min_matched: LS_ICP_STARVED; k >= 1 and
 *               E_{k-1} - E_k <= rel_thr E_{k-1}: LS_ICP_CONVERGED; k == max_iter: LS_ICP_MAX_ITER.  At most max_iter updates and
 *               max_iter + 1 searches.
 *   update      over the matched queries, the ORIGINAL row x_i of B and its neighbour a_j, in float64 with the products formed in float64
 *               from the fp32 inputs (exact): sum x [3], sum a [3], sum x a^T [9], each by the chunk rule (a fixed order inside a chunk
 *               of 256 queries, partials in chunk order; no floating-point atomics).  mu_x = sum x / n, mu_a = sum a / n,
 *               H = sum x a^T - (sum x)(sum a)^T / n; R = the rotation of ls_kabsch_batched_f32 for the covariance H (x -> a), rounded to
 *               fp32; t = mu_a - R_fp32 mu_x in float64, rounded to fp32; g_{k+1} = (R | t).  If that solver reports anything but
 *               LS_KABSCH_OK (rank < 2 as it decides it: an exactly collinear or coincident matched set, or non-finite sums):
 *               LS_ICP_DEGENERATE, g_out = g_k, iters = k.  The UNCENTRED moments are a float64 choice: with coordinates up to a few
 *               hundred object extents from the origin the cancellation in H stays far below one fp32 ulp of the result.
 * Outputs: g_out [3,4] fp32; stop int32 (LS_ICP_*); iters int32; and the complete result of the final search -- nn_idx [b], nn_d2 [b],
 * counts [3], sum_d2 -- which are BIT FOR BIT what ls_cloud_nearest_f32(A, B, g_out, r) returns (it is the last search of the loop, not
 * one more); status_out as there.  Optional trace (both nullable): g_trace float [max_iter+1, 12] = g_k and stat_trace double
 * [max_iter+1, 3] = (f_k, n_k, S_k); the rows k <= iters are written, the others are left alone.
 * By construction: every output of a problem is the same bits alone, in any batch composition and in any run; a problem that has stopped
 * is frozen -- later iterations of its batch neither read nor write it; the number of launches depends on max_iter alone (2 max_iter + 5
 * after the grid build), not on P and not on when problems stop; no host synchronisation, no allocation, no waiting between workgroups,
 * and every loop on the device is bounded by the table size, the member count or the chunk count.  The workspace is the search's plus the
 * poses and one record of 15 float64 per chunk of queries; the queries return 0 for sizes the op refuses. */
#define LS_ICP_CONVERGED 0  /* the cost fell by no more than rel_thr of itself */
#define LS_ICP_MAX_ITER 1   /* max_iter updates were made */
#define LS_ICP_STARVED 2    /* fewer than min_matched correspondences within r */
#define LS_ICP_DEGENERATE 3 /* the matched pairs do not determine a rotation */
size_t ls_cloud_icp_workspace_bytes(long long a, long long b);
int ls_cloud_icp_f32(const float* A, long long a, const float* B, long long b, const float* g0, float radius, int max_iter, double rel_thr,
                     int min_matched, float* g_out, int32_t* stop, int32_t* iters, int32_t* nn_idx, float* nn_d2, long long* counts, double* sum_d2,
                     int* status_out, float* g_trace, double* stat_trace, void* workspace, size_t workspace_bytes, void* stream);
/* P >= 1 problems per call with the conventions of ls_cloud_nearest_batch_f32: a_off / b_off / radius are HOST arrays, checked with
 * max_iter, rel_thr and min_matched (shared by the batch) before the first HIP call -- the error names the problem; g0 [P,3,4] DEVICE or
 * NULL.  g_out [P,3,4], stop / iters [P], nn_idx / nn_d2 [b_total] packed, counts [P,3], sum_d2 [P], status_out [P] (nullable), g_trace
 * [P, max_iter+1, 12] and stat_trace [P, max_iter+1, 3] (nullable), all DEVICE.  Every output of every problem is BIT-IDENTICAL to
 * ls_cloud_icp_f32 on that problem alone. */
size_t ls_cloud_icp_batch_workspace_bytes(int P, long long a_total, long long b_total);
int ls_cloud_icp_batch_f32(int P, const float* A, long long a_total, const long long* a_off, const float* B, long long b_total,
                           const long long* b_off, const float* g0, const float* radius, int max_iter, double rel_thr, int min_matched,
                           float* g_out, int32_t* stop, int32_t* iters, int32_t* nn_idx, float* nn_d2, long long* counts, double* sum_d2,
                           int* status_out, float* g_trace, double* stat_trace, void* workspace, size_t workspace_bytes, void* stream);

/* Scene memory, a normal per kept point (csrc/cloudnear.hip): what the point-to-plane metric below needs and the memory does not hold.  AN
 * EXTENSION BEYOND THE RELEASED REFERENCE, like the merge, the search and the ICP.  Definition, per problem (tests/normals_oracle.py is the
 * same text as NumPy), with the conventions of ls_cloud_nearest_f32 -- cells of edge r, inv = 1.0f / r and r2 = r r formed on the host, all
 * three finite and positive.  For every row i of A [a,3] that has a cell:
 *   neighbours  the rows j of the same problem, i itself included, whose cell differs from i's by at most 1 on every axis and with
 *               d2 <= r2, dx = A[i][0] - A[j][0] and so on, d2 = ((dx dx + dy dy) + dz dz) in fp32: the search's expression with the query
 *               A[i] and no pose.  m_i is their number.
 *   moments     u = dx inv in fp32, q = (int)rintf(u 32768.0f) per axis (|q| <= 2^15); s1 [3] = sum q and s2 [6] = sum q_a q_b in int64
 *               (below 2^61 for any a <= INT_MAX).  The order of a cell's members depends on a race, so no float sum over them could be
 *               reproducible; these integer sums are, and NumPy's int64 gives the same integers.
 *   covariance  C_ab = (double)s2_ab - ((double)s1_a (double)s1_b) / (double)m_i, in this order, in float64.
 *   eigenvalues lmin <= lmid <= lmax of the symmetric C by cyclic Jacobi in float64.
 *   validity    the row is valid iff m_i >= min_nbrs, lmax > 0 and lmid > 2^-40 lmax: a coincident or collinear neighbourhood has no
 *               normal.  min_nbrs >= 1 is the caller's; the rank rule does the real work.
 *   normal      the unit eigenvector of lmin, rounded to fp32, with the sign that makes its component of largest fp32 magnitude (the first
 *               such) positive.  The sign is a convention only: point-to-plane does not depend on it.
 * Outputs: normals float [a,3]; nbr_cnt int32 [a] = m_i; variation float [a] = lmin / ((lmin + lmid) + lmax) in float64, rounded: the
 * surface variation, for callers who want to leave edges and corners out; an invalid row has the normal (0, 0, 0) and variation 0, a row
 * without a cell (a non-finite coordinate) also nbr_cnt 0; counts long long [2] = (rows with a cell, valid rows); status_out as in the search.
 * One thread per row walks the 27 cells of the search's grid with ten integer accumulators in registers; 2 launches after the grid build.
 * No host synchronisation, no allocation, integer atomics only and only on the table: every output is the same bits in any run. */
size_t ls_cloud_normals_workspace_bytes(long long a);
int ls_cloud_normals_f32(const float* A, long long a, float radius, int min_nbrs, float* normals, int32_t* nbr_cnt, float* variation,
                         long long* counts, int* status_out, void* workspace, size_t workspace_bytes, void* stream);
/* P >= 1 problems per call with the conventions of ls_cloud_nearest_batch_f32: a_off (HOST int64, P + 1 entries) and radius (HOST float,
 * P entries) are checked before the first HIP call -- the error names the problem; min_nbrs is shared by the batch; empty problems are
 * allowed.  normals [a_total,3], nbr_cnt / variation [a_total], counts [P,2], status_out [P] (nullable), all DEVICE.  Every output of every
 * problem is BIT-IDENTICAL to ls_cloud_normals_f32 on that problem alone, and the number of launches does not depend on P. */
size_t ls_cloud_normals_batch_workspace_bytes(int P, long long a_total);
int ls_cloud_normals_batch_f32(int P, const float* A, long long a_total, const long long* a_off, const float* radius, int min_nbrs,
                               float* normals, int32_t* nbr_cnt, float* variation, long long* counts, int* status_out, void* workspace,
                               size_t workspace_bytes, void* stream);

/* Scene memory, one projection of a kept cloud onto its local planes (csrc/cloudnear.hip): the repair step of a consolidation on request --
 * a kept point carries the sensor noise of the scan that delivered it, and the plane through its neighbourhood averages that noise out.
 * AN EXTENSION BEYOND THE RELEASED REFERENCE, like the normals, whose neighbourhood this is.  It MOVES kept points, which no merge does, so
 * nothing calls it unasked.  Definition, per problem (tests/project_oracle.py is the same text as NumPy).  For every row i of A [a,3] that
 * has a cell: the neighbours, m_i, the integer moments s1 / s2, the covariance, the eigenvalues and the validity rule of
 * ls_cloud_normals_f32, exactly.  Then, all in float64, for a valid row:
 *   normal      n_k = V[k][lo] / len, the unit eigenvector of lmin BEFORE any fp32 rounding; no sign rule: the result does not depend on it
 *   offset      unit = 1.0 / ((double)inv 32768.0); d_k = ((double)s1_k / (double)m_i) unit: the row minus the centroid of its
 *               neighbourhood, from the integers, so the same near the origin and 300 m from it
 *   distance    s = (d_0 n_0 + d_1 n_1) + d_2 n_2: the signed distance of the row to the plane through the centroid
 *   variation   lmin / ((lmin + lmid) + lmax), as in the normals but not rounded
 * state int32 [a], out_pts float [a,3], shift float [a]:
 *   0  no cell (a non-finite coordinate)                                         out_pts = the input row bit for bit, shift 0
 *   1  no plane (the validity rule fails)                                        out_pts = the input row bit for bit, shift 0
 *   2  held: variation > (double)max_variation or |s| > (double)max_shift        out_pts = the input row bit for bit, shift (float)|s|
 *   3  moved: out_pts_k = (float)((double)A[i]_k - s n_k)                        shift (float)|s|
 * variation <= 1/3 by construction, so max_variation >= 1/3 is "no limit", as max_shift = +inf is.  counts long long [4] = the rows per
 * state; sum_shift2 double [1] = the sum of s^2 over the moved rows by the chunk rule of ls_cloud_nearest_f32 (chunks of 256 rows in a
 * fixed tree, the partials in chunk order, no floating-point atomics); status_out as in the search.  Every row is projected from the INPUT
 * positions (a Jacobi step), so out_pts must not overlap A: refused on the host, like a radius that is not finite and > 0, min_nbrs < 1,
 * and a max_variation or max_shift that is NaN or < 0.  One thread per row walks the 27 cells; 2 launches after the grid build.  No host
 * synchronisation, no allocation, integer atomics only and only on the table: every output is the same bits in any run.  The workspace
 * is the normals' plus 8 bytes per chunk of 256 rows. */
size_t ls_cloud_project_workspace_bytes(long long a);
int ls_cloud_project_f32(const float* A, long long a, float radius, int min_nbrs, float max_variation, float max_shift, float* out_pts,
                         int32_t* state, float* shift, long long* counts, double* sum_shift2, int* status_out, void* workspace,
                         size_t workspace_bytes, void* stream);
/* P >= 1 problems per call with the conventions of ls_cloud_normals_batch_f32: a_off and radius are HOST arrays, checked before the first
 * HIP call -- the error names the problem; min_nbrs, max_variation and max_shift are shared by the batch; empty problems are allowed.
 * out_pts [a_total,3], state / shift [a_total], counts [P,4], sum_shift2 [P], status_out [P] (nullable), all DEVICE.  Every output of every
 * problem is BIT-IDENTICAL to ls_cloud_project_f32 on that problem alone, and the number of launches does not depend on P. */
size_t ls_cloud_project_batch_workspace_bytes(int P, long long a_total);
int ls_cloud_project_batch_f32(int P, const float* A, long long a_total, const long long* a_off, const float* radius, int min_nbrs,
                               float max_variation, float max_shift, float* out_pts, int32_t* state, float* shift, long long* counts,
                               double* sum_shift2, int* status_out, void* workspace, size_t workspace_bytes, void* stream);

/* Scene memory, kept points carved out of observed free space (csrc/cloudcarve.hip, csrc/carve_plan.h): the one operator that REMOVES
 * points.  AN EXTENSION BEYOND THE RELEASED REFERENCE, like the merge.  A depth image says where there is nothing: every pixel is a ray
 * that reached its depth without hitting anything on the way.  A kept row that a posed depth view looks THROUGH lies in observed free
 * space and may be dropped; a row the view confirms, a row it cannot see and a row it cannot judge stay.  The output is a subsequence of
 * the input: rows and bits are untouched, nothing is averaged or moved; float64 comparisons and integer counts, no sums.
 * Inputs: the kept cloud A [a,3] fp32; `views` depth images depth [views,H,W] fp32, 0 = the ray hit nothing (the renderer's convention);
 * intrinsics [views,4] float64 = (fx, fy, cx, cy); world_to_cam E [views,3,4] float64 FROM THE FRAME OF A (composing a camera with a
 * registration is the caller's work); all DEVICE.  Definition per (row i, view v) (tests/carve_oracle.py is the same text as NumPy).
 * Everything is float64 and nothing is contracted; x is the fp32 row widened.
 *   1. c = ((E[:,0] x_0 + E[:,1] x_1) + E[:,2] x_2) + E[:,3].
 *   2. OUT if a component of c is not finite or c.z < znear.
 *   3. u = fx (c.x / c.z) + cx and v = fy (c.y / c.z) + cy.  qx = floor(u + 0.5), qy = floor(v + 0.5): the ray of pixel q goes through the
 *      integer coordinate, as in ls_depth_points_f32.  OUT unless 0 <= qx <= W - 1 and 0 <= qy <= H - 1; the comparison is made on the
 *      doubles, so NaN fails it.
 *   4. Over the window pixels (qx + dx, qy + dy), |dx|, |dy| <= k = window, that lie inside the image (n_in of them), let
 *      d = (double) depth[v, y, x], lo = d - tol and hi = d + tol.  Each pixel is exactly one of:
 *        empty   !(d > 0), so 0, negative and NaN count as empty
 *        front   c.z < lo
 *        behind  c.z > hi
 *        hit     otherwise, both ends inclusive
 *   5. The state of the (row, view), uint8:
 *        1 SEEN      if n_hit > 0
 *        2 FREE      else if n_front + (empty_is_free ? n_empty : 0) == n_in
 *        3 OCCLUDED  else if n_behind > 0 and n_front == 0
 *        4 MIXED     else
 *      and 0 is OUT.
 * Per row: seen_i and free_i are the numbers of views in those states.  ROW i IS DROPPED IFF free_i >= min_free AND seen_i <= max_seen.
 * A non-finite row is OUT everywhere and therefore stays.  The nearest-pixel rounding of step 3 moves the ray by up to half a pixel, so
 * the window defaults to 1 in the bindings (derived).  NO tol IS RECOMMENDED, and no min_free or max_seen: none has been measured on real
 * scans.
 * Outputs (DEVICE): out_pts [a,3] fp32, the kept rows in order, the same bits; out_src [a] int32, the row's index in its problem; out_off
 * [2] int64 = (0, kept rows); seen, free [a] int32; counts [4] int64 = rows with seen >= 1, rows with free >= 1, rows dropped, rows OUT
 * in every view (every row, when there is no view); view_counts [views,5] int64, the histogram of the five states by value; state, uint8
 * [views,a], NULL: not written; status_out [1] (nullable): LS_OK.  a = 0 and views = 0 are allowed; with no views nothing is dropped.
 * Refused on the host before the first HIP call, with a message that names the problem: tol not finite or < 0, znear not finite or <= 0,
 * window outside {0, 1, 2}, min_free < 1, max_seen < 0, empty_is_free outside {0, 1}, H or W < 1, a beyond the scan's reach (2^24 rows).
 * A workgroup owns one chunk of 256 rows of one problem, so the problem's views are the same for the whole workgroup; one thread per row
 * loops over the views and gathers at most (2k+1)^2 pixels per view; then flag, scan, scatter as in the merge.  The histograms are one
 * integer add per wave, view and state, from a ballot.  Launches, whatever P and the number of views: with rows, 2 memsets (counts,
 * view_counts; the latter only with views) and 6 kernels (carve, the scan's three, scatter, offsets); without rows, at most 4 memsets
 * and no kernel.  No host synchronisation, no allocation, no floating-point atomics: every output is the same bits in any run.  The
 * workspace depends on (a, views) alone -- in fact on a: two int32 per row and the scan's block sums; 0 for refused sizes. */
size_t ls_cloud_carve_workspace_bytes(long long a, long long views);
int ls_cloud_carve_f32(const float* A, long long a, const float* depth, long long views, int height, int width, const double* intrinsics,
                       const double* world_to_cam, double tol, double znear, int window, int min_free, int max_seen, int empty_is_free,
                       float* out_pts, int32_t* out_src, long long* out_off, int32_t* seen, int32_t* free_views, long long* counts,
                       long long* view_counts, uint8_t* state, int* status_out, void* workspace, size_t workspace_bytes, void* stream);
/* P >= 1 problems per call: problem p owns the rows [a_off[p], a_off[p+1]) of A and the views [view_off[p], view_off[p+1]) of the
 * views_total images; a_off and view_off are HOST int64 [P+1], checked before the first HIP call -- the error names the problem -- and
 * copied into the workspace.  One H x W and one set of scalars per call.  A problem with no rows or no views is allowed.  out_pts / out_src
 * hold the kept rows of every problem back to back, problem p's at [out_off[p], out_off[p+1]), out_off [P+1]; seen / free [a_total];
 * counts [P,4]; view_counts [views_total,5]; state: problem p's block is [V_p, a_p], the blocks back to back; status_out [P] (nullable).
 * Every output of every problem is BIT-IDENTICAL to ls_cloud_carve_f32 on that problem alone, and the number of launches does not depend
 * on P.  The workspace depends on (P, a_total, views_total) alone. */
size_t ls_cloud_carve_batch_workspace_bytes(int P, long long a_total, long long views_total);
int ls_cloud_carve_batch_f32(int P, const float* A, long long a_total, const long long* a_off, const float* depth, long long views_total,
                             const long long* view_off, int height, int width, const double* intrinsics, const double* world_to_cam, double tol,
                             double znear, int window, int min_free, int max_seen, int empty_is_free, float* out_pts, int32_t* out_src,
                             long long* out_off, int32_t* seen, int32_t* free_views, long long* counts, long long* view_counts, uint8_t* state,
                             int* status_out, void* workspace, size_t workspace_bytes, void* stream);

/* Scene memory, posed depth views fused into a truncated signed distance volume per instance (csrc/depthfuse.hip, csrc/fuse_plan.h).  AN
 * EXTENSION BEYOND THE RELEASED REFERENCE, like the merge and the carve.  The carve asks of a kept point whether a view looks through it;
 * the fusion asks it of every sample of a grid and keeps the answer as a distance: averaged over all views, the zero set of the volume is
 * the surface that was OBSERVED (ls_tsdf_volume_f64 reads the volume out), sensor noise averages out, and a free-space
 * observation pulls a stale surface away as the carve drops a stale point.
 * State per problem: two int32 volumes [nx,ny,nz], k fastest as marching cubes reads a volume: sum, the quantised distances, and n, the
 * observation count.  Both are updated IN PLACE; a fresh state is all zeros.  Grid per problem: origin[3] (the centre of voxel (0,0,0)),
 * voxel h > 0 and trunc > 0, float64, HOST; one (nx,ny,nz) per call.  Views: depth [views,H,W] fp32, 0 = the ray hit nothing (the
 * renderer's convention); intrinsics [views,4] float64 = (fx, fy, cx, cy); world_to_cam E [views,3,4] float64 FROM THE GRID'S FRAME
 * (composing a camera with a registration is the caller's work); all DEVICE.  Definition per voxel (i_0,i_1,i_2) and view v, the views in
 * the call's order (tests/fuse_oracle.py is the same text as NumPy).  Everything is float64 and nothing is contracted.
 *   1. x_a = origin_a + h * (double)i_a, one multiply and one add.  c = ((E[:,0] x_0 + E[:,1] x_1) + E[:,2] x_2) + E[:,3].
 *   2. OUT if a component of c is not finite or c.z < znear.
 *   3. u, v and the pixel q = floor(. + 0.5) exactly as step 3 of ls_cloud_carve_f32.  OUT unless q is inside the image.
 *   4. d = (double) depth[v, qy, qx].  EMPTY if !(d > 0), so 0, negative and NaN.  With empty_is_free an EMPTY voxel-view is taken with
 *      t = +1 (step 6: q = 16384) and counted as FREE; otherwise it is skipped.
 *   5. s = d - c.z, the PROJECTIVE distance along the optical axis.  OCCLUDED, and skipped, if s < -trunc.
 *   6. t = min(s, trunc) / trunc, so t is in [-1, 1]; q = (int) floor(t * 16384 + 0.5).  The class is NEAR if s <= trunc, else FREE.
 *   7. SATURATED, and skipped, if n == 65535.
 *   8. Otherwise sum += q and n += 1.  |sum| <= 65535 * 16384 < 2^30.
 * THE UPDATE IS INTEGER, so the state does not depend on the order of the views, on how they are split over calls, or on the batch; only
 * a saturated voxel depends on the order, and the order is the call's.
 * view_counts [views,6] int64 (DEVICE) is the histogram of OUT, EMPTY (skipped), OCCLUDED, NEAR, FREE and SATURATED, by value 0 .. 5, over
 * the voxels of the view's problem; every row sums to nx ny nz.
 * Refused on the host before the first HIP call: voxel, trunc or znear not finite or <= 0, a non-finite origin -- the error names the
 * problem --, dims < 1, H or W < 1, P nx ny nz >= 2^31, empty_is_free outside {0, 1}, a view_off that does not start at 0, decreases or
 * does not end at the number of views.
 * A workgroup owns 256 consecutive voxels of one problem; one thread per voxel keeps (sum, n) in registers, loops over its problem's
 * views, and reads and writes its state once; a view's E and K are wave-uniform; the histogram is one integer add per wave, view and class
 * from a ballot.  Launches, whatever P and the number of views: the copy of the host arrays into the workspace, 1 memset (view_counts)
 * and 1 kernel; a call without views does nothing.  No host synchronisation, no allocation, no floating-point atomics.  The workspace
 * holds the device copy of view_off and the grids: a function of its arguments alone (in fact of P), 0 for refused sizes.
 * NO voxel, trunc OR min_obs IS RECOMMENDED: none has been measured on real scans. */
size_t ls_depth_fuse_workspace_bytes(int nx, int ny, int nz, long long views);
int ls_depth_fuse_f32(int32_t* sum, int32_t* n, int nx, int ny, int nz, const double* origin, double voxel, double trunc, const float* depth,
                      long long views, int height, int width, const double* intrinsics, const double* world_to_cam, double znear, int empty_is_free,
                      long long* view_counts, void* workspace, size_t workspace_bytes, void* stream);
/* P >= 1 problems per call: sum, n [P,nx,ny,nz]; problem p owns the views [view_off[p], view_off[p+1]) of the views_total images.  origin
 * [P,3], voxel [P], trunc [P] (float64) and view_off [P+1] (int64) are HOST arrays, checked before the first HIP call and copied into the
 * workspace.  One H x W, one znear and one empty_is_free per call.  A problem without views changes nothing.  The state of every problem
 * is BIT-IDENTICAL to ls_depth_fuse_f32 on that problem alone (which is this entry with P = 1). */
size_t ls_depth_fuse_batch_workspace_bytes(int P, int nx, int ny, int nz, long long views_total);
int ls_depth_fuse_batch_f32(int P, int32_t* sum, int32_t* n, int nx, int ny, int nz, const double* origin, const double* voxel, const double* trunc,
                            const float* depth, long long views_total, const long long* view_off, int height, int width, const double* intrinsics,
                            const double* world_to_cam, double znear, int empty_is_free, long long* view_counts, void* workspace,
                            size_t workspace_bytes, void* stream);
/* State to volume, per sample of sum, n [B,nx,ny,nz]: valid = n >= min_obs (min_obs >= 1); D = (double)sum / ((double)n * 16384.0) where
 * valid, else EXACTLY +1.0.  volume_out float64 and valid_out uint8 [B,nx,ny,nz]; counts_out [B,3] int64 = valid samples, valid samples
 * with D <= 0, samples with n == 0 (all DEVICE).  1 memset and 1 kernel.  Filling what was never observed with +1 puts a second shell
 * where the truncation band ends: a mesher of this volume must drop every cube that has a corner with valid_out == 0.
 * ls_marching_cubes_f64 takes no mask; ls_tsdf_mesh_f64 below meshes the STATE and needs no volume. */
int ls_tsdf_volume_f64(const int32_t* sum, const int32_t* n, int B, int nx, int ny, int nz, int min_obs, double* volume_out, uint8_t* valid_out,
                       long long* counts_out, void* stream);

/* Scene memory, the mesh of a fused state where it was OBSERVED (csrc/tsdfmesh.hip, csrc/tsdfmesh_plan.h).  AN EXTENSION BEYOND THE
 * RELEASED REFERENCE, like the fusion.  Marching cubes of the state at isovalue 0 (not an argument), restricted to what was seen; no float64
 * volume is materialised and there is no compaction step.  Inputs per problem: sum, n int32 [nx,ny,nz] (DEVICE, read only), min_obs >= 1,
 * origin[3] and voxel > 0 (float64, HOST).  Definition (tests/fuse_oracle.py: mesh is the same text as NumPy, tests/tsdf_mesh_oracle.py the
 * local rule of step 3):
 *   1. sample   valid iff n >= min_obs; D = (double)sum / ((double)n * 16384.0) where valid (ls_tsdf_volume_f64's value; an invalid sample
 *               reads +1 in the pattern and in nothing else).
 *   2. cube     the (nx-1)(ny-1)(nz-1) cubes in C order, the pattern from D <= 0 on the eight corners in ls_marching_cubes_f64's corner
 *               order.  A cube is KEPT iff all eight corners are valid; a kept cube emits the triangles of its row of the triangle table,
 *               in table order; a dropped cube emits none.
 *   3. vertex   libmcubes creates the vertex of a crossed edge in the first cube that owns it: every cube owns its edges 6, 5, 10 and, on
 *               the low faces of the volume, the otherwise inherited ones.  A created vertex is CARRIED iff a kept cube names it: its own
 *               cube, or, for the edges 6, 5, 10, one of the up to three other cubes around that lattice edge.  Both ends of a carried
 *               edge are valid: NO POSITION EVER READS AN UNOBSERVED SAMPLE.  The owner of a carried vertex need not be a kept cube.
 *   4. order    the carried vertices in libmcubes' creation order (owner cubes in C order; inside a cube 6, 5, 10, 0, 1, 2, 3, 4, 7, 8, 9,
 *               11): the vertices ls_marching_cubes_f64 would number, with the ones no kept face names left out.
 *   5. position the libmcubes interpolation on D with the +0.5 offset, x = (f2 == f1) ? (x2 + x1) / 2 : (x2 - x1) * (0 - f1) / (f2 - f1) + x1,
 *               then (V - 0.5) * voxel + origin as three separate operations, nothing contracted: the result is exact, not approximate.
 *   6. faces    indices count from the mesh's own first vertex.
 * Calling convention of ls_marching_cubes_batch_f64: off_out (DEVICE long long [2][P+1]) = first vertex / first face of every mesh and the
 * totals, always the FULL counts; nothing is written at or past cap_v vertices / cap_f faces of the packed outputs; vertices = faces = NULL
 * is a sizing call.  stats_out (DEVICE long long [P][3], may be NULL) = kept cubes, dropped cubes whose pattern holds a crossing, valid
 * samples.  A problem without a kept cube yields an empty mesh and the ones after it are unaffected; a dim < 2 zeroes off_out.
 * Refused on the host before the first HIP call, the problem named where there is one: dims < 1, P outside 1 .. 65535,
 * 15 P nx ny nz >= 2^31 (int bases), min_obs < 1, voxel not finite or <= 0, a non-finite origin, a negative capacity, vertices without
 * faces or the reverse, a short workspace (LS_ERR_WORKSPACE).
 * Passes, one launch each whatever P: classify (4096 samples per workgroup, k on consecutive lanes, 8 gathers of (sum, n) -> pattern and kept
 * bit, 16 bit per cube; the statistics are three integer atomics per workgroup), count (the carried mask per cube from the kept bits of its neighbours; vertices << 32 | face indices summed per workgroup
 * of 4096 cubes), one scan over the workgroup sums of the batch, vertices (per-cube bases, positions), faces (final indices: own vertices
 * by rank, inherited ones from the owner's base plus the rank among the owner's CARRIED vertices).  Also the copy of the host grids into
 * the workspace and, with stats_out, 1 memset.  hipGetLastError() is read after EVERY launch and the error names the pass.  No host
 * synchronisation, no allocation, no floating-point atomics.  The workspace is a function of (P, nx, ny, nz) alone, 0 for refused sizes.
 * The single entry is the batch of one problem, BIT-IDENTICAL.  NO min_obs IS RECOMMENDED: 1 is the least, unmeasured on real scans. */
size_t ls_tsdf_mesh_workspace_bytes(int nx, int ny, int nz);
int ls_tsdf_mesh_f64(const int32_t* sum, const int32_t* n, int nx, int ny, int nz, int min_obs, const double* origin, double voxel, double* vertices,
                     long long cap_v, long long* faces, long long cap_f, long long* off_out, long long* stats_out, void* workspace,
                     size_t workspace_bytes, void* stream);
size_t ls_tsdf_mesh_batch_workspace_bytes(int P, int nx, int ny, int nz);
int ls_tsdf_mesh_batch_f64(int P, const int32_t* sum, const int32_t* n, int nx, int ny, int nz, int min_obs, const double* origin, const double* voxel,
                           double* vertices, long long cap_v, long long* faces, long long cap_f, long long* off_out, long long* stats_out,
                           void* workspace, size_t workspace_bytes, void* stream);

/* Scene memory, the fused state READ at a point (csrc/tsdficp.hip).  AN EXTENSION BEYOND THE RELEASED REFERENCE, like ls_depth_fuse_f32,
 * whose state (sum, n int32 [nx,ny,nz], DEVICE) and grid (origin [3], voxel h, trunc: float64, HOST, origin the centre of voxel (0,0,0))
 * these are.  min_obs >= 1; queries B [b,3] fp32 (DEVICE); pose g [3,4] fp32 (DEVICE), rescan -> memory, NULL: B bit for bit.
 * Definition, per query (csrc/tsdfsample_plan.h is this text as pure C++, tests/tsdf_sample_oracle.py as NumPy); everything after step 1
 * is float64 and nothing is contracted:
 *   1 posed query   y_a = ((R_a0 x_0 + R_a1 x_1) + R_a2 x_2) + t_a in fp32, every product and sum rounded: the expression of
 *                   ls_cloud_merge_f32; yd = (double) y.
 *   2 grid coord.   u_a = (yd_a - origin_a) / h.  State OUT (0) if a component of y is not finite, if a dimension is below 2 (no cell), or
 *                   unless 0 <= u_a <= n_a - 1 on every axis.  Else the base index i_a = min((int) floor(u_a), n_a - 2) -- the far face
 *                   belongs to the last cell -- and f_a = u_a - (double) i_a.
 *   3 corners       the eight samples (i_0 + alpha, i_1 + beta, i_2 + gamma), each valid iff n >= min_obs, D = sum / (n * 16384) as in
 *                   ls_tsdf_volume_f64.  State UNSEEN (1) if any corner is invalid -- no value ever reads an unobserved sample -- else
 *                   SAMPLED (2).
 *   4 value         with lerp(a, b, f) = a + f * (b - a): along axis 2, a[alpha beta] = lerp(D[alpha beta 0], D[alpha beta 1], f_2); along
 *                   axis 1, b[alpha] = lerp(a[alpha 0], a[alpha 1], f_1); along axis 0, v = lerp(b[0], b[1], f_0).  phi = trunc * v, metres.
 *   5 gradient      the exact derivative of that interpolant, which is affine in every f_a:
 *                   G_2 = lerp_0(lerp_1(D[alpha beta 1] - D[alpha beta 0])): first over beta with f_1, then over alpha with f_0;
 *                   G_1 = lerp_0(lerp_2(D[alpha 1 gamma] - D[alpha 0 gamma])): first over gamma with f_2, then over alpha with f_0;
 *                   G_0 = lerp_1(lerp_2(D[1 beta gamma] - D[0 beta gamma])): first over gamma with f_2, then over beta with f_1;
 *                   grad_a = (trunc / h) * G_a, trunc / h formed once per problem on the host.  The gradient is NOT normalised.
 *   6 outputs       OUT and UNSEEN queries write phi = +trunc and grad = 0.
 * Outputs (DEVICE): phi double [b], grad double [b,3], state uint8 [b], counts long long [3] = finite queries, queries inside the grid
 * (not OUT), SAMPLED queries; sum_phi2 double [1] = the sum of phi^2 over the SAMPLED queries by the chunk rule of ls_cloud_icp_f32: a
 * workgroup owns 256 consecutive queries of ONE problem, a fixed tree inside each wave of 64 (lane l with l + 32, l + 16, ..., l + 1), a
 * fixed tree over the four waves ((w0 + w1) + (w2 + w3)), one record per chunk, the records added in chunk order.  No atomics.
 * Refused on the host before the first HIP call, the error naming the problem: dims < 1, P nx ny nz >= 2^31, min_obs < 1, b < 0 or
 * > 2^31 - 1, null pointers, an origin that is not finite, voxel or trunc not finite and > 0, trunc / voxel not finite, bad offsets.
 * Launches: the copy of the host arrays into the workspace and 2 kernels, whatever P; no host synchronisation, no allocation;
 * hipGetLastError() is read after every launch and the error names the pass.  The workspace is a function of (P, b) alone, 0 for refused
 * sizes.  Queries arrive in no spatial order, so the corner gathers are scattered; they are not sorted here.  NO min_obs IS RECOMMENDED. */
#define LS_SAMPLE_OUT 0
#define LS_SAMPLE_UNSEEN 1
#define LS_SAMPLE_SAMPLED 2
size_t ls_tsdf_sample_workspace_bytes(int nx, int ny, int nz, long long b);
int ls_tsdf_sample_f32(const int32_t* sum, const int32_t* n, int nx, int ny, int nz, int min_obs, const double* origin, double voxel, double trunc,
                       const float* B, long long b, const float* g, double* phi, double* grad, uint8_t* state, long long* counts, double* sum_phi2,
                       void* workspace, size_t workspace_bytes, void* stream);
/* P >= 1 problems per call: one (nx, ny, nz) per call, sum / n [P,nx,ny,nz], origin [P,3], voxel [P], trunc [P] (HOST), B [b_total,3] with
 * b_off HOST int64 [P+1] (empty problems allowed), g [P,3,4] or NULL, counts [P,3], sum_phi2 [P].  Every output of every problem is
 * BIT-IDENTICAL to ls_tsdf_sample_f32 on that problem alone: the single entry is the batch of one problem. */
size_t ls_tsdf_sample_batch_workspace_bytes(int P, int nx, int ny, int nz, long long b_total);
int ls_tsdf_sample_batch_f32(int P, const int32_t* sum, const int32_t* n, int nx, int ny, int nz, int min_obs, const double* origin,
                             const double* voxel, const double* trunc, const float* B, long long b_total, const long long* b_off, const float* g,
                             double* phi, double* grad, uint8_t* state, long long* counts, double* sum_phi2, void* workspace, size_t workspace_bytes,
                             void* stream);

/* Scene memory, a rescan REGISTERED onto the fused state without any search (csrc/tsdficp.hip; Bylow, Sturm, Kerl, Kahl, Cremers, RSS
 * 2013).  AN EXTENSION BEYOND THE RELEASED REFERENCE.  The arguments are those of ls_tsdf_sample_f32 with g0 (NULL: the identity as a
 * matrix) in the place of g, plus max_iter, rel_thr, min_matched (>= 3) as in ls_cloud_icp_plane_f32.  Per problem, g_0 as in
 * ls_cloud_icp_f32, for k = 0, 1, ...:
 *   sample      exactly ls_tsdf_sample_f32 under g_k -> f_k (finite), w_k (SAMPLED), Q_k = sum phi^2 by the chunk rule.
 *   cost        E_k = (Q_k + (f_k - w_k) trunc^2) / f_k, 0 for f_k = 0: the truncated quadratic of ls_cloud_icp_f32 with trunc in the place
 *               of r.  A query in saturated free space has phi = trunc and grad = 0: it costs what an unsampled one costs and pulls on
 *               nothing.
 *   stop tests  those of ls_cloud_icp_plane_f32 in its order, each keeping g_k, min_matched applied to w_k: w_k < min_matched:
 *               LS_ICP_STARVED; k >= 1 and E_{k-1} - E_k <= rel_thr E_{k-1}: LS_ICP_CONVERGED; k == max_iter: LS_ICP_MAX_ITER.
 *   update      minimise sum (phi + omega . (y x grad) + v . grad)^2 over the SAMPLED queries: J = (grad, yd x grad) in the twist order
 *               (v, omega); the 28 float64 moments (phi^2, J phi [6], J J^T [21, the upper triangle by rows]) per chunk, added by the chunk
 *               rule, in the record layout of ls_cloud_icp_plane_f32.  THE GRADIENT IS NOT NORMALISED, NOTHING IS WEIGHTED, AND THERE IS NO
 *               LINE SEARCH AND NO DAMPING: a step that raises E ends the loop as LS_ICP_CONVERGED at the next test, with the pose that
 *               step produced.
 *   solve and retraction  exactly those of ls_cloud_icp_plane_f32 (one text, csrc/se3_gn.h): Cholesky in float64 in a fixed order, a pivot
 *               that is not > 1e-12 times the original diagonal entry or any non-finite value: LS_ICP_DEGENERATE, g_k is kept (the state
 *               of one plane, all gradients parallel, is the exact case); exp of the twist; R' onto SO(3); rounded to fp32.
 * Outputs: g_out [3,4] fp32, stop int32 (LS_ICP_*), iters int32, and the complete result of the final sample -- phi, grad, state, counts,
 * sum_phi2 -- bit for bit ls_tsdf_sample_f32 at g_out: a stopped problem is frozen (its sample workgroups return at once), so these are
 * its last live sample's.  Optional traces: g_trace float [max_iter+1, 12], stat_trace double [max_iter+1, 3] = (f_k, w_k, Q_k); rows
 * past the stop are left alone.  Launches: the copy and 2 max_iter + 4 kernels, whatever P and whenever problems stop; no host
 * synchronisation, no allocation, no atomics.  The start error must lie within trunc.  NO SETTING IS RECOMMENDED. */
size_t ls_tsdf_icp_workspace_bytes(int nx, int ny, int nz, long long b);
int ls_tsdf_icp_f32(const int32_t* sum, const int32_t* n, int nx, int ny, int nz, int min_obs, const double* origin, double voxel, double trunc,
                    const float* B, long long b, const float* g0, int max_iter, double rel_thr, int min_matched, float* g_out, int32_t* stop,
                    int32_t* iters, double* phi, double* grad, uint8_t* state, long long* counts, double* sum_phi2, float* g_trace,
                    double* stat_trace, void* workspace, size_t workspace_bytes, void* stream);
/* P >= 1 problems per call with the conventions of ls_tsdf_sample_batch_f32; g0 [P,3,4] or NULL, g_out [P,3,4], stop / iters [P], g_trace
 * [P, max_iter+1, 12], stat_trace [P, max_iter+1, 3].  Every output of every problem is BIT-IDENTICAL to ls_tsdf_icp_f32 on it alone. */
size_t ls_tsdf_icp_batch_workspace_bytes(int P, int nx, int ny, int nz, long long b_total);
int ls_tsdf_icp_batch_f32(int P, const int32_t* sum, const int32_t* n, int nx, int ny, int nz, int min_obs, const double* origin, const double* voxel,
                          const double* trunc, const float* B, long long b_total, const long long* b_off, const float* g0, int max_iter,
                          double rel_thr, int min_matched, float* g_out, int32_t* stop, int32_t* iters, double* phi, double* grad, uint8_t* state,
                          long long* counts, double* sum_phi2, float* g_trace, double* stat_trace, void* workspace, size_t workspace_bytes,
                          void* stream);

/* Scene memory, the fused state as a TRAINING SIGNAL for the latent codes (csrc/tsdffit.hip; off-surface samples and the clamp of free
 * space: Park et al., DeepSDF, CVPR 2019).  AN EXTENSION BEYOND THE RELEASED REFERENCE, whose code optimisation is supervised by
 * MSE(sdf(points), 0) alone.  Definition (csrc/tsdffit_plan.h is the same text as C++, tests/tsdf_fit_oracle.py as NumPy).
 *
 * THE DRAW, per problem: state sum / n int32 [nx,ny,nz], k fastest (DEVICE), origin [3], voxel, trunc (HOST doubles), a seed (uint64).
 *   eligibility  a lattice sample is eligible iff n >= min_obs (min_obs >= 1).
 *   kinds        FREE (2) iff sum == n * 16384: every view that looked saw the sample at or beyond +trunc (the projective distance is
 *                clamped on that side only).  Every other eligible sample is BAND (1): ls_depth_fuse_f32 never records less than -1 (an
 *                occluded sample is skipped), so D = -1 is an exact value, not a clamp.  Integer comparisons only.
 *   lists        the eligible samples of a kind in linear index order form a list of length L.
 *   quotas       a quota m (n_band or n_free, each >= 0, N = n_band + n_free >= 1) takes T = min(L, m) of them, one per stratum: stratum
 *                j is the list ranks [floor(j L / T), floor((j + 1) L / T)), of width w_j >= 1; the rank taken is
 *                floor(j L / T) + ((r_j * w_j) >> 32) in 64-bit unsigned arithmetic, r_j = the top 32 bits of
 *                mix64(key + (j + 1) * 0x9E3779B97F4A7C15), key = mix64(seed + kind * 0x9E3779B97F4A7C15), mix64 the finaliser of
 *                splitmix64.  The ranks are distinct and ascending, and with L <= m every sample is taken.
 *   outputs      (DEVICE) columns [0, n_band) for the band and [n_band, N) for free space: points float [N,3] = the float64
 *                origin_a + voxel * index_a of each axis rounded once to fp32; target double [N] = trunc * sum / (n * 16384), metres;
 *                kind uint8 [N]; index int32 [N] = the linear sample index; counts long long [3] = eligible, band, free samples.  A
 *                column beyond T is a PAD (0): the position of lattice sample 0, target 0, index -1.
 * A problem's draw depends on its own state, grid and seed only.  Refused on the host before the first HIP call: dims < 1,
 * P nx ny nz >= 2^31, nx ny nz above 4096 blocks of 4096 samples (the scan of a problem's block counts is one workgroup; the error names
 * the bound), min_obs < 1, a negative quota, N = 0, P N >= 2^31, P > 65535, null pointers, a grid that ls_depth_fuse_f32 refuses.
 * Launches: the copy of the host arrays into the workspace and 3 kernels (classify, scan, resolve), whatever P; no host
 * synchronisation, no allocation, no atomics.  The ranks are resolved by a search over the scanned block counts and two mask words per
 * 64 samples: no compact list is written.  The workspace is a function of (P, nx, ny, nz), 0 for refused sizes.
 * NO QUOTA AND NO min_obs IS RECOMMENDED: nothing here can measure one. */
#define LS_FIT_PAD 0
#define LS_FIT_BAND 1
#define LS_FIT_FREE 2
size_t ls_tsdf_draw_workspace_bytes(int nx, int ny, int nz);
int ls_tsdf_draw_f32(const int32_t* sum, const int32_t* n, int nx, int ny, int nz, int min_obs, const double* origin, double voxel, double trunc,
                     long long n_band, long long n_free, unsigned long long seed, float* points, double* target, uint8_t* kind, int32_t* index, long long* counts,
                     void* workspace, size_t workspace_bytes, void* stream);
/* P >= 1 problems per call: one (nx, ny, nz) and one pair of quotas per call, sum / n [P,nx,ny,nz], origin [P,3], voxel [P], trunc [P],
 * seeds [P] (HOST), points [P,N,3], target / kind / index [P,N], counts [P,3].  Every output of every problem is BIT-IDENTICAL to
 * ls_tsdf_draw_f32 on that problem alone, wherever it stands in the batch: the single entry is the batch of one problem. */
size_t ls_tsdf_draw_batch_workspace_bytes(int P, int nx, int ny, int nz);
int ls_tsdf_draw_batch_f32(int P, const int32_t* sum, const int32_t* n, int nx, int ny, int nz, int min_obs, const double* origin, const double* voxel,
                           const double* trunc, long long n_band, long long n_free, const unsigned long long* seeds, float* points, double* target, uint8_t* kind,
                           int32_t* index, long long* counts, void* workspace, size_t workspace_bytes, void* stream);
/* THE LOSS, in the decoder's own units.  THIS BUILD'S DEFINITION, pinned by no test of the reference: the decoder's value times the
 * instance's scale s is a metric distance.  It follows the reference's training loss, which compares the decoder's output with distances
 * in the normalised frame; the reference's point loss MSE(sdf, 0) is the special case target = 0.  Inputs (DEVICE): sdf float [P,N],
 * s float [P], trunc double [P], target double [P,N], kind uint8 [P,N] (LS_FIT_*).  With u = (double) sdf:
 *   BAND e = u - target / (double) s;   FREE e = min(u - trunc / (double) s, 0.0), a one-sided hinge;   PAD e = 0.
 * m_p = the number of non-PAD columns.  loss[p] (double) = (sum of e^2 by the chunk rule of ls_tsdf_sample_f32: chunks of 256 columns,
 * a fixed tree in each wave of 64, a fixed tree over the four waves, the records added in chunk order from 0.0) / m_p, 0.0 where
 * m_p = 0; grad[p,i] = (float)(2 e / m_p), 0 where m_p = 0.  Optional min_loss double [P] and improved int32 [P]: where
 * loss < min_loss, min_loss = loss and improved = 1, the bookkeeping of ls_mse_f32.  NO WEIGHT BETWEEN THE KINDS (the quotas set the
 * balance), NO CLAMP OF THE BAND ERROR, AND s IS NOT OPTIMISED (the reference's loop does not move it either).  One launch for any P,
 * one workgroup per chunk; the workgroup of a problem's chunk 0 adds that problem's records in order.  No atomics. */
int ls_tsdf_fit_loss_f64(const float* sdf, const float* s, const double* trunc, const double* target, const uint8_t* kind, int P, int N, double* loss,
                         float* grad, double* min_loss, int32_t* improved, void* stream);

/* Scene memory, the fused state SEEN FROM A CAMERA (csrc/tsdfray.hip; the raycast of Newcombe et al., KinectFusion, ISMAR 2011).  AN
 * EXTENSION BEYOND THE RELEASED REFERENCE, like the fusion.  Definition (csrc/tsdfray_plan.h is the same text as C++,
 * tests/tsdf_ray_oracle.py as NumPy).
 *
 * Per problem: state sum / n int32 [nx,ny,nz], k fastest (DEVICE), origin [3], voxel h, trunc (HOST doubles, the grid
 * ls_depth_fuse_f32 accepts, trunc / h finite), min_obs >= 1.  Per view (DEVICE doubles): cam_to_world M [3,4], camera to the grid's
 * frame with camera x right, y down, z forward -- the convention of ls_depth_points_f32, so a raycast depth map goes straight back into
 * ls_depth_points_f32, ls_cloud_carve_f32 and ls_depth_fuse_f32 -- and intrinsics (fx, fy, cx, cy).  Per call: height, width, znear > 0,
 * step in voxels with 1/16 <= step <= 1.  Per pixel (px, py), the ray through the integer pixel coordinate, float64 throughout, no
 * a * b + c contracted:
 *   1 ray      rx = (px - cx) / fx, ry = (py - cy) / fy; a_a = (M[a,3] - origin_a) / h; b_a = ((M[a,0] rx + M[a,1] ry) + M[a,2]) / h.
 *              The grid coordinate at camera depth z is u_a(z) = a_a + z b_a: the ray parameter IS the depth.
 *   2 slab     against [0, n_a - 1] on every axis: an axis with b_a == 0 imposes no bound if 0 <= a_a <= n_a - 1 and else makes the
 *              pixel OUTSIDE; any other axis gives the quotients (0 - a_a) / b_a and (n_a - 1 - a_a) / b_a, their minimum and maximum;
 *              z_in = max(znear, the largest minimum), z_out = the smallest maximum.  OUTSIDE: a value that is not finite, a dimension
 *              below 2, max |b_a| = 0, or !(z_in <= z_out).
 *   3 march    dz = step / max |b_a| (no axis advances more than `step` voxels per sample); K = floor((z_out - z_in) / dz), capped at
 *              ceil((max n_a - 1) / step) + 1 (reached only by a camera so far away that its quotients round coarser than the grid);
 *              the samples are z_k = z_in + (double) k dz, k = 0 .. K, never accumulated: an integer trip count known before the loop.
 *   4 sample   u_a clamped to [0, n_a - 1], i_a = min((int) floor(u_a), n_a - 2), f_a = u_a - i_a, then the value of
 *              ls_tsdf_sample_f32 on the eight corners: SAMPLED with (phi, grad phi), or UNSEEN (a corner with n < min_obs).
 *   5 state    walk k upward and stop at the first SAMPLED sample with phi_k <= 0: HIT if sample k - 1 exists, was SAMPLED and had
 *              phi_{k-1} > 0, with z* = z_{k-1} + dz (phi_{k-1} / (phi_{k-1} - phi_k)); BEHIND otherwise (the first thing known along
 *              the ray is the inside of something, or the crossing lay in unobserved space).  Never stopped: FREE if every sample was
 *              SAMPLED (the memory looked all along this ray and found nothing), else UNSEEN.
 *   6 outputs  a HIT: depth = (float) z*; one more sample at z*: where it is SAMPLED with g.g > 0 the normal is
 *              (float)(grad_a / sqrt((g0 g0 + g1 g1) + g2 g2)), in the grid's frame, pointing out of the surface, else (0, 0, 0).
 *              Every other pixel: depth 0 (the renderer's "nothing") and normal 0.
 * NO secant iteration and NO empty-space skipping.  Outputs (DEVICE): depth float [views,H,W], normal float [views,H,W,3], state uint8
 * [views,H,W] (LS_RAY_*), counts long long [views,5], the histogram of the states.  Depth, state and counts are the same bits as the
 * NumPy twin; so is the normal on an MI355X with this toolchain (one device float64 sqrt, one division, one rounding to fp32: the
 * rounding of the device's sqrt is pinned nowhere in this project, so this is what the tests observe and hold, not a promise of hipcc).
 * Refused on the host before the first HIP call: dims < 1, P nx ny nz >= 2^31, min_obs < 1, views < 0, an empty image,
 * views * H * W >= 2^31, znear not finite or <= 0, step outside [1/16, 1], more than 2^20 samples per ray, a grid that
 * ls_tsdf_sample_f32 refuses, null pointers, bad offsets.  Launches: the copy of the host arrays into the workspace, one memset (counts)
 * and one kernel, whatever P and the number of views; no floating-point atomics, one integer add per wave, view and state.  The workspace
 * is a function of P alone, 0 for refused sizes.  step = 0.5 in the bindings is UNMEASURED; what is derived: step <= 1 keeps consecutive
 * samples in the same or an adjacent cell, and the band is 2 trunc / h >= 2 voxels thick. */
#define LS_RAY_OUTSIDE 0
#define LS_RAY_FREE 1
#define LS_RAY_UNSEEN 2
#define LS_RAY_BEHIND 3
#define LS_RAY_HIT 4
size_t ls_tsdf_raycast_workspace_bytes(int nx, int ny, int nz, long long views, int height, int width);
int ls_tsdf_raycast_f64(const int32_t* sum, const int32_t* n, int nx, int ny, int nz, int min_obs, const double* origin, double voxel, double trunc,
                        const double* cam_to_world, const double* intrinsics, long long views, int height, int width, double znear, double step,
                        float* depth, float* normal, uint8_t* state, long long* counts, void* workspace, size_t workspace_bytes, void* stream);
/* P >= 1 problems per call: one (nx, ny, nz), one H x W, one znear and one step per call, sum / n [P,nx,ny,nz], origin [P,3], voxel [P],
 * trunc [P], ragged views by HOST view_off [P+1] (a problem without views is allowed).  Every output of every view is BIT-IDENTICAL to
 * ls_tsdf_raycast_f64 on its problem alone, wherever it stands in the batch: the single entry is the batch of one problem. */
size_t ls_tsdf_raycast_batch_workspace_bytes(int P, int nx, int ny, int nz, long long views_total, int height, int width);
int ls_tsdf_raycast_batch_f64(int P, const int32_t* sum, const int32_t* n, int nx, int ny, int nz, int min_obs, const double* origin,
                              const double* voxel, const double* trunc, const double* cam_to_world, const double* intrinsics, long long views_total,
                              const long long* view_off, int height, int width, double znear, double step, float* depth, float* normal, uint8_t* state,
                              long long* counts, void* workspace, size_t workspace_bytes, void* stream);
/* THE VIEW COMPARISON, per pixel: observed depth d_obs (fp32), the predicted (depth, state) of a raycast, tol > 0 (HOST double):
 *   NO_OBS when !(d_obs > 0) (0, negative, NaN); UNKNOWN when the prediction is not a HIT; otherwise s = (double) d_obs - (double) d_pred:
 *   AGREE when |s| <= tol, IN_FRONT when s < -tol (something new stands before the memory's surface), THROUGH when s > tol (the view sees
 *   past a surface the memory holds).  Comparisons and integer counts only.
 * observed / depth float [views,H,W], state uint8 [views,H,W] -> cls uint8 [views,H,W] (LS_VIEW_*), counts long long [views,5].  One
 * memset and one kernel; it needs no workspace, so it has no size query.  NO tol IS RECOMMENDED: nothing here can measure one. */
#define LS_VIEW_NO_OBS 0
#define LS_VIEW_UNKNOWN 1
#define LS_VIEW_AGREE 2
#define LS_VIEW_IN_FRONT 3
#define LS_VIEW_THROUGH 4
int ls_depth_compare_f32(const float* observed, const float* depth, const uint8_t* state, long long views, int height, int width, double tol,
                         uint8_t* cls, long long* counts, void* stream);

/* Scene memory, a normal per pixel of a depth view (csrc/depthplane.hip, csrc/plane_plan.h).  AN EXTENSION BEYOND THE RELEASED
 * REFERENCE, like the fusion; what the weighted fuse below reads its planes from.  Inputs: depth [views,H,W] fp32 (DEVICE), intrinsics
 * [views,4] float64 = (fx, fy, cx, cy) (DEVICE), max_jump [views] float64 > 0 (HOST, copied into the workspace as the fuse copies its
 * grids).  Definition per view and pixel (x, y) (tests/plane_oracle.py is the same text as NumPy).  Everything is float64 and nothing is
 * contracted.
 *   1. d = (double) depth[v, y, x].  NO_DEPTH unless d is finite and > 0 (so 0, negative, NaN and inf).
 *   2. P(x, y) = (d * ((double)x - cx) / fx, d * ((double)y - cy) / fy, d): the product first, then the quotient.
 *   3. A neighbour is usable iff it is inside the image, is a depth pixel by step 1 and |d_nb - d| <= max_jump.
 *   4. a = P(x+1, y) - P(x-1, y) if both neighbours are usable, else P(x+1, y) - P(x, y), else P(x, y) - P(x-1, y), else none; b likewise
 *      along y.  NO_NEIGHBOUR if a or b is missing.
 *   5. m = a x b, every product rounded on its own; mm = (m_x m_x + m_y m_y) + m_z m_z.  DEGENERATE if mm is 0 or not finite.
 *   6. n = m / sqrt(mm); t = (n_x P_x + n_y P_y) + n_z P_z.  DEGENERATE if t == 0; n = -n if t > 0, so the normal faces the camera.
 *   7. VALID: normals_out = the three float64 components rounded once to fp32.
 * normals_out [views,H,W,3] fp32 is (0, 0, 0) unless VALID; state_out [views,H,W] uint8 = NO_DEPTH 0, VALID 1, NO_NEIGHBOUR 2,
 * DEGENERATE 3, by value; counts_out [views,4] int64 is their histogram (all DEVICE).
 * Refused on the host before the first HIP call: H or W < 1, views < 0, views H W >= 2^31, a max_jump that is not finite or <= 0 -- the
 * error names the view --, null pointers with views > 0.
 * One thread per pixel; a workgroup stays inside one view, so its intrinsics and max_jump are wave-uniform; the histogram is one integer
 * add per wave, view and state from a ballot.  Launches, whatever the number of views: the copy of max_jump into the workspace, 1 memset
 * (counts_out) and 1 kernel.  No host synchronisation, no allocation, no floating-point atomics.  The workspace holds the device copy of
 * max_jump: a function of its arguments alone, 0 for refused sizes.  NO max_jump IS RECOMMENDED: none has been measured on real scans. */
size_t ls_depth_normals_workspace_bytes(long long views, int height, int width);
int ls_depth_normals_f32(const float* depth, long long views, int height, int width, const double* intrinsics, const double* max_jump,
                         float* normals_out, uint8_t* state_out, long long* counts_out, void* workspace, size_t workspace_bytes, void* stream);

/* Scene memory, the depth fusion with integer weights and a point-to-plane value inside the band (csrc/depthplane.hip,
 * csrc/plane_plan.h).  AN EXTENSION BEYOND THE RELEASED REFERENCE, opt-in beside ls_depth_fuse_f32, whose state, grids, views and
 * refusals it shares.  Why: on the analytic sphere most of the fused field's error comes from the t = +1 votes of pixels that hit
 * nothing, cast with the weight of a surface observation onto voxels that hug the silhouette; the 1 / cos overstatement of the projective
 * distance comes second.  The arguments are those of ls_depth_fuse_f32 plus normals [views,H,W,3] fp32 (DEVICE, nullable:
 * ls_depth_normals_f32 of the same views, in the CAMERA frame) and weights[4] = (w_plane, w_proj, w_free, w_empty), HOST ints, each in
 * 1 .. 255.  Definition per voxel and view, the views in the call's order (tests/plane_oracle.py).  Everything is float64 and nothing
 * is contracted.
 *   1 - 5. literally steps 1 - 5 of ls_depth_fuse_f32: x, c, OUT, the pixel (qx, qy), d, EMPTY, s = d - c.z, OCCLUDED if s < -trunc on
 *      the PROJECTIVE s.  With empty_is_free an EMPTY voxel-view is taken with q = 16384 and w = w_empty and counted as FREE.
 *   6. FREE if s > trunc: q = 16384, w = w_free.  The band is decided projectively: a plane distance is wrong far from its pixel.
 *   7. NEAR, |s| <= trunc.  NEAR_PLANE if normals is given and the pixel's normal n is usable (three finite components, not all zero):
 *      p = P(qx, qy) as in step 2 of ls_depth_normals_f32; s_n = ((n_x (c_x - p_x) + n_y (c_y - p_y)) + n_z (c_z - p_z));
 *      value = clamp(s_n, -trunc, trunc) (a NaN reads -trunc); w = w_plane.  Otherwise NEAR_PROJ: value = s, w = w_proj.
 *      In both cases q = (int) floor(value / trunc * 16384 + 0.5).
 *   8. SATURATED, and skipped, if n + w > 65535.
 *   9. Otherwise sum += w * q and n += w.  |sum| <= n * 16384, n <= 65535, and sum == n * 16384 iff every vote was free: every reader of
 *      a fused state runs on a weighted one as it is, and min_obs becomes a weight threshold.
 * THE UPDATE IS INTEGER, so the state does not depend on the order of the views, on how they are split over calls, or on the batch; only
 * a saturated voxel depends on the order, and the order is the call's.  With normals NULL and weights (any, 1, 1, 1) the state is BIT FOR
 * BIT that of ls_depth_fuse_f32.
 * view_counts [views,7] int64 (DEVICE) is the histogram of OUT, EMPTY (skipped), OCCLUDED, NEAR_PLANE, NEAR_PROJ, FREE and SATURATED, by
 * value 0 .. 6, over the voxels of the view's problem; every row sums to nx ny nz.
 * Refused on the host before the first HIP call: whatever ls_depth_fuse_f32 refuses, null weights, a weight outside 1 .. 255.
 * The kernel has the shape of the fuse's: a workgroup owns 256 consecutive voxels of one problem, one thread per voxel keeps (sum, n) in
 * registers over its problem's views; E, K, the weights and the image bases are wave-uniform; one depth gather per voxel-view and three
 * normal gathers per NEAR one.  Launches, whatever P and the number of views: the copy of the host arrays into the workspace, 1 memset
 * (view_counts) and 1 kernel; a call without views does nothing.  No host synchronisation, no allocation, no floating-point atomics.
 * NO WEIGHTS ARE RECOMMENDED: 64 : 1 comes from one synthetic sphere, nothing has been measured on real scans. */
size_t ls_depth_fuse_weighted_workspace_bytes(int nx, int ny, int nz, long long views);
int ls_depth_fuse_weighted_f32(int32_t* sum, int32_t* n, int nx, int ny, int nz, const double* origin, double voxel, double trunc, const float* depth,
                               const float* normals, long long views, int height, int width, const double* intrinsics, const double* world_to_cam,
                               double znear, int empty_is_free, const int* weights, long long* view_counts, void* workspace, size_t workspace_bytes,
                               void* stream);
/* P >= 1 problems per call, as ls_depth_fuse_batch_f32: sum, n [P,nx,ny,nz]; problem p owns the views [view_off[p], view_off[p+1]) of the
 * views_total images and of normals [views_total,H,W,3]; one set of weights per call.  The state of every problem is BIT-IDENTICAL to
 * ls_depth_fuse_weighted_f32 on that problem alone (which is this entry with P = 1). */
size_t ls_depth_fuse_weighted_batch_workspace_bytes(int P, int nx, int ny, int nz, long long views_total);
int ls_depth_fuse_weighted_batch_f32(int P, int32_t* sum, int32_t* n, int nx, int ny, int nz, const double* origin, const double* voxel,
                                     const double* trunc, const float* depth, const float* normals, long long views_total, const long long* view_off,
                                     int height, int width, const double* intrinsics, const double* world_to_cam, double znear, int empty_is_free,
                                     const int* weights, long long* view_counts, void* workspace, size_t workspace_bytes, void* stream);

/* Scene memory, the fused state COMPLETED by the shape prior's field (csrc/tsdfprior.hip).  AN EXTENSION BEYOND THE RELEASED REFERENCE,
 * like the fusion: the decoder's value at the lattice samples the cameras left short of observations enters a SECOND state of the same
 * format as integer votes, so ls_tsdf_mesh_f64, ls_tsdf_raycast_f64 and ls_tsdf_sample_f32 read the completed state unchanged.  The
 * observed state is never written.  Definition (csrc/tsdfprior_plan.h is the same text as C++, tests/tsdf_prior_oracle.py as NumPy), for
 * problem p with grid (origin, voxel h, trunc), scale s_p > 0, an integer prior weight w0 in 1 .. 65535, and a lattice sample with state
 * (sum, n) and linear index i (k fastest):
 *   1 weight   w = max(w0 - n, 0): the prior tops a sample up to w0 votes and fades out as observations arrive.  w > 0: ELIGIBLE.
 *   2 row      the query row of an eligible sample: each axis the float64 origin_a + h * index_a of ls_depth_fuse_f32 rounded once to
 *              fp32.  Rows in ascending i within a problem, problems in order: ONE packed list, row_off [P+1] its offsets; every row
 *              carries row_inst = p and row_index = i (int32).  The rows of an instance are contiguous: the layout the ragged decoder
 *              entry takes.
 *   3 vote     with f the fp32 value the decoder returned for the row: d = (double) s_p * (double) f; t = d / trunc clamped to
 *              [-1, 1]; q = (int) floor(t * 16384 + 0.5); sum' = sum + w q, n' = n + w.  THE CONVENTION OF ls_tsdf_fit_loss_f64: the
 *              decoder's value times s is a metric distance with the sign of the fused distance.  A NaN f casts no vote: the sample
 *              keeps (sum, n) and is counted; +-inf clamps to +-1.  A sample that is not eligible keeps (sum, n) bit for bit.
 *   4 state    n' = max(n, w0) <= 65535 and |sum'| <= n' * 16384: the invariants of ls_depth_fuse_f32's state survive.
 * Integer and float64 arithmetic only, nothing contracted: given the same f, the rows, their order, the counts and (sum', n') do not
 * depend on the batch, on its order or on the run.  counts long long [P,4] = eligible, voted, skipped (NaN), untouched samples; the rows
 * entry leaves voted and skipped 0.
 * ls_tsdf_prior_rows_f32: n int32 [nx,ny,nz] (DEVICE, read only; the rows do not read sum), origin [3] and voxel (HOST doubles); outputs
 * (DEVICE) points float [R,3], row_inst / row_index int32 [R], row_off long long [P+1] -- always the FULL offsets; nothing is written at
 * or past cap_rows rows; points = row_inst = row_index = NULL is a sizing call (the convention of ls_tsdf_mesh_f64); counts may be NULL.
 * ls_tsdf_prior_vote_f32: sum, n (DEVICE, read only), s and trunc (HOST doubles), values float [rows] (DEVICE) in the order of the rows
 * entry; sum_out, n_out int32 [nx,ny,nz] (DEVICE), a SEPARATE pair, written for every sample.  An eligible sample finds its row as the
 * rows entry did (block offset + popcount of the lower lanes): no index array is read.  A row at or past `rows` casts no vote.
 * Refused on the host before the first HIP call, the problem named where there is one: dims < 1, P nx ny nz >= 2^31, nx ny nz above
 * 4096 blocks of 4096 samples (the scan limit of ls_tsdf_draw_f32), P outside 1 .. 65535, weight outside 1 .. 65535, s not finite or
 * <= 0, a grid that ls_depth_fuse_f32 refuses, null pointers, rows without their indices, a negative capacity, an output that aliases the
 * input state, a short workspace (LS_ERR_WORKSPACE).  Both entries take the workspace of ls_tsdf_prior_rows(_batch)_workspace_bytes, a
 * function of (P, nx, ny, nz), 0 for refused sizes: one ballot word per 64 samples and one count per block of 4096.
 * Launches, whatever P: the copy of the host scalars into the workspace and classify, ONE scan over the block counts of the batch,
 * emit (rows; none in a sizing call) or vote.  No host synchronisation, no allocation, no compact list; the voted / skipped counts are
 * two integer atomics per workgroup.  NO WEIGHT IS RECOMMENDED: nothing here can measure one. */
size_t ls_tsdf_prior_rows_workspace_bytes(int nx, int ny, int nz);
int ls_tsdf_prior_rows_f32(const int32_t* n, int nx, int ny, int nz, int weight, const double* origin, double voxel, float* points, int32_t* row_inst,
                           int32_t* row_index, long long cap_rows, long long* row_off, long long* counts, void* workspace, size_t workspace_bytes,
                           void* stream);
int ls_tsdf_prior_vote_f32(const int32_t* sum, const int32_t* n, int nx, int ny, int nz, int weight, double s, double trunc, const float* values,
                           long long rows, int32_t* sum_out, int32_t* n_out, long long* counts, void* workspace, size_t workspace_bytes, void* stream);
/* P >= 1 problems per call: one (nx, ny, nz) and one weight per call, sum / n / sum_out / n_out [P,nx,ny,nz], origin [P,3], voxel, s,
 * trunc [P] (HOST), counts [P,4]; the rows and the values of the batch are one packed list.  Every output of every problem is
 * BIT-IDENTICAL to the single entry on that problem alone (row_inst apart, which names the problem): the single entry is the batch of one. */
size_t ls_tsdf_prior_rows_batch_workspace_bytes(int P, int nx, int ny, int nz);
int ls_tsdf_prior_rows_batch_f32(int P, const int32_t* n, int nx, int ny, int nz, int weight, const double* origin, const double* voxel, float* points,
                                 int32_t* row_inst, int32_t* row_index, long long cap_rows, long long* row_off, long long* counts, void* workspace,
                                 size_t workspace_bytes, void* stream);
int ls_tsdf_prior_vote_batch_f32(int P, const int32_t* sum, const int32_t* n, int nx, int ny, int nz, int weight, const double* s, const double* trunc,
                                 const float* values, long long rows, int32_t* sum_out, int32_t* n_out, long long* counts, void* workspace,
                                 size_t workspace_bytes, void* stream);

/* Scene memory, the trimmed ICP with the point-to-plane metric (csrc/cloudnear.hip).  AN EXTENSION BEYOND THE RELEASED REFERENCE, like
 * ls_cloud_icp_f32, whose loop this is: a partial view registered point-to-point onto one point per voxel of a SURFACE slides along it
 * slowly; the distance to the tangent plane of the neighbour lets it slide.  The arguments are those of ls_cloud_icp_f32 plus N [a,3] fp32
 * (DEVICE) after A: the targets' normals, a zero row meaning "no normal".  The normals are an INPUT, so the operator does not depend on how
 * they were made (ls_cloud_normals_f32 is one way).  Definition, per problem (tests/plane_icp_oracle.py is the same text as NumPy), g_0 as
 * in ls_cloud_icp_f32, for k = 0, 1, ...:
 *   search      exactly ls_cloud_nearest_f32(A, B, g_k, r) -> f_k, n_k, S_k, nn_idx, nn_d2, as in ls_cloud_icp_f32.
 *   planar      a matched query is planar iff its neighbour's row of N is not (0, 0, 0); w_k is their number.  With y the posed row as the
 *               search formed it (fp32), a the neighbour and n its normal, all converted to float64:
 *               rho = ((y_0 - a_0) n_0 + (y_1 - a_1) n_1) + (y_2 - a_2) n_2, Q_k = sum rho^2 over the planar matches by the chunk rule.
 *   cost        E_k = (Q_k + (f_k - w_k) (double)r2) / f_k, 0 for f_k = 0: the truncated quadratic again, since rho^2 <= d2 <= r2 for
 *               unit normals.
 *   stop tests  those of ls_cloud_icp_f32 in the same order, each keeping g_k, with min_matched applied to w_k: w_k < min_matched:
 *               LS_ICP_STARVED; k >= 1 and E_{k-1} - E_k <= rel_thr E_{k-1}: LS_ICP_CONVERGED; k == max_iter: LS_ICP_MAX_ITER.  THE
 *               LINEARISED STEP IS NOT GUARANTEED TO LOWER E: there is no line search and no damping, and a step that raises E ends the
 *               loop as LS_ICP_CONVERGED at the next test, with the pose that step produced.  The trace shows E.
 *   update      minimise sum (rho + omega . (y x n) + v . n)^2 over the planar matches: J = (n, y x n) in R^6 in float64, the twist order
 *               (v, omega) of ls_se3_adam_step_f32; M = sum J J^T (21 unique entries), b = -sum J rho.  With Q these are 28 float64
 *               quantities per chunk, added by the rule of ls_cloud_icp_f32 (a fixed tree in each wave, a fixed tree over the four waves,
 *               one record per chunk, the records in chunk order).  Coordinates are not centred: the float64 choice of ls_cloud_icp_f32.
 *               M xi = b by Cholesky in float64 in a fixed order; a pivot that is not > 1e-12 times the original diagonal entry, or any
 *               non-finite value: LS_ICP_DEGENERATE, g_k is kept (one plane, or all normals parallel, is the exact case).
 *   retraction  Delta = exp(xi) in float64 by Rodrigues with the left Jacobian for the translation (first order below theta = 1e-6);
 *               R' = R_Delta R_k, t' = R_Delta t_k + t_Delta; R' is projected onto SO(3) by the rotation of ls_kabsch_batched_f32 for
 *               R'^T (its polar factor) and both are rounded to fp32: every g_k is orthonormal to fp32 rounding.
 * Outputs: those of ls_cloud_icp_f32 -- the final search is bit for bit ls_cloud_nearest_f32(A, B, g_out, r), the last search of the loop
 * -- plus planar long long [1] = w and sum_rho2 double [1] = Q of that search; stat_trace double [max_iter+1, 5] = (f_k, n_k, S_k, w_k,
 * Q_k).  Launches: 2 max_iter + 5 after the grid build, as there; a stopped problem is frozen.  The workspace is that of ls_cloud_icp_f32
 * with a record of 28 float64 and one more int per chunk of queries. */
size_t ls_cloud_icp_plane_workspace_bytes(long long a, long long b);
int ls_cloud_icp_plane_f32(const float* A, const float* N, long long a, const float* B, long long b, const float* g0, float radius, int max_iter,
                           double rel_thr, int min_matched, float* g_out, int32_t* stop, int32_t* iters, int32_t* nn_idx, float* nn_d2,
                           long long* counts, double* sum_d2, long long* planar, double* sum_rho2, int* status_out, float* g_trace,
                           double* stat_trace, void* workspace, size_t workspace_bytes, void* stream);
/* P >= 1 problems per call with the conventions of ls_cloud_icp_batch_f32; N [a_total,3] packed like A, planar / sum_rho2 [P], stat_trace
 * [P, max_iter+1, 5].  Every output of every problem is BIT-IDENTICAL to ls_cloud_icp_plane_f32 on that problem alone. */
size_t ls_cloud_icp_plane_batch_workspace_bytes(int P, long long a_total, long long b_total);
int ls_cloud_icp_plane_batch_f32(int P, const float* A, const float* N, long long a_total, const long long* a_off, const float* B,
                                 long long b_total, const long long* b_off, const float* g0, const float* radius, int max_iter, double rel_thr,
                                 int min_matched, float* g_out, int32_t* stop, int32_t* iters, int32_t* nn_idx, float* nn_d2, long long* counts,
                                 double* sum_d2, long long* planar, double* sum_rho2, int* status_out, float* g_trace, double* stat_trace,
                                 void* workspace, size_t workspace_bytes, void* stream);

/* The registration metrics of the relocalisation evaluation on P (reference instance, rescan instance, predicted pose, ground-truth pose)
 * tuples per call -- what eval_3rscan.py:384-401 / eval_flyingshape.py:136-148 compute pair by pair.  Pair p owns the rows
 * [x_off[p], x_off[p+1]) of X [n_total,3] (pc1) and [y_off[p], y_off[p+1]) of Y [m_total,3] (pc2); pred, gt [P,3,4] are the (R | t) that map
 * pc1 to pc2.  out [P,4] float64 = (rre_deg, rte, rmse, chamfer), the reference's definitions evaluated in float64 from the fp32 inputs:
 *   rre_deg  lib_more/pose_estimation.py:157-180 rotation_error: 180/pi acos(clamp((tr(R_pred^T R_gt) - 1) / 2, -1, 1)); the symmetry fold
 *            (eval_3rscan.py:387-393) stays with the caller
 *   rte      lib_more/pose_estimation.py:183-196 translation_error: |t_pred - t_gt|
 *   rmse     lib_more/pose_estimation.py:214-233 compute_transformation_error: sqrt((sum_x |pred x - gt x|^2 + sum_y |pred^-1 y - gt^-1 y|^2)
 *            / (3 (n_p + m_p))), inverses (R^T | -R^T t)
 *   chamfer  evaluate.py:111-123 chamfer_distance_torch on the rows 0, s, 2 s, ... (s = chamfer_stride; eval_3rscan.py:401 passes
 *            inst[:, ::10]) of each cloud, read in place: mean_i min_j |pred x'_i - y'_j|^2 + mean_j min_i |y'_j - (pred o gt^-1) y'_i|^2
 * x_off / y_off: HOST int64 arrays of P + 1 entries (P >= 1) starting at 0, never decreasing, ending at the totals, at most 2^31 - 1 rows per
 * cloud and no empty cloud (the reference gives NaN): checked before the first HIP call, with errors that name the problem, and copied into the
 * workspace on the stream.  No floating-point atomics: every sum is cut into chunks that depend on the pair alone and added in a fixed order,
 * so a pair's four values are BIT-IDENTICAL alone, first, last or anywhere in a batch.  Four launches whatever P; no host synchronisation,
 * no allocation.  ls_reg_metrics_batch_workspace_bytes: 0 for P < 1, a negative total or chamfer_stride < 1; a missing or short workspace
 * is LS_ERR_WORKSPACE. */
size_t ls_reg_metrics_batch_workspace_bytes(int P, long long n_total, long long m_total, int chamfer_stride);
int ls_reg_metrics_batch(int P, const float* X, long long n_total, const long long* x_off, const float* Y, long long m_total, const long long* y_off,
                         const float* pred, const float* gt, int chamfer_stride, double* out, void* workspace, size_t workspace_bytes,
                         void* stream);

/* ------------------------------------------------------------------------------------------------
 * Live per-kernel timing (bench.py's roofline leg): while enabled, every kernel ls_encode / ls_sdf_decode
 * launches is bracketed by hipEvents on the stream it is launched on.  ls_profile_end synchronises those
 * streams and returns, per (kind, layer), the number of launches and their summed duration.
 * ---------------------------------------------------------------------------------------------- */
typedef enum {
    LS_K_PROLOGUE = 0, LS_K_FPS, LS_K_KNN, LS_K_GEMM_EDGE, LS_K_EDGE_L0, LS_K_EDGE_POOL, LS_K_EDGE_ATTN, LS_K_MEAN,
    LS_K_GEMM_GLOB, LS_K_VN_ACT, LS_K_GEMM_TAIL, LS_K_TAIL, LS_K_SDF_PREP, LS_K_SDF_AFFINE, LS_K_GEMM_SDF, LS_K_SDF_OUT,
    LS_K_COUNT
} ls_kernel_kind;

typedef struct {
    int32_t kind;      /* ls_kernel_kind */
    int32_t layer;     /* encoder layer / FPS level / decoder layer */
    int32_t launches;
    float total_ms;
} ls_profile_entry;

int ls_profile_begin(ls_model_t* m);
int ls_profile_end(ls_model_t* m, ls_profile_entry* out_host, int max_entries, int* n_out_host);
/* Exact-phase statistics of the k-NN graph builds of the profiled ls_encode calls since ls_profile_begin (call BEFORE ls_profile_end, or
 * after it: the counters persist until the next ls_profile_begin): for encoder layer i, out_host[2 i] = candidates that were given a
 * canonical distance beyond the hints, summed over queries and calls, out_host[2 i + 1] = queries (0 for layers that do not run the
 * filter / exact-phase path).  bench.py derives the EXECUTED fp32 VALU work of the dominant k-NN launch from it (roofline.frac_hw). */
int ls_profile_knn_stats(ls_model_t* m, unsigned long long* out_host, int max_layers);

#ifdef __cplusplus
}
#endif
#endif /* LIVINGSCENES_HIP_H */
