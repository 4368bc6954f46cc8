"""Tensor-level wrappers over the C ABI (include/livingscenes_hip.h).  Inputs/outputs are HIP torch tensors;
torch only provides device memory and the current stream.  No CPU fallback anywhere (see _lib.ptr)."""
import ctypes
import os

import numpy as np
import torch

from . import _lib
from ._lib import call, check, load, ptr, stream_ptr

DEFAULT_FLAGS = 0  # canonical arithmetic: separately rounded multiply/add (oracle contract=0)


def _f32(t):
    return t.contiguous().float() if (t.dtype != torch.float32 or not t.is_contiguous()) else t


def _scratch(nbytes, device):
    """Caller-owned scratch for one operator call (torch's caching allocator: stream-ordered reuse, no hipMalloc per call)."""
    return torch.empty(nbytes, dtype=torch.uint8, device=device) if nbytes else None


def knn(dst, src, K=16, dst_rows=None, flags=DEFAULT_FLAGS, return_dist=False, seeds=None):
    """dst [B,Nd',3,C], src [B,Ns,3,C] -> idx [B,Nd,K] int32 (Nd = dst_rows.shape[1] if given).
    seeds [B,Nd,16] int32: optional candidate hints (result independent of them)."""
    dst, src = _f32(dst), _f32(src)
    B, dst_n, _, C = dst.shape
    Ns = src.shape[1]
    Nd = dst_rows.shape[1] if dst_rows is not None else dst_n
    idx = torch.empty(B, Nd, K, dtype=torch.int32, device=src.device)
    dist = torch.empty(B, Nd, K, dtype=torch.float32, device=src.device) if return_dist else None
    if seeds is not None:
        seeds = seeds.to(torch.int32).contiguous()
        assert seeds.shape == (B, Nd, 16)
    ws = _scratch(load().ls_knn_workspace_bytes(B, Nd, dst_n, Ns, C, int(seeds is not None), flags), src.device)
    call(src.device, "ls_knn_f32", ptr(dst), ptr(src), ptr(dst_rows), ptr(seeds), B, Nd, dst_n, Ns, C, K, flags, ptr(idx), ptr(dist),
                            ptr(ws), 0 if ws is None else ws.numel(), stream_ptr(src.device))
    return (idx, dist) if return_dist else idx


def fps(pts, K, lengths=None, flags=DEFAULT_FLAGS, return_points=False):
    """pts [B,N,3] -> idx [B,K] int32 (and the gathered points [B,K,3])."""
    pts = _f32(pts)
    B, N, _ = pts.shape
    idx = torch.empty(B, K, dtype=torch.int32, device=pts.device)
    out = torch.empty(B, K, 3, dtype=torch.float32, device=pts.device) if return_points else None
    if lengths is not None:
        lengths = lengths.to(device=pts.device, dtype=torch.int32).contiguous()
    ws = _scratch(load().ls_fps_workspace_bytes(B, N, K), pts.device)
    call(pts.device, "ls_fps_f32", ptr(pts), ptr(lengths), B, N, K, flags, ptr(idx), ptr(out), ptr(ws), 0 if ws is None else ws.numel(),
         stream_ptr(pts.device))
    return (idx, out) if return_points else idx


def gemm(A, W, bias=None, relu=False):
    """act(A[M,K] @ W[N,K]^T + bias) -> [M,N]."""
    A, W = _f32(A), _f32(W)
    M, K = A.shape
    N = W.shape[0]
    out = torch.empty(M, N, dtype=torch.float32, device=A.device)
    ws = _scratch(load().ls_gemm_workspace_bytes(M, N, K), A.device)
    call(A.device, "ls_gemm_f32", ptr(A), K, ptr(W), K, ptr(bias), ptr(out), N, M, N, K, int(relu), ptr(ws), 0 if ws is None else ws.numel(),
                             stream_ptr(A.device))
    return out


def rowmax(X):
    """max_k |X[r, k]| -> [rows]: the operand range ls_gemm_f32_ex takes for a weight matrix (once) or an input."""
    X = _f32(X)
    out = torch.empty(X.shape[0], dtype=torch.float32, device=X.device)
    call(X.device, "ls_rowmax_f32", ptr(X), X.shape[0], X.shape[1], X.shape[1], ptr(out), stream_ptr(X.device))
    return out


def presplit_w(W, w_rowmax):
    """ls_gemm_presplit_w_f32: both f16 pieces of the range-scaled rows of a weight matrix, for ``gemm_chain(..., w_planes=)``.  None when
    no kernel reads planes at this K (K < 512 or K % 32 != 0)."""
    W = _f32(W)
    N, K = W.shape
    nb = load().ls_gemm_w_planes_bytes(N, K)
    if nb == 0:
        return None
    planes = torch.empty(nb, dtype=torch.uint8, device=W.device)
    call(W.device, "ls_gemm_presplit_w_f32", ptr(W), K, N, K, ptr(w_rowmax), ptr(planes), nb, stream_ptr(W.device))
    return planes


def gemm_chain(A, W, bias=None, relu=False, a_rowmax=None, w_rowmax=None, want_rowmax=True, w_planes=None):
    """ls_gemm_f32_ex: the GEMM of ``gemm`` for a chain of layers -- takes the row maxima of its operands (``a_rowmax`` [M, parts] from
    the previous call, ``w_rowmax`` [N] from ``rowmax(W)``) and returns (out, out_rowmax [M, parts']) for the next one.  Never splits
    K (a row's result does not depend on the other rows of the call).  ``w_planes`` (``presplit_w(W, w_rowmax)``): ls_gemm_f32_planes,
    the same result without re-splitting W in every workgroup."""
    A, W = _f32(A), _f32(W)
    M, K = A.shape
    N = W.shape[0]
    out = torch.empty(M, N, dtype=torch.float32, device=A.device)
    parts = load().ls_gemm_rowmax_parts(N)
    orm = torch.empty(M, parts, dtype=torch.float32, device=A.device) if want_rowmax else None
    a_parts = 0 if a_rowmax is None else (1 if a_rowmax.dim() == 1 else a_rowmax.shape[1])
    if w_planes is not None:
        call(A.device, "ls_gemm_f32_planes", ptr(A), K, ptr(W), K, ptr(w_planes), ptr(bias), ptr(out), N, M, N, K, int(relu), ptr(a_rowmax),
             a_parts, ptr(w_rowmax), ptr(orm), stream_ptr(A.device))
        return out, orm
    call(A.device, "ls_gemm_f32_ex", ptr(A), K, ptr(W), K, ptr(bias), ptr(out), N, M, N, K, int(relu), ptr(a_rowmax), a_parts, ptr(w_rowmax),
         ptr(orm), None, 0, stream_ptr(A.device))
    return out, orm


def encode_prologue(x):
    """x [B,3,N] -> (pts [B,N,3], centroid [B,3], scale0 [B])."""
    x = _f32(x)
    B, _, N = x.shape
    pts = torch.empty(B, N, 3, dtype=torch.float32, device=x.device)
    cen = torch.empty(B, 3, dtype=torch.float32, device=x.device)
    sc = torch.empty(B, dtype=torch.float32, device=x.device)
    call(x.device, "ls_encode_prologue_f32", ptr(x), B, N, ptr(pts), ptr(cen), ptr(sc), stream_ptr(x.device))
    return pts, cen, sc


def cosine_scores(m0, m1):
    m0, m1 = _f32(m0), _f32(m1)
    n, D = m0.shape
    m = m1.shape[0]
    S = torch.empty(n, m, dtype=torch.float32, device=m0.device)
    ws = _scratch(load().ls_cosine_scores_workspace_bytes(n, m), m0.device)
    call(m0.device, "ls_cosine_scores_f32", ptr(m0), ptr(m1), n, m, D, ptr(S), ptr(ws), ws.numel(), stream_ptr(m0.device))
    return S


def greedy_match(scores):
    """scores [n,m] -> (matches0 [n], matches1 [m]) int64.  (The large-problem kernel normalises its input in place: copied then;
    the single-wave kernel of n * m <= 1024 keeps the matrix in registers and leaves `scores` untouched.)"""
    S = _f32(scores)
    n, m = S.shape
    if n * m > 1024:
        S = S.clone()
    m0 = torch.empty(n, dtype=torch.int64, device=S.device)
    m1 = torch.empty(m, dtype=torch.int64, device=S.device)
    call(S.device, "ls_greedy_match_f32", ptr(S), n, m, ptr(m0), ptr(m1), stream_ptr(S.device))
    return m0, m1


def nn_match(scores):
    """scores [n,m] -> mutual-nearest-neighbour (matches0 [n], matches1 [m]) int64 (matcher_new.py:89-98), one launch."""
    S = _f32(scores)
    n, m = S.shape
    m0 = torch.empty(n, dtype=torch.int64, device=S.device)
    m1 = torch.empty(m, dtype=torch.int64, device=S.device)
    call(S.device, "ls_nn_match_f32", ptr(S), n, m, ptr(m0), ptr(m1), stream_ptr(S.device))
    return m0, m1


def sinkhorn_match(scores, score_divisor, alpha=1.0, iters=100, match_threshold=0.0):
    """scores [n,m] -> (matches0 [n], matches1 [m]) int64: log-space optimal transport with a dustbin + mutual arg-maxes (matcher_new.py:20-71),
    the whole loop in one launch."""
    S = _f32(scores)
    n, m = S.shape
    m0 = torch.empty(n, dtype=torch.int64, device=S.device)
    m1 = torch.empty(m, dtype=torch.int64, device=S.device)
    call(S.device, "ls_sinkhorn_match_f32", ptr(S), n, m, float(score_divisor), float(alpha), int(iters), float(match_threshold), ptr(m0), ptr(m1),
         stream_ptr(S.device))
    return m0, m1


# ---- ragged batches of matching problems (ls_*_batch_f32): one call for P problems, every problem's result bit-identical to the single form.
# Offsets come from shapes (sizes), never from the device.  A problem with n == 0 or m == 0 is allowed: no scores, every match -1.
def _match_sizes(sizes):
    sizes = [(int(n), int(m)) for n, m in sizes]
    if any(n < 0 or m < 0 for n, m in sizes):
        raise ValueError(f"negative problem size in {sizes}")
    return sizes


def _match_offsets(sizes):
    return _offsets([n for n, _ in sizes]), _offsets([m for _, m in sizes])


def _pack_rows(x, sizes, side, what):
    """list of [rows_p, ...] tensors, or a packed [rows_total, ...] tensor whose rows `sizes` divides -> (packed float32 contiguous, sizes of the side)"""
    if torch.is_tensor(x):
        if sizes is None:
            raise ValueError(f"{what}: a packed tensor needs sizes=[(n_p, m_p), ...]")
        rows = [s[side] for s in _match_sizes(sizes)]
        if x.shape[0] != sum(rows):
            raise ValueError(f"{what}: {x.shape[0]} packed rows, the sizes add up to {sum(rows)}")
        return _f32(x), rows
    xs = list(x)
    if not xs:
        raise ValueError(f"{what}: empty list of problems")
    tails = {tuple(t.shape[1:]) for t in xs}
    if len(tails) != 1:
        raise ValueError(f"{what}: the problems of one call share their row shape (descriptor width), got {sorted(tails)}")
    return _f32(torch.cat([_f32(t) for t in xs], 0)), [t.shape[0] for t in xs]


def _pack_scores(scores, sizes, what, copy=False):
    """list of [n_p, m_p] score matrices, or a packed 1-D tensor plus sizes -> (packed float32 [sum n_p m_p], sizes)"""
    if torch.is_tensor(scores):
        if sizes is None:
            raise ValueError(f"{what}: packed scores need sizes=[(n_p, m_p), ...]")
        sizes = _match_sizes(sizes)
        S = _f32(scores.reshape(-1))
        if S.numel() != sum(n * m for n, m in sizes):
            raise ValueError(f"{what}: {S.numel()} packed scores, the sizes add up to {sum(n * m for n, m in sizes)}")
        return (S.clone() if copy and S.data_ptr() == scores.data_ptr() else S), sizes
    mats = list(scores)
    if not mats:
        raise ValueError(f"{what}: empty list of problems")
    if any(t.dim() != 2 for t in mats):
        raise ValueError(f"{what}: every problem's scores are a matrix [n, m]")
    return torch.cat([_f32(t).reshape(-1) for t in mats], 0), [tuple(t.shape) for t in mats]     # (cat: always a new tensor)


def _split_scores(S, sizes):
    """packed scores -> per-problem [n_p, m_p] views"""
    return [part.view(n, m) for part, (n, m) in zip(torch.split(S, [n * m for n, m in sizes]), sizes)]


def _split_matches(m0, m1, sizes):
    return list(zip(torch.split(m0, [n for n, _ in sizes]), torch.split(m1, [m for _, m in sizes])))


def _match_batch_call(name, dev, sizes, head_of, outs):
    """workspace query + the call: head_of(n_total, so, m_total, to) -> the arguments between P and the outputs"""
    P = len(sizes)
    so, to = _match_offsets(sizes)
    nt, mt = int(so[-1]), int(to[-1])
    ws = _scratch(getattr(load(), name.replace("_f32", "_workspace_bytes"))(P, nt, mt), dev)
    call(dev, name, P, *head_of(nt, _hptr(so), mt, _hptr(to)), *[ptr(o) for o in outs], ptr(ws), 0 if ws is None else ws.numel(), stream_ptr(dev))


def cosine_scores_batch(m0, m1, sizes=None, packed=False):
    """cosine_scores on P problems in one call: m0 / m1 = lists of [n_p, D] / [m_p, D] tensors, or packed [n_total, D] / [m_total, D] tensors
    plus sizes = [(n_p, m_p), ...] -> list of P [n_p, m_p] views of one packed tensor (packed=True: that tensor and the sizes), problem p
    bit-identical to cosine_scores(m0_p, m1_p)."""
    M0, ns = _pack_rows(m0, sizes, 0, "cosine_scores_batch")
    M1, ms = _pack_rows(m1, sizes, 1, "cosine_scores_batch")
    if M0.dim() != 2 or M1.dim() != 2 or M0.shape[1] != M1.shape[1]:
        raise ValueError(f"cosine_scores_batch: descriptors [n, D] of one width on both sides, got {tuple(M0.shape)} and {tuple(M1.shape)}")
    if len(ns) != len(ms):
        raise ValueError(f"cosine_scores_batch: {len(ns)} source sets for {len(ms)} target sets")
    sizes = list(zip(ns, ms))
    S = torch.empty(sum(n * m for n, m in sizes), dtype=torch.float32, device=M0.device)
    _match_batch_call("ls_cosine_scores_batch_f32", M0.device, sizes,
                      lambda nt, so, mt, to: (ptr(M0), nt, so, ptr(M1), mt, to, M0.shape[1]), [S])
    return (S, sizes) if packed else _split_scores(S, sizes)


def _assign_batch(name, scores, sizes, extra, copy):
    S, sizes = _pack_scores(scores, sizes, name, copy=copy)
    dev = S.device
    m0 = torch.empty(sum(n for n, _ in sizes), dtype=torch.int64, device=dev)
    m1 = torch.empty(sum(m for _, m in sizes), dtype=torch.int64, device=dev)
    _match_batch_call(name, dev, sizes, lambda nt, so, mt, to: (ptr(S), nt, so, mt, to) + tuple(extra), [m0, m1])
    return _split_matches(m0, m1, sizes)


def greedy_match_batch(scores, sizes=None):
    """greedy_match on P problems in one call: scores = list of [n_p, m_p] matrices, or the packed scores plus sizes -> list of P
    (matches0 [n_p], matches1 [m_p]) int64 views, indices local to the problem.  Works on its own copy: the caller's scores are untouched."""
    return _assign_batch("ls_greedy_match_batch_f32", scores, sizes, (), copy=True)


def nn_match_batch(scores, sizes=None):
    """nn_match on P problems in one call (arguments and result as greedy_match_batch)."""
    return _assign_batch("ls_nn_match_batch_f32", scores, sizes, (), copy=False)


def sinkhorn_match_batch(scores, score_divisor, alpha=1.0, iters=100, match_threshold=0.0, sizes=None):
    """sinkhorn_match on P problems in one call; score_divisor, alpha, iters and match_threshold hold for the whole batch."""
    return _assign_batch("ls_sinkhorn_match_batch_f32", scores, sizes, (float(score_divisor), float(alpha), int(iters), float(match_threshold)),
                         copy=False)


def kabsch_residual_matrix_batch(src, tgt, sizes=None, packed=False):
    """kabsch_residual_matrix on P problems in one call: src / tgt = lists of [n_p, C, 3] / [m_p, C, 3] tensors, or packed tensors plus sizes
    -> list of P [n_p, m_p] views of one packed tensor (packed=True: that tensor and the sizes)."""
    A, ns = _pack_rows(src, sizes, 0, "kabsch_residual_matrix_batch")
    B, ms = _pack_rows(tgt, sizes, 1, "kabsch_residual_matrix_batch")
    if A.dim() != 3 or A.shape[2] != 3 or A.shape[1:] != B.shape[1:]:
        raise ValueError(f"kabsch_residual_matrix_batch: point sets [n, C, 3] of one C on both sides, got {tuple(A.shape)} and {tuple(B.shape)}")
    if len(ns) != len(ms):
        raise ValueError(f"kabsch_residual_matrix_batch: {len(ns)} source sets for {len(ms)} target sets")
    sizes = list(zip(ns, ms))
    res = torch.empty(sum(n * m for n, m in sizes), dtype=torch.float32, device=A.device)
    _match_batch_call("ls_kabsch_residual_matrix_batch_f32", A.device, sizes,
                      lambda nt, so, mt, to: (ptr(A), nt, so, ptr(B), mt, to, A.shape[1]), [res])
    return (res, sizes) if packed else _split_scores(res, sizes)


def _poses_3x4(g, P, what):
    """[P,3,4] or [P,4,4] -> fp32 contiguous [P,3,4]"""
    if g.dim() != 3 or g.shape[0] != P or g.shape[1] not in (3, 4) or g.shape[2] != 4:
        raise ValueError(f"reg_metrics_batch: {what} must be [P,3,4] or [P,4,4] with P = {P}, got {tuple(g.shape)}")
    return _f32(g[:, :3, :])


def reg_metrics_batch(pcs1, pcs2, pred, gt, chamfer_stride=10, sizes=None):
    """The registration metrics of P pairs in one call (ls_reg_metrics_batch): pcs1 / pcs2 = lists of [n_p,3] / [m_p,3] clouds (the reference
    instance and the rescan instance), or packed [n_total,3] / [m_total,3] tensors plus sizes = [(n_p, m_p), ...]; pred, gt [P,3,4] or
    [P,4,4] map pc1 to pc2 -> float64 [P,4] = (rre_deg, rte, rmse, chamfer) per pair: rotation_error (unfolded), translation_error,
    compute_transformation_error and chamfer_distance_torch on every chamfer_stride-th row, in float64.  Row p is the same bits whatever
    else is in the batch."""
    X, ns = _pack_rows(pcs1, sizes, 0, "reg_metrics_batch")
    Y, ms = _pack_rows(pcs2, sizes, 1, "reg_metrics_batch")
    if X.dim() != 2 or Y.dim() != 2 or X.shape[1] != 3 or Y.shape[1] != 3:
        raise ValueError(f"reg_metrics_batch: clouds are [n, 3], got {tuple(X.shape)} and {tuple(Y.shape)}")
    if len(ns) != len(ms):
        raise ValueError(f"reg_metrics_batch: {len(ns)} reference clouds for {len(ms)} rescan clouds")
    P, dev = len(ns), X.device
    pred, gt = _poses_3x4(pred.to(dev), P, "pred"), _poses_3x4(gt.to(dev), P, "gt")
    xo, yo = _offsets(ns), _offsets(ms)
    s = int(chamfer_stride)
    out = torch.empty(P, 4, dtype=torch.float64, device=dev)
    ws = _scratch(load().ls_reg_metrics_batch_workspace_bytes(P, X.shape[0], Y.shape[0], s), dev)
    call(dev, "ls_reg_metrics_batch", P, ptr(X), X.shape[0], _hptr(xo), ptr(Y), Y.shape[0], _hptr(yo), ptr(pred), ptr(gt), s, ptr(out), ptr(ws),
         0 if ws is None else ws.numel(), stream_ptr(dev))
    return out


def kabsch(x1, x2, weights=None, return_flags=False, raw_weights=False):
    """x1,x2 [b,n,3] -> R [b,3,3], t [b,3,1], res [b,n] (, status [b] int32: _lib.KABSCH_*).  raw_weights: use `weights` as
    they are instead of normalising them (pose_estimation.py:52-54)."""
    x1, x2 = _f32(x1), _f32(x2)
    b, n, _ = x1.shape
    if weights is not None:
        weights = _f32(weights)
    R = torch.empty(b, 3, 3, dtype=torch.float32, device=x1.device)
    t = torch.empty(b, 3, dtype=torch.float32, device=x1.device)
    res = torch.empty(b, n, dtype=torch.float32, device=x1.device)
    fl = torch.empty(b, dtype=torch.int32, device=x1.device)
    call(x1.device, "ls_kabsch_batched_f32", ptr(x1), ptr(x2), ptr(weights), b, n, _lib.FLAG_KABSCH_RAW_WEIGHTS if raw_weights else 0,
                                       ptr(R), ptr(t), ptr(res), ptr(fl),
                                       stream_ptr(x1.device))
    return (R, t.unsqueeze(2), res, fl) if return_flags else (R, t.unsqueeze(2), res)


def kabsch_codes(z1, t1, z2, t2, sel2=None, sel1=None, want_res=False):
    """Kabsch on the pseudo-points z + t of two code sets (more_solver.py:114-116) in ONE launch: z [n,c,3], t [n,1,3] or [n,3];
    sel2 / sel1 (int64 [b], optional): problem p pairs set sel1[p] (default p) of side 1 with set sel2[p] of side 2 -- e.g. matches0
    (negative = unmatched -> set 0, as matches0.clamp(min=0)).  -> R [b,3,3], t [b,3,1] (, res [b,c])."""
    z1, z2 = _f32(z1), _f32(z2)
    t1, t2 = _f32(t1.reshape(-1, 3)), _f32(t2.reshape(-1, 3))
    b = (sel1 if sel1 is not None else sel2).shape[0] if (sel1 is not None or sel2 is not None) else z1.shape[0]
    n = z1.shape[1]
    R = torch.empty(b, 3, 3, dtype=torch.float32, device=z1.device)
    t = torch.empty(b, 3, dtype=torch.float32, device=z1.device)
    res = torch.empty(b, n, dtype=torch.float32, device=z1.device) if want_res else None
    if sel1 is not None:
        sel1 = sel1.contiguous().long()
    if sel2 is not None:
        sel2 = sel2.contiguous().long()
    call(z1.device, "ls_kabsch_codes_f32", ptr(z1), ptr(t1), ptr(sel1), ptr(z2), ptr(t2), ptr(sel2), b, n, ptr(R), ptr(t), ptr(res), None,
         stream_ptr(z1.device))
    return (R, t.unsqueeze(2), res) if want_res else (R, t.unsqueeze(2))


def kabsch_residual_matrix(src, tgt):
    """src [n,P,3], tgt [m,P,3] -> mean residual [n,m]."""
    src, tgt = _f32(src), _f32(tgt)
    n, P, _ = src.shape
    m = tgt.shape[0]
    res = torch.empty(n, m, dtype=torch.float32, device=src.device)
    call(src.device, "ls_kabsch_residual_matrix_f32", ptr(src), ptr(tgt), n, m, P, ptr(res), stream_ptr(src.device))
    return res


def icp(X, Y, R0, T0, max_iter=100, rel_rmse_thr=1e-6, flags=DEFAULT_FLAGS):
    """Row-vector convention Xt = X R + T.  X [b,n,3], Y [b,m,3], R0 [b,3,3], T0 [b,3] -> R, T, rmse [b], iters [b]."""
    X, Y, R0, T0 = _f32(X), _f32(Y), _f32(R0), _f32(T0)
    b, n, _ = X.shape
    m = Y.shape[1]
    R = torch.empty(b, 3, 3, dtype=torch.float32, device=X.device)
    T = torch.empty(b, 3, dtype=torch.float32, device=X.device)
    rmse = torch.empty(b, dtype=torch.float32, device=X.device)
    iters = torch.empty(b, dtype=torch.int32, device=X.device)
    ws = torch.empty(load().ls_icp_workspace_bytes(b, n), dtype=torch.uint8, device=X.device)
    call(X.device, "ls_icp_f32", ptr(X), ptr(Y), ptr(R0), ptr(T0), b, n, m, max_iter, rel_rmse_thr, flags, ptr(R), ptr(T),
                            ptr(rmse), ptr(iters), ptr(ws), ws.numel(), stream_ptr(X.device))
    return R, T, rmse, iters


def se3_transform(g, src):
    """g [P,3,4] (R | t), src [P,N,3] -> g . src [P,N,3]."""
    g, src = _f32(g), _f32(src)
    P, N, _ = src.shape
    out = torch.empty_like(src)
    call(src.device, "ls_se3_transform_f32", ptr(g), ptr(src), P, N, ptr(out), stream_ptr(src.device))
    return out


def smooth_l1(sdf, loss=None):
    """Per-row mean SmoothL1(sdf, 0) of sdf [P,N] -> (loss [P] (added to `loss` if given), d loss / d sdf [P,N])."""
    sdf = _f32(sdf)
    P, N = sdf.shape
    acc = loss is not None
    if loss is None:
        loss = torch.empty(P, dtype=torch.float32, device=sdf.device)
    grad = torch.empty_like(sdf)
    call(sdf.device, "ls_smooth_l1_f32", ptr(sdf), P, N, int(acc), ptr(loss), ptr(grad), stream_ptr(sdf.device))
    return loss, grad


def mse(sdf, min_loss=None, improved=None):
    """Per-row MSELoss(sdf, 0) of sdf [P,N] -> (loss [P], d loss / d sdf [P,N]); min_loss [P] float / improved [P] int32 (optional) are
    updated in place where the loss improved (More_Solver._optimize_code's bookkeeping, more_solver.py:219-221)."""
    sdf = _f32(sdf)
    P, N = sdf.shape
    loss = torch.empty(P, dtype=torch.float32, device=sdf.device)
    grad = torch.empty_like(sdf)
    call(sdf.device, "ls_mse_f32", ptr(sdf), P, N, ptr(loss), ptr(grad), ptr(min_loss), ptr(improved), stream_ptr(sdf.device))
    return loss, grad


class Adam:
    """torch.optim.Adam(params with per-group lr) on the device: ONE launch per step for up to four tensors (csrc/optim.hip:
    adam_multi_kernel, torch's operation order).  params: list of (tensor updated in place, lr)."""

    def __init__(self, params, betas=(0.9, 0.999), eps=1e-8):
        assert 1 <= len(params) <= 4
        self.params = [(p, float(lr)) for p, lr in params]
        for p, _ in self.params:
            assert p.is_contiguous() and p.dtype == torch.float32
        self.m = [torch.zeros_like(p) for p, _ in self.params]
        self.v = [torch.zeros_like(p) for p, _ in self.params]
        self.betas, self.eps, self.step_no = betas, eps, 0

    def step(self, grads, lr_scale=1.0):
        groups = (_lib.AdamGroup * len(self.params))()
        keep = []
        for i, ((p, lr), g) in enumerate(zip(self.params, grads)):
            g = _f32(g.reshape(p.shape))
            keep.append(g)
            groups[i] = _lib.AdamGroup(p.data_ptr(), g.data_ptr(), self.m[i].data_ptr(), self.v[i].data_ptr(), p.numel(), lr * lr_scale)
        call(self.params[0][0].device, "ls_adam_step_f32", groups, len(self.params), self.betas[0], self.betas[1], self.eps, self.step_no,
             stream_ptr(self.params[0][0].device))
        self.step_no += 1


class Se3Adam:
    """State of the batched SE(3) Adam of the optimisation-based registration (csrc/optim.hip: se3_adam_step_kernel)."""

    def __init__(self, g0, src, stop_angle, betas=(0.9, 0.999), eps=1e-8):
        self.src = _f32(src)
        self.g = _f32(g0).clone()
        P = self.g.shape[0]
        dev = self.g.device
        self.m1 = torch.zeros(P, 6, device=dev)
        self.m2 = torch.zeros(P, 6, device=dev)
        self.min_loss = torch.full((P,), 100.0, device=dev)       # more_solver.py:141
        self.best_g = self.g.clone()
        self.init_R = self.g[:, :, :3].contiguous().clone()
        self.active = torch.ones(P, dtype=torch.int32, device=dev)
        self.query = se3_transform(self.g, self.src)
        self.betas, self.eps, self.stop_angle, self.step_no = betas, eps, float(stop_angle), 0

    def step(self, grad_query, loss, lr):
        P, N, _ = self.src.shape
        call(self.src.device, "ls_se3_adam_step_f32", ptr(self.src), ptr(_f32(grad_query)), ptr(_f32(loss)), P, N, float(lr), self.betas[0],
             self.betas[1], self.eps, self.step_no, self.stop_angle, ptr(self.g), ptr(self.m1), ptr(self.m2), ptr(self.min_loss),
             ptr(self.best_g), ptr(self.init_R), ptr(self.active), ptr(self.query), stream_ptr(self.src.device))
        self.step_no += 1


class HipModel:
    """Owner of an ls_model_t (device-resident packed weights) with encode / sdf_decode entry points."""

    def __init__(self, desc, blob, device):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.LsError("HipModel needs a HIP device: the MI355X path has no CPU fallback")
        self.desc = desc
        self._h = ctypes.c_void_p()
        self._ws = {}
        with torch.cuda.device(self.device):
            check(load().ls_model_create(ctypes.byref(desc), blob.ctypes.data_as(ctypes.c_void_p), ctypes.byref(self._h)),
                  "ls_model_create")

    def close(self):
        if self._h:
            load().ls_model_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _workspace(self, nbytes):
        """Grow-only scratch, one buffer per STREAM the handle is used on (two streams driving one handle must not share it)."""
        key = torch.cuda.current_stream(self.device).cuda_stream
        ws = self._ws.get(key)
        if ws is None or ws.numel() < nbytes:
            ws = self._ws[key] = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return ws

    def get_option(self, option):
        """ls_model_get_option (_lib.OPT_*): the handle's current value, read from the library (never mirrored in Python)."""
        v = ctypes.c_int(0)
        check(load().ls_model_get_option(self._h, int(option), ctypes.byref(v)), "ls_model_get_option")
        return int(v.value)

    def set_option(self, option, value):
        """ls_model_set_option (_lib.OPT_*) -> the value the option had before (asked of the library), so that a temporary change can be
        undone without clobbering a caller's setting or the environment's default."""
        prev = self.get_option(option)
        check(load().ls_model_set_option(self._h, int(option), int(value)), "ls_model_set_option")
        return prev

    def profile_begin(self):
        check(load().ls_profile_begin(self._h), "ls_profile_begin")

    def profile_end(self):
        """-> list of dicts {kind, layer, launches, total_ms} (hipEvent-bracketed per launch)."""
        buf = (_lib.ProfileEntry * 256)()
        n = ctypes.c_int(0)
        check(load().ls_profile_end(self._h, buf, 256, ctypes.byref(n)), "ls_profile_end")
        return [dict(kind=_lib.KERNEL_KINDS[buf[i].kind], layer=buf[i].layer, launches=buf[i].launches, total_ms=buf[i].total_ms)
                for i in range(n.value)]

    def profile_knn_stats(self):
        """ls_profile_knn_stats -> {layer: (candidates given a canonical distance beyond the hints, queries)} of the profiled encode calls."""
        buf = (ctypes.c_ulonglong * 16)()
        check(load().ls_profile_knn_stats(self._h, buf, 8), "ls_profile_knn_stats")
        return {i: (int(buf[2 * i]), int(buf[2 * i + 1])) for i in range(8) if buf[2 * i + 1]}

    def n_levels(self):
        return [int(self.desc.down_factor[i]) for i in range(self.desc.num_layers)]

    def encode(self, x, pre_normalised=False, flags=DEFAULT_FLAGS, trace=False):
        """x [B,3,N] -> (z_so3 [B,C,3], z_inv [B,C], s [B], t [B,3]) (+ per-layer knn / fps index lists)."""
        x = _f32(x)
        B, three, N = x.shape
        assert three == 3
        d = self.desc
        C = d.c_dim
        dev = x.device
        z_so3 = torch.empty(B, C, 3, dtype=torch.float32, device=dev)
        z_inv = torch.empty(B, C, dtype=torch.float32, device=dev)
        s = torch.empty(B, dtype=torch.float32, device=dev)
        t = torch.empty(B, 3, dtype=torch.float32, device=dev)
        need = load().ls_encoder_workspace_bytes(self._h, B, N)
        if need == 0:
            raise _lib.LsError("ls_encoder_workspace_bytes: " + load().ls_last_error().decode())
        ws = self._workspace(need)
        tk = tf = None
        nds, fps_n = [], []
        cur = N
        for i in range(d.num_layers):
            if d.down_factor[i] > 1:
                cur //= d.down_factor[i]
                fps_n.append(cur)
            nds.append(cur)
        if trace:
            tk = torch.empty(B * sum(nds) * 16, dtype=torch.int32, device=dev)
            tf = torch.empty(max(1, B * sum(fps_n)), dtype=torch.int32, device=dev)
        call(dev, "ls_encode", self._h, ptr(x), B, N, int(pre_normalised), flags, ptr(z_so3), ptr(z_inv), ptr(s), ptr(t),
                               ptr(tk), ptr(tf), ptr(ws), ws.numel(), stream_ptr(dev))
        if not trace:
            return z_so3, z_inv, s, t
        knn_l, fps_l, o = [], [], 0
        for nd in nds:
            knn_l.append(tk[o:o + B * nd * 16].view(B, nd, 16))
            o += B * nd * 16
        o = 0
        for nf in fps_n:
            fps_l.append(tf[o:o + B * nf].view(B, nf))
            o += B * nf
        return z_so3, z_inv, s, t, knn_l, fps_l

    # ---- the encoder's layer operators on their own (same code path as ls_encode)
    def edgeconv(self, layer, src_f, knn, dst_rows=None, _ws=None):
        """Edge-conv layer `layer` without its residual global conv: src_f [B,Ns,3,C_in] (layer 0: cloud [B,Ns,3]), knn [B,Nd,16]
        int32, dst_rows [B,Nd] int32 or None -> [B,Nd,3,C_out]."""
        src_f = _f32(src_f)
        knn = knn.to(torch.int32).contiguous()
        B, Ns = src_f.shape[0], src_f.shape[1]
        Nd = knn.shape[1]
        if dst_rows is not None:
            dst_rows = dst_rows.to(torch.int32).contiguous()
        Co = int(self.desc.feat_dim[layer])
        out = torch.empty(B, Nd, 3, Co, dtype=torch.float32, device=src_f.device)
        ws = _ws if _ws is not None else _scratch(load().ls_vn_edgeconv_workspace_bytes(self._h, layer, B, Ns, Nd, int(dst_rows is not None)), src_f.device)
        fn = "ls_vn_edgeconv_attn_f32" if layer >= self.desc.atten_start_layer else "ls_vn_edgeconv_pool_f32"
        call(src_f.device, fn, self._h, layer, ptr(src_f), ptr(knn), ptr(dst_rows), B, Ns, Nd, ptr(out), ptr(ws), 0 if ws is None else ws.numel(),
             stream_ptr(src_f.device))
        return out

    def vn_lna_global(self, layer, f):
        """Residual global conv of `layer`: f [B,N,3,C] -> VecLNA_G(cat(f, mean_n f)) [B,N,3,C]."""
        f = _f32(f)
        B, N = f.shape[0], f.shape[1]
        out = torch.empty_like(f)
        ws = _scratch(load().ls_vn_lna_workspace_bytes(self._h, layer, B, N), f.device)
        call(f.device, "ls_vn_lna_f32", self._h, layer, ptr(f), B, N, ptr(out), ptr(ws), ws.numel(), stream_ptr(f.device))
        return out

    def encoder_tail(self, f, centroid=None, scale0=None):
        """f [B,NP,3,C_last] -> (z_so3 [B,c,3], z_inv [B,c], s [B], t [B,3])."""
        f = _f32(f)
        B, NP = f.shape[0], f.shape[1]
        C, dev = self.desc.c_dim, f.device
        z_so3 = torch.empty(B, C, 3, dtype=torch.float32, device=dev)
        z_inv = torch.empty(B, C, dtype=torch.float32, device=dev)
        s, t = torch.empty(B, dtype=torch.float32, device=dev), torch.empty(B, 3, dtype=torch.float32, device=dev)
        ws = _scratch(load().ls_encoder_tail_workspace_bytes(self._h, B, NP), dev)
        call(dev, "ls_encoder_tail_f32", self._h, ptr(f), ptr(None if centroid is None else _f32(centroid)),
                                         ptr(None if scale0 is None else _f32(scale0)), B, NP, ptr(z_so3), ptr(z_inv), ptr(s), ptr(t),
                                         ptr(ws), ws.numel(), stream_ptr(dev))
        return z_so3, z_inv, s, t

    def sdf_decode(self, query, z_so3, z_inv, s, t, max_ws_bytes=2 << 30):
        """query [B,M,3] + code -> sdf [B,M]; queries are processed in chunks that keep the workspace bounded."""
        query = _f32(query)
        B, M, _ = query.shape
        z_so3, z_inv, s, t = _f32(z_so3), _f32(z_inv), _f32(s), _f32(t.reshape(B, 3))
        sdf = torch.empty(B, M, dtype=torch.float32, device=query.device)
        per_q = 2 * self.desc.dec_width * 4 * B
        chunk = max(64, min(M, int(max_ws_bytes // max(per_q, 1))))
        for m0 in range(0, M, chunk):
            mc = min(chunk, M - m0)
            q = query[:, m0:m0 + mc].contiguous()
            out = sdf if mc == M else torch.empty(B, mc, dtype=torch.float32, device=query.device)
            need = load().ls_sdf_workspace_bytes(self._h, B, mc)
            ws = self._workspace(need)
            call(query.device, "ls_sdf_decode", self._h, ptr(q), ptr(z_so3), ptr(z_inv), ptr(s), ptr(t), B, mc, ptr(out), ptr(ws),
                                       ws.numel(), stream_ptr(query.device))
            if mc != M:
                sdf[:, m0:m0 + mc] = out
        return sdf

    def sdf_decode_rows(self, query, row_inst, z_so3, z_inv, s, t, max_rows=1 << 20):
        """Ragged batch: query [R,3], row_inst [R] int32 (instance of each row; rows of an instance contiguous) -> sdf [R]."""
        query = _f32(query)
        R = query.shape[0]
        B = z_inv.shape[0]
        row_inst = row_inst.to(torch.int32).contiguous()
        z_so3, z_inv, s, t = _f32(z_so3), _f32(z_inv), _f32(s), _f32(t.reshape(B, 3))
        sdf = torch.empty(R, dtype=torch.float32, device=query.device)
        for r0 in range(0, R, max_rows):
            rc = min(max_rows, R - r0)
            q, ri, out = query[r0:r0 + rc], row_inst[r0:r0 + rc], sdf[r0:r0 + rc]
            need = load().ls_sdf_rows_workspace_bytes(self._h, B, rc)
            ws = self._workspace(need)
            call(query.device, "ls_sdf_decode_rows", self._h, ptr(q), ptr(ri), ptr(z_so3), ptr(z_inv), ptr(s), ptr(t), B, rc, ptr(out), ptr(ws),
                                            ws.numel(), stream_ptr(query.device))
        return sdf

    def sdf_decode_train(self, query, z_so3, z_inv, s, t):
        """Forward that keeps the activations: -> (sdf [B,M], saved) where ``saved`` feeds sdf_backward (its workspace is
        private to the call, so several graphs can be alive at once)."""
        query = _f32(query)
        B, M, _ = query.shape
        z_so3, z_inv, s, t = _f32(z_so3), _f32(z_inv), _f32(s), _f32(t.reshape(B, 3))
        sdf = torch.empty(B, M, dtype=torch.float32, device=query.device)
        need = load().ls_sdf_train_workspace_bytes(self._h, B, M)
        ws = torch.empty(need, dtype=torch.uint8, device=query.device)
        call(query.device, "ls_sdf_decode_train", self._h, ptr(query), ptr(z_so3), ptr(z_inv), ptr(s), ptr(t), B, M, ptr(sdf), ptr(ws),
                                         ws.numel(), stream_ptr(query.device))
        return sdf, (query, z_so3, z_inv, s, t, sdf, ws)

    def sdf_backward(self, saved, grad_sdf, need_query_grad=True, need_code_grad=True):
        """-> (grad_query [B,M,3] or None, grad_z_so3 [B,c,3] or None, grad_z_inv [B,c] or None, grad_s [B], grad_t [B,3])."""
        query, z_so3, z_inv, s, t, sdf, ws = saved
        B, M, _ = query.shape
        dev = query.device
        g = _f32(grad_sdf).reshape(B, M)
        gq = torch.empty(B, M, 3, dtype=torch.float32, device=dev) if need_query_grad else None
        gso3, ginv = (torch.empty_like(z_so3), torch.empty_like(z_inv)) if need_code_grad else (None, None)
        gs, gt = torch.empty_like(s), torch.empty_like(t)
        call(dev, "ls_sdf_backward", self._h, ptr(query), ptr(z_so3), ptr(z_inv), ptr(s), ptr(t), B, M, ptr(sdf), ptr(g), ptr(ws),
                                     ws.numel(), ptr(gq), ptr(gso3), ptr(ginv), ptr(gs), ptr(gt), stream_ptr(dev))
        return gq, gso3, ginv, gs, gt


# ------------------------------------------------------------------------------------------------ mesh metrics (csrc/meshmetrics.hip)
def _mesh_dev(V, F):
    """V [nv,3] float64, F [nf,3] int32 HIP tensors (the caller converted and range-checked them: evaluate._device_mesh)."""
    if V.dtype != torch.float64 or F.dtype != torch.int32 or V.dim() != 2 or F.dim() != 2 or V.shape[1] != 3 or F.shape[1] != 3:
        raise _lib.LsError("mesh operators take vertices [nv,3] float64 and faces [nf,3] int32")
    return V.contiguous(), F.contiguous()


def _sized_call(dev, name, head, out, ws_bytes):
    """Sizing call (entries = NULL -> bin entry count on the device), host read, allocation, real call -- ls_marching_cubes_f64's convention."""
    counts = torch.empty(1, dtype=torch.int64, device=dev)
    ws = _scratch(ws_bytes, dev)
    nbytes = 0 if ws is None else ws.numel()
    call(dev, name, *head, ptr(out), None, 0, ptr(counts), ptr(ws), nbytes, stream_ptr(dev))
    entries = torch.empty(max(int(counts.item()), 1), dtype=torch.int32, device=dev)
    call(dev, name, *head, ptr(out), ptr(entries), entries.numel(), ptr(counts), ptr(ws), nbytes, stream_ptr(dev))
    return out


def _binned(name, ws_bytes, V, F, points, extra, out):
    head = (ptr(V), V.shape[0], ptr(F), F.shape[0], ptr(points), points.shape[0]) + tuple(extra)
    return _sized_call(V.device, name, head, out, ws_bytes)


def mesh_contains(V, F, points, hash_resolution=512):
    """libmesh.check_mesh_contains on the device: points [n,3] float64 -> bool [n] (bit-identical to the reference)."""
    V, F = _mesh_dev(V, F)
    points = points.to(torch.float64).contiguous()
    out = torch.empty(points.shape[0], dtype=torch.bool, device=V.device)
    ws_bytes = load().ls_mesh_contains_workspace_bytes(F.shape[0], int(hash_resolution))
    return _binned("ls_mesh_contains_f64", ws_bytes, V, F, points, [int(hash_resolution)], out)


def mesh_distance(V, F, points, max_dist):
    """Unsigned point-to-mesh distance under a cap: points [n,3] float64 -> float64 [n], +inf where the distance is >= max_dist."""
    V, F = _mesh_dev(V, F)
    points = points.to(torch.float64).contiguous()
    out = torch.empty(points.shape[0], dtype=torch.float64, device=V.device)
    ws_bytes = load().ls_mesh_distance_workspace_bytes(F.shape[0])
    return _binned("ls_mesh_distance_f64", ws_bytes, V, F, points, [float(max_dist)], out)


def mesh_sample(V, F, count, seed=0):
    """Area-weighted surface samples (trimesh.sample.sample_surface's algorithm, counter-based uniforms of `seed`):
    -> points [count,3] float64, face index [count] int64."""
    V, F = _mesh_dev(V, F)
    dev = V.device
    pts = torch.empty(int(count), 3, dtype=torch.float64, device=dev)
    face = torch.empty(int(count), dtype=torch.int64, device=dev)
    ws = _scratch(load().ls_mesh_sample_workspace_bytes(F.shape[0]), dev)
    call(dev, "ls_mesh_sample_f64", ptr(V), V.shape[0], ptr(F), F.shape[0], int(count), ctypes.c_ulonglong(int(seed) & (2 ** 64 - 1)),
         ptr(pts), ptr(face), ptr(ws), 0 if ws is None else ws.numel(), stream_ptr(dev))
    return pts, face


# ---- ragged batches of meshes (ls_mesh_*_batch_f64): one call for M meshes, every mesh's result bit-identical to the single form
def _offsets(sizes):
    """int64 host offsets [M+1] of consecutive ranges of the given sizes"""
    off = np.zeros(len(sizes) + 1, dtype=np.int64)
    np.cumsum(np.asarray(sizes, dtype=np.int64), out=off[1:])
    return off


def _pack_meshes(meshes):
    """meshes: list of (V [nv,3] float64, F [nf,3] int32) HIP tensors, indices local to each mesh -> (V, vert_off, F, face_off) packed back
    to back, with no host read.  As for the single forms, the caller range-checks the faces (evaluate._device_meshes); an index outside
    its own mesh gives what the single op gives on that mesh."""
    Vs, Fs = zip(*[_mesh_dev(V, F) for V, F in meshes]) if meshes else ((), ())
    for i, V in enumerate(Vs):
        if V.shape[0] >= 2 ** 31:
            raise ValueError(f"mesh {i} has {V.shape[0]} vertices: the mesh operators index vertices with int32 (nv < 2^31)")
    dev = Vs[0].device if Vs else torch.device("cuda", torch.cuda.current_device())
    V = torch.cat(Vs, 0) if Vs else torch.zeros(0, 3, dtype=torch.float64, device=dev)
    F = torch.cat(Fs, 0) if Fs else torch.zeros(0, 3, dtype=torch.int32, device=dev)
    return V, _offsets([v.shape[0] for v in Vs]), F, _offsets([f.shape[0] for f in Fs])


def _pack_points(points_list, M, dev):
    if len(points_list) != M:
        raise ValueError(f"{len(points_list)} point sets for {M} meshes")
    P = [p.to(device=dev, dtype=torch.float64).reshape(-1, 3) for p in points_list]
    return (torch.cat(P, 0) if P else torch.zeros(0, 3, dtype=torch.float64, device=dev)).contiguous(), _offsets([p.shape[0] for p in P])


def _hptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def _binned_batch(name, ws_bytes, meshes, points_list, extra, dtype):
    """ragged form of _binned: one sizing call (one host read) for the whole batch -> list of per-mesh outputs (views of one tensor)"""
    if not meshes:
        return []
    V, vo, F, fo = _pack_meshes(meshes)
    dev = V.device
    P, po = _pack_points(points_list, len(meshes), dev)
    out = torch.empty(P.shape[0], dtype=dtype, device=dev)
    head = (len(meshes), ptr(V), V.shape[0], _hptr(vo), ptr(F), F.shape[0], _hptr(fo), ptr(P), P.shape[0], _hptr(po)) + tuple(extra)
    _sized_call(dev, name, head, out, ws_bytes(len(meshes), F.shape[0]))
    return list(torch.split(out, np.diff(po).tolist()))


def mesh_contains_batch(meshes, points_list, hash_resolution=512):
    """mesh_contains on M meshes in one call: meshes = list of (V [nv,3] float64, F [nf,3] int32), points_list = M point sets [n,3]
    -> list of M bool tensors, element i bit-identical to mesh_contains(*meshes[i], points_list[i], hash_resolution)."""
    R = int(hash_resolution)
    return _binned_batch("ls_mesh_contains_batch_f64", lambda M, nf: load().ls_mesh_contains_batch_workspace_bytes(M, nf, R), meshes, points_list,
                         [R], torch.bool)


def mesh_distance_batch(meshes, points_list, max_dist):
    """mesh_distance on M meshes in one call (one max_dist) -> list of M float64 tensors, each bit-identical to the single form."""
    return _binned_batch("ls_mesh_distance_batch_f64", lambda M, nf: load().ls_mesh_distance_batch_workspace_bytes(M, nf), meshes, points_list,
                         [float(max_dist)], torch.float64)


def mesh_sample_batch(meshes, counts, seeds=None):
    """mesh_sample on M meshes in one call: counts = int or M ints (0 allowed), seeds = M ints (None: 0 for every mesh) -> list of M
    (points [count,3] float64, face index [count] int64 local to the mesh), each bit-identical to mesh_sample(*meshes[i], counts[i], seeds[i])."""
    M = len(meshes)
    counts = [int(counts)] * M if isinstance(counts, (int, np.integer)) else [int(c) for c in counts]
    seeds = [0] * M if seeds is None else [int(s) & (2 ** 64 - 1) for s in seeds]
    if len(counts) != M or len(seeds) != M:
        raise ValueError(f"{len(counts)} counts / {len(seeds)} seeds for {M} meshes")
    if M == 0:
        return []
    V, vo, F, fo = _pack_meshes(meshes)
    dev = V.device
    co = _offsets(counts)
    n = int(co[-1])
    pts = torch.empty(n, 3, dtype=torch.float64, device=dev)
    face = torch.empty(n, dtype=torch.int64, device=dev)
    sd = torch.tensor(np.asarray(seeds, dtype=np.uint64).view(np.int64), device=dev)
    ws = _scratch(load().ls_mesh_sample_batch_workspace_bytes(M, F.shape[0]), dev)
    call(dev, "ls_mesh_sample_batch_f64", M, ptr(V), V.shape[0], _hptr(vo), ptr(F), F.shape[0], _hptr(fo), n, _hptr(co), ptr(sd), ptr(pts),
         ptr(face), ptr(ws), 0 if ws is None else ws.numel(), stream_ptr(dev))
    return list(zip(torch.split(pts, counts), torch.split(face, counts)))


# ------------------------------------------------------------------------------------------------ depth views (csrc/meshrender.hip)
def _f64_dev(x, what, op, tail, views=None):
    """a float64 HIP tensor [views, *tail] (a single [*tail] is shared by the views when `views` is given)"""
    if not torch.is_tensor(x) or x.device.type != "cuda":
        kind = f"{x.device.type} {x.dtype}" if torch.is_tensor(x) else type(x).__name__
        raise _lib.LsError(f"{op}: {what} must be a HIP (cuda) tensor, got {kind}: the MI355X path has no CPU fallback")
    if views is not None and tuple(x.shape) == tail:
        x = x.expand((views,) + tail)
    if tuple(x.shape[1:]) != tail or (views is not None and x.shape[0] != views):
        raise ValueError(f"{op}: {what} is [views, {', '.join(map(str, tail))}]" + (f" with views = {views}" if views is not None else "") +
                         f", got {tuple(x.shape)}")
    return x.to(torch.float64).contiguous()


def _render_args(op, world_to_cam, intrinsics, height, width, znear):
    E = _f64_dev(world_to_cam, "world_to_cam", op, (3, 4))
    K = _f64_dev(intrinsics, "intrinsics", op, (4,), E.shape[0])
    H, W, znear = int(height), int(width), float(znear)
    if H < 1 or W < 1:
        raise ValueError(f"{op}: the image must have at least one pixel, got {H} x {W}")
    if E.shape[0] * H * W >= 2 ** 31:
        raise ValueError(f"{op}: {E.shape[0]} views of {H} x {W} pixels: the renderer ranks pixels with int32 (views * height * width < 2^31)")
    if not (0 < znear < float("inf")):
        raise ValueError(f"{op}: znear must be positive and finite, got {znear}")
    return E, K, H, W, znear


def _render_out(op, views, H, W, dev):
    depth = torch.empty(views, H, W, dtype=torch.float32, device=dev)
    face = torch.empty(views, H, W, dtype=torch.int32, device=dev)
    return depth, face, _Meta(1, dev, [("counts", np.int64, 0, 4 * views), ("status", np.int32, 1)])


def _render_read(op, m, views):
    """the call's one host read: the counts; a face that names a vertex outside its mesh is an error of the call"""
    host = m.buf.cpu().numpy().view(np.uint8)
    o = m.at["status"][0]
    if host[o:o + 4].view(np.int32)[0] != 0:
        raise _lib.LsError(f"{op}: a face names a vertex outside its mesh")
    return torch.from_numpy(host[:views * 32].view(np.int64).reshape(views, 4).copy())


def mesh_render_depth(V, F, world_to_cam, intrinsics, height, width, znear=0.05):
    """ls_mesh_render_depth_f64: depth views of one mesh (V [nv,3] float64, F [nf,3] int32, HIP tensors).  world_to_cam [views,3,4] float64
    takes world points into the camera frame (x right, y down, z forward), intrinsics [views,4] or [4] = (fx, fy, cx, cy), HIP tensors too.
    -> (depth [views,H,W] fp32, 0 = nothing hit; face [views,H,W] int32, -1 = none; counts [views,4] int64 on the HOST: pixels hit, faces
    that reached the pixel box with a non-zero area, faces dropped at the near test, faces dropped at the snap).  The definition is in
    include/livingscenes_hip.h; tests/render_oracle.py is the same text as NumPy and the outputs equal it bit for bit.  One host read."""
    op = "mesh_render_depth"
    V, F = _mesh_dev(V, F)
    E, K, H, W, znear = _render_args(op, world_to_cam, intrinsics, height, width, znear)
    dev, views = V.device, E.shape[0]
    depth, face, m = _render_out(op, views, H, W, dev)
    ws = _scratch(load().ls_mesh_render_depth_workspace_bytes(views, H, W), dev)
    call(dev, "ls_mesh_render_depth_f64", ptr(V), V.shape[0], ptr(F), F.shape[0], views, ptr(E), ptr(K), H, W, znear, ptr(depth), ptr(face),
         m.ptr("counts"), m.ptr("status"), ptr(ws), 0 if ws is None else ws.numel(), stream_ptr(dev))
    return depth, face, _render_read(op, m, views)


def mesh_render_depth_batch(meshes, world_to_cam, intrinsics, height, width, znear=0.05):
    """ls_mesh_render_depth_batch_f64: meshes = list of M (V, F); world_to_cam = list of M HIP tensors [views_m,3,4] (zero views allowed),
    intrinsics = [4] shared, or a list of M tensors [views_m,4] -> list of M (depth, face, counts), mesh m bit-identical to
    mesh_render_depth(*meshes[m], world_to_cam[m], ...).  One device call and one host read whatever M."""
    op = "mesh_render_depth_batch"
    M = len(meshes)
    if len(world_to_cam) != M:
        raise ValueError(f"{op}: {len(world_to_cam)} camera sets for {M} meshes")
    if M == 0:
        return []
    Vp, vo, Fp, fo = _pack_meshes(meshes)
    dev = Vp.device
    Es = [_f64_dev(e, "world_to_cam", op, (3, 4)) for e in world_to_cam]
    nviews = [e.shape[0] for e in Es]
    if torch.is_tensor(intrinsics):
        Ks = [_f64_dev(intrinsics, "intrinsics", op, (4,), n) for n in nviews]
    else:
        if len(intrinsics) != M:
            raise ValueError(f"{op}: {len(intrinsics)} intrinsics for {M} meshes")
        Ks = [_f64_dev(k, "intrinsics", op, (4,), n) for k, n in zip(intrinsics, nviews)]
    E, K, H, W, znear = _render_args(op, torch.cat(Es, 0), torch.cat(Ks, 0), height, width, znear)
    views, wo = E.shape[0], _offsets(nviews)
    depth, face, m = _render_out(op, views, H, W, dev)
    ws = _scratch(load().ls_mesh_render_depth_batch_workspace_bytes(M, views, H, W), dev)
    call(dev, "ls_mesh_render_depth_batch_f64", M, ptr(Vp), Vp.shape[0], _hptr(vo), ptr(Fp), Fp.shape[0], _hptr(fo), views, _hptr(wo), ptr(E),
         ptr(K), H, W, znear, ptr(depth), ptr(face), m.ptr("counts"), m.ptr("status"), ptr(ws), 0 if ws is None else ws.numel(), stream_ptr(dev))
    counts = _render_read(op, m, views)
    return list(zip(torch.split(depth, nviews), torch.split(face, nviews), torch.split(counts, nviews)))


def depth_points(depth, intrinsics, cam_to_world=None, packed=False):
    """ls_depth_points_f32: the back-projection of depth maps (the reference's utils/render.py pointcloud, plus the move to another frame).
    depth [views,H,W] fp32, intrinsics [views,4] or [4] float64 = (fx, fy, cx, cy), cam_to_world [views,3,4] float64 or None (the points
    stay in the camera frame: x right, y down, z forward); HIP tensors.  Per view every pixel with depth > 0 in ascending row-major order
    -> list of views (pts [n,3] fp32, pix [n] int32: the pixel index py * W + px), views of one packed tensor; packed=True: (pts, pix, off)
    with off the host int64 offsets [views+1].  One call, one host read (the offsets)."""
    op = "depth_points"
    if not torch.is_tensor(depth) or depth.device.type != "cuda" or depth.dtype != torch.float32:
        kind = f"{depth.device.type} {depth.dtype}" if torch.is_tensor(depth) else type(depth).__name__
        raise _lib.LsError(f"{op}: depth must be an fp32 HIP (cuda) tensor, got {kind}: the MI355X path has no CPU fallback and converts nothing")
    if depth.dim() != 3 or depth.shape[1] < 1 or depth.shape[2] < 1:
        raise ValueError(f"{op}: depth is [views, H, W] with at least one pixel, got {tuple(depth.shape)}")
    depth = depth.contiguous()
    dev, (views, H, W) = depth.device, depth.shape
    K = _f64_dev(intrinsics, "intrinsics", op, (4,), views)
    Mw = None if cam_to_world is None else _f64_dev(cam_to_world, "cam_to_world", op, (3, 4), views)
    n = views * H * W
    if n > 2 ** 24:
        raise ValueError(f"{op}: {views} views of {H} x {W} pixels: at most 2^24 pixels per call")
    pts = torch.empty(n, 3, dtype=torch.float32, device=dev)
    pix = torch.empty(n, dtype=torch.int32, device=dev)
    off = torch.empty(views + 1, dtype=torch.int64, device=dev)
    ws = _scratch(load().ls_depth_points_workspace_bytes(views, H, W), dev)
    call(dev, "ls_depth_points_f32", ptr(depth), views, H, W, ptr(K), ptr(Mw), ptr(pts), ptr(pix), ptr(off), ptr(ws),
         0 if ws is None else ws.numel(), stream_ptr(dev))
    off = off.cpu().numpy()
    n_out = int(off[views])
    if packed:
        return pts[:n_out], pix[:n_out], off
    sizes = np.diff(off).tolist()
    return list(zip(torch.split(pts[:n_out], sizes), torch.split(pix[:n_out], sizes)))


# ------------------------------------------------------------------------------------------------ scene memory (csrc/cloud_grid.h, cloudmerge.hip, cloudnear.hip)
# The fourteen wrappers (the carve's two, further down, included) share one binding scheme: _cloud / _pose / _poses / _per_problem check the arguments, _pack puts a list of clouds back
# to back, _Meta holds the per-problem outputs that the host reads, and _icp_result assembles what the four ICP wrappers return.
def _cloud(x, what, op):
    if not torch.is_tensor(x) or x.device.type != "cuda" or x.dtype != torch.float32:
        kind = f"{x.device.type} {x.dtype}" if torch.is_tensor(x) else type(x).__name__
        raise _lib.LsError(f"{op}: {what} must be an fp32 HIP (cuda) tensor, got {kind}: the MI355X path has no CPU fallback and converts nothing")
    if x.dim() != 2 or x.shape[1] != 3:
        raise ValueError(f"{op}: {what} is [n, 3], got {tuple(x.shape)}")
    return x.contiguous()


def _pose(g, op, dev):
    """the pose of a single problem: [3,4] or [4,4] (None stays None) -> [3,4] fp32 on dev"""
    if g is None:
        return None
    if not torch.is_tensor(g) or tuple(g.shape) not in ((3, 4), (4, 4)):
        raise ValueError(f"{op}: g must be [3,4] or [4,4], got {tuple(g.shape) if torch.is_tensor(g) else type(g).__name__}")
    return _f32(g.to(dev)[:3, :])


def _poses(g, op, P, dev):
    """the poses of a batch: [P,3,4] or [P,4,4] (None stays None) -> [P,3,4] fp32 on dev"""
    if g is None:
        return None
    if not torch.is_tensor(g) or g.dim() != 3 or g.shape[0] != P or g.shape[1] not in (3, 4) or g.shape[2] != 4:
        raise ValueError(f"{op}: g must be [P,3,4] or [P,4,4] with P = {P}, got {tuple(g.shape) if torch.is_tensor(g) else type(g).__name__}")
    return _f32(g.to(dev)[:, :3, :])


def _per_problem(v, P, op, noun):
    """one value or P values -> host fp32 [P]"""
    v = np.full(P, float(v), dtype=np.float32) if np.ndim(v) == 0 else np.ascontiguousarray(v, dtype=np.float32).reshape(-1)
    if v.shape[0] != P:
        raise ValueError(f"{op}: {v.shape[0]} {noun} for {P} problems")
    return v


def _pack(xs):
    """a list of clouds -> (the clouds back to back, host int64 offsets)"""
    return (torch.cat(xs, 0) if len(xs) > 1 else xs[0]), _offsets([x.shape[0] for x in xs])


def _pairs(op, As, Bs, g, edge, observations="observations", edges="radii"):
    """the argument checks and the packing of a ragged batch of (kept cloud, observation) problems -> (P, dev, A, a_off, B, b_off, edges, g)"""
    As, Bs = [_cloud(x, "A", op) for x in As], [_cloud(x, "B", op) for x in Bs]
    P = len(As)
    if len(Bs) != P:
        raise ValueError(f"{op}: {P} kept clouds for {len(Bs)} {observations}")
    if P == 0:
        raise ValueError(f"{op}: no problem given")
    dev = As[0].device
    edge = _per_problem(edge, P, op, edges)
    g = _poses(g, op, P, dev)
    return (P, dev) + _pack(As) + _pack(Bs) + (edge, g)


class _Meta:
    """The per-problem outputs of a call that the host reads, packed into ONE int64 device tensor -- one host read per call.  fields:
    (name, dtype, entries per problem[, further entries]) in their order in the tensor, the 8-byte ones first."""

    def __init__(self, P, dev, fields):
        self.P, self.at, n = P, {}, 0
        for name, dtype, per, *more in fields:
            count = per * P + sum(more)
            self.at[name] = (n, np.dtype(dtype), count, per)
            n += count * np.dtype(dtype).itemsize
        self.buf = torch.empty((n + 7) // 8, dtype=torch.int64, device=dev)

    def ptr(self, name):
        return ctypes.c_void_p(self.buf.data_ptr() + self.at[name][0])

    def read(self, op, name_problem=True):
        """the host read -> {name: array [P] or [P, per]}; raises on a status that is not LS_OK"""
        host = self.buf.cpu().numpy().view(np.uint8)
        out = {}
        for name, (o, dtype, count, per) in self.at.items():
            v = host[o:o + count * dtype.itemsize].view(dtype).copy()
            out[name] = v.reshape(self.P, per) if per > 1 else v
        st = out.pop("status")
        if st.any():
            p = int(np.flatnonzero(st)[0])
            raise _lib.LsError(f"{op}: " + (f"problem {p}: " if name_problem else "") + f"status {int(st[p])} (the cell table overflowed: a defect)")
        return out


def _cloud_call(dev, name, sizes, *args):
    """the entry `name` with the scratch that its size query asks for at `sizes`: every entry ends in (workspace, bytes, stream)"""
    ws = _scratch(getattr(load(), name.replace("_f32", "_workspace_bytes"))(*sizes), dev)
    call(dev, name, *args, ptr(ws), 0 if ws is None else ws.numel(), stream_ptr(dev))


def cloud_merge_batch(As, Bs, g=None, *, voxel, packed=False):
    """ls_cloud_merge_batch_f32: As / Bs = lists of P kept clouds [a_p,3] and new observations [b_p,3] (fp32 HIP tensors, empty ones allowed),
    g [P,3,4] or [P,4,4] taking B_p into A_p's frame (None: identity, B bit for bit), voxel = one edge or P edges.  Candidates are A_p's rows then
    B_p's transformed rows; one is kept iff no earlier candidate of its problem lies in the same voxel (include/livingscenes_hip.h)
    -> list of P (pts [n_p,3], src [n_p] int32: the candidate index, >= a_p: from B), views of one packed tensor; packed=True: (pts, src, off)
    with off the host int64 offsets [P+1].  One call, one host read (the offsets), whatever P."""
    P, dev, A, ao, B, bo, vox, g = _pairs("cloud_merge", As, Bs, g, voxel, "new observations", "voxel edges")
    n = A.shape[0] + B.shape[0]
    pts = torch.empty(n, 3, dtype=torch.float32, device=dev)
    src = torch.empty(n, dtype=torch.int32, device=dev)
    m = _Meta(P, dev, [("off", np.int64, 1, 1), ("status", np.int32, 1)])
    _cloud_call(dev, "ls_cloud_merge_batch_f32", (P, A.shape[0], B.shape[0]), P, ptr(A), A.shape[0], _hptr(ao), ptr(B), B.shape[0], _hptr(bo),
                ptr(g), _hptr(vox), ptr(pts), ptr(src), m.ptr("off"), m.ptr("status"))
    off = m.read("cloud_merge")["off"]
    n_out = int(off[P])
    if packed:
        return pts[:n_out], src[:n_out], off
    sizes = np.diff(off).tolist()
    return list(zip(torch.split(pts[:n_out], sizes), torch.split(src[:n_out], sizes)))


def cloud_merge(A, B, g=None, *, voxel):
    """ls_cloud_merge_f32: the kept cloud A [a,3] and the new observation B [b,3] (fp32 HIP tensors), g [3,4] or [4,4] taking B into A's
    frame (None: identity) -> (pts [n,3], src [n] int32): A's rows, then B's transformed rows, each kept iff no earlier one lies in the same
    voxel of edge `voxel`.  Bit-identical to the same problem inside any cloud_merge_batch."""
    op = "cloud_merge"
    A, B = _cloud(A, "A", op), _cloud(B, "B", op)
    dev = A.device
    g = _pose(g, op, dev)
    n = A.shape[0] + B.shape[0]
    pts = torch.empty(n, 3, dtype=torch.float32, device=dev)
    src = torch.empty(n, dtype=torch.int32, device=dev)
    m = _Meta(1, dev, [("off", np.int64, 1, 1), ("status", np.int32, 1)])
    _cloud_call(dev, "ls_cloud_merge_f32", (A.shape[0], B.shape[0]), ptr(A), A.shape[0], ptr(B), B.shape[0], ptr(g), float(voxel), ptr(pts),
                ptr(src), m.ptr("off"), m.ptr("status"))
    n_out = int(m.read(op, name_problem=False)["off"][1])
    return pts[:n_out], src[:n_out]


_NEAR_META = [("counts", np.int64, 3), ("sum_d2", np.float64, 1), ("status", np.int32, 1)]


def cloud_nearest_batch(As, Bs, g=None, *, radius, packed=False):
    """ls_cloud_nearest_batch_f32: As / Bs = lists of P kept clouds [a_p,3] (targets) and observations [b_p,3] (queries; fp32 HIP tensors,
    empty ones allowed), g [P,3,4] or [P,4,4] taking B_p into A_p's frame (None: identity, B bit for bit), radius = one radius or P radii.
    The neighbour of a query is the target within `radius` -- and within one cell of edge `radius` on every axis -- that is least under
    (d2, index) (include/livingscenes_hip.h) -> list of P (idx [b_p] int32: the row of A_p, -1 for none; d2 [b_p] fp32, +inf for none;
    counts: host int64 [3] = finite queries, queries with a neighbour, targets that are somebody's neighbour; sum_d2: float, the float64 sum
    of the finite d2), idx / d2 views of one packed tensor; packed=True: (idx, d2, counts [P,3], sum_d2 [P], b_off) with the host int64
    query offsets [P+1].  One call, one host read (counts, sums and status), whatever P."""
    P, dev, A, ao, B, bo, rad, g = _pairs("cloud_nearest", As, Bs, g, radius)
    idx = torch.empty(B.shape[0], dtype=torch.int32, device=dev)
    d2 = torch.empty(B.shape[0], dtype=torch.float32, device=dev)
    m = _Meta(P, dev, _NEAR_META)
    _cloud_call(dev, "ls_cloud_nearest_batch_f32", (P, A.shape[0], B.shape[0]), P, ptr(A), A.shape[0], _hptr(ao), ptr(B), B.shape[0], _hptr(bo),
                ptr(g), _hptr(rad), ptr(idx), ptr(d2), m.ptr("counts"), m.ptr("sum_d2"), m.ptr("status"))
    f = m.read("cloud_nearest")
    if packed:
        return idx, d2, f["counts"], f["sum_d2"], bo
    sizes = np.diff(bo).tolist()
    return [(i, d, f["counts"][p], float(f["sum_d2"][p])) for p, (i, d) in enumerate(zip(torch.split(idx, sizes), torch.split(d2, sizes)))]


def cloud_nearest(A, B, g=None, *, radius):
    """ls_cloud_nearest_f32: the kept cloud A [a,3] (targets) and the observation B [b,3] (queries; fp32 HIP tensors), g [3,4] or [4,4]
    taking B into A's frame (None: identity) -> (idx [b] int32, d2 [b] fp32, counts host int64 [3], sum_d2 float) as cloud_nearest_batch
    describes them.  Bit-identical to the same problem inside any cloud_nearest_batch."""
    op = "cloud_nearest"
    A, B = _cloud(A, "A", op), _cloud(B, "B", op)
    dev = A.device
    g = _pose(g, op, dev)
    idx = torch.empty(B.shape[0], dtype=torch.int32, device=dev)
    d2 = torch.empty(B.shape[0], dtype=torch.float32, device=dev)
    m = _Meta(1, dev, _NEAR_META)
    _cloud_call(dev, "ls_cloud_nearest_f32", (A.shape[0], B.shape[0]), ptr(A), A.shape[0], ptr(B), B.shape[0], ptr(g), float(radius), ptr(idx),
                ptr(d2), m.ptr("counts"), m.ptr("sum_d2"), m.ptr("status"))
    f = m.read(op)
    return idx, d2, f["counts"][0], float(f["sum_d2"][0])


# ------------------------------------------------------------------------------------------------ scene memory: trimmed ICP on the search's grid
ICP_STOP = ("converged", "max_iter", "starved", "degenerate")   # LS_ICP_* of include/livingscenes_hip.h, by value


_PLANE_META = [("planar", np.int64, 1), ("sum_rho2", np.float64, 1)]
_ICP_SCALARS = {"stop": int, "iters": int, "sum_d2": float, "planar": int, "sum_rho2": float}   # what a per-problem dict holds as Python numbers


def _icp_result(out, bo, traces, packed):
    """what an ICP wrapper returns, for either metric.  out: the packed outputs by name, device tensors and host arrays [P, ...];
    packed: `out` with b_off (and the traces) -> else the list of P dicts, idx / d2 split at the query offsets bo."""
    if packed:
        out["b_off"] = bo
    out.update(traces)
    if packed:
        return out
    sizes = np.diff(bo).tolist()
    out["idx"], out["d2"] = torch.split(out["idx"], sizes), torch.split(out["d2"], sizes)
    return [{k: _ICP_SCALARS[k](v[p]) if k in _ICP_SCALARS else v[p] for k, v in out.items()} for p in range(len(sizes))]


def _icp(op, name, head, sizes, P, dev, bo, max_iter, rel_thr, min_matched, trace, packed, plane=False):
    """The call of the ICP entry `name` of the operator `op`.  head: the entry's arguments up to the radius, sizes: those of its size query,
    bo: the host offsets of the queries; plane: the point-to-plane metric, with planar / sum_rho2 and five columns of statistics."""
    max_iter, b = int(max_iter), int(bo[-1])
    idx = torch.empty(b, dtype=torch.int32, device=dev)
    d2 = torch.empty(b, dtype=torch.float32, device=dev)
    g_out = torch.empty(P, 3, 4, dtype=torch.float32, device=dev)
    traces = {}
    if trace:
        traces = {"g_trace": torch.zeros(P, max(max_iter, 0) + 1, 12, dtype=torch.float32, device=dev),
                  "stat_trace": torch.zeros(P, max(max_iter, 0) + 1, 5 if plane else 3, dtype=torch.float64, device=dev)}
    extra = _PLANE_META if plane else []
    m = _Meta(P, dev, _NEAR_META[:2] + extra + [("status", np.int32, 1), ("stop", np.int32, 1), ("iters", np.int32, 1)])
    _cloud_call(dev, name, sizes, *head, max_iter, float(rel_thr), int(min_matched), ptr(g_out), m.ptr("stop"), m.ptr("iters"), ptr(idx), ptr(d2),
                m.ptr("counts"), m.ptr("sum_d2"), *[m.ptr(k) for k, _, _ in extra], m.ptr("status"), ptr(traces.get("g_trace")),
                ptr(traces.get("stat_trace")))
    f = m.read(op)
    out = {"g": g_out, "stop": f["stop"], "iters": f["iters"], "idx": idx, "d2": d2, "counts": f["counts"], "sum_d2": f["sum_d2"]}
    out.update({k: f[k] for k, _, _ in extra})
    return _icp_result(out, bo, traces, packed)


def cloud_icp_batch(As, Bs, g=None, *, radius, max_iter=100, rel_thr=1e-6, min_matched=3, trace=False, packed=False):
    """ls_cloud_icp_batch_f32 (an extension beyond the released reference, like cloud_merge and cloud_nearest): trimmed ICP of P observations
    Bs[p] [b_p,3] onto the kept clouds As[p] [a_p,3] on cloud_nearest's grid, at full resolution.  g [P,3,4] or [P,4,4] is the initial pose
    taking B_p into A_p's frame (None: the identity), radius = one radius or P radii: only correspondences within it count, so the part of
    A_p the observation does not see pulls on nothing.  Per iteration: cloud_nearest under the current pose, the truncated-quadratic cost
    E = (sum d2 + unmatched r^2) / finite, the stop tests (fewer than min_matched matches: starved; E fell by <= rel_thr E: converged;
    max_iter updates made), else a float64 Kabsch update from the matched pairs (include/livingscenes_hip.h has the definition to the bit).
    max_iter = 100 and rel_thr = 1e-6 are the defaults of ops.icp, which are pytorch3d's: INHERITED, NOT TUNED.
    -> list of P dicts: g [3,4] fp32 (device), stop (int, LS_ICP_*; ICP_STOP names them), iters (int), and the final search exactly as
    cloud_nearest(A_p, B_p, g, radius) returns it: idx, d2, counts (host int64 [3]), sum_d2 (float); trace=True adds g_trace
    [max_iter+1,12] and stat_trace [max_iter+1,3] float64 = (finite, matched, sum d2) per iteration (device; rows <= iters are written).
    packed=True: one dict of the packed tensors (g [P,3,4], stop / iters int32 [P], counts [P,3], sum_d2 [P], ...) plus b_off.  One call,
    one host read (counts, sums, status, stop, iters), whatever P and however many iterations."""
    op = "cloud_icp"
    P, dev, A, ao, B, bo, rad, g = _pairs(op, As, Bs, g, radius)
    head = (P, ptr(A), A.shape[0], _hptr(ao), ptr(B), B.shape[0], _hptr(bo), ptr(g), _hptr(rad))
    return _icp(op, "ls_cloud_icp_batch_f32", head, (P, A.shape[0], B.shape[0]), P, dev, bo, max_iter, rel_thr, min_matched, trace, packed)


def cloud_icp(A, B, g=None, *, radius, max_iter=100, rel_thr=1e-6, min_matched=3, trace=False):
    """ls_cloud_icp_f32: trimmed ICP of the observation B [b,3] onto the kept cloud A [a,3] (fp32 HIP tensors), g [3,4] or [4,4] the initial
    pose taking B into A's frame (None: identity) -> the dict cloud_icp_batch describes.  max_iter = 100 and rel_thr = 1e-6 are ops.icp's
    defaults, pytorch3d's: inherited, not tuned.  Bit-identical to the same problem inside any cloud_icp_batch."""
    op = "cloud_icp"
    A, B = _cloud(A, "A", op), _cloud(B, "B", op)
    dev = A.device
    g = _pose(g, op, dev)
    head = (ptr(A), A.shape[0], ptr(B), B.shape[0], ptr(g), float(radius))
    return _icp(op, "ls_cloud_icp_f32", head, (A.shape[0], B.shape[0]), 1, dev, _offsets([B.shape[0]]), max_iter, rel_thr, min_matched, trace, False)[0]


# ------------------------------------------------------------------------------------------------ scene memory: normals and the point-to-plane ICP
def _normals(op, name, head, sizes, P, dev, a):
    """the call of the normals' entry `name` of the operator `op` -> (normals, nbr_cnt, variation, counts [P,2])"""
    normals = torch.empty(a, 3, dtype=torch.float32, device=dev)
    cnt = torch.empty(a, dtype=torch.int32, device=dev)
    var = torch.empty(a, dtype=torch.float32, device=dev)
    m = _Meta(P, dev, [("counts", np.int64, 2), ("status", np.int32, 1)])
    _cloud_call(dev, name, sizes, *head, ptr(normals), ptr(cnt), ptr(var), m.ptr("counts"), m.ptr("status"))
    return normals, cnt, var, m.read(op)["counts"]


def cloud_normals_batch(As, *, radius, min_nbrs=5, packed=False):
    """ls_cloud_normals_batch_f32 (an extension beyond the released reference, like cloud_merge, cloud_nearest and cloud_icp): a normal per
    row of the P kept clouds As[p] [a_p,3] (fp32 HIP tensors, empty ones allowed) from the rows within `radius` of it (one radius or P
    radii) on cloud_nearest's grid: integer moments of the neighbours' offsets, the covariance and its eigenvalues in float64
    (include/livingscenes_hip.h has the definition to the bit).  A row is valid iff it has at least min_nbrs neighbours (itself included)
    and they are neither coincident nor collinear; min_nbrs = 5 IS NOT TUNED -- the rank rule does the real work.
    -> list of P (normals [a_p,3] fp32: unit, the component of largest magnitude positive, (0, 0, 0) for an invalid row; nbr_cnt [a_p]
    int32; variation [a_p] fp32 = lmin / (lmin + lmid + lmax); counts: host int64 [2] = rows with a cell, valid rows), views of packed
    tensors; packed=True: (normals, nbr_cnt, variation, counts [P,2], a_off).  One call, one host read, whatever P."""
    op = "cloud_normals"
    As = [_cloud(x, "A", op) for x in As]
    P = len(As)
    if P == 0:
        raise ValueError(f"{op}: no problem given")
    dev = As[0].device
    rad = _per_problem(radius, P, op, "radii")
    A, ao = _pack(As)
    normals, cnt, var, counts = _normals(op, "ls_cloud_normals_batch_f32", (P, ptr(A), A.shape[0], _hptr(ao), _hptr(rad), int(min_nbrs)),
                                         (P, A.shape[0]), P, dev, A.shape[0])
    if packed:
        return normals, cnt, var, counts, ao
    sizes = np.diff(ao).tolist()
    return [(n, c, v, counts[p]) for p, (n, c, v) in enumerate(zip(torch.split(normals, sizes), torch.split(cnt, sizes), torch.split(var, sizes)))]


def cloud_normals(A, *, radius, min_nbrs=5):
    """ls_cloud_normals_f32: the kept cloud A [a,3] (fp32 HIP tensor) -> (normals [a,3] fp32, nbr_cnt [a] int32, variation [a] fp32, counts
    host int64 [2]) as cloud_normals_batch describes them (min_nbrs = 5 is not tuned).  Bit-identical to the same problem inside any
    cloud_normals_batch."""
    op = "cloud_normals"
    A = _cloud(A, "A", op)
    normals, cnt, var, counts = _normals(op, "ls_cloud_normals_f32", (ptr(A), A.shape[0], float(radius), int(min_nbrs)), (A.shape[0],), 1,
                                         A.device, A.shape[0])
    return normals, cnt, var, counts[0]


def _project(op, name, head, sizes, P, dev, a):
    """the call of the projection's entry `name` of the operator `op` -> (points, state, shift, counts [P,4], sum_shift2 [P])"""
    pts = torch.empty(a, 3, dtype=torch.float32, device=dev)
    state = torch.empty(a, dtype=torch.int32, device=dev)
    shift = torch.empty(a, dtype=torch.float32, device=dev)
    m = _Meta(P, dev, [("counts", np.int64, 4), ("sum_shift2", np.float64, 1), ("status", np.int32, 1)])
    _cloud_call(dev, name, sizes, *head, ptr(pts), ptr(state), ptr(shift), m.ptr("counts"), m.ptr("sum_shift2"), m.ptr("status"))
    f = m.read(op)
    return pts, state, shift, f["counts"], f["sum_shift2"]


PROJECT_STATE = ("no_cell", "no_plane", "held", "moved")   # the values of `state`, by value


def cloud_project_batch(As, *, radius, min_nbrs=5, max_variation=1 / 3, max_shift=float("inf"), packed=False):
    """ls_cloud_project_batch_f32 (an extension beyond the released reference, like cloud_normals, whose neighbourhood it uses): ONE
    projection of every row of the P kept clouds As[p] [a_p,3] (fp32 HIP tensors, empty ones allowed) onto the plane through the centroid
    of the rows within `radius` of it (one radius or P radii), normal to the eigenvector of the least eigenvalue of their covariance:
    integer moments, the rest in float64 (include/livingscenes_hip.h has the definition to the bit).  Every row is projected from the
    input positions; the inputs are not written.  A row whose neighbourhood has no plane (fewer than min_nbrs rows, coincident, collinear)
    stays; so does one with variation = lmin / (lmin + lmid + lmax) > max_variation (an edge or a corner) or a distance to its plane >
    max_shift.  max_variation = 1/3 IS "NO LIMIT", because variation <= 1/3 by construction, and max_shift = inf is no limit either: NO
    VALUE OF EITHER IS RECOMMENDED, none has been measured on real scans.  min_nbrs = 5 is cloud_normals': not tuned.
    -> list of P (points [a_p,3] fp32; state [a_p] int32: 0 no cell, 1 no plane, 2 held, 3 moved (PROJECT_STATE names them); shift [a_p]
    fp32: the distance to the plane, 0 in states 0 and 1; counts: host int64 [4] = rows per state; sum_shift2: float, the float64 sum of
    the squared distances of the moved rows), views of packed tensors; packed=True: (points, state, shift, counts [P,4], sum_shift2 [P],
    a_off).  One call, one host read, whatever P."""
    op = "cloud_project"
    As = [_cloud(x, "A", op) for x in As]
    P = len(As)
    if P == 0:
        raise ValueError(f"{op}: no problem given")
    dev = As[0].device
    rad = _per_problem(radius, P, op, "radii")
    A, ao = _pack(As)
    pts, state, shift, counts, sums = _project(op, "ls_cloud_project_batch_f32", (P, ptr(A), A.shape[0], _hptr(ao), _hptr(rad), int(min_nbrs),
                                                                                 float(max_variation), float(max_shift)),
                                               (P, A.shape[0]), P, dev, A.shape[0])
    if packed:
        return pts, state, shift, counts, sums, ao
    sizes = np.diff(ao).tolist()
    return [(x, s, d, counts[p], float(sums[p]))
            for p, (x, s, d) in enumerate(zip(torch.split(pts, sizes), torch.split(state, sizes), torch.split(shift, sizes)))]


def cloud_project(A, *, radius, min_nbrs=5, max_variation=1 / 3, max_shift=float("inf")):
    """ls_cloud_project_f32: the kept cloud A [a,3] (fp32 HIP tensor) -> (points [a,3] fp32, state [a] int32, shift [a] fp32, counts host
    int64 [4], sum_shift2 float) as cloud_project_batch describes them (max_variation = 1/3 is "no limit": by construction
    variation <= 1/3; min_nbrs = 5 is not tuned).  Bit-identical to the same problem inside any cloud_project_batch."""
    op = "cloud_project"
    A = _cloud(A, "A", op)
    pts, state, shift, counts, sums = _project(op, "ls_cloud_project_f32", (ptr(A), A.shape[0], float(radius), int(min_nbrs), float(max_variation),
                                                                           float(max_shift)), (A.shape[0],), 1, A.device, A.shape[0])
    return pts, state, shift, counts[0], float(sums[0])


# ------------------------------------------------------------------------------------------------ scene memory: carving by depth views (csrc/cloudcarve.hip)
CARVE_STATE = ("out", "seen", "free", "occluded", "mixed")   # the values of `state`, by value
_CARVE_EMPTY = {"unknown": 0, "free": 1}


def _carve_views(op, depth, intrinsics, world_to_cam, dev):
    """the views of one problem: depth [V,H,W] fp32, intrinsics [V,4] or [4] and world_to_cam [V,3,4] float64, HIP tensors on dev"""
    if not torch.is_tensor(depth) or depth.device.type != "cuda" or depth.dtype != torch.float32:
        kind = f"{depth.device.type} {depth.dtype}" if torch.is_tensor(depth) else type(depth).__name__
        raise _lib.LsError(f"{op}: depth must be an fp32 HIP (cuda) tensor, got {kind}: the MI355X path has no CPU fallback and converts nothing")
    if depth.dim() != 3 or depth.shape[1] < 1 or depth.shape[2] < 1:
        raise ValueError(f"{op}: depth is [views, H, W] with at least one pixel, got {tuple(depth.shape)}")
    if depth.device != dev:
        raise ValueError(f"{op}: depth is on {depth.device}, the kept cloud on {dev}")
    V = depth.shape[0]
    return depth.contiguous(), _f64_dev(intrinsics, "intrinsics", op, (4,), V), _f64_dev(world_to_cam, "world_to_cam", op, (3, 4), V)


def _carve_scalars(op, tol, znear, window, min_free, max_seen, empty):
    if empty not in _CARVE_EMPTY:
        raise ValueError(f"{op}: empty must be 'unknown' or 'free', got {empty!r}")
    return float(tol), float(znear), int(window), int(min_free), int(max_seen), _CARVE_EMPTY[empty]


def _carve(op, name, head, sizes, scalars, P, dev, a, views, n_state):
    """the call of the carve's entry `name` of the operator `op` -> (pts, src, off [P+1], dict of seen, free, counts [P,4], view_counts
    [views,5] and state (device uint8, or None))"""
    pts = torch.empty(a, 3, dtype=torch.float32, device=dev)
    src = torch.empty(a, dtype=torch.int32, device=dev)
    seen = torch.empty(a, dtype=torch.int32, device=dev)
    free = torch.empty(a, dtype=torch.int32, device=dev)
    state = None if n_state is None else torch.empty(n_state, dtype=torch.uint8, device=dev)
    m = _Meta(P, dev, [("off", np.int64, 1, 1), ("counts", np.int64, 4), ("view_counts", np.int64, 0, 5 * views), ("status", np.int32, 1)])
    _cloud_call(dev, name, sizes, *head, *scalars, ptr(pts), ptr(src), m.ptr("off"), ptr(seen), ptr(free), m.ptr("counts"), m.ptr("view_counts"),
                ptr(state), m.ptr("status"))
    f = m.read(op)
    n_out = int(f["off"][P])
    return pts[:n_out], src[:n_out], f["off"], {"seen": seen, "free": free, "counts": f["counts"].reshape(P, 4),
                                                 "view_counts": f["view_counts"].reshape(views, 5), "state": state}


def cloud_carve_batch(As, depths, intrinsics, world_to_cam, *, tol, window=1, min_free=1, max_seen=0, empty="unknown", znear=0.05,
                      return_state=False, packed=False):
    """ls_cloud_carve_batch_f32 (an extension beyond the released reference, like cloud_merge; the one operator of the scene memory that
    REMOVES points): As = list of P kept clouds [a_p,3] (fp32 HIP tensors, empty ones allowed); depths / intrinsics / world_to_cam =
    lists of P: depth views [V_p,H,W] fp32 (0 = the ray hit nothing; one H x W per call, V_p = 0 allowed), intrinsics [V_p,4] or [4]
    float64 = (fx, fy, cx, cy), world_to_cam [V_p,3,4] float64 FROM THE FRAME OF As[p] (composing a camera with a registration is the
    caller's work).  Per (row, view) the see-through test of include/livingscenes_hip.h: the row's ray is rounded to its nearest pixel,
    and over the (2 window + 1)^2 pixels around it the row is seen (within tol of some depth), free (in front of every depth by more
    than tol; empty="free": pixels that hit nothing count as looked through too, "unknown": they do not), occluded, mixed, or out of
    the view.  A row is dropped iff at least min_free views look through it and at most max_seen views see it.  window = 1 is DERIVED
    (the rounding moves the ray by up to half a pixel); tol HAS NO DEFAULT AND NONE IS RECOMMENDED, nor any min_free or max_seen: none
    has been measured on real scans.
    -> (list of P (pts [n_p,3]: the kept rows in order, the same bits; src [n_p] int32: their rows in As[p]), views of one packed tensor,
        dict: seen / free = lists of P int32 [a_p] (views per row in those states), counts host int64 [P,4] = rows seen at least once,
        rows free at least once, rows dropped, rows out of every view; view_counts = list of P host int64 [V_p,5], the rows per state
        (CARVE_STATE names them); return_state=True: state = list of P uint8 [V_p,a_p]).
    packed=True: (pts, src, off) with the host int64 offsets [P+1], and the dict's entries packed (state: the blocks back to back, flat)
    plus a_off and view_off.  One call, one host read, whatever P and however many views."""
    op = "cloud_carve"
    As = [_cloud(x, "A", op) for x in As]
    P = len(As)
    if P == 0:
        raise ValueError(f"{op}: no problem given")
    if not (len(depths) == len(world_to_cam) == P) or (not torch.is_tensor(intrinsics) and len(intrinsics) != P):
        raise ValueError(f"{op}: {P} kept clouds for {len(depths)} sets of depth views and {len(world_to_cam)} sets of cameras")
    dev = As[0].device
    Ks = [intrinsics] * P if torch.is_tensor(intrinsics) else list(intrinsics)
    vw = [_carve_views(op, d, k, e, dev) for d, k, e in zip(depths, Ks, world_to_cam)]
    if len({tuple(d.shape[1:]) for d, _, _ in vw}) != 1:
        raise ValueError(f"{op}: one H x W per call, got {sorted({tuple(d.shape[1:]) for d, _, _ in vw})}")
    scalars = _carve_scalars(op, tol, znear, window, min_free, max_seen, empty)
    A, ao = _pack(As)
    D, K, E = (torch.cat(t, 0) if P > 1 else t[0] for t in zip(*vw))
    nviews = [d.shape[0] for d, _, _ in vw]
    vo = _offsets(nviews)
    views, (H, W) = D.shape[0], D.shape[1:]
    n_state = sum(a.shape[0] * v for a, v in zip(As, nviews)) if return_state else None
    pts, src, off, f = _carve(op, "ls_cloud_carve_batch_f32", (P, ptr(A), A.shape[0], _hptr(ao), ptr(D), views, _hptr(vo), H, W, ptr(K), ptr(E)),
                              (P, A.shape[0], views), scalars, P, dev, A.shape[0], views, n_state)
    if packed:
        f.update({"a_off": ao, "view_off": vo})
        return pts, src, off, f
    rows = np.diff(ao).tolist()
    f["seen"], f["free"] = list(torch.split(f["seen"], rows)), list(torch.split(f["free"], rows))
    f["view_counts"] = [f["view_counts"][vo[p]:vo[p + 1]] for p in range(P)]
    if return_state:
        f["state"] = [s.reshape(v, a) for s, v, a in zip(torch.split(f["state"], [a * v for a, v in zip(rows, nviews)]), nviews, rows)]
    else:
        del f["state"]
    sizes = np.diff(off).tolist()
    return list(zip(torch.split(pts, sizes), torch.split(src, sizes))), f


def cloud_carve(A, depth, intrinsics, world_to_cam, *, tol, window=1, min_free=1, max_seen=0, empty="unknown", znear=0.05, return_state=False):
    """ls_cloud_carve_f32: the kept cloud A [a,3] (fp32 HIP tensor) carved by the depth views depth [V,H,W] fp32 with intrinsics [V,4] or
    [4] and world_to_cam [V,3,4] float64 from A's frame -> (pts [n,3], src [n] int32, dict: seen / free int32 [a], counts host int64 [4],
    view_counts host int64 [V,5]; return_state=True: state uint8 [V,a]) as cloud_carve_batch describes them (window = 1 is derived; no tol,
    min_free or max_seen is recommended).  Bit-identical to the same problem inside any cloud_carve_batch."""
    op = "cloud_carve"
    A = _cloud(A, "A", op)
    dev = A.device
    D, K, E = _carve_views(op, depth, intrinsics, world_to_cam, dev)
    scalars = _carve_scalars(op, tol, znear, window, min_free, max_seen, empty)
    a, (views, H, W) = A.shape[0], D.shape
    pts, src, _, f = _carve(op, "ls_cloud_carve_f32", (ptr(A), a, ptr(D), views, H, W, ptr(K), ptr(E)), (a, views), scalars, 1, dev, a, views,
                            a * views if return_state else None)
    f["counts"] = f["counts"][0]
    if return_state:
        f["state"] = f["state"].reshape(views, a)
    else:
        del f["state"]
    return pts, src, f


# ------------------------------------------------------------------------------------------------ depth fusion (csrc/depthfuse.hip)
FUSE_CLASS = ("out", "empty", "occluded", "near", "free", "saturated")   # the columns of view_counts, by value


def tsdf_state(P, dims, device="cuda"):
    """a fresh fusion state for P problems: (sum, n), int32 zeros [P,nx,ny,nz] on `device` (ls_depth_fuse_f32 updates them in place)"""
    P, dims = int(P), tuple(int(d) for d in dims)
    if P < 1 or len(dims) != 3 or min(dims) < 1 or P * dims[0] * dims[1] * dims[2] >= 2 ** 31:
        raise ValueError(f"tsdf_state: P >= 1 problems of dims (nx, ny, nz) >= 1 with P * nx * ny * nz < 2^31, got P = {P}, dims = {dims}")
    return tuple(torch.zeros((P,) + dims, dtype=torch.int32, device=device) for _ in range(2))


def _fuse_state(op, state, batch):
    """state = (sum, n): int32 HIP tensors of one shape, [P,nx,ny,nz] (batch) or [nx,ny,nz] -> (sum, n, P, dims); nothing is copied"""
    if not isinstance(state, (tuple, list)) or len(state) != 2:
        raise ValueError(f"{op}: state is the pair (sum, n) that tsdf_state returns")
    for name, t in zip(("state sum", "state n"), state):
        if not torch.is_tensor(t) or t.device.type != "cuda" or t.dtype != torch.int32:
            kind = f"{t.device.type} {t.dtype}" if torch.is_tensor(t) else type(t).__name__
            raise _lib.LsError(f"{op}: {name} must be an int32 HIP (cuda) tensor, got {kind}: the MI355X path has no CPU fallback and converts nothing")
        if t.dim() != (4 if batch else 3) or t.numel() == 0:
            raise ValueError(f"{op}: {name} is {'[P,nx,ny,nz]' if batch else '[nx,ny,nz]'}, got {tuple(t.shape)}")
        if not t.is_contiguous():
            raise ValueError(f"{op}: {name} must be contiguous: it is updated in place")
    S, N = state
    if S.shape != N.shape or S.device != N.device:
        raise ValueError(f"{op}: state sum is {tuple(S.shape)} on {S.device}, state n {tuple(N.shape)} on {N.device}")
    return S, N, (S.shape[0] if batch else 1), tuple(S.shape[-3:])


def _fuse_grid(op, P, origin, voxel, trunc=None):
    """origin [P,3] (or [3]), voxel and trunc one value or P -> host float64 arrays [P,3], [P], [P]"""
    o = torch.as_tensor(origin).detach().cpu().numpy() if torch.is_tensor(origin) else np.asarray(origin)
    o = np.ascontiguousarray(o, dtype=np.float64)
    if o.shape == (3,):
        o = np.ascontiguousarray(np.broadcast_to(o, (P, 3)))
    if o.shape != (P, 3):
        raise ValueError(f"{op}: origin is [P,3] with P = {P}, got {o.shape}")
    out = [o]
    for name, v in (("voxel", voxel), ("trunc", trunc)):
        if v is None:
            continue
        v = v.detach().cpu().numpy() if torch.is_tensor(v) else v
        v = np.full(P, float(v), dtype=np.float64) if np.ndim(v) == 0 else np.ascontiguousarray(v, dtype=np.float64).reshape(-1)
        if v.shape[0] != P:
            raise ValueError(f"{op}: {v.shape[0]} values of {name} for {P} problems")
        out.append(v)
    return out


def _fuse_empty(op, empty):
    if empty not in _CARVE_EMPTY:
        raise ValueError(f"{op}: empty must be 'unknown' or 'free', got {empty!r}")
    return _CARVE_EMPTY[empty]


def depth_fuse_batch(state, depths, intrinsics, world_to_cam, *, origin, voxel, trunc, empty="unknown", znear=0.05):
    """ls_depth_fuse_batch_f32 (an extension beyond the released reference, like cloud_carve): posed depth views fused into the truncated
    signed distance state of P instances IN PLACE.  state = (sum, n) int32 HIP tensors [P,nx,ny,nz] (tsdf_state); depths / intrinsics /
    world_to_cam = lists of P: depth views [V_p,H,W] fp32 (0 = the ray hit nothing; one H x W per call; V_p = 0 or None: the problem is
    left as it is), intrinsics [V_p,4] or [4] float64, world_to_cam [V_p,3,4] float64 FROM THE GRID'S FRAME; origin [P,3] (the centre
    of voxel (0,0,0)), voxel and trunc (one value or P), host float64.  Per voxel and view the definition of
    include/livingscenes_hip.h: the projective distance d - c.z at the nearest pixel, truncated to [-1, 1] and added as an integer, so
    the state does not depend on the order of the views, on how they are split over calls or on the batch.  empty="free": pixels that
    hit nothing count as free space (t = +1), "unknown": they are skipped.  NO voxel OR trunc IS RECOMMENDED: none has been measured
    on real scans.  -> list of P device int64 [V_p,6]: voxels per class of FUSE_CLASS and view.  One call, no host read."""
    op = "depth_fuse_batch"
    S, N, P, dims = _fuse_state(op, state, True)
    dev = S.device
    if not (len(depths) == len(world_to_cam) == P) or (not torch.is_tensor(intrinsics) and len(intrinsics) != P):
        raise ValueError(f"{op}: {P} problems in state for {len(depths)} sets of depth views and {len(world_to_cam)} sets of cameras")
    o, h, tr = _fuse_grid(op, P, origin, voxel, trunc)
    eif, znear = _fuse_empty(op, empty), float(znear)
    Ks = [intrinsics] * P if torch.is_tensor(intrinsics) else list(intrinsics)
    vw = [None if d is None else _carve_views(op, d, k, e, dev) for d, k, e in zip(depths, Ks, world_to_cam)]
    shapes = sorted({tuple(v[0].shape[1:]) for v in vw if v is not None})
    if len(shapes) > 1:
        raise ValueError(f"{op}: one H x W per call, got {shapes}")
    nviews = [0 if v is None else v[0].shape[0] for v in vw]
    vo = _offsets(nviews)
    views = int(vo[P])
    if views == 0:
        return [torch.zeros(0, 6, dtype=torch.int64, device=dev) for _ in range(P)]
    have = [v for v in vw if v is not None and v[0].shape[0]]
    D, K, E = (torch.cat(t, 0) if len(have) > 1 else t[0] for t in zip(*have))
    H, W = shapes[0]
    vc = torch.empty(views, 6, dtype=torch.int64, device=dev)
    ws_bytes = load().ls_depth_fuse_batch_workspace_bytes(P, *dims, views)
    if ws_bytes == 0:
        raise ValueError(f"{op}: P = {P} problems of dims {dims} with {views} views unsupported (include/livingscenes_hip.h: P nx ny nz < 2^31)")
    ws = _scratch(ws_bytes, dev)
    call(dev, "ls_depth_fuse_batch_f32", P, ptr(S), ptr(N), *dims, _hptr(o), _hptr(h), _hptr(tr), ptr(D), views, _hptr(vo), H, W, ptr(K), ptr(E),
         znear, eif, ptr(vc), ptr(ws), ws.numel(), stream_ptr(dev))
    return list(torch.split(vc, nviews))


def depth_fuse(state, depth, intrinsics, world_to_cam, *, origin, voxel, trunc, empty="unknown", znear=0.05):
    """ls_depth_fuse_f32: the views depth [V,H,W] fp32 with intrinsics [V,4] or [4] and world_to_cam [V,3,4] float64 from the grid's frame
    fused into state = (sum, n), int32 HIP tensors [nx,ny,nz] (a slice of tsdf_state), IN PLACE; origin [3], voxel and trunc host float64.
    -> device int64 [V,6], the voxels per class of FUSE_CLASS, as depth_fuse_batch describes them (no voxel or trunc is recommended).
    Bit-identical to the same problem inside any depth_fuse_batch, and to the same views in any order or split over calls."""
    op = "depth_fuse"
    S, N, _, dims = _fuse_state(op, state, False)
    dev = S.device
    o, h, tr = _fuse_grid(op, 1, origin, voxel, trunc)
    eif, znear = _fuse_empty(op, empty), float(znear)
    D, K, E = _carve_views(op, depth, intrinsics, world_to_cam, dev)
    views, H, W = D.shape
    vc = torch.empty(views, 6, dtype=torch.int64, device=dev)
    if views == 0:
        return vc
    ws_bytes = load().ls_depth_fuse_workspace_bytes(*dims, views)
    if ws_bytes == 0:
        raise ValueError(f"{op}: dims {dims} with {views} views unsupported (include/livingscenes_hip.h: nx ny nz < 2^31)")
    ws = _scratch(ws_bytes, dev)
    call(dev, "ls_depth_fuse_f32", ptr(S), ptr(N), *dims, _hptr(o), float(h[0]), float(tr[0]), ptr(D), views, H, W, ptr(K), ptr(E), znear, eif,
         ptr(vc), ptr(ws), ws.numel(), stream_ptr(dev))
    return vc


def tsdf_volume(state, min_obs=1):
    """ls_tsdf_volume_f64: state = (sum, n) int32 HIP tensors [P,nx,ny,nz] or [nx,ny,nz] -> (volume float64, valid uint8, of the state's
    shape; counts device int64 [P,3] or [3] = valid samples, valid samples with D <= 0, samples never observed).  A sample is valid iff
    n >= min_obs (>= 1); D = sum / (n * 16384) where valid, else exactly +1.0.  NO min_obs IS RECOMMENDED: 1 is the least, unmeasured."""
    op = "tsdf_volume"
    batch = isinstance(state, (tuple, list)) and len(state) == 2 and torch.is_tensor(state[0]) and state[0].dim() == 4
    S, N, P, dims = _fuse_state(op, state, batch)
    min_obs = int(min_obs)
    if min_obs < 1:
        raise ValueError(f"{op}: min_obs must be >= 1, got {min_obs}")
    dev = S.device
    vol = torch.empty(S.shape, dtype=torch.float64, device=dev)
    valid = torch.empty(S.shape, dtype=torch.uint8, device=dev)
    counts = torch.empty(P, 3, dtype=torch.int64, device=dev)
    call(dev, "ls_tsdf_volume_f64", ptr(S), ptr(N), P, *dims, min_obs, ptr(vol), ptr(valid), ptr(counts), stream_ptr(dev))
    return vol, valid, (counts if batch else counts[0])


MESH_COUNT = ("kept_cubes", "dropped_crossed_cubes", "valid_samples")   # the columns of tsdf_mesh's counts, by value


def _tsdf_mesh_packed(op, single, state, origin, voxel, min_obs):
    """-> (vertices [sum nv,3] float64, faces [sum nf,3] int64, vertex offsets, face offsets: host lists of P+1, counts device int64 [P,3])"""
    S, N, P, dims = _fuse_state(op, state, not single)
    min_obs = int(min_obs)
    if min_obs < 1:
        raise ValueError(f"{op}: min_obs must be >= 1, got {min_obs}")
    o, h = _fuse_grid(op, P, origin, voxel)
    dev = S.device
    name = "ls_tsdf_mesh" if single else "ls_tsdf_mesh_batch"
    ws_bytes = getattr(load(), name + "_workspace_bytes")(*(() if single else (P,)), *dims)
    if ws_bytes == 0:
        raise ValueError(f"{op}: P = {P} problems of dims {dims} unsupported (include/livingscenes_hip.h: P <= 65535, 15 P nx ny nz < 2^31)")
    ws = _scratch(ws_bytes, dev)
    off = torch.zeros(2, P + 1, dtype=torch.int64, device=dev)
    counts = torch.empty(P, 3, dtype=torch.int64, device=dev)
    head = (ptr(S), ptr(N), *dims, min_obs, _hptr(o), float(h[0]) if single else _hptr(h))
    if not single:
        head = (P,) + head
    call(dev, name + "_f64", *head, None, 0, None, 0, ptr(off), None, ptr(ws), ws.numel(), stream_ptr(dev))
    vo, fo = off.cpu().tolist()                                          # the one host read
    verts = torch.empty(vo[P], 3, dtype=torch.float64, device=dev)
    faces = torch.empty(fo[P], 3, dtype=torch.int64, device=dev)
    # the real call also when the meshes are empty: it fills the counts (and writes nothing into the empty outputs)
    call(dev, name + "_f64", *head, ptr(verts) if vo[P] else None, vo[P], ptr(faces) if vo[P] else None, fo[P], ptr(off), ptr(counts), ptr(ws),
         ws.numel(), stream_ptr(dev))
    return verts, faces, vo, fo, counts


def tsdf_mesh_batch(state, *, origin, voxel, min_obs=1, packed=False):
    """ls_tsdf_mesh_batch_f64 (an extension beyond the released reference, like depth_fuse): the fused states of P instances meshed where
    they were OBSERVED.  state = (sum, n) int32 HIP tensors [P,nx,ny,nz] (tsdf_state, depth_fuse_batch); origin [P,3] or [3], voxel (one
    value or P): host float64, the grids the views were fused on.  Marching cubes at 0 of D = sum / (n * 16384) over the cubes whose eight
    corners have n >= min_obs, with exactly the vertices those cubes name, in libmcubes' order, at (V - 0.5) * voxel + origin: the
    definition of include/livingscenes_hip.h, by equality.  No float64 volume is made and nothing is compacted afterwards.
    -> (list of P (vertices [nv,3] float64, faces [nf,3] int64) device tensors, views of the packed outputs, face indices local to their
    mesh; counts device int64 [P,3], the columns of MESH_COUNT: kept cubes, dropped cubes that hold a crossing, valid samples).
    packed=True -> (vertices, faces, vertex offsets, face offsets: host lists of P+1, counts).  One sizing call, ONE host read of the
    offsets, one real call.  An instance nothing kept yields an empty mesh.  DO NOT index a device tensor with the faces before they have
    been range-checked on the host: faces < nv is what the tests assert there.  NO min_obs IS RECOMMENDED: 1 is the least, unmeasured
    on real scans."""
    verts, faces, vo, fo, counts = _tsdf_mesh_packed("tsdf_mesh_batch", False, state, origin, voxel, min_obs)
    if packed:
        return verts, faces, vo, fo, counts
    return [(verts[vo[p]:vo[p + 1]], faces[fo[p]:fo[p + 1]]) for p in range(len(vo) - 1)], counts


def tsdf_mesh(state, *, origin, voxel, min_obs=1):
    """ls_tsdf_mesh_f64: state = (sum, n) int32 HIP tensors [nx,ny,nz] (a slice of tsdf_state), origin [3] and voxel host float64 ->
    (vertices [nv,3] float64, faces [nf,3] int64, counts device int64 [3] of MESH_COUNT), as tsdf_mesh_batch describes them and
    bit-identical to the same problem inside any batch.  NO min_obs IS RECOMMENDED: 1 is the least, unmeasured on real scans."""
    verts, faces, _, _, counts = _tsdf_mesh_packed("tsdf_mesh", True, state, origin, voxel, min_obs)
    return verts, faces, counts[0]


def _plane_normals(x, A, op):
    x = _cloud(x, "N", op)
    if x.shape[0] != A.shape[0] or x.device != A.device:
        raise ValueError(f"{op}: N is {tuple(x.shape)} on {x.device} for A {tuple(A.shape)} on {A.device}: one normal row per kept row")
    return x


def cloud_icp_plane_batch(As, Ns, Bs, g=None, *, radius, max_iter=100, rel_thr=1e-6, min_matched=6, trace=False, packed=False):
    """ls_cloud_icp_plane_batch_f32 (an extension beyond the released reference, like cloud_icp): the trimmed ICP of cloud_icp_batch with
    the point-to-plane metric.  Ns[p] [a_p,3] are the normals of the kept rows As[p] (cloud_normals makes them; a zero row means "no
    normal"); the other arguments are cloud_icp_batch's.  Per iteration: cloud_nearest under the current pose; a match is planar iff its
    neighbour has a normal; E = (sum rho^2 + (finite - planar) r^2) / finite with rho the distance to the neighbour's tangent plane; the
    stop tests of cloud_icp on the PLANAR count (min_matched = 6: six unknowns); else the 6 x 6 normal equations of the linearised step in
    float64, Cholesky (a failed pivot: degenerate -- one plane, or all normals parallel), exp of the twist, the rotation re-orthonormalised.
    The linearised step is not guaranteed to lower E: there is no line search and no damping, and a step that raises E ends the loop as
    converged with the pose it produced.  max_iter and rel_thr are cloud_icp's defaults: inherited, not tuned.
    -> list of P dicts as cloud_icp_batch returns them plus planar (int) and sum_rho2 (float) of the final search; trace=True adds g_trace
    [max_iter+1,12] and stat_trace [max_iter+1,5] = (finite, matched, sum d2, planar, sum rho^2).  packed=True: one dict of packed tensors."""
    op = "cloud_icp_plane"
    P, dev, A, ao, B, bo, rad, g = _pairs(op, As, Bs, g, radius)
    if len(Ns) != P:
        raise ValueError(f"{op}: {P} kept clouds for {len(Ns)} arrays of normals")
    N, _ = _pack([_plane_normals(n, a, op) for n, a in zip(Ns, As)])
    head = (P, ptr(A), ptr(N), A.shape[0], _hptr(ao), ptr(B), B.shape[0], _hptr(bo), ptr(g), _hptr(rad))
    return _icp(op, "ls_cloud_icp_plane_batch_f32", head, (P, A.shape[0], B.shape[0]), P, dev, bo, max_iter, rel_thr, min_matched, trace, packed,
                plane=True)


def cloud_icp_plane(A, N, B, g=None, *, radius, max_iter=100, rel_thr=1e-6, min_matched=6, trace=False):
    """ls_cloud_icp_plane_f32: the point-to-plane trimmed ICP of the observation B [b,3] onto the kept cloud A [a,3] with the normals N [a,3]
    (fp32 HIP tensors), g [3,4] or [4,4] the initial pose (None: identity) -> the dict cloud_icp_plane_batch describes.  Bit-identical to
    the same problem inside any cloud_icp_plane_batch."""
    op = "cloud_icp_plane"
    A, B = _cloud(A, "A", op), _cloud(B, "B", op)
    dev = A.device
    g = _pose(g, op, dev)
    N = _plane_normals(N, A, op)
    head = (ptr(A), ptr(N), A.shape[0], ptr(B), B.shape[0], ptr(g), float(radius))
    return _icp(op, "ls_cloud_icp_plane_f32", head, (A.shape[0], B.shape[0]), 1, dev, _offsets([B.shape[0]]), max_iter, rel_thr, min_matched, trace,
                False, plane=True)[0]


# ------------------------------------------------------------------------------------------------ the fused state read and registered against (csrc/tsdficp.hip)
SAMPLE_STATE = ("out", "unseen", "sampled")                 # the values of a query's state, by value
SAMPLE_COUNT = ("finite", "inside", "sampled")              # the columns of tsdf_sample's counts, by value
_SAMPLE_META = [("counts", np.int64, 3), ("sum_phi2", np.float64, 1)]


def _tsdf_queries(op, single, state, B, g, origin, voxel, trunc, min_obs):
    """the argument checks of the four wrappers -> (S, N, P, dims, dev, B packed, host b_off, g [P,3,4] or [3,4] or None, o, h, tr, min_obs)"""
    S, N, P, dims = _fuse_state(op, state, not single)
    dev = S.device
    min_obs = int(min_obs)
    if min_obs < 1:
        raise ValueError(f"{op}: min_obs must be >= 1, got {min_obs}")
    o, h, tr = _fuse_grid(op, P, origin, voxel, trunc)
    if single:
        B = _cloud(B, "B", op)
        bo = _offsets([B.shape[0]])
        g = _pose(g, op, dev)
    else:
        Bs = [_cloud(x, "B", op) for x in B]
        if len(Bs) != P:
            raise ValueError(f"{op}: {P} problems in state for {len(Bs)} arrays of queries")
        B, bo = _pack(Bs)
        g = _poses(g, op, P, dev)
    if B.device != dev:
        raise ValueError(f"{op}: the state is on {dev}, B on {B.device}")
    return S, N, P, dims, dev, B, bo, g, o, h, tr, min_obs


def _tsdf_call(op, single, S, N, P, dims, dev, B, bo, g, o, h, tr, min_obs, tail, outs):
    """the entry of `op` with the scratch its size query asks for; tail: the ICP's scalars, outs: the output pointers in the entry's order"""
    name = "ls_" + op
    b = B.shape[0]
    ws_bytes = getattr(load(), name + "_workspace_bytes")(*(() if single else (P,)), *dims, b)
    if ws_bytes == 0:
        raise ValueError(f"{op}: P = {P} problems of dims {dims} with {b} queries unsupported (include/livingscenes_hip.h: P nx ny nz < 2^31)")
    ws = _scratch(ws_bytes, dev)
    if single:
        head = (ptr(S), ptr(N), *dims, min_obs, _hptr(o), float(h[0]), float(tr[0]), ptr(B), b, ptr(g))
    else:
        head = (P, ptr(S), ptr(N), *dims, min_obs, _hptr(o), _hptr(h), _hptr(tr), ptr(B), b, _hptr(bo), ptr(g))
    call(dev, name + "_f32", *head, *tail, *outs, ptr(ws), ws.numel(), stream_ptr(dev))


def _tsdf_sample(op, single, state, B, g, origin, voxel, trunc, min_obs, packed):
    S, N, P, dims, dev, B, bo, g, o, h, tr, min_obs = _tsdf_queries(op, single, state, B, g, origin, voxel, trunc, min_obs)
    b = B.shape[0]
    phi = torch.empty(b, dtype=torch.float64, device=dev)
    grad = torch.empty(b, 3, dtype=torch.float64, device=dev)
    st = torch.empty(b, dtype=torch.uint8, device=dev)
    m = _Meta(P, dev, _SAMPLE_META + [("status", np.int32, 1)])
    m.buf.zero_()                                                        # the entries have no status: LS_OK
    _tsdf_call(op, single, S, N, P, dims, dev, B, bo, g, o, h, tr, min_obs, (), (ptr(phi), ptr(grad), ptr(st), m.ptr("counts"), m.ptr("sum_phi2")))
    f = m.read(op)
    if single:
        return phi, grad, st, f["counts"][0], float(f["sum_phi2"][0])
    if packed:
        return phi, grad, st, f["counts"], f["sum_phi2"], bo
    sizes = np.diff(bo).tolist()
    return [(x, y, z, f["counts"][p], float(f["sum_phi2"][p]))
            for p, (x, y, z) in enumerate(zip(torch.split(phi, sizes), torch.split(grad, sizes), torch.split(st, sizes)))]


def tsdf_sample_batch(state, Bs, g=None, *, origin, voxel, trunc, min_obs=1, packed=False):
    """ls_tsdf_sample_batch_f32 (an extension beyond the released reference, like depth_fuse): the fused states of P instances READ at
    posed points.  state = (sum, n) int32 HIP tensors [P,nx,ny,nz] (tsdf_state, depth_fuse_batch); Bs = list of P query arrays [b_p,3]
    (fp32 HIP tensors, empty ones allowed); g [P,3,4] or [P,4,4] taking B_p into the grid's frame (None: B bit for bit); origin [P,3]
    or [3], voxel, trunc (one value or P): host float64, the grids the views were fused on.  Per query the definition of
    include/livingscenes_hip.h: the posed row in fp32, its cell, and -- only where all eight corners have n >= min_obs -- the trilinear
    value phi of the truncated distance in METRES and the exact gradient of that interpolant (not normalised), float64.  A query outside
    the grid ("out") or with an unobserved corner ("unseen") gets phi = +trunc, grad = 0: no value ever reads an unobserved sample.
    -> list of P (phi [b_p] float64, grad [b_p,3] float64, state [b_p] uint8 of SAMPLE_STATE, counts host int64 [3] of SAMPLE_COUNT,
    sum_phi2 float: the float64 sum of phi^2 over the sampled queries); packed=True: (phi, grad, state, counts [P,3], sum_phi2 [P], b_off).
    One call, one host read, whatever P.  NO min_obs IS RECOMMENDED: 1 is the least, unmeasured on real scans."""
    return _tsdf_sample("tsdf_sample_batch", False, state, Bs, g, origin, voxel, trunc, min_obs, packed)


def tsdf_sample(state, B, g=None, *, origin, voxel, trunc, min_obs=1):
    """ls_tsdf_sample_f32: state = (sum, n) int32 HIP tensors [nx,ny,nz] (a slice of tsdf_state), B [b,3] fp32, g [3,4] or [4,4] or None,
    origin [3], voxel and trunc host float64 -> (phi [b] float64, grad [b,3] float64, state [b] uint8, counts host int64 [3], sum_phi2
    float) as tsdf_sample_batch describes them, bit-identical to the same problem inside any batch.  NO min_obs IS RECOMMENDED."""
    return _tsdf_sample("tsdf_sample", True, state, B, g, origin, voxel, trunc, min_obs, False)


_TSDF_ICP_SCALARS = {"stop": int, "iters": int, "sum_phi2": float}


def _tsdf_icp(op, single, state, B, g, origin, voxel, trunc, min_obs, max_iter, rel_thr, min_matched, trace, packed):
    S, N, P, dims, dev, B, bo, g, o, h, tr, min_obs = _tsdf_queries(op, single, state, B, g, origin, voxel, trunc, min_obs)
    b, max_iter = B.shape[0], int(max_iter)
    phi = torch.empty(b, dtype=torch.float64, device=dev)
    grad = torch.empty(b, 3, dtype=torch.float64, device=dev)
    st = torch.empty(b, dtype=torch.uint8, device=dev)
    g_out = torch.empty(P, 3, 4, dtype=torch.float32, device=dev)
    traces = {}
    if trace:
        traces = {"g_trace": torch.zeros(P, max(max_iter, 0) + 1, 12, dtype=torch.float32, device=dev),
                  "stat_trace": torch.zeros(P, max(max_iter, 0) + 1, 3, dtype=torch.float64, device=dev)}
    m = _Meta(P, dev, _SAMPLE_META + [("status", np.int32, 1), ("stop", np.int32, 1), ("iters", np.int32, 1)])
    m.buf.zero_()
    _tsdf_call(op, single, S, N, P, dims, dev, B, bo, g, o, h, tr, min_obs, (max_iter, float(rel_thr), int(min_matched)),
               (ptr(g_out), m.ptr("stop"), m.ptr("iters"), ptr(phi), ptr(grad), ptr(st), m.ptr("counts"), m.ptr("sum_phi2"),
                ptr(traces.get("g_trace")), ptr(traces.get("stat_trace"))))
    f = m.read(op)
    out = {"g": g_out, "stop": f["stop"], "iters": f["iters"], "phi": phi, "grad": grad, "state": st, "counts": f["counts"], "sum_phi2": f["sum_phi2"]}
    if packed:
        out["b_off"] = bo
    out.update(traces)
    if packed:
        return out
    sizes = np.diff(bo).tolist()
    for k in ("phi", "grad", "state"):
        out[k] = torch.split(out[k], sizes)
    res = [{k: _TSDF_ICP_SCALARS[k](v[p]) if k in _TSDF_ICP_SCALARS else v[p] for k, v in out.items()} for p in range(P)]
    return res[0] if single else res


def tsdf_icp_batch(state, Bs, g=None, *, origin, voxel, trunc, min_obs=1, max_iter=100, rel_thr=1e-6, min_matched=6, trace=False, packed=False):
    """ls_tsdf_icp_batch_f32 (an extension beyond the released reference, like cloud_icp_plane): P observations Bs[p] [b_p,3] registered
    onto the fused states of their instances without any search (Bylow et al., RSS 2013).  state, origin, voxel, trunc, min_obs:
    tsdf_sample_batch's; g [P,3,4] or [P,4,4] is the initial pose taking B_p into the grid's frame (None: the identity).  Per iteration:
    tsdf_sample under the current pose; E = (sum phi^2 + (finite - sampled) trunc^2) / finite, the truncated quadratic of cloud_icp
    with trunc in the place of the radius; the stop tests of cloud_icp_plane on the SAMPLED count (min_matched = 6: six unknowns); else
    the 6 x 6 normal equations of sum (phi + omega . (y x grad) + v . grad)^2 in float64, Cholesky (a failed pivot: degenerate -- the
    state of one plane, all gradients parallel), exp of the twist, the rotation re-orthonormalised: the solver text of cloud_icp_plane.
    The gradient is NOT normalised, nothing is weighted, and there is no line search and no damping: a step that raises E ends the loop
    as converged with the pose it produced.  A query in saturated free space has phi = trunc and grad = 0: it costs what an unsampled
    one costs and pulls on nothing.  The start error must lie within trunc.  max_iter = 100 and rel_thr = 1e-6 are ops.icp's defaults,
    pytorch3d's: INHERITED, NOT TUNED.
    -> list of P dicts: g [3,4] fp32 (device), stop (int, LS_ICP_*; ICP_STOP names them), iters (int), and the final sample exactly as
    tsdf_sample(state_p, B_p, g, ...) returns it: phi, grad, state, counts (host int64 [3]), sum_phi2 (float); trace=True adds g_trace
    [max_iter+1,12] and stat_trace [max_iter+1,3] float64 = (finite, sampled, sum phi^2) per iteration (device; rows <= iters are
    written).  packed=True: one dict of the packed tensors plus b_off.  One call, one host read, whatever P and however many iterations.
    NO min_obs IS RECOMMENDED."""
    return _tsdf_icp("tsdf_icp_batch", False, state, Bs, g, origin, voxel, trunc, min_obs, max_iter, rel_thr, min_matched, trace, packed)


def tsdf_icp(state, B, g=None, *, origin, voxel, trunc, min_obs=1, max_iter=100, rel_thr=1e-6, min_matched=6, trace=False):
    """ls_tsdf_icp_f32: the observation B [b,3] registered onto the fused state (sum, n) [nx,ny,nz] -> the dict tsdf_icp_batch describes.
    max_iter = 100 and rel_thr = 1e-6 are ops.icp's defaults, pytorch3d's: inherited, not tuned.  Bit-identical to the same problem
    inside any tsdf_icp_batch.  NO min_obs IS RECOMMENDED."""
    return _tsdf_icp("tsdf_icp", True, state, B, g, origin, voxel, trunc, min_obs, max_iter, rel_thr, min_matched, trace, False)


# ------------------------------------------------------------------------------------------------ the fused state as a training signal (csrc/tsdffit.hip)
FIT_KIND = ("pad", "band", "free")                         # the values of a column's kind, by value
DRAW_COUNT = ("eligible", "band", "free")                  # the columns of tsdf_draw's counts, by value


def _tsdf_draw(op, single, state, origin, voxel, trunc, n_band, n_free, seeds, min_obs):
    S, N, P, dims = _fuse_state(op, state, not single)
    dev = S.device
    min_obs, n_band, n_free = int(min_obs), int(n_band), int(n_free)
    if min_obs < 1:
        raise ValueError(f"{op}: min_obs must be >= 1, got {min_obs}")
    if n_band < 0 or n_free < 0 or n_band + n_free < 1:
        raise ValueError(f"{op}: quotas n_band, n_free >= 0 with n_band + n_free >= 1, got {n_band}, {n_free}")
    o, h, tr = _fuse_grid(op, P, origin, voxel, trunc)
    sd = np.asarray(seeds.detach().cpu().numpy() if torch.is_tensor(seeds) else seeds)
    if sd.ndim == 0:
        sd = sd.reshape(1)
    if sd.shape != (P,) or sd.dtype.kind not in "iu" or (sd.dtype.kind == "i" and (sd < 0).any()):
        raise ValueError(f"{op}: seeds are {P} non-negative integers (uint64), one per problem, got {sd.dtype} {sd.shape}")
    sd = np.ascontiguousarray(sd, dtype=np.uint64)
    cols = n_band + n_free
    name = "ls_" + op
    ws_bytes = getattr(load(), name + "_workspace_bytes")(*(() if single else (P,)), *dims)
    if ws_bytes == 0 or P * cols >= 2 ** 31:
        raise ValueError(f"{op}: P = {P} problems of dims {dims} with {cols} columns unsupported (include/livingscenes_hip.h: P nx ny nz < 2^31, "
                         "nx ny nz <= 4096 blocks of 4096 samples, P <= 65535, P (n_band + n_free) < 2^31)")
    ws = _scratch(ws_bytes, dev)
    points = torch.empty(P, cols, 3, dtype=torch.float32, device=dev)
    target = torch.empty(P, cols, dtype=torch.float64, device=dev)
    kind = torch.empty(P, cols, dtype=torch.uint8, device=dev)
    index = torch.empty(P, cols, dtype=torch.int32, device=dev)
    counts = torch.empty(P, 3, dtype=torch.int64, device=dev)
    outs = (ptr(points), ptr(target), ptr(kind), ptr(index), ptr(counts), ptr(ws), ws.numel(), stream_ptr(dev))
    if single:
        call(dev, name + "_f32", ptr(S), ptr(N), *dims, min_obs, _hptr(o), float(h[0]), float(tr[0]), n_band, n_free, int(sd[0]), *outs)
        return points[0], target[0], kind[0], index[0], counts[0].cpu().numpy()
    call(dev, name + "_f32", P, ptr(S), ptr(N), *dims, min_obs, _hptr(o), _hptr(h), _hptr(tr), n_band, n_free, _hptr(sd), *outs)
    return points, target, kind, index, counts.cpu().numpy()


def tsdf_draw_batch(state, *, origin, voxel, trunc, n_band, n_free, seeds, min_obs=1):
    """ls_tsdf_draw_batch_f32 (an extension beyond the released reference, like tsdf_icp): a fixed-size, deterministic set of training
    samples drawn out of the fused states of P instances.  state = (sum, n) int32 HIP tensors [P,nx,ny,nz] (tsdf_state, depth_fuse_batch);
    origin [P,3] or [3], voxel, trunc (one value or P): host float64, the grids the views were fused on; seeds: P uint64.  A lattice
    sample with n >= min_obs is FREE iff sum == n * 16384 (every view that looked saw it at or beyond +trunc), else BAND.  Of each kind's
    list, in linear index order, a quota (n_band, n_free; the same for every problem) takes one sample per stratum, chosen by a
    splitmix64 stream of the problem's seed: the definition of include/livingscenes_hip.h, by equality.  A list shorter than its quota
    is taken whole and the remaining columns are PAD.
    -> (points fp32 [P,N,3], target float64 [P,N] in metres, kind uint8 [P,N] of FIT_KIND, index int32 [P,N] (-1: PAD): device tensors,
    columns [0, n_band) the band and [n_band, N) free space; counts host int64 [P,3] of DRAW_COUNT).  One call, three kernels and one
    host read (the counts), whatever P.  A problem's draw does not depend on the batch.  NO QUOTA AND NO min_obs IS RECOMMENDED."""
    return _tsdf_draw("tsdf_draw_batch", False, state, origin, voxel, trunc, n_band, n_free, seeds, min_obs)


def tsdf_draw(state, *, origin, voxel, trunc, n_band, n_free, seeds, min_obs=1):
    """ls_tsdf_draw_f32: state = (sum, n) int32 HIP tensors [nx,ny,nz] (a slice of tsdf_state), origin [3], voxel and trunc host float64,
    seeds one uint64 -> (points [N,3], target [N], kind [N], index [N], counts host int64 [3]) as tsdf_draw_batch describes them,
    bit-identical to the same problem anywhere inside any batch.  NO QUOTA AND NO min_obs IS RECOMMENDED."""
    return _tsdf_draw("tsdf_draw", True, state, origin, voxel, trunc, n_band, n_free, seeds, min_obs)


def tsdf_fit_loss(sdf, s, trunc, target, kind, min_loss=None, improved=None):
    """ls_tsdf_fit_loss_f64: the loss that holds the decoder to a draw, in the decoder's own units -- THIS BUILD'S DEFINITION: the
    decoder's value times s is a metric distance.  sdf fp32 [P,N], s fp32 [P], trunc float64 [P], target float64 [P,N], kind uint8 [P,N]
    (HIP tensors; tsdf_draw_batch makes the last two).  BAND: e = sdf - target / s; FREE: e = min(sdf - trunc / s, 0), a one-sided
    hinge; PAD: 0; float64.  -> (loss float64 [P] = sum e^2 / m_p over the m_p non-PAD columns, 0 where there is none;
    grad fp32 [P,N] = 2 e / m_p).  min_loss float64 [P] / improved int32 [P] (optional) are updated in place where the loss improved,
    as ops.mse does.  No weight between the kinds, no clamp of the band error; MSE(sdf, 0) is the case target = 0, all BAND."""
    op = "tsdf_fit_loss"
    sdf = _f32(sdf)
    if sdf.dim() != 2 or sdf.numel() == 0:
        raise ValueError(f"{op}: sdf is [P,N], got {tuple(sdf.shape)}")
    P, N = sdf.shape
    dev = sdf.device
    for name, t, dtype, shape in (("s", s, torch.float32, (P,)), ("trunc", trunc, torch.float64, (P,)), ("target", target, torch.float64, (P, N)),
                                  ("kind", kind, torch.uint8, (P, N)), ("min_loss", min_loss, torch.float64, (P,)),
                                  ("improved", improved, torch.int32, (P,))):
        if t is None and name in ("min_loss", "improved"):
            continue
        if not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != shape or t.device != dev or not t.is_contiguous():
            got = f"{t.dtype} {tuple(t.shape)} on {t.device}" if torch.is_tensor(t) else type(t).__name__
            raise ValueError(f"{op}: {name} must be a contiguous {dtype} tensor {shape} on {dev}, got {got}")
    loss = torch.empty(P, dtype=torch.float64, device=dev)
    grad = torch.empty_like(sdf)
    call(dev, "ls_tsdf_fit_loss_f64", ptr(sdf), ptr(s), ptr(trunc), ptr(target), ptr(kind), P, N, ptr(loss), ptr(grad), ptr(min_loss), ptr(improved),
         stream_ptr(dev))
    return loss, grad


# ------------------------------------------------------------------------------------------------ the fused state seen from a camera (csrc/tsdfray.hip)
RAY_STATE = ("outside", "free", "unseen", "behind", "hit")               # the values of a pixel's state, by value
VIEW_CLASS = ("no_obs", "unknown", "agree", "in_front", "through")      # the values of a compared pixel's class, by value


def _ray_cameras(op, cam_to_world, intrinsics, dev):
    """the cameras of one problem: cam_to_world [V,3,4] and intrinsics [V,4] or [4], float64 HIP tensors on dev (None: no view)"""
    if cam_to_world is None:
        return None
    M = _f64_dev(cam_to_world, "cam_to_world", op, (3, 4))
    K = _f64_dev(intrinsics, "intrinsics", op, (4,), M.shape[0])
    if M.device != dev or K.device != dev:
        raise ValueError(f"{op}: the state is on {dev}, cam_to_world on {M.device}, intrinsics on {K.device}")
    return M, K


def _tsdf_raycast(op, single, state, cam_to_world, intrinsics, height, width, origin, voxel, trunc, min_obs, step, znear, packed):
    S, N, P, dims = _fuse_state(op, state, not single)
    dev = S.device
    min_obs, H, W, step, znear = int(min_obs), int(height), int(width), float(step), float(znear)
    if min_obs < 1:
        raise ValueError(f"{op}: min_obs must be >= 1, got {min_obs}")
    if H < 1 or W < 1:
        raise ValueError(f"{op}: the image must have at least one pixel, got {H} x {W}")
    o, h, tr = _fuse_grid(op, P, origin, voxel, trunc)
    if single:
        cams = [_ray_cameras(op, cam_to_world, intrinsics, dev)]
        if cams[0] is None:
            raise ValueError(f"{op}: cam_to_world is [views,3,4], got None")
    else:
        if len(cam_to_world) != P or (not torch.is_tensor(intrinsics) and len(intrinsics) != P):
            raise ValueError(f"{op}: {P} problems in state for {len(cam_to_world)} sets of cameras")
        Ks = [intrinsics] * P if torch.is_tensor(intrinsics) else list(intrinsics)
        cams = [_ray_cameras(op, m, k, dev) for m, k in zip(cam_to_world, Ks)]
    nviews = [0 if c is None else c[0].shape[0] for c in cams]
    vo = _offsets(nviews)
    views = int(vo[P])
    name = "ls_" + op
    ws_bytes = getattr(load(), name + "_workspace_bytes")(*(() if single else (P,)), *dims, views, H, W)
    if ws_bytes == 0:
        raise ValueError(f"{op}: P = {P} problems of dims {dims} with {views} views of {H} x {W} unsupported (include/livingscenes_hip.h: "
                         "P nx ny nz < 2^31, views * height * width < 2^31)")
    ws = _scratch(ws_bytes, dev)
    depth = torch.empty(views, H, W, dtype=torch.float32, device=dev)
    normal = torch.empty(views, H, W, 3, dtype=torch.float32, device=dev)
    st = torch.empty(views, H, W, dtype=torch.uint8, device=dev)
    counts = torch.empty(views, 5, dtype=torch.int64, device=dev)
    have = [c for c in cams if c is not None and c[0].shape[0]]
    M, K = (torch.cat(t, 0) if len(have) > 1 else t[0] for t in zip(*have)) if have else (None, None)
    outs = (H, W, znear, step, ptr(depth), ptr(normal), ptr(st), ptr(counts), ptr(ws), ws.numel(), stream_ptr(dev))
    if single:
        call(dev, name + "_f64", ptr(S), ptr(N), *dims, min_obs, _hptr(o), float(h[0]), float(tr[0]), ptr(M), ptr(K), views, *outs)
        return depth, normal, st, counts
    call(dev, name + "_f64", P, ptr(S), ptr(N), *dims, min_obs, _hptr(o), _hptr(h), _hptr(tr), ptr(M), ptr(K), views, _hptr(vo), *outs)
    if packed:
        return depth, normal, st, counts, vo
    return list(zip(torch.split(depth, nviews), torch.split(normal, nviews), torch.split(st, nviews), torch.split(counts, nviews)))


def tsdf_raycast_batch(state, cam_to_world, intrinsics, height, width, *, origin, voxel, trunc, min_obs=1, step=0.5, znear=0.05, packed=False):
    """ls_tsdf_raycast_batch_f64 (an extension beyond the released reference, like depth_fuse; the raycast of KinectFusion): the fused
    states of P instances SEEN from posed cameras.  state = (sum, n) int32 HIP tensors [P,nx,ny,nz] (tsdf_state, depth_fuse_batch);
    cam_to_world = list of P float64 HIP tensors [V_p,3,4] taking the CAMERA frame (x right, y down, z forward, the convention of
    depth_points) into the grid's frame (V_p = 0 or None: no view of that problem); intrinsics = a list of P [V_p,4] or [4], or one [4]
    tensor for all: (fx, fy, cx, cy); one height x width per call; origin [P,3] or [3], voxel, trunc (one value or P): host float64, the
    grids the views were fused on.  Per pixel the definition of include/livingscenes_hip.h: the ray through the integer pixel coordinate,
    parametrised by the camera depth, clipped to the grid, marched in steps of `step` voxels along its fastest axis; at every sample the
    value of tsdf_sample; the first sample at or below 0 after a positive one is a HIT, whose depth is the linear interpolation between
    the two (no secant iteration, no empty-space skipping) and whose normal is the unit gradient there, in the grid's frame.
    -> list of P (depth fp32 [V_p,H,W] (0: no hit), normal fp32 [V_p,H,W,3], state uint8 [V_p,H,W] of RAY_STATE, counts int64 [V_p,5],
    the histogram of the states): device tensors; packed=True: (depth, normal, state, counts, view_off) over all views.  One call, no
    host read, whatever P.  "free" says the memory looked all along the ray and found nothing, "unseen" that it never looked somewhere
    along it, "behind" that the first thing known is the inside of something.  step = 0.5 IS AN UNMEASURED DEFAULT (derived: step <= 1
    keeps consecutive samples in the same or an adjacent cell; the band is 2 trunc / voxel >= 2 voxels thick); NO min_obs IS RECOMMENDED."""
    return _tsdf_raycast("tsdf_raycast_batch", False, state, cam_to_world, intrinsics, height, width, origin, voxel, trunc, min_obs, step, znear, packed)


def tsdf_raycast(state, cam_to_world, intrinsics, height, width, *, origin, voxel, trunc, min_obs=1, step=0.5, znear=0.05):
    """ls_tsdf_raycast_f64: state = (sum, n) int32 HIP tensors [nx,ny,nz] (a slice of tsdf_state), cam_to_world [V,3,4] and intrinsics
    [V,4] or [4] float64 HIP tensors, origin [3], voxel and trunc host float64 -> (depth [V,H,W], normal [V,H,W,3], state [V,H,W], counts
    [V,5]) as tsdf_raycast_batch describes them, bit-identical to the same problem inside any batch.  step = 0.5 IS AN UNMEASURED
    DEFAULT; NO min_obs IS RECOMMENDED."""
    return _tsdf_raycast("tsdf_raycast", True, state, cam_to_world, intrinsics, height, width, origin, voxel, trunc, min_obs, step, znear, False)


def depth_compare(observed, depth, state, *, tol):
    """ls_depth_compare_f32: an observed depth view against a predicted one (tsdf_raycast's depth and state), per pixel.  observed, depth
    fp32 [V,H,W], state uint8 [V,H,W], HIP tensors; tol > 0 in the depth's unit.  no_obs: the observation is not > 0; unknown: the
    prediction is not a hit; else with s = observed - predicted in float64: agree |s| <= tol, in_front s < -tol (something new stands
    before the memory's surface), through s > tol (the view sees past a surface the memory holds).  -> (cls uint8 [V,H,W] of VIEW_CLASS,
    counts int64 [V,5]): device tensors, no host read.  Comparisons and integer counts only.  NO tol IS RECOMMENDED."""
    op = "depth_compare"
    tol = float(tol)
    if not tol > 0.0:
        raise ValueError(f"{op}: tol must be > 0, got {tol}")
    if not torch.is_tensor(observed) or observed.device.type != "cuda" or observed.dim() != 3 or observed.shape[1] < 1 or observed.shape[2] < 1:
        raise ValueError(f"{op}: observed is an fp32 HIP (cuda) tensor [views, H, W] with at least one pixel")
    dev, shape = observed.device, tuple(observed.shape)
    for name, t, dtype in (("observed", observed, torch.float32), ("depth", depth, torch.float32), ("state", state, torch.uint8)):
        if not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != shape or t.device != dev or not t.is_contiguous():
            got = f"{t.dtype} {tuple(t.shape)} on {t.device}" if torch.is_tensor(t) else type(t).__name__
            raise ValueError(f"{op}: {name} must be a contiguous {dtype} tensor {shape} on {dev}, got {got}")
    V, H, W = shape
    if V * H * W >= 2 ** 31:
        raise ValueError(f"{op}: {V} views of {H} x {W} pixels unsupported (views * height * width < 2^31)")
    cls = torch.empty(shape, dtype=torch.uint8, device=dev)
    counts = torch.empty(V, 5, dtype=torch.int64, device=dev)
    call(dev, "ls_depth_compare_f32", ptr(observed), ptr(depth), ptr(state), V, H, W, tol, ptr(cls), ptr(counts), stream_ptr(dev))
    return cls, counts


# ------------------------------------------------------------------------------------------------ depth normals and the weighted fuse (csrc/depthplane.hip)
DEPTH_NORMAL_STATE = ("no_depth", "valid", "no_neighbour", "degenerate")                               # the values of depth_normals' state
FUSE_WEIGHTED_CLASS = ("out", "empty", "occluded", "near_plane", "near_proj", "free", "saturated")    # the columns of the weighted view_counts


def depth_normals(depth, intrinsics, *, max_jump):
    """ls_depth_normals_f32 (an extension beyond the released reference, like depth_fuse): a normal per pixel of depth views, in the
    CAMERA frame.  depth [V,H,W] fp32 and intrinsics [V,4] or [4] float64, HIP tensors; max_jump > 0 (one value or V, host float64), in
    the depth's unit.  Per pixel the definition of include/livingscenes_hip.h: the back-projected points of the left / right and upper /
    lower neighbours whose depth differs by at most max_jump (central differences, one-sided beside a hole, an edge or a jump), their
    cross product normalised in float64 and turned towards the camera, rounded once to fp32.
    -> (normals fp32 [V,H,W,3], (0, 0, 0) unless valid; state uint8 [V,H,W] of DEPTH_NORMAL_STATE; counts int64 [V,4], the histogram of
    the states): device tensors, one call, no host read.  NO max_jump IS RECOMMENDED: none has been measured on real scans."""
    op = "depth_normals"
    if not torch.is_tensor(depth) or depth.device.type != "cuda" or depth.dtype != torch.float32:
        kind = f"{depth.device.type} {depth.dtype}" if torch.is_tensor(depth) else type(depth).__name__
        raise _lib.LsError(f"{op}: depth must be an fp32 HIP (cuda) tensor, got {kind}: the MI355X path has no CPU fallback and converts nothing")
    if depth.dim() != 3 or depth.shape[1] < 1 or depth.shape[2] < 1:
        raise ValueError(f"{op}: depth is [views, H, W] with at least one pixel, got {tuple(depth.shape)}")
    dev = depth.device
    V, H, W = depth.shape
    D, K = depth.contiguous(), _f64_dev(intrinsics, "intrinsics", op, (4,), V)
    mj = max_jump.detach().cpu().numpy() if torch.is_tensor(max_jump) else max_jump
    mj = np.full(V, float(mj), dtype=np.float64) if np.ndim(mj) == 0 else np.ascontiguousarray(mj, dtype=np.float64).reshape(-1)
    if mj.shape[0] != V:
        raise ValueError(f"{op}: {mj.shape[0]} values of max_jump for {V} views")
    if not (np.isfinite(mj) & (mj > 0.0)).all():
        raise ValueError(f"{op}: max_jump must be finite and > 0, got {mj[~(np.isfinite(mj) & (mj > 0.0))][0]}")
    normals = torch.empty(V, H, W, 3, dtype=torch.float32, device=dev)
    state = torch.empty(V, H, W, dtype=torch.uint8, device=dev)
    counts = torch.empty(V, 4, dtype=torch.int64, device=dev)
    if V == 0:
        return normals, state, counts
    ws_bytes = load().ls_depth_normals_workspace_bytes(V, H, W)
    if ws_bytes == 0:
        raise ValueError(f"{op}: {V} views of {H} x {W} pixels unsupported (include/livingscenes_hip.h: views * height * width < 2^31)")
    ws = _scratch(ws_bytes, dev)
    call(dev, "ls_depth_normals_f32", ptr(D), V, H, W, ptr(K), _hptr(mj), ptr(normals), ptr(state), ptr(counts), ptr(ws), ws.numel(), stream_ptr(dev))
    return normals, state, counts


def _fuse_weights(op, weights):
    """weights = (w_plane, w_proj, w_free, w_empty): four integers in 1 .. 255 -> host int32 [4]"""
    try:
        w = [int(k) for k in weights]
        exact = all(k == v for k, v in zip(w, weights))
    except (TypeError, ValueError):
        w, exact = [], False
    if len(w) != 4 or not exact or min(w) < 1 or max(w) > 255:
        raise ValueError(f"{op}: weights are four integers (w_plane, w_proj, w_free, w_empty), each in 1 .. 255, got {weights!r}")
    return np.asarray(w, dtype=np.int32)


def _fuse_normals(op, normals, D, dev):
    """the normals of the views D [V,H,W]: None, or an fp32 HIP tensor [V,H,W,3] (depth_normals of the same views)"""
    if normals is None:
        return None
    if not torch.is_tensor(normals) or normals.device.type != "cuda" or normals.dtype != torch.float32:
        kind = f"{normals.device.type} {normals.dtype}" if torch.is_tensor(normals) else type(normals).__name__
        raise _lib.LsError(f"{op}: normals must be an fp32 HIP (cuda) tensor, got {kind}: the MI355X path has no CPU fallback and converts nothing")
    if tuple(normals.shape) != tuple(D.shape) + (3,) or normals.device != dev:
        raise ValueError(f"{op}: normals is {tuple(D.shape) + (3,)} on {dev}, one per depth pixel, got {tuple(normals.shape)} on {normals.device}")
    return normals.contiguous()


def depth_fuse_weighted_batch(state, depths, intrinsics, world_to_cam, *, origin, voxel, trunc, weights, normals=None, empty="unknown", znear=0.05):
    """ls_depth_fuse_weighted_batch_f32 (an extension beyond the released reference, opt-in beside depth_fuse_batch): posed depth views
    fused into the truncated signed distance state of P instances IN PLACE, with integer weights and a point-to-plane value inside the
    band.  state, depths, intrinsics, world_to_cam, origin, voxel, trunc, empty and znear as depth_fuse_batch takes them; weights =
    (w_plane, w_proj, w_free, w_empty), four integers in 1 .. 255; normals = None, a list of P fp32 HIP tensors [V_p,H,W,3] (depth_normals
    of the same views; None where the problem has no views) or ONE packed tensor [views_total,H,W,3] in the order of the views.  Per voxel
    and view the definition of include/livingscenes_hip.h: the class and the band are the projective fuse's; a NEAR voxel-view whose
    pixel has a normal takes the distance to that pixel's plane, clamped to the band, with w_plane, any other NEAR one the projective
    distance with w_proj; free space counts w_free, an empty pixel taken as free w_empty; sum += w q, n += w.  The state format is the
    fuse's: tsdf_volume, tsdf_mesh, tsdf_sample, tsdf_icp, tsdf_draw and tsdf_raycast read it as it is, min_obs being a weight threshold.
    With normals=None and weights (any, 1, 1, 1) the state is bit for bit depth_fuse_batch's.  weights HAS NO DEFAULT AND NONE IS
    RECOMMENDED: 64 : 1 comes from one synthetic sphere.  -> list of P device int64 [V_p,7]: voxels per class of FUSE_WEIGHTED_CLASS
    and view.  One call, no host read."""
    op = "depth_fuse_weighted_batch"
    S, N, P, dims = _fuse_state(op, state, True)
    dev = S.device
    if not (len(depths) == len(world_to_cam) == P) or (not torch.is_tensor(intrinsics) and len(intrinsics) != P):
        raise ValueError(f"{op}: {P} problems in state for {len(depths)} sets of depth views and {len(world_to_cam)} sets of cameras")
    o, h, tr = _fuse_grid(op, P, origin, voxel, trunc)
    eif, znear, wts = _fuse_empty(op, empty), float(znear), _fuse_weights(op, weights)
    Ks = [intrinsics] * P if torch.is_tensor(intrinsics) else list(intrinsics)
    vw = [None if d is None else _carve_views(op, d, k, e, dev) for d, k, e in zip(depths, Ks, world_to_cam)]
    shapes = sorted({tuple(v[0].shape[1:]) for v in vw if v is not None})
    if len(shapes) > 1:
        raise ValueError(f"{op}: one H x W per call, got {shapes}")
    nviews = [0 if v is None else v[0].shape[0] for v in vw]
    vo = _offsets(nviews)
    views = int(vo[P])
    if views == 0:
        return [torch.zeros(0, 7, dtype=torch.int64, device=dev) for _ in range(P)]
    have = [v for v in vw if v is not None and v[0].shape[0]]
    D, K, E = (torch.cat(t, 0) if len(have) > 1 else t[0] for t in zip(*have))
    if normals is not None and not torch.is_tensor(normals):
        if len(normals) != P:
            raise ValueError(f"{op}: {P} problems in state for {len(normals)} sets of normals")
        parts = [nr for nr, c in zip(normals, nviews) if c]
        if any(nr is None for nr in parts):
            raise ValueError(f"{op}: normals for every problem that has views, or for none")
        normals = torch.cat(parts, 0) if len(parts) > 1 else parts[0]
    Nr = _fuse_normals(op, normals, D, dev)
    H, W = shapes[0]
    vc = torch.empty(views, 7, dtype=torch.int64, device=dev)
    ws_bytes = load().ls_depth_fuse_weighted_batch_workspace_bytes(P, *dims, views)
    if ws_bytes == 0:
        raise ValueError(f"{op}: P = {P} problems of dims {dims} with {views} views unsupported (include/livingscenes_hip.h: P nx ny nz < 2^31)")
    ws = _scratch(ws_bytes, dev)
    call(dev, "ls_depth_fuse_weighted_batch_f32", P, ptr(S), ptr(N), *dims, _hptr(o), _hptr(h), _hptr(tr), ptr(D), ptr(Nr), views, _hptr(vo), H, W,
         ptr(K), ptr(E), znear, eif, _hptr(wts), ptr(vc), ptr(ws), ws.numel(), stream_ptr(dev))
    return list(torch.split(vc, nviews))


def depth_fuse_weighted(state, depth, intrinsics, world_to_cam, *, origin, voxel, trunc, weights, normals=None, empty="unknown", znear=0.05):
    """ls_depth_fuse_weighted_f32: the views depth [V,H,W] fp32 with intrinsics [V,4] or [4] and world_to_cam [V,3,4] float64 from the
    grid's frame fused into state = (sum, n), int32 HIP tensors [nx,ny,nz] (a slice of tsdf_state), IN PLACE, as
    depth_fuse_weighted_batch describes it: weights = (w_plane, w_proj, w_free, w_empty) in 1 .. 255 (NO DEFAULT, NONE RECOMMENDED),
    normals = None or fp32 [V,H,W,3] (depth_normals of the same views).  -> device int64 [V,7], the voxels per class of
    FUSE_WEIGHTED_CLASS.  Bit-identical to the same problem inside any batch, and to the same views in any order or split over calls."""
    op = "depth_fuse_weighted"
    S, N, _, dims = _fuse_state(op, state, False)
    dev = S.device
    o, h, tr = _fuse_grid(op, 1, origin, voxel, trunc)
    eif, znear, wts = _fuse_empty(op, empty), float(znear), _fuse_weights(op, weights)
    D, K, E = _carve_views(op, depth, intrinsics, world_to_cam, dev)
    Nr = _fuse_normals(op, normals, D, dev)
    views, H, W = D.shape
    vc = torch.empty(views, 7, dtype=torch.int64, device=dev)
    if views == 0:
        return vc
    ws_bytes = load().ls_depth_fuse_weighted_workspace_bytes(*dims, views)
    if ws_bytes == 0:
        raise ValueError(f"{op}: dims {dims} with {views} views unsupported (include/livingscenes_hip.h: nx ny nz < 2^31)")
    ws = _scratch(ws_bytes, dev)
    call(dev, "ls_depth_fuse_weighted_f32", ptr(S), ptr(N), *dims, _hptr(o), float(h[0]), float(tr[0]), ptr(D), ptr(Nr), views, H, W, ptr(K), ptr(E),
         znear, eif, _hptr(wts), ptr(vc), ptr(ws), ws.numel(), stream_ptr(dev))
    return vc


# ------------------------------------------------------------------------------------------------ the fused state completed by the prior (csrc/tsdfprior.hip)
PRIOR_COUNT = ("eligible", "voted", "skipped_nonfinite", "untouched")   # the columns of the counts, by value


def _prior_weight(op, weight):
    if isinstance(weight, bool) or not isinstance(weight, (int, np.integer)) or not 1 <= int(weight) <= 65535:
        raise ValueError(f"{op}: weight is an integer in 1 .. 65535 (the votes the prior tops a sample up to; NONE IS RECOMMENDED), got {weight!r}")
    return int(weight)


def _prior_ws(op, single, P, dims, dev):
    ws_bytes = getattr(load(), "ls_tsdf_prior_rows" + ("" if single else "_batch") + "_workspace_bytes")(*(() if single else (P,)), *dims)
    if ws_bytes == 0:
        raise ValueError(f"{op}: P = {P} problems of dims {dims} unsupported (include/livingscenes_hip.h: P nx ny nz < 2^31, "
                         "nx ny nz <= 4096 blocks of 4096 samples, P <= 65535)")
    return _scratch(ws_bytes, dev)


def _tsdf_prior_rows(op, single, state, origin, voxel, weight, packed):
    S, N, P, dims = _fuse_state(op, state, not single)
    weight = _prior_weight(op, weight)
    o, h = _fuse_grid(op, P, origin, voxel)
    dev = S.device
    ws = _prior_ws(op, single, P, dims, dev)
    name = "ls_" + op + "_f32"
    off = torch.zeros(P + 1, dtype=torch.int64, device=dev)
    counts = torch.empty(P, 4, dtype=torch.int64, device=dev)
    head = (ptr(N), *dims, weight, _hptr(o), float(h[0]) if single else _hptr(h))
    if not single:
        head = (P,) + head
    call(dev, name, *head, None, None, None, 0, ptr(off), ptr(counts), ptr(ws), ws.numel(), stream_ptr(dev))
    ro = off.cpu().tolist()                                              # the one host read
    R = ro[P]
    points = torch.empty(R, 3, dtype=torch.float32, device=dev)
    inst = torch.empty(R, dtype=torch.int32, device=dev)
    index = torch.empty(R, dtype=torch.int32, device=dev)
    if R:
        call(dev, name, *head, ptr(points), ptr(inst), ptr(index), R, ptr(off), ptr(counts), ptr(ws), ws.numel(), stream_ptr(dev))
    if single:
        counts = counts[0]
    if packed or single:
        return points, inst, index, ro, counts
    cut = lambda t: [t[ro[p]:ro[p + 1]] for p in range(P)]                # noqa: E731
    return cut(points), cut(inst), cut(index), ro, counts


def tsdf_prior_rows_batch(state, *, origin, voxel, weight, packed=False):
    """ls_tsdf_prior_rows_batch_f32 (an extension beyond the released reference, like depth_fuse): the lattice samples of P fused states
    that the cameras left short of `weight` observations, as query rows for the shape prior.  state = (sum, n) int32 HIP tensors
    [P,nx,ny,nz] (tsdf_state, depth_fuse_batch; read only); origin [P,3] or [3], voxel (one value or P): host float64, the grids the
    views were fused on; weight: an integer in 1 .. 65535, NO DEFAULT AND NONE RECOMMENDED.  A sample is eligible iff weight - n > 0;
    its row is the float64 position origin_a + voxel * index_a rounded once to fp32: the definition of include/livingscenes_hip.h, by
    equality.  Rows in ascending linear index within a problem, problems in order, so the rows of an instance are contiguous: the
    layout HipModel.sdf_decode_rows takes.
    -> (points fp32 [R,3], row_inst int32 [R], row_index int32 [R]: device tensors; offsets: host list of P+1; counts device int64
    [P,4], the columns of PRIOR_COUNT with voted and skipped still 0) with packed=True; packed=False: the first three as lists of P
    views of the packed tensors.  One sizing call, ONE host read of the offsets, one real call (none where R = 0); no compact list and
    no atomics on the way.  A problem's rows do not depend on the batch."""
    return _tsdf_prior_rows("tsdf_prior_rows_batch", False, state, origin, voxel, weight, packed)


def tsdf_prior_rows(state, *, origin, voxel, weight, packed=False):
    """ls_tsdf_prior_rows_f32: state = (sum, n) int32 HIP tensors [nx,ny,nz] (a slice of tsdf_state), origin [3] and voxel host float64
    -> (points [R,3], row_inst [R] (zeros), row_index [R], offsets [0, R], counts device int64 [4]) as tsdf_prior_rows_batch describes
    them (packed changes nothing for one problem), bit-identical to the same problem anywhere inside any batch."""
    return _tsdf_prior_rows("tsdf_prior_rows", True, state, origin, voxel, weight, packed)


def _tsdf_complete(op, single, state, values, rows, s, trunc, weight):
    S, N, P, dims = _fuse_state(op, state, not single)
    weight = _prior_weight(op, weight)
    dev = S.device
    if not isinstance(rows, (tuple, list)) or len(rows) != 5:
        raise ValueError(f"{op}: rows is what tsdf_prior_rows{'' if single else '_batch'} returned: (points, row_inst, row_index, offsets, counts)")
    ro, rcounts = [int(v) for v in rows[3]], rows[4]
    if len(ro) != P + 1 or ro[0] != 0 or any(b < a for a, b in zip(ro, ro[1:])):
        raise ValueError(f"{op}: the offsets of rows are {P + 1} ascending values from 0 for {P} problems, got {ro}")
    R = ro[P]
    if not torch.is_tensor(values) or values.device.type != "cuda" or values.dtype != torch.float32:
        kind = f"{values.device.type} {values.dtype}" if torch.is_tensor(values) else type(values).__name__
        raise _lib.LsError(f"{op}: values must be an fp32 HIP (cuda) tensor, got {kind}: the MI355X path has no CPU fallback and converts nothing")
    if values.dim() != 1 or values.shape[0] != R or values.device != dev or not values.is_contiguous():
        raise ValueError(f"{op}: values is a contiguous [R] tensor on {dev} with R = {R}, the last offset of rows; got {tuple(values.shape)} on {values.device}")
    sv = np.ascontiguousarray(s.detach().cpu().numpy() if torch.is_tensor(s) else s, dtype=np.float64).reshape(-1)
    if sv.shape[0] == 1 and P > 1:
        sv = np.full(P, sv[0], dtype=np.float64)
    if sv.shape[0] != P or not (np.isfinite(sv) & (sv > 0)).all():
        raise ValueError(f"{op}: s is {P} finite values > 0 (the scale of every instance), got {sv.tolist()}")
    _, _, tr = _fuse_grid(op, P, np.zeros(3), 1.0, trunc)
    if not (np.isfinite(tr) & (tr > 0)).all():
        raise ValueError(f"{op}: trunc must be finite and > 0, got {tr.tolist()}")
    if R == 0:                                                          # nothing to vote on: the completed state is a copy
        counts = rcounts.clone() if torch.is_tensor(rcounts) else torch.as_tensor(np.asarray(rcounts), device=dev)
        return (S.clone(), N.clone()), counts
    ws = _prior_ws(op, single, P, dims, dev)
    So, No = torch.empty_like(S), torch.empty_like(N)
    counts = torch.empty(P, 4, dtype=torch.int64, device=dev)
    tail = (ptr(values), R, ptr(So), ptr(No), ptr(counts), ptr(ws), ws.numel(), stream_ptr(dev))
    if single:
        call(dev, "ls_tsdf_prior_vote_f32", ptr(S), ptr(N), *dims, weight, float(sv[0]), float(tr[0]), *tail)
        return (So, No), counts[0]
    call(dev, "ls_tsdf_prior_vote_batch_f32", P, ptr(S), ptr(N), *dims, weight, _hptr(sv), _hptr(tr), *tail)
    return (So, No), counts


def tsdf_complete_batch(state, values, rows, *, s, trunc, weight):
    """ls_tsdf_prior_vote_batch_f32: the shape prior's field entered into a COPY of P fused states as integer votes.  state = (sum, n)
    int32 HIP tensors [P,nx,ny,nz], never written; rows: what tsdf_prior_rows_batch(state, weight=weight) returned (its offsets are
    checked against values); values fp32 [R] on the device: the decoder's value of every row, in row order; s (one value or P; the
    scale of every instance) and trunc (one value or P): host float64; weight as for the rows.  THE CONVENTION OF tsdf_fit_loss: the
    decoder's value times s is a metric distance with the sign of the fused distance.  Per eligible sample, w = weight - n:
    q = floor(clip(s f / trunc, -1, 1) * 16384 + 0.5), sum' = sum + w q, n' = n + w = weight; a NaN casts no vote, +-inf clamps; every
    other sample keeps (sum, n) bit for bit: the definition of include/livingscenes_hip.h, by equality.
    -> ((sum', n') new int32 tensors of the state's shape -- the format every tsdf_* operator reads, meshed whole with
    min_obs = weight; counts device int64 [P,4] of PRIOR_COUNT).  One call, no host read; R = 0: two copies and no kernel.  An
    eligible sample finds its row by block offset + popcount, so row_index is not read.  NO WEIGHT IS RECOMMENDED."""
    return _tsdf_complete("tsdf_complete_batch", False, state, values, rows, s, trunc, weight)


def tsdf_complete(state, values, rows, *, s, trunc, weight):
    """ls_tsdf_prior_vote_f32: state = (sum, n) int32 HIP tensors [nx,ny,nz], values fp32 [R], rows what tsdf_prior_rows returned, s and
    trunc host float64 -> ((sum', n'), counts device int64 [4]) as tsdf_complete_batch describes them, bit-identical to the same
    problem inside any batch.  NO WEIGHT IS RECOMMENDED."""
    return _tsdf_complete("tsdf_complete", True, state, values, rows, s, trunc, weight)
