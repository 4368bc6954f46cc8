"""NumPy twin of the trimmed ICP of csrc/cloudnear.hip (ls_cloud_icp_f32 / ls_cloud_icp_batch_f32) -- not a test module.
The definition of include/livingscenes_hip.h step by step, on top of nearest_oracle (the search) and merge_oracle (the query expression):
  g_0         the given pose; None: the identity MATRIX, which goes through the query expression like any other pose
  search      nearest_oracle.nearest(A, B, g_k, r) -> f_k finite queries, n_k matched queries, S_k = math.fsum of the matched d2 in float64
              (the exactly rounded sum the device's chunked float64 sum is held to)
  cost        E_k = (S_k + (f_k - n_k) * float64(r2)) / f_k, r2 = float32(r) * float32(r); f_k = 0: E_k = 0
  stop tests  in this order, each keeping g_k: n_k < min_matched: STARVED; k >= 1 and E_{k-1} - E_k <= rel_thr * E_{k-1}: CONVERGED;
              k == max_iter: MAX_ITER
  update      over the matched queries, the ORIGINAL rows x_i of B and their neighbours a_j in float64: sx = sum x, sa = sum a,
              sxa = sum x a^T (math.fsum each: exactly rounded), H = sxa - sx sa^T / n, R = V diag(1, 1, det(V U^T)) U^T for H = U S V^T --
              the rotation of ls_kabsch_batched_f32 for the covariance H (x -> a) -- rounded to fp32; t = sa / n - R_fp32 (sx / n) in
              float64, rounded to fp32.  A second singular value that is not > 1e-150, or a non-finite H: DEGENERATE, g_k is kept.
`step` is one iteration (search, sums, update) as the GPU tests compare it with the device's trace; `step_brute` the O(a b) literal reading
of it; `icp` the loop."""
import math

import numpy as np

import nearest_oracle as no
from merge_oracle import transform

CONVERGED, MAX_ITER, STARVED, DEGENERATE = 0, 1, 2, 3      # LS_ICP_* of include/livingscenes_hip.h
IDENTITY = np.concatenate([np.eye(3), np.zeros((3, 1))], 1).astype(np.float32)


def pose0(g):
    return IDENTITY.copy() if g is None else np.ascontiguousarray(g, dtype=np.float32).reshape(-1, 4)[:3]


def images(B, g):
    """the rows of B under the pose g by the query expression of the definition (None: the identity matrix)"""
    return transform(B, pose0(g))


def cost(f, n, S, r):
    r = np.float32(r)
    r2 = float(r * r)
    return (S + float(f - n) * r2) / float(f) if f > 0 else 0.0


def _fsum_cols(M):
    return np.array([math.fsum(col.tolist()) for col in M.T], dtype=np.float64)


def kabsch(H):
    """-> (R [3,3] float32 or None, singular values): R = V diag(1, 1, det(V U^T)) U^T maps x onto a for H = sum (x - mx)(a - ma)^T"""
    if not np.isfinite(H).all():
        return None, np.full(3, np.nan)
    U, s, Vt = np.linalg.svd(H)
    if not s[1] > 1e-150:
        return None, s
    V = Vt.T
    d = np.sign(np.linalg.det(V @ U.T))
    return (V @ np.diag([1.0, 1.0, d]) @ U.T).astype(np.float32), s


def update(A, B, idx):
    """the float64 update from the correspondences idx (-1: none) -> (g_next [3,4] float32 or None, H, mu_x, mu_a)"""
    A = np.ascontiguousarray(A, dtype=np.float32).reshape(-1, 3)
    B = np.ascontiguousarray(B, dtype=np.float32).reshape(-1, 3)
    has = idx >= 0
    n = int(has.sum())
    X, Y = B[has].astype(np.float64), A[idx[has]].astype(np.float64)
    sx, sa = _fsum_cols(X), _fsum_cols(Y)
    sxa = _fsum_cols((X[:, :, None] * Y[:, None, :]).reshape(n, 9)).reshape(3, 3)
    with np.errstate(all="ignore"):
        H = sxa - np.outer(sx, sa) / n
        mx, ma = sx / n, sa / n
    R, _ = kabsch(H)
    if R is None:
        return None, H, mx, ma
    t = (ma - R.astype(np.float64) @ mx).astype(np.float32)
    return np.concatenate([R, t[:, None]], 1), H, mx, ma


def step(A, B, g, r, search=no.nearest):
    """one iteration at the pose g (a [3,4] matrix) -> dict: idx, d2, counts, f, n, S, E, and g_next / H / mu_x / mu_a when n >= 1"""
    idx, d2, counts, S = search(A, B, g, r)
    f, n = int(counts[0]), int(counts[1])
    out = {"idx": idx, "d2": d2, "counts": counts, "f": f, "n": n, "S": S, "E": cost(f, n, S, r), "g_next": None}
    if n >= 1:
        out["g_next"], out["H"], out["mu_x"], out["mu_a"] = update(A, B, idx)
    return out


def step_brute(A, B, g, r):
    """`step` read literally: the O(a b) search and plain Python loops for the sums"""
    A = np.ascontiguousarray(A, dtype=np.float32).reshape(-1, 3)
    B = np.ascontiguousarray(B, dtype=np.float32).reshape(-1, 3)
    idx, d2, counts, S = no.nearest_brute(A, B, g, r)
    f, n = int(counts[0]), int(counts[1])
    sx, sa, sxa = [[] for _ in range(3)], [[] for _ in range(3)], [[] for _ in range(9)]
    for i in range(B.shape[0]):
        if idx[i] < 0:
            continue
        x, a = [float(v) for v in B[i]], [float(v) for v in A[idx[i]]]
        for u in range(3):
            sx[u].append(x[u])
            sa[u].append(a[u])
            for v in range(3):
                sxa[u * 3 + v].append(x[u] * a[v])
    out = {"idx": idx, "d2": d2, "counts": counts, "f": f, "n": n, "S": S, "E": cost(f, n, S, r), "g_next": None}
    if n >= 1:
        sx, sa = np.array([math.fsum(v) for v in sx]), np.array([math.fsum(v) for v in sa])
        H = np.array([math.fsum(v) for v in sxa]).reshape(3, 3) - np.outer(sx, sa) / n
        R, _ = kabsch(H)
        if R is not None:
            t = (sa / n - R.astype(np.float64) @ (sx / n)).astype(np.float32)
            out["g_next"] = np.concatenate([R, t[:, None]], 1)
        out["H"] = H
    return out


def stop_rule(k, n, E, E_prev, max_iter, rel_thr, min_matched):
    """the stop tests of iteration k before the update -> STARVED / CONVERGED / MAX_ITER or None (go on)"""
    if n < min_matched:
        return STARVED
    if k >= 1 and E_prev - E <= rel_thr * E_prev:
        return CONVERGED
    if k == max_iter:
        return MAX_ITER
    return None


def icp(A, B, g0, r, max_iter=100, rel_thr=1e-6, min_matched=3):
    """-> dict: g [3,4] float32, stop, iters, the final search (idx, d2, counts, sum_d2) and the trace: g_trace [iters+1] poses,
    stat_trace [iters+1] (f, n, S), E [iters+1]"""
    g = pose0(g0)
    E_prev = 0.0
    gs, stats, Es = [], [], []
    k = 0
    while True:
        s = step(A, B, g, r)
        gs.append(g)
        stats.append((s["f"], s["n"], s["S"]))
        Es.append(s["E"])
        why = stop_rule(k, s["n"], s["E"], E_prev, max_iter, rel_thr, min_matched)
        if why is None and s["g_next"] is None:
            why = DEGENERATE
        if why is not None:
            return {"g": g, "stop": why, "iters": k, "idx": s["idx"], "d2": s["d2"], "counts": s["counts"], "sum_d2": s["S"],
                    "g_trace": gs, "stat_trace": stats, "E": Es}
        g, E_prev = s["g_next"], s["E"]
        k += 1


def icp_batch(As, Bs, gs, rs, **kw):
    return [icp(A, B, None if gs is None else gs[p], rs[p], **kw) for p, (A, B) in enumerate(zip(As, Bs))]
