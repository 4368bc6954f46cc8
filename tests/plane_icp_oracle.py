"""NumPy twin of the point-to-plane trimmed ICP of csrc/cloudnear.hip (ls_cloud_icp_plane_f32 / ls_cloud_icp_plane_batch_f32) -- not a test
module.  The definition of include/livingscenes_hip.h step by step, on top of nearest_oracle (the search), merge_oracle (the query
expression) and icp_oracle (g_0, the cost expression, the LS_ICP_* values):
  search      nearest_oracle.nearest(A, B, g_k, r) -> f_k, n_k, S_k, idx, d2
  planar      a matched query whose neighbour's row of N is not (0, 0, 0); w_k of them.  y = the posed row in fp32, a the neighbour, n its
              normal, as float64: rho = ((y0 - a0) n0 + (y1 - a1) n1) + (y2 - a2) n2; Q_k = math.fsum(rho^2) (the exactly rounded sum the
              device's chunked float64 sum is held to)
  cost        E_k = (Q_k + (f_k - w_k) * float64(r2)) / f_k; f_k = 0: E_k = 0
  stop tests  in this order, each keeping g_k: w_k < min_matched: STARVED; k >= 1 and E_{k-1} - E_k <= rel_thr * E_{k-1}: CONVERGED;
              k == max_iter: MAX_ITER.  The linearised step may raise E; the loop then ends as CONVERGED with the pose that step produced.
  update      J = (n, y x n), twist order (v, omega); M = sum J J^T, b = -sum J rho (math.fsum each); M xi = b by a hand-written Cholesky,
              column by column, every inner sum from k = 0 upwards; a pivot that is not > 1e-12 * the original diagonal entry, or a
              non-finite value: DEGENERATE, g_k is kept
  retraction  Delta = exp(xi) by Rodrigues with the left Jacobian (first order below theta = 1e-6); R' = R_Delta R_k,
              t' = R_Delta t_k + t_Delta in float64; R' replaced by its polar factor U V^T (R' = U S V^T); both rounded to fp32
`step` is one iteration as the GPU tests compare it with the device's trace, `step_brute` the O(a b) literal reading with plain Python
loops, `icp` the loop."""
import math

import numpy as np

import icp_oracle as io
import nearest_oracle as no
from merge_oracle import transform

CONVERGED, MAX_ITER, STARVED, DEGENERATE = io.CONVERGED, io.MAX_ITER, io.STARVED, io.DEGENERATE
PIVOT = 1e-12
TRIU = [(r, c) for r in range(6) for c in range(r, 6)]


def _arr(X):
    return np.ascontiguousarray(X, dtype=np.float32).reshape(-1, 3)


def planar_mask(N, idx):
    """which queries have a neighbour with a normal"""
    N = _arr(N)
    has = idx >= 0
    out = np.zeros(idx.shape[0], dtype=bool)
    out[has] = (N[idx[has]] != 0).any(1)
    return out


def moments(A, N, B, g, idx):
    """-> (w, Q, M [6,6], b [6]) over the planar matches of the correspondences idx at the pose g"""
    A, N = _arr(A), _arr(N)
    pl = planar_mask(N, idx)
    w = int(pl.sum())
    y = transform(B, g)[pl].astype(np.float64)
    a, n = A[idx[pl]].astype(np.float64), N[idx[pl]].astype(np.float64)
    with np.errstate(all="ignore"):
        rho = ((y[:, 0] - a[:, 0]) * n[:, 0] + (y[:, 1] - a[:, 1]) * n[:, 1]) + (y[:, 2] - a[:, 2]) * n[:, 2]
        J = np.concatenate([n, np.stack([y[:, 1] * n[:, 2] - y[:, 2] * n[:, 1], y[:, 2] * n[:, 0] - y[:, 0] * n[:, 2],
                                         y[:, 0] * n[:, 1] - y[:, 1] * n[:, 0]], 1)], 1)
        Q = _fsum((rho * rho).tolist())
        b = np.array([-_fsum((J[:, r] * rho).tolist()) for r in range(6)])
        M = np.zeros((6, 6))
        for r, c in TRIU:
            M[r, c] = M[c, r] = _fsum((J[:, r] * J[:, c]).tolist())
    return w, Q, M, b


def _fsum(v):
    try:
        return math.fsum(v)
    except (OverflowError, ValueError):                                  # non-finite terms: what a float sum makes of them
        return float(np.sum(np.asarray(v, dtype=np.float64)))


def cholesky_solve(M, b):
    """-> (xi [6] or None, the smallest pivot / original diagonal entry seen before a stop)"""
    L = np.array(M, dtype=np.float64)
    ratio = math.inf
    for j in range(6):
        mjj = float(L[j, j])
        d = mjj
        for k in range(j):
            d -= float(L[j, k]) * float(L[j, k])
        if not math.isfinite(d) or not d > PIVOT * mjj:
            return None, (d / mjj if mjj > 0 and math.isfinite(d) else 0.0)
        ratio = min(ratio, d / mjj)
        l = math.sqrt(d)
        L[j, j] = l
        for i in range(j + 1, 6):
            v = float(L[i, j])
            for k in range(j):
                v -= float(L[i, k]) * float(L[j, k])
            L[i, j] = v / l
    z, xi = [0.0] * 6, [0.0] * 6
    for i in range(6):
        v = float(b[i])
        for k in range(i):
            v -= float(L[i, k]) * z[k]
        z[i] = v / float(L[i, i])
    for i in range(5, -1, -1):
        v = z[i]
        for k in range(i + 1, 6):
            v -= float(L[k, i]) * xi[k]
        xi[i] = v / float(L[i, i])
    if not all(math.isfinite(v) for v in xi):
        return None, ratio
    return np.array(xi), ratio


def se3_exp(xi):
    """the twist (v, omega) -> (R [3,3], t [3]) in float64, More_Solver's _se3_exp"""
    v, w = xi[:3], xi[3:]
    th = math.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-6:
        R, V = np.eye(3) + K, np.eye(3) + 0.5 * K
    else:
        ca, cb, cc = math.sin(th) / th, (1.0 - math.cos(th)) / (th * th), (th - math.sin(th)) / (th * th * th)
        R, V = np.eye(3) + ca * K + cb * (K @ K), np.eye(3) + cb * K + cc * (K @ K)
    return R, V @ v


def retract(g, xi):
    """g_{k+1} [3,4] float32 from g_k [3,4] float32 and the twist, or None if anything is non-finite"""
    g = np.asarray(g, dtype=np.float32).astype(np.float64)
    Rd, td = se3_exp(xi)
    R, t = Rd @ g[:, :3], Rd @ g[:, 3] + td
    if not (np.isfinite(R).all() and np.isfinite(t).all()):
        return None
    U, _, Vt = np.linalg.svd(R)
    return np.concatenate([U @ Vt, t[:, None]], 1).astype(np.float32)


def _out(A, N, B, g, r, idx, d2, counts, S, w, Q, M, b):
    f, n = int(counts[0]), int(counts[1])
    out = {"idx": idx, "d2": d2, "counts": counts, "f": f, "n": n, "S": S, "w": w, "Q": Q, "E": io.cost(f, w, Q, r), "M": M, "b": b,
           "g_next": None, "xi": None, "pivot": 0.0}
    if w >= 1:
        out["xi"], out["pivot"] = cholesky_solve(M, b)
        if out["xi"] is not None:
            out["g_next"] = retract(g, out["xi"])
    return out


def step(A, N, B, g, r, search=no.nearest):
    """one iteration at the pose g (a [3,4] matrix) -> dict: idx, d2, counts, f, n, S, w, Q, E, M, b, xi, pivot (the smallest pivot ratio)
    and g_next (None: degenerate)"""
    idx, d2, counts, S = search(A, B, g, r)
    w, Q, M, b = moments(A, N, B, g, idx)
    return _out(A, N, B, g, r, idx, d2, counts, S, w, Q, M, b)


def step_brute(A, N, B, g, r):
    """`step` read literally: the O(a b) search and plain Python loops for the sums"""
    A, N = _arr(A), _arr(N)
    idx, d2, counts, S = no.nearest_brute(A, B, g, r)
    Y = transform(B, g)
    w, rho2, Jr, JJ = 0, [], [[] for _ in range(6)], {rc: [] for rc in TRIU}
    for i in range(Y.shape[0]):
        if idx[i] < 0 or not (N[idx[i]] != 0).any():
            continue
        w += 1
        y, a, n = ([float(v) for v in X] for X in (Y[i], A[idx[i]], N[idx[i]]))
        rho = ((y[0] - a[0]) * n[0] + (y[1] - a[1]) * n[1]) + (y[2] - a[2]) * n[2]
        J = n + [y[1] * n[2] - y[2] * n[1], y[2] * n[0] - y[0] * n[2], y[0] * n[1] - y[1] * n[0]]
        rho2.append(rho * rho)
        for u in range(6):
            Jr[u].append(J[u] * rho)
        for u, v in TRIU:
            JJ[(u, v)].append(J[u] * J[v])
    M = np.zeros((6, 6))
    for u, v in TRIU:
        M[u, v] = M[v, u] = _fsum(JJ[(u, v)])
    b = np.array([-_fsum(v) for v in Jr])
    return _out(A, N, B, g, r, idx, d2, counts, S, w, _fsum(rho2), M, b)


def stop_rule(k, w, E, E_prev, max_iter, rel_thr, min_matched):
    """the stop tests of iteration k before the update, on the PLANAR count -> STARVED / CONVERGED / MAX_ITER or None (go on)"""
    return io.stop_rule(k, w, E, E_prev, max_iter, rel_thr, min_matched)


def icp(A, N, B, g0, r, max_iter=100, rel_thr=1e-6, min_matched=6):
    """-> dict: g [3,4] float32, stop, iters, the final search (idx, d2, counts, sum_d2), planar, sum_rho2 and the trace: g_trace [iters+1]
    poses, stat_trace [iters+1] (f, n, S, w, Q), E [iters+1]"""
    g = io.pose0(g0)
    E_prev = 0.0
    gs, stats, Es = [], [], []
    k = 0
    while True:
        s = step(A, N, B, g, r)
        gs.append(g)
        stats.append((s["f"], s["n"], s["S"], s["w"], s["Q"]))
        Es.append(s["E"])
        why = stop_rule(k, s["w"], s["E"], E_prev, max_iter, rel_thr, min_matched)
        if why is None and s["g_next"] is None:
            why = DEGENERATE
        if why is not None:
            return {"g": g, "stop": why, "iters": k, "idx": s["idx"], "d2": s["d2"], "counts": s["counts"], "sum_d2": s["S"],
                    "planar": s["w"], "sum_rho2": s["Q"], "g_trace": gs, "stat_trace": stats, "E": Es}
        g, E_prev = s["g_next"], s["E"]
        k += 1


def icp_batch(As, Ns, Bs, gs, rs, **kw):
    return [icp(A, N, B, None if gs is None else gs[p], rs[p], **kw) for p, (A, N, B) in enumerate(zip(As, Ns, Bs))]
