"""NumPy twin of the scene memory's sampling of a fused state and of the registration on it (csrc/tsdficp.hip: ls_tsdf_sample_f32 /
ls_tsdf_icp_f32 and their batch forms) -- not a test module.  The definition of include/livingscenes_hip.h step by step, the same text as
csrc/tsdfsample_plan.h: float64 throughout, every product and sum rounded on its own (NumPy never contracts), so the header and the kernels
are held to it by equality.
  posed query   merge_oracle.transform(B, g): fp32, the expression of ls_cloud_merge_f32; g None: B bit for bit
  cell          u_a = (double(y_a) - origin_a) / h; OUT unless y is finite, every dim >= 2 and 0 <= u_a <= n_a - 1 on every axis;
                i_a = min(floor(u_a), n_a - 2), f_a = u_a - i_a
  corners       UNSEEN if one of the eight has n < min_obs, else SAMPLED; D = fuse_oracle.volume's expression
  value         lerp(a, b, f) = a + f * (b - a) along axis 2, then 1, then 0; phi = trunc * D_interp
  gradient      G_2 = lerp_0(lerp_1(D[..1] - D[..0])), G_1 = lerp_0(lerp_2(D[.1.] - D[.0.])), G_0 = lerp_1(lerp_2(D[1..] - D[0..]));
                grad_a = (trunc / h) * G_a, trunc / h formed once
  sums          chunk_sum: chunks of 256 consecutive queries of the problem, a fixed tree over each 64 (l with l + 32, l + 16, ...), a fixed
                tree over the four ((w0 + w1) + (w2 + w3)), the chunk records added in chunk order
  registration  per iteration the sample, E = (Q + (f - w) trunc^2) / f, the stop tests and the update of plane_icp_oracle with
                rho = phi and J = (grad, y x grad): the solver text is the same (cholesky_solve, retract)."""
import math

import numpy as np

import icp_oracle as io
import plane_icp_oracle as po
from fuse_oracle import SCALE
from merge_oracle import transform

OUT, UNSEEN, SAMPLED = 0, 1, 2
CHUNK, WAVE = 256, 64
CONVERGED, MAX_ITER, STARVED, DEGENERATE = io.CONVERGED, io.MAX_ITER, io.STARVED, io.DEGENERATE


def lerp(a, b, f):
    return a + f * (b - a)


def corner_values(state, min_obs):
    """-> (D float64 [nx,ny,nz], valid bool): D = sum / (n * 16384) where n >= min_obs, else exactly 1.0"""
    S, N = state
    valid = N >= int(min_obs)
    with np.errstate(all="ignore"):
        D = np.where(valid, S.astype(np.float64) / (np.maximum(N, 1).astype(np.float64) * np.float64(SCALE)), 1.0)
    return D, valid


def interpolate(D8, f):
    """D8 [m,2,2,2] float64 (alpha, beta, gamma), f [m,3] -> (D_interp [m], G [m,3]) in the stated order of operations"""
    f0, f1, f2 = f[:, 0], f[:, 1], f[:, 2]
    a = lerp(D8[:, :, :, 0], D8[:, :, :, 1], f2[:, None, None])          # [m, alpha, beta]
    b = lerp(a[:, :, 0], a[:, :, 1], f1[:, None])                        # [m, alpha]
    v = lerp(b[:, 0], b[:, 1], f0)
    d2 = D8[:, :, :, 1] - D8[:, :, :, 0]                                 # [m, alpha, beta]
    d1 = D8[:, :, 1, :] - D8[:, :, 0, :]                                 # [m, alpha, gamma]
    d0 = D8[:, 1, :, :] - D8[:, 0, :, :]                                 # [m, beta, gamma]
    e2 = lerp(d2[:, :, 0], d2[:, :, 1], f1[:, None])
    G2 = lerp(e2[:, 0], e2[:, 1], f0)
    e1 = lerp(d1[:, :, 0], d1[:, :, 1], f2[:, None])
    G1 = lerp(e1[:, 0], e1[:, 1], f0)
    e0 = lerp(d0[:, :, 0], d0[:, :, 1], f2[:, None])
    G0 = lerp(e0[:, 0], e0[:, 1], f1)
    return v, np.stack([G0, G1, G2], 1)


def chunk_sum(v):
    """the float64 sum of the definition over the values v [b] of ONE problem (zeros where a query adds nothing)"""
    v = np.asarray(v, np.float64).reshape(-1)
    total = np.float64(0.0)
    for c in range(0, v.shape[0], CHUNK):
        part = np.zeros(CHUNK, np.float64)
        part[:min(CHUNK, v.shape[0] - c)] = v[c:c + CHUNK]
        w = part.reshape(CHUNK // WAVE, WAVE).copy()
        o = WAVE // 2
        while o > 0:
            w[:, :o] = w[:, :o] + w[:, o:2 * o]
            o //= 2
        total = total + ((w[0, 0] + w[1, 0]) + (w[2, 0] + w[3, 0]))
    return float(total)


def sample(state, B, g, origin, voxel, trunc, min_obs=1):
    """-> dict: phi [b] float64, grad [b,3] float64, state [b] uint8, counts int64 [3] = (finite, inside, sampled), sum_phi2 (the
    chunk-ordered sum), y [b,3] the posed queries (fp32)"""
    S, N = state
    dims = S.shape
    origin, h, trunc = np.asarray(origin, np.float64).reshape(3), np.float64(voxel), np.float64(trunc)
    toh = trunc / h
    y = transform(B, g)
    b = y.shape[0]
    finite = np.isfinite(y).all(1)
    inside = finite & (min(dims) >= 2)
    idx, f = np.zeros((b, 3), np.int64), np.zeros((b, 3), np.float64)
    with np.errstate(all="ignore"):
        for a in range(3):
            u = (y[:, a].astype(np.float64) - origin[a]) / h
            ok = (u >= 0.0) & (u <= np.float64(dims[a] - 1))
            inside &= ok
            ia = np.minimum(np.floor(np.where(ok, u, 0.0)).astype(np.int64), dims[a] - 2)
            idx[:, a], f[:, a] = ia, u - ia.astype(np.float64)
    phi, grad, st = np.full(b, trunc, np.float64), np.zeros((b, 3), np.float64), np.zeros(b, np.uint8)
    st[inside] = UNSEEN
    if inside.any():
        D, valid = corner_values(state, min_obs)
        q = np.flatnonzero(inside)
        i0, i1, i2 = idx[q, 0], idx[q, 1], idx[q, 2]
        D8, V8 = np.zeros((q.size, 2, 2, 2)), np.zeros((q.size, 2, 2, 2), bool)
        for al in range(2):
            for be in range(2):
                for ga in range(2):
                    D8[:, al, be, ga] = D[i0 + al, i1 + be, i2 + ga]
                    V8[:, al, be, ga] = valid[i0 + al, i1 + be, i2 + ga]
        seen = V8.reshape(-1, 8).all(1)
        v, G = interpolate(D8[seen], f[q][seen])
        qs = q[seen]
        phi[qs], grad[qs], st[qs] = trunc * v, toh * G, SAMPLED
    counts = np.array([finite.sum(), inside.sum(), (st == SAMPLED).sum()], np.int64)
    return {"phi": phi, "grad": grad, "state": st, "counts": counts, "sum_phi2": chunk_sum(np.where(st == SAMPLED, phi * phi, 0.0)), "y": y}


def cost(f, w, Q, trunc):
    trunc = float(trunc)
    return (Q + float(f - w) * (trunc * trunc)) / float(f) if f > 0 else 0.0


def moments(s):
    """the sums of the update over the SAMPLED queries of the sample s -> (Q, M [6,6], b [6]), math.fsum each"""
    m = s["state"] == SAMPLED
    y, n, rho = s["y"][m].astype(np.float64), s["grad"][m], s["phi"][m]
    with np.errstate(all="ignore"):
        J = np.concatenate([n, np.stack([y[:, 1] * n[:, 2] - y[:, 2] * n[:, 1], y[:, 2] * n[:, 0] - y[:, 0] * n[:, 2],
                                         y[:, 0] * n[:, 1] - y[:, 1] * n[:, 0]], 1)], 1)
        Q = po._fsum((rho * rho).tolist())
        b = np.array([-po._fsum((J[:, r] * rho).tolist()) for r in range(6)])
        M = np.zeros((6, 6))
        for r, c in po.TRIU:
            M[r, c] = M[c, r] = po._fsum((J[:, r] * J[:, c]).tolist())
    return Q, M, b


def record(s, rows=slice(None)):
    """the 28 moments of the definition added by the chunk rule over the queries `rows` of the sample s: what one Gauss-Newton record
    (or, over a whole problem, the sum of its records) holds -> float64 [28]"""
    m = (s["state"] == SAMPLED)[rows]
    y = np.where(m[:, None], s["y"][rows].astype(np.float64), 0.0)
    n, rho = np.where(m[:, None], s["grad"][rows], 0.0), np.where(m, s["phi"][rows], 0.0)
    J = np.concatenate([n, np.stack([y[:, 1] * n[:, 2] - y[:, 2] * n[:, 1], y[:, 2] * n[:, 0] - y[:, 0] * n[:, 2],
                                     y[:, 0] * n[:, 1] - y[:, 1] * n[:, 0]], 1)], 1)
    cols = [rho * rho] + [J[:, r] * rho for r in range(6)] + [J[:, r] * J[:, c] for r, c in po.TRIU]
    return np.array([chunk_sum(c) for c in cols])


def step(state, B, g, origin, voxel, trunc, min_obs=1):
    """one iteration at the pose g (a [3,4] matrix) -> the sample's dict plus f, w, Q (math.fsum), E, M, b, xi, pivot and g_next (None:
    degenerate)"""
    s = sample(state, B, g, origin, voxel, trunc, min_obs)
    f, w = int(s["counts"][0]), int(s["counts"][2])
    Q, M, b = moments(s)
    s.update({"f": f, "w": w, "Q": Q, "E": cost(f, w, Q, trunc), "M": M, "b": b, "g_next": None, "xi": None, "pivot": 0.0})
    if w >= 1:
        s["xi"], s["pivot"] = po.cholesky_solve(M, b)
        if s["xi"] is not None:
            s["g_next"] = po.retract(g, s["xi"])
    return s


def icp(state, B, g0, origin, voxel, trunc, min_obs=1, max_iter=100, rel_thr=1e-6, min_matched=6):
    """-> dict: g [3,4] float32, stop, iters, the final sample (phi, grad, state, counts, sum_phi2) and the trace: g_trace [iters+1] poses,
    stat_trace [iters+1] (f, w, Q), E [iters+1]"""
    g = io.pose0(g0)
    E_prev, gs, stats, Es, k = 0.0, [], [], [], 0
    while True:
        s = step(state, B, g, origin, voxel, trunc, min_obs)
        gs.append(g)
        stats.append((s["f"], s["w"], s["Q"]))
        Es.append(s["E"])
        why = po.stop_rule(k, s["w"], s["E"], E_prev, max_iter, rel_thr, min_matched)
        if why is None and s["g_next"] is None:
            why = DEGENERATE
        if why is not None:
            return {"g": g, "stop": why, "iters": k, "phi": s["phi"], "grad": s["grad"], "state": s["state"], "counts": s["counts"],
                    "sum_phi2": s["sum_phi2"], "g_trace": gs, "stat_trace": stats, "E": Es}
        g, E_prev = s["g_next"], s["E"]
        k += 1
