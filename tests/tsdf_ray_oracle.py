"""NumPy twin of the scene memory's raycast of a fused state and of the view comparison (csrc/tsdfray.hip: ls_tsdf_raycast_f64 /
ls_tsdf_raycast_batch_f64, ls_depth_compare_f32) -- not a test module.  The definition of include/livingscenes_hip.h step by step, the same
text as csrc/tsdfray_plan.h: float64 throughout, every product and sum rounded on its own (NumPy never contracts), so the header and the
kernels are held to it by equality.  The value at a point is tsdf_sample_oracle's: corner_values and interpolate.
  ray           rx = (px - cx) / fx, ry = (py - cy) / fy; a_a = (M[a,3] - origin_a) / h; b_a = ((M[a,0] rx + M[a,1] ry) + M[a,2]) / h;
                u_a(z) = a_a + z b_a: the ray parameter is the camera depth
  slab          per axis with b_a != 0 the quotients (0 - a_a) / b_a and (n_a - 1 - a_a) / b_a; z_in = max(znear, the largest minimum),
                z_out = the smallest maximum; OUTSIDE: a value not finite, a dim < 2, max |b_a| = 0, an axis with b_a = 0 and a_a outside,
                !(z_in <= z_out)
  march         dz = step / max |b_a|, K = floor((z_out - z_in) / dz) capped at max_trips - 1, z_k = z_in + k dz
  sample        u clamped to [0, n_a - 1], i_a = min(floor(u_a), n_a - 2), f_a = u_a - i_a; SAMPLED iff all eight corners have n >= min_obs
  ray           stop at the first SAMPLED sample with phi <= 0: HIT if the sample before it was SAMPLED with phi > 0, with
                z* = z_{k-1} + dz (phi_{k-1} / (phi_{k-1} - phi_k)), else BEHIND; never stopped: FREE if every sample was SAMPLED, else UNSEEN
  hit           depth = fp32(z*); one more sample at z*: normal = fp32(grad_a / sqrt((g0 g0 + g1 g1) + g2 g2)) where SAMPLED and > 0
No secant iteration, no empty-space skipping."""
import math

import numpy as np

from tsdf_sample_oracle import corner_values, interpolate

OUTSIDE, FREE, UNSEEN, BEHIND, HIT = range(5)
NO_OBS, UNKNOWN, AGREE, IN_FRONT, THROUGH = range(5)
RAY_STATE = ("outside", "free", "unseen", "behind", "hit")
VIEW_CLASS = ("no_obs", "unknown", "agree", "in_front", "through")
TILE = 16


def max_trips(dims, step):
    return int(math.ceil(float(max(dims) - 1) / float(step))) + 2


def _sample(D, valid, a, b, z, dims):
    """the samples at depths z [m] of the rays (a, b) [m,3] -> (sampled bool [m], D_interp [m], G [m,3])"""
    m = z.shape[0]
    idx, f = np.zeros((m, 3), np.int64), np.zeros((m, 3), np.float64)
    with np.errstate(all="ignore"):
        for r in range(3):
            u = a[:, r] + z * b[:, r]
            far = np.float64(dims[r] - 1)
            u = np.where(~(u >= 0.0), 0.0, np.where(u > far, far, u))
            ir = np.minimum(np.floor(u).astype(np.int64), dims[r] - 2)
            idx[:, r], f[:, r] = ir, u - ir.astype(np.float64)
    D8, V8 = np.zeros((m, 2, 2, 2)), np.zeros((m, 2, 2, 2), bool)
    for al in range(2):
        for be in range(2):
            for ga in range(2):
                D8[:, al, be, ga] = D[idx[:, 0] + al, idx[:, 1] + be, idx[:, 2] + ga]
                V8[:, al, be, ga] = valid[idx[:, 0] + al, idx[:, 1] + be, idx[:, 2] + ga]
    v, G = interpolate(D8, f)
    return V8.reshape(m, 8).all(1), v, G


def raycast(state, cam_to_world, intrinsics, height, width, origin, voxel, trunc, min_obs=1, step=0.5, znear=0.05):
    """state (sum, n) int32 [nx,ny,nz]; cam_to_world [V,3,4], intrinsics [V,4] or [4] float64 -> dict: depth fp32 [V,H,W], normal fp32
    [V,H,W,3], state uint8 [V,H,W], counts int64 [V,5]"""
    S, N = state
    dims = S.shape
    Ms = np.asarray(cam_to_world, np.float64).reshape(-1, 3, 4)
    V = Ms.shape[0]
    Ks = np.broadcast_to(np.asarray(intrinsics, np.float64), (V, 4))
    origin, h, trunc, step, znear = np.asarray(origin, np.float64).reshape(3), np.float64(voxel), np.float64(trunc), np.float64(step), np.float64(znear)
    toh = trunc / h
    H, W = int(height), int(width)
    depth, normal = np.zeros((V, H, W), np.float32), np.zeros((V, H, W, 3), np.float32)
    st, counts = np.zeros((V, H, W), np.uint8), np.zeros((V, 5), np.int64)
    D, valid = corner_values(state, min_obs) if min(dims) >= 2 else (None, None)
    cap = np.float64(max_trips(dims, step) - 1)
    py, px = (t.reshape(-1).astype(np.float64) for t in np.mgrid[0:H, 0:W])
    for v in range(V):
        M, (fx, fy, cx, cy) = Ms[v], Ks[v]
        with np.errstate(all="ignore"):
            rx, ry = (px - cx) / fx, (py - cy) / fy
            a = np.stack([np.broadcast_to((M[r, 3] - origin[r]) / h, rx.shape) for r in range(3)], 1)
            b = np.stack([((M[r, 0] * rx + M[r, 1] * ry) + M[r, 2]) / h for r in range(3)], 1)
            ok = np.isfinite(a).all(1) & np.isfinite(b).all(1) & (min(dims) >= 2)
            lo, hi, bmax = np.full(rx.shape, znear), np.full(rx.shape, np.inf), np.zeros(rx.shape)
            for r in range(3):
                far = np.float64(dims[r] - 1)
                zero = b[:, r] == 0.0
                ok &= ~zero | ((a[:, r] >= 0.0) & (a[:, r] <= far))
                q0, q1 = (0.0 - a[:, r]) / b[:, r], (far - a[:, r]) / b[:, r]
                ok &= zero | (np.isfinite(q0) & np.isfinite(q1))
                mn, mx = np.where(q0 < q1, q0, q1), np.where(q0 < q1, q1, q0)
                lo = np.where(~zero & (mn > lo), mn, lo)
                hi = np.where(~zero & (mx < hi), mx, hi)
                bmax = np.where(~zero & (np.abs(b[:, r]) > bmax), np.abs(b[:, r]), bmax)
            ok &= (bmax != 0.0) & (lo <= hi)
            dz = step / bmax
            q = (hi - lo) / dz
            ok &= np.isfinite(dz) & np.isfinite(q)
            K = np.where(ok, np.floor(np.where(q < cap, q, cap)), -1.0)
        K = np.nan_to_num(K, nan=-1.0).astype(np.int64)
        m = rx.shape[0]
        state_v = np.where(ok, -1, OUTSIDE)
        prev_sampled, all_sampled = np.zeros(m, bool), np.ones(m, bool)
        phi_prev, z_star = np.zeros(m), np.zeros(m)
        for k in range(int(K.max()) + 1 if m else 0):
            live = np.flatnonzero((state_v < 0) & (K >= k))
            if live.size == 0:
                break
            z = lo[live] + np.float64(k) * dz[live]
            sampled, val, _ = _sample(D, valid, a[live], b[live], z, dims)
            phi = np.where(sampled, trunc * val, trunc)
            stop = sampled & (phi <= 0.0)
            hit = stop & prev_sampled[live] & (phi_prev[live] > 0.0) & (k > 0)
            with np.errstate(all="ignore"):
                zs = (lo[live] + np.float64(k - 1) * dz[live]) + dz[live] * (phi_prev[live] / (phi_prev[live] - phi))
            z_star[live[hit]] = zs[hit]
            state_v[live[stop]] = np.where(hit[stop], HIT, BEHIND)
            go = live[~stop]
            prev_sampled[go], phi_prev[go] = sampled[~stop], phi[~stop]
            all_sampled[go] &= sampled[~stop]
        never = state_v < 0
        state_v[never] = np.where(all_sampled[never], FREE, UNSEEN)
        hits = np.flatnonzero(state_v == HIT)
        d, nrm = np.zeros(m, np.float32), np.zeros((m, 3), np.float32)
        if hits.size:
            sampled, _, G = _sample(D, valid, a[hits], b[hits], z_star[hits], dims)
            g = toh * G
            gg = (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]
            good = sampled & (gg > 0.0)
            with np.errstate(all="ignore"):
                unit = (g / np.sqrt(gg)[:, None]).astype(np.float32)
            nrm[hits] = np.where(good[:, None], unit, np.float32(0.0))
            d[hits] = z_star[hits].astype(np.float32)
        depth[v], normal[v], st[v] = d.reshape(H, W), nrm.reshape(H, W, 3), state_v.astype(np.uint8).reshape(H, W)
        counts[v] = np.bincount(state_v, minlength=5)
    return {"depth": depth, "normal": normal, "state": st, "counts": counts}


def compare(observed, depth, state, tol):
    """observed, depth fp32 [V,H,W], state uint8 [V,H,W] -> (cls uint8 [V,H,W], counts int64 [V,5])"""
    obs, pred = np.asarray(observed, np.float32).astype(np.float64), np.asarray(depth, np.float32).astype(np.float64)
    state, tol = np.asarray(state), np.float64(tol)
    with np.errstate(all="ignore"):
        s = obs - pred
        cls = np.where(s < -tol, IN_FRONT, np.where(s > tol, THROUGH, AGREE))
    cls = np.where(state != HIT, UNKNOWN, cls)
    cls = np.where(~(obs > 0.0), NO_OBS, cls).astype(np.uint8)
    V = cls.shape[0]
    return cls, np.stack([np.bincount(cls[v].reshape(-1), minlength=5) for v in range(V)]).astype(np.int64).reshape(V, 5)


def agreement(counts):
    """counts [5] of one or more views summed -> (agree or None, through, in_front)"""
    c = np.asarray(counts, np.int64).reshape(-1, 5).sum(0)
    den = int(c[AGREE] + c[IN_FRONT] + c[THROUGH])
    return (float(c[AGREE]) / float(den) if den else None), int(c[THROUGH]), int(c[IN_FRONT])
