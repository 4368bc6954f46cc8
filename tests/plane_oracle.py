"""The NumPy twin of the normals of a depth map and of the weighted point-to-plane depth fusion (csrc/depthplane.hip, csrc/plane_plan.h:
ls_depth_normals_f32, ls_depth_fuse_weighted_f32 / ls_depth_fuse_weighted_batch_f32) -- not a test module.  The definitions of
include/livingscenes_hip.h step by step: float64 comparisons and integer sums throughout, every product and sum rounded on its own (NumPy
never contracts), so the header and the kernels are held to it by equality.  Steps 1 - 5 of the weighted fuse are the fuse's:
fuse_oracle.positions and fuse_oracle.view_classes give the class and the projective q; only the pixel a NEAR voxel-view reads its plane
from is formed here again, by the same expressions."""
import numpy as np

import fuse_oracle as fo

NO_DEPTH, VALID, NO_NEIGHBOUR, DEGENERATE = range(4)
STATES = 4
OUT, EMPTY, OCCLUDED, NEAR_PLANE, NEAR_PROJ, FREE, SATURATED = range(7)
CLASSES = 7
SCALE, MAX_OBS = fo.SCALE, fo.MAX_OBS
MAX_WEIGHT = 255


def _shift(a, dx, dy, fill):
    """a [H,W] read at (x + dx, y + dy); `fill` outside the image"""
    H, W = a.shape
    out = np.full_like(a, fill)
    ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
    xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
    out[yd, xd] = a[ys, xs]
    return out


def points(d, K):
    """P(x, y) = (d * ((double)x - cx) / fx, d * ((double)y - cy) / fy, d) of a float64 image d [H,W] -> three arrays"""
    fx, fy, cx, cy = (np.float64(k) for k in np.asarray(K, np.float64).reshape(4))
    H, W = d.shape
    y, x = (t.astype(np.float64) for t in np.mgrid[0:H, 0:W])
    with np.errstate(all="ignore"):
        return [d * (x - cx) / fx, d * (y - cy) / fy, d]


def view_normals(depth, K, max_jump):
    """ONE view: depth [H,W] float32, K [4] -> (normal float32 [H,W,3], state uint8 [H,W])"""
    depth = np.asarray(depth, np.float32)
    d = depth.astype(np.float64)
    mj = np.float64(max_jump)
    with np.errstate(all="ignore"):
        isd = np.isfinite(d) & (d > 0.0)
        P = points(d, K)
        diffs, have = [], []
        for dx, dy in ((1, 0), (0, 1)):
            use = []
            for sg in (1, -1):
                dn = _shift(d, sg * dx, sg * dy, np.nan)
                use.append(_shift(isd, sg * dx, sg * dy, False) & (np.abs(dn - d) <= mj))
            up, um = use
            diffs.append([np.where(up, _shift(P[r], dx, dy, 0.0), P[r]) - np.where(um, _shift(P[r], -dx, -dy, 0.0), P[r]) for r in range(3)])
            have.append(up | um)
        a, b = diffs
        m = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
        mm = (m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]
        deg = ~(np.isfinite(mm) & (mm > 0.0))
        ln = np.sqrt(mm)
        u = [m[r] / ln for r in range(3)]
        t = (u[0] * P[0] + u[1] * P[1]) + u[2] * P[2]
        deg |= ~((t < 0.0) | (t > 0.0))
        u = [np.where(t > 0.0, -u[r], u[r]) for r in range(3)]
    state = np.where(deg, DEGENERATE, VALID)
    state = np.where(have[0] & have[1], state, NO_NEIGHBOUR)
    state = np.where(isd, state, NO_DEPTH).astype(np.uint8)
    with np.errstate(all="ignore"):
        n = np.stack([np.where(state == VALID, u[r], 0.0) for r in range(3)], -1).astype(np.float32)
    return n, state


def normals(depth, K, max_jump):
    """depth [V,H,W] float32, K [V,4] or [4], max_jump one value or [V] -> (normals float32 [V,H,W,3], state uint8 [V,H,W], counts int64 [V,4])"""
    depth = np.asarray(depth, np.float32)
    V, H, W = depth.shape
    K = np.broadcast_to(np.asarray(K, np.float64), (V, 4))
    mj = np.broadcast_to(np.asarray(max_jump, np.float64), (V,))
    n, st = np.zeros((V, H, W, 3), np.float32), np.zeros((V, H, W), np.uint8)
    counts = np.zeros((V, STATES), np.int64)
    for v in range(V):
        if not (np.isfinite(mj[v]) and mj[v] > 0):
            raise ValueError(f"view {v}: max_jump must be finite and > 0, got {mj[v]}")
        n[v], st[v] = view_normals(depth[v], K[v], mj[v])
        counts[v] = np.bincount(st[v].reshape(-1), minlength=STATES)
    return n, st, counts


def check_weights(weights):
    w = [int(k) for k in weights]
    if len(w) != 4 or any(k < 1 or k > MAX_WEIGHT for k in w) or any(int(k) != k for k in weights):
        raise ValueError(f"weights are four integers (w_plane, w_proj, w_free, w_empty) in 1 .. {MAX_WEIGHT}, got {tuple(weights)}")
    return w


def view_classes(x, depth, normal, K, E, trunc, weights, empty_is_free=False, znear=0.05):
    """all steps before the update for the positions x (three float64 arrays of one shape) against ONE view: depth [H,W] float32, normal
    [H,W,3] float32 or None, K [4], E [3,4] -> (class uint8, q int64, w int64); q and w are 0 where the voxel-view is skipped"""
    w_plane, w_proj, w_free, w_empty = check_weights(weights)
    depth = np.asarray(depth, np.float32)
    cls0, q = fo.view_classes(x, depth, K, E, trunc, empty_is_free, znear)          # steps 1 - 5, the projective q
    E = np.asarray(E, np.float64).reshape(3, 4)
    fx, fy, cx, cy = (np.float64(k) for k in np.asarray(K, np.float64).reshape(4))
    trunc = np.float64(trunc)
    inside = cls0 != fo.OUT
    with np.errstate(all="ignore"):
        c = [((E[r, 0] * x[0] + E[r, 1] * x[1]) + E[r, 2] * x[2]) + E[r, 3] for r in range(3)]
        u, v = fx * (c[0] / c[2]) + cx, fy * (c[1] / c[2]) + cy
        qx = np.where(inside, np.floor(u + 0.5), 0.0).astype(np.int64)
        qy = np.where(inside, np.floor(v + 0.5), 0.0).astype(np.int64)
        d = depth[qy, qx].astype(np.float64)
        near = cls0 == fo.NEAR
        plane = np.zeros(cls0.shape, bool)
        if normal is not None:
            n = np.asarray(normal, np.float32)[qy, qx].astype(np.float64)
            plane = near & np.isfinite(n).all(-1) & (n != 0.0).any(-1)
            p = [d * (qx.astype(np.float64) - cx) / fx, d * (qy.astype(np.float64) - cy) / fy, d]
            s = ((n[..., 0] * (c[0] - p[0]) + n[..., 1] * (c[1] - p[1])) + n[..., 2] * (c[2] - p[2]))
            value = np.where(s > -trunc, np.where(s < trunc, s, trunc), -trunc)
            qn = np.floor(np.where(plane, value, 0.0) / trunc * np.float64(SCALE) + 0.5).astype(np.int64)
            q = np.where(plane, qn, q)
    cls = np.select([cls0 == fo.OUT, cls0 == fo.EMPTY, cls0 == fo.OCCLUDED, cls0 == fo.FREE, plane], [OUT, EMPTY, OCCLUDED, FREE, NEAR_PLANE], NEAR_PROJ)
    w = np.select([cls == FREE, cls == NEAR_PLANE, cls == NEAR_PROJ], [np.where(d > 0.0, w_free, w_empty), w_plane, w_proj], 0)
    return cls.astype(np.uint8), q, w.astype(np.int64)


def fuse_weighted(state, depth, K, E, origin, voxel, trunc, weights, normals=None, empty="unknown", znear=0.05):
    """the views depth [V,H,W] float32, normals [V,H,W,3] float32 or None, K [V,4], E [V,3,4] fused into state = (sum, n) IN PLACE, in
    order -> view_counts int64 [V,7]"""
    if empty not in ("unknown", "free"):
        raise ValueError(f"empty must be 'unknown' or 'free', got {empty!r}")
    check_weights(weights)
    S, N = state
    depth = np.asarray(depth, np.float32)
    V = depth.shape[0]
    K, E = np.broadcast_to(np.asarray(K, np.float64), (V, 4)), np.asarray(E, np.float64).reshape(V, 3, 4)
    x = fo.positions(S.shape, origin, voxel)
    counts = np.zeros((V, CLASSES), np.int64)
    for v in range(V):
        cls, q, w = view_classes(x, depth[v], None if normals is None else normals[v], K[v], E[v], trunc, weights, empty == "free", znear)
        take = (cls == NEAR_PLANE) | (cls == NEAR_PROJ) | (cls == FREE)
        full = take & (N.astype(np.int64) + w > MAX_OBS)
        cls = np.where(full, SATURATED, cls)
        take &= ~full
        S += np.where(take, w * q, 0).astype(np.int32)
        N += np.where(take, w, 0).astype(np.int32)
        counts[v] = np.bincount(cls.reshape(-1), minlength=CLASSES)
    return counts
