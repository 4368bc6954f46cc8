"""The NumPy twin of the scene memory's carve: the definition of include/livingscenes_hip.h (ls_cloud_carve_f32) vectorised over the rows
of a cloud, one view and one window pixel at a time.  float64 comparisons and integer counts throughout, every product and sum rounded on
its own (NumPy never contracts), so csrc/carve_plan.h and the kernels of csrc/cloudcarve.hip are held to it by equality."""
import numpy as np

OUT, SEEN, FREE, OCCLUDED, MIXED = range(5)
STATES = 5


def view_states(A, depth, K, E, tol, window=1, empty_is_free=False, znear=0.05):
    """steps 1 - 5 for every row of A [a,3] float32 against ONE view: depth [H,W] float32, K [4] = (fx, fy, cx, cy), E [3,4] -> uint8 [a]"""
    A = np.asarray(A, np.float32).reshape(-1, 3)
    depth = np.asarray(depth, np.float32)
    H, W = depth.shape
    E = np.asarray(E, np.float64).reshape(3, 4)
    fx, fy, cx, cy = (np.float64(k) for k in np.asarray(K, np.float64).reshape(4))
    tol, znear, k = np.float64(tol), np.float64(znear), int(window)
    x = A.astype(np.float64)
    with np.errstate(all="ignore"):
        c = [((E[r, 0] * x[:, 0] + E[r, 1] * x[:, 1]) + E[r, 2] * x[:, 2]) + E[r, 3] for r in range(3)]
        ok = np.isfinite(c[0]) & np.isfinite(c[1]) & np.isfinite(c[2]) & ~(c[2] < znear)
        u, v = fx * (c[0] / c[2]) + cx, fy * (c[1] / c[2]) + cy
        rx, ry = np.floor(u + 0.5), np.floor(v + 0.5)
        ok &= (rx >= 0.0) & (rx <= np.float64(W - 1)) & (ry >= 0.0) & (ry <= np.float64(H - 1))      # on the doubles: NaN fails
    qx, qy = np.where(ok, rx, 0.0).astype(np.int64), np.where(ok, ry, 0.0).astype(np.int64)
    z = c[2]
    n_in, n_hit, n_front, n_behind, n_empty = (np.zeros(len(A), np.int64) for _ in range(5))
    for dy in range(-k, k + 1):
        for dx in range(-k, k + 1):
            y, xx = qy + dy, qx + dx
            inside = ok & (y >= 0) & (y < H) & (xx >= 0) & (xx < W)
            d = depth[np.clip(y, 0, H - 1), np.clip(xx, 0, W - 1)].astype(np.float64)
            with np.errstate(all="ignore"):
                empty = ~(d > 0.0)
                lo, hi = d - tol, d + tol
                front = ~empty & (z < lo)
                behind = ~empty & ~front & (z > hi)
            hit = ~empty & ~front & ~behind
            n_in += inside
            n_hit += inside & hit
            n_front += inside & front
            n_behind += inside & behind
            n_empty += inside & empty
    free = n_front + (n_empty if empty_is_free else 0) == n_in
    st = np.where(n_hit > 0, SEEN, np.where(free, FREE, np.where((n_behind > 0) & (n_front == 0), OCCLUDED, MIXED)))
    return np.where(ok, st, OUT).astype(np.uint8)


def carve(A, depth, K, E, tol, window=1, min_free=1, max_seen=0, empty="unknown", znear=0.05):
    """A [a,3] float32, depth [V,H,W] float32, K [V,4], E [V,3,4] -> dict: state uint8 [V,a], seen / free int32 [a], dropped bool [a],
    points float32 [n,3] (the kept rows, the same bits), src int32 [n], counts int64 [4], view_counts int64 [V,5]"""
    if empty not in ("unknown", "free"):
        raise ValueError(f"empty must be 'unknown' or 'free', got {empty!r}")
    A = np.ascontiguousarray(A, np.float32).reshape(-1, 3)
    depth = np.asarray(depth, np.float32)
    V = depth.shape[0]
    K, E = np.asarray(K, np.float64).reshape(V, 4), np.asarray(E, np.float64).reshape(V, 3, 4)
    state = np.zeros((V, len(A)), np.uint8)
    for v in range(V):
        state[v] = view_states(A, depth[v], K[v], E[v], tol, window, empty == "free", znear)
    seen, free = (state == SEEN).sum(0).astype(np.int32), (state == FREE).sum(0).astype(np.int32)
    dropped = (free >= int(min_free)) & (seen <= int(max_seen))
    src = np.flatnonzero(~dropped).astype(np.int32)
    counts = np.array([(seen >= 1).sum(), (free >= 1).sum(), dropped.sum(), (state == OUT).all(0).sum()], np.int64)
    view_counts = np.stack([(state == s).sum(1) for s in range(STATES)], 1).astype(np.int64).reshape(V, STATES)
    return {"state": state, "seen": seen, "free": free, "dropped": dropped, "points": A[src], "src": src, "counts": counts,
            "view_counts": view_counts}
