"""The NumPy twin of the scene memory's depth fusion: the definition of include/livingscenes_hip.h (ls_depth_fuse_f32, ls_tsdf_volume_f64)
vectorised over the voxels of a grid, one view at a time.  float64 comparisons and integer sums throughout, every product and sum rounded
on its own (NumPy never contracts), so csrc/fuse_plan.h and the kernels of csrc/depthfuse.hip are held to it by equality.  The meshing
half (masked_marching_cubes, mesh: oracle.mcubes plus a mask that only selects among its faces) has NO device counterpart yet; the CPU
tests use it to show what a mesher of the fused volume has to do."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
from oracle import mcubes as om   # noqa: E402

OUT, EMPTY, OCCLUDED, NEAR, FREE, SATURATED = range(6)
CLASSES = 6
SCALE = 16384
MAX_OBS = 65535


def new_state(dims):
    """a fresh state: (sum, n), int32 zeros [nx,ny,nz]"""
    return np.zeros(dims, np.int32), np.zeros(dims, np.int32)


def positions(dims, origin, voxel):
    """x_a = origin_a + h * (double)index_a -> three float64 arrays [nx,ny,nz]"""
    idx = np.meshgrid(*(np.arange(d) for d in dims), indexing="ij")
    h = np.float64(voxel)
    return [np.float64(origin[a]) + h * idx[a].astype(np.float64) for a in range(3)]


def view_classes(x, depth, K, E, trunc, empty_is_free=False, znear=0.05):
    """steps 1 - 6 for the positions x (three float64 arrays of one shape) against ONE view: depth [H,W] float32, K [4], E [3,4]
    -> (class uint8, q int64), before the saturation test; q is 0 where the voxel-view is skipped"""
    depth = np.asarray(depth, np.float32)
    H, W = depth.shape
    E = np.asarray(E, np.float64).reshape(3, 4)
    fx, fy, cx, cy = (np.float64(k) for k in np.asarray(K, np.float64).reshape(4))
    trunc, znear = np.float64(trunc), np.float64(znear)
    with np.errstate(all="ignore"):
        c = [((E[r, 0] * x[0] + E[r, 1] * x[1]) + E[r, 2] * x[2]) + E[r, 3] for r in range(3)]
        ok = np.isfinite(c[0]) & np.isfinite(c[1]) & np.isfinite(c[2]) & ~(c[2] < znear)
        u, v = fx * (c[0] / c[2]) + cx, fy * (c[1] / c[2]) + cy
        rx, ry = np.floor(u + 0.5), np.floor(v + 0.5)
        ok &= (rx >= 0.0) & (rx <= np.float64(W - 1)) & (ry >= 0.0) & (ry <= np.float64(H - 1))      # on the doubles: NaN fails
        qx, qy = np.where(ok, rx, 0.0).astype(np.int64), np.where(ok, ry, 0.0).astype(np.int64)
        d = depth[qy, qx].astype(np.float64)
        empty = ~(d > 0.0)
        s = d - c[2]
        occluded = ~empty & (s < -trunc)
        t = np.where(s < trunc, s, trunc) / trunc
        q = np.floor(np.where(empty | occluded | ~ok, 0.0, t) * np.float64(SCALE) + 0.5).astype(np.int64)
        cls = np.where(s <= trunc, NEAR, FREE)
    cls = np.where(occluded, OCCLUDED, cls)
    if empty_is_free:
        cls, q = np.where(empty, FREE, cls), np.where(empty, SCALE, q)
    else:
        cls, q = np.where(empty, EMPTY, cls), np.where(empty, 0, q)
    cls = np.where(ok, cls, OUT)
    q = np.where((cls == NEAR) | (cls == FREE), q, 0)
    return cls.astype(np.uint8), q


def fuse(state, depth, K, E, origin, voxel, trunc, empty="unknown", znear=0.05):
    """the views depth [V,H,W] float32, K [V,4], E [V,3,4] fused into state = (sum, n) IN PLACE, in order -> view_counts int64 [V,6]"""
    if empty not in ("unknown", "free"):
        raise ValueError(f"empty must be 'unknown' or 'free', got {empty!r}")
    S, N = state
    depth = np.asarray(depth, np.float32)
    V = depth.shape[0]
    K, E = np.asarray(K, np.float64).reshape(V, 4), np.asarray(E, np.float64).reshape(V, 3, 4)
    x = positions(S.shape, origin, voxel)
    counts = np.zeros((V, CLASSES), np.int64)
    for v in range(V):
        cls, q = view_classes(x, depth[v], K[v], E[v], trunc, empty == "free", znear)
        take = (cls == NEAR) | (cls == FREE)
        full = take & (N == MAX_OBS)
        cls = np.where(full, SATURATED, cls)
        take &= ~full
        S += np.where(take, q, 0).astype(np.int32)
        N += take.astype(np.int32)
        counts[v] = np.bincount(cls.reshape(-1), minlength=CLASSES)
    return counts


def volume(state, min_obs=1):
    """-> (D float64, valid bool, counts int64 [3] = valid, valid with D <= 0, n == 0)"""
    S, N = state
    valid = N >= int(min_obs)
    with np.errstate(all="ignore"):
        D = np.where(valid, S.astype(np.float64) / (np.maximum(N, 1).astype(np.float64) * np.float64(SCALE)), 1.0)
    return D, valid, np.array([valid.sum(), (valid & (D <= 0.0)).sum(), (N == 0).sum()], np.int64)


def cube_ok(valid):
    """valid [nx,ny,nz] -> bool [ncubes], cube order = C order: all eight corners valid"""
    valid = np.asarray(valid).astype(bool)
    nx, ny, nz = (s - 1 for s in valid.shape)
    ok = np.ones((nx, ny, nz), bool)
    for a, b, c in om.CORNER:
        ok &= valid[a:a + nx, b:b + ny, c:c + nz]
    return ok.reshape(-1)


def triangles_per_cube(vol, isovalue):
    tri, _ = om._tables()
    vol = np.asarray(vol, np.float64)
    nx, ny, nz = (s - 1 for s in vol.shape)
    iso = float(np.float32(isovalue))
    cfg = np.zeros((nx, ny, nz), np.int64)
    for m, (a, b, c) in enumerate(om.CORNER):
        cfg |= (vol[a:a + nx, b:b + ny, c:c + nz] <= iso).astype(np.int64) << m
    return (tri[cfg.reshape(-1)] >= 0).sum(1) // 3


def masked_marching_cubes(vol, valid, isovalue=0.0):
    """oracle.mcubes.marching_cubes plus the mask: every vertex, the faces of the cubes whose eight corners are valid"""
    vol = np.asarray(vol, np.float64)
    if min(vol.shape) < 2:
        return np.zeros((0, 3)), np.zeros((0, 3), np.int64)
    verts, faces = om.marching_cubes(vol, isovalue)
    if valid is None:
        return verts, faces
    keep = np.repeat(cube_ok(valid), triangles_per_cube(vol, isovalue))
    assert len(keep) == len(faces)
    return verts, faces[keep]


def compact(verts, faces):
    """drop the vertices no face names; the order of the rest is kept"""
    used = np.zeros(len(verts), bool)
    used[faces.reshape(-1)] = True
    new = np.cumsum(used) - 1
    return verts[used], new[faces]


def mesh(state, origin, voxel, min_obs=1, do_compact=True):
    """state -> volume -> masked marching cubes at 0 -> vertices in the grid's frame, (V - 0.5) * voxel + origin as three elementwise ops"""
    D, valid, _ = volume(state, min_obs)
    verts, faces = masked_marching_cubes(D, valid, 0.0)
    if do_compact:
        verts, faces = compact(verts, faces)
    verts = (verts - 0.5) * np.float64(voxel) + np.asarray(origin, np.float64).reshape(1, 3)
    return verts, faces


def fusion_grid(cloud, res, trunc_voxels=4):
    """More_Solver._fusion_grids for one cloud [n,3] -> (origin [3], voxel, trunc), float64"""
    if res < 2 * trunc_voxels + 2:
        raise ValueError("res too small")
    c = np.asarray(cloud, np.float64)
    lo, hi = c.min(0), c.max(0)
    h = (hi - lo).max() / np.float64(res - 1 - 2 * trunc_voxels)
    origin = (lo + hi) / 2 - h * np.float64(res - 1) / 2
    return origin, float(h), float(np.float64(trunc_voxels) * h)
