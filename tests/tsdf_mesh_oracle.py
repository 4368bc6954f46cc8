"""The NumPy twin of the scene memory's mesh of a fused state (include/livingscenes_hip.h: ls_tsdf_mesh_f64; csrc/tsdfmesh_plan.h).  The
answer itself is tests/fuse_oracle.py: mesh -- oracle.mcubes on the volume, the faces of the cubes whose eight corners are valid, the
vertices no face names dropped.  What this file adds is the LOCAL rule the device uses instead of that compaction, computed from the kept
bits alone and independent of fuse_oracle.compact, so that the two can be compared: a created vertex is carried iff its cube is kept or,
for the edges 6, 5 and 10, one of the up to three other cubes around the lattice edge is."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import fuse_oracle as fo   # noqa: E402
from oracle import mcubes as om   # noqa: E402

# the other cubes that name the vertex of a cube's edge 6 / 5 / 10, as offsets (di, dj, dk)
SHARERS = {6: ((0, 1, 1), (0, 0, 1), (0, 1, 0)), 5: ((0, 0, 1), (1, 0, 1), (1, 0, 0)), 10: ((1, 1, 0), (0, 1, 0), (1, 0, 0))}


def random_state(seed, dims, P=None):
    """the seeded states of the tests: n in 0 .. 3 (5 % never observed), sum = n * a value in [-16384, 16384] -> (sum, n) int32"""
    rng = np.random.default_rng(seed)
    shape = tuple(dims) if P is None else (P,) + tuple(dims)
    N = rng.choice([0, 1, 2, 3], size=shape, p=[.05, .35, .3, .3])
    S = rng.integers(-16384, 16385, size=shape) * N
    return S.astype(np.int32), N.astype(np.int32)


def patterns(D):
    """D [nx,ny,nz] -> the pattern of every cube, int64 [cx,cy,cz]: bit m set iff D <= 0 at corner m"""
    cx, cy, cz = (s - 1 for s in D.shape)
    cfg = np.zeros((cx, cy, cz), np.int64)
    for m, (a, b, c) in enumerate(om.CORNER):
        cfg |= (D[a:a + cx, b:b + cy, c:c + cz] <= 0.0).astype(np.int64) << m
    return cfg


def crossed_edges(cfg):
    """-> bool [...,12]: the two corners of the edge differ"""
    return np.stack([((cfg >> om.EDGE_A[e]) & 1) != ((cfg >> om.EDGE_B[e]) & 1) for e in range(12)], -1)


def created_edges(crossed):
    """crossed [cx,cy,cz,12] -> the edges every cube creates (oracle.mcubes: 6, 5, 10 always, the others on the low faces)"""
    cx, cy, cz = crossed.shape[:3]
    I, J, K = np.meshgrid(np.arange(cx), np.arange(cy), np.arange(cz), indexing="ij")
    i0, j0, k0 = I == 0, J == 0, K == 0
    cond = {0: j0 | k0, 1: k0, 2: k0, 3: i0 | k0, 4: j0, 7: i0, 8: i0 | j0, 9: j0, 11: i0}
    creates = np.zeros_like(crossed)
    for e in (6, 5, 10):
        creates[..., e] = crossed[..., e]
    for e, c in cond.items():
        creates[..., e] = crossed[..., e] & c
    return creates


def carried_edges(creates, kept):
    """the local rule: creates [cx,cy,cz,12], kept bool [cx,cy,cz] -> the created edges whose vertex some kept cube names"""
    cx, cy, cz = kept.shape
    pad = np.zeros((cx + 1, cy + 1, cz + 1), bool)
    pad[:cx, :cy, :cz] = kept
    carried = creates & kept[..., None]
    for e, offs in SHARERS.items():
        near = np.zeros_like(kept)
        for di, dj, dk in offs:
            near |= pad[di:di + cx, dj:dj + cy, dk:dk + cz]
        carried[..., e] |= creates[..., e] & near
    return carried


def analyse(state, min_obs=1):
    """-> dict(D, valid, cfg, kept [cx,cy,cz], creates, carried [cx,cy,cz,12], stats int64 [3] = kept cubes, dropped cubes that hold a
    crossing, valid samples)"""
    D, valid, _ = fo.volume(state, min_obs)
    cfg = patterns(D)
    kept = fo.cube_ok(valid).reshape(cfg.shape)
    creates = created_edges(crossed_edges(cfg))
    carried = carried_edges(creates, kept)
    stats = np.array([kept.sum(), (~kept & (cfg != 0) & (cfg != 255)).sum(), valid.sum()], np.int64)
    return dict(D=D, valid=valid, cfg=cfg, kept=kept, creates=creates, carried=carried, stats=stats)


def carried_in_creation_order(a):
    """-> bool [created vertices]: which of oracle.mcubes' vertices, in its numbering, the local rule carries"""
    order = np.array(om.ORDER)
    return a["carried"][..., order].reshape(-1)[a["creates"][..., order].reshape(-1)]


def mesh(state, origin, voxel, min_obs=1):
    """the expected mesh (fuse_oracle.mesh) -> (vertices float64 [nv,3], faces int64 [nf,3]); a state with a dim < 2 has none"""
    if min(state[0].shape) < 2:
        return np.zeros((0, 3)), np.zeros((0, 3), np.int64)
    return fo.mesh(state, origin, voxel, min_obs)


def mesh_by_rule(state, origin, voxel, min_obs=1):
    """the same mesh WITHOUT fuse_oracle.compact: the vertices the local rule carries, the faces renumbered by its running count"""
    a = analyse(state, min_obs)
    verts, faces = fo.masked_marching_cubes(a["D"], a["valid"], 0.0)
    used = carried_in_creation_order(a)
    assert len(used) == len(verts)
    new = np.cumsum(used) - 1
    assert used[faces.reshape(-1)].all(), "a kept face names a vertex the rule does not carry"
    verts = (verts[used] - 0.5) * np.float64(voxel) + np.asarray(origin, np.float64).reshape(1, 3)
    return verts, new[faces]
