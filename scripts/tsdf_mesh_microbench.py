"""Scene-memory mesh of the fused states (csrc/tsdfmesh.hip) against what the library could do for the same result before it existed.

    python scripts/tsdf_mesh_microbench.py [--instances 64] [--views 8] [--res 64] [--mesh-res 48] [--min-obs 1] [--reps 20]

The workload is the one of scripts/depth_fuse_microbench.py: P instances (synth.canonical_mesh shapes), `views` rendered depth views each,
fused into P grids of res^3 samples (trunc = 4 voxels, empty pixels unknown); the fused states are the input of both forms.  Timed with
device events after warm-up, median of `reps`, the forms alternating in one process:
  mesh      ONE ops.tsdf_mesh_batch(packed=True): the sizing call, the one host read of the offsets, the real call
  kernels   the real ls_tsdf_mesh_batch_f64 call alone, into outputs already sized (no host read): what the bytes are set against
  baseline  ops.tsdf_volume (the float64 volume and its valid flags), mesh_extractor2.marching_cubes_batch machinery on that volume (its
            own sizing call and host read), then the mask and the compaction as torch device ops: kept cubes from eight shifted slices of
            `valid`, the patterns from eight shifted slices of the volume, repeat_interleave of the kept flag over the triangles per
            cube, a mark / cumsum renumbering of the vertices the kept faces name (one more host read, of the vertex counts per mesh),
            and the move into the grids' frames
Both forms are compared on host copies -- offsets, faces, and vertices bit for bit -- BEFORE anything is timed.  Bytes: `min` = what any
method must move (read both int32 volumes once, write every vertex and face once), over the `kernels` time, against the 8.0 TB/s HBM peak.
Nothing here was profiled with counters: the figures are wall times of whole calls."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from depth_fuse_microbench import HBM_PEAK, median_ms  # noqa: E402
from livingscenes_amd import _lib, mesh_extractor2 as me, ops, synth  # noqa: E402
from livingscenes_amd.lib_more.more_solver import More_Solver  # noqa: E402

CORNER = ((0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1))


def triangles_per_pattern():
    """int64 [256] from the table the library compiles (csrc/mc_tables.h)"""
    path = os.path.join(os.path.dirname(os.path.abspath(me.__file__)), "csrc", "mc_tables.h")
    text = open(path).read().split("MC_TRI_TABLE[256][16] = {")[1].split("};")[0]
    rows = np.array([int(t) for t in text.replace("{", " ").replace("}", " ").replace(",", " ").split()]).reshape(256, 16)
    return (rows >= 0).sum(1) // 3


def baseline(state, origin, voxel, min_obs, ntri_of):
    """-> (vertices, faces, vertex offsets, face offsets) as ops.tsdf_mesh_batch(packed=True) returns them"""
    vol, valid, _ = ops.tsdf_volume(state, min_obs)
    verts, faces, vo, fo = me._marching_cubes_packed(vol, 0.0)
    P, nx, ny, nz = vol.shape
    cx, cy, cz = nx - 1, ny - 1, nz - 1
    ok = valid.bool()
    kept = torch.ones(P, cx, cy, cz, dtype=torch.bool, device=vol.device)
    cfg = torch.zeros(P, cx, cy, cz, dtype=torch.int64, device=vol.device)
    for m, (a, b, c) in enumerate(CORNER):
        kept &= ok[:, a:a + cx, b:b + cy, c:c + cz]
        cfg |= (vol[:, a:a + cx, b:b + cy, c:c + cz] <= 0.0).long() << m
    keep_face = torch.repeat_interleave(kept.reshape(-1), ntri_of[cfg.reshape(-1)])              # the packed face order: problem, cube, table
    vo_d, fo_d = (torch.tensor(x, device=vol.device) for x in (vo, fo))
    mesh_of_face = torch.repeat_interleave(torch.arange(P, device=vol.device), fo_d[1:] - fo_d[:-1])
    glob = (faces + vo_d[mesh_of_face][:, None])[keep_face]
    mesh_of_face = mesh_of_face[keep_face]
    mark = torch.zeros(verts.shape[0], dtype=torch.bool, device=vol.device)
    mark[glob.reshape(-1)] = True
    new = torch.cumsum(mark, 0) - 1
    before = torch.cat([new.new_zeros(1), torch.cumsum(mark, 0)])[vo_d]                            # carried vertices before every mesh
    nfaces = torch.bincount(mesh_of_face, minlength=P)
    new_vo, nf = before.cpu().tolist(), nfaces.cpu().tolist()                                     # the baseline's second host read
    mesh_of_vertex = torch.repeat_interleave(torch.arange(P, device=vol.device), vo_d[1:] - vo_d[:-1])[mark]
    o, h = origin.to(vol.device), voxel.to(vol.device)
    v_out = (verts[mark] - 0.5) * h[mesh_of_vertex][:, None] + o[mesh_of_vertex]
    f_out = new[glob] - before[mesh_of_face][:, None]
    return v_out, f_out, new_vo, np.concatenate([[0], np.cumsum(nf)]).tolist()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=64)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--res", type=int, default=64)
    ap.add_argument("--mesh-res", type=int, default=48)
    ap.add_argument("--min-obs", type=int, default=1)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    P, V, res = a.instances, a.views, a.res
    parts = synth.make_partial_views(range(P), V, res=a.mesh_res, with_depth=True, device=dev)
    grids = More_Solver._fusion_grids([torch.cat(p["clouds"]) for p in parts], res, 4)
    state = ops.tsdf_state(P, (res,) * 3, dev)
    ops.depth_fuse_batch(state, [p["depth"] for p in parts], [p["intrinsics"] for p in parts], [p["world_to_cam"] for p in parts],
                         origin=grids["origin"], voxel=grids["voxel"], trunc=grids["trunc"])
    origin, voxel = grids["origin"], grids["voxel"]
    ntri_of = torch.from_numpy(triangles_per_pattern()).to(dev)

    def mesh():
        return ops.tsdf_mesh_batch(state, origin=origin, voxel=voxel, min_obs=a.min_obs, packed=True)

    def base():
        return baseline(state, origin, voxel, a.min_obs, ntri_of)
    # identical meshes, on host copies, before anything is timed
    gv, gf, gvo, gfo, counts = mesh()
    bv, bf, bvo, bfo = base()
    gv, gf, bv, bf = (x.cpu().numpy() for x in (gv, gf, bv, bf))
    assert gvo == bvo and gfo == bfo, "the two forms disagree on the offsets"
    assert gf.shape == bf.shape and (gf >= 0).all() and np.array_equal(gf, bf), "the two forms disagree on the faces"
    assert np.array_equal(gv.view(np.int64), bv.view(np.int64)), "the two forms disagree on the vertices"
    nv, nf = gvo[P], gfo[P]

    lib = _lib.load()
    st = _lib.stream_ptr(dev)
    o, h = ops._fuse_grid("tsdf_mesh_microbench", P, origin, voxel)
    ws = torch.empty(lib.ls_tsdf_mesh_batch_workspace_bytes(P, res, res, res), dtype=torch.uint8, device=dev)
    Vb, Fb = torch.empty(nv, 3, dtype=torch.float64, device=dev), torch.empty(nf, 3, dtype=torch.int64, device=dev)
    off = torch.empty(2, P + 1, dtype=torch.int64, device=dev)

    def kernels():
        _lib.call(dev, "ls_tsdf_mesh_batch_f64", P, _lib.ptr(state[0]), _lib.ptr(state[1]), res, res, res, a.min_obs, ops._hptr(o), ops._hptr(h),
                  _lib.ptr(Vb), nv, _lib.ptr(Fb), nf, _lib.ptr(off), None, _lib.ptr(ws), ws.numel(), st)
    (t_mesh, t_base, t_kern), spread = median_ms([mesh, base, kernels], a.reps)
    c = counts.cpu().numpy().sum(0)
    samples = P * res ** 3
    min_bytes = samples * 8 + nv * 24 + nf * 24
    print(f"instances {P} x {res}^3 samples fused from {V} views each, min_obs {a.min_obs}: {nv} vertices, {nf} faces; kept cubes {int(c[0])}, dropped "
          f"cubes that hold a crossing {int(c[1])}, valid samples {int(c[2])} of {samples}")
    for name, t, (lo, hi) in (("mesh", t_mesh, spread[0]), ("baseline", t_base, spread[1]), ("kernels", t_kern, spread[2])):
        print(f"{name:9s}{t:9.3f} ms (min {lo:.3f}, max {hi:.3f})")
    print(f"baseline / mesh {t_base / t_mesh:.2f}x")
    print(f"bytes  min {min_bytes / 1e6:.0f} MB over the kernels' time -> {min_bytes / t_kern / 1e9:.3f} TB/s "
          f"({100 * min_bytes / (t_kern * 1e-3) / HBM_PEAK:.1f} % of the 8.0 TB/s HBM peak)")


if __name__ == "__main__":
    main()
