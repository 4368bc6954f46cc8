"""Scene-memory raycast of the fused states (csrc/tsdfray.hip) against the way such images were made before it.

    python scripts/tsdf_raycast_microbench.py [--instances 64] [--views 8] [--res 64] [--mesh-res 48] [--min-obs 1] [--step 0.5] [--reps 20]

The states of scripts/tsdf_mesh_microbench.py and scripts/tsdf_icp_microbench.py: P synth shapes, `views` rendered depth views of
100 x 100 each (synth.make_partial_views), fused into P grids of res^3 samples (trunc = 4 voxels, empty pixels unknown).  Every state is
then seen from its own `views` cameras.  Timed with device events after warm-up, median of `reps`, the forms alternating in the same run:
  raycast  one ls_tsdf_raycast_batch_f64 call on inputs already packed and outputs already sized (the library call alone)
  mesh     what a user did before: ops.tsdf_mesh_batch (a sizing call, one host read, the real call) followed by
           ops.mesh_render_depth_batch at the same cameras, as the wrappers make them (their host reads included: that IS the path)
  compare  one ls_depth_compare_f32 call of the views' own depth maps against the raycast
Bytes that must move for the raycast: its outputs (17 bytes per pixel: depth, normal, state) plus the state cells the rays touch, for
which the whole state (sum, n: 8 bytes per sample) is an UPPER bound -- a cell is counted once however many rays cross it.  Nothing here
was profiled with counters: the figures are wall times of whole calls, and nothing is said about what bounds them."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from livingscenes_amd import _lib, ops, synth  # noqa: E402
from livingscenes_amd.lib_more.more_solver import More_Solver  # noqa: E402
from cloud_nearest_microbench import median_ms  # noqa: E402

PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=64)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--res", type=int, default=64)
    ap.add_argument("--mesh-res", type=int, default=48)
    ap.add_argument("--min-obs", type=int, default=1)
    ap.add_argument("--step", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    P, V, res = a.instances, a.views, a.res
    parts = synth.make_partial_views(range(P), V, res=a.mesh_res, with_depth=True, device=dev)
    clouds = [torch.cat(p["clouds"]) for p in parts]
    grids = More_Solver._fusion_grids(clouds, res, 4)
    S, N = ops.tsdf_state(P, (res,) * 3, dev)
    ops.depth_fuse_batch((S, N), [p["depth"] for p in parts], [p["intrinsics"] for p in parts], [p["world_to_cam"] for p in parts],
                         origin=grids["origin"], voxel=grids["voxel"], trunc=grids["trunc"])
    o, h, tr = (np.ascontiguousarray(grids[k].numpy(), np.float64) for k in ("origin", "voxel", "trunc"))
    Es = [p["world_to_cam"].to(torch.float64) for p in parts]
    E = torch.cat(Es).cpu()
    Rt = E[:, :, :3].transpose(1, 2)
    M = torch.cat([Rt, -(Rt @ E[:, :, 3:4])], -1).contiguous().to(dev)          # camera to memory frame, formed in float64 on the host
    K = torch.cat([p["intrinsics"].to(torch.float64).reshape(-1, 4).expand(V, 4) for p in parts]).contiguous()
    observed = torch.cat([p["depth"] for p in parts]).contiguous()
    views, H, W = observed.shape
    vo = ops._offsets([V] * P)
    depth, normal = torch.empty(views, H, W, device=dev), torch.empty(views, H, W, 3, device=dev)
    state, counts = torch.empty(views, H, W, dtype=torch.uint8, device=dev), torch.empty(views, 5, dtype=torch.int64, device=dev)
    cls, ccounts = torch.empty(views, H, W, dtype=torch.uint8, device=dev), torch.empty(views, 5, dtype=torch.int64, device=dev)
    lib = _lib.load()
    ws = torch.empty(lib.ls_tsdf_raycast_batch_workspace_bytes(P, res, res, res, views, H, W), dtype=torch.uint8, device=dev)
    st = _lib.stream_ptr(dev)

    def raycast():
        _lib.call(dev, "ls_tsdf_raycast_batch_f64", P, _lib.ptr(S), _lib.ptr(N), res, res, res, a.min_obs, ops._hptr(o), ops._hptr(h), ops._hptr(tr),
                  _lib.ptr(M), _lib.ptr(K), views, ops._hptr(vo), H, W, 0.05, a.step, _lib.ptr(depth), _lib.ptr(normal), _lib.ptr(state), _lib.ptr(counts),
                  _lib.ptr(ws), ws.numel(), st)

    tol = float(tr.mean()) / 4                                                # one voxel: a placeholder, not a recommendation

    def compare():
        _lib.call(dev, "ls_depth_compare_f32", _lib.ptr(observed), _lib.ptr(depth), _lib.ptr(state), views, H, W, tol, _lib.ptr(cls), _lib.ptr(ccounts), st)

    shared = parts[0]["intrinsics"]
    rendered = {}

    def mesh_form():
        meshes = ops.tsdf_mesh_batch((S, N), origin=grids["origin"], voxel=grids["voxel"], min_obs=a.min_obs)[0]
        rendered["out"] = ops.mesh_render_depth_batch([(v, f.to(torch.int32)) for v, f in meshes], Es, shared, H, W)
        rendered["faces"] = sum(int(f.shape[0]) for _, f in meshes)

    raycast()
    compare()
    mesh_form()
    torch.cuda.synchronize()
    hist, chist = counts.sum(0).tolist(), ccounts.sum(0).tolist()
    mesh_depth = torch.cat([d for d, _, _ in rendered["out"]])
    both = (mesh_depth > 0) & (state == 4)
    gap = float((mesh_depth[both] - depth[both]).abs().double().mean() / float(h.mean())) if bool(both.any()) else float("nan")
    (t_r, t_c, t_m), spread = median_ms([raycast, compare, mesh_form], a.reps)
    print(f"instances {P} x {res}^3 samples fused from {V} views each, {views} views of {H} x {W} raycast at step {a.step}, min_obs {a.min_obs}")
    print("ray states   " + ", ".join(f"{n} {c}" for n, c in zip(ops.RAY_STATE, hist)))
    print(f"view classes " + ", ".join(f"{n} {c}" for n, c in zip(ops.VIEW_CLASS, chist)) + f" (tol {tol:.4f}, one voxel: a placeholder)")
    print(f"the meshes of the same states: {rendered['faces']} faces; pixels both forms hit: {int(both.sum())}, mean |mesh depth - raycast depth| there "
          f"{gap:.3f} voxels")
    for name, t, (lo, hi) in zip(("raycast", "compare", "mesh"), (t_r, t_c, t_m), spread):
        print(f"{name:8s} {t:9.3f} ms (min {lo:.3f}, max {hi:.3f})")
    out_bytes, state_bytes = views * H * W * 17 + views * 40, 8 * P * res ** 3
    print(f"raycast: outputs {out_bytes / 2 ** 20:.0f} MiB = {100 * out_bytes / (t_r * 1e-3) / PEAK:.2f} % of 8.0 TB/s; with the whole state (an upper bound "
          f"on the cells the rays touch) {(out_bytes + state_bytes) / 2 ** 20:.0f} MiB = {100 * (out_bytes + state_bytes) / (t_r * 1e-3) / PEAK:.2f} %; "
          f"workspace {ws.numel()} bytes; mesh / raycast = {t_m / t_r:.1f}")
    cmp_bytes = views * H * W * 10
    print(f"compare: {cmp_bytes / 2 ** 20:.0f} MiB (9 in + 1 out per pixel) = {100 * cmp_bytes / (t_c * 1e-3) / PEAK:.2f} % of 8.0 TB/s")


if __name__ == "__main__":
    main()
