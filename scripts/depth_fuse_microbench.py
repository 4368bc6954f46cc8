"""Scene-memory depth fusion and its volume (csrc/depthfuse.hip), each timed on its own, and the fuse against the same update written with
torch device ops.

    python scripts/depth_fuse_microbench.py [--instances 64] [--views 8] [--res 64] [--mesh-res 48] [--reps 20]

P instances: synth.canonical_mesh(seed, res=mesh_res) shapes, `views` rendered depth views of 100 x 100 pixels each
(synth.make_partial_views(with_depth=True)), fused into P grids of res^3 samples (More_Solver._fusion_grids of the views' clouds,
trunc = 4 voxels, empty pixels unknown).  Timed with device events after warm-up, median of `reps`, the forms alternating; every timed
fuse starts from a zeroed state (the memset is outside the events):
  fuse    ONE ls_depth_fuse_batch_f32 call on pre-packed inputs (the library call alone: no torch.cat, no host read)
  torch   all instances at once, one view after the other: positions, the float64 projection, floor, one indexed gather per (voxel,
          view), the quantised distance and the integer update as tensor expressions -- no histogram, which the op does make
  volume  ONE ls_tsdf_volume_f64 call
The states of fuse and torch are compared (torch contracts and orders its float64 products as it likes, so a voxel at a boundary may
differ).  Bytes: `min` = what any method must move for the fuse (read and write both int32 volumes once, read every image once), over
the fuse's time, against the 8.0 TB/s HBM peak."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from livingscenes_amd import _lib, ops, synth  # noqa: E402
from livingscenes_amd.lib_more.more_solver import More_Solver  # noqa: E402

HBM_PEAK = 8.0e12


def median_ms(fns, reps, before=None):
    """every fn warmed up, then timed `reps` times in turn -> the medians; `before` runs ahead of every timed call, outside the events"""
    for fn in fns:
        fn(), fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            if before is not None:
                before()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    return [float(np.median(t)) for t in times], [(float(np.min(t)), float(np.max(t))) for t in times]


def torch_form(S, N, origin, voxel, trunc, D, K, E, znear):
    """S, N [P,n] int32 updated in place; origin [P,3], voxel, trunc [P] float64 on the device; D [P,V,H,W], K [P,V,4], E [P,V,3,4]"""
    P, V, H, W = D.shape
    res = round(S.shape[1] ** (1 / 3))
    idx = torch.arange(S.shape[1], device=S.device)
    ijk = torch.stack([idx // (res * res), (idx // res) % res, idx % res], -1).double()           # [n,3]
    x = origin[:, None, :] + voxel[:, None, None] * ijk[None]                                    # [P,n,3]
    flat = D.reshape(P, V, H * W)
    tr = trunc[:, None]
    for v in range(V):
        c = torch.einsum("prc,pnc->pnr", E[:, v, :, :3], x) + E[:, v, None, :, 3]
        z = c[..., 2]
        ok = torch.isfinite(c).all(-1) & ~(z < znear)
        rx = torch.floor(K[:, v, None, 0] * (c[..., 0] / z) + K[:, v, None, 2] + 0.5)
        ry = torch.floor(K[:, v, None, 1] * (c[..., 1] / z) + K[:, v, None, 3] + 0.5)
        ok &= (rx >= 0) & (rx <= W - 1) & (ry >= 0) & (ry <= H - 1)
        pix = torch.where(ok, ry * W + rx, 0.0).long()
        d = torch.gather(flat[:, v], 1, pix).double()
        s = d - z
        take = ok & (d > 0) & ~(s < -tr) & (N < 65535)
        q = torch.floor(torch.minimum(s, tr) / tr * 16384.0 + 0.5)
        S += torch.where(take, q, 0.0).int()
        N += take.int()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=64)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--res", type=int, default=64)
    ap.add_argument("--mesh-res", type=int, default=48)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    P, V, res, znear = a.instances, a.views, a.res, 0.05
    parts = synth.make_partial_views(range(P), V, res=a.mesh_res, with_depth=True, device=dev)
    grids = More_Solver._fusion_grids([torch.cat(p["clouds"]) for p in parts], res, 4)
    D = torch.cat([p["depth"] for p in parts]).contiguous()
    H, W = D.shape[1:]
    K = torch.cat([p["intrinsics"].reshape(1, 4).expand(V, 4) for p in parts]).contiguous()
    E = torch.cat([p["world_to_cam"] for p in parts]).contiguous()
    o, h, t = (grids[k].numpy().copy() for k in ("origin", "voxel", "trunc"))
    vo = ops._offsets([V] * P)
    lib = _lib.load()
    st = _lib.stream_ptr(dev)
    S, N = ops.tsdf_state(P, (res,) * 3, dev)
    S2, N2 = (torch.zeros(P, res ** 3, dtype=torch.int32, device=dev) for _ in range(2))
    vc = torch.empty(P * V, 6, dtype=torch.int64, device=dev)
    ws = torch.empty(lib.ls_depth_fuse_batch_workspace_bytes(P, res, res, res, P * V), dtype=torch.uint8, device=dev)

    def zero():
        for x in (S, N, S2, N2):
            x.zero_()

    def fuse():
        _lib.call(dev, "ls_depth_fuse_batch_f32", P, _lib.ptr(S), _lib.ptr(N), res, res, res, ops._hptr(o), ops._hptr(h), ops._hptr(t), _lib.ptr(D),
                  P * V, ops._hptr(vo), H, W, _lib.ptr(K), _lib.ptr(E), znear, 0, _lib.ptr(vc), _lib.ptr(ws), ws.numel(), st)
    od, hd, td = (torch.from_numpy(x).to(dev) for x in (o, h, t))
    D4, K3, E4 = D.reshape(P, V, H, W), K.reshape(P, V, 4), E.reshape(P, V, 3, 4)

    def tf():
        torch_form(S2, N2, od, hd, td, D4, K3, E4, znear)
    (t_fuse, t_torch), spread = median_ms([fuse, tf], a.reps, before=zero)
    zero(), fuse(), tf()                                                   # once more from zeros, for the comparison and for the volume below
    same = (S.reshape(P, -1) == S2) & (N.reshape(P, -1) == N2)
    hist = vc.cpu().numpy().sum(0)

    vol = torch.empty(P, res, res, res, dtype=torch.float64, device=dev)
    valid = torch.empty(P, res, res, res, dtype=torch.uint8, device=dev)
    counts = torch.empty(P, 3, dtype=torch.int64, device=dev)

    def volume():
        _lib.call(dev, "ls_tsdf_volume_f64", _lib.ptr(S), _lib.ptr(N), P, res, res, res, 1, _lib.ptr(vol), _lib.ptr(valid), _lib.ptr(counts), st)
    (t_vol,), spread2 = median_ms([volume], a.reps)
    voxels, pairs = P * res ** 3, P * res ** 3 * V
    min_bytes = voxels * 16 + D.numel() * 4
    c = counts.cpu().numpy().sum(0)
    print(f"instances {P} x {res}^3 samples x {V} views of {H} x {W}, trunc 4 voxels, empty pixels unknown")
    print(f"classes (out, empty, occluded, near, free, saturated) over all (voxel, view) pairs: {hist.tolist()}; valid samples {int(c[0])} of {voxels}, "
          f"inside {int(c[1])}, never observed {int(c[2])}")
    print(f"fuse   {t_fuse:9.3f} ms (min {spread[0][0]:.3f}, max {spread[0][1]:.3f}); {pairs / t_fuse / 1e6:.1f} G (voxel, view) pairs / s")
    print(f"torch  {t_torch:9.3f} ms (min {spread[1][0]:.3f}, max {spread[1][1]:.3f}); ratio {t_torch / t_fuse:.1f}x; voxels whose state differs "
          f"{int((~same).sum())} of {voxels}")
    print(f"volume {t_vol:9.3f} ms (min {spread2[0][0]:.3f}, max {spread2[0][1]:.3f}); {voxels * 17 / t_vol / 1e9:.3f} TB/s of 17 bytes per sample")
    print(f"bytes  min {min_bytes / 1e6:.0f} MB -> {min_bytes / t_fuse / 1e9:.3f} TB/s ({100 * min_bytes / (t_fuse * 1e-3) / HBM_PEAK:.1f} % of the 8.0 TB/s HBM peak)")


if __name__ == "__main__":
    main()
