"""Depth views of meshes on the device (csrc/meshrender.hip: ls_mesh_render_depth_batch_f64) against the same images from torch device
ops, and what accumulating partial views buys on surface scans.

    python scripts/render_depth_microbench.py [--shapes 64] [--views 8] [--res 48] [--reps 20] [--torch-shapes 2] [--samples 30000]

Time.  Device events after warm-up, median of `reps`, the two forms alternating in one process, on pre-packed inputs (the library call
alone: no torch.cat, no host read).  Three cases:
  batch    `shapes` synth.canonical_mesh(res) meshes x `views` views at 100 x 100 (the reference's camera settings): ONE library call.  The
           torch form is timed on the first `torch-shapes` meshes, and the library on those same meshes beside it
  one      one such mesh, one view at 640 x 480
  box      a 12-triangle box, one view at 640 x 480: every face is large, the wave-wide walk decides the time
  torch    per view, chunks of faces against ALL pixels: the same float64 projection, snap and int64 edge functions, the same key, a masked
           amin over the chunk.  Its images are compared with the library's bit for bit before anything is timed.
Also reported: the bytes any method must move -- the key image written and read (16 B per pixel), the two output images (8 B per pixel),
3 indices and 72 B of corners per (view, face) -- and that figure over the measured time as a share of the 8.0 TB/s peak.
Illustration (NOT a recommendation): the 1 .. `views` partial views of each shape merged at their true poses with ops.cloud_merge_batch at
0.01 m; per number of views, the share of `samples` ops.mesh_sample points per shape that have a memory point within 0.02 m
(ops.cloud_nearest_batch)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from livingscenes_amd import _lib, ops, render, synth  # noqa: E402
from livingscenes_amd.evaluate import _device_meshes  # noqa: E402
from cloud_nearest_microbench import median_ms  # noqa: E402

PEAK = 8.0e12
SUB, SNAP_MAX = 256, 1 << 24


class Call:
    """one ls_mesh_render_depth_batch_f64 call on a packed workload, with its output buffers"""

    def __init__(self, meshes, Es, K, H, W, dev):
        self.dev, self.M, self.H, self.W = dev, len(meshes), H, W
        self.V, self.vo, self.F, self.fo = ops._pack_meshes(meshes)
        self.E = torch.cat(Es).contiguous()
        self.views = self.E.shape[0]
        self.K = K.expand(self.views, 4).contiguous()
        self.wo = ops._offsets([e.shape[0] for e in Es])
        self.depth = torch.empty(self.views, H, W, dtype=torch.float32, device=dev)
        self.face = torch.empty(self.views, H, W, dtype=torch.int32, device=dev)
        self.meta = torch.empty(self.views * 4 + 1, dtype=torch.int64, device=dev)
        self.ws = torch.empty(_lib.load().ls_mesh_render_depth_batch_workspace_bytes(self.M, self.views, H, W), dtype=torch.uint8, device=dev)
        self.st = _lib.stream_ptr(dev)
        self.items = int(sum((self.fo[m + 1] - self.fo[m]) * (self.wo[m + 1] - self.wo[m]) for m in range(self.M)))

    def run(self):
        _lib.call(self.dev, "ls_mesh_render_depth_batch_f64", self.M, _lib.ptr(self.V), self.V.shape[0], ops._hptr(self.vo), _lib.ptr(self.F),
                  self.F.shape[0], ops._hptr(self.fo), self.views, ops._hptr(self.wo), _lib.ptr(self.E), _lib.ptr(self.K), self.H, self.W, 0.05,
                  _lib.ptr(self.depth), _lib.ptr(self.face), _lib.ptr(self.meta), _lib.ptr(self.meta[self.views * 4:]), _lib.ptr(self.ws),
                  self.ws.numel(), self.st)

    def floor_bytes(self):
        return self.views * self.H * self.W * (16 + 8) + self.items * (12 + 72)


def torch_render(V, F, E, K, H, W, znear=0.05, chunk_elems=1 << 24):
    """the definition with torch device ops: one view of one mesh -> (depth [H,W] fp32, face [H,W] int32)"""
    dev = V.device
    c = ((E[:, 0] * V[:, 0:1] + E[:, 1] * V[:, 1:2]) + E[:, 2] * V[:, 2:3]) + E[:, 3]               # [nv,3]
    u, v = K[0] * (c[:, 0] / c[:, 2]) + K[2], K[1] * (c[:, 1] / c[:, 2]) + K[3]
    tu, tv = torch.floor(u * SUB + 0.5), torch.floor(v * SUB + 0.5)
    ok_v = torch.isfinite(c[:, 2]) & (c[:, 2] >= znear) & (tu.abs() <= SNAP_MAX) & (tv.abs() <= SNAP_MAX)
    xs, ys = torch.where(ok_v, tu, 0.0).long(), torch.where(ok_v, tv, 0.0).long()
    iz = 1.0 / c[:, 2]
    Fl = F.long()
    ok_f = ok_v[Fl].all(1)
    X = (torch.arange(W, device=dev) * SUB).repeat(H)[None]                                           # [1,HW]
    Y = (torch.arange(H, device=dev) * SUB).repeat_interleave(W)[None]
    best = torch.full((H * W,), torch.iinfo(torch.int64).max, dtype=torch.int64, device=dev)
    chunk = max(chunk_elems // (H * W), 1)
    for s in range(0, Fl.shape[0], chunk):
        f = Fl[s:s + chunk]
        x, y, z = xs[f][:, :, None], ys[f][:, :, None], iz[f][:, :, None]                            # [C,3,1]
        e0 = (x[:, 2] - x[:, 1]) * (Y - y[:, 1]) - (y[:, 2] - y[:, 1]) * (X - x[:, 1])
        e1 = (x[:, 0] - x[:, 2]) * (Y - y[:, 2]) - (y[:, 0] - y[:, 2]) * (X - x[:, 2])
        e2 = (x[:, 1] - x[:, 0]) * (Y - y[:, 0]) - (y[:, 1] - y[:, 0]) * (X - x[:, 0])
        A = e0 + e1 + e2
        cov = (A != 0) & (((e0 >= 0) & (e1 >= 0) & (e2 >= 0)) | ((e0 <= 0) & (e1 <= 0) & (e2 <= 0))) & ok_f[s:s + chunk, None]
        d = (A.double() / ((e0.double() * z[:, 0] + e1.double() * z[:, 1]) + e2.double() * z[:, 2])).float()
        key = (d.view(torch.int32).long() << 32) | torch.arange(s, s + f.shape[0], device=dev)[:, None]   # d > 0: the sign bit is clear
        best = torch.minimum(best, torch.where(cov, key, torch.iinfo(torch.int64).max).amin(0))
    hit = best != torch.iinfo(torch.int64).max
    depth = torch.where(hit, (best >> 32).int().view(torch.float32), 0.0)
    face = torch.where(hit, (best & 0xFFFFFFFF).int(), -1)
    return depth.reshape(H, W), face.reshape(H, W)


def torch_form(meshes, Es, K, H, W):
    out = [torch_render(V, F, E, K, H, W) for (V, F), Em in zip(meshes, Es) for E in Em]
    return torch.stack([d for d, _ in out]), torch.stack([f for _, f in out])


def case(name, meshes, Es, K, H, W, reps, dev, torch_meshes=None):
    full = Call(meshes, Es, K, H, W, dev)
    n_t = len(meshes) if torch_meshes is None else min(torch_meshes, len(meshes))
    sub = full if n_t == len(meshes) else Call(meshes[:n_t], Es[:n_t], K, H, W, dev)
    sub.run()
    t_depth, t_face = torch_form(meshes[:n_t], Es[:n_t], K, H, W)
    torch.cuda.synchronize()
    assert not int(sub.meta[-1:].view(torch.int32)[0]), "a face names a vertex outside its mesh"   # status: the int32 after the counts
    assert torch.equal(sub.depth.view(torch.int32), t_depth.view(torch.int32)) and torch.equal(sub.face, t_face), "the two forms disagree"
    fns = [full.run, sub.run, lambda: torch_form(meshes[:n_t], Es[:n_t], K, H, W)]
    (t_full, t_sub, t_torch), spread = median_ms(fns, reps)
    counts = full.meta[:-1].reshape(-1, 4).cpu().numpy()
    print(f"{name}: {len(meshes)} mesh(es), {full.views} views of {H} x {W}, {full.F.shape[0]} faces, {full.items} (view, face) items, "
          f"{counts[:, 0].sum()} pixels hit; workspace {full.ws.numel() / 2 ** 20:.1f} MiB")
    print(f"  library            {t_full:9.3f} ms (min {spread[0][0]:.3f}, max {spread[0][1]:.3f}); bytes any method moves {full.floor_bytes() / 1e6:.1f} MB "
          f"= {full.floor_bytes() / (t_full * 1e-3) / PEAK * 100:.2f} % of the 8.0 TB/s peak at this time")
    if sub is not full:
        print(f"  library, {n_t} mesh(es) {t_sub:9.3f} ms (min {spread[1][0]:.3f}, max {spread[1][1]:.3f})")
    print(f"  torch, {n_t} mesh(es)   {t_torch:9.3f} ms (min {spread[2][0]:.3f}, max {spread[2][1]:.3f}); torch / library on the same images = "
          f"{t_torch / t_sub:.1f}; images bit-identical")


def box_mesh(dev):
    V = np.array([[x, y, z] for x in (-0.3, 0.3) for y in (-0.25, 0.25) for z in (-0.2, 0.2)], np.float64)
    F = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]])
    return torch.from_numpy(V).to(dev), torch.from_numpy(F).to(device=dev, dtype=torch.int32)


def coverage(meshes, partial, n_views, samples, dev):
    """per number of merged views, the share of surface samples with a memory point within 0.02 m"""
    P = len(meshes)
    dense = [p.float().contiguous() for p, _ in ops.mesh_sample_batch(meshes, samples, list(range(P)))]
    mem = [o["clouds"][0][:0] for o in partial]
    print(f"illustration: {P} shapes, views merged at their true poses with cloud_merge_batch at 0.01 m; share of {samples} mesh_sample points per "
          f"shape with a memory point within 0.02 m (cloud_nearest_batch)")
    for k in range(n_views):
        mem = [x for x, _ in ops.cloud_merge_batch(mem, [o["clouds"][k].contiguous() for o in partial], voxel=0.01)]
        res = ops.cloud_nearest_batch(mem, dense, radius=0.02)
        share = np.array([r[2][1] / max(r[2][0], 1) for r in res])
        print(f"  {k + 1} view(s): memory rows {sum(m.shape[0] for m in mem) / P:8.0f} per shape, covered {share.mean():.4f} (min {share.min():.4f}, max {share.max():.4f})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=int, default=64)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--res", type=int, default=48)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--torch-shapes", type=int, default=2)
    ap.add_argument("--samples", type=int, default=30000)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    shapes = [synth.canonical_mesh(s, res=a.res, device=dev) for s in range(a.shapes)]
    meshes = _device_meshes(shapes, dev)
    poses = [render.gen_random_poses(a.views, s) for s in range(a.shapes)]
    Es = [up(np.stack([render.world_to_cam(p) for p in ps])) for ps in poses]
    K100 = torch.tensor([100.0, 100.0, 50.0, 50.0], dtype=torch.float64, device=dev)
    K640 = torch.tensor([640.0, 640.0, 320.0, 240.0], dtype=torch.float64, device=dev)
    case("batch", meshes, Es, K100, 100, 100, a.reps, dev, torch_meshes=a.torch_shapes)
    case("one", meshes[:1], [Es[0][:1]], K640, 480, 640, a.reps, dev)
    case("box", [box_mesh(dev)], [Es[0][:1]], K640, 480, 640, a.reps, dev)
    partial = synth.make_partial_views(list(range(a.shapes)), a.views, res=a.res, device=dev)
    coverage(meshes, partial, a.views, a.samples, dev)


if __name__ == "__main__":
    main()
