"""Scene-memory normals and point-to-plane ICP (csrc/cloudnear.hip: ls_cloud_normals_batch_f32, ls_cloud_icp_plane_batch_f32) against their
yardsticks: one ls_cloud_nearest_batch_f32 call, and the point-to-point ls_cloud_icp_batch_f32.

    python scripts/cloud_plane_icp_microbench.py [--instances 64] [--points 60000] [--voxel 0.01] [--reps 20] [--iters 4] [--shape-points 20000]

Timed with device events after warm-up, median of `reps`, the forms alternating in one process, all on pre-packed inputs (the library calls
alone: no torch.cat, no host read).  Two workloads.
The slab of scripts/cloud_icp_microbench.py -- P x (`points` memory rows at one per voxel | `points` posed rows), radius 2 * voxel, g0 off by
0.2 degrees and 0.3 voxels:
  normals  ONE ls_cloud_normals_batch_f32 call (grid build, one thread per memory row, the counts)
  self     ONE ls_cloud_nearest_batch_f32 call of the memory onto itself (grid build, one thread per memory row as the query, the counts):
           the same 27-cell walk over the same members
  point K / plane K   both ICPs with max_iter K (--iters) and rel_thr 0, and with max_iter 0: if every problem ran K iterations,
           (icp K - icp 0) / K is ONE ITERATION with all P problems live.  The slab is FILLED with points, so its normals mean little; the
           figure is the cost of the gather and of 28 moments against 15, not a convergence claim
A surface -- P synth.canonical_shape clouds merged at `voxel` against noisy (sigma 0.002) half views of another draw of the same shape, from a
start 2 degrees and 0.015 off, radius 3 * voxel, normals at 3 * voxel:
  both metrics at the defaults of ops (max_iter 100, rel_thr 1e-6; min_matched 3 | 6): iterations, stop codes, the whole-call time (the
  plane form with and without its normals call) and the mean distance of the posed rows to their images under the true pose."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from livingscenes_amd import _lib, ops, synth  # noqa: E402
from cloud_icp_microbench import rodrigues  # noqa: E402
from cloud_nearest_microbench import median_ms  # noqa: E402


class Calls:
    """the four library calls on one packed workload, with their output buffers"""

    def __init__(self, As, Bs, g0, r, dev):
        self.dev, self.P = dev, len(As)
        P = self.P
        self.A, self.B, self.g0 = torch.cat(As), torch.cat(Bs), g0
        self.ao, self.bo = ops._offsets([x.shape[0] for x in As]), ops._offsets([x.shape[0] for x in Bs])
        self.rad = np.full(P, r, np.float32)
        a, b = self.A.shape[0], self.B.shape[0]
        n = max(a, b)
        self.idx, self.d2 = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, device=dev)
        self.counts, self.sums = torch.empty(P, 3, dtype=torch.int64, device=dev), torch.empty(P, dtype=torch.float64, device=dev)
        self.status = torch.empty(P, dtype=torch.int32, device=dev)
        self.g_out = torch.empty(P, 3, 4, device=dev)
        self.stop, self.iters = torch.empty(P, dtype=torch.int32, device=dev), torch.empty(P, dtype=torch.int32, device=dev)
        self.planar, self.rho2 = torch.empty(P, dtype=torch.int64, device=dev), torch.empty(P, dtype=torch.float64, device=dev)
        self.N, self.cnt, self.var = torch.empty(a, 3, device=dev), torch.empty(a, dtype=torch.int32, device=dev), torch.empty(a, device=dev)
        self.ncounts = torch.empty(P, 2, dtype=torch.int64, device=dev)
        lib = _lib.load()
        self.ws = torch.empty(max(lib.ls_cloud_icp_plane_batch_workspace_bytes(P, a, max(a, b)), lib.ls_cloud_normals_batch_workspace_bytes(P, a)),
                              dtype=torch.uint8, device=dev)
        self.st = _lib.stream_ptr(dev)

    def normals(self, radius=None, min_nbrs=5):
        rad = self.rad if radius is None else np.full(self.P, radius, np.float32)
        _lib.call(self.dev, "ls_cloud_normals_batch_f32", self.P, _lib.ptr(self.A), self.A.shape[0], ops._hptr(self.ao), ops._hptr(rad), min_nbrs,
                  _lib.ptr(self.N), _lib.ptr(self.cnt), _lib.ptr(self.var), _lib.ptr(self.ncounts), _lib.ptr(self.status), _lib.ptr(self.ws),
                  self.ws.numel(), self.st)

    def self_search(self):
        _lib.call(self.dev, "ls_cloud_nearest_batch_f32", self.P, _lib.ptr(self.A), self.A.shape[0], ops._hptr(self.ao), _lib.ptr(self.A),
                  self.A.shape[0], ops._hptr(self.ao), None, ops._hptr(self.rad), _lib.ptr(self.idx), _lib.ptr(self.d2), _lib.ptr(self.counts),
                  _lib.ptr(self.sums), _lib.ptr(self.status), _lib.ptr(self.ws), self.ws.numel(), self.st)

    def point(self, max_iter, rel_thr):
        _lib.call(self.dev, "ls_cloud_icp_batch_f32", self.P, _lib.ptr(self.A), self.A.shape[0], ops._hptr(self.ao), _lib.ptr(self.B),
                  self.B.shape[0], ops._hptr(self.bo), _lib.ptr(self.g0), ops._hptr(self.rad), max_iter, rel_thr, 3, _lib.ptr(self.g_out),
                  _lib.ptr(self.stop), _lib.ptr(self.iters), _lib.ptr(self.idx), _lib.ptr(self.d2), _lib.ptr(self.counts), _lib.ptr(self.sums),
                  _lib.ptr(self.status), None, None, _lib.ptr(self.ws), self.ws.numel(), self.st)

    def plane(self, max_iter, rel_thr):
        _lib.call(self.dev, "ls_cloud_icp_plane_batch_f32", self.P, _lib.ptr(self.A), _lib.ptr(self.N), self.A.shape[0], ops._hptr(self.ao),
                  _lib.ptr(self.B), self.B.shape[0], ops._hptr(self.bo), _lib.ptr(self.g0), ops._hptr(self.rad), max_iter, rel_thr, 6,
                  _lib.ptr(self.g_out), _lib.ptr(self.stop), _lib.ptr(self.iters), _lib.ptr(self.idx), _lib.ptr(self.d2), _lib.ptr(self.counts),
                  _lib.ptr(self.sums), _lib.ptr(self.planar), _lib.ptr(self.rho2), _lib.ptr(self.status), None, None, _lib.ptr(self.ws),
                  self.ws.numel(), self.st)

    def result(self):
        torch.cuda.synchronize()
        assert not self.status.any()
        return self.iters.cpu().numpy().copy(), self.stop.cpu().numpy().copy(), self.g_out.double().cpu()


def slab(P, n, h, dev):
    """the workload of scripts/cloud_icp_microbench.py -> (As, Bs, g0)"""
    gen = torch.Generator().manual_seed(0)
    scale = torch.tensor([2.0, 1.2, 0.04]) * (n / 60000) ** (1 / 3) * (h / 0.01)
    raw = [((torch.rand(3 * n, 3, generator=gen) - 0.5) * scale).to(dev) for _ in range(P)]
    mem = ops.cloud_merge_batch(raw, [x[:0] for x in raw], voxel=h)
    assert all(m[0].shape[0] >= n for m in mem), "too few voxels for the memory rows asked for"
    As = [m[0][:n].contiguous() for m in mem]
    g = torch.empty(P, 3, 4, dtype=torch.float64)
    for p in range(P):
        q, _ = torch.linalg.qr(torch.randn(3, 3, generator=gen, dtype=torch.float64))
        g[p, :, :3], g[p, :, 3] = q, torch.rand(3, generator=gen, dtype=torch.float64) - 0.5
    Bs = []
    for p in range(P):
        y = ((torch.rand(n, 3, generator=gen) - 0.5) * scale).double()
        Bs.append(((y - g[p, :, 3]) @ g[p, :, :3]).float().to(dev).contiguous())
    rng = np.random.default_rng(0)
    g0 = torch.empty(P, 3, 4, dtype=torch.float64)
    for p in range(P):
        dR = torch.from_numpy(rodrigues(rng.standard_normal(3), 0.2))
        shift = rng.standard_normal(3)
        g0[p, :, :3], g0[p, :, 3] = dR @ g[p, :, :3], dR @ g[p, :, 3] + torch.from_numpy(0.3 * h * shift / np.linalg.norm(shift))
    return As, Bs, g0.float().to(dev).contiguous()


def surface(P, n, h, dev):
    """P synth shapes merged at h against noisy half views of another draw, g0 off by 2 degrees about the view's centroid and 0.015
    -> (As, Bs, g0, g_true [P,3,4] float64)"""
    rng = np.random.default_rng(1)
    raw, views, g_true, g0 = [], [], [], []
    for p in range(P):
        full = synth.canonical_shape(n, p).astype(np.float64)
        other = synth.canonical_shape(max(n // 3, 1000) + 1, p).astype(np.float64)
        half = other[other[:, 0] > 0.5 * (full[:, 0].max() + full[:, 0].min())]
        pts = half + rng.normal(0, 0.002, half.shape)
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        q *= np.sign(np.linalg.det(q))
        gt = np.concatenate([q, rng.uniform(-1, 1, (3, 1))], 1)           # takes the view into the memory's frame
        views.append(torch.from_numpy(((pts - gt[:, 3]) @ gt[:, :3]).astype(np.float32)).to(dev))
        c = half.mean(0)
        dR = rodrigues(rng.standard_normal(3), 2.0)
        shift = rng.standard_normal(3)
        d = np.concatenate([dR, (c - dR @ c + 0.015 * shift / np.linalg.norm(shift)).reshape(3, 1)], 1)
        g0.append(np.concatenate([d[:, :3] @ gt[:, :3], d[:, :3] @ gt[:, 3:] + d[:, 3:]], 1))
        g_true.append(gt)
        raw.append(torch.from_numpy(full.astype(np.float32)).to(dev))
    mem = ops.cloud_merge_batch(raw, [x[:0] for x in raw], voxel=h)
    return [m[0].contiguous() for m in mem], views, torch.from_numpy(np.stack(g0)).float().to(dev).contiguous(), torch.from_numpy(np.stack(g_true))


def image_distance(Bs, g, g_true):
    """mean over the problems of the mean distance between the rows under g and under the true pose"""
    out = []
    for p, B in enumerate(Bs):
        x = B.double().cpu()
        out.append(float(torch.linalg.norm((x @ g[p, :, :3].T + g[p, :, 3]) - (x @ g_true[p, :, :3].T + g_true[p, :, 3]), dim=1).mean()))
    return float(np.mean(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=64)
    ap.add_argument("--points", type=int, default=60000)
    ap.add_argument("--voxel", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--shape-points", type=int, default=20000)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    P, n, h, K = a.instances, a.points, a.voxel, a.iters
    names = "(converged, max_iter, starved, degenerate)"

    As, Bs, g0 = slab(P, n, h, dev)
    w = Calls(As, Bs, g0, 2 * h, dev)
    w.normals()
    torch.cuda.synchronize()
    nc = w.ncounts.cpu().numpy()
    cnt = w.cnt.cpu().numpy()
    fns = [w.normals, w.self_search, lambda: w.point(0, 0.0), lambda: w.point(K, 0.0), lambda: w.plane(0, 0.0), lambda: w.plane(K, 0.0)]
    (t_n, t_s, t_p0, t_pk, t_q0, t_qk), spread = median_ms(fns, a.reps)
    print(f"slab: instances {P} x ({n} memory rows, {n} queries), voxel {h}, radius {2 * h}; workspace {w.ws.numel() / 2 ** 20:.0f} MiB")
    print(f"normals  {t_n:9.3f} ms (min {spread[0][0]:.3f}, max {spread[0][1]:.3f}); valid rows {nc[:, 1].sum()} of {nc[:, 0].sum()}; neighbours "
          f"min {cnt.min()} median {int(np.median(cnt))} max {cnt.max()}")
    print(f"self     {t_s:9.3f} ms (min {spread[1][0]:.3f}, max {spread[1][1]:.3f}); normals / self = {t_n / t_s:.2f}")
    w.point(K, 0.0)
    it_p = w.result()[0]
    w.plane(K, 0.0)
    it_q, stop_q, _ = w.result()
    print(f"point 0  {t_p0:9.3f} ms; point {K} {t_pk:9.3f} ms; iterations min {it_p.min()} max {it_p.max()}")
    print(f"plane 0  {t_q0:9.3f} ms; plane {K} {t_qk:9.3f} ms; iterations min {it_q.min()} max {it_q.max()}; stop codes "
          f"{np.bincount(stop_q, minlength=4).tolist()} {names}")
    Kc = int(min(it_p.min(), it_q.min()))
    if 1 <= Kc < K:                                                       # a linearised step raised E somewhere: time the iterations all problems ran
        print(f"some problems stopped before {K} iterations: timing max_iter {Kc}, which every problem ran")
        (t_pk, t_qk), _ = median_ms([lambda: w.point(Kc, 0.0), lambda: w.plane(Kc, 0.0)], a.reps)
        print(f"point {Kc}  {t_pk:9.3f} ms; plane {Kc}  {t_qk:9.3f} ms")
    if Kc >= 1:
        per_p, per_q = (t_pk - t_p0) / Kc, (t_qk - t_q0) / Kc
        print(f"one iteration with all {P} problems live: point {per_p:.3f} ms, plane {per_q:.3f} ms, plane / point = {per_q / per_p:.2f}")
    else:
        print("some problems stopped at once: no per-iteration figure from this run")
    del w, As, Bs

    As, Bs, g0, g_true = surface(P, a.shape_points, h, dev)
    r = 3 * h
    w = Calls(As, Bs, g0, r, dev)
    w.normals()
    torch.cuda.synchronize()
    nc, cnt = w.ncounts.cpu().numpy(), w.cnt.cpu().numpy()

    def plane_with_normals():
        w.normals()
        w.plane(100, 1e-6)

    fns = [lambda: w.point(100, 1e-6), lambda: w.plane(100, 1e-6), plane_with_normals, w.normals]
    (t_p, t_q, t_qn, t_n), spread = median_ms(fns, a.reps)
    sizes_a, sizes_b = [x.shape[0] for x in As], [x.shape[0] for x in Bs]
    print(f"surface: instances {P} x (memory rows {min(sizes_a)} - {max(sizes_a)}, queries {min(sizes_b)} - {max(sizes_b)}), voxel {h}, radius {r}; "
          f"normals: valid rows {nc[:, 1].sum()} of {nc[:, 0].sum()}, neighbours min {cnt.min()} median {int(np.median(cnt))} max {cnt.max()}; "
          f"start: mean distance to the true-pose images {image_distance(Bs, g0.double().cpu(), g_true):.3e}")
    for name, fn, t, sp in (("point", lambda: w.point(100, 1e-6), t_p, spread[0]), ("plane", lambda: w.plane(100, 1e-6), t_q, spread[1])):
        fn()
        it, stop, g = w.result()
        print(f"{name}    {t:9.3f} ms (min {sp[0]:.3f}, max {sp[1]:.3f}); iterations min {it.min()} median {int(np.median(it))} max {it.max()}, sum "
              f"{it.sum()}; stop codes {np.bincount(stop, minlength=4).tolist()} {names}; mean distance to the true-pose images "
              f"{image_distance(Bs, g, g_true):.3e}")
    print(f"plane with its normals call {t_qn:9.3f} ms (normals alone {t_n:.3f} ms); point / plane-with-normals = {t_p / t_qn:.2f}")


if __name__ == "__main__":
    main()
