"""Scene-memory carve (csrc/cloudcarve.hip) against the same states formed from torch device ops, and beside the radius search.

    python scripts/cloud_carve_microbench.py [--instances 64] [--points 60000] [--views 8] [--size 100] [--tol 0.01] [--reps 20]

P instances of `points` kept rows -- half of them on a sphere of radius 0.3, half on a copy of it displaced by (0.12, 0.05, -0.08) --
against `views` depth views of size x size pixels (f = size, the camera 1.5 from the origin) that hold the analytic depth of the sphere,
0 elsewhere; window 1, empty pixels free.  Timed with device events after warm-up, median of `reps`, the forms alternating:
  op      ONE ls_cloud_carve_batch_f32 call on pre-packed inputs (the library call alone: no torch.cat, no host read, no `state`)
  torch   all instances at once: the float64 projection as three batched products, floor, nine indexed gathers per (row, view), the
          classes and the states as tensor expressions, the per-view histogram by bincount -- no compaction, which the op does make
  search  ONE ls_cloud_nearest_batch_f32 call at the same row counts (the kept rows as targets, the same rows jittered by 2 mm as
          queries, radius 0.01): the operator a step already pays for, as a yardstick
The histograms of op and torch are compared (torch contracts and orders its float64 products as it likes, so a row at a boundary may
differ).  Bytes: `min` = what any method must move (read every row and every image once, write seen / free per row and point and index
per kept row), `kernels` = what this operator's passes move, counted from the code; both over the op's time, against the 8.0 TB/s HBM
peak."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from livingscenes_amd import _lib, ops, render  # noqa: E402

HBM_PEAK = 8.0e12


def median_ms(fns, reps):
    """every fn warmed up, then timed `reps` times in turn -> the medians"""
    for fn in fns:
        fn(), fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    return [float(np.median(t)) for t in times], [(float(np.min(t)), float(np.max(t))) for t in times]


def sphere_depth(E, K, H, W, radius):
    """the analytic depth of the sphere of `radius` at the origin under the cameras E [V,3,4] float64 -> [V,H,W] fp32, 0 where the ray misses"""
    py, px = torch.meshgrid(torch.arange(H, device=E.device, dtype=torch.float64), torch.arange(W, device=E.device, dtype=torch.float64), indexing="ij")
    out = []
    for v in range(E.shape[0]):
        fx, fy, cx, cy = K[v].tolist()
        d = torch.stack([(px - cx) / fx, (py - cy) / fy, torch.ones_like(px)], -1)     # the ray through the integer pixel coordinate, z = 1
        c = E[v, :, 3]                                                                  # the sphere's centre in the camera frame
        a, b = (d * d).sum(-1), -2.0 * (d @ c)
        disc = b * b - 4.0 * a * (c @ c - radius ** 2)
        t = (-b - torch.sqrt(disc.clamp_min(0))) / (2.0 * a)
        out.append(torch.where(disc > 0, t, torch.zeros_like(t)).float())
    return torch.stack(out)


def torch_form(A, D, K, E, tol, znear, k):
    """A [P,n,3] fp32, D [P,V,H,W], K [P,V,4], E [P,V,3,4] -> states uint8 [P,V,n] and view_counts [P,V,5], empty pixels free"""
    P, V, H, W = D.shape
    x = A.double()
    c = torch.einsum("pvrc,pnc->pvnr", E[..., :3], x) + E[..., 3][:, :, None, :]
    z = c[..., 2]
    ok = torch.isfinite(c).all(-1) & ~(z < znear)
    u = K[:, :, None, 0] * (c[..., 0] / z) + K[:, :, None, 2]
    v = K[:, :, None, 1] * (c[..., 1] / z) + K[:, :, None, 3]
    rx, ry = torch.floor(u + 0.5), torch.floor(v + 0.5)
    ok &= (rx >= 0) & (rx <= W - 1) & (ry >= 0) & (ry <= H - 1)
    qx, qy = torch.where(ok, rx, 0.0).long(), torch.where(ok, ry, 0.0).long()
    flat = D.reshape(P, V, H * W)
    n_in = torch.zeros_like(qx)
    n_hit, n_front, n_behind, n_empty = (torch.zeros_like(qx) for _ in range(4))
    for dy in range(-k, k + 1):
        for dx in range(-k, k + 1):
            yy, xx = qy + dy, qx + dx
            inside = ok & (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            d = torch.gather(flat, 2, yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).double()
            empty = ~(d > 0)
            front = ~empty & (z < d - tol)
            behind = ~empty & ~front & (z > d + tol)
            n_in += inside
            n_hit += inside & ~empty & ~front & ~behind
            n_front += inside & front
            n_behind += inside & behind
            n_empty += inside & empty
    st = torch.where(n_hit > 0, 1, torch.where(n_front + n_empty == n_in, 2, torch.where((n_behind > 0) & (n_front == 0), 3, 4)))
    st = torch.where(ok, st, 0)
    hist = torch.stack([(st == s).sum(-1) for s in range(5)], -1)
    return st.to(torch.uint8), hist


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=64)
    ap.add_argument("--points", type=int, default=60000)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--size", type=int, default=100)
    ap.add_argument("--tol", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    P, n, V, H, W, tol, znear, k = a.instances, a.points, a.views, a.size, a.size, a.tol, 0.05, 1
    gen = torch.Generator().manual_seed(0)
    As, Es = [], []
    for p in range(P):
        d = torch.randn(n, 3, generator=gen)
        x = 0.3 * d / d.norm(dim=1, keepdim=True)
        x[n // 2:] += torch.tensor([0.12, 0.05, -0.08])
        As.append(x.to(dev))
        Es.append(torch.from_numpy(np.stack([render.world_to_cam(q) for q in render.gen_random_poses(V, seed=p)])).to(dev))
    K1 = torch.tensor([float(W), float(H), W / 2.0, H / 2.0], dtype=torch.float64, device=dev).expand(V, 4).contiguous()
    Ds = [sphere_depth(E, K1, H, W, 0.3) for E in Es]
    A, D, K, E = torch.cat(As), torch.cat(Ds), K1.repeat(P, 1), torch.cat(Es)
    ao, vo = ops._offsets([n] * P), ops._offsets([V] * P)
    lib = _lib.load()
    st = _lib.stream_ptr(dev)
    pts, src = torch.empty(P * n, 3, device=dev), torch.empty(P * n, dtype=torch.int32, device=dev)
    off = torch.empty(P + 1, dtype=torch.int64, device=dev)
    seen, free = torch.empty(P * n, dtype=torch.int32, device=dev), torch.empty(P * n, dtype=torch.int32, device=dev)
    counts, vcounts = torch.empty(P, 4, dtype=torch.int64, device=dev), torch.empty(P * V, 5, dtype=torch.int64, device=dev)
    status = torch.empty(P, dtype=torch.int32, device=dev)
    ws = torch.empty(lib.ls_cloud_carve_batch_workspace_bytes(P, P * n, P * V), dtype=torch.uint8, device=dev)

    def op():
        _lib.call(dev, "ls_cloud_carve_batch_f32", P, _lib.ptr(A), P * n, ops._hptr(ao), _lib.ptr(D), P * V, ops._hptr(vo), H, W, _lib.ptr(K),
                  _lib.ptr(E), tol, znear, k, 1, 0, 1, _lib.ptr(pts), _lib.ptr(src), _lib.ptr(off), _lib.ptr(seen), _lib.ptr(free),
                  _lib.ptr(counts), _lib.ptr(vcounts), None, _lib.ptr(status), _lib.ptr(ws), ws.numel(), st)
    ref = []
    A3, D4, K3, E4 = A.reshape(P, n, 3), D.reshape(P, V, H, W), K.reshape(P, V, 4), E.reshape(P, V, 3, 4)

    def tf():
        ref[:] = torch_form(A3, D4, K3, E4, tol, znear, k)

    # the radius search at the same row counts
    Bq = A + 0.002 * torch.randn(P * n, 3, generator=gen).to(dev)
    rad = np.full(P, 0.01, np.float32)
    idx, d2 = torch.empty(P * n, dtype=torch.int32, device=dev), torch.empty(P * n, device=dev)
    ncounts, nsums = torch.empty(P, 3, dtype=torch.int64, device=dev), torch.empty(P, dtype=torch.float64, device=dev)
    nstatus = torch.empty(P, dtype=torch.int32, device=dev)
    nws = torch.empty(lib.ls_cloud_nearest_batch_workspace_bytes(P, P * n, P * n), dtype=torch.uint8, device=dev)

    def search():
        _lib.call(dev, "ls_cloud_nearest_batch_f32", P, _lib.ptr(A), P * n, ops._hptr(ao), _lib.ptr(Bq), P * n, ops._hptr(ao), None,
                  ops._hptr(rad), _lib.ptr(idx), _lib.ptr(d2), _lib.ptr(ncounts), _lib.ptr(nsums), _lib.ptr(nstatus), _lib.ptr(nws), nws.numel(), st)
    (t_op, t_torch, t_search), spread = median_ms([op, tf, search], a.reps)
    assert not status.any() and not nstatus.any()
    h_op, h_t = vcounts.cpu().numpy().reshape(P, V, 5), ref[1].cpu().numpy()
    kept = int(off.cpu()[P])
    rows, pairs = P * n, P * n * V
    min_bytes = rows * 12 + D.numel() * 4 + rows * 8 + kept * 16
    # per row -- carve: read 12, write seen 4, free 4, keep 4; the scan reads keep twice and writes pos: 12; scatter: read keep 4 + pos 4,
    # and per kept row read 12, write 16.  per (row, view) -- (2k+1)^2 gathers of 4 bytes, from L2 once the images are there
    per_row, per_pair = 24 + 12 + 8, (2 * k + 1) ** 2 * 4
    kern_bytes = rows * per_row + kept * 28 + pairs * per_pair + D.numel() * 4
    print(f"instances {P} x {n} kept rows x {V} views of {H} x {W}, tol {tol}, window {k}, empty pixels free: dropped {int(counts[:, 2].sum())} of "
          f"{rows}, kept {kept}")
    print(f"states (out, seen, free, occluded, mixed) over all (row, view) pairs: op {h_op.sum((0, 1)).tolist()}  torch {h_t.sum((0, 1)).tolist()}; "
          f"views whose histograms differ {int((h_op != h_t).any(-1).sum())} of {P * V}, largest difference {int(np.abs(h_op - h_t).max())}")
    print(f"op     {t_op:9.3f} ms (min {spread[0][0]:.3f}, max {spread[0][1]:.3f}); workspace {ws.numel() / 2 ** 20:.0f} MiB; "
          f"{pairs / t_op / 1e6:.1f} G (row, view) pairs / s")
    print(f"torch  {t_torch:9.3f} ms (min {spread[1][0]:.3f}, max {spread[1][1]:.3f}); ratio {t_torch / t_op:.1f}x")
    print(f"search {t_search:9.3f} ms (min {spread[2][0]:.3f}, max {spread[2][1]:.3f}); matched {int(ncounts[:, 1].sum())} of {rows}; "
          f"carve / search {t_op / t_search:.2f}")
    print(f"bytes  min {min_bytes / 1e6:.0f} MB -> {min_bytes / t_op / 1e9:.3f} TB/s ({100 * min_bytes / (t_op * 1e-3) / HBM_PEAK:.1f} % of the 8.0 TB/s HBM peak); "
          f"kernels {kern_bytes / 1e6:.0f} MB ({per_row} per row, {per_pair} per (row, view) from L2) -> {kern_bytes / t_op / 1e9:.3f} TB/s "
          f"({100 * kern_bytes / (t_op * 1e-3) / HBM_PEAK:.1f} %)")


if __name__ == "__main__":
    main()
