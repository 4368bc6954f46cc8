"""Scene-memory trimmed ICP (csrc/cloudnear.hip: ls_cloud_icp_batch_f32) against its yardstick, ONE ls_cloud_nearest_batch_f32 call.

    python scripts/cloud_icp_microbench.py [--instances 64] [--points 60000] [--voxel 0.01] [--reps 20] [--iters 4]

The workload of scripts/cloud_nearest_microbench.py: P instances of `points` memory rows -- one per voxel of edge `voxel`, made by
ops.cloud_merge_batch from samples of a slab -- against `points` observation rows of the same slab given in another frame; radius 2 * voxel.
The initial pose is the true one off by 0.2 degrees about the slab's centre and 0.3 voxels, so the iterations have something to do.  Timed
with device events after warm-up, median of `reps`, the forms alternating, all on pre-packed inputs (the library calls alone: no torch.cat,
no host read):
  icp      the whole call with the defaults of ops.cloud_icp_batch (max_iter 100, rel_thr 1e-6); the iterations every problem ran are reported
  icp 0    max_iter 0: the grid build, one search with its moments, the solve kernel, the hit flags and the counts
  icp K    max_iter K (--iters) with rel_thr 0, which stops a problem only when its cost does not fall: if every problem ran K iterations,
           (icp K - icp 0) / K is the cost of ONE ITERATION with all P problems live -- a search under the current pose with the float64
           moments, and the solve kernel
  search   one ls_cloud_nearest_batch_f32 call on the same inputs and the same initial pose: grid build, one search, the counts
An iteration repeats the search's probe walk, adds the moments and the solve, and skips the grid build; `ratio` = iteration / search."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from livingscenes_amd import _lib, ops  # noqa: E402
from cloud_nearest_microbench import median_ms  # noqa: E402


def rodrigues(axis, deg):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    a = np.deg2rad(deg)
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=64)
    ap.add_argument("--points", type=int, default=60000)
    ap.add_argument("--voxel", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--iters", type=int, default=4)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    P, n, h, K = a.instances, a.points, a.voxel, a.iters
    r = 2 * h
    gen = torch.Generator().manual_seed(0)
    scale = torch.tensor([2.0, 1.2, 0.04]) * (n / 60000) ** (1 / 3) * (h / 0.01)
    raw = [((torch.rand(3 * n, 3, generator=gen) - 0.5) * scale).to(dev) for _ in range(P)]
    mem = ops.cloud_merge_batch(raw, [x[:0] for x in raw], voxel=h)
    assert all(m[0].shape[0] >= n for m in mem), "too few voxels for the memory rows asked for"
    As = [m[0][:n].contiguous() for m in mem]
    del raw, mem
    g = torch.empty(P, 3, 4, dtype=torch.float64)
    for p in range(P):
        q, _ = torch.linalg.qr(torch.randn(3, 3, generator=gen, dtype=torch.float64))
        g[p, :, :3], g[p, :, 3] = q, torch.rand(3, generator=gen, dtype=torch.float64) - 0.5
    Bs = []
    for p in range(P):
        y = ((torch.rand(n, 3, generator=gen) - 0.5) * scale).double()
        Bs.append(((y - g[p, :, 3]) @ g[p, :, :3]).float().to(dev).contiguous())         # g[p] takes it back onto the slab
    rng = np.random.default_rng(0)
    g0 = torch.empty(P, 3, 4, dtype=torch.float64)
    for p in range(P):                                                    # a rotation about the slab's centre (the origin) and a shift
        dR = torch.from_numpy(rodrigues(rng.standard_normal(3), 0.2))
        shift = rng.standard_normal(3)
        g0[p, :, :3], g0[p, :, 3] = dR @ g[p, :, :3], dR @ g[p, :, 3] + torch.from_numpy(0.3 * h * shift / np.linalg.norm(shift))
    g0 = g0.float().to(dev).contiguous()
    A, B = torch.cat(As), torch.cat(Bs)
    ao, bo = ops._offsets([n] * P), ops._offsets([n] * P)
    rad = np.full(P, r, np.float32)
    idx, d2 = torch.empty(P * n, dtype=torch.int32, device=dev), torch.empty(P * n, device=dev)
    counts, sums = torch.empty(P, 3, dtype=torch.int64, device=dev), torch.empty(P, dtype=torch.float64, device=dev)
    status = torch.empty(P, dtype=torch.int32, device=dev)
    g_out = torch.empty(P, 3, 4, device=dev)
    stop, iters = torch.empty(P, dtype=torch.int32, device=dev), torch.empty(P, dtype=torch.int32, device=dev)
    lib = _lib.load()
    ws = torch.empty(lib.ls_cloud_icp_batch_workspace_bytes(P, A.shape[0], B.shape[0]), dtype=torch.uint8, device=dev)
    assert ws.numel() >= lib.ls_cloud_nearest_batch_workspace_bytes(P, A.shape[0], B.shape[0])
    st = _lib.stream_ptr(dev)

    def icp(max_iter, rel_thr):
        def run():
            _lib.call(dev, "ls_cloud_icp_batch_f32", P, _lib.ptr(A), A.shape[0], ops._hptr(ao), _lib.ptr(B), B.shape[0], ops._hptr(bo), _lib.ptr(g0),
                      ops._hptr(rad), max_iter, rel_thr, 3, _lib.ptr(g_out), _lib.ptr(stop), _lib.ptr(iters), _lib.ptr(idx), _lib.ptr(d2),
                      _lib.ptr(counts), _lib.ptr(sums), _lib.ptr(status), None, None, _lib.ptr(ws), ws.numel(), st)
        return run

    def search():
        _lib.call(dev, "ls_cloud_nearest_batch_f32", P, _lib.ptr(A), A.shape[0], ops._hptr(ao), _lib.ptr(B), B.shape[0], ops._hptr(bo), _lib.ptr(g0),
                  ops._hptr(rad), _lib.ptr(idx), _lib.ptr(d2), _lib.ptr(counts), _lib.ptr(sums), _lib.ptr(status), _lib.ptr(ws), ws.numel(), st)

    full, zero, fixed = icp(100, 1e-6), icp(0, 1e-6), icp(K, 0.0)
    (t_full, t_zero, t_fixed, t_search), spread = median_ms([full, zero, fixed, search], a.reps)
    search()
    torch.cuda.synchronize()
    c_search = counts.cpu().numpy().copy()
    fixed()
    torch.cuda.synchronize()
    it_fixed = iters.cpu().numpy().copy()
    full()
    torch.cuda.synchronize()
    assert not status.any()
    it_full, stop_full, c_full = iters.cpu().numpy(), stop.cpu().numpy(), counts.cpu().numpy()
    err0 = float(torch.linalg.norm((g0.double().cpu() - g)[:, :, 3], dim=1).mean())
    err1 = float(torch.linalg.norm((g_out.double().cpu() - g)[:, :, 3], dim=1).mean())
    print(f"instances {P} x ({n} memory rows, {n} queries), voxel {h}, radius {r}; workspace {ws.numel() / 2 ** 20:.0f} MiB")
    print(f"icp      {t_full:9.3f} ms (min {spread[0][0]:.3f}, max {spread[0][1]:.3f}); iterations per problem: min {it_full.min()} median "
          f"{int(np.median(it_full))} max {it_full.max()}; stop codes {np.bincount(stop_full, minlength=4).tolist()} (converged, max_iter, starved, "
          f"degenerate); matched {c_search[:, 1].sum()} -> {c_full[:, 1].sum()} of {P * n}; mean |t - t_true| {err0:.5f} -> {err1:.5f}")
    print(f"icp 0    {t_zero:9.3f} ms (min {spread[1][0]:.3f}, max {spread[1][1]:.3f})")
    print(f"icp {K:<4d} {t_fixed:9.3f} ms (min {spread[2][0]:.3f}, max {spread[2][1]:.3f}); iterations per problem: min {it_fixed.min()} max {it_fixed.max()}")
    print(f"search   {t_search:9.3f} ms (min {spread[3][0]:.3f}, max {spread[3][1]:.3f})")
    if it_fixed.min() == K:
        per = (t_fixed - t_zero) / K
        print(f"one iteration with all {P} problems live: {per:.3f} ms = {per / t_search:.2f} of the search call; first search of the ICP with its "
              f"moments and solve: icp 0 / search = {t_zero / t_search:.2f}")
    else:
        print(f"some problems stopped before {K} iterations: no per-iteration figure from this run")
    print(f"whole call / (1 + max iterations) = {t_full / (1 + it_full.max()):.3f} ms per search of the longest problem, the empty launches after it included")


if __name__ == "__main__":
    main()
