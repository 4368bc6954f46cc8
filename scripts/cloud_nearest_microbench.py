"""Scene-memory radius search (csrc/cloudnear.hip) against the same statistics formed from torch device ops.

    python scripts/cloud_nearest_microbench.py [--instances 64] [--points 60000] [--voxel 0.01] [--reps 20]

P instances of `points` memory rows -- one per voxel of edge `voxel`, made by ops.cloud_merge_batch from samples of a slab -- against
`points` observation rows of the same slab given in another frame, with the pose that brings them back; radius 2 * voxel.  Timed with
device events after warm-up, median of `reps`, the two forms alternating:
  op     ONE ls_cloud_nearest_batch_f32 call on pre-packed inputs (the library call alone: no torch.cat, no host read)
  torch  per instance: the observation posed with a matmul, torch.cdist against the memory in chunks of 4096 queries, min over the
         memory, the radius test, and the three counts (torch.unique of the neighbours for the third) -- the cell condition left out
and the counts of both are compared.  Bytes: `min` = what any method must move (read every row once, write index and distance per query),
`kernels` = what this operator's passes move, counted from the code (see below; the members a query scans are counted from the data);
both over the op's time, against the 8.0 TB/s HBM peak."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from livingscenes_amd import _lib, ops  # noqa: E402

HBM_PEAK = 8.0e12
CHUNK = 4096


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


def torch_form(As, Bs, g, r):
    """-> counts [P,3] and sum of squared distances [P], on the device"""
    counts, sums = [], []
    for p, (A, B) in enumerate(zip(As, Bs)):
        Y = B @ g[p, :, :3].T + g[p, :, 3]
        best, arg = [], []
        for s in range(0, Y.shape[0], CHUNK):
            d, j = torch.cdist(Y[s:s + CHUNK], A).min(1)
            best.append(d), arg.append(j)
        d, j = torch.cat(best), torch.cat(arg)
        has = d <= r
        counts.append(torch.stack([torch.isfinite(Y).all(1).sum(), has.sum(), torch.unique(j[has]).numel() + 0 * has.sum()]))
        sums.append((d[has].double() ** 2).sum())
    return torch.stack(counts), torch.stack(sums)


def members_scanned(A, Y, inv):
    """mean number of memory rows in the 27 cells around a query's cell (one instance; cells in a dense grid)"""
    ca, cy = torch.floor(A * inv).long(), torch.floor(Y * inv).long()
    lo = torch.minimum(ca.min(0)[0], cy.min(0)[0]) - 1
    dims = (torch.maximum(ca.max(0)[0], cy.max(0)[0]) + 2 - lo).tolist()
    grid = torch.zeros(dims, device=A.device)
    ca, cy = ca - lo, cy - lo
    grid.index_put_((ca[:, 0], ca[:, 1], ca[:, 2]), torch.ones(ca.shape[0], device=A.device), accumulate=True)
    box = torch.nn.functional.avg_pool3d(grid[None, None], 3, stride=1, padding=1, divisor_override=1)[0, 0]
    return float(box[cy[:, 0], cy[:, 1], cy[:, 2]].mean()), int((grid > 0).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=64)
    ap.add_argument("--points", type=int, default=60000)
    ap.add_argument("--voxel", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    P, n, h = a.instances, a.points, a.voxel
    r = 2 * h
    gen = torch.Generator().manual_seed(0)
    scale = torch.tensor([2.0, 1.2, 0.04]) * (n / 60000) ** (1 / 3) * (h / 0.01)      # some 1.6 voxels of the slab per memory row
    raw = [((torch.rand(3 * n, 3, generator=gen) - 0.5) * scale).to(dev) for _ in range(P)]
    mem = ops.cloud_merge_batch(raw, [x[:0] for x in raw], voxel=h)
    assert all(m[0].shape[0] >= n for m in mem), "too few voxels for the memory rows asked for"
    As = [m[0][:n].contiguous() for m in mem]
    del raw, mem
    g = torch.empty(P, 3, 4)
    for p in range(P):
        q, _ = torch.linalg.qr(torch.randn(3, 3, generator=gen))
        g[p, :, :3], g[p, :, 3] = q, torch.rand(3, generator=gen) - 0.5
    g = g.to(dev)
    Bs = []
    for p in range(P):
        y = ((torch.rand(n, 3, generator=gen) - 0.5) * scale).to(dev)
        Bs.append(((y - g[p, :, 3]) @ g[p, :, :3]).contiguous())          # g[p] takes it back onto the slab: R (R^T (y - t)) + t
    A, B = torch.cat(As), torch.cat(Bs)
    ao, bo = ops._offsets([n] * P), ops._offsets([n] * P)
    rad = np.full(P, r, np.float32)
    idx, d2 = torch.empty(P * n, dtype=torch.int32, device=dev), torch.empty(P * n, device=dev)
    counts, sums = torch.empty(P, 3, dtype=torch.int64, device=dev), torch.empty(P, dtype=torch.float64, device=dev)
    status = torch.empty(P, dtype=torch.int32, device=dev)
    lib = _lib.load()
    ws = torch.empty(lib.ls_cloud_nearest_batch_workspace_bytes(P, A.shape[0], B.shape[0]), dtype=torch.uint8, device=dev)
    st = _lib.stream_ptr(dev)

    def op():
        _lib.call(dev, "ls_cloud_nearest_batch_f32", P, _lib.ptr(A), A.shape[0], ops._hptr(ao), _lib.ptr(B), B.shape[0], ops._hptr(bo), _lib.ptr(g),
                  ops._hptr(rad), _lib.ptr(idx), _lib.ptr(d2), _lib.ptr(counts), _lib.ptr(sums), _lib.ptr(status), _lib.ptr(ws), ws.numel(), st)
    ref = []

    def tf():
        ref[:] = torch_form(As, Bs, g, r)
    (t_op, t_torch), spread = median_ms([op, tf], a.reps)
    assert not status.any()
    c_op, c_t = counts.cpu().numpy(), ref[0].cpu().numpy()
    s_op, s_t = sums.cpu().numpy(), ref[1].cpu().numpy()
    scanned, cells = members_scanned(As[0], Bs[0] @ g[0, :, :3].T + g[0, :, 3], float(np.float32(1) / np.float32(r)))
    Na, Nb = P * n, P * n
    min_bytes = Na * 12 + Nb * 12 + Nb * 8
    # per memory row -- cleared: table 8, count 8, hit 1; cell: read 12, write 12; claim: read 12, table atomic 4 + the occupant's cell 12 (per
    # probe, one counted), count atomic 4, write 4 + 4; scan over 2 slots: read 4 twice, write 4; slot record, 2 slots: read 4 + 4, write 16, and
    # the cell 12 of an occupied one; fill: read 12 + 4 + 4 + 4, write 16; the last kernel reads the hit flag 1
    # per query -- read 12, write 8; 27 probe walks of one 16-byte slot record each (one step counted); per found cell its count 4 (left out)
    # and 16 bytes per member scanned; the partial sums 16 per 256 queries
    per_target = 17 + 24 + 40 + 24 + 48 + 12 * cells / n + 40 + 1
    per_query = 12 + 8 + 27 * 16 + 16 * scanned + 16 / 256
    kern_bytes = Na * per_target + Nb * per_query
    print(f"instances {P} x ({n} memory rows, {n} queries), voxel {h}, radius {r}: {cells} cells in instance 0, {scanned:.1f} members scanned per query")
    print(f"counts (finite, matched, memory rows seen), summed over the instances: op {c_op.sum(0).tolist()}  torch {c_t.sum(0).tolist()}; "
          f"instances whose counts differ, per count: {(c_op != c_t).sum(0).tolist()}, largest difference {np.abs(c_op - c_t).max(0).tolist()}; "
          f"rmse op {np.sqrt(s_op.sum() / c_op[:, 1].sum()):.6f} torch {np.sqrt(s_t.sum() / c_t[:, 1].sum()):.6f}")
    print(f"op     {t_op:9.3f} ms (min {spread[0][0]:.3f}, max {spread[0][1]:.3f}); workspace {ws.numel() / 2 ** 20:.0f} MiB")
    print(f"torch  {t_torch:9.3f} ms (min {spread[1][0]:.3f}, max {spread[1][1]:.3f}); ratio {t_torch / t_op:.1f}x")
    print(f"bytes  min {min_bytes / 1e6:.0f} MB -> {min_bytes / t_op / 1e9:.3f} TB/s ({100 * min_bytes / (t_op * 1e-3) / HBM_PEAK:.1f} % of the 8.0 TB/s HBM peak); "
          f"kernels {kern_bytes / 1e6:.0f} MB ({per_target:.0f} per memory row, {per_query:.0f} per query) -> {kern_bytes / t_op / 1e9:.3f} TB/s "
          f"({100 * kern_bytes / (t_op * 1e-3) / HBM_PEAK:.1f} %)")


if __name__ == "__main__":
    main()
