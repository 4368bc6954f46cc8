"""Scene-memory merge (csrc/cloudmerge.hip) against the same result formed from torch device ops.

    python scripts/cloud_merge_microbench.py [--instances 64] [--points 60000] [--voxel 0.01] [--reps 20]

P instances of `points` kept + `points` new rows each (a box surface-like slab, so that observations overlap).  Timed with device events
after warm-up, median of `reps`, the two forms alternating:
  op     ONE ls_cloud_merge_batch_f32 call on pre-packed inputs (the library call alone: no torch.cat, no host read)
  torch  per instance: quantise, torch.unique(dim=0, return_inverse=True), scatter_reduce amin of the index, a boolean mask
and the kept rows of both are compared.  Bytes: `min` = what any method must move (read every candidate once, write every kept row and its
index), `kernels` = what this operator's passes move (counted from the code: 12 + 12 + 8 + 12 + 4 .. per candidate, see below); both over
the op's time, against the 8.0 TB/s HBM peak."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from livingscenes_amd import _lib, ops  # noqa: E402

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


def torch_form(As, Bs, inv):
    out = []
    for A, B in zip(As, Bs):
        Y = torch.cat([A, B], 0)
        c = torch.floor(Y * inv).to(torch.int32)
        _, inverse = torch.unique(c, dim=0, return_inverse=True)
        idx = torch.arange(Y.shape[0], device=Y.device)
        first = torch.full((Y.shape[0],), Y.shape[0], device=Y.device, dtype=idx.dtype).scatter_reduce(0, inverse, idx, "amin")
        out.append(Y[first[inverse] == idx])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=64)
    ap.add_argument("--points", type=int, default=60000)
    ap.add_argument("--voxel", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    P, n = a.instances, a.points
    gen = torch.Generator().manual_seed(0)
    scale = torch.tensor([1.0, 0.6, 0.02])
    As = [((torch.rand(n, 3, generator=gen) - 0.5) * scale).to(dev) for _ in range(P)]
    Bs = [((torch.rand(n, 3, generator=gen) - 0.5) * scale + torch.tensor([0.3, 0.0, 0.0])).to(dev) for _ in range(P)]
    A, B = torch.cat(As), torch.cat(Bs)
    ao, bo = ops._offsets([n] * P), ops._offsets([n] * P)
    vox = np.full(P, a.voxel, np.float32)
    N = 2 * n * P
    pts, src = torch.empty(N, 3, device=dev), torch.empty(N, dtype=torch.int32, device=dev)
    off = torch.empty(P + 1, dtype=torch.int64, device=dev)
    lib = _lib.load()
    ws = torch.empty(lib.ls_cloud_merge_batch_workspace_bytes(P, A.shape[0], B.shape[0]), dtype=torch.uint8, device=dev)
    st = _lib.stream_ptr(dev)

    def op():
        _lib.call(dev, "ls_cloud_merge_batch_f32", P, _lib.ptr(A), A.shape[0], ops._hptr(ao), _lib.ptr(B), B.shape[0], ops._hptr(bo), None,
                  ops._hptr(vox), _lib.ptr(pts), _lib.ptr(src), _lib.ptr(off), None, _lib.ptr(ws), ws.numel(), st)
    inv = float(np.float32(1) / np.float32(a.voxel))
    kept = []

    def tf():
        kept[:] = torch_form(As, Bs, inv)
    (t_op, t_torch), spread = median_ms([op, tf], a.reps)
    o = off.cpu().numpy()
    same = all(torch.equal(pts[o[p]:o[p + 1]], kept[p]) for p in range(P))
    n_out = int(o[P])
    min_bytes = N * 12 + n_out * 16
    # cell: read 12, write 12; hash: read 12, table atomic 4 + occupant's cell 12 (per probe, one counted), write 4; keep: read 4 + 4, write 4;
    # scan: read 4 twice, write 4; scatter: read 4 + 4 per candidate, 12 + write 16 per kept row; table cleared: 8
    kern_bytes = N * (24 + 32 + 12 + 12 + 8 + 8) + n_out * 28
    print(f"instances {P} x ({n} + {n}) rows, voxel {a.voxel}: kept {n_out} of {N}; same rows as the torch form: {same}")
    print(f"op     {t_op:9.3f} ms (min {spread[0][0]:.3f}, max {spread[0][1]:.3f}); workspace {ws.numel() / 2 ** 20:.0f} MiB")
    print(f"torch  {t_torch:9.3f} ms (min {spread[1][0]:.3f}, max {spread[1][1]:.3f}); ratio {t_torch / t_op:.1f}x")
    print(f"bytes  min {min_bytes / 1e6:.0f} MB -> {min_bytes / t_op / 1e9:.3f} TB/s ({100 * min_bytes / (t_op * 1e-3) / HBM_PEAK:.1f} % of the 8.0 TB/s HBM peak); "
          f"kernels {kern_bytes / 1e6:.0f} MB -> {kern_bytes / t_op / 1e9:.3f} TB/s ({100 * kern_bytes / (t_op * 1e-3) / HBM_PEAK:.1f} %)")


if __name__ == "__main__":
    main()
