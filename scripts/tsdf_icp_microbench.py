"""Scene-memory sampling of the fused states and the registration on them (csrc/tsdficp.hip) against their yardsticks.

    python scripts/tsdf_icp_microbench.py [--instances 64] [--views 8] [--res 64] [--mesh-res 48] [--points 60000] [--min-obs 1] [--reps 20]

The states of scripts/tsdf_mesh_microbench.py: P synth shapes, `views` rendered depth views each (synth.make_partial_views), fused into P
grids of res^3 samples (trunc = 4 voxels, empty pixels unknown).  Every instance is sampled at `points` rows: rows of its own views'
back-projected clouds drawn with replacement, given in another frame, under a pose that is the true one off by --deg (1) degrees about
the cloud's centre and --shift (1) voxels, so that two updates have something to do -- in no spatial order.  Timed with device events
after warm-up, median of `reps`, the forms alternating, all on pre-packed inputs and outputs already sized (the library calls alone: no
torch.cat, no host read):
  sample   one ls_tsdf_sample_batch_f32 call
  icp 1/2  ls_tsdf_icp_batch_f32 with max_iter 1 and 2 and rel_thr 0 (a problem stops only when its cost does not fall): if every problem
           ran 2 iterations, icp 2 - icp 1 is the cost of ONE ITERATION with all P problems live -- a sample under the current pose with
           the 28 float64 moments, and the solve kernel
  plane    the same difference for ls_cloud_icp_plane_batch_f32 at the same row counts, on the workload of scripts/cloud_icp_microbench.py
           (P slabs of `points` memory rows, one per voxel of 0.01, against `points` observation rows, radius 0.02, normals at 0.03)
  torch    the same sample from torch device ops: gathers and lerps in float64, per problem; its states, counts and values are asserted
           IDENTICAL to the kernel's before anything is timed
Bytes: a query must move 12 in (its row) and 33 out (phi, grad, state); its eight corners are 64 more where no line is shared.  Nothing
here was profiled with counters: the figures are wall times of whole calls."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from livingscenes_amd import _lib, ops, synth  # noqa: E402
from livingscenes_amd.lib_more.more_solver import More_Solver  # noqa: E402
from cloud_icp_microbench import rodrigues  # noqa: E402
from cloud_nearest_microbench import median_ms  # noqa: E402

PEAK = 8.0e12


def torch_sample(S, N, B, g, origin, h, trunc, min_obs):
    """one problem in torch device ops, the definition's order of operations -> (phi, grad, state, counts)"""
    x0, x1, x2 = B[:, 0], B[:, 1], B[:, 2]
    y = torch.stack([((g[a, 0] * x0 + g[a, 1] * x1) + g[a, 2] * x2) + g[a, 3] for a in range(3)], 1)
    dims = torch.tensor(S.shape, device=B.device)
    u = (y.double() - origin) / h
    finite = torch.isfinite(y).all(1)
    inside = finite & ((u >= 0.0) & (u <= (dims - 1).double())).all(1)
    i = torch.minimum(torch.floor(torch.where(inside[:, None], u, torch.zeros_like(u))).long(), dims - 2)
    f = u - i.double()
    D = torch.where(N >= min_obs, S.double() / (N.clamp(min=1).double() * 16384.0), torch.ones((), dtype=torch.float64, device=B.device))
    valid = N >= min_obs
    c = [[[(i[:, 0] + a, i[:, 1] + b, i[:, 2] + c) for c in range(2)] for b in range(2)] for a in range(2)]
    D8 = torch.stack([torch.stack([torch.stack([D[c[a][b][k]] for k in range(2)], -1) for b in range(2)], -2) for a in range(2)], -3)
    seen = torch.stack([valid[c[a][b][k]] for a in range(2) for b in range(2) for k in range(2)], 1).all(1) & inside
    lerp = lambda p, q, t: p + t * (q - p)   # noqa: E731
    f0, f1, f2 = f[:, 0], f[:, 1], f[:, 2]
    a_ = lerp(D8[:, :, :, 0], D8[:, :, :, 1], f2[:, None, None])
    b_ = lerp(a_[:, :, 0], a_[:, :, 1], f1[:, None])
    v = lerp(b_[:, 0], b_[:, 1], f0)
    d2, d1, d0 = D8[:, :, :, 1] - D8[:, :, :, 0], D8[:, :, 1, :] - D8[:, :, 0, :], D8[:, 1, :, :] - D8[:, 0, :, :]
    e2, e1, e0 = lerp(d2[:, :, 0], d2[:, :, 1], f1[:, None]), lerp(d1[:, :, 0], d1[:, :, 1], f2[:, None]), lerp(d0[:, :, 0], d0[:, :, 1], f2[:, None])
    G = torch.stack([lerp(e0[:, 0], e0[:, 1], f1), lerp(e1[:, 0], e1[:, 1], f0), lerp(e2[:, 0], e2[:, 1], f0)], 1)
    phi = torch.where(seen, trunc * v, torch.full_like(v, trunc))
    grad = torch.where(seen[:, None], (trunc / h) * G, torch.zeros_like(G))
    state = inside.to(torch.uint8) + seen.to(torch.uint8)
    return phi, grad, state, torch.stack([finite.sum(), inside.sum(), seen.sum()])


def plane_workload(P, n, dev, gen):
    """the slabs of scripts/cloud_icp_microbench.py with their normals -> the arguments of ls_cloud_icp_plane_batch_f32"""
    h = 0.01
    scale = torch.tensor([2.0, 1.2, 0.04]) * (n / 60000) ** (1 / 3)
    raw = [((torch.rand(3 * n, 3, generator=gen) - 0.5) * scale).to(dev) for _ in range(P)]
    mem = ops.cloud_merge_batch(raw, [x[:0] for x in raw], voxel=h)
    assert all(m[0].shape[0] >= n for m in mem), "too few voxels for the memory rows asked for"
    As = [m[0][:n].contiguous() for m in mem]
    del raw, mem
    Ns = [x[0] for x in ops.cloud_normals_batch(As, radius=3 * h)]
    rng = np.random.default_rng(0)
    g0 = torch.empty(P, 3, 4, dtype=torch.float64)
    for p in range(P):
        shift = rng.standard_normal(3)
        g0[p, :, :3], g0[p, :, 3] = torch.from_numpy(rodrigues(rng.standard_normal(3), 0.2)), torch.from_numpy(0.3 * h * shift / np.linalg.norm(shift))
    Bs = [((torch.rand(n, 3, generator=gen) - 0.5) * scale).to(dev) for _ in range(P)]
    return torch.cat(As), torch.cat(Ns), torch.cat(Bs), g0.float().to(dev).contiguous(), np.full(P, 2 * h, np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=64)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--res", type=int, default=64)
    ap.add_argument("--mesh-res", type=int, default=48)
    ap.add_argument("--points", type=int, default=60000)
    ap.add_argument("--min-obs", type=int, default=1)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--deg", type=float, default=1.0, help="the start's rotation off the true pose, about the cloud's centre")
    ap.add_argument("--shift", type=float, default=1.0, help="the start's translation off the true pose, in voxels (trunc is 4)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    P, V, res, n = a.instances, a.views, a.res, a.points
    parts = synth.make_partial_views(range(P), V, res=a.mesh_res, with_depth=True, device=dev)
    clouds = [torch.cat(p["clouds"]) for p in parts]
    grids = More_Solver._fusion_grids(clouds, res, 4)
    S, N = ops.tsdf_state(P, (res,) * 3, dev)
    ops.depth_fuse_batch((S, N), [p["depth"] for p in parts], [p["intrinsics"] for p in parts], [p["world_to_cam"] for p in parts],
                         origin=grids["origin"], voxel=grids["voxel"], trunc=grids["trunc"])
    o, h, tr = (np.ascontiguousarray(grids[k].numpy(), np.float64) for k in ("origin", "voxel", "trunc"))
    gen = torch.Generator().manual_seed(0)
    rng = np.random.default_rng(0)
    Bs, g0 = [], torch.empty(P, 3, 4, dtype=torch.float64)
    for p in range(P):
        rows = clouds[p][torch.randint(0, clouds[p].shape[0], (n,), generator=gen).to(dev)].double().cpu()
        q, _ = torch.linalg.qr(torch.randn(3, 3, generator=gen, dtype=torch.float64))
        q = q * torch.sign(torch.linalg.det(q))
        t = torch.rand(3, generator=gen, dtype=torch.float64) - 0.5
        Bs.append(((rows - t) @ q).float().to(dev).contiguous())           # (q | t) takes it back into the memory's frame
        c = rows.mean(0)
        dR = torch.from_numpy(rodrigues(rng.standard_normal(3), a.deg))
        shift = rng.standard_normal(3)
        g0[p, :, :3], g0[p, :, 3] = dR @ q, dR @ (t - c) + c + torch.from_numpy(a.shift * h[p] * shift / np.linalg.norm(shift))
    g0 = g0.float().to(dev).contiguous()
    B, bo = torch.cat(Bs), ops._offsets([n] * P)
    b = B.shape[0]
    phi, grad, state = torch.empty(b, dtype=torch.float64, device=dev), torch.empty(b, 3, dtype=torch.float64, device=dev), torch.empty(b, dtype=torch.uint8, device=dev)
    counts, sums = torch.empty(P, 3, dtype=torch.int64, device=dev), torch.empty(P, dtype=torch.float64, device=dev)
    g_out = torch.empty(P, 3, 4, device=dev)
    stop, iters = torch.empty(P, dtype=torch.int32, device=dev), torch.empty(P, dtype=torch.int32, device=dev)
    lib = _lib.load()
    ws = torch.empty(lib.ls_tsdf_icp_batch_workspace_bytes(P, res, res, res, b), dtype=torch.uint8, device=dev)
    assert ws.numel() >= lib.ls_tsdf_sample_batch_workspace_bytes(P, res, res, res, b)
    st = _lib.stream_ptr(dev)
    head = (P, _lib.ptr(S), _lib.ptr(N), res, res, res, a.min_obs, ops._hptr(o), ops._hptr(h), ops._hptr(tr), _lib.ptr(B), b, ops._hptr(bo), _lib.ptr(g0))
    outs = (_lib.ptr(phi), _lib.ptr(grad), _lib.ptr(state), _lib.ptr(counts), _lib.ptr(sums))

    def sample():
        _lib.call(dev, "ls_tsdf_sample_batch_f32", *head, *outs, _lib.ptr(ws), ws.numel(), st)

    def icp(max_iter):
        def run():
            _lib.call(dev, "ls_tsdf_icp_batch_f32", *head, max_iter, 0.0, 6, _lib.ptr(g_out), _lib.ptr(stop), _lib.ptr(iters), *outs, None, None,
                      _lib.ptr(ws), ws.numel(), st)
        return run

    od, hd, td = (torch.from_numpy(x).to(dev) for x in (o, h, tr))

    def torch_form():
        return [torch_sample(S[p], N[p], Bs[p], g0[p], od[p], hd[p], td[p], a.min_obs) for p in range(P)]
    # identical states, counts and values before anything is timed
    sample()
    torch.cuda.synchronize()
    ref = torch_form()
    assert torch.equal(torch.cat([r[2] for r in ref]), state), "the two forms disagree on the states"
    assert torch.equal(torch.stack([r[3] for r in ref]), counts), "the two forms disagree on the counts"
    assert torch.equal(torch.cat([r[0] for r in ref]).view(torch.int64), phi.view(torch.int64)), "the two forms disagree on phi"
    assert torch.equal(torch.cat([r[1] for r in ref]).view(torch.int64), grad.view(torch.int64)), "the two forms disagree on the gradient"
    c_sample = counts.cpu().numpy().copy()
    del ref
    # the plane ICP at the same row counts
    A2, N2, B2, g2, rad = plane_workload(P, n, dev, gen)
    ao = ops._offsets([n] * P)
    idx, d2 = torch.empty(P * n, dtype=torch.int32, device=dev), torch.empty(P * n, device=dev)
    c2, s2, status = torch.empty(P, 3, dtype=torch.int64, device=dev), torch.empty(P, dtype=torch.float64, device=dev), torch.empty(P, dtype=torch.int32, device=dev)
    planar, rho2 = torch.empty(P, dtype=torch.int64, device=dev), torch.empty(P, dtype=torch.float64, device=dev)
    it2, stop2, g2_out = torch.empty(P, dtype=torch.int32, device=dev), torch.empty(P, dtype=torch.int32, device=dev), torch.empty(P, 3, 4, device=dev)
    ws2 = torch.empty(lib.ls_cloud_icp_plane_batch_workspace_bytes(P, A2.shape[0], B2.shape[0]), dtype=torch.uint8, device=dev)

    def plane(max_iter):
        def run():
            _lib.call(dev, "ls_cloud_icp_plane_batch_f32", P, _lib.ptr(A2), _lib.ptr(N2), A2.shape[0], ops._hptr(ao), _lib.ptr(B2), B2.shape[0],
                      ops._hptr(ao), _lib.ptr(g2), ops._hptr(rad), max_iter, 0.0, 6, _lib.ptr(g2_out), _lib.ptr(stop2), _lib.ptr(it2), _lib.ptr(idx),
                      _lib.ptr(d2), _lib.ptr(c2), _lib.ptr(s2), _lib.ptr(planar), _lib.ptr(rho2), _lib.ptr(status), None, None, _lib.ptr(ws2),
                      ws2.numel(), st)
        return run

    fns = [sample, icp(1), icp(2), plane(1), plane(2), torch_form]
    (t_s, t_i1, t_i2, t_p1, t_p2, t_t), spread = median_ms(fns, a.reps)
    fns[2]()
    torch.cuda.synchronize()
    it_tsdf, c_icp = iters.cpu().numpy().copy(), counts.cpu().numpy().copy()
    fns[4]()
    torch.cuda.synchronize()
    it_plane = it2.cpu().numpy().copy()
    assert not status.any()
    print(f"instances {P} x {res}^3 samples fused from {V} views each, {n} queries each, min_obs {a.min_obs}; finite {c_sample[:, 0].sum()}, inside "
          f"{c_sample[:, 1].sum()}, sampled {c_sample[:, 2].sum()} of {b}; after two updates sampled {c_icp[:, 2].sum()}")
    names = ("sample", "icp 1", "icp 2", "plane 1", "plane 2", "torch")
    for name, t, (lo, hi) in zip(names, (t_s, t_i1, t_i2, t_p1, t_p2, t_t), spread):
        print(f"{name:8s} {t:9.3f} ms (min {lo:.3f}, max {hi:.3f})")
    must, gather = 45 * b, 64 * b
    print(f"sample: must-move {must / 2 ** 20:.0f} MiB (12 in + 33 out per query) = {must / (t_s * 1e-3) / 1e9:.0f} GB/s, {100 * must / (t_s * 1e-3) / PEAK:.1f} % of "
          f"8.0 TB/s; with 64 bytes of corners per query {(must + gather) / (t_s * 1e-3) / 1e9:.0f} GB/s, {100 * (must + gather) / (t_s * 1e-3) / PEAK:.1f} %; "
          f"torch / sample = {t_t / t_s:.1f}")
    if it_tsdf.min() == 2 and it_plane.min() == 2:
        per, per_p = t_i2 - t_i1, t_p2 - t_p1
        print(f"one iteration with all {P} problems live: tsdf {per:.3f} ms, plane {per_p:.3f} ms, plane / tsdf = {per_p / per:.1f}; the tsdf iteration "
              f"moves at least {must / 2 ** 20:.0f} MiB = {100 * must / (per * 1e-3) / PEAK:.1f} % of 8.0 TB/s")
    else:
        print(f"some problems stopped before 2 iterations (tsdf: {int((it_tsdf < 2).sum())} of {P}, plane: {int((it_plane < 2).sum())} of {P}): no "
              f"per-iteration figure from this run")


if __name__ == "__main__":
    main()
