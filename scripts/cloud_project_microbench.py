"""Scene-memory projection onto local planes (csrc/cloudnear.hip: ls_cloud_project_batch_f32) against the operator that does the same walk,
ls_cloud_normals_batch_f32, and what a consolidation (More_Solver._consolidate_batch) does to noisy memories.

    python scripts/cloud_project_microbench.py [--instances 64] [--points 60000] [--voxel 0.01] [--reps 20] [--shape-points 20000]
                                               [--rescans 5] [--sigma 0.002] [--dense 100000] [--max-variation 0.05]

Time.  Device events after warm-up, median of `reps`, the two forms alternating in one process, on pre-packed inputs (the library calls
alone: no torch.cat, no host read).  The slab of scripts/cloud_icp_microbench.py -- P x `points` memory rows at one per voxel -- at radius
2 * voxel:
  normals  ONE ls_cloud_normals_batch_f32 call (grid build, one thread per memory row, the counts)
  project  ONE ls_cloud_project_batch_f32 call (the same grid build and walk, the float64 projection, 20 more output bytes per row, one
           float64 partial per chunk of 256 rows, the counts and sums)
Quality.  P memories: a reference scan and `rescans` more draws of the same shape, every scan with Gaussian noise sigma, merged at the
true pose at `voxel`.  Reported before and after More_Solver._consolidate_batch at its default radius (3 * voxel): the rows, the mean
distance of the kept rows to their nearest row of a dense noise-free sample of the same shape (ops.cloud_nearest_batch; bounded below by
the sample's own spacing, which it mostly shows), and the mean ANALYTIC distance to the shape.  Two families of shapes:
  solid   synth.canonical_shape as it is: it FILLS its boxes, so the memory is a solid with no surface to project onto; the analytic
          distance is that to the union of the boxes, 0 inside
  faces   the faces of the same boxes, sampled by area: surfaces with edges; the analytic distance is that to the nearest face
Four runs each: consolidated ONCE after the last rescan and after EVERY rescan, without a limit and with --max-variation (an
illustration, NOT a recommendation)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from livingscenes_amd import _lib, ops, synth  # noqa: E402
from livingscenes_amd.lib_more.more_solver import More_Solver  # noqa: E402
from cloud_nearest_microbench import median_ms  # noqa: E402
from cloud_plane_icp_microbench import slab  # noqa: E402


class Calls:
    """the two library calls on one packed workload, with their output buffers"""

    def __init__(self, As, r, dev):
        self.dev, self.P = dev, len(As)
        P = self.P
        self.A = torch.cat(As)
        self.ao = ops._offsets([x.shape[0] for x in As])
        self.rad = np.full(P, r, np.float32)
        a = self.A.shape[0]
        self.N, self.cnt, self.var = torch.empty(a, 3, device=dev), torch.empty(a, dtype=torch.int32, device=dev), torch.empty(a, device=dev)
        self.ncounts = torch.empty(P, 2, dtype=torch.int64, device=dev)
        self.out, self.state, self.shift = torch.empty(a, 3, device=dev), torch.empty(a, dtype=torch.int32, device=dev), torch.empty(a, device=dev)
        self.pcounts, self.sums = torch.empty(P, 4, dtype=torch.int64, device=dev), torch.empty(P, dtype=torch.float64, device=dev)
        self.status = torch.empty(P, dtype=torch.int32, device=dev)
        lib = _lib.load()
        self.ws = torch.empty(max(lib.ls_cloud_project_batch_workspace_bytes(P, a), lib.ls_cloud_normals_batch_workspace_bytes(P, a)),
                              dtype=torch.uint8, device=dev)
        self.st = _lib.stream_ptr(dev)

    def normals(self):
        _lib.call(self.dev, "ls_cloud_normals_batch_f32", self.P, _lib.ptr(self.A), self.A.shape[0], ops._hptr(self.ao), ops._hptr(self.rad), 5,
                  _lib.ptr(self.N), _lib.ptr(self.cnt), _lib.ptr(self.var), _lib.ptr(self.ncounts), _lib.ptr(self.status), _lib.ptr(self.ws),
                  self.ws.numel(), self.st)

    def project(self):
        _lib.call(self.dev, "ls_cloud_project_batch_f32", self.P, _lib.ptr(self.A), self.A.shape[0], ops._hptr(self.ao), ops._hptr(self.rad), 5,
                  1 / 3, float("inf"), _lib.ptr(self.out), _lib.ptr(self.state), _lib.ptr(self.shift), _lib.ptr(self.pcounts), _lib.ptr(self.sums),
                  _lib.ptr(self.status), _lib.ptr(self.ws), self.ws.numel(), self.st)


def box_distance(x, boxes):
    """[n,3] -> the distance of every row to the union of the boxes ((x0, x1), (y0, y1), (z0, z1)), 0 inside (float64, on x's device)"""
    b = torch.tensor(boxes, dtype=torch.float64, device=x.device)        # [nb,3,2]
    x = x.double()[:, None, :]
    gap = torch.clamp(torch.maximum(b[None, :, :, 0] - x, x - b[None, :, :, 1]), min=0.0)
    return torch.linalg.norm(gap, dim=2).min(1).values


def face_distance(x, boxes):
    """[n,3] -> the distance of every row to the nearest face of a box: outside a box the distance to it, inside its depth"""
    b = torch.tensor(boxes, dtype=torch.float64, device=x.device)
    x = x.double()[:, None, :]
    gap = torch.clamp(torch.maximum(b[None, :, :, 0] - x, x - b[None, :, :, 1]), min=0.0)
    out = torch.linalg.norm(gap, dim=2)
    depth = torch.minimum(x - b[None, :, :, 0], b[None, :, :, 1] - x).min(2).values
    return torch.where(out > 0, out, depth).min(1).values


def face_sample(boxes, n, rng):
    """n points on the faces of the boxes, a face chosen by its area -> [n,3] float64"""
    b = np.asarray(boxes, np.float64)                                    # [nb,3,2]
    e = b[:, :, 1] - b[:, :, 0]
    area = np.stack([e[:, 1] * e[:, 2], e[:, 0] * e[:, 2], e[:, 0] * e[:, 1]], 1)          # [nb,3]: the pair of faces normal to the axis
    pick = rng.choice(area.size, n, p=(area / area.sum()).ravel())
    box, axis = pick // 3, pick % 3
    pts = b[box, :, 0] + rng.random((n, 3)) * e[box]
    pts[np.arange(n), axis] = b[box, axis, (rng.random(n) < 0.5).astype(int)]
    return pts


def figures(mems, dense, boxes, r, distance):
    """-> (rows, mean distance to the nearest dense row, share of rows with one within r, mean analytic distance)"""
    res = ops.cloud_nearest_batch(dense, mems, radius=r)
    d = torch.cat([x[1] for x in res])
    has = torch.isfinite(d)
    exact = torch.cat([distance(m, bx) for m, bx in zip(mems, boxes)])
    return sum(m.shape[0] for m in mems), float(d[has].double().sqrt().mean()), float(has.double().mean()), float(exact.mean())


def quality(name, what, solver, scans, clean, dense, boxes, h, distance, limit):
    """the four runs on one family of memories: scans[k][p] the noisy scans, clean[p] a noise-free one, dense[p] the dense sample"""
    fig = lambda mems: figures(mems, dense, boxes, 5 * h, distance)
    floor = fig([x for x, _ in ops.cloud_merge_batch(clean, [c[:0] for c in clean], voxel=h)])
    print(f"{name}: a NOISE-FREE scan merged at {h}: rows {floor[0]}, mean distance to the dense sample {floor[1]:.3e} (the floor of that "
          f"figure: the sample's own spacing), {what} {floor[3]:.3e}")
    for every in (False, True):
        for lim in (1 / 3, limit):
            mem = solver._accumulate_batch(scans[0], [c[:0] for c in scans[0]], None)
            trace = []
            for k in range(1, len(scans)):
                mem = solver._accumulate_batch(mem, scans[k], None)
                if every:
                    mem, info = solver._consolidate_batch(mem, max_variation=lim)
                    trace.append(fig(mem))
            before = fig(mem)
            if not every:
                mem, info = solver._consolidate_batch(mem, max_variation=lim)
            after = fig(mem)
            run = f"{name}, {'after EVERY rescan' if every else 'ONCE after the last'}, max_variation {'none' if lim >= 1 / 3 else lim}"
            if every:
                steps = "; ".join(f"{t[0]} rows {t[1]:.3e} / {t[3]:.3e}" for t in trace)
                print(f"{run}: per step (rows, mean distance to the dense sample / {what}) {steps}")
            else:
                print(f"{run}: before {before[0]} rows, dense {before[1]:.3e} (matched {before[2]:.4f}), {what} {before[3]:.3e}; after {after[0]} "
                      f"rows, dense {after[1]:.3e} (matched {after[2]:.4f}), {what} {after[3]:.3e}")
            print(f"    last consolidation: moved {sum(info['moved'])}, held {sum(info['held'])}, no plane {sum(info['no_plane'])}, mean rms shift "
                  f"{float(np.nanmean(info['rms_shift'])):.3e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=64)
    ap.add_argument("--points", type=int, default=60000)
    ap.add_argument("--voxel", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shape-points", type=int, default=20000)
    ap.add_argument("--rescans", type=int, default=5)
    ap.add_argument("--sigma", type=float, default=0.002)
    ap.add_argument("--dense", type=int, default=100000)
    ap.add_argument("--max-variation", type=float, default=0.05)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    P, n, h = a.instances, a.points, a.voxel

    As, _, _ = slab(P, n, h, dev)
    w = Calls(As, 2 * h, dev)
    (t_n, t_p), spread = median_ms([w.normals, w.project], a.reps)
    torch.cuda.synchronize()
    assert not w.status.any()
    pc, nc = w.pcounts.cpu().numpy(), w.ncounts.cpu().numpy()
    assert (pc[:, 1:].sum(1) == nc[:, 0]).all() and (pc[:, 2] + pc[:, 3] == nc[:, 1]).all()      # the same neighbourhoods, the same validity
    print(f"slab: instances {P} x {n} memory rows, voxel {h}, radius {2 * h}; workspace {w.ws.numel() / 2 ** 20:.0f} MiB")
    print(f"normals  {t_n:9.3f} ms (min {spread[0][0]:.3f}, max {spread[0][1]:.3f}); valid rows {nc[:, 1].sum()} of {nc[:, 0].sum()}")
    print(f"project  {t_p:9.3f} ms (min {spread[1][0]:.3f}, max {spread[1][1]:.3f}); moved rows {pc[:, 3].sum()}; project / normals = {t_p / t_n:.2f}")
    del w, As

    m = a.shape_points
    rng = np.random.default_rng(2)
    solver = More_Solver({"accumulate": {"voxel_size": h}}, model=object())
    boxes = [synth._chair_boxes(synth._rng(p, "shape")) for p in range(P)]
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)
    noisy = lambda x: x + rng.normal(0, a.sigma, x.shape)
    print(f"quality: instances {P} x ({m} points per scan, 1 + {a.rescans} scans, sigma {a.sigma}), voxel {h}, consolidation radius {3 * h}; "
          f"dense sample {a.dense} rows per shape")
    # synth.canonical_shape as it is: it FILLS its boxes, so the memory is a solid and has no surface to project onto
    scans = [[up(noisy(synth.canonical_shape(m + k, p))) for p in range(P)] for k in range(a.rescans + 1)]
    quality("solid", "to the boxes", solver, scans, [up(synth.canonical_shape(m, p)) for p in range(P)],
            [up(synth.canonical_shape(a.dense, p)) for p in range(P)], boxes, h, box_distance, a.max_variation)
    del scans
    # the faces of the same boxes: surfaces with edges
    scans = [[up(noisy(face_sample(boxes[p], m, rng))) for p in range(P)] for k in range(a.rescans + 1)]
    quality("faces", "to the faces", solver, scans, [up(face_sample(boxes[p], m, rng)) for p in range(P)],
            [up(face_sample(boxes[p], a.dense, rng)) for p in range(P)], boxes, h, face_distance, a.max_variation)

if __name__ == "__main__":
    main()
