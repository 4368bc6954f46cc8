"""Mesh metrics on the device (csrc/meshmetrics.hip) vs the host path, at (faces, points) = (5k, 20k), (100k, 100k), (100k, 1M).

    python scripts/meshmetrics_microbench.py [--no-host]

Device: wall time per call of each operator (ops.mesh_contains / mesh_distance at max_dist 0.05 / mesh_sample) and of the three metrics of
evaluate.py, after warm-up, including the host read of the bin entry count the binned ops make.  Host: numpy / scipy at 16 threads -- the
hash-binned parity count of tests/meshmetrics_oracle.py (the reference's algorithm, vectorised), its brute-force Ericson distance (the
smallest config only: O(points x faces)), the numpy sampler, and scipy cKDTree (workers=16) for the Chamfer distance.
Meshes: marching cubes of a smooth random field in the unit cube, sized to the face counts above."""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
os.environ.setdefault("OMP_NUM_THREADS", "16")
import numpy as np  # noqa: E402
import torch  # noqa: E402

import meshmetrics_oracle as mo  # noqa: E402
from livingscenes_amd import evaluate, ops  # noqa: E402
from livingscenes_amd.mesh_extractor2 import marching_cubes  # noqa: E402

dev = torch.device("cuda:0")
torch.set_num_threads(16)


class Mesh:
    def __init__(self, V, F):
        self.vertices, self.faces = V, F


def field_mesh(n, seed=0):
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(*[np.linspace(0, 1, n)] * 3, indexing="ij"), -1)
    c, w = rng.uniform(0.25, 0.75, (10, 3)), rng.uniform(0.1, 0.2, 10)
    f = 0.5 - sum(np.exp(-((g - ci) ** 2).sum(-1) / (2 * wi * wi)) for ci, wi in zip(c, w))
    v, faces = marching_cubes(torch.from_numpy(f).to(dev), 0.0)
    return (v.cpu().numpy() - 0.5) / (n - 1), faces.cpu().numpy()


def mesh_with_faces(target):
    n = 16
    while True:
        V, F = field_mesh(n)
        if len(F) >= target:
            return V, F[:target] if len(F) < 1.5 * target else F
        n = int(n * max(1.1, (target / max(len(F), 1)) ** 0.5))


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps * 1e3


def host_timed(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def main():
    host = "--no-host" not in sys.argv
    rng = np.random.default_rng(1)
    print(f"{'faces':>7} {'points':>8} | {'contains':>9} {'distance':>9} {'sample30k':>9} | {'chamfer':>8} {'sdf_rec':>8} {'v_iou':>8}  (ms, device)")
    rows = []
    for nf_target, n in ((5000, 20000), (100000, 100000), (100000, 1000000)):
        V, F = mesh_with_faces(nf_target)
        P = rng.uniform(-0.05, 1.05, (n, 3))
        Vd, Fd = torch.from_numpy(V).to(dev), torch.from_numpy(F.astype(np.int32)).to(dev)
        Pd = torch.from_numpy(P).to(dev)
        reps = 10 if n <= 100000 else 3
        t_in = timed(lambda: ops.mesh_contains(Vd, Fd, Pd), reps)
        t_d = timed(lambda: ops.mesh_distance(Vd, Fd, Pd, 0.05), reps)
        t_s = timed(lambda: ops.mesh_sample(Vd, Fd, 30000, 0), reps)
        gt, m, q = Mesh(P, np.zeros((0, 3), np.int64)), Mesh(V, F), Mesh(P, F)
        t_cd = timed(lambda: evaluate.compute_chamfer_distance(gt, m, 0, 1), reps)
        t_sr = timed(lambda: evaluate.compute_sdf_recall(m, q, 0.05), reps)
        t_iou = timed(lambda: evaluate.compute_volumetric_iou(m, q), reps)
        print(f"{len(F):>7} {n:>8} | {t_in:9.2f} {t_d:9.2f} {t_s:9.2f} | {t_cd:8.2f} {t_sr:8.2f} {t_iou:8.2f}", flush=True)
        rows.append((V, F, P))
    if not host:
        return
    from scipy.spatial import cKDTree
    print(f"{'faces':>7} {'points':>8} | {'contains':>9} {'distance':>9} {'sample30k':>9} | {'chamfer':>8}  (ms, host numpy/scipy, 16 threads)")
    for V, F, P in rows:
        h_in = host_timed(lambda: mo.contains(V, F, P))
        h_d = host_timed(lambda: mo.distance(V, F, P, 0.05)) if len(F) * len(P) <= 2e8 else float("nan")
        samples = []
        h_s = host_timed(lambda: samples.append(mo.sample(V, F, 30000, 0)[0]))
        h_cd = host_timed(lambda: (cKDTree(samples[0]).query(P, workers=16), cKDTree(P).query(samples[0], workers=16)))
        print(f"{len(F):>7} {len(P):>8} | {h_in:9.1f} {h_d:9.1f} {h_s:9.1f} | {h_cd:8.1f}", flush=True)


if __name__ == "__main__":
    main()
