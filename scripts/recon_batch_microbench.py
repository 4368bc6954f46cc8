"""Batched reconstruction leg vs the per-object one (docs/history.md 18).

    python scripts/recon_batch_microbench.py [--objects 32] [--json out.json]

1. Mesh metrics: M single-mesh calls (ops.mesh_contains / mesh_distance at max_dist 0.05 / mesh_sample) against ONE ragged call
   (ops.mesh_*_batch) for M in {1, 8, 32, 128} meshes of about 5 k faces with 20 k query points (20 k samples) each; wall time per
   call after warm-up, including the host read of the bin entry count the binned ops make.
2. A synthetic scene of --objects instances (untrained decoder at the released extraction settings: resolution0 32, two up-sampling steps,
   simplify_nfaces 5000, iso-level = median logit) through the per-object leg (eval_grid, marching cubes, serial decimation, the three
   per-mesh metrics) and the batched leg (eval_grid_batch and _mc_arrays_batch in groups of 16, simplify_mesh_arrays_batch on
   mesh_extractor2.default_threads() host threads, the *_batch metrics), stage by stage.
3. The same scene through the batched leg twice in one run, decimated by the host edge collapse (simplify_method "collapse", the thread pool)
   and by the device vertex clustering ("cluster", docs/history.md 26): ms per scene and stage, faces per mesh, and Chamfer / SDF recall /
   V-IoU of both against the same ground truth (synthetic weights and analytic shapes: a comparison of the two decimators, not a result)."""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from livingscenes_amd import evaluate, ops, synth  # noqa: E402
from livingscenes_amd import mesh_extractor2 as me  # noqa: E402
from livingscenes_amd.model_utils import Shape_Prior  # noqa: E402

dev = torch.device("cuda:0")


def sync_time():
    torch.cuda.synchronize()
    return time.perf_counter()


def timed(fn, reps):
    fn()
    t = sync_time()
    for _ in range(reps):
        fn()
    return (sync_time() - t) / reps * 1e3


def field_mesh(n, seed):
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(*[np.linspace(0, 1, n)] * 3, indexing="ij"), -1)
    c, w = rng.uniform(0.25, 0.75, (10, 3)), rng.uniform(0.1, 0.2, 10)
    f = 0.5 - sum(np.exp(-((g - ci) ** 2).sum(-1) / (2 * wi * wi)) for ci, wi in zip(c, w))
    v, faces = me.marching_cubes(torch.from_numpy(f).to(dev), 0.0)
    return ((v - 0.5) / (n - 1)).contiguous(), faces.to(torch.int32).contiguous()


def ops_bench(out):
    base = [field_mesh(30, s) for s in range(8)]        # ~5 k faces each
    rng = np.random.default_rng(0)
    res = []
    for M in (1, 8, 32, 128):
        meshes = [(base[k % 8][0] + float(k // 8), base[k % 8][1]) for k in range(M)]
        pts = [torch.from_numpy(rng.uniform(0, 1, (20000, 3)) + k // 8).to(dev) for k in range(M)]
        reps = max(2, 64 // M)
        row = {"M": M, "faces_mean": float(np.mean([F.shape[0] for _, F in meshes]))}
        row["contains_single_ms"] = timed(lambda: [ops.mesh_contains(V, F, P) for (V, F), P in zip(meshes, pts)], reps)
        row["contains_batch_ms"] = timed(lambda: ops.mesh_contains_batch(meshes, pts), reps)
        row["distance_single_ms"] = timed(lambda: [ops.mesh_distance(V, F, P, 0.05) for (V, F), P in zip(meshes, pts)], reps)
        row["distance_batch_ms"] = timed(lambda: ops.mesh_distance_batch(meshes, pts, 0.05), reps)
        row["sample_single_ms"] = timed(lambda: [ops.mesh_sample(V, F, 20000, k) for k, (V, F) in enumerate(meshes)], reps)
        row["sample_batch_ms"] = timed(lambda: ops.mesh_sample_batch(meshes, 20000, list(range(M))), reps)
        print(" ".join(f"{k}={v:.3f}" if isinstance(v, float) else f"{k}={v}" for k, v in row.items()), flush=True)
        res.append(row)
    out["ops"] = res


def scene_setup(n_obj):
    ecfg, dcfg = synth.default_encoder_cfg(), synth.default_decoder_cfg()
    sp = Shape_Prior.from_state(ecfg, dcfg, synth.make_encoder_weights(ecfg, 0), synth.make_decoder_weights(dcfg, 0), device=dev)
    with torch.no_grad():
        emb = sp.encode(synth.make_instances(n_obj, 1024, seed=0).to(dev))
    canon = {k: emb[k].detach() for k in ("z_so3", "z_inv")}
    canon["t"], canon["s"] = torch.zeros_like(emb["t"]), torch.ones_like(emb["s"])
    gen = me.Generator3D(threshold=0.5, resolution0=32, upsampling_steps=2, padding=0.1, points_batch_size=400000, simplify_nfaces=5000)
    level = float(np.median(gen.eval_grid({k: v[:1] for k, v in canon.items()}, sp.decoder)))
    gen.threshold = 1.0 / (1.0 + np.exp(-level))
    gts = [synth.canonical_mesh(1000 + i, res=64) for i in range(n_obj)]
    return sp, canon, gen, gts


def scene_bench(out, n_obj):
    sp, canon, gen, gts = scene_setup(n_obj)
    row = lambda i: {k: v[i:i + 1] for k, v in canon.items()}
    # warm-up of both legs on two objects
    gen._mc_arrays_batch(gen.eval_grid_batch({k: v[:2] for k, v in canon.items()}, sp.decoder, on_device=True))
    gen._mc_arrays(gen.eval_grid(row(0), sp.decoder, on_device=True))

    per = {"mise": 0.0, "marching_cubes": 0.0, "decimation": 0.0, "metrics": 0.0}
    faces_mc, faces_out = [], []
    for i in range(n_obj):
        t0 = sync_time()
        g = gen.eval_grid(row(i), sp.decoder, on_device=True)
        t1 = sync_time()
        v, f = gen._mc_arrays(g)
        t2 = sync_time()
        faces_mc.append(len(f))
        if len(v):
            v, f = me.simplify_mesh_arrays(v, f, 5000, 5.0)
        t3 = time.perf_counter()
        m = me.make_mesh(v, f)
        faces_out.append(len(f))
        if len(v):
            evaluate.compute_chamfer_distance(gts[i], m, offset=0, scale=1)
            evaluate.compute_sdf_recall(m, gts[i], 0.05)
            evaluate.compute_volumetric_iou(m, gts[i])
        t4 = sync_time()
        for k, dt in zip(per, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
            per[k] += dt * 1e3

    bat = {}
    t0 = sync_time()
    grids = []
    for g0 in range(0, n_obj, 16):
        grids += gen.eval_grid_batch({k: v[g0:g0 + 16] for k, v in canon.items()}, sp.decoder, on_device=True)
    t1 = sync_time()
    arrays = []
    for g0 in range(0, n_obj, 16):
        arrays += gen._mc_arrays_batch(grids[g0:g0 + 16])
    t2 = sync_time()
    live = [i for i, (v, _) in enumerate(arrays) if len(v)]
    for i, vf in zip(live, me.simplify_mesh_arrays_batch([arrays[i] for i in live], 5000, 5.0)):
        arrays[i] = vf
    t3 = time.perf_counter()
    meshes = [me.make_mesh(v, f) for v, f in arrays]
    P, G = [meshes[i] for i in live], [gts[i] for i in live]
    evaluate.compute_chamfer_distance_batch(G, P, offset=0, scale=1)
    evaluate.compute_sdf_recall_batch(P, G, 0.05)
    evaluate.compute_volumetric_iou_batch(P, G)
    t4 = sync_time()
    for k, dt in zip(per, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
        bat[k] = dt * 1e3
    per["total"], bat["total"] = sum(per.values()), sum(bat.values())
    out["scene"] = {"objects": n_obj, "host_threads": me.default_threads(), "faces_mc_mean": float(np.mean(faces_mc)),
                    "faces_out_mean": float(np.mean(faces_out)), "gt_vertices_mean": float(np.mean([len(g.vertices) for g in gts])),
                    "per_object_ms": per, "batched_ms": bat}
    print(json.dumps(out["scene"]), flush=True)


def cluster_bench(out, n_obj):
    """the batched leg with both decimators, stage by stage (groups of 16 instances, as the harness runs it)"""
    sp, canon, gen, gts = scene_setup(n_obj)
    logit = np.log(gen.threshold) - np.log(1.0 - gen.threshold)
    groups = [{k: v[g0:g0 + 16] for k, v in canon.items()} for g0 in range(0, n_obj, 16)]
    res = {"objects": n_obj, "host_threads": me.default_threads()}
    for method in ("collapse", "cluster", "collapse", "cluster"):      # the first pass of each warms up
        t = {"mise": 0.0, "marching_cubes": 0.0, "decimation": 0.0, "to_host": 0.0}
        arrays, faces_mc = [], []
        for codes in groups:
            t0 = sync_time()
            grids = gen._eval_grid_batch_device(codes, sp.decoder)
            t1 = sync_time()
            vol = torch.nn.functional.pad(grids.to(torch.float64), (1, 1, 1, 1, 1, 1), value=-1e6)
            verts, faces, vo, fo = me._marching_cubes_packed(vol, logit)
            t2 = sync_time()
            faces_mc += np.diff(fo).tolist()
            if method == "cluster":
                verts, faces, vo, fo, _ = me._cluster_packed(verts, vo, faces, fo, 5000, 256)
            t3 = sync_time()
            hv, hf = gen._normalise_vertices(verts.cpu().numpy(), grids[0].shape), faces.cpu().numpy()
            part = [(hv[vo[b]:vo[b + 1]], hf[fo[b]:fo[b + 1]]) for b in range(len(vo) - 1)]
            t4 = sync_time()
            if method == "collapse":
                live = [i for i, (v, _) in enumerate(part) if len(v)]
                for i, vf in zip(live, me.simplify_mesh_arrays_batch([part[i] for i in live], 5000, 5.0)):
                    part[i] = vf
            t5 = time.perf_counter()
            arrays += part
            for k, dt in zip(t, (t1 - t0, t2 - t1, (t3 - t2) + (t5 - t4), t4 - t3)):
                t[k] += dt * 1e3
        meshes = [me.make_mesh(v, f) for v, f in arrays]
        live = [i for i, (v, _) in enumerate(arrays) if len(v)]
        P, G = [meshes[i] for i in live], [gts[i] for i in live]
        t0 = sync_time()
        cd = evaluate.compute_chamfer_distance_batch(G, P, offset=0, scale=1)
        rec = evaluate.compute_sdf_recall_batch(P, G, 0.05)
        iou = evaluate.compute_volumetric_iou_batch(P, G)
        t["metrics"] = (sync_time() - t0) * 1e3
        t["total"] = sum(t.values())
        nf = [len(f) for _, f in arrays]
        res[method] = {"ms": t, "faces_mc_mean": float(np.mean(faces_mc)), "faces_out_mean": float(np.mean(nf)), "faces_out_min": int(min(nf)),
                       "faces_out_max": int(max(nf)), "chamfer_mean": np.mean(np.asarray(cd, np.float64), 0).tolist(),
                       "sdf_recall_mean": float(np.mean(rec)), "viou_mean": float(np.mean(iou))}
    out["cluster_scene"] = res
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=32)
    ap.add_argument("--skip-ops", action="store_true")
    ap.add_argument("--skip-scene", action="store_true")
    ap.add_argument("--skip-cluster", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "cpus_available": len(os.sched_getaffinity(0)),
           "OMP_NUM_THREADS": os.environ.get("OMP_NUM_THREADS")}
    print(json.dumps(out), flush=True)
    if not a.skip_ops:
        ops_bench(out)
    if not a.skip_scene:
        scene_bench(out, a.objects)
    if not a.skip_cluster:
        cluster_bench(out, a.objects)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
