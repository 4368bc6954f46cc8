"""GPU tests of the ragged multi-mesh metrics (csrc/meshmetrics.hip: ls_mesh_contains_batch_f64 / ls_mesh_distance_batch_f64 /
ls_mesh_sample_batch_f64; ops.mesh_*_batch; evaluate's *_batch functions) and of the batched reconstruction leg built on them
(More_Solver._mesh_from_latent_batch, harness.eval_reconstruction / eval_3rscan_reconstruction with batched=True).  The bar everywhere is
bit-identity with the single-mesh path, mesh by mesh."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


class Mesh:
    def __init__(self, V, F):
        self.vertices, self.faces = np.asarray(V, np.float64), np.asarray(F, np.int64)


def _base_meshes():
    """ragged content: marching-cubes meshes of several resolutions, a flat mesh, an empty mesh"""
    from livingscenes_amd import synth
    out = [synth.canonical_mesh(11 + i, res=r) for i, r in enumerate((16, 24, 36))]
    out.append(Mesh([[0, 0, 0.3], [1, 0, 0.3], [1, 1, 0.3], [0, 1, 0.3]], [[0, 1, 2], [0, 2, 3]]))   # flat: zero extent in z
    out.append(Mesh(np.zeros((0, 3)), np.zeros((0, 3))))                                            # empty
    return out


def _case(M, seed=0):
    """M meshes (cycled, shifted) as device (V, F int32) pairs and M point sets: random points around each mesh, points far outside every
    mesh, one mesh with no query points"""
    rng = np.random.default_rng(seed)
    base = _base_meshes()
    meshes, pts = [], []
    for k in range(M):
        b = base[k % len(base)]
        shift = rng.uniform(-1, 1, 3) * (k // len(base))
        V = b.vertices + shift
        meshes.append((torch.as_tensor(V).to(_dev()), torch.as_tensor(b.faces.astype(np.int32)).to(_dev())))
        lo, hi = (V.min(0), V.max(0)) if len(V) else (shift - 0.5, shift + 0.5)
        pad = 0.2 * (hi - lo) + 0.05
        n = 0 if k == 2 else int(rng.integers(200, 2500))
        P = rng.uniform(lo - pad, hi + pad, (n, 3))
        if n:
            P[: n // 10] += [100.0, -50.0, 30.0]                     # far outside every mesh
        pts.append(torch.as_tensor(P).to(_dev()))
    return meshes, pts


def _assert_outputs_equal(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, i
        assert torch.equal(g.cpu(), w.cpu()), (i, int((g.cpu() != w.cpu()).sum()))


def _single_contains(meshes, pts, R):
    from livingscenes_amd import ops
    return [ops.mesh_contains(V, F, P, R) for (V, F), P in zip(meshes, pts)]


def _single_distance(meshes, pts, md):
    from livingscenes_amd import ops
    return [ops.mesh_distance(V, F, P, md) for (V, F), P in zip(meshes, pts)]


def _counts_seeds(meshes, rng):
    counts = [0 if F.shape[0] == 0 else int(rng.choice([0, 1, 777, 5000])) for _, F in meshes]
    seeds = [int(s) for s in rng.integers(0, 2 ** 63, len(meshes))]
    return counts, seeds


def _single_sample(meshes, counts, seeds):
    from livingscenes_amd import ops
    out = []
    for (V, F), c, s in zip(meshes, counts, seeds):
        if c == 0:
            out.append((torch.zeros(0, 3, dtype=torch.float64, device=_dev()), torch.zeros(0, dtype=torch.int64, device=_dev())))
        else:
            out.append(ops.mesh_sample(V, F, c, s))
    return out


# ------------------------------------------------------------------------------------------------ 1. batch ops == single-mesh ops
@pytest.mark.parametrize("M", [1, 5, 40])
def test_batch_ops_equal_single_ops(M):
    from livingscenes_amd import ops
    meshes, pts = _case(M, seed=M)
    for R in (64, 512):
        _assert_outputs_equal(ops.mesh_contains_batch(meshes, pts, R), _single_contains(meshes, pts, R))
    for md in (0.02, 0.3):
        _assert_outputs_equal(ops.mesh_distance_batch(meshes, pts, md), _single_distance(meshes, pts, md))
    counts, seeds = _counts_seeds(meshes, np.random.default_rng(M))
    got, want = ops.mesh_sample_batch(meshes, counts, seeds), _single_sample(meshes, counts, seeds)
    _assert_outputs_equal([p for p, _ in got], [p for p, _ in want])
    _assert_outputs_equal([f for _, f in got], [f for _, f in want])
    # seeds=None: seed 0 everywhere; one count for every mesh
    live = [m for m in meshes if m[1].shape[0]]
    got = ops.mesh_sample_batch(live, 300)
    _assert_outputs_equal([p for p, _ in got], [ops.mesh_sample(V, F, 300, 0)[0] for V, F in live])


def test_batch_ops_results_make_sense():
    """not only equal to the single op: volume samples of a watertight shape are inside it and near its surface, far points are outside
    and +inf, a flat mesh contains nothing, an empty mesh contains nothing and is infinitely far away"""
    from livingscenes_amd import ops, synth
    seed = 3 * 100003
    m = synth.canonical_mesh(seed, res=32)
    solid = np.asarray(synth.canonical_shape(3000, seed), np.float64)
    V, F = torch.as_tensor(m.vertices).to(_dev()), torch.as_tensor(m.faces.astype(np.int32)).to(_dev())
    flat = (torch.tensor([[0, 0, 0.3], [1, 0, 0.3], [1, 1, 0.3], [0, 1, 0.3]], dtype=torch.float64, device=_dev()),
            torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int32, device=_dev()))
    empty = (torch.zeros(0, 3, dtype=torch.float64, device=_dev()), torch.zeros(0, 3, dtype=torch.int32, device=_dev()))
    on_plane = np.random.default_rng(0).uniform(0, 1, (500, 3)) * [1, 1, 0] + [0, 0, 0.3]
    P = [np.concatenate([solid, solid[:300] + [100.0, -50.0, 30.0]]), on_plane, solid, np.zeros((0, 3))]
    P = [torch.as_tensor(p).to(_dev()) for p in P]
    meshes = [(V, F), flat, empty, (V, F)]
    inside = [t.cpu().numpy() for t in ops.mesh_contains_batch(meshes, P)]
    dist = [t.cpu().numpy() for t in ops.mesh_distance_batch(meshes, P, 0.3)]
    assert inside[0][:3000].mean() > 0.85 and not inside[0][3000:].any()
    assert np.isfinite(dist[0][:3000]).mean() > 0.9 and np.isinf(dist[0][3000:]).all()
    assert not inside[1].any() and np.isfinite(dist[1]).all() and dist[1].max() < 1e-12      # flat: on it, never inside it
    assert not inside[2].any() and np.isinf(dist[2]).all()                                    # empty
    assert inside[3].size == 0 and dist[3].size == 0


def test_batch_ops_beside_encode_stream():
    """the batch ops on one stream while another runs Shape_Prior.encode: the same results as alone"""
    from livingscenes_amd import ops, synth
    from livingscenes_amd.model_utils import Shape_Prior
    ecfg, dcfg = synth.small_encoder_cfg(), synth.small_decoder_cfg()
    sp = Shape_Prior.from_state(ecfg, dcfg, synth.make_encoder_weights(ecfg, 2), synth.make_decoder_weights(dcfg, 2), device=_dev(), n_pcl=256)
    x = synth.make_instances(64, 256, seed=5).to(_dev())
    meshes, pts = _case(5, seed=7)
    counts, seeds = _counts_seeds(meshes, np.random.default_rng(7))

    def run():
        return (ops.mesh_contains_batch(meshes, pts), ops.mesh_distance_batch(meshes, pts, 0.05),
                [p for p, _ in ops.mesh_sample_batch(meshes, counts, seeds)])
    alone = [[t.cpu() for t in r] for r in run()]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    for _ in range(2):
        with torch.no_grad(), torch.cuda.stream(s2):
            for _ in range(3):
                sp.encode(x)
        with torch.cuda.stream(s1):
            res = run()
        torch.cuda.synchronize()
        for a, r in zip(alone, res):
            _assert_outputs_equal([t.cpu() for t in r], a)


# ------------------------------------------------------------------------------------------------ 2. argument errors
def _contains_raw(V, vo, F, fo, P, po, nv_total=None, nf_total=None):
    from livingscenes_amd import _lib
    from livingscenes_amd._lib import call, ptr, stream_ptr
    vo, fo, po = (np.asarray(o, np.int64) for o in (vo, fo, po))
    out = torch.empty(P.shape[0], dtype=torch.bool, device=_dev())
    cnt = torch.empty(1, dtype=torch.int64, device=_dev())
    M = len(vo) - 1
    ws = torch.empty(max(1, _lib.load().ls_mesh_contains_batch_workspace_bytes(M, F.shape[0], 64)), dtype=torch.uint8, device=_dev())
    h = lambda a: ctypes.c_void_p(a.ctypes.data)
    call(_dev(), "ls_mesh_contains_batch_f64", M, ptr(V), V.shape[0] if nv_total is None else nv_total, h(vo), ptr(F),
         F.shape[0] if nf_total is None else nf_total, h(fo), ptr(P), P.shape[0], h(po), 64, ptr(out), None, 0, ptr(cnt), ptr(ws), ws.numel(),
         stream_ptr(_dev()))
    return out


def test_batch_argument_errors():
    from livingscenes_amd import _lib, ops
    meshes, pts = _case(3, seed=1)
    V = torch.cat([m[0] for m in meshes])
    F = torch.cat([m[1] for m in meshes])
    P = torch.cat(pts)
    nv = [m[0].shape[0] for m in meshes]
    nf = [m[1].shape[0] for m in meshes]
    vo, fo, po = (np.concatenate([[0], np.cumsum(a)]) for a in (nv, nf, [p.shape[0] for p in pts]))
    _contains_raw(V, vo, F, fo, P, po)                              # the well-formed call goes through
    bad = fo.copy()
    bad[2] = bad[1] - 1                                              # mesh 1's face range runs backwards
    with pytest.raises(_lib.LsError, match=r"mesh 1: face_off decreases"):
        _contains_raw(V, vo, F, bad, P, po)
    with pytest.raises(_lib.LsError, match=r"mesh 2: vert_off ends at .* disagrees with the total"):
        _contains_raw(V, vo, F, fo, P, po, nv_total=V.shape[0] + 1)
    with pytest.raises(_lib.LsError, match=r"mesh 2: face_off ends at .* disagrees with the total"):
        _contains_raw(V, vo, F, fo, P, po, nf_total=F.shape[0] - 1)
    empty = (torch.zeros(0, 3, dtype=torch.float64, device=_dev()), torch.zeros(0, 3, dtype=torch.int32, device=_dev()))
    with pytest.raises(_lib.LsError, match=r"mesh 1: empty mesh .* cannot give 5 samples"):
        ops.mesh_sample_batch([meshes[0], empty], [10, 5])
    Vb, Fb = meshes[1]
    Fb = Fb.clone()
    Fb[3, 1] = Vb.shape[0]                                           # one past its own mesh's vertices (valid in the packed array)
    from livingscenes_amd import evaluate
    bad_meshes = [Mesh(V.cpu().numpy(), F.cpu().numpy()) for V, F in (meshes[0], (Vb, Fb), meshes[2])]
    with pytest.raises(ValueError, match=r"mesh 1: faces index vertices outside"):
        evaluate.check_mesh_contains_batch(bad_meshes, pts)
    with pytest.raises(ValueError, match=r"mesh 1: faces index vertices outside"):
        evaluate.compute_sdf_recall_batch(bad_meshes, [Mesh(p.cpu().numpy(), np.zeros((0, 3))) for p in pts])
    # the ops themselves do not read the device to check (nor do the single forms): they give what the single op gives on that mesh
    _assert_outputs_equal(ops.mesh_contains_batch([meshes[0], (Vb, Fb)], pts[:2]), _single_contains([meshes[0], (Vb, Fb)], pts[:2], 512))
    _assert_outputs_equal(ops.mesh_distance_batch([meshes[0], (Vb, Fb)], pts[:2], 0.1), _single_distance([meshes[0], (Vb, Fb)], pts[:2], 0.1))
    with pytest.raises(_lib.LsError):                                # the dtype checks of the single forms
        ops.mesh_distance_batch([(meshes[0][0].float(), meshes[0][1])], pts[:1], 0.1)
    with pytest.raises(ValueError, match=r"mesh 0: faces index vertices outside"):
        evaluate.check_mesh_contains_batch([Mesh(meshes[0][0].cpu().numpy(), meshes[0][1].cpu().numpy().astype(np.int64) + 2 ** 32)], [pts[0]])


# ------------------------------------------------------------------------------------------------ 3. evaluate's batch functions
def _same(a, b):
    return a == b or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


def test_evaluate_batch_functions_equal_per_mesh():
    from livingscenes_amd import _lib, evaluate, synth
    preds = [synth.canonical_mesh(21 + i, res=r) for i, r in enumerate((20, 28, 32))]
    preds.insert(1, Mesh(np.zeros((0, 3)), np.zeros((0, 3))))        # an empty predicted mesh inside the batch
    gts = [synth.canonical_mesh(21 + i, res=24) for i in range(4)]
    gts[2] = Mesh(gts[2].vertices + 0.01, gts[2].faces)
    rec = evaluate.compute_sdf_recall_batch(preds, gts, 0.05)
    iou = evaluate.compute_volumetric_iou_batch(preds, gts)
    assert len(rec) == len(iou) == 4
    for i, (p, g) in enumerate(zip(preds, gts)):
        assert _same(rec[i], evaluate.compute_sdf_recall(p, g, 0.05)), i
        assert _same(iou[i], evaluate.compute_volumetric_iou(p, g)), i
    assert rec[1] == 0.0 and iou[1] == 0.0
    ins = evaluate.check_mesh_contains_batch(preds, [g.vertices for g in gts])
    for p, g, a in zip(preds, gts, ins):
        assert a.dtype == bool and np.array_equal(a, evaluate.check_mesh_contains(p, g.vertices))
    live = [0, 2, 3]
    for seeds, off, sc in ((None, 0, 1), ([3, 0, 2 ** 63 + 5], 0.1, 1.5)):
        cd = evaluate.compute_chamfer_distance_batch([gts[i] for i in live], [preds[i] for i in live], off, sc, num_mesh_samples=4000, seeds=seeds)
        for k, i in enumerate(live):
            want = evaluate.compute_chamfer_distance(gts[i], preds[i], off, sc, num_mesh_samples=4000, seed=0 if seeds is None else seeds[k])
            assert cd[k] == want, (k, cd[k], want)
    # an empty mesh raises where the single function raises
    with pytest.raises(_lib.LsError):
        evaluate.compute_chamfer_distance(gts[1], preds[1], 0, 1)
    with pytest.raises(_lib.LsError, match="mesh 1"):
        evaluate.compute_chamfer_distance_batch(gts[:2], preds[:2], 0, 1)
    assert evaluate.compute_sdf_recall_batch([], []) == [] and evaluate.compute_chamfer_distance_batch([], [], 0, 1) == []


# ------------------------------------------------------------------------------------------------ 4. batched meshing and the harness legs
@pytest.fixture(scope="module")
def small_solver():
    from livingscenes_amd import synth
    from livingscenes_amd.lib_more.more_solver import More_Solver
    from livingscenes_amd.model_utils import Shape_Prior
    ecfg, dcfg = synth.small_encoder_cfg(), synth.small_decoder_cfg()
    sp = Shape_Prior.from_state(ecfg, dcfg, synth.make_encoder_weights(ecfg, 4), synth.make_decoder_weights(dcfg, 4), device=_dev(), n_pcl=128)
    cfg = {"shape_priors": {"n_input_point": 128, "prior_name": "chair", "ckpt_dir": ""}, "fps": {"n_init": 1, "random_start": False},
           "mesh_extractor": dict(threshold=0.5, resolution0=16, upsampling_steps=1, sample=False, simplify_nfaces=None,
                                  points_batch_size=100000, refinement_step=0)}
    solver = More_Solver(cfg, model=sp)
    code = sp.encode(synth.make_instances(1, 128, seed=1).to(_dev()))
    canon = {k: v.clone() for k, v in code.items()}
    canon["t"], canon["s"] = torch.zeros_like(canon["t"]), torch.ones_like(canon["s"])
    level = float(np.median(solver.mesh_extractor.eval_grid(canon, sp.decoder)))   # iso-level of the untrained field
    solver.mesh_extractor.threshold = 1.0 / (1.0 + np.exp(-level))
    return solver


def test_mesh_from_latent_batch_equals_per_row(small_solver):
    from livingscenes_amd import synth
    from livingscenes_amd.model_utils import slice_code_dict
    with torch.no_grad():
        codes = small_solver.model.encode(synth.make_instances(18, 128, seed=9).to(_dev()))   # two groups: 16 + 2
    ext = small_solver.mesh_extractor
    full = None
    try:
        for nfaces, threads in ((None, 1), (300, 1), (300, 4)):
            ext.simplify_nfaces = nfaces
            got = small_solver._mesh_from_latent_batch(codes, threads=threads)
            assert len(got) == 18
            for i, m in enumerate(got):
                want = small_solver._mesh_from_latent(slice_code_dict(codes, i))
                assert np.array_equal(m.vertices, want.vertices) and np.array_equal(m.faces, want.faces), (nfaces, threads, i)
            sizes = [len(m.faces) for m in got]
            assert max(sizes) > 0
            if nfaces is None:
                full = sizes
            else:                        # decimated (it may stop above the target when no legal collapse is left)
                assert all(a <= b for a, b in zip(sizes, full)) and sum(sizes) < sum(full)
    finally:
        ext.simplify_nfaces = None
    from livingscenes_amd.lib_more.more_solver import More_Solver
    with pytest.raises(ValueError, match="mesh_extractor"):
        More_Solver({k: v for k, v in small_solver.cfg.items() if k != "mesh_extractor"}, model=small_solver.model)._mesh_from_latent_batch(codes)


def _dict_equal(a, b):
    assert set(a) == set(b)
    for k in a:
        x, y = a[k], b[k]
        if isinstance(x, list):
            assert len(x) == len(y) and all(_same(float(u), float(v)) for u, v in zip(x, y)), k
        else:
            assert _same(x, y), (k, x, y)


def test_eval_reconstruction_batched_equals_per_object(small_solver):
    from livingscenes_amd import harness, synth
    scenes = [synth.make_scene_pair(n_obj=2, N=128, seed=s) for s in (3, 4)]
    gts = [[synth.canonical_mesh(s * 100003 + i, res=32) for i in range(2)] for s in (3, 4)]
    per_object = harness.eval_reconstruction(scenes, small_solver, gts)
    batched = harness.eval_reconstruction(scenes, small_solver, gts, batched=True)
    assert batched["n_objects"] == 4
    _dict_equal(batched, per_object)


def test_eval_3rscan_reconstruction_batched(small_solver, tmp_path, monkeypatch):
    from livingscenes_amd import evaluate, harness, rscan, synth
    rng = np.random.default_rng(6)
    root = tmp_path / "data"
    objs = {3: ("chair", 1300, 401), 8: ("table", 1100, 402), 12: ("lamp", 700, 403), 15: ("chair", 1200, 404)}
    pts, ids, shifts = [], [], []
    for oid, (_, n, sd) in objs.items():
        shifts.append(rng.uniform(-2, 2, 3))
        pts.append((synth.canonical_shape(n, sd) + shifts[-1]).astype(np.float32))
        ids.append(np.full(n, oid))
    rscan.write_scan(str(root / "val_set"), "scanA", np.concatenate(pts), np.concatenate(ids),
                     [{"objectId": o, "label": l} for o, (l, _, _) in objs.items()])
    rscan.write_index(str(root), "val", [{"reference": "scanA", "scans": []}])
    os.makedirs(root / "val_set_recon" / "scanA")
    for (oid, (_, _, sd)), t in zip(objs.items(), shifts):
        m = synth.canonical_mesh(sd, res=32)
        rscan.write_ply_mesh(str(root / "val_set_recon" / "scanA" / f"objectId_{oid}.ply"), m.vertices + t, m.faces)
    ds = rscan.Dataset_3RScan({"root_path": str(root), "split": "val", "category_list": ["chair", "table"], "n_point_per_instance": 1024,
                               "use_gt_mask": True}, device=_dev())
    ref, _ = ds._get_scene(0)
    gts = [rscan.load_ply_mesh(str(root / "val_set_recon" / "scanA" / f"objectId_{int(o)}.ply")) for o in ref["objectId"]]
    orig = small_solver._mesh_from_latent_batch
    for optim in (False, True):
        made = []

        def spy(codes, **kw):
            out = orig(codes, **kw)
            made.extend(out)
            return out
        monkeypatch.setattr(small_solver, "_mesh_from_latent_batch", spy)
        out = harness.eval_3rscan_reconstruction(ds, small_solver, optim=optim, batched=True)
        monkeypatch.undo()
        base = harness.eval_3rscan_reconstruction(ds, small_solver, optim=optim)
        assert set(out) == set(base)
        assert out["n_objects"] == base["n_objects"] == 3 and out["n_empty"] == base["n_empty"]
        assert len(made) == 3 and len(out["sdf_recall"]) == 3 and len(out["cd"]) == 3 - out["n_empty"]
        cd = iter(out["cd"])
        for m, (gv, gf), r in zip(made, gts, out["sdf_recall"]):
            g = Mesh(gv, gf)
            if len(m.vertices) == 0:
                assert r == 0.0
                continue
            assert next(cd) == evaluate.compute_chamfer_distance(g, m, offset=0, scale=1)[0]
            assert r == evaluate.compute_sdf_recall(m, g, 0.05)
        assert out["chamfer_1way_mean"] == pytest.approx(np.mean(out["cd"]), rel=1e-12) if out["cd"] else math.isnan(out["chamfer_1way_mean"])
