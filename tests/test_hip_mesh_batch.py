"""GPU tests of the batched mesh extraction: B MISE octrees per launch (csrc/mise.hip, ls_mise_*_batch), B volumes per marching-cubes launch
(csrc/mcubes.hip, ls_marching_cubes_batch_f64) and Generator3D on top of them.  Everything here is integer / flag work or a float64 formula
evaluated once per output, so every comparison is exact: against the reference's recorded rounds and meshes (tests/golden), the CPU oracles,
and the single ops item by item."""
import ctypes
import os

import numpy as np
import pytest
import torch

from livingscenes_amd import synth
from livingscenes_amd._lib import call, load, ptr, stream_ptr
from livingscenes_amd.mesh_extractor2 import MISE, Generator3D, MISEBatch, marching_cubes, marching_cubes_batch
from mise_fields import FIELDS

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BOX = 1.1
NAMES = sorted(FIELDS)


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _points(idx, R):
    """query coordinates of lattice indices (mesh_extractor2.py:122-124, float32)"""
    G = R + 1
    p = np.stack([idx // (G * G), (idx // G) % G, idx % G], 1)
    return np.float32(BOX) * (p.astype(np.float32) / np.float32(R) - np.float32(0.5))


def _drive(mb, names, max_rounds=16):
    """The loop of eval_grid_batch with analytic fields, octree b following FIELDS[names[b]] -> rounds[r][b] = the lattice indices octree b asked
    for in round r.  Checks on the way that inst / pts / offsets describe idx."""
    rounds = []
    for _ in range(max_rounds):
        idx, inst, pts, off = mb.query_device(BOX)
        assert len(off) == mb.B + 1 and off[0] == 0 and all(a <= b for a, b in zip(off, off[1:])) and idx.shape[0] == off[-1]
        if off[-1] == 0:
            return rounds
        idx_h, inst_h = idx.cpu().numpy().astype(np.int64), inst.cpu().numpy()
        assert np.array_equal(inst_h, np.repeat(np.arange(mb.B), np.diff(off)))
        pf = _points(idx_h, mb.resolution)
        assert np.array_equal(pts.cpu().numpy(), pf)
        vals = np.empty(off[-1], np.float32)
        which = np.asarray([NAMES.index(n) for n in names])[inst_h]
        for k, name in enumerate(NAMES):
            vals[which == k] = FIELDS[name](pf[which == k])
        rounds.append([idx_h[off[b]:off[b + 1]] for b in range(mb.B)])
        mb.update_device(idx, inst, torch.from_numpy(vals).to(mb.device))
    raise AssertionError("the octrees did not finish")


# ------------------------------------------------------------------------------------------------ 1. against the reference's recorded rounds
@pytest.mark.parametrize("keys", [("sphere_8_2", "torus_8_2"), ("empty_4_2", "plane_tie_4_2"), ("plane_tie_4_2", "empty_4_2")])
def test_mise_batch_matches_reference_golden(keys):
    """Octrees of one batch against the rounds recorded from the reference's Cython MISE.  `empty` is finished after round 0 while `plane_tie`
    runs three rounds: from then on its slice of the packed query is empty (once the first slice, once the last) and every further batched
    update has to leave it as it is -- the fixed point of ls_mise_update_batch."""
    g = np.load(os.path.join(GOLDEN, "mise.npz"))
    cfgs = [tuple(g[k + "_cfg"]) for k in keys]
    assert len(set(cfgs)) == 1
    res0, depth, thr = cfgs[0]
    mb = MISEBatch(len(keys), int(res0), int(depth), float(thr), device=_dev())
    rounds = _drive(mb, [k.rsplit("_", 2)[0] for k in keys])
    nrounds = [int(g[k + "_nrounds"]) for k in keys]
    assert len(rounds) == max(nrounds)
    for r, per in enumerate(rounds):
        for b, k in enumerate(keys):
            want = g[k + f"_round{r}"] if r < nrounds[b] else np.zeros(0, np.int64)
            assert np.array_equal(per[b], want), (k, r)
    dense = mb.to_dense_device().cpu().numpy()
    for b, k in enumerate(keys):
        assert np.array_equal(dense[b], g[k + "_dense"]), k


# ------------------------------------------------------------------------------------------------ 2. against oracle/mise.py
RES0, DEPTH = 4, 3          # G = 33: 35 937 lattice points = 8 compaction blocks of 4096 and a partial ninth


@pytest.fixture(scope="module")
def oracle_runs():
    """name -> (lattice indices per round, dense grid) of oracle/mise.py at (4, 3); 1 (empty) to 5 (two_blobs) rounds"""
    from oracle import mise as om
    G = (RES0 << DEPTH) + 1
    out = {}
    for name in NAMES:
        tr = []
        dense = om.run(FIELDS[name], RES0, DEPTH, threshold=0.0, box_size=BOX, trace=tr)
        out[name] = ([(p[:, 0] * G + p[:, 1]) * G + p[:, 2] for p in tr], dense.astype(np.float32))
    assert sorted(len(r) for r, _ in out.values()) == [1, 4, 4, 4, 5]
    return out


def test_mise_batch_five_fields_vs_oracle(oracle_runs):
    mb = MISEBatch(len(NAMES), RES0, DEPTH, 0.0, device=_dev())
    rounds = _drive(mb, NAMES)
    assert len(rounds) == 5
    for r, per in enumerate(rounds):
        for b, name in enumerate(NAMES):
            want = oracle_runs[name][0]
            assert np.array_equal(per[b], want[r] if r < len(want) else np.zeros(0, np.int64)), (name, r)
    dense = mb.to_dense_device().cpu().numpy()
    for b, name in enumerate(NAMES):
        assert np.array_equal(dense[b], oracle_runs[name][1]), name


def test_mise_batch_of_one_equals_the_single_ops():
    d = _dev()
    for name in ("two_blobs", "empty"):
        one, mb = MISE(RES0, DEPTH, 0.0, device=d), MISEBatch(1, RES0, DEPTH, 0.0, device=d)
        for r in range(8):
            i1, p1 = one.query_device(BOX)
            ib, inst, pb, off = mb.query_device(BOX)
            assert off == [0, i1.shape[0]] and torch.equal(i1, ib) and torch.equal(p1, pb) and int(inst.abs().sum()) == 0, (name, r)
            if i1.shape[0] == 0:
                break
            vals = torch.from_numpy(FIELDS[name](p1.cpu().numpy())).to(d)
            one.update_device(i1, vals)
            mb.update_device(ib, inst, vals)
        assert r == (5 if name == "two_blobs" else 1)
        assert torch.equal(one.to_dense_device(), mb.to_dense_device()[0]), name


def _single_query(mb, b):
    """ls_mise_query on slice b of a batch state"""
    stride = load().ls_mise_state_bytes(mb.resolution_0, mb.depth)
    cap = int(load().ls_mise_lattice_points(mb.resolution_0, mb.depth))
    idx = torch.empty(cap, dtype=torch.int32, device=mb.device)
    pts = torch.empty(cap, 3, dtype=torch.float32, device=mb.device)
    count = torch.zeros(1, dtype=torch.int32, device=mb.device)
    call(mb.device, "ls_mise_query", ptr(mb._state[b * stride:(b + 1) * stride]), mb.resolution_0, mb.depth, BOX, ptr(idx), ptr(pts), cap, ptr(count),
         stream_ptr(mb.device))
    n = int(count.item())
    return idx[:n], pts[:n]


def test_mise_batch_state_layout_and_cap():
    """Slice b of a batch state is a state of the single ops, and a query with a small cap writes nothing at or past it."""
    d = _dev()
    mb = MISEBatch(len(NAMES), RES0, DEPTH, 0.0, device=d)
    for _ in range(2):                                            # two rounds in: `empty` is finished, the others are not
        idx, inst, pts, off = mb.query_device(BOX)
        vals = np.empty(off[-1], np.float32)
        for b, name in enumerate(NAMES):
            vals[off[b]:off[b + 1]] = FIELDS[name](pts[off[b]:off[b + 1]].cpu().numpy())
        mb.update_device(idx, inst, torch.from_numpy(vals).to(d))
    idx, inst, pts, off = (t.clone() if torch.is_tensor(t) else t for t in mb.query_device(BOX))
    sizes = np.diff(off)
    assert sizes[NAMES.index("empty")] == 0 and (np.delete(sizes, NAMES.index("empty")) > 0).all()
    for b in range(mb.B):
        i1, p1 = _single_query(mb, b)
        assert torch.equal(i1, idx[off[b]:off[b + 1]]) and torch.equal(p1, pts[off[b]:off[b + 1]]), b
    total = off[-1]
    cap = off[2] + 7                                              # inside the third slice
    assert 0 < cap < total
    bi = torch.full((total,), -7, dtype=torch.int32, device=d)
    bn, bp = bi.clone(), torch.full((total, 3), -7.0, dtype=torch.float32, device=d)
    boff = torch.zeros(mb.B + 1, dtype=torch.int64, device=d)
    call(d, "ls_mise_query_batch", ptr(mb._state), mb.B, RES0, DEPTH, BOX, ptr(bi), ptr(bn), ptr(bp), cap, ptr(boff), stream_ptr(d))
    assert boff.cpu().tolist() == off                             # the full counts
    assert torch.equal(bi[:cap], idx[:cap]) and torch.equal(bn[:cap], inst[:cap]) and torch.equal(bp[:cap], pts[:cap])
    assert bool((bi[cap:] == -7).all()) and bool((bn[cap:] == -7).all()) and bool((bp[cap:] == -7.0).all())


# ------------------------------------------------------------------------------------------------ 3. more block sums than one scan pass
def test_mise_batch_scan_wider_than_one_pass():
    """(4, 2): 17^3 = 4913 lattice points = 2 compaction blocks per octree; B = 520 gives 1040 block sums, more than the 1024 threads of the scan."""
    d = _dev()
    B = 520
    names = [NAMES[b % len(NAMES)] for b in range(B)]
    mb = MISEBatch(B, 4, 2, 0.0, device=d)
    assert len(_drive(mb, names)) == 4                           # two_blobs runs four rounds at this size
    dense = mb.to_dense_device()
    ones = MISEBatch(1, 4, 2, 0.0, device=d)
    for k, name in enumerate(NAMES):
        ones.reset()
        _drive(ones, [name])
        want = ones.to_dense_device()[0]
        assert torch.equal(dense[k::len(NAMES)], want.expand(len(range(k, B, len(NAMES))), -1, -1, -1)), name


# ------------------------------------------------------------------------------------------------ 4. marching cubes
def _np(pairs):
    return [(v.cpu().numpy(), f.cpu().numpy()) for v, f in pairs]


def test_marching_cubes_batch_of_one_matches_reference_golden():
    g = np.load(os.path.join(GOLDEN, "mcubes.npz"))
    for name in sorted(k[:-4] for k in g.files if k.endswith("_vol")):
        (v, f), = _np(marching_cubes_batch(torch.from_numpy(g[name + "_vol"][None]).to(_dev()), float(g[name + "_iso"])))
        assert np.array_equal(v, g[name + "_v"]) and np.array_equal(f, g[name + "_f"]), name


def _six_volumes():
    rng = np.random.default_rng(11)
    r = [rng.standard_normal((7, 6, 5)) for _ in range(3)]
    tie = rng.standard_normal((7, 6, 5))
    tie[rng.random((7, 6, 5)) < 0.3] = 0.25                      # exactly the iso-value: the `<=` corner test and equal-valued edge ends
    return {"r0": r[0], "r1": r[1], "r2": r[2], "below": np.full((7, 6, 5), -1.0), "above": np.full((7, 6, 5), 2.0), "tie": tie}


@pytest.mark.parametrize("order", [("below", "r0", "above", "r1", "tie", "r2"), ("r0", "tie", "below", "r1", "r2", "above")])
def test_marching_cubes_batch_stack_vs_oracle_and_single(order):
    """Six 7 x 6 x 5 volumes; the two empty meshes (all below / all above the iso-value) stand first and in the middle, then in the middle and last."""
    from oracle import mcubes as om
    iso = 0.25
    vols = _six_volumes()
    stack = torch.from_numpy(np.stack([vols[k] for k in order])).to(_dev())
    got = _np(marching_cubes_batch(stack, iso))
    assert len(got) == 6
    for b, k in enumerate(order):
        v, f = got[b]
        wv, wf = om.marching_cubes(vols[k], iso)
        assert (len(wf) == 0) == (k in ("below", "above")), k
        assert v.shape == wv.shape and f.shape == wf.shape and np.array_equal(v, wv) and np.array_equal(f, wf), k
        (sv, sf), = _np([marching_cubes(stack[b], iso)])
        assert np.array_equal(v, sv) and np.array_equal(f, sf), k
        assert f.size == 0 or (0 <= f.min() and f.max() < len(v)), k


def _mc_raw(stack, iso, verts, cap_v, faces, cap_f):
    d = stack.device
    B, nx, ny, nz = stack.shape
    n = load().ls_mcubes_batch_workspace_bytes(B, nx, ny, nz)
    ws = torch.empty(n, dtype=torch.uint8, device=d)
    off = torch.full((2, B + 1), -1, dtype=torch.int64, device=d)
    call(d, "ls_marching_cubes_batch_f64", ptr(stack), B, nx, ny, nz, ctypes.c_double(iso), ptr(verts), cap_v, ptr(faces), cap_f, ptr(off), ptr(ws), n,
         stream_ptr(d))
    return off.cpu().numpy()


def test_marching_cubes_batch_sizing_call_and_caps():
    """The sizing call alone returns the offsets; with caps below the totals nothing at or past them is written and the offsets stay the full counts."""
    d = _dev()
    vols = _six_volumes()
    stack = torch.from_numpy(np.stack([vols[k] for k in ("r0", "below", "tie", "r1", "r2", "above")])).to(d).contiguous()
    full = marching_cubes_batch(stack, 0.25)
    vo = np.cumsum([0] + [len(v) for v, _ in full])
    fo = np.cumsum([0] + [len(f) for _, f in full])
    assert np.array_equal(_mc_raw(stack, 0.25, None, 0, None, 0), np.stack([vo, fo]))
    V, F = torch.cat([v for v, _ in full]), torch.cat([f for _, f in full])
    for cap_v, cap_f in ((0, 0), (int(vo[3]) + 1, int(fo[2]) + 2)):
        bv = torch.full((int(vo[-1]), 3), -7.0, dtype=torch.float64, device=d)
        bf = torch.full((int(fo[-1]), 3), -7, dtype=torch.int64, device=d)
        assert np.array_equal(_mc_raw(stack, 0.25, bv, cap_v, bf, cap_f), np.stack([vo, fo]))
        assert torch.equal(bv[:cap_v], V[:cap_v]) and torch.equal(bf[:cap_f], F[:cap_f])
        assert bool((bv[cap_v:] == -7.0).all()) and bool((bf[cap_f:] == -7).all())


def test_marching_cubes_batch_scan_wider_than_one_pass():
    """B = 520 volumes of 19^3: 18^3 = 5832 cubes = 2 blocks each, 1040 block sums; the analytic fields, each volume cut at another level."""
    d = _dev()
    B, n = 520, 19
    lin = np.linspace(-0.55, 0.55, n, dtype=np.float32)
    p = np.stack(np.meshgrid(lin, lin, lin, indexing="ij"), -1).reshape(-1, 3)
    base = {name: FIELDS[name](p).astype(np.float64).reshape(n, n, n) for name in NAMES}
    stack = torch.from_numpy(np.stack([base[NAMES[b % 5]] - 0.0001 * (b // 5) for b in range(B)])).to(d)
    got = marching_cubes_batch(stack, 0.0)
    nonempty = 0
    for b in range(B):
        sv, sf = marching_cubes(stack[b], 0.0)
        assert torch.equal(got[b][0], sv) and torch.equal(got[b][1], sf), b
        nonempty += sf.shape[0] > 0
    assert nonempty >= B // 2 and nonempty < B                   # `empty` stays empty


# ------------------------------------------------------------------------------------------------ 5. end to end
@pytest.fixture(scope="module")
def small_prior():
    from livingscenes_amd.model_utils import Shape_Prior
    ecfg, dcfg = synth.small_encoder_cfg(), synth.small_decoder_cfg()
    return Shape_Prior.from_state(ecfg, dcfg, synth.make_encoder_weights(ecfg, 4), synth.make_decoder_weights(dcfg, 4), device=_dev(), n_pcl=128)


def _generator_at_median(sp, codes):
    gen = Generator3D(threshold=0.5, resolution0=8, upsampling_steps=2, padding=0.1, simplify_nfaces=None)
    level = float(np.median(gen.eval_grid({k: v[:1] for k, v in codes.items()}, sp.decoder)))   # the synthetic field has no zero level set
    gen.threshold = 1.0 / (1.0 + np.exp(-level))
    return gen, level


def _assert_batch_equals_per_instance(gen, sp, codes):
    meshes = gen.generate_from_latent_batch(codes, sp.decoder)
    B = codes["z_inv"].shape[0]
    assert len(meshes) == B
    faces = []
    for b in range(B):
        one = gen.generate_from_latent({k: v[b:b + 1] for k, v in codes.items()}, sp.decoder)
        v, f, wv, wf = (np.asarray(a) for a in (meshes[b].vertices, meshes[b].faces, one.vertices, one.faces))
        assert v.shape == wv.shape and f.shape == wf.shape and np.array_equal(v, wv) and np.array_equal(f, wf), b
        faces.append(len(f))
    return faces


def test_generate_from_latent_batch_equals_per_instance(small_prior):
    sp = small_prior
    codes = {k: v.clone() for k, v in sp.encode(synth.make_instances(3, 128, seed=41).to(_dev())).items()}
    gen, _ = _generator_at_median(sp, codes)
    faces = _assert_batch_equals_per_instance(gen, sp, codes)
    assert faces[0] > 100


EMPTY_SHIFTS = [(s * a, s * b, s * c) for s in (3.0, 10.0, 100.0) for a, b, c in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))]


def test_generate_from_latent_batch_with_an_empty_grid(small_prior):
    """One of the three codes has no surface at the shared iso-level: every logit of its grid lies below it, so its mesh is empty (in the middle of the
    packed marching-cubes output) while the others keep theirs."""
    sp, d = small_prior, _dev()
    codes = {k: v.clone() for k, v in sp.encode(synth.make_instances(3, 128, seed=41).to(d)).items()}
    gen, level = _generator_at_median(sp, codes)
    # move instance 1 away from the query box until its logits on the whole 33^3 lattice are below the level
    G = 33
    lin = torch.arange(G, device=d, dtype=torch.float32) / (G - 1) - 0.5
    q = 1.1 * torch.stack(torch.meshgrid(lin, lin, lin, indexing="ij"), -1).reshape(1, -1, 3)
    t0 = codes["t"][1:2].clone()
    for shift in EMPTY_SHIFTS:
        codes["t"][1:2] = t0 + torch.tensor(shift, device=d, dtype=t0.dtype)
        with torch.no_grad():
            logits = sp.decoder(q, None, {k: v[1:2] for k, v in codes.items()}).logits
        if float(logits.max()) < level:
            break
    else:
        raise AssertionError("no shift of instance 1 empties its grid")
    faces = _assert_batch_equals_per_instance(gen, sp, codes)
    assert faces[1] == 0 and faces[0] > 100

