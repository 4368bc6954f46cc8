"""GPU tests of the device decimator (csrc/meshcluster.hip: ls_mesh_cluster_f64 / ls_mesh_cluster_batch_f64, mesh_extractor2.cluster_mesh_arrays*,
Generator3D(simplify_method="cluster")) against its NumPy twin (tests/cluster_oracle.py).  The cell keys, the resolution search and the face
selection are integer work on the same float64 quotients, so r and the faces are compared exactly; a vertex solves a system of condition
<= 1001 whose float64 sums have at most a few thousand terms about the cell mean (rounding <~ 1e-9 h), compared within 1e-7 h."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cluster_oracle as co  # noqa: E402
import meshmetrics_oracle as mo  # noqa: E402
from livingscenes_amd import ops, synth  # noqa: E402
from livingscenes_amd._lib import load, ptr, stream_ptr  # noqa: E402
from livingscenes_amd.mesh_extractor2 import (Generator3D, cluster_mesh_arrays, cluster_mesh_arrays_batch,  # noqa: E402
                                              marching_cubes)

pytestmark = pytest.mark.gpu
TARGETS = {"sphere": (386, 154, 514), "torus": (476, 190, 634), "open_sheet": (134, 53, 178), "flat": (32, 12, 42)}
CASES = [(n, t) for n, ts in TARGETS.items() for t in ts]


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(V, F):
    return torch.from_numpy(np.ascontiguousarray(V, np.float64)).to(_dev()), torch.from_numpy(np.ascontiguousarray(F, np.int64)).to(_dev())


def _assert_equals_twin(V, F, f_target, r_max=256, twin=None):
    wv, wf, wr, info = twin if twin is not None else co.cluster_mesh(V, F, f_target, r_max)
    v, f, r = cluster_mesh_arrays(*_t(V, F), f_target, r_max, return_r=True)
    v, f = v.cpu().numpy(), f.cpu().numpy()
    assert r == wr
    assert f.shape == wf.shape and np.array_equal(f, wf)
    assert v.shape == wv.shape
    if wr == 0:
        assert np.array_equal(v, wv)
    else:
        err = np.abs(v - wv).max() / info["h"]
        print(f"f_target {f_target}: r {r}, {len(f)} faces, {len(v)} vertices, max |dv| = {err:.2e} h")
        assert err <= 1e-7
    return v, f, r, info


# ------------------------------------------------------------------------------------------------ (a) the fixture meshes
@pytest.mark.parametrize("name,f_target", CASES, ids=[f"{n}-{t}" for n, t in CASES])
def test_cluster_fixture_meshes_equal_the_twin(golden, name, f_target):
    g = golden("simplify")
    _assert_equals_twin(g[name + "_v"], g[name + "_f"], f_target)


# ------------------------------------------------------------------------------------------------ (b) a closed mesh larger than any one block
@pytest.fixture(scope="module")
def bumpy():
    """unit icosphere, five subdivisions (20 480 faces), radius * (1 + 0.2 sin(5x) cos(4y)), axes scaled (0.4, 0.9, 0.4); its twin at 5000"""
    V, F = mo.icosphere(5)
    V = V * (1 + 0.2 * np.sin(5 * V[:, 0]) * np.cos(4 * V[:, 1]))[:, None] * np.array([0.4, 0.9, 0.4])
    assert F.shape[0] == 20480
    return V, F, co.cluster_mesh(V, F, 5000)


def test_cluster_large_mesh_equals_the_twin(bumpy):
    V, F, twin = bumpy
    v, f, r, _ = _assert_equals_twin(V, F, 5000, twin=twin)
    assert 30 <= r <= 60 and 4000 <= len(f) <= 5000
    _assert_equals_twin(V, F, 100000)                # under the target: an unchanged copy
    v8, f8, r8, _ = _assert_equals_twin(V, F, 5000, r_max=8)
    assert r8 == 8 and len(f8) < len(f)              # the search ends at r_max


def test_cluster_large_mesh_stays_within_a_cell_diagonal(bumpy):
    """A representative stays in its cell, so no surface point moves farther than the cell diagonal h sqrt(3): samples of the output lie that
    close to the input, and every point farther than that from the input surface keeps its mod-2 winding number (the map is simplicial and
    faces cancel in pairs), so ray parity answers the same for the output as for the input."""
    V, F, (wv, wf, wr, info) = bumpy
    Vd, Fd = _t(V, F)
    v, f = cluster_mesh_arrays(Vd, Fd, 5000)
    bound = info["h"] * np.sqrt(3.0)
    Fi, fi = Fd.to(torch.int32), f.to(torch.int32)
    samples, _ = ops.mesh_sample(v, fi, 20000, seed=5)
    d = ops.mesh_distance(Vd, Fi, samples, 4 * bound)
    print(f"output -> input distance: max {float(d.max()):.3e}, bound h sqrt(3) = {bound:.3e}")
    assert bool((d <= bound).all())
    rng = np.random.default_rng(3)
    lo, hi = V.min(0) - 0.05, V.max(0) + 0.05
    P = torch.from_numpy(lo + rng.random((40000, 3)) * (hi - lo)).to(_dev())
    far = torch.isinf(ops.mesh_distance(Vd, Fi, P, bound * (1 + 1e-9)))      # +inf: not closer than the cap
    inside_in, inside_out = ops.mesh_contains(Vd, Fi, P), ops.mesh_contains(v, fi, P)
    n_far, n_in = int(far.sum()), int((far & inside_in).sum())
    print(f"{n_far} of {P.shape[0]} points farther than h sqrt(3) from the input, {n_in} of them inside")
    assert n_far > 10000 and n_in > 1000
    assert torch.equal(inside_in[far], inside_out[far])


# ------------------------------------------------------------------------------------------------ (c) ragged batches
def _batch_meshes(golden, M):
    """ragged content at f_target 150: decimated meshes, an empty mesh, a mesh already under the target (flat, 128 faces), and the same mesh
    (torus) at two positions"""
    g = golden("simplify")
    empty = (np.zeros((0, 3)), np.zeros((0, 3), np.int64))
    kinds = [("torus", 0.0), ("empty", 0.0), ("flat", 0.0), ("sphere", 0.0), ("torus", 0.0), ("open_sheet", 0.0), ("sphere", 3.5)]
    out = []
    for m in range(M):
        name, shift = kinds[m % len(kinds)]
        out.append(empty if name == "empty" else (g[name + "_v"] + shift, g[name + "_f"]))
    return [_t(v, f) for v, f in out]


@pytest.mark.parametrize("M", [1, 5, 17])
def test_cluster_batch_is_bit_identical_to_the_single_op(golden, M):
    meshes = _batch_meshes(golden, M)
    got, r = cluster_mesh_arrays_batch(meshes, 150, return_r=True)
    again, r2 = cluster_mesh_arrays_batch(meshes, 150, return_r=True)
    assert len(got) == M and r == r2
    seen = set()
    for m, (V, F) in enumerate(meshes):
        sv, sf, sr = cluster_mesh_arrays(V, F, 150, return_r=True)
        assert r[m] == sr and torch.equal(got[m][0], sv) and torch.equal(got[m][1], sf), m
        assert torch.equal(again[m][0], got[m][0]) and torch.equal(again[m][1], got[m][1]), m
        assert sf.shape[0] <= 150 and (sr == 0) == (F.shape[0] <= 150)
        if sr == 0:
            assert torch.equal(sv, V) and torch.equal(sf, F)
        seen.add("empty" if F.shape[0] == 0 else "copied" if sr == 0 else "decimated")
    if M > 1:
        assert seen == {"empty", "copied", "decimated"}
        assert torch.equal(got[0][0], got[4][0]) and torch.equal(got[0][1], got[4][1])      # the torus twice
    # the packed form gives the same views
    V, F = torch.cat([v for v, _ in meshes]), torch.cat([f for _, f in meshes])
    vo, fo = np.cumsum([0] + [v.shape[0] for v, _ in meshes]), np.cumsum([0] + [f.shape[0] for _, f in meshes])
    packed = cluster_mesh_arrays_batch((V, F), 150, offsets=(vo, fo))
    assert all(torch.equal(a, c) and torch.equal(b, e) for (a, b), (c, e) in zip(packed, got))


def _raw_batch(meshes, f_target, verts, cap_v, faces, cap_f):
    """ls_mesh_cluster_batch_f64 as it is -> (status, off [2,M+1], r [M])"""
    d = _dev()
    M = len(meshes)
    V, F = torch.cat([v for v, _ in meshes]).contiguous(), torch.cat([f for _, f in meshes]).contiguous()
    vo = np.cumsum([0] + [v.shape[0] for v, _ in meshes]).astype(np.int64)
    fo = np.cumsum([0] + [f.shape[0] for _, f in meshes]).astype(np.int64)
    n = load().ls_mesh_cluster_batch_workspace_bytes(M, V.shape[0], F.shape[0], 256)
    ws = torch.empty(n, dtype=torch.uint8, device=d)
    off = torch.full((2, M + 1), -1, dtype=torch.int64, device=d)
    r = torch.full((M,), -9, dtype=torch.int32, device=d)
    P = ctypes.c_void_p
    with torch.cuda.device(d):
        rc = load().ls_mesh_cluster_batch_f64(M, ptr(V), V.shape[0], P(vo.ctypes.data), ptr(F), F.shape[0], P(fo.ctypes.data), f_target, 256, ptr(verts),
                                              cap_v, ptr(faces), cap_f, ptr(off), ptr(r), ptr(ws), n, stream_ptr(d))
    return rc, off.cpu().numpy(), r.cpu().numpy()


def test_cluster_batch_sizing_call_and_caps(golden):
    """The sizing call alone returns the offsets and the resolutions.  Caps below the totals are an error: refused on the host where a copied
    mesh (whose size is known there) does not fit, else reported as LS_ERR_INVALID in r_out for every mesh that reaches past a cap, with
    nothing written at or past the caps and the offsets still the full counts."""
    d = _dev()
    meshes = _batch_meshes(golden, 5)        # torus, empty, flat (copied), sphere, torus
    full, r = cluster_mesh_arrays_batch(meshes, 150, return_r=True)
    vo, fo = np.cumsum([0] + [len(v) for v, _ in full]), np.cumsum([0] + [len(f) for _, f in full])
    rc, off, rs = _raw_batch(meshes, 150, None, 0, None, 0)
    assert rc == 0 and np.array_equal(off, np.stack([vo, fo])) and rs.tolist() == r
    V, F = torch.cat([v for v, _ in full]), torch.cat([f for _, f in full])

    def run(cap_v, cap_f):
        bv = torch.full((int(vo[-1]), 3), -7.0, dtype=torch.float64, device=d)
        bf = torch.full((int(fo[-1]), 3), -7, dtype=torch.int64, device=d)
        rc, off, rs = _raw_batch(meshes, 150, bv, cap_v, bf, cap_f)
        return rc, off, rs, bv, bf

    rc, off, rs, bv, bf = run(int(vo[-1]), int(fo[-1]))           # exactly the totals
    assert rc == 0 and rs.tolist() == r and torch.equal(bv, V) and torch.equal(bf, F)
    for cap_v, cap_f, bad in ((int(vo[4]) + 3, int(fo[-1]), [4]), (int(vo[-1]), int(fo[3]) + 2, [3, 4]), (int(vo[3]) + 1, int(fo[3]) + 1, [3, 4])):
        rc, off, rs, bv, bf = run(cap_v, cap_f)
        assert rc == 0 and np.array_equal(off, np.stack([vo, fo]))
        assert rs.tolist() == [-1 if m in bad else r[m] for m in range(5)]
        assert torch.equal(bv[:cap_v], V[:cap_v]) and torch.equal(bf[:cap_f], F[:cap_f])
        assert bool((bv[cap_v:] == -7.0).all()) and bool((bf[cap_f:] == -7).all())
    # the copied mesh alone (95 vertices, 128 faces) does not fit: refused before any launch
    for cap_v, cap_f in ((94, int(fo[-1])), (int(vo[-1]), 127)):
        rc, _, _, bv, bf = run(cap_v, cap_f)
        assert rc == -1 and b"mesh 2" in load().ls_last_error()
        assert bool((bv == -7.0).all()) and bool((bf == -7).all())


# ------------------------------------------------------------------------------------------------ (d) Generator3D
@pytest.fixture(scope="module")
def small_prior():
    from livingscenes_amd.model_utils import Shape_Prior
    ecfg, dcfg = synth.small_encoder_cfg(), synth.small_decoder_cfg()
    return Shape_Prior.from_state(ecfg, dcfg, synth.make_encoder_weights(ecfg, 4), synth.make_decoder_weights(dcfg, 4), device=_dev(), n_pcl=128)


def _generator_at_median(sp, codes):
    gen = Generator3D(threshold=0.5, resolution0=16, upsampling_steps=1, padding=0.1, simplify_nfaces=500, simplify_method="cluster")
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
        assert len(f) <= 500
        faces.append(len(f))
    return meshes, faces


def test_generator_cluster_batch_equals_per_instance_and_the_op(small_prior):
    sp = small_prior
    codes = {k: v.clone() for k, v in sp.encode(synth.make_instances(3, 128, seed=41).to(_dev())).items()}
    gen, _ = _generator_at_median(sp, codes)
    meshes, faces = _assert_batch_equals_per_instance(gen, sp, codes)
    assert faces[0] > 100
    # the same as the op on the marching-cubes output, normalised afterwards
    logit = np.log(gen.threshold) - np.log(1.0 - gen.threshold)
    for b in range(3):
        grid = gen.eval_grid({k: v[b:b + 1] for k, v in codes.items()}, sp.decoder, on_device=True)
        mv, mf = marching_cubes(torch.nn.functional.pad(grid, (1, 1, 1, 1, 1, 1), value=-1e6), logit)
        assert mf.shape[0] > 500
        cv, cf = cluster_mesh_arrays(mv, mf, 500)
        want_v = gen._normalise_vertices(cv.cpu().numpy(), grid.shape)
        assert np.array_equal(np.asarray(meshes[b].vertices), want_v) and np.array_equal(np.asarray(meshes[b].faces), cf.cpu().numpy()), b
    # the default decimator is untouched by the switch
    assert Generator3D(simplify_nfaces=500).simplify_method == "collapse"


EMPTY_SHIFTS = [(s * a, s * b, s * c) for s in (3.0, 10.0, 100.0) for a, b, c in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))]


def test_generator_cluster_batch_with_an_empty_grid(small_prior):
    """One of the three codes has no surface at the shared iso-level: its mesh is empty, in the middle of the packed marching-cubes output that
    is decimated, while the others keep theirs."""
    sp, d = small_prior, _dev()
    codes = {k: v.clone() for k, v in sp.encode(synth.make_instances(3, 128, seed=41).to(d)).items()}
    gen, level = _generator_at_median(sp, codes)
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
    _, faces = _assert_batch_equals_per_instance(gen, sp, codes)
    assert faces[1] == 0 and faces[0] > 100
