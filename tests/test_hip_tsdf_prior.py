"""GPU tests of the completion of a fused state by the shape prior's field (csrc/tsdfprior.hip: ls_tsdf_prior_rows_f32,
ls_tsdf_prior_vote_f32 and their batches) against tests/tsdf_prior_oracle.py BY EQUALITY at the size edges of the ballot words and the
4096-sample blocks; the batch invariants; the state that needs no row; the mesh and the raycast of a completed state; the capability
itself (an open observed shell closed by the field); the decoder path of More_Solver._complete_fusion_batch; solve_sequence_completed.
Every test asserts that the observed state keeps its bits.  The states, the planted values and the sphere live in
tests/test_tsdf_prior_cpu.py."""
import functools

import numpy as np
import pytest
import torch

import fuse_oracle as fo
import tsdf_prior_oracle as tpo
from cloud_testlib import CODE_KEYS, _dev, _scene, _solver, small_prior  # noqa: F401 (small_prior is a fixture)
from livingscenes_amd import ops
from test_depth_fuse_cpu import _look_at, _rot, _sphere_depth
from test_hip_tsdf_fit import _fusion_scene
from test_tsdf_prior_cpu import EDGE_DIMS, WEIGHTS, boundary_edges, edge_grid, hand_set, least_seen_around, planted_values, sphere_case

pytestmark = pytest.mark.gpu
KINDS3 = ("empty", "saturated", "mixed")


def _d(x, dtype=None):
    t = torch.from_numpy(np.array(x)).to(_dev())                         # a copy: the shared host arrays are read-only
    return t if dtype is None else t.to(dtype)


def _np(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def fused_host(dims):
    """two small synthetic views of a sphere fused ON THE DEVICE (ops.depth_fuse) into a grid of `dims` -> host (sum, n), read-only"""
    origin, h, trunc = edge_grid(dims)
    centre = origin + h * (np.array(dims) - 1) / 2
    rng = np.random.default_rng(sum(dims))
    K = np.array([48.0, 48.0, 24.0, 24.0])
    E = np.stack([_look_at(_rot(rng)) for _ in range(2)])
    depth = np.stack([_sphere_depth(e, K, 48, 48, 0.3 * h * max(dims)) for e in E])
    E[:, :, 3] -= E[:, :, :3] @ centre
    S, N = (t[0] for t in ops.tsdf_state(1, dims, _dev()))
    ops.depth_fuse((S, N), _d(depth), _d(np.tile(K, (2, 1))), _d(E), origin=origin, voxel=h, trunc=trunc, empty="free")
    out = (_np(S), _np(N))
    for t in out:
        t.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def edge_case(dims, w0):
    """-> (host states of KINDS3, origin, h, trunc): the fused views plus hand-set samples; computed once and shared"""
    origin, h, trunc = edge_grid(dims)
    sts = []
    for k, kind in enumerate(KINDS3):
        st = hand_set(tuple(t.copy() for t in fused_host(dims)), w0, kind, 10 * k + sum(dims) + w0 % 5)
        for t in st:
            t.setflags(write=False)
        sts.append(st)
    return sts, origin, h, trunc


def _same_rows(got, want, inst=None):
    assert np.array_equal(_np(got[2]), want["row_index"]) and np.array_equal(_np(got[0]).view(np.uint32), want["points"].view(np.uint32))
    assert np.array_equal(_np(got[1]), want["row_inst"] if inst is None else np.full(len(want["row_index"]), inst, np.int32))


def _unchanged(dev_state, host_state):
    return all(np.array_equal(_np(a), b) for a, b in zip(dev_state, host_state))


@pytest.mark.parametrize("w0", WEIGHTS)
@pytest.mark.parametrize("dims", EDGE_DIMS)
def test_rows_votes_and_counts_equal_the_twin(dims, w0):
    """P = 1 (the mixed state through the single entries) and P = 3 (empty: every sample eligible; saturated: no row; mixed): the rows,
    their order, the offsets, the counts and (sum', n') equal the twin's, f random fp32 with the special values planted"""
    sts, origin, h, trunc = edge_case(dims, w0)
    s = [2.0, 0.37, 1.9]
    tr = [0.25, trunc, trunc]
    # the single entries on the mixed state
    state = tuple(_d(t) for t in sts[2])
    want = tpo.rows(sts[2], origin, h, w0)
    rows = ops.tsdf_prior_rows(state, origin=origin, voxel=h, weight=w0)
    _same_rows(rows, want)
    assert rows[3] == [0, len(want["row_index"])] and np.array_equal(_np(rows[4]), want["counts"]) and 0 < rows[3][1] < np.prod(dims)
    f = planted_values(rows[3][1], s[2], tr[2], w0 + sum(dims))
    (S2, N2), counts = ops.tsdf_complete(state, _d(f), rows, s=s[2], trunc=tr[2], weight=w0)
    (ws, wn), wc = tpo.vote(sts[2], f, s[2], tr[2], w0)
    print(dims, w0, "single", _np(counts).tolist(), wc.tolist())
    assert np.array_equal(_np(S2), ws) and np.array_equal(_np(N2), wn) and np.array_equal(_np(counts), wc)
    assert _unchanged(state, sts[2]) and S2.data_ptr() != state[0].data_ptr()
    # the batch
    bstate = tuple(_d(np.stack([st[i] for st in sts])) for i in range(2))
    want = tpo.rows_batch(sts, [origin] * 3, [h] * 3, w0)
    rows = ops.tsdf_prior_rows_batch(bstate, origin=origin, voxel=h, weight=w0, packed=True)
    _same_rows(rows, want)
    assert rows[3] == want["offsets"] and np.array_equal(_np(rows[4]), want["counts"])
    assert rows[3][1] == np.prod(dims) and rows[3][2] == rows[3][1] and rows[3][3] > rows[3][2]
    f = np.concatenate([planted_values(want["offsets"][p + 1] - want["offsets"][p], s[p], tr[p], 7 * p + w0) for p in range(3)])
    (S2, N2), counts = ops.tsdf_complete_batch(bstate, _d(f), rows, s=s, trunc=tr, weight=w0)
    wstates, wc = tpo.vote_batch(sts, f, want["offsets"], s, tr, w0)
    print(dims, w0, "batch", _np(counts).tolist())
    for p in range(3):
        assert np.array_equal(_np(S2[p]), wstates[p][0]) and np.array_equal(_np(N2[p]), wstates[p][1]), p
    assert np.array_equal(_np(counts), wc) and wc[0, 2] >= (1 if np.prod(dims) > 8 else 0) and wc[1].tolist() == [0, 0, 0, int(np.prod(dims))]
    assert int(N2.max()) <= 65535 and bool((S2.long().abs() <= N2.long() * 16384).all()) and bool((N2 == torch.maximum(bstate[1], N2)).all())
    assert all(_unchanged(tuple(t[p] for t in bstate), sts[p]) for p in range(3))
    lists = ops.tsdf_prior_rows_batch(bstate, origin=origin, voxel=h, weight=w0)
    assert [len(x) for x in lists[:3]] == [3, 3, 3] and all(torch.equal(torch.cat(lists[i]), rows[i]) for i in range(3))


@pytest.mark.parametrize("dims", EDGE_DIMS)
def test_batch_invariants(dims):
    """the single call equals the same problem inside the batch, bit for bit; the batch in reversed order equals the permuted result;
    two runs are identical"""
    w0 = 3
    sts, origin, h, trunc = edge_case(dims, w0)
    origins = np.stack([origin, origin + 0.01, origin - 0.02])
    hs, tr, s = [h, 1.5 * h, 0.7 * h], [trunc, 0.25, 2 * trunc], [0.37, 2.0, 1.9]
    bstate = tuple(_d(np.stack([st[i] for st in sts])) for i in range(2))

    def run(order):
        st = tuple(t[list(order)].contiguous() for t in bstate)
        rows = ops.tsdf_prior_rows_batch(st, origin=origins[list(order)], voxel=[hs[i] for i in order], weight=w0, packed=True)
        f = torch.cat([_d(planted_values(rows[3][k + 1] - rows[3][k], s[i], tr[i], 3 + i)) for k, i in enumerate(order)])
        done, counts = ops.tsdf_complete_batch(st, f, rows, s=[s[i] for i in order], trunc=[tr[i] for i in order], weight=w0)
        return rows, f, done, counts

    rows, f, done, counts = run((0, 1, 2))
    again = run((0, 1, 2))
    assert all(torch.equal(a, b) for a, b in zip(rows[:3], again[0][:3])) and rows[3] == again[0][3] and torch.equal(rows[4], again[0][4])
    assert torch.equal(done[0], again[2][0]) and torch.equal(done[1], again[2][1]) and torch.equal(counts, again[3])
    rrows, rf, rdone, rcounts = run((2, 1, 0))
    for k, i in enumerate((2, 1, 0)):
        a, b = slice(rows[3][i], rows[3][i + 1]), slice(rrows[3][k], rrows[3][k + 1])
        assert torch.equal(rows[0][a], rrows[0][b]) and torch.equal(rows[2][a], rrows[2][b]) and bool((rrows[1][b] == k).all())
        assert torch.equal(done[0][i], rdone[0][k]) and torch.equal(done[1][i], rdone[1][k]) and torch.equal(counts[i], rcounts[k])
        one = tuple(t[i] for t in bstate)
        srows = ops.tsdf_prior_rows(one, origin=origins[i], voxel=hs[i], weight=w0)
        assert torch.equal(srows[0], rows[0][a]) and torch.equal(srows[2], rows[2][a]) and torch.equal(srows[4], rows[4][i])
        sdone, scounts = ops.tsdf_complete(one, f[a].contiguous(), srows, s=s[i], trunc=tr[i], weight=w0)
        assert torch.equal(sdone[0], done[0][i]) and torch.equal(sdone[1], done[1][i]) and torch.equal(scounts, counts[i])
    assert all(_unchanged(tuple(t[p] for t in bstate), sts[p]) for p in range(3))


def test_a_state_without_a_row_is_copied():
    dims, w0 = (3, 5, 7), 3
    sts, origin, h, trunc = edge_case(dims, w0)
    sat = sts[1]
    for state, single in ((tuple(_d(t) for t in sat), True), (tuple(_d(np.stack([t, t])) for t in sat), False)):
        rows = (ops.tsdf_prior_rows if single else ops.tsdf_prior_rows_batch)(state, origin=origin, voxel=h, weight=w0, packed=True)
        assert rows[0].shape == (0, 3) and rows[1].shape == (0,) and rows[2].shape == (0,) and set(rows[3]) == {0}
        done, counts = (ops.tsdf_complete if single else ops.tsdf_complete_batch)(state, torch.empty(0, device=_dev()), rows, s=1.0, trunc=trunc, weight=w0)
        assert torch.equal(done[0], state[0]) and torch.equal(done[1], state[1]) and done[0].data_ptr() != state[0].data_ptr()
        assert _np(counts).reshape(-1, 4).tolist() == [[0, 0, 0, 105]] * (1 if single else 2)
        assert _unchanged(tuple(t if single else t[0] for t in state), sat)
        with pytest.raises(ValueError, match="values"):
            (ops.tsdf_complete if single else ops.tsdf_complete_batch)(state, torch.zeros(3, device=_dev()), rows, s=1.0, trunc=trunc, weight=w0)
    for bad in (0, 65536, 1.5, None):
        with pytest.raises(ValueError, match="weight"):
            ops.tsdf_prior_rows(tuple(_d(t) for t in sat), origin=origin, voxel=h, weight=bad)
    state = tuple(_d(t) for t in sts[2])
    rows = ops.tsdf_prior_rows(state, origin=origin, voxel=h, weight=w0)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="s is"):
            ops.tsdf_complete(state, torch.zeros(rows[3][1], device=_dev()), rows, s=bad, trunc=trunc, weight=w0)
    with pytest.raises(ValueError, match="trunc"):
        ops.tsdf_complete(state, torch.zeros(rows[3][1], device=_dev()), rows, s=1.0, trunc=0.0, weight=w0)


def _complete_sphere(w0, s=1.3):
    host, origin, h, trunc, centre, depth, K, E = sphere_case()
    state = tuple(_d(t) for t in host)
    rows = ops.tsdf_prior_rows(state, origin=origin, voxel=h, weight=w0)
    p = rows[0].double()
    f = ((((p - _d(centre)[None, :]) ** 2).sum(1).sqrt() - 0.3) / s).float()      # the analytic field at the emitted rows, on the device
    done, counts = ops.tsdf_complete(state, f, rows, s=s, trunc=trunc, weight=w0)
    return host, state, rows, f, done, counts


def test_downstream_mesh_and_raycast_read_the_completed_state():
    """ops.tsdf_mesh of the completed state with min_obs = weight equals the twin's mesh of the twin's state; ops.tsdf_raycast on it has
    no UNSEEN pixel (every sample holds `weight` votes), while the observed state has some from the same cameras"""
    w0 = 2
    host, origin, h, trunc, centre, depth, K, E = sphere_case()
    _, state, rows, f, done, counts = _complete_sphere(w0)
    want_state, want_counts = tpo.vote(host, _np(f), 1.3, trunc, w0)
    assert np.array_equal(_np(done[0]), want_state[0]) and np.array_equal(_np(done[1]), want_state[1]) and np.array_equal(_np(counts), want_counts)
    v, fc, _ = ops.tsdf_mesh(done, origin=origin, voxel=h, min_obs=w0)
    wv, wf = fo.mesh(want_state, origin, h, w0)
    assert np.array_equal(_np(v).view(np.uint64), wv.view(np.uint64)) and np.array_equal(_np(fc), wf) and len(wf) > 100
    rng = np.random.default_rng(11)
    Ew = np.stack([_look_at(_rot(rng)) for _ in range(3)])                        # world -> camera around the sphere's centre, from any side
    Ew[:, :, 3] -= Ew[:, :, :3] @ centre
    c2w = np.stack([np.concatenate([e[:, :3].T, (-e[:, :3].T @ e[:, 3])[:, None]], 1) for e in Ew])
    Kr = _d(np.array([60.0, 60.0, 16.0, 16.0]))
    _, _, st_done, cnt = ops.tsdf_raycast(done, _d(c2w), Kr, 32, 32, origin=origin, voxel=h, trunc=trunc, min_obs=w0)
    _, _, st_obs, _ = ops.tsdf_raycast(state, _d(c2w), Kr, 32, 32, origin=origin, voxel=h, trunc=trunc, min_obs=1)
    unseen, hit = ops.RAY_STATE.index("unseen"), ops.RAY_STATE.index("hit")
    print("raycast states completed", _np(cnt).tolist(), "observed unseen", int((st_obs == unseen).sum()))
    assert int((st_done == unseen).sum()) == 0 and int((st_done == hit).sum()) > 100 and int((st_obs == unseen).sum()) > 0
    assert _unchanged(state, host)


def test_the_field_closes_the_shell_the_cameras_left_open():
    """r = 0.3 in 24^3, trunc 3 h, 2 views, weight 2, f the analytic distance / s evaluated on the device at the emitted rows.  The
    observed mesh has boundary edges; the completed mesh has none: every edge is shared by exactly two faces.  A vertex flagged
    vertex_observed around which every sample that a cube naming it reads has n >= 2 (least_seen_around) -- so none of them received
    a vote -- is a vertex of the observed mesh, bit for bit."""
    from livingscenes_amd.lib_more.more_solver import More_Solver
    w0 = 2
    host, state, rows, f, done, counts = _complete_sphere(w0)
    _, origin, h, trunc, centre, *_ = sphere_case()
    vo, fo_, _ = ops.tsdf_mesh(state, origin=origin, voxel=h, min_obs=1)
    open_edges, many = boundary_edges(_np(fo_))
    assert open_edges > 0 and many == 0
    fusion = {"sum": state[0][None], "n": state[1][None], "origin": origin[None], "voxel": np.array([h]), "trunc": np.array([trunc])}
    completed = {"sum": done[0][None].contiguous(), "n": done[1][None].contiguous(), "origin": origin[None], "voxel": np.array([h]),
                 "trunc": np.array([trunc]), "weight": w0}
    (mesh,) = More_Solver._completed_mesh_batch(fusion, completed)
    assert boundary_edges(mesh["faces"]) == (0, 0) and mesh["faces"].max() < len(mesh["vertices"])
    flag = mesh["vertex_observed"]
    assert flag.dtype == np.bool_ and flag.shape == (len(mesh["vertices"]),) and 0 < flag.sum() < len(flag)
    solid = least_seen_around(host[1], mesh["vertices"], origin, h) >= w0
    check = flag & solid
    assert flag[solid].all()                                                    # n >= 2 all around: its cell was seen
    seen = {r.tobytes() for r in _np(vo)}
    print("vertices", len(flag), "observed", int(flag.sum()), "held to the observed mesh", int(check.sum()), "open edges before", open_edges)
    assert check.sum() > 50 and all(r.tobytes() in seen for r in mesh["vertices"][check])
    err = np.abs(np.linalg.norm(mesh["vertices"] - centre, axis=1) - 0.3)
    assert err.max() < h and _unchanged(state, host)


def test_complete_fusion_batch_with_the_decoder(small_prior):
    """More_Solver._complete_fusion_batch, P = 2 at 12^3, the synthetic weights of the sibling tests: the completed state equals the twin
    fed with the device's own decoder values, and those values lie within the project's 1e-4 max-norm bar of the CPU oracle decoder on
    the same rows"""
    from oracle import net
    from test_tsdf_fit_cpu import loop_start
    names = (("sphere", (9, 8, 7)), ("box", (9, 8, 7)))
    start, dcfg, dw = loop_start(names)
    solver = _solver(small_prior)
    w0, dims = 3, (12, 12, 12)
    h = 0.09
    centre = np.array([0.1875, -0.3125, 1.0])
    origin = np.stack([centre - h * 5.5, centre - h * 5.5 + 0.01])
    rng = np.random.default_rng(2)
    sts = []
    for p in range(2):
        N = rng.choice([0, 1, 2, 3, 4], size=dims).astype(np.int32)
        sts.append(((N * rng.integers(-16384, 16385, size=dims)).astype(np.int32), N))
    fusion = {"sum": _d(np.stack([s[0] for s in sts])), "n": _d(np.stack([s[1] for s in sts])), "origin": origin, "voxel": np.array([h, h]),
              "trunc": np.array([3 * h, 2 * h])}
    code = {k: v.clone().to(_dev()) for k, v in start.items()}
    seen = {}
    real = small_prior.hip_model().sdf_decode_rows

    def spy(*a, **k):
        seen["values"] = real(*a, **k)
        seen["points"], seen["inst"] = a[0], a[1]
        return seen["values"]

    hip = small_prior.hip_model()
    hip.sdf_decode_rows = spy
    try:
        out = solver._complete_fusion_batch(fusion, code, weight=w0, max_rows=1000)      # several decoder launches
    finally:
        del hip.sdf_decode_rows
    want_rows = tpo.rows_batch(sts, origin, [h, h], w0)
    assert np.array_equal(_np(seen["points"]).view(np.uint32), want_rows["points"].view(np.uint32)) and np.array_equal(_np(seen["inst"]), want_rows["row_inst"])
    values = _np(seen["values"])
    s = start["s"].reshape(-1).numpy().astype(np.float64)
    wstates, wc = tpo.vote_batch(sts, values, want_rows["offsets"], s, fusion["trunc"], w0)
    for p in range(2):
        assert np.array_equal(_np(out["sum"][p]), wstates[p][0]) and np.array_equal(_np(out["n"][p]), wstates[p][1]), p
    assert np.array_equal(_np(out["counts"]), wc) and out["weight"] == w0 and out["rows"] == want_rows["offsets"][2] > 1000
    assert out["origin"] is not None and np.array_equal(out["trunc"], fusion["trunc"]) and set(out) == {"sum", "n", "origin", "voxel", "trunc", "weight", "counts", "rows"}
    worst = 0.0
    for p in range(2):
        lo, hi = want_rows["offsets"][p], want_rows["offsets"][p + 1]
        one = {k: v[p:p + 1] for k, v in start.items()}
        ref = net.field_query(dw, dcfg, torch.from_numpy(want_rows["points"][lo:hi])[None], one).reshape(-1).numpy()
        worst = max(worst, float(np.abs(values[lo:hi] - ref).max()))
    print("decoder values against the CPU oracle: max abs", worst)
    assert worst <= 1e-4
    assert _unchanged((fusion["sum"][0], fusion["n"][0]), sts[0]) and _unchanged((fusion["sum"][1], fusion["n"][1]), sts[1])
    one = solver._complete_fusion_batch(fusion, {k: v[1:2] for k, v in code.items()}, slots=[1], weight=w0)
    assert torch.equal(one["sum"][0], out["sum"][1]) and torch.equal(one["n"][0], out["n"][1]) and torch.equal(one["counts"][0], out["counts"][1])
    with pytest.raises(ValueError, match="slots"):
        solver._complete_fusion_batch(fusion, code, slots=[0], weight=w0)
    with pytest.raises(TypeError):
        solver._complete_fusion_batch(fusion, code)


def test_solve_sequence_completed(small_prior):
    """the synthetic two-rescan scene of the fusion tests: memory['completed'] equals a by-hand _complete_fusion_batch on the returned
    fusion and codes, completed_meshes has one entry per slot; solve_sequence with the same kw returns the same steps and the same other
    memory entries, bit for bit; the ValueErrors come before any device work"""
    from livingscenes_amd.lib_more import more_solver
    solver = _solver(small_prior)
    n, w0 = 3, 2
    views, ref, rescans = _fusion_scene(n, rescans=2)
    kw = dict(voxel=0.02, fuse_res=16, fuse_empty="free")
    scene = lambda: (dict(_scene(ref), views=views), [dict(_scene(r), views=views) for r in rescans])   # noqa: E731
    steps, memory = more_solver.solve_sequence_completed(solver, *scene(), complete_weight=w0, **kw)
    psteps, plain = more_solver.solve_sequence(solver, *scene(), **kw)
    assert set(memory) == set(plain) | {"completed", "completed_meshes"} and len(steps) == len(psteps) == 2
    for i in range(n):
        assert torch.equal(memory["clouds"][i], plain["clouds"][i])
    for k in CODE_KEYS:
        assert torch.equal(memory["codes"][k], plain["codes"][k]), k
    for k in ("sum", "n"):
        assert torch.equal(memory["fusion"][k], plain["fusion"][k]), k
    for a, b in zip(steps, psteps):
        assert set(a) == set(b) and a["merged_sizes"] == b["merged_sizes"] and torch.equal(a["matches"], b["matches"])
        for x, y in zip(a["registration"], b["registration"]):
            assert (x is None and y is None) or torch.equal(x, y)
        for x, y in zip(a["codes"], b["codes"]):
            assert (x is None and y is None) or all(torch.equal(x[k], y[k]) for k in CODE_KEYS)
        assert a["n_fused_views"] == b["n_fused_views"] and a["n_new_points"] == b["n_new_points"]
    hand = solver._complete_fusion_batch(memory["fusion"], memory["codes"], weight=w0)
    done = memory["completed"]
    assert torch.equal(done["sum"], hand["sum"]) and torch.equal(done["n"], hand["n"]) and torch.equal(done["counts"], hand["counts"])
    assert done["weight"] == w0 and done["sum"].shape == memory["fusion"]["sum"].shape and bool((done["n"] >= w0).all())
    cnt = _np(done["counts"])
    assert (cnt[:, 0] > 0).all() and (cnt[:, 3] > 0).all() and (cnt.sum(1) - cnt[:, 0] == 16 ** 3).all() and (cnt[:, 1] + cnt[:, 2] == cnt[:, 0]).all()
    meshes = memory["completed_meshes"]
    assert len(meshes) == n
    for m in meshes:
        assert m is None or (set(m) == {"vertices", "faces", "vertex_observed"} and len(m["vertex_observed"]) == len(m["vertices"]))
    _, no_mesh = more_solver.solve_sequence_completed(solver, *scene(), complete_weight=w0, complete_mesh=False, **kw)
    assert no_mesh["completed_meshes"] is None and torch.equal(no_mesh["completed"]["sum"], done["sum"])
    with pytest.raises(ValueError, match="fuse_res"):
        more_solver.solve_sequence_completed(None, None, [], complete_weight=w0, voxel=0.02)
    with pytest.raises(ValueError, match="weight"):
        more_solver.solve_sequence_completed(None, None, [], complete_weight=0, **kw)
