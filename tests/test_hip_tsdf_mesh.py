"""GPU tests of the scene memory's mesh of a fused state (csrc/tsdfmesh.hip) and of the layers on top (ops.tsdf_mesh / tsdf_mesh_batch,
More_Solver._observed_mesh_batch, solve_sequence(fuse_mesh=True)).  The arithmetic is float64 written without contraction and the
numbering is integer, so every comparison with the NumPy twin (tests/fuse_oracle.py: mesh, tests/tsdf_mesh_oracle.py) is by equality.
EVERY comparison is made on host copies, and no device tensor is ever indexed with a face array the operator returned: where the test
calls the C ABI itself the outputs are pre-filled (faces -1, vertices NaN) and the first assertions are that no sentinel is left below
the counts and that 0 <= face < nv, so an array the kernels did not write is a failing assertion and nothing else.  The states, the
size edges and the expected meshes are those of tests/test_tsdf_mesh_cpu.py."""
import ctypes

import numpy as np
import pytest
import torch

import fuse_oracle as fo
import tsdf_mesh_oracle as tmo
from cloud_testlib import _dev, _scene, _solver, small_prior  # noqa: F401 (small_prior is a fixture)
from test_depth_fuse_cpu import _look_at, _rot, _sphere_depth, sphere_state
from test_hip_depth_fuse import _fusion_scene, _part_views
from test_tsdf_mesh_cpu import EDGE_DIMS, ORIGIN, PER_BLOCK, VOXEL, expected, state_of

pytestmark = pytest.mark.gpu
TAIL = 5                              # rows behind the capacity that must stay as they were


def _d(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x)).to(_dev(), dtype)


def _raw(S, N, origin, voxel, min_obs, single, short_v=0, short_f=0):
    """the C entry called directly on host arrays S, N [P,nx,ny,nz]: a sizing call, then the real call into pre-filled outputs with
    capacities the full counts minus short_* -> host copies (vertices with TAIL rows behind the total, faces likewise, the offsets of the
    sizing call and of the real call [2,P+1], stats [P,3])"""
    from livingscenes_amd import _lib
    lib, dev = _lib.load(), _dev()
    P, dims = S.shape[0], S.shape[1:]
    Sd, Nd = _d(S, torch.int32), _d(N, torch.int32)
    o = np.ascontiguousarray(np.broadcast_to(np.asarray(origin, np.float64), (P, 3)))
    h = np.ascontiguousarray(np.broadcast_to(np.asarray(voxel, np.float64), (P,)))
    need = lib.ls_tsdf_mesh_workspace_bytes(*dims) if single else lib.ls_tsdf_mesh_batch_workspace_bytes(P, *dims)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    off0 = torch.full((2, P + 1), -7, dtype=torch.int64, device=dev)
    off1 = torch.full((2, P + 1), -7, dtype=torch.int64, device=dev)
    stats = torch.full((P, 3), -7, dtype=torch.int64, device=dev)
    st = _lib.stream_ptr(dev)

    def call(V, cap_v, F, cap_f, off, stats):
        tail = (V, cap_v, F, cap_f, _lib.ptr(off), stats, _lib.ptr(ws), need, st)
        if single:
            assert P == 1
            _lib.call(dev, "ls_tsdf_mesh_f64", _lib.ptr(Sd), _lib.ptr(Nd), *dims, min_obs, ctypes.c_void_p(o.ctypes.data), float(h[0]), *tail)
        else:
            _lib.call(dev, "ls_tsdf_mesh_batch_f64", P, _lib.ptr(Sd), _lib.ptr(Nd), *dims, min_obs, ctypes.c_void_p(o.ctypes.data),
                      ctypes.c_void_p(h.ctypes.data), *tail)
    call(None, 0, None, 0, off0, None)
    off0 = off0.cpu().numpy()
    assert (off0 >= 0).all(), "the sizing call left the offsets unwritten"
    nv, nf = int(off0[0, P]), int(off0[1, P])
    V = torch.full((nv + TAIL, 3), float("nan"), dtype=torch.float64, device=dev)
    F = torch.full((nf + TAIL, 3), -1, dtype=torch.int64, device=dev)
    call(_lib.ptr(V), max(nv - short_v, 0), _lib.ptr(F), max(nf - short_f, 0), off1, _lib.ptr(stats))
    torch.cuda.synchronize(dev)
    return V.cpu().numpy(), F.cpu().numpy(), off0, off1.cpu().numpy(), stats.cpu().numpy()


def _meshes(V, F, off, short_v=0, short_f=0):
    """FIRST the sentinels and the ranges, on the host; then the meshes of the packed outputs as host arrays"""
    P = off.shape[1] - 1
    nv, nf = int(off[0, P]), int(off[1, P])
    assert V.shape[0] == nv + TAIL and F.shape[0] == nf + TAIL
    wv, wf = max(nv - short_v, 0), max(nf - short_f, 0)
    assert np.isnan(V[wv:]).all() and (F[wf:] == -1).all(), "something was written at or past the capacity"
    assert not np.isnan(V[:wv]).any(), "a vertex below the count was not written"
    assert (F[:wf] != -1).all(), "a face below the count was not written"
    assert (np.diff(off[0]) >= 0).all() and (np.diff(off[1]) >= 0).all() and off[0, 0] == 0 and off[1, 0] == 0
    out = []
    for p in range(P):
        v, f = V[off[0, p]:min(off[0, p + 1], wv)], F[off[1, p]:min(off[1, p + 1], wf)]
        assert (f >= 0).all() and (f < max(off[0, p + 1] - off[0, p], 1)).all() and (len(f) == 0 or off[0, p + 1] > off[0, p]), p
        out.append((v, f))
    return out


def _equal(got, want):
    (gv, gf), (wv, wf) = got, want[:2]
    assert gv.shape == wv.shape and gf.shape == wf.shape, (gv.shape, wv.shape, gf.shape, wf.shape)
    assert np.array_equal(gf, wf)
    assert np.array_equal(gv.view(np.int64), wv.view(np.int64))              # bitwise


def test_the_states_cover_what_they_are_chosen_for():
    for dims in ((20, 21, 22), (17, 17, 17)):
        a = tmo.analyse(state_of(dims), 1)
        assert len(np.unique(a["cfg"][a["kept"]])) == 256                     # all 256 patterns occur in kept cubes
        assert 0 < a["carried"].sum() < a["creates"].sum()                    # carried < created
        assert len(expected(dims, 1)[1]) > 0                                  # faces > 0
    cubes = [int(np.prod([d - 1 for d in dims])) for dims in EDGE_DIMS]
    assert cubes[:7] == [1, 63, 64, 65, PER_BLOCK - 1, PER_BLOCK, PER_BLOCK + 1]


# ------------------------------------------------------------------------------------------------ the operator against the twin
@pytest.mark.parametrize("min_obs", (1, 2))
@pytest.mark.parametrize("dims", EDGE_DIMS)
def test_mesh_equals_the_twin_at_the_size_edges(dims, min_obs):
    """one cube; 63 / 64 / 65 cubes; one short of, exactly and one over the 4096 cubes of a workgroup of the count pass; unequal dims"""
    from livingscenes_amd import ops
    S, N = state_of(dims)
    want = expected(dims, min_obs)
    V, F, off0, off1, stats = _raw(S[None], N[None], ORIGIN, VOXEL, min_obs, single=True)
    (got,) = _meshes(V, F, off1)
    assert np.array_equal(off0, off1) and off1.tolist() == [[0, len(want[0])], [0, len(want[1])]]
    _equal(got, want)
    assert np.array_equal(stats[0], want[2])
    # the binding: the same arrays, read on the host
    v, f, counts = ops.tsdf_mesh((_d(S, torch.int32), _d(N, torch.int32)), origin=ORIGIN, voxel=VOXEL, min_obs=min_obs)
    assert v.dtype == torch.float64 and f.dtype == torch.int64 and v.shape == (len(want[0]), 3) and f.shape == (len(want[1]), 3)
    _equal((v.cpu().numpy(), f.cpu().numpy()), want)
    assert counts.cpu().tolist() == want[2].tolist()


def test_batch_with_an_empty_mesh_in_the_middle():
    """P = 3, two workgroups of the count pass per problem; problem 1 was never observed; every problem has its own origin and voxel.
    Every mesh is the twin's and bit-identical to the single call; the batch of one is the single call."""
    from livingscenes_amd import ops
    dims = (20, 21, 22)
    states = [state_of(dims, 0), tuple(np.zeros_like(t) for t in state_of(dims, 0)), state_of(dims, 1)]
    S, N = (np.stack([s[k] for s in states]) for k in (0, 1))
    origins = np.array([ORIGIN, [5.0, -3.0, 0.25], [-0.5, -0.5, -0.5]])
    voxels = np.array([VOXEL, 1.0, 1.0 / 39])
    wants = [tmo.mesh(s, origins[p], voxels[p], 1) for p, s in enumerate(states)]
    assert len(wants[1][1]) == 0 and len(wants[0][1]) > 0 and len(wants[2][1]) > 0 and len(wants[2][0]) != len(wants[0][0])
    V, F, off0, off1, stats = _raw(S, N, origins, voxels, 1, single=False)
    got = _meshes(V, F, off1)
    assert np.array_equal(off0, off1)
    assert off1[0].tolist() == np.concatenate([[0], np.cumsum([len(w[0]) for w in wants])]).tolist()
    assert off1[1].tolist() == np.concatenate([[0], np.cumsum([len(w[1]) for w in wants])]).tolist()
    for p in range(3):
        _equal(got[p], wants[p])
        assert np.array_equal(stats[p], tmo.analyse(states[p], 1)["stats"])
        for single in (True, False):                                          # the single entry, and the batch of one
            V1, F1, _, o1, s1 = _raw(S[p:p + 1], N[p:p + 1], origins[p], voxels[p], 1, single=single)
            (one,) = _meshes(V1, F1, o1)
            _equal(one, got[p])
            assert np.array_equal(s1[0], stats[p])
    # the binding: views of the packed outputs, one host read; the packed form
    state = (_d(S, torch.int32), _d(N, torch.int32))
    meshes, counts = ops.tsdf_mesh_batch(state, origin=origins, voxel=voxels)
    assert len(meshes) == 3 and counts.cpu().numpy().tolist() == stats.tolist()
    for p, (v, f) in enumerate(meshes):
        _equal((v.cpu().numpy(), f.cpu().numpy()), wants[p])
    pv, pf, vo, fo_, _ = ops.tsdf_mesh_batch(state, origin=origins, voxel=voxels, packed=True)
    assert vo == off1[0].tolist() and fo_ == off1[1].tolist() and pv.shape == (vo[3], 3) and pf.shape == (fo_[3], 3)
    assert meshes[2][0].data_ptr() != pv.data_ptr() and meshes[0][0].shape[0] == vo[1]
    # min_obs = 2 through the batch: the sparse meshes
    meshes, _ = ops.tsdf_mesh_batch(state, origin=origins, voxel=voxels, min_obs=2)
    for p, (v, f) in enumerate(meshes):
        _equal((v.cpu().numpy(), f.cpu().numpy()), tmo.mesh(states[p], origins[p], voxels[p], 2))


def test_sizing_call_and_short_capacities():
    dims = (17, 17, 17)
    S, N = state_of(dims)
    want = expected(dims, 1)
    for short_v, short_f in ((0, 1), (1, 0), (3, 2)):
        V, F, off0, off1, _ = _raw(S[None], N[None], ORIGIN, VOXEL, 1, single=False, short_v=short_v, short_f=short_f)
        assert np.array_equal(off0, off1) and off1.tolist() == [[0, len(want[0])], [0, len(want[1])]]     # always the full counts
        (got,) = _meshes(V, F, off1, short_v, short_f)                        # the last face's / vertex's sentinel is untouched
        assert np.array_equal(got[0].view(np.int64), want[0][:len(want[0]) - short_v].view(np.int64))
        assert np.array_equal(got[1], want[1][:len(want[1]) - short_f])


def test_no_cube_and_nothing_kept():
    from livingscenes_amd import ops
    S, N = state_of((5, 7, 11))
    for sl in ((slice(0, 1), slice(None), slice(None)), (slice(None), slice(2, 3), slice(None)), (slice(None), slice(None), slice(10, 11))):
        s, n = np.ascontiguousarray(S[sl]), np.ascontiguousarray(N[sl])
        V, F, off0, off1, stats = _raw(s[None], n[None], ORIGIN, VOXEL, 1, single=True)
        assert not off0.any() and not off1.any() and V.shape == (TAIL, 3) and np.isnan(V).all() and (F == -1).all()
        assert stats[0].tolist() == [0, 0, int((n >= 1).sum())]
    v, f, counts = ops.tsdf_mesh((_d(S, torch.int32), _d(N, torch.int32)), origin=ORIGIN, voxel=VOXEL, min_obs=4)      # no sample is valid
    assert v.shape == (0, 3) and f.shape == (0, 3) and counts.cpu().tolist() == [0, 0, 0]
    with pytest.raises(ValueError, match="min_obs must be >= 1"):
        ops.tsdf_mesh((_d(S, torch.int32), _d(N, torch.int32)), origin=ORIGIN, voxel=VOXEL, min_obs=0)
    with pytest.raises(Exception, match="voxel must be finite and > 0"):
        ops.tsdf_mesh((_d(S, torch.int32), _d(N, torch.int32)), origin=ORIGIN, voxel=0.0)
    with pytest.raises(Exception, match="int32 HIP"):
        ops.tsdf_mesh((torch.from_numpy(S), torch.from_numpy(N)), origin=ORIGIN, voxel=VOXEL)


# ------------------------------------------------------------------------------------------------ end to end
def test_fused_sphere_to_mesh_equals_the_twin_chain():
    """ops.depth_fuse of the 4-view analytic sphere at res 18, then ops.tsdf_mesh, against fuse_oracle.fuse -> fuse_oracle.mesh"""
    from livingscenes_amd import ops
    res, r = 18, 0.4
    (S, N), origin, h = sphere_state(4, res, r)
    rng = np.random.default_rng(0)
    _rot(rng)
    K = np.array([100.0, 100.0, 50.0, 50.0])
    E = np.stack([_look_at(_rot(rng)) for _ in range(4)])
    depth = np.stack([_sphere_depth(e, K, 100, 100, r) for e in E])
    state = ops.tsdf_state(1, (res,) * 3, _dev())
    state = (state[0][0], state[1][0])
    ops.depth_fuse(state, _d(depth, torch.float32), _d(np.tile(K, (4, 1)), torch.float64), _d(E, torch.float64), origin=origin, voxel=h, trunc=4 * h)
    assert np.array_equal(state[0].cpu().numpy(), S) and np.array_equal(state[1].cpu().numpy(), N)
    v, f, counts = ops.tsdf_mesh(state, origin=origin, voxel=h)
    v, f = v.cpu().numpy(), f.cpu().numpy()
    wv, wf = fo.mesh((S, N), origin, h)
    assert (len(wf), len(wv)) == (1148, 728)
    assert f.shape == wf.shape and (f >= 0).all() and (f < len(wv)).all()
    _equal((v, f), (wv, wf))
    assert np.abs(np.linalg.norm(v, axis=1) - r).max() <= np.sqrt(3) * h
    assert counts.cpu().tolist() == tmo.analyse((S, N), 1)["stats"].tolist()


def test_observed_mesh_batch_returns_none_for_an_empty_mesh():
    from livingscenes_amd.lib_more.more_solver import More_Solver
    dims = (5, 7, 11)
    states = [state_of(dims, 0), tuple(np.zeros_like(t) for t in state_of(dims, 0)), state_of(dims, 1)]
    origins, voxels = np.array([ORIGIN, ORIGIN + 1.0, ORIGIN - 2.0]), np.array([VOXEL, 0.5, 0.02])
    fusion = dict(sum=_d(np.stack([s[0] for s in states]), torch.int32), n=_d(np.stack([s[1] for s in states]), torch.int32),
                  origin=torch.from_numpy(origins), voxel=torch.from_numpy(voxels))
    for min_obs in (1, 2):
        got = More_Solver._observed_mesh_batch(fusion, min_obs)
        assert len(got) == 3 and got[1] is None
        for p in (0, 2):
            _equal((np.asarray(got[p].vertices, np.float64), np.asarray(got[p].faces, np.int64)), tmo.mesh(states[p], origins[p], voxels[p], min_obs))


def test_solve_sequence_meshes_the_fused_state_once(small_prior, monkeypatch):
    """fuse_mesh=True: memory['observed_meshes'] is ops.tsdf_mesh_batch(memory['fusion']) replayed by hand, made in ONE call after the
    last step; fuse_mesh=False: the memory's keys are what they were"""
    from livingscenes_amd import ops
    from livingscenes_amd.lib_more import more_solver
    solver = _solver(small_prior)
    parts, ref, rescan = _fusion_scene(3)
    views = [_part_views(p) for p in parts]
    calls = []

    def spy(fusion, min_obs=1, _real=solver._observed_mesh_batch):
        calls.append(min_obs)
        return _real(fusion, min_obs)
    monkeypatch.setattr(solver, "_observed_mesh_batch", spy)
    args = (solver, dict(_scene(ref), views=views), [dict(_scene(rescan), views=views)])
    _, off = more_solver.solve_sequence(*args, voxel=0.02, fuse_res=16)
    assert set(off) == {"clouds", "codes", "meshes", "fusion"} and not calls
    _, memory = more_solver.solve_sequence(*args, voxel=0.02, fuse_res=16, fuse_mesh=True, fuse_min_obs=2)
    monkeypatch.undo()
    assert set(memory) == set(off) | {"observed_meshes"} and calls == [2]
    fusion, got = memory["fusion"], memory["observed_meshes"]
    assert torch.equal(fusion["sum"], off["fusion"]["sum"]) and torch.equal(fusion["n"], off["fusion"]["n"])      # meshing changes nothing
    meshes, _ = ops.tsdf_mesh_batch((fusion["sum"], fusion["n"]), origin=fusion["origin"], voxel=fusion["voxel"], min_obs=2)
    S, N = fusion["sum"].cpu().numpy(), fusion["n"].cpu().numpy()
    assert len(got) == 3 and any(g is not None for g in got)
    for p in range(3):
        v, f = meshes[p][0].cpu().numpy(), meshes[p][1].cpu().numpy()
        assert (f >= 0).all() and (f < max(len(v), 1)).all()
        _equal((v, f), tmo.mesh((S[p], N[p]), fusion["origin"][p].numpy(), float(fusion["voxel"][p]), 2))
        assert (got[p] is None) == (len(f) == 0)
        if got[p] is not None:
            _equal((np.asarray(got[p].vertices, np.float64), np.asarray(got[p].faces, np.int64)), (v, f))
    with pytest.raises(ValueError, match="fuse_mesh needs fuse_res"):
        more_solver.solve_sequence(*args, voxel=0.02, fuse_mesh=True)
