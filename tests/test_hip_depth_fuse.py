"""GPU tests of the scene memory's depth fusion (csrc/depthfuse.hip) and of the layers on top (ops.depth_fuse / tsdf_volume,
More_Solver._fuse_batch, solve_sequence(fuse_res=...)).  The update is integer and the rest is
float64 written without contraction, so every comparison with the NumPy twin (tests/fuse_oracle.py) is by equality.  The generators and
the size-edge problems are those of tests/test_depth_fuse_cpu.py, where the twin shows that they reach every class."""
import numpy as np
import pytest
import torch

import fuse_oracle as fo
from cloud_testlib import CODE_KEYS, F, _dev, _pose, _scene, _solver, small_prior  # noqa: F401 (small_prior is a fixture)
from livingscenes_amd import synth
from test_depth_fuse_cpu import EYE, GPU_DIMS, fuse_problem, gpu_cases, run_twin

pytestmark = pytest.mark.gpu


def _d(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x)).to(_dev(), dtype)


def _views(pr):
    return _d(pr["depth"], torch.float32), _d(pr["K"], torch.float64), _d(pr["E"], torch.float64)


def _grid(pr):
    return dict(origin=pr["origin"], voxel=pr["voxel"], trunc=pr["trunc"])


def _state(dims, P=None, like=None):
    """a fresh device state, or the device copy of a twin state"""
    from livingscenes_amd import ops
    if like is not None:
        return tuple(_d(a, torch.int32) for a in like)
    S, N = ops.tsdf_state(1 if P is None else P, dims, _dev())
    return (S[0], N[0]) if P is None else (S, N)


def _same(state, want):
    return all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(state, want))


def _fuse(dims, pr, empty="unknown", state=None):
    from livingscenes_amd import ops
    state = _state(dims) if state is None else state
    vc = ops.depth_fuse(state, *_views(pr), empty=empty, **_grid(pr))
    return state, vc.cpu().numpy()


# ------------------------------------------------------------------------------------------------ the operator against the twin
@pytest.mark.parametrize("dims", GPU_DIMS)
def test_fuse_size_edges(dims):
    """voxel counts where a wave of 64 or a chunk of 256 is full, one short and one over; 0, 1 and 3 views; four image sizes; both modes"""
    for V, (H, W), pr in gpu_cases(dims):
        for empty in ("unknown", "free"):
            want, wc = run_twin(dims, pr, empty)
            got, vc = _fuse(dims, pr, empty)
            assert _same(got, want) and vc.shape == (V, 6) and np.array_equal(vc, wc), (dims, V, H, W, empty)
            assert (vc.sum(1) == np.prod(dims)).all()


def test_fuse_hand_cases():
    one = np.ones((1, 5, 5), F)
    hole = one.copy()
    hole[0, 2, 2] = 0.0
    K = np.array([[4.0, 4.0, 2.0, 2.0]])
    for x, img, empty, want in (((0, 0, 0.90), one, "unknown", (fo.FREE, 16384, 1)), ((0, 0, 0.99), one, "unknown", (fo.NEAR, 4096, 1)),
                                ((0, 0, 1.00), one, "free", (fo.NEAR, 0, 1)), ((0, 0, 1.03), one, "unknown", (fo.NEAR, -12288, 1)),
                                ((0, 0, 1.05), one, "unknown", (fo.OCCLUDED, 0, 0)), ((0, 0, 0.04), one, "unknown", (fo.OUT, 0, 0)),
                                ((1.0, 0, 1.0), one, "unknown", (fo.OUT, 0, 0)), ((0.625, 0, 1.0), one, "unknown", (fo.OUT, 0, 0)),
                                ((-0.625, 0, 1.0), one, "unknown", (fo.NEAR, 0, 1)), ((0, 0, 0.99), hole, "unknown", (fo.EMPTY, 0, 0)), ((0, 0, 0.99), hole, "free", (fo.FREE, 16384, 1))):
        pr = dict(origin=np.array(x, np.float64), voxel=1.0, trunc=0.04, depth=img, K=K, E=EYE[None])
        (S, N), vc = _fuse((1, 1, 1), pr, empty)
        assert (int(np.flatnonzero(vc[0])[0]), int(S[0, 0, 0]), int(N[0, 0, 0])) == want and vc.sum() == 1, (x, empty)
    for bad in (float("nan"), float("inf")):                               # a camera-frame position that is not finite (the origin itself is refused)
        E = EYE[None].copy()
        E[0, 0, 3] = bad
        (S, N), vc = _fuse((1, 1, 1), dict(origin=np.array([0, 0, 1.0]), voxel=1.0, trunc=0.04, depth=one, K=K, E=E))
        assert vc[0].tolist() == [1, 0, 0, 0, 0, 0] and int(N[0, 0, 0]) == 0 and np.array_equal(vc, run_twin((1, 1, 1), dict(depth=one, K=K, E=E, origin=[0, 0, 1.0],
                                                                                                                      voxel=1.0, trunc=0.04))[1])


def test_fuse_saturation():
    """a state prefilled with n = 65534 and 65535 (and fresh voxels between them), three views: the order of the call decides"""
    dims = (4, 8, 9)
    rng = np.random.Generator(np.random.Philox(key=[7, 1]))
    pr = fuse_problem(rng, dims, 3, 16, 16)
    S0 = rng.integers(-1000, 1000, dims).astype(np.int32)
    N0 = rng.choice([0, 65533, 65534, 65535], dims).astype(np.int32)
    for empty in ("unknown", "free"):
        want = (S0.copy(), N0.copy())
        wc = fo.fuse(want, pr["depth"], pr["K"], pr["E"], pr["origin"], pr["voxel"], pr["trunc"], empty)
        assert wc[:, fo.SATURATED].all() and (wc[0, fo.SATURATED] < wc[2, fo.SATURATED]) and want[1].max() == 65535
        got, vc = _fuse(dims, pr, empty, _state(dims, like=(S0, N0)))
        assert _same(got, want) and np.array_equal(vc, wc), empty


def test_fuse_split_calls_and_order():
    """two calls of 2 + 1 views equal one call of 3, equal the reversed order"""
    dims = (6, 7, 8)
    pr = fuse_problem(np.random.Generator(np.random.Philox(key=[7, 2])), dims, 3, 16, 16)
    part = lambda idx: dict(pr, depth=pr["depth"][idx], K=pr["K"][idx], E=pr["E"][idx])
    for empty in ("unknown", "free"):
        want, wc = run_twin(dims, pr, empty)
        whole, vc = _fuse(dims, pr, empty)
        state = _state(dims)
        _, va = _fuse(dims, part([0, 1]), empty, state)
        _, vb = _fuse(dims, part([2]), empty, state)
        back, vr = _fuse(dims, part([2, 1, 0]), empty)
        assert _same(whole, want) and _same(state, want) and _same(back, want) and want[1].max() == 3
        assert np.array_equal(vc, wc) and np.array_equal(np.concatenate([va, vb]), wc) and np.array_equal(vr, wc[::-1])


def _batch_problems():
    dims = (5, 9, 7)
    rng = np.random.Generator(np.random.Philox(key=[7, 3]))
    return dims, [fuse_problem(rng, dims, V, 16, 16) for V in (3, 0, 1, 0, 2)]


def test_fuse_batch_is_the_single_op_reversed_and_again():
    """five problems, two of them without views: every slice is the single op's bits, and again with the problems reversed"""
    from livingscenes_amd import ops
    dims, probs = _batch_problems()
    for empty in ("unknown", "free"):
        singles = [_fuse(dims, pr, empty) for pr in probs]
        for order in (list(range(5)), list(range(4, -1, -1))):
            ps = [probs[i] for i in order]
            state = _state(dims, P=5)
            assert ps[1]["depth"].shape[0] == 0                            # slot 1 holds a problem WITHOUT views in both orders (1, then 3):
            state[0][1].fill_(11)                                          # its state is not fresh, and the call must leave it as it is
            pre = [t.clone() for t in state]
            views = [None if i == 3 else _views(pr) for i, pr in zip(order, ps)]                    # no views: None, or [0,H,W]
            vcs = ops.depth_fuse_batch(state, [None if v is None else v[0] for v in views], [None if v is None else v[1] for v in views],
                                       [None if v is None else v[2] for v in views], origin=np.stack([pr["origin"] for pr in ps]),
                                       voxel=[pr["voxel"] for pr in ps], trunc=[pr["trunc"] for pr in ps], empty=empty)
            for b, i in enumerate(order):
                (S, N), vc = singles[i]
                if b == 1:                                                 # the single op started from zeros and changed nothing either
                    assert not S.any() and not N.any()
                    S = S + 11
                assert torch.equal(state[0][b], S) and torch.equal(state[1][b], N) and np.array_equal(vcs[b].cpu().numpy(), vc), (empty, order, b)
                if probs[i]["depth"].shape[0] == 0:
                    assert torch.equal(state[0][b], pre[0][b]) and torch.equal(state[1][b], pre[1][b]) and vcs[b].shape == (0, 6)
    none = ops.depth_fuse_batch(_state(dims, P=2), [None, None], [None, None], [None, None], origin=np.zeros((2, 3)), voxel=0.1, trunc=0.4)
    assert [tuple(v.shape) for v in none] == [(0, 6)] * 2


def test_fuse_launch_count_depends_on_nothing():
    """one kernel for one problem with one view, and one for five problems with up to three views"""
    from livingscenes_amd import _lib, ops
    from test_hip_render import _kernel_launches
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=_dev())
    rng = np.random.Generator(np.random.Philox(key=[7, 4]))
    dims = (5, 9, 7)

    def raw(nviews):
        probs = [fuse_problem(rng, dims, V, 16, 16) for V in nviews]
        P, views = len(nviews), sum(nviews)
        S, N = _state(dims, P=P)
        D, K, E = (torch.cat(t) for t in zip(*[_views(pr) for pr in probs]))
        o, h, t = np.stack([pr["origin"] for pr in probs]), np.array([pr["voxel"] for pr in probs]), np.array([pr["trunc"] for pr in probs])
        vo, vc = ops._offsets(nviews), torch.empty(views, 6, dtype=torch.int64, device=_dev())
        torch.cuda.synchronize()
        keep = (o, h, t, vo)                                               # the host arrays live as long as the closure
        return lambda: _lib.call(_dev(), "ls_depth_fuse_batch_f32", P, _lib.ptr(S), _lib.ptr(N), *dims, ops._hptr(keep[0]), ops._hptr(keep[1]),
                                 ops._hptr(keep[2]), _lib.ptr(D), views, ops._hptr(keep[3]), 16, 16, _lib.ptr(K), _lib.ptr(E), 0.05, 0, _lib.ptr(vc),
                                 _lib.ptr(ws), ws.numel(), _lib.stream_ptr(_dev()))
    one, five = _kernel_launches(raw([1])), _kernel_launches(raw([3, 0, 1, 0, 2]))
    assert len(one) == len(five) == 1 and "fuse_kernel" in one[0] and "fuse_kernel" in five[0], (one, five)
    S, N = _state(dims, P=2)
    vol, valid, counts = (torch.empty(2, *dims, dtype=dt, device=_dev()) for dt in (torch.float64, torch.uint8, torch.int64))
    names = _kernel_launches(lambda: _lib.call(_dev(), "ls_tsdf_volume_f64", _lib.ptr(S), _lib.ptr(N), 2, *dims, 1, _lib.ptr(vol), _lib.ptr(valid),
                                               _lib.ptr(counts), _lib.stream_ptr(_dev())))
    assert len(names) == 1 and "volume_kernel" in names[0], names


def test_bindings_refuse_what_the_device_path_cannot_take():
    from livingscenes_amd import _lib, ops
    dims = (4, 4, 4)
    pr = fuse_problem(np.random.Generator(np.random.Philox(key=[7, 5])), dims, 2, 5, 7)
    D, K, E = _views(pr)
    g = _grid(pr)
    ok = _state(dims)
    with pytest.raises(_lib.LsError, match="state sum must be an int32 HIP"):
        ops.depth_fuse((ok[0].cpu(), ok[1]), D, K, E, **g)
    with pytest.raises(_lib.LsError, match="state n must be an int32 HIP"):
        ops.depth_fuse((ok[0], ok[1].long()), D, K, E, **g)
    with pytest.raises(ValueError, match="state sum is"):
        ops.depth_fuse((ok[0][None], ok[1][None]), D, K, E, **g)
    with pytest.raises(ValueError, match="state sum is .* state n"):
        ops.depth_fuse((ok[0], ok[1][:2].contiguous()), D, K, E, **g)
    with pytest.raises(_lib.LsError, match="depth must be an fp32 HIP"):
        ops.depth_fuse(ok, D.cpu(), K, E, **g)
    with pytest.raises(_lib.LsError, match="depth must be an fp32 HIP"):
        ops.depth_fuse(ok, D.double(), K, E, **g)
    with pytest.raises(ValueError, match="intrinsics is"):
        ops.depth_fuse(ok, D, K[:1].expand(3, 4), E, **g)
    with pytest.raises(ValueError, match="world_to_cam is"):
        ops.depth_fuse(ok, D, K, E[:, :, :3], **g)
    with pytest.raises(_lib.LsError, match="world_to_cam must be a HIP"):
        ops.depth_fuse(ok, D, K, E.cpu(), **g)
    with pytest.raises(ValueError, match="origin is"):
        ops.depth_fuse(ok, D, K, E, origin=np.zeros(2), voxel=0.1, trunc=0.4)
    with pytest.raises(ValueError, match="empty must be"):
        ops.depth_fuse(ok, D, K, E, empty="maybe", **g)
    with pytest.raises(_lib.LsError, match="voxel must be finite and > 0"):
        ops.depth_fuse(ok, D, K, E, origin=pr["origin"], voxel=0.0, trunc=0.4)
    with pytest.raises(_lib.LsError, match="problem 1: trunc must be finite and > 0"):
        ops.depth_fuse_batch(_state(dims, P=2), [D, D], K, [E, E], origin=np.zeros((2, 3)), voxel=0.1, trunc=[0.4, float("nan")])
    with pytest.raises(ValueError, match="2 problems in state for 1 sets"):
        ops.depth_fuse_batch(_state(dims, P=2), [D], K, [E], origin=np.zeros((2, 3)), voxel=0.1, trunc=0.4)
    with pytest.raises(ValueError, match="one H x W per call"):
        ops.depth_fuse_batch(_state(dims, P=2), [D, D[:, :3].contiguous()], K, [E, E], origin=np.zeros((2, 3)), voxel=0.1, trunc=0.4)
    with pytest.raises(ValueError, match="min_obs must be >= 1"):
        ops.tsdf_volume(ok, 0)
    with pytest.raises(_lib.LsError, match="state sum must be an int32 HIP"):
        ops.tsdf_volume((ok[0].cpu(), ok[1].cpu()))
    assert not ok[0].any() and not ok[1].any()                              # every refusal came before the state was touched


# ------------------------------------------------------------------------------------------------ the volume
def test_volume_min_obs_counts_and_the_exact_one():
    from livingscenes_amd import ops
    dims, probs = _batch_problems()
    states = [run_twin(dims, pr)[0] for pr in probs]
    dev = tuple(_d(np.stack([s[k] for s in states]), torch.int32) for k in (0, 1))
    for min_obs in (1, 2):
        vol, valid, counts = ops.tsdf_volume(dev, min_obs)
        for b, s in enumerate(states):
            D, ok, c = fo.volume(s, min_obs)
            assert np.array_equal(vol[b].cpu().numpy().view(np.uint64), D.view(np.uint64)) and np.array_equal(valid[b].cpu().numpy(), ok.astype(np.uint8))
            assert counts[b].tolist() == c.tolist() and (vol[b].cpu().numpy()[~ok].view(np.uint64) == np.float64(1.0).view(np.uint64)).all()
            v1, k1, c1 = ops.tsdf_volume((dev[0][b], dev[1][b]), min_obs)
            assert torch.equal(v1, vol[b]) and torch.equal(k1, valid[b]) and torch.equal(c1, counts[b])
        assert counts[0, 0] > 0 and counts[0, 1] > 0 and counts[1].tolist() == [0, 0, int(np.prod(dims))]
    for dims1 in ((1, 1, 1), (255, 1, 1), (4, 8, 8), (257, 1, 1), (3, 5, 17)):                                 # the chunk's edges
        rng = np.random.default_rng(sum(dims1))
        S, N = rng.integers(-50000, 50000, dims1).astype(np.int32), rng.integers(0, 4, dims1).astype(np.int32)
        vol, valid, counts = ops.tsdf_volume((_d(S, torch.int32), _d(N, torch.int32)), 2)
        D, ok, c = fo.volume((S, N), 2)
        assert np.array_equal(vol.cpu().numpy().view(np.uint64), D.view(np.uint64)) and np.array_equal(valid.cpu().numpy(), ok) and counts.tolist() == c.tolist()


# ------------------------------------------------------------------------------------------------ end to end
def _part_views(p):
    return {k: p[k] for k in ("depth", "intrinsics", "world_to_cam")}


def _twin_fuse_part(state, p, origin, h, trunc, E=None, empty="unknown"):
    V = p["depth"].shape[0]
    E = p["world_to_cam"].cpu().numpy() if E is None else E
    return fo.fuse(state, p["depth"].cpu().numpy(), np.tile(p["intrinsics"].cpu().numpy().reshape(-1, 4), (V, 1))[:V], E, origin, h, trunc, empty)


def test_partial_views_to_fused_volumes_equal_the_twin_chain():
    """synth.make_partial_views -> More_Solver._fusion_grids -> ops.depth_fuse_batch -> ops.tsdf_volume against the twin chain, bit for bit"""
    from livingscenes_amd import ops
    from livingscenes_amd.lib_more.more_solver import More_Solver
    seeds, res = [2, 5], 20
    parts = synth.make_partial_views(seeds, 3, res=24, with_depth=True, device=_dev())
    clouds = [torch.cat(p["clouds"]) for p in parts]
    grids = More_Solver._fusion_grids(clouds, res, 4)
    state = ops.tsdf_state(2, grids["dims"], _dev())
    vcs = ops.depth_fuse_batch(state, [p["depth"] for p in parts], [p["intrinsics"] for p in parts], [p["world_to_cam"] for p in parts],
                               origin=grids["origin"], voxel=grids["voxel"], trunc=grids["trunc"])
    twins = []
    for b, p in enumerate(parts):
        origin, h, trunc = fo.fusion_grid(clouds[b].cpu().numpy(), res, 4)
        assert np.array_equal(grids["origin"][b].numpy(), origin) and float(grids["voxel"][b]) == h and float(grids["trunc"][b]) == trunc
        tw = fo.new_state((res,) * 3)
        wc = _twin_fuse_part(tw, p, origin, h, trunc)
        assert _same((state[0][b], state[1][b]), tw) and np.array_equal(vcs[b].cpu().numpy(), wc) and wc[:, fo.NEAR].all()
        twins.append((tw, origin, h))
    vol, valid, counts = ops.tsdf_volume(state)
    for b, (tw, _, _) in enumerate(twins):
        D, ok, c = fo.volume(tw)
        assert np.array_equal(vol[b].cpu().numpy().view(np.uint64), D.view(np.uint64)) and np.array_equal(valid[b].cpu().numpy(), ok) and counts[b].tolist() == c.tolist()
        assert c[1] > 0 and c[0] > c[1]                                   # the views saw the inside of the surface and the space before it


def test_fuse_batch_with_T_and_with_g(small_prior):
    from livingscenes_amd import ops
    from livingscenes_amd.lib_math.torch_se3 import inverse
    from livingscenes_amd.lib_more.more_solver import More_Solver
    solver = _solver(small_prior)
    parts = synth.make_partial_views([1, 4], 2, res=24, with_depth=True, device=_dev())
    views = [_part_views(p) for p in parts]
    rng = np.random.default_rng(9)
    T = torch.from_numpy(np.stack([_pose(rng, 0.3), _pose(rng, 0.3)])).to(_dev())               # memory -> rescan, [P,3,4] fp32
    T4 = torch.cat([T, T.new_tensor([0.0, 0.0, 0.0, 1.0]).expand(2, 1, 4)], 1)
    g = inverse(T).contiguous()                                                                  # rescan -> memory, fp32
    mems = [(torch.cat(p["clouds"]) @ g[b, :, :3].T + g[b, :, 3]).contiguous() for b, p in enumerate(parts)]   # the clouds in the memory's frame
    grids = More_Solver._fusion_grids(mems, 16, 4)
    dims = grids.pop("dims")
    for name, pose, to_obs in (("T", T, T.double()), ("T4", T4, T.double()), ("g", g, inverse(g.double()))):
        S, N = ops.tsdf_state(2, dims, _dev())
        vcs = solver._fuse_batch(dict(grids, sum=S, n=N), views, **{name[0]: pose}, empty="free")
        for b in range(2):
            cams = More_Solver._memory_cameras(views[b]["world_to_cam"], to_obs[b])
            s1 = _state(dims)
            vc = ops.depth_fuse(s1, views[b]["depth"], views[b]["intrinsics"], cams, origin=grids["origin"][b], voxel=grids["voxel"][b],
                                trunc=grids["trunc"][b], empty="free")
            assert torch.equal(S[b], s1[0]) and torch.equal(N[b], s1[1]) and torch.equal(vcs[b], vc), (name, b)
            tw = fo.new_state(dims)
            wc = _twin_fuse_part(tw, parts[b], grids["origin"][b].numpy(), float(grids["voxel"][b]), float(grids["trunc"][b]), cams.cpu().numpy(), "free")
            assert _same(s1, tw) and np.array_equal(vc.cpu().numpy(), wc) and wc[:, fo.NEAR].all(), (name, b)
    S, N = ops.tsdf_state(2, dims, _dev())
    vcs = solver._fuse_batch(dict(grids, sum=S, n=N), [views[0], None])                          # neither pose; a slot without views
    assert vcs[1].shape == (0, 6) and not N[1].any() and N[0].any()
    with pytest.raises(ValueError, match="not both"):
        solver._fuse_batch(dict(grids, sum=S, n=N), views, T=T, g=g)


def _fusion_scene(n, n_views=3):
    parts = synth.make_partial_views(range(n), n_views, res=32, with_depth=True, device=_dev())
    rng = np.random.default_rng(17)
    ref, rescan = [], []
    for p in parts:
        cloud = torch.cat(p["clouds"])
        assert cloud.shape[0] >= 700
        ref.append(cloud[torch.from_numpy(rng.permutation(cloud.shape[0])[:600]).to(cloud.device)])
        rescan.append(cloud[torch.from_numpy(rng.permutation(cloud.shape[0])[:700]).to(cloud.device)])
    return parts, torch.stack(ref), torch.stack(rescan)


def test_solve_sequence_without_fuse_res_is_unchanged(small_prior):
    from livingscenes_amd.lib_more import more_solver
    solver = _solver(small_prior)
    parts, ref, rescan = _fusion_scene(3)
    views = [_part_views(p) for p in parts]
    plain_steps, plain = more_solver.solve_sequence(solver, _scene(ref), [_scene(rescan)], voxel=0.02)
    off_steps, off = more_solver.solve_sequence(solver, dict(_scene(ref), views=views), [dict(_scene(rescan), views=views)], voxel=0.02, fuse_res=None,
                                                fuse_trunc_voxels=2, fuse_empty="free")
    assert set(off) == set(plain) == {"clouds", "codes", "meshes"} and len(off_steps) == len(plain_steps) == 1
    for i in range(3):
        assert torch.equal(off["clouds"][i], plain["clouds"][i]), i
    for key in CODE_KEYS:
        assert torch.equal(off["codes"][key], plain["codes"][key]), key
    a, b = off_steps[0], plain_steps[0]
    assert set(a) == set(b) and "n_fused_views" not in a
    assert a["merged_sizes"] == b["merged_sizes"] and a["n_new_points"] == b["n_new_points"] and torch.equal(a["matches"], b["matches"])
    for x, y in zip(a["registration"], b["registration"]):
        assert (x is None and y is None) or torch.equal(x, y)


def test_solve_sequence_fuses_under_the_pose_of_the_merge(small_prior, monkeypatch):
    """The matcher of the small random prior is replaced by the truth (slot i is rescan instance i) and the registration by a known
    rigid pose per pair, so memory['fusion'] can be replayed by hand: the same grids, ref views under the identity, then the rescan's
    views under T -- one _fuse_batch call per rescan, after the gate and independent of carve_tol."""
    from livingscenes_amd import ops
    from livingscenes_amd.lib_more import more_solver
    from livingscenes_amd.lib_more.more_solver import More_Solver
    solver = _solver(small_prior)
    n, h, res = 3, 0.02, 16
    parts, ref, rescan = _fusion_scene(n)
    views = [_part_views(p) for p in parts]
    rviews = list(views)
    rviews[1] = None                                                      # the second rescan instance has no views
    dev = _dev()
    rng = np.random.default_rng(4)
    Rt = torch.from_numpy(np.stack([_pose(rng, 0.05) for _ in range(n)])).to(dev)               # memory -> rescan
    moved = torch.stack([rescan[i].to(dev) @ Rt[i, :, :3].T + Rt[i, :, 3] for i in range(n)])   # the rescan clouds in the rescan's frame
    monkeypatch.setattr(solver, "_solve_object_matching", lambda *a, **k: {"matches0": torch.arange(n, device=dev)})
    monkeypatch.setattr(solver, "_solve_pairwise_registration_batch",
                        lambda src, tgt, **k: (Rt[:len(src), :, :3].contiguous(), Rt[:len(src), :, 3:].contiguous()))
    calls = []

    def spy(fusion, vws, *args, _real=solver._fuse_batch, **k):
        calls.append(([v is not None for v in vws], k))
        return _real(fusion, vws, *args, **k)
    monkeypatch.setattr(solver, "_fuse_batch", spy)
    plain_steps, plain = more_solver.solve_sequence(solver, _scene(ref), [_scene(moved)], voxel=h)
    steps, memory = more_solver.solve_sequence(solver, dict(_scene(ref), views=views), [dict(_scene(moved), views=rviews)], voxel=h, fuse_res=res,
                                               fuse_empty="free", mesh=False)
    monkeypatch.undo()
    step, fusion = steps[0], memory["fusion"]
    assert set(step) == set(plain_steps[0]) | {"n_fused_views"} and step["n_fused_views"] == [3, 0, 3]
    assert set(memory) == set(plain) | {"fusion"} and set(fusion) == {"sum", "n", "origin", "voxel", "trunc"}
    assert len(calls) == 2 and calls[0][0] == [True] * n and calls[1][0] == [True, False, True] and calls[1][1]["empty"] == "free"
    for i in range(n):
        assert torch.equal(memory["clouds"][i], plain["clouds"][i]), i     # the fusion changes nothing else
    # the replay: grids of the memory after the initial merge (= the step's ref_pc_lst), the ref views, the rescan's views under T
    grids = More_Solver._fusion_grids(step["ref_pc_lst"], res, 4)
    for k in ("origin", "voxel", "trunc"):
        assert torch.equal(fusion[k], grids[k]), k
    S, N = ops.tsdf_state(n, grids["dims"], dev)
    ops.depth_fuse_batch((S, N), [v["depth"] for v in views], [v["intrinsics"] for v in views], [v["world_to_cam"] for v in views],
                         origin=grids["origin"], voxel=grids["voxel"], trunc=grids["trunc"], empty="free")
    assert N.any()
    T = torch.cat([t for t in step["registration"]])                       # [n,4,4], what the merge used
    cams = [None if v is None else More_Solver._memory_cameras(v["world_to_cam"], T[i].double()[:3]) for i, v in enumerate(rviews)]
    ops.depth_fuse_batch((S, N), [None if v is None else v["depth"] for v in rviews], [views[0]["intrinsics"]] * n, cams,
                         origin=grids["origin"], voxel=grids["voxel"], trunc=grids["trunc"], empty="free")
    assert torch.equal(fusion["sum"], S) and torch.equal(fusion["n"], N)
    assert int(N[0].max()) > int(N[1].max()) >= 1                          # slot 1 saw the reference views only
