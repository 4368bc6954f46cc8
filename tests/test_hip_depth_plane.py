"""GPU tests of the normals of a depth map and of the weighted point-to-plane depth fusion (csrc/depthplane.hip: ls_depth_normals_f32,
ls_depth_fuse_weighted_f32 / ls_depth_fuse_weighted_batch_f32) and of the layers on top (ops.depth_normals / depth_fuse_weighted(_batch),
More_Solver._fuse_weighted_batch, solve_sequence_weighted_fusion).

Reference: tests/plane_oracle.py, the definitions of include/livingscenes_hip.h in NumPy float64.  The update is integer and the rest is
float64 written without contraction, so states, counts and the fused (sum, n) are held to the twin by EQUALITY.  A normal is one device
float64 square root, three divisions and one rounding to fp32 away from the twin's; NORMAL_ULPS is the allowance per component, 0: on
an MI355X every component of the cases below came out equal to the twin's bits.  The fuse is tested with the TWIN's normals
uploaded, so its equality does not hang on the normals kernel.  The generators and the cases are those of tests/test_depth_plane_cpu.py,
where the twin alone is shown to reach every state and class on them."""
import numpy as np
import pytest
import torch

import fuse_oracle as fo
import plane_oracle as po
import tsdf_mesh_oracle as tmo
import tsdf_ray_oracle as tro
from cloud_testlib import F, _dev, _pose, _scene, _solver, small_prior  # noqa: F401 (small_prior is a fixture)
from livingscenes_amd import synth
from test_depth_fuse_cpu import GPU_DIMS, fuse_problem
from test_depth_plane_cpu import WEIGHTS, case_normals, normal_cases, run_weighted, weighted_cases
from test_hip_depth_fuse import _fusion_scene, _part_views

pytestmark = pytest.mark.gpu
NORMAL_ULPS = 0


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


def _fuse(dims, pr, weights, normals=None, empty="unknown", state=None):
    from livingscenes_amd import ops
    state = _state(dims) if state is None else state
    vc = ops.depth_fuse_weighted(state, *_views(pr), weights=weights, normals=None if normals is None else _d(normals, torch.float32), empty=empty, **_grid(pr))
    return state, vc.cpu().numpy()


def _ordered(a):
    """fp32 bits as integers that grow with the value: the distance of two of them is their distance in ulps"""
    b = np.ascontiguousarray(a, F).view(np.int32).astype(np.int64)
    return np.where(b < 0, -(b & 0x7FFFFFFF), b)


def _normals_differ(got, want):
    """-> (components whose bits differ, components more than NORMAL_ULPS away)"""
    bits = got.view(np.uint32) != want.view(np.uint32)
    return int(bits.sum()), int((np.abs(_ordered(got) - _ordered(want)) > NORMAL_ULPS).sum())


# ------------------------------------------------------------------------------------------------ the normals against the twin
def test_normals_equal_the_twin():
    """ten image sizes (63 / 64 / 65 and 255 / 256 / 257 pixels per view, one row, one column, one pixel) x the wild view alone, three views
    and one plain view: states and counts integer-equal, normals bitwise (NORMAL_ULPS)"""
    from livingscenes_amd import ops
    total = differ = 0
    for H, W, views, pr, (n, st, counts) in normal_cases():
        gn, gs, gc = ops.depth_normals(_d(pr["depth"], torch.float32), _d(pr["K"], torch.float64), max_jump=pr["max_jump"])
        what = (H, W, views)
        assert gn.shape == n.shape and gs.shape == st.shape and gc.shape == counts.shape
        assert np.array_equal(gs.cpu().numpy(), st) and np.array_equal(gc.cpu().numpy(), counts), what
        gn = gn.cpu().numpy()
        assert not gn[st != po.VALID].view(np.uint32).any(), what                        # +0.0 by its bits
        b, far = _normals_differ(gn, n)
        total, differ = total + 3 * int((st == po.VALID).sum()), differ + b
        assert far == 0, (what, b, far)
    print(f"{differ} of {total} components of VALID normals differ from the twin's bits")
    one = ops.depth_normals(_d(np.ones((2, 4, 4), F), torch.float32), _d(np.array([4.0, 4.0, 1.5, 1.5]), torch.float64), max_jump=0.1)       # one K for all views
    assert torch.equal(one[0][0], one[0][1]) and one[2].tolist() == [[0, 16, 0, 0]] * 2
    none = ops.depth_normals(torch.zeros(0, 4, 4, device=_dev()), _d(np.zeros((0, 4)), torch.float64), max_jump=0.1)
    assert [tuple(t.shape) for t in none] == [(0, 4, 4, 3), (0, 4, 4), (0, 4)]


# ------------------------------------------------------------------------------------------------ the weighted fuse against the twin
@pytest.mark.parametrize("dims", GPU_DIMS)
def test_weighted_fuse_size_edges(dims):
    """voxel counts where a wave of 64 or a chunk of 256 is full, one short and one over; 0, 1 and 3 views; four image sizes; two sets of
    weights; without normals and with the TWIN's; the mode alternates with the weights"""
    for V, (H, W), pr, nrm in weighted_cases(dims):
        for k, w in enumerate(WEIGHTS):
            for use in (None, nrm):
                empty = ("unknown", "free")[(k + (use is None)) % 2]
                want, wc = run_weighted(dims, pr, w, use, empty)
                got, vc = _fuse(dims, pr, w, use, empty)
                assert _same(got, want) and vc.shape == (V, 7) and np.array_equal(vc, wc), (dims, V, H, W, w, use is None, empty)
                assert (vc.sum(1) == np.prod(dims)).all()


@pytest.mark.parametrize("dims", GPU_DIMS)
def test_unit_weights_without_normals_are_the_fuse(dims):
    """weights (9, 1, 1, 1) and normals=None: the state of ops.depth_fuse on the same inputs, bit for bit -- the new kernel tied to the old"""
    from livingscenes_amd import ops
    for V, (H, W), pr, _ in weighted_cases(dims):
        for empty in ("unknown", "free"):
            old = _state(dims)
            oc = ops.depth_fuse(old, *_views(pr), empty=empty, **_grid(pr)).cpu().numpy()
            new, vc = _fuse(dims, pr, (9, 1, 1, 1), None, empty)
            assert torch.equal(new[0], old[0]) and torch.equal(new[1], old[1]), (dims, V, H, W, empty)
            assert np.array_equal(vc[:, [po.OUT, po.EMPTY, po.OCCLUDED, po.NEAR_PROJ, po.FREE, po.SATURATED]], oc) and not vc[:, po.NEAR_PLANE].any()


def test_weighted_fuse_saturation():
    """a state prefilled with n where a weight of 64 fits exactly (65535 - 64), is one over (65535 - 63), and 0 and 65535; three views: the
    order of the call decides"""
    dims = (4, 8, 9)
    rng = np.random.Generator(np.random.Philox(key=[8, 1]))
    pr = fuse_problem(rng, dims, 3, 16, 16)
    nrm = case_normals(pr)
    S0 = rng.integers(-1000, 1000, dims).astype(np.int32)
    N0 = rng.choice([0, 65535 - 64, 65535 - 63, 65535 - 5, 65535], dims).astype(np.int32)
    for w in WEIGHTS:
        for empty in ("unknown", "free"):
            want = (S0.copy(), N0.copy())
            wc = po.fuse_weighted(want, pr["depth"], pr["K"], pr["E"], pr["origin"], pr["voxel"], pr["trunc"], w, nrm, empty)
            assert wc[:, po.SATURATED].all() and want[1].max() == 65535 and (want[1] != N0).any()
            got, vc = _fuse(dims, pr, w, nrm, empty, _state(dims, like=(S0, N0)))
            assert _same(got, want) and np.array_equal(vc, wc), (w, empty)
    # one voxel, by hand: 65535 - 64 takes a plane vote of 64 and is full, 65535 - 63 refuses it
    one, flat = np.ones((1, 5, 5), F), np.tile(np.array([0, 0, -1], F), (1, 5, 5, 1))
    pr1 = dict(origin=np.array([0, 0, 0.99]), voxel=1.0, trunc=0.04, depth=one, K=np.array([[4.0, 4.0, 2.0, 2.0]]), E=np.eye(3, 4)[None])
    for n0, cls, n1 in ((65535 - 64, po.NEAR_PLANE, 65535), (65535 - 63, po.SATURATED, 65535 - 63)):
        st = _state((1, 1, 1), like=(np.full((1, 1, 1), 7, np.int32), np.full((1, 1, 1), n0, np.int32)))
        (S, N), vc = _fuse((1, 1, 1), pr1, (64, 1, 64, 1), flat, state=st)
        assert (int(np.flatnonzero(vc[0])[0]), int(S[0, 0, 0]), int(N[0, 0, 0])) == (cls, 7 + (64 * 4096 if n1 == 65535 else 0), n1)


def test_weighted_fuse_split_calls_and_order():
    """two calls of 2 + 1 views equal one call of 3, equal the reversed order"""
    dims = (6, 7, 8)
    pr = fuse_problem(np.random.Generator(np.random.Philox(key=[8, 2])), dims, 3, 16, 16)
    nrm = case_normals(pr)
    part = lambda idx: dict(pr, depth=pr["depth"][idx], K=pr["K"][idx], E=pr["E"][idx])    # noqa: E731
    for w, empty in zip(WEIGHTS, ("free", "unknown")):
        want, wc = run_weighted(dims, pr, w, nrm, empty)
        whole, vc = _fuse(dims, pr, w, nrm, empty)
        state = _state(dims)
        _, va = _fuse(dims, part([0, 1]), w, nrm[[0, 1]], empty, state)
        _, vb = _fuse(dims, part([2]), w, nrm[[2]], empty, state)
        back, vr = _fuse(dims, part([2, 1, 0]), w, nrm[[2, 1, 0]], empty)
        assert _same(whole, want) and _same(state, want) and _same(back, want) and want[1].max() > 3
        assert np.array_equal(vc, wc) and np.array_equal(np.concatenate([va, vb]), wc) and np.array_equal(vr, wc[::-1])


def _batch_problems():
    dims = (5, 9, 7)
    rng = np.random.Generator(np.random.Philox(key=[8, 3]))
    probs = [fuse_problem(rng, dims, V, 16, 16) for V in (3, 0, 1, 2, 2)]
    return dims, probs, [case_normals(pr) for pr in probs]


def test_weighted_batch_is_the_single_op_reversed_and_again():
    """five problems, one of them without views: every slice is the single op's bits, twice, and again with the problems reversed; the
    normals as a list and as one packed tensor"""
    from livingscenes_amd import ops
    dims, probs, nrms = _batch_problems()
    w = WEIGHTS[1]
    for empty in ("unknown", "free"):
        singles = [_fuse(dims, pr, w, nr, empty) for pr, nr in zip(probs, nrms)]
        for order in (list(range(5)), list(range(5)), list(range(4, -1, -1))):
            ps, ns = [probs[i] for i in order], [nrms[i] for i in order]
            state = _state(dims, P=5)
            hole = order.index(1)                                          # the problem WITHOUT views: its state is not fresh, and the call must
            state[0][hole].fill_(11)                                       # leave it as it is
            views = [None if pr["depth"].shape[0] == 0 else _views(pr) for pr in ps]
            dn = [None if v is None else _d(nr, torch.float32) for v, nr in zip(views, ns)]
            packed = order[0] == 4
            vcs = ops.depth_fuse_weighted_batch(state, [None if v is None else v[0] for v in views], [None if v is None else v[1] for v in views],
                                                [None if v is None else v[2] for v in views], origin=np.stack([pr["origin"] for pr in ps]),
                                                voxel=[pr["voxel"] for pr in ps], trunc=[pr["trunc"] for pr in ps], weights=w,
                                                normals=torch.cat([t for t in dn if t is not None]) if packed else dn, empty=empty)
            for b, i in enumerate(order):
                (S, N), vc = singles[i]
                if b == hole:
                    assert not S.any() and not N.any() and vcs[b].shape == (0, 7) and not state[1][b].any()
                    S = S + 11
                assert torch.equal(state[0][b], S) and torch.equal(state[1][b], N) and np.array_equal(vcs[b].cpu().numpy(), vc), (empty, order, b)
    none = ops.depth_fuse_weighted_batch(_state(dims, P=2), [None, None], [None, None], [None, None], origin=np.zeros((2, 3)), voxel=0.1, trunc=0.4, weights=w)
    assert [tuple(v.shape) for v in none] == [(0, 7)] * 2


def test_launch_counts_depend_on_nothing():
    """one kernel for one problem with one view, and one for five problems with up to three views; one kernel for the normals of one view
    and of eight"""
    from livingscenes_amd import _lib, ops
    from test_hip_render import _kernel_launches
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=_dev())
    rng = np.random.Generator(np.random.Philox(key=[8, 4]))
    dims = (5, 9, 7)

    def raw(nviews):
        probs = [fuse_problem(rng, dims, V, 16, 16) for V in nviews]
        P, views = len(nviews), sum(nviews)
        S, N = _state(dims, P=P)
        D, K, E = (torch.cat(t) for t in zip(*[_views(pr) for pr in probs]))
        Nr = _d(np.concatenate([case_normals(pr) for pr in probs]), torch.float32)
        o, h, t = np.stack([pr["origin"] for pr in probs]), np.array([pr["voxel"] for pr in probs]), np.array([pr["trunc"] for pr in probs])
        vo, vc, wts = ops._offsets(nviews), torch.empty(views, 7, dtype=torch.int64, device=_dev()), np.array([64, 1, 64, 1], np.int32)
        torch.cuda.synchronize()
        keep = (o, h, t, vo, wts)                                          # the host arrays live as long as the closure
        return lambda: _lib.call(_dev(), "ls_depth_fuse_weighted_batch_f32", P, _lib.ptr(S), _lib.ptr(N), *dims, ops._hptr(keep[0]), ops._hptr(keep[1]),
                                 ops._hptr(keep[2]), _lib.ptr(D), _lib.ptr(Nr), views, ops._hptr(keep[3]), 16, 16, _lib.ptr(K), _lib.ptr(E), 0.05, 0,
                                 ops._hptr(keep[4]), _lib.ptr(vc), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(_dev()))
    one, five = _kernel_launches(raw([1])), _kernel_launches(raw([3, 0, 1, 0, 2]))
    assert len(one) == len(five) == 1 and "fuse_weighted_kernel" in one[0] and "fuse_weighted_kernel" in five[0], (one, five)

    def raw_normals(V):
        D, K = torch.rand(V, 17, 15, device=_dev()) + 0.5, _d(np.tile([20.0, 20.0, 7.0, 8.0], (V, 1)), torch.float64)
        n, s, c = torch.empty(V, 17, 15, 3, device=_dev()), torch.empty(V, 17, 15, dtype=torch.uint8, device=_dev()), torch.empty(V, 4, dtype=torch.int64, device=_dev())
        mj = np.full(V, 0.1)
        torch.cuda.synchronize()
        return lambda: _lib.call(_dev(), "ls_depth_normals_f32", _lib.ptr(D), V, 17, 15, _lib.ptr(K), ops._hptr(mj), _lib.ptr(n), _lib.ptr(s), _lib.ptr(c),
                                 _lib.ptr(ws), ws.numel(), _lib.stream_ptr(_dev()))
    one, eight = _kernel_launches(raw_normals(1)), _kernel_launches(raw_normals(8))
    assert len(one) == len(eight) == 1 and "normals_kernel" in one[0] and "normals_kernel" in eight[0], (one, eight)


def test_bindings_refuse_what_the_device_path_cannot_take():
    from livingscenes_amd import _lib, ops
    dims = (4, 4, 4)
    pr = fuse_problem(np.random.Generator(np.random.Philox(key=[8, 5])), dims, 2, 5, 7)
    D, K, E = _views(pr)
    Nr = _d(case_normals(pr), torch.float32)
    g = dict(_grid(pr), weights=(64, 1, 64, 1))
    ok = _state(dims)
    with pytest.raises(_lib.LsError, match="state sum must be an int32 HIP"):
        ops.depth_fuse_weighted((ok[0].cpu(), ok[1]), D, K, E, **g)
    with pytest.raises(_lib.LsError, match="depth must be an fp32 HIP"):
        ops.depth_fuse_weighted(ok, D.double(), K, E, **g)
    with pytest.raises(_lib.LsError, match="normals must be an fp32 HIP"):
        ops.depth_fuse_weighted(ok, D, K, E, normals=Nr.cpu(), **g)
    with pytest.raises(_lib.LsError, match="normals must be an fp32 HIP"):
        ops.depth_fuse_weighted(ok, D, K, E, normals=Nr.double(), **g)
    with pytest.raises(ValueError, match="normals is"):
        ops.depth_fuse_weighted(ok, D, K, E, normals=Nr[:1], **g)
    with pytest.raises(ValueError, match="normals is"):
        ops.depth_fuse_weighted(ok, D, K, E, normals=Nr[..., :2], **g)
    with pytest.raises(TypeError, match="weights"):
        ops.depth_fuse_weighted(ok, D, K, E, **_grid(pr))                                           # no default
    for bad in ((0, 1, 1, 1), (1, 1, 1, 256), (1, 1, 1), (1, 2.5, 1, 1)):
        with pytest.raises(ValueError, match="weights are four integers"):
            ops.depth_fuse_weighted(ok, D, K, E, **dict(g, weights=bad))
    with pytest.raises(ValueError, match="empty must be"):
        ops.depth_fuse_weighted(ok, D, K, E, empty="maybe", **g)
    with pytest.raises(_lib.LsError, match="voxel must be finite and > 0"):
        ops.depth_fuse_weighted(ok, D, K, E, origin=pr["origin"], voxel=0.0, trunc=0.4, weights=(1, 1, 1, 1))
    with pytest.raises(ValueError, match="normals for every problem that has views"):
        ops.depth_fuse_weighted_batch(_state(dims, P=2), [D, D], K, [E, E], origin=np.zeros((2, 3)), voxel=0.1, trunc=0.4, weights=(1, 1, 1, 1), normals=[Nr, None])
    with pytest.raises(ValueError, match="sets of normals"):
        ops.depth_fuse_weighted_batch(_state(dims, P=2), [D, D], K, [E, E], origin=np.zeros((2, 3)), voxel=0.1, trunc=0.4, weights=(1, 1, 1, 1), normals=[Nr])
    with pytest.raises(_lib.LsError, match="depth must be an fp32 HIP"):
        ops.depth_normals(D.cpu(), K, max_jump=0.1)
    with pytest.raises(ValueError, match="depth is"):
        ops.depth_normals(D[0], K, max_jump=0.1)
    with pytest.raises(ValueError, match="intrinsics is"):
        ops.depth_normals(D, K[:1].expand(3, 4), max_jump=0.1)
    with pytest.raises(ValueError, match="values of max_jump"):
        ops.depth_normals(D, K, max_jump=[0.1, 0.1, 0.1])
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="max_jump must be finite and > 0"):
            ops.depth_normals(D, K, max_jump=[0.1, bad])
    assert not ok[0].any() and not ok[1].any()                              # every refusal came before the state was touched


# ------------------------------------------------------------------------------------------------ the layers
def _twin_chain(state, views, cams, origin, h, trunc, weights, value, empty, max_jump=None):
    """what _fuse_weighted_batch does to one slot, on the twin: the normals of the views (max_jump None: the slot's trunc), then the fuse"""
    depth = views["depth"].cpu().numpy()
    V = depth.shape[0]
    K = np.broadcast_to(views["intrinsics"].cpu().numpy().reshape(-1, 4), (V, 4))
    nrm = po.normals(depth, K, trunc if max_jump is None else max_jump)[0] if value == "plane" else None
    return po.fuse_weighted(state, depth, K, cams, origin, h, trunc, weights, nrm, empty)


def test_fuse_weighted_batch_with_T_and_with_g(small_prior):
    from livingscenes_amd import ops
    from livingscenes_amd.lib_math.torch_se3 import inverse
    from livingscenes_amd.lib_more.more_solver import More_Solver
    solver = _solver(small_prior)
    parts = synth.make_partial_views([1, 4], 2, res=24, with_depth=True, device=_dev())
    views = [_part_views(p) for p in parts]
    rng = np.random.default_rng(9)
    T = torch.from_numpy(np.stack([_pose(rng, 0.3), _pose(rng, 0.3)])).to(_dev())               # memory -> rescan, [P,3,4] fp32
    g = inverse(T).contiguous()                                                                  # rescan -> memory, fp32
    mems = [(torch.cat(p["clouds"]) @ g[b, :, :3].T + g[b, :, 3]).contiguous() for b, p in enumerate(parts)]
    grids = More_Solver._fusion_grids(mems, 16, 4)
    dims = grids.pop("dims")
    w = (64, 1, 64, 1)
    for name, pose, to_obs, value, jump in (("T", T, T.double(), "plane", None), ("g", g, inverse(g.double()), "plane", 0.01), ("T", T, T.double(), "projective", None)):
        S, N = ops.tsdf_state(2, dims, _dev())
        vcs = solver._fuse_weighted_batch(dict(grids, sum=S, n=N), views, **{name: pose}, weights=w, value=value, max_jump=jump, empty="free")
        for b in range(2):
            cams = More_Solver._memory_cameras(views[b]["world_to_cam"], to_obs[b]).cpu().numpy()
            tw = fo.new_state(dims)
            wc = _twin_chain(tw, views[b], cams, grids["origin"][b].numpy(), float(grids["voxel"][b]), float(grids["trunc"][b]), w, value, "free", jump)
            assert _same((S[b], N[b]), tw) and np.array_equal(vcs[b].cpu().numpy(), wc), (name, value, b)
            assert wc[:, po.NEAR_PLANE].all() == (value == "plane") and (value == "plane" or wc[:, po.NEAR_PROJ].all()), (name, value, b, wc)
    S, N = ops.tsdf_state(2, dims, _dev())
    vcs = solver._fuse_weighted_batch(dict(grids, sum=S, n=N), [views[0], None], weights=w)      # neither pose; a slot without views
    assert vcs[1].shape == (0, 7) and not N[1].any() and N[0].any()
    with pytest.raises(ValueError, match="not both"):
        solver._fuse_weighted_batch(dict(grids, sum=S, n=N), views, T=T, g=g, weights=w)
    with pytest.raises(ValueError, match="value must be"):
        solver._fuse_weighted_batch(dict(grids, sum=S, n=N), views, weights=w, value="cosine")
    with pytest.raises(TypeError, match="weights"):
        solver._fuse_weighted_batch(dict(grids, sum=S, n=N), views)


def test_solve_sequence_weighted_fusion_equals_the_twin_chain(small_prior, monkeypatch):
    """test_hip_depth_fuse's scene and replacements (the matcher is the truth, the registration a known rigid pose per pair), so that
    memory['fusion'] can be replayed on the twin: the same grids, ref views under the identity, then the rescan's views under T, every
    fuse through _fuse_weighted_batch and none through _fuse_batch.  Then the readers of a fused state on the WEIGHTED state: the raycast
    and the mesh run and equal their twins."""
    from livingscenes_amd import ops
    from livingscenes_amd.lib_more import more_solver
    from livingscenes_amd.lib_more.more_solver import More_Solver
    from test_hip_tsdf_raycast import _same as _same_views
    solver = _solver(small_prior)
    n, h, res = 3, 0.02, 16
    parts, ref, rescan = _fusion_scene(n)
    views = [_part_views(p) for p in parts]
    rviews = list(views)
    rviews[1] = None                                                      # the second rescan instance has no views
    dev = _dev()
    rng = np.random.default_rng(4)
    Rt = torch.from_numpy(np.stack([_pose(rng, 0.05) for _ in range(n)])).to(dev)               # memory -> rescan
    moved = torch.stack([rescan[i].to(dev) @ Rt[i, :, :3].T + Rt[i, :, 3] for i in range(n)])
    monkeypatch.setattr(solver, "_solve_object_matching", lambda *a, **k: {"matches0": torch.arange(n, device=dev)})
    monkeypatch.setattr(solver, "_solve_pairwise_registration_batch",
                        lambda src, tgt, **k: (Rt[:len(src), :, :3].contiguous(), Rt[:len(src), :, 3:].contiguous()))
    calls, plain_calls = [], []

    def spy(fusion, vws, *args, _real=solver._fuse_weighted_batch, **k):
        calls.append(([v is not None for v in vws], k))
        return _real(fusion, vws, *args, **k)
    monkeypatch.setattr(solver, "_fuse_weighted_batch", spy)
    monkeypatch.setattr(solver, "_fuse_batch", lambda *a, **k: plain_calls.append(1))
    w = (64, 1, 64, 1)
    steps, memory = more_solver.solve_sequence_weighted_fusion(solver, dict(_scene(ref), views=views), [dict(_scene(moved), views=rviews)], fuse_weights=w,
                                                               voxel=h, fuse_res=res, fuse_empty="free", mesh=False)
    monkeypatch.undo()
    step, fusion = steps[0], memory["fusion"]
    assert step["n_fused_views"] == [3, 0, 3] and set(fusion) == {"sum", "n", "origin", "voxel", "trunc"} and not plain_calls
    assert len(calls) == 2 and calls[0][0] == [True] * n and calls[1][0] == [True, False, True]
    assert all(c[1]["weights"] == w and c[1]["value"] == "plane" and c[1]["max_jump"] is None and c[1]["empty"] == "free" for c in calls)
    grids = More_Solver._fusion_grids(step["ref_pc_lst"], res, 4)
    for k in ("origin", "voxel", "trunc"):
        assert torch.equal(fusion[k], grids[k]), k
    T = torch.cat([t for t in step["registration"]])                       # [n,4,4], what the merge used
    twins = []
    for i in range(n):
        o, hh, tr = grids["origin"][i].numpy(), float(grids["voxel"][i]), float(grids["trunc"][i])
        tw = fo.new_state(grids["dims"])
        _twin_chain(tw, views[i], views[i]["world_to_cam"].cpu().numpy(), o, hh, tr, w, "plane", "free")
        if rviews[i] is not None:
            cams = More_Solver._memory_cameras(rviews[i]["world_to_cam"], T[i].double()[:3]).cpu().numpy()
            _twin_chain(tw, rviews[i], cams, o, hh, tr, w, "plane", "free")
        assert _same((fusion["sum"][i], fusion["n"][i]), tw), i
        twins.append((tw, o, hh, tr))
    assert int(fusion["n"][0].max()) > int(fusion["n"][1].max()) >= 64      # weights, not counts; slot 1 saw the reference views only
    # the readers of the state
    for i, (tw, o, hh, tr) in enumerate(twins):
        state = (fusion["sum"][i].contiguous(), fusion["n"][i].contiguous())
        for min_obs in (1, 65):                                             # a weight threshold: more than one surface vote
            v, f, counts = ops.tsdf_mesh(state, origin=o, voxel=hh, min_obs=min_obs)
            wv, wf = tmo.mesh(tw, o, hh, min_obs)[:2]
            assert np.array_equal(f.cpu().numpy(), wf) and np.array_equal(v.cpu().numpy().view(np.int64), wv.view(np.int64)) and (min_obs > 1 or len(wf) > 100), (i, min_obs)
        E = views[i]["world_to_cam"][:1].cpu().numpy()[0]
        M = np.concatenate([E[:, :3].T, (-E[:, :3].T @ E[:, 3])[:, None]], 1)[None]
        K = views[i]["intrinsics"].cpu().numpy().reshape(-1, 4)[0]
        H, W = views[i]["depth"].shape[1:]
        got = ops.tsdf_raycast(state, _d(M, torch.float64), _d(K, torch.float64), H, W, origin=o, voxel=hh, trunc=tr)
        want = tro.raycast(tw, M, K, H, W, o, hh, tr)
        _same_views(got, want, i)
        assert want["counts"][0, tro.HIT] > 20, want["counts"]
