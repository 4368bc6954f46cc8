"""GPU tests of the scene memory's raycast of a fused state and of the view comparison (csrc/tsdfray.hip: ls_tsdf_raycast_f64 /
ls_tsdf_raycast_batch_f64, ls_depth_compare_f32) and of the layers above them (More_Solver._predict_views_batch, _view_agreement_batch,
solve_sequence_view_gated(view_tol=, min_view_agreement=)).

Reference: tests/tsdf_ray_oracle.py, the definition of include/livingscenes_hip.h in NumPy float64.  Depth bits, states, counts and
classes are held to it by EQUALITY, alone, in any batch and in any run.  The normal is one device float64 square root, one division and
one rounding to fp32 away from the twin's, and the project pins the rounding of the device's sqrt nowhere, so the allowance first
written here was 2^-22 per component.  On an MI355X all 371 448 normal components of the cases below came out EQUAL to the twin's bits,
so the check was tightened: the normals are held by equality too.  The states, cameras and cases are those of tests/test_tsdf_ray_cpu.py, where the twin alone is shown to
reach every ray state and every view class on them."""
import numpy as np
import pytest
import torch

import tsdf_ray_oracle as tro
from cloud_testlib import STEP_KEYS, F, _dev, _scene, _solver, small_prior  # noqa: F401 (a fixture)
from test_hip_cloud_icp import _step_values_equal
from test_tsdf_ray_cpu import DIMS, TOL, ZNEAR, _call, bits, cameras_of, cases, expected, observed_of, ray_state_of

pytestmark = pytest.mark.gpu


def _state(state):
    return tuple(torch.from_numpy(np.array(t)).to(_dev()) for t in state)      # a copy: the shared states are read-only


def _d(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float64)).to(_dev())


def _same(got, want, what):
    """got: device (depth, normal, state, counts); want: the twin's dict; every output the same bits"""
    depth, normal, st, counts = (t.cpu().numpy() for t in got)
    assert np.array_equal(st, want["state"]), what
    assert np.array_equal(counts, want["counts"]), what
    assert np.array_equal(bits(depth), bits(want["depth"])), what
    differ = int((bits(normal) != bits(want["normal"])).sum())
    assert differ == 0, (what, differ, np.abs(normal.astype(np.float64) - want["normal"].astype(np.float64)).max())


@pytest.mark.parametrize("dims", DIMS)
def test_raycast_equals_the_twin(dims):
    from livingscenes_amd import ops
    for kind, d, min_obs, image, step in cases():
        if d != dims:
            continue
        state, origin, h, trunc = ray_state_of(kind, dims)
        M, K, want = expected(kind, dims, min_obs, image, step)
        got = ops.tsdf_raycast(_state(state), _d(M), _d(K), image[0], image[1], origin=origin, voxel=h, trunc=trunc, min_obs=min_obs, step=step, znear=ZNEAR)
        _same(got, want, (kind, dims, min_obs, image, step))


def _batch():
    """P = 5 on (9,8,7): sphere with 3 views, a problem without views, the all-zero state with 2 views, box with 1 view, holes with 2"""
    dims, image = (9, 8, 7), (13, 17)
    probs = []
    for kind, pick in (("sphere", [0, 4, 5]), ("box", []), ("zero", [0, 1]), ("box", [4]), ("holes", [0, 2])):
        state, origin, h, trunc = ray_state_of(kind, dims)
        M, K = cameras_of(kind, dims, *image)
        probs.append((state, origin, h, trunc, M[pick], K[pick]))
    return probs, image


def _run_batch(probs, image, packed):
    from livingscenes_amd import ops
    S = torch.stack([_state(p[0])[0] for p in probs])
    N = torch.stack([_state(p[0])[1] for p in probs])
    return ops.tsdf_raycast_batch((S, N), [_d(p[4]) if len(p[4]) else None for p in probs], [_d(p[5]) for p in probs], image[0], image[1],
                                  origin=np.stack([p[1] for p in probs]), voxel=[p[2] for p in probs], trunc=[p[3] for p in probs], min_obs=1, step=0.5,
                                  znear=ZNEAR, packed=packed)


def test_raycast_batch_is_the_single_op_in_any_run():
    from livingscenes_amd import ops
    probs, image = _batch()
    first = _run_batch(probs, image, False)
    again = _run_batch(probs, image, False)
    depth, normal, st, counts, vo = _run_batch(probs, image, True)
    assert vo.tolist() == [0, 3, 3, 5, 6, 8] and tuple(depth.shape) == (8, 13, 17) and tuple(normal.shape) == (8, 13, 17, 3)
    for p, (state, origin, h, trunc, M, K) in enumerate(probs):
        assert first[p][0].shape[0] == len(M)
        for a, b in zip(first[p], again[p]):
            assert torch.equal(a, b), p
        for a, b in zip(first[p], (depth, normal, st, counts)):
            assert torch.equal(a, b[vo[p]:vo[p + 1]]), p
        if len(M) == 0:
            continue
        single = ops.tsdf_raycast(_state(state), _d(M), _d(K), image[0], image[1], origin=origin, voxel=h, trunc=trunc, step=0.5, znear=ZNEAR)
        for a, b in zip(first[p], single):
            assert np.array_equal(a.cpu().numpy().view(np.uint8), b.cpu().numpy().view(np.uint8)), p     # the same bytes
        want = tro.raycast(state, M, K, image[0], image[1], origin, h, trunc, 1, 0.5, ZNEAR)
        _same(first[p], want, p)
    assert first[2][2].cpu().numpy().max() <= tro.UNSEEN                      # the all-zero state: nothing known


def test_depth_compare_equals_the_twin():
    """observed depths with NaN, 0, negative and +inf values and with tol exactly on both boundaries (observed_of)"""
    from livingscenes_amd import ops
    seen, boundary = set(), 0
    for kind, dims, min_obs, image, step in cases()[3::5]:
        want = expected(kind, dims, min_obs, image, step)[2]
        obs = observed_of(want)
        cls, cnt = tro.compare(obs, want["depth"], want["state"], TOL)
        dev = [torch.from_numpy(np.ascontiguousarray(x)).to(_dev()) for x in (obs, want["depth"], want["state"])]
        got_cls, got_cnt = ops.depth_compare(*dev, tol=TOL)
        assert np.array_equal(got_cls.cpu().numpy(), cls) and np.array_equal(got_cnt.cpu().numpy(), cnt), (kind, dims, image)
        again = ops.depth_compare(*dev, tol=TOL)
        assert torch.equal(again[0], got_cls) and torch.equal(again[1], got_cnt)
        seen |= set(np.unique(cls).tolist())
        s = obs.astype(np.float64) - want["depth"].astype(np.float64)
        with np.errstate(all="ignore"):
            boundary += int(((want["state"] == tro.HIT) & (np.abs(s) == TOL)).sum())
    assert seen == {0, 1, 2, 3, 4} and boundary > 5 and np.isnan(obs).any() and np.isinf(obs).any() and (obs < 0).any() and (obs == 0).any()


def test_refusals_are_made_on_the_host():
    from livingscenes_amd import _lib, ops
    state, origin, h, trunc = ray_state_of("sphere", (9, 8, 7))
    M, K = cameras_of("sphere", (9, 8, 7), 13, 17)
    dev_state = _state(state)
    good = dict(origin=origin, voxel=h, trunc=trunc)
    for kw, word in ((dict(step=0.05), "step must lie in"), (dict(step=1.5), "step must lie in"), (dict(step=float("nan")), "step must lie in"),
                     (dict(znear=0.0), "znear must be finite and > 0"), (dict(znear=-1.0), "znear must be finite and > 0"),
                     (dict(voxel=float("inf")), "voxel must be finite and > 0"), (dict(trunc=float("nan")), "trunc must be finite and > 0"),
                     (dict(origin=[0.0, float("nan"), 0.0]), "origin must be finite")):
        with pytest.raises(_lib.LsError, match=word):
            ops.tsdf_raycast(dev_state, _d(M), _d(K), 13, 17, **dict(good, **kw))
    with pytest.raises(ValueError, match="min_obs"):
        ops.tsdf_raycast(dev_state, _d(M), _d(K), 13, 17, min_obs=0, **good)
    with pytest.raises(ValueError, match="at least one pixel"):
        ops.tsdf_raycast(dev_state, _d(M), _d(K), 0, 17, **good)
    with pytest.raises(ValueError, match="sets of cameras"):
        ops.tsdf_raycast_batch((dev_state[0][None], dev_state[1][None]), [_d(M), _d(M)], _d(K[0]), 13, 17, **good)
    with pytest.raises(ValueError, match="tol must be > 0"):
        ops.depth_compare(torch.zeros(1, 2, 2, device=_dev()), torch.zeros(1, 2, 2, device=_dev()), torch.zeros(1, 2, 2, dtype=torch.uint8, device=_dev()), tol=0.0)
    # bad offsets, with buffers that are not device memory: the call returns before anything could be launched on them
    lib = _lib.load()
    for off, word in (([0, 4, 3], "decreases"), ([0, 1, 2], "disagrees with the total"), ([1, 2, 3], "is 1, not 0")):
        rc, msg = _call(lib, view_off=off)
        assert rc == -1 and word in msg, msg


# ------------------------------------------------------------------------------------------------ the layers above
def _views_scene(n=2, n_views=2):
    from test_hip_depth_fuse import _fusion_scene, _part_views
    parts, ref, rescan = _fusion_scene(n, n_views)
    return [_part_views(p) for p in parts], ref, rescan


def _twin_agreement(fusion, views, pred, tol, min_obs=1, step=0.5):
    """the twin's raycast at the camera-to-memory matrices the solver formed (pred[p]['cam_to_world']) and its comparison -> per slot
    (agree, through, in_front, counts)"""
    S, N = fusion["sum"].cpu().numpy(), fusion["n"].cpu().numpy()
    out = []
    for p, v in enumerate(views):
        if v is None:
            out.append(None)
            continue
        H, W = v["depth"].shape[1:]
        r = tro.raycast((S[p], N[p]), pred[p]["cam_to_world"].cpu().numpy(), v["intrinsics"].cpu().numpy(), H, W, fusion["origin"][p].numpy(),
                        float(fusion["voxel"][p]), float(fusion["trunc"][p]), min_obs, step, 0.05)
        _same((pred[p]["depth"], pred[p]["normal"], pred[p]["state"], pred[p]["counts"]), r, ("slot", p))
        _, cnt = tro.compare(v["depth"].cpu().numpy(), r["depth"], r["state"], tol)
        out.append((*tro.agreement(cnt), cnt.sum(0)))
    return out


def _shifted(fusion, views, factor=3.0):
    """memory -> rescan poses [P,4,4] float64: the identity moved by factor * trunc along the optical axis of every slot's first view"""
    T = torch.eye(4, dtype=torch.float64).repeat(len(views), 1, 1)
    for p, v in enumerate(views):
        axis = v["world_to_cam"][0, 2, :3].cpu().to(torch.float64)            # the third row of the rotation: the camera's z in the memory's frame
        T[p, :3, 3] = factor * float(fusion["trunc"][p]) * axis
    return T.to(_dev())


def test_view_agreement_batch_equals_the_twin_and_falls_under_a_wrong_pose():
    from livingscenes_amd import ops
    solver = _solver(object())
    views, ref, _ = _views_scene()
    fusion = solver._fusion_grids([c for c in ref], 32, 4)
    fusion["sum"], fusion["n"] = ops.tsdf_state(len(views), fusion.pop("dims"), _dev())
    solver._fuse_batch(fusion, views, empty="free")
    tol = 0.02
    slots = views
    figures = {}
    for name, T in (("true", None), ("wrong", _shifted(fusion, views))):
        pred = solver._predict_views_batch(fusion, slots, T)
        assert all(tuple(q["depth"].shape) == tuple(v["depth"].shape) and q["cam_to_world"].dtype == torch.float64 for q, v in zip(pred, views))
        want = _twin_agreement(fusion, slots, pred, tol)
        got = solver._view_agreement_batch(fusion, slots, T, tol=tol)
        for p, (agree, through, in_front, cnt) in enumerate(want):
            assert got["agree"][p] == agree and got["through"][p] == through and got["in_front"][p] == in_front, (name, p, got["agree"][p], agree)
            assert np.array_equal(got["counts"][p], cnt), (name, p)
            print(f"{name} pose, slot {p}: agree {agree}, through {through}, in_front {in_front}, counts {cnt.tolist()}")
        figures[name] = [w[0] for w in want]
    for p in range(len(views)):                                                # asserted on the twin; the device only by equality with it
        assert figures["true"][p] is not None and figures["wrong"][p] is not None and figures["wrong"][p] < figures["true"][p], (p, figures)
    # a slot without views, and g in the place of T: the same numbers
    half = solver._view_agreement_batch(fusion, [views[0], None], None, tol=tol)
    assert half["agree"][1] is None and half["counts"][1] is None and half["through"][1] is None
    assert half["agree"][0] == figures["true"][0]
    with pytest.raises(ValueError, match="not both"):
        solver._view_agreement_batch(fusion, views, _shifted(fusion, views), _shifted(fusion, views), tol=tol)
    # what the raycast predicts goes straight back into the fuse: the state it came from takes it without a complaint
    pred = solver._predict_views_batch(fusion, views)
    back = ops.depth_points(pred[0]["depth"][:1], views[0]["intrinsics"], pred[0]["cam_to_world"][:1])[0][0]
    assert back.shape[0] == int((pred[0]["state"][0] == tro.HIT).sum())


def test_solve_sequence_view_gate(small_prior, monkeypatch):
    from livingscenes_amd.lib_more import more_solver
    solver = _solver(small_prior)
    n, h, res, tol = 2, 0.02, 32, 0.02
    views, ref, rescan = _views_scene(n)
    dev = _dev()
    scene = dict(_scene(ref), views=views)
    _, start = more_solver.solve_sequence(solver, scene, [], voxel=h, fuse_res=res, fuse_empty="free")      # the state before the rescan is fused
    before = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in start["fusion"].items()}
    wrong = _shifted(before, views).to(torch.float32)
    Rt = torch.eye(4, device=dev).repeat(n, 1, 1)
    Rt[1] = wrong[1]                                                          # slot 1 comes with the wrong registration
    monkeypatch.setattr(solver, "_solve_object_matching", lambda *a, **k: {"matches0": torch.arange(n, device=dev)})
    monkeypatch.setattr(solver, "_solve_pairwise_registration_batch",
                        lambda src, tgt, **k: (Rt[:len(src), :3, :3].contiguous(), Rt[:len(src), :3, 3:].contiguous()))
    seen = {"agree": [], "predict": []}
    for name, key in (("_view_agreement_batch", "agree"), ("_predict_views_batch", "predict")):
        def spy(*a, _real=getattr(solver, name), _key=key, **kw):
            out = _real(*a, **kw)
            seen[_key].append((a, kw, out))
            return out
        monkeypatch.setattr(solver, name, spy)
    rescans = [dict(_scene(rescan), views=views)]
    base_steps, base = more_solver.solve_sequence(solver, scene, rescans, voxel=h, fuse_res=res, fuse_empty="free")
    assert not seen["agree"] and not seen["predict"] and set(base_steps[0]) == STEP_KEYS | {"n_fused_views"}      # without the arguments: as before
    steps, memory = more_solver.solve_sequence_view_gated(solver, scene, rescans, voxel=h, fuse_res=res, fuse_empty="free", view_tol=tol)
    assert len(seen["agree"]) == 1 and len(seen["predict"]) == 1                                                  # ONE call per step
    st = steps[0]
    assert set(st) == STEP_KEYS | {"n_fused_views", "view_agree", "view_through", "view_in_front"}
    _step_values_equal(st, base_steps[0])                                      # reported, nothing gated: every other value as without it
    assert st["n_fused_views"] == base_steps[0]["n_fused_views"] and torch.equal(memory["fusion"]["sum"], base["fusion"]["sum"])
    (fusion_arg, slot_views), kw, _ = seen["agree"][0]
    assert kw["tol"] == tol and kw["min_obs"] == 1 and kw.get("g") is None and torch.equal(kw["T"].to(torch.float32)[:, :3], Rt[:, :3])
    want = _twin_agreement(before, views, seen["predict"][0][2], tol)
    for i in range(n):
        assert st["view_agree"][i] == want[i][0] and st["view_through"][i] == want[i][1] and st["view_in_front"][i] == want[i][2], (i, st["view_agree"], want[i])
        print(f"slot {i}: view_agree {st['view_agree'][i]}, through {st['view_through'][i]}, in_front {st['view_in_front'][i]}")
    assert want[1][0] < want[0][0], (want[0][0], want[1][0])                   # on the twin: the wrong pose agrees less
    bar = 0.5 * (want[0][0] + want[1][0])
    steps, memory = more_solver.solve_sequence_view_gated(solver, scene, rescans, voxel=h, fuse_res=res, fuse_empty="free", view_tol=tol, min_view_agreement=bar)
    st = steps[0]
    assert st["rejected"] == [1] and st["n_fused_views"] == [views[0]["depth"].shape[0], 0] and st["n_new_points"][1] == 0
    assert torch.equal(memory["fusion"]["sum"][1], before["sum"][1]) and torch.equal(memory["fusion"]["n"][1], before["n"][1])
    assert torch.equal(memory["fusion"]["sum"][0], base["fusion"]["sum"][0]) and torch.equal(memory["clouds"][1], start["clouds"][1])
    # both gates: a pair must pass both
    steps, _ = more_solver.solve_sequence_view_gated(solver, scene, rescans, voxel=h, fuse_res=res, fuse_empty="free", view_tol=tol, min_view_agreement=bar,
                                          overlap_radius=0.04, min_overlap=2.0)
    assert steps[0]["rejected"] == [0, 1] and steps[0]["n_fused_views"] == [0, 0]
    monkeypatch.undo()
