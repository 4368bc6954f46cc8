"""GPU tests of the scene memory's sampling of a fused state and of the registration on it (csrc/tsdficp.hip: ls_tsdf_sample_f32 /
ls_tsdf_icp_f32 and their batch forms; ops.tsdf_sample*, ops.tsdf_icp*) and of the layers on top (More_Solver._refine_on_fusion_batch,
solve_sequence(refine_metric="tsdf")).

Sample.  phi, grad, state and counts must EQUAL tests/tsdf_sample_oracle.py bit for bit: the kernel is a loop around csrc/tsdfsample_plan.h,
which tests/test_tsdf_sample_cpu.py holds to the same twin on the host, nothing is contracted and there is no transcendental in it.
sum_phi2 equals the twin's chunk-ordered sum bit for bit, alone and in a batch.  The states, grids and queries are those of
tests/test_tsdf_sample_cpu.py, whose docstring says what they cover and where the precondition (every state holds OUT, UNSEEN and SAMPLED
queries) can hold.

ICP.  Held to the twin STEP BY STEP with the protocol and the tolerances of tests/test_hip_cloud_plane.py (the solver text is the same,
csrc/se3_gn.h): at every traced g_k the twin's sample gives the same f, w and states; Q within w 2^-52 Q of the twin's math.fsum; the
twin's update from its own sums gives g_{k+1}: R within 2^-23 per entry, t_a within 2^-23 (|t_a| + sum_b |c_b|) with c the centroid of
the posed SAMPLED queries; g_k orthonormal to 2^-22; asserted on the twin: the smallest Cholesky pivot ratio >= 1e-8.  stop / iters are
re-derived from the device's own traced statistics; the final sample is compared bit for bit with ops.tsdf_sample at g_out."""
import functools

import numpy as np
import pytest
import torch

import icp_oracle as io
import plane_icp_oracle as po
import tsdf_sample_oracle as tso
from cloud_testlib import GATE_KEYS, REFINE_KEYS, STEP_KEYS, F, _bits, _dev, _g, _scene, _solver, _t, small_prior  # noqa: F401 (a fixture)
from test_hip_cloud_icp import _step_values_equal
from test_tsdf_sample_cpu import COUNTS, DIMS, KINDS, expected, queries_of, state_of

pytestmark = pytest.mark.gpu


def _state(state):
    return tuple(torch.from_numpy(np.array(t, np.int32)).to(_dev()) for t in state)


def _b64(x):
    return np.ascontiguousarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x, np.float64).view(np.uint64)


def _host(res):
    return {k: v.cpu().numpy() if torch.is_tensor(v) else v for k, v in res.items()}


def _sample(state, B, g, origin, h, trunc, min_obs=1):
    from livingscenes_amd import ops
    phi, grad, st, counts, q = ops.tsdf_sample(_state(state), _t(B), g=_g(g), origin=origin, voxel=h, trunc=trunc, min_obs=min_obs)
    b = np.asarray(B).reshape(-1, 3).shape[0]
    assert phi.dtype == torch.float64 and grad.dtype == torch.float64 and st.dtype == torch.uint8 and counts.dtype == np.int64 and isinstance(q, float)
    assert tuple(phi.shape) == (b,) and tuple(grad.shape) == (b, 3) and tuple(st.shape) == (b,) and counts.shape == (3,)
    return {"phi": phi.cpu().numpy(), "grad": grad.cpu().numpy(), "state": st.cpu().numpy(), "counts": counts, "sum_phi2": q}


def _prefix(want, b):
    """the twin's sample of the first b queries from its sample of all of them: a query's outputs do not depend on the others"""
    st, phi = want["state"][:b], want["phi"][:b]
    counts = np.array([np.isfinite(want["y"][:b]).all(1).sum(), (st != tso.OUT).sum(), (st == tso.SAMPLED).sum()], np.int64)
    return {"phi": phi, "grad": want["grad"][:b], "state": st, "counts": counts, "sum_phi2": tso.chunk_sum(np.where(st == tso.SAMPLED, phi * phi, 0.0))}


def _same_sample(got, tw, what=""):
    assert np.array_equal(got["state"], tw["state"]), (what, "state", np.flatnonzero(got["state"] != tw["state"])[:5])
    assert np.array_equal(_b64(got["phi"]), _b64(tw["phi"])), (what, "phi")
    assert np.array_equal(_b64(got["grad"]), _b64(tw["grad"])), (what, "grad")
    assert np.array_equal(got["counts"], tw["counts"]), (what, got["counts"], tw["counts"])
    assert np.float64(got["sum_phi2"]).view(np.uint64) == np.float64(tw["sum_phi2"]).view(np.uint64), (what, got["sum_phi2"], tw["sum_phi2"])


# ------------------------------------------------------------------------------------------------ the sample
@pytest.mark.parametrize("b", COUNTS)
@pytest.mark.parametrize("dims", DIMS)
def test_sample_equals_the_twin(dims, b):
    for kind in KINDS:
        state, origin, h, trunc = state_of(kind, dims)
        for min_obs in (1, 2):
            for posed in (False, True):
                B, g, want = expected(kind, dims, min_obs, posed)
                if b == 513 and dims != (2, 2, 2):                        # the precondition, asserted again where it is used
                    assert set(np.unique(want["state"]).tolist()) == {tso.OUT, tso.UNSEEN, tso.SAMPLED}
                _same_sample(_sample(state, B[:b], g, origin, h, trunc, min_obs), _prefix(want, b), (kind, dims, min_obs, posed, b))


def test_sample_without_a_cell_or_an_observation():
    S, N = state_of("holes", (9, 8, 7))[0]
    _, origin, h, trunc = state_of("holes", (9, 8, 7))
    B = queries_of("holes", (9, 8, 7), 1)
    for state in ((S[:1], N[:1]), (S[:, :1], N[:, :1]), (np.zeros_like(S), np.zeros_like(N))):
        state = tuple(np.ascontiguousarray(t) for t in state)
        got = _sample(state, B, None, origin, h, trunc)
        _same_sample(got, tso.sample(state, B, None, origin, h, trunc), str(state[0].shape))
        assert got["counts"][2] == 0 and (got["phi"] == trunc).all() and not got["grad"].any() and got["sum_phi2"] == 0.0
    empty = _sample((S, N), np.zeros((0, 3), F), None, origin, h, trunc)
    assert empty["counts"].tolist() == [0, 0, 0] and empty["sum_phi2"] == 0.0


@functools.lru_cache(maxsize=None)
def _batch():
    """P = 5 on dims (9, 8, 7): a sphere; a problem without queries; an all-zero state; a one-query problem; the holes on their own grid"""
    dims = (9, 8, 7)
    probs = []
    for kind, b, posed in (("sphere", 513, True), ("box", 0, False), ("zero", 300, False), ("box", 1, False), ("holes", 257, True)):
        state, origin, h, trunc = state_of("box" if kind == "zero" else kind, dims)
        if kind == "zero":
            state = tuple(np.zeros_like(t) for t in state)
        B, g, _ = expected("box" if kind == "zero" else kind, dims, 1, posed)
        probs.append((state, B[:b], io.pose0(g), origin, h, trunc))
    return probs


def _run_sample_batch(probs, packed=False, min_obs=1):
    from livingscenes_amd import ops
    S = torch.stack([_state(p[0])[0] for p in probs])
    N = torch.stack([_state(p[0])[1] for p in probs])
    return ops.tsdf_sample_batch((S, N), [_t(p[1]) for p in probs], g=_g(np.stack([p[2] for p in probs])), origin=np.stack([p[3] for p in probs]),
                                 voxel=[p[4] for p in probs], trunc=[p[5] for p in probs], min_obs=min_obs, packed=packed)


def test_sample_batch_is_the_single_op():
    from livingscenes_amd import _lib, ops
    probs = _batch()
    P = len(probs)
    assert P == 5 and [len(p[1]) for p in probs] == [513, 0, 300, 1, 257]
    res = _run_sample_batch(probs)
    rev = _run_sample_batch(probs[::-1])[::-1]
    for p in range(P):
        got = dict(zip(("phi", "grad", "state", "counts", "sum_phi2"), res[p]))
        got = _host(got)
        alone = _sample(*probs[p])
        _same_sample(got, alone, f"problem {p} alone")
        _same_sample(_host(dict(zip(("phi", "grad", "state", "counts", "sum_phi2"), rev[p]))), alone, f"problem {p} reversed")
        _same_sample(got, tso.sample(*probs[p]), f"problem {p}, the twin: counts and the chunk-ordered sum")
    assert res[1][3].tolist() == [0, 0, 0] and res[2][3][2] == 0 and res[2][3][1] > 0 and res[0][3][2] > 0 and res[4][3][2] > 0
    phi, grad, st, counts, q, off = _run_sample_batch(probs, packed=True)
    assert off.tolist() == [0, 513, 513, 813, 814, 1071] and tuple(counts.shape) == (P, 3) and q.shape == (P,)
    assert torch.equal(phi, torch.cat([x[0] for x in res])) and torch.equal(grad, torch.cat([x[1] for x in res])) and torch.equal(st, torch.cat([x[2] for x in res]))
    two = _run_sample_batch(probs, min_obs=2)
    for p in (0, 4):
        _same_sample(_host(dict(zip(("phi", "grad", "state", "counts", "sum_phi2"), two[p]))), tso.sample(*probs[p], min_obs=2), f"problem {p}, min_obs 2")
    state, B, g, origin, h, trunc = probs[0]
    with pytest.raises(_lib.LsError, match="problem 3.*voxel"):
        ops.tsdf_sample_batch((torch.stack([_state(p[0])[0] for p in probs]), torch.stack([_state(p[0])[1] for p in probs])), [_t(p[1]) for p in probs],
                              origin=origin, voxel=[h, h, h, float("nan"), h], trunc=trunc)
    with pytest.raises(ValueError, match="min_obs"):
        ops.tsdf_sample(_state(state), _t(B), origin=origin, voxel=h, trunc=trunc, min_obs=0)
    with pytest.raises(_lib.LsError, match="no CPU fallback"):
        ops.tsdf_sample(_state(state), torch.zeros(3, 3), origin=origin, voxel=h, trunc=trunc)
    with pytest.raises(_lib.LsError, match="no CPU fallback"):
        ops.tsdf_sample(tuple(torch.from_numpy(np.array(t, np.int32)) for t in state), _t(B), origin=origin, voxel=h, trunc=trunc)
    with pytest.raises(ValueError):
        ops.tsdf_sample_batch((torch.stack([_state(p[0])[0] for p in probs]), torch.stack([_state(p[0])[1] for p in probs])), [_t(B)] * 4,
                              origin=origin, voxel=h, trunc=trunc)


# ------------------------------------------------------------------------------------------------ the ICP, P = 1
ICP_DIMS = (17, 16, 33)
BOX = np.array([0.15, 0.11, 0.3])


def _rodrigues(axis, deg):
    w = np.asarray(axis, np.float64)
    w = w / np.linalg.norm(w) * np.deg2rad(deg)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    th = np.linalg.norm(w)
    return np.eye(3) if th == 0 else np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)


BOX_R = _rodrigues([1.0, 2.0, -1.5], 25.0)


@functools.lru_cache(maxsize=None)
def _solid(kind):
    """hand-made states on the dyadic grid of dims (17, 16, 33), every sample observed twice except where noted:
    box: the signed distance of a box that is not aligned with the axes, all six faces inside the grid, truncated and quantised as the
    fusion does; the samples deeper than trunc inside are unobserved.  plane: D = (z - z0) / trunc: all gradients parallel."""
    _, origin, h, trunc = state_of("sphere", ICP_DIMS)
    idx = np.stack(np.meshgrid(*(np.arange(d) for d in ICP_DIMS), indexing="ij"), -1).astype(np.float64)
    x = origin + h * idx
    centre = origin + h * (np.array(ICP_DIMS) - 1) / 2
    if kind == "box":
        q = np.abs((x - centre) @ BOX_R) - BOX                            # the box frame: columns of BOX_R are its axes
        sdf = np.linalg.norm(np.maximum(q, 0), axis=-1) + np.minimum(q.max(-1), 0)
    else:
        sdf = x[..., 2] - (centre[2] + 0.013)
    N = np.where(sdf < -trunc, 0, 2) if kind == "box" else np.full(ICP_DIMS, 2)
    S = np.floor(np.clip(sdf / trunc, -1, 1) * 16384 + 0.5).astype(np.int64) * N
    state = (S.astype(np.int32), N.astype(np.int32))
    for t in state:
        t.setflags(write=False)
    return state, origin, h, trunc, centre


def _box_points(b, seed):
    """b points on the six faces of the box of _solid('box'), in the grid's frame, with a millimetre of noise"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-1, 1, (b, 3)) * BOX
    face = rng.integers(0, 6, b)
    p[np.arange(b), face % 3] = np.where(face < 3, 1.0, -1.0) * BOX[face % 3]
    centre = _solid("box")[4]
    return (centre + p @ BOX_R.T + rng.normal(0, 0.0005, (b, 3))).astype(F)


def _start(centre, deg, shift, seed=0):
    """a pose [3,4] fp32 that turns by deg about the centre and moves by `shift` metres"""
    rng = np.random.default_rng(100 + seed)
    R = _rodrigues(rng.normal(size=3), deg)
    d = rng.normal(size=3)
    return np.concatenate([R, (centre - R @ centre + shift * d / np.linalg.norm(d))[:, None]], 1).astype(F)


def _icp(state, B, g0, origin, h, trunc, trace=True, **kw):
    from livingscenes_amd import ops
    res = ops.tsdf_icp(_state(state), _t(B), g=_g(g0), origin=origin, voxel=h, trunc=trunc, trace=trace, **kw)
    assert res["g"].dtype == torch.float32 and tuple(res["g"].shape) == (3, 4) and res["state"].dtype == torch.uint8
    assert all(isinstance(res[k], int) for k in ("stop", "iters")) and isinstance(res["sum_phi2"], float)
    return _host(res)


def _identical(x, y, what=""):
    assert (x["stop"], x["iters"]) == (y["stop"], y["iters"]), (what, x["stop"], y["stop"], x["iters"], y["iters"])
    assert np.array_equal(_bits(x["g"]), _bits(y["g"])), (what, "g")
    _same_sample(x, y, what)
    if "g_trace" in x and "g_trace" in y:
        k = x["iters"] + 1
        assert np.array_equal(_bits(x["g_trace"][:k]), _bits(y["g_trace"][:k])), (what, "g_trace")
        assert np.array_equal(x["stat_trace"][:k].view(np.uint64), y["stat_trace"][:k].view(np.uint64)), (what, "stat_trace")


def _steps(state, B, g0, origin, h, trunc, res, min_obs=1, max_iter=100, rel_thr=1e-6, min_matched=6, what=""):
    """the per-step check of the module docstring -> the device's E_k, k <= iters"""
    B = np.asarray(B, np.float32).reshape(-1, 3)
    iters, stop = res["iters"], res["stop"]
    assert 0 <= iters <= max_iter, (what, iters)
    gt, st = res["g_trace"].reshape(-1, 3, 4), res["stat_trace"]
    assert gt.shape[0] == st.shape[0] == max_iter + 1 and st.shape[1] == 3
    assert np.array_equal(_bits(gt[0]), _bits(io.pose0(g0))), (what, "g_0 is g0 (None: the identity matrix)")
    assert np.array_equal(_bits(res["g"]), _bits(gt[iters])), (what, "g_out is g_k of the stop")
    assert not _bits(gt[iters + 1:]).any() and not st[iters + 1:].any(), (what, "trace rows past the stop are left alone")
    E, E_prev = [], 0.0
    for k in range(iters + 1):
        R = gt[k][:, :3].astype(np.float64)
        if np.isfinite(R).all() and k > 0:
            assert np.abs(R @ R.T - np.eye(3)).max() <= 2.0 ** -22, (what, k, "g_k is orthonormal to fp32 rounding")
        tw = tso.step(state, B, gt[k], origin, h, trunc, min_obs)
        f, w, Q = st[k]
        assert (f, w) == (tw["f"], tw["w"]), (what, k, "f, w", f, w, tw["f"], tw["w"])
        assert abs(Q - tw["Q"]) <= tw["w"] * 2.0 ** -52 * tw["Q"], (what, k, "Q", Q, tw["Q"])
        E.append(tso.cost(int(f), int(w), float(Q), trunc))
        why = po.stop_rule(k, int(w), E[k], E_prev, max_iter, rel_thr, min_matched)
        if k < iters:
            assert why is None, (what, k, "the device went on where the rule stops", why)
            assert tw["g_next"] is not None and tw["pivot"] >= 1e-8, (what, k, "the twin's M is ill-conditioned: a case of its own", tw["pivot"])
            Rd, td, Rt, tt = gt[k + 1][:, :3], gt[k + 1][:, 3], tw["g_next"][:, :3], tw["g_next"][:, 3]
            assert np.abs(Rd.astype(np.float64) - Rt).max() <= 2.0 ** -23, (what, k, "R", np.abs(Rd.astype(np.float64) - Rt).max())
            c = tw["y"][tw["state"] == tso.SAMPLED].astype(np.float64).mean(0)
            tol = 2.0 ** -23 * (np.abs(tt.astype(np.float64)) + np.abs(c).sum())
            assert (np.abs(td.astype(np.float64) - tt) <= tol).all(), (what, k, "t", td, tt, tol)
            E_prev = E[k]
        else:
            assert np.array_equal(res["state"], tw["state"]), (what, "the final states")
            assert (int(res["counts"][0]), int(res["counts"][2]), res["sum_phi2"]) == (int(f), int(w), float(Q)), (what, "the final (f, w, Q)")
            if why is None:                                              # the rule goes on: only a failed solve stops here
                assert stop == tso.DEGENERATE and tw["g_next"] is None, (what, k, stop)
            else:
                assert stop == why, (what, k, stop, why)
    return E


def _final(state, B, origin, h, trunc, res, min_obs=1, what=""):
    """the final sample: bit for bit ops.tsdf_sample at g_out, and the twin's"""
    got = _sample(state, B, res["g"], origin, h, trunc, min_obs)
    _same_sample(res, got, what + ": the final sample is ops.tsdf_sample at g_out")
    _same_sample(res, tso.sample(state, B, res["g"], origin, h, trunc, min_obs), what + ": and the twin's")


@pytest.mark.parametrize("posed", (False, True))
@pytest.mark.parametrize("b", (0, 5, 255, 256, 257, 513))
def test_icp_size_edges(b, posed):
    state, origin, h, trunc, centre = _solid("box")
    B = _box_points(b, b)
    g0 = _start(centre, 2.0, 0.3 * trunc, b) if posed else None
    res = _icp(state, B, g0, origin, h, trunc, max_iter=4)
    _steps(state, B, g0, origin, h, trunc, res, max_iter=4, what=f"b = {b}")
    _final(state, B, origin, h, trunc, res, what=f"b = {b}")
    if b <= 5:
        assert res["stop"] == tso.STARVED and res["iters"] == 0 and np.array_equal(_bits(res["g"]), _bits(io.pose0(g0)))
    else:
        assert res["iters"] >= 1 and res["stop"] in (tso.CONVERGED, tso.MAX_ITER) and res["counts"][2] > 0.5 * b
        untraced = _icp(state, B, g0, origin, h, trunc, trace=False, max_iter=4)      # the trace is an observer: the same bits without it
        assert "g_trace" not in untraced
        _identical(untraced, res, f"b = {b} untraced")
    zero = _icp(state, B, g0, origin, h, trunc, max_iter=0)               # max_iter 0: one sample, no update
    assert zero["iters"] == 0 and zero["stop"] == (tso.MAX_ITER if zero["counts"][2] >= 6 else tso.STARVED)
    assert np.array_equal(_bits(zero["g"]), _bits(io.pose0(g0)))
    _final(state, B, origin, h, trunc, zero, what=f"b = {b} max_iter 0")


def test_icp_every_stop_reason():
    state, origin, h, trunc, centre = _solid("box")
    B = _box_points(600, 1)
    g0 = _start(centre, 2.0, 0.4 * trunc, 1)
    # CONVERGED, and closer than it started
    res = _icp(state, B, g0, origin, h, trunc)
    E = _steps(state, B, g0, origin, h, trunc, res, what="converged")
    _final(state, B, origin, h, trunc, res, what="converged")
    move = lambda g: float(np.linalg.norm(io.images(B, g).astype(np.float64) - B.astype(np.float64), axis=1).mean())   # noqa: E731
    print(f"box: iters {res['iters']} stop {res['stop']} E {E[0]:.4e} -> {E[-1]:.4e}; mean distance to the true place {move(g0):.3e} -> {move(res['g']):.3e}")
    assert res["stop"] == tso.CONVERGED and 2 <= res["iters"] <= 30 and move(res["g"]) < 0.2 * move(g0) and E[-1] < E[0]
    # MAX_ITER at max_iter 1 (max_iter 0: test_icp_size_edges): one update, then the stop at k = 1
    one = _icp(state, B, g0, origin, h, trunc, max_iter=1)
    _steps(state, B, g0, origin, h, trunc, one, max_iter=1, what="one update")
    assert one["stop"] == tso.MAX_ITER and one["iters"] == 1 and np.array_equal(_bits(one["g"]), _bits(res["g_trace"].reshape(-1, 3, 4)[1]))
    # STARVED: every query UNSEEN
    blank = tuple(np.zeros_like(t) for t in state)
    for g in (None, g0):                                                  # under the identity every row lies inside the grid
        res = _icp(blank, B, g, origin, h, trunc, max_iter=5)
        _steps(blank, B, g, origin, h, trunc, res, max_iter=5, what="starved")
        assert res["stop"] == tso.STARVED and res["iters"] == 0 and res["counts"][2] == 0 and (res["state"] != tso.SAMPLED).all()
        assert np.array_equal(_bits(res["g"]), _bits(io.pose0(g)))
        if g is None:
            assert (res["state"] == tso.UNSEEN).all() and res["counts"].tolist() == [600, 600, 0]
    nan_pose = g0.copy()
    nan_pose[1, 3] = np.nan                                               # every query non-finite: f = 0, E = 0, starved
    nothing = _icp(state, B, nan_pose, origin, h, trunc, max_iter=5)
    assert nothing["stop"] == tso.STARVED and nothing["counts"].tolist() == [0, 0, 0] and nothing["sum_phi2"] == 0.0
    # DEGENERATE: the state of one plane, all gradients parallel
    plane, origin, h, trunc, centre = _solid("plane")
    rng = np.random.default_rng(3)
    Bp = (centre + np.concatenate([rng.uniform(-0.2, 0.2, (700, 2)), rng.uniform(-0.3, 0.3, (700, 1)) * trunc + 0.013], 1)).astype(F)
    for g in (None, F([[1, 0, 0, 0.001], [0, 1, 0, 0], [0, 0, 1, 0.004]])):
        res = _icp(plane, Bp, g, origin, h, trunc, max_iter=5)
        _steps(plane, Bp, g, origin, h, trunc, res, max_iter=5, what="one plane")
        _final(plane, Bp, origin, h, trunc, res, what="one plane")
        assert res["stop"] == tso.DEGENERATE and res["iters"] == 0 and res["counts"][2] >= 600
        assert np.array_equal(_bits(res["g"]), _bits(io.pose0(g)))
        sampled = res["state"] == tso.SAMPLED
        assert not res["grad"][sampled][:, :2].any() and (res["grad"][sampled][:, 2] > 0.9).all()


# ------------------------------------------------------------------------------------------------ the ragged batch
@functools.lru_cache(maxsize=None)
def _icp_batch():
    box, origin, h, trunc, centre = _solid("box")
    plane = _solid("plane")[0]
    blank = tuple(np.zeros_like(t) for t in box)
    rng = np.random.default_rng(3)
    Bp = (centre + np.concatenate([rng.uniform(-0.2, 0.2, (300, 2)), rng.uniform(-0.3, 0.3, (300, 1)) * trunc + 0.013], 1)).astype(F)
    eye = io.IDENTITY
    probs = [(blank, _box_points(300, 7), eye), (box, np.zeros((0, 3), F), eye), (plane, Bp, eye)]
    for b, deg, shift, seed in ((257, 0.5, 0.1, 2), (1200, 2.0, 0.4, 3), (600, 3.0, 0.3, 4), (513, 1.0, 0.45, 5)):
        probs.append((box, _box_points(b, seed), _start(centre, deg, shift * trunc, seed)))
    return probs, origin, h, trunc


def _run_icp_batch(probs, origin, h, trunc, packed=False, **kw):
    from livingscenes_amd import ops
    S = torch.stack([_state(p[0])[0] for p in probs])
    N = torch.stack([_state(p[0])[1] for p in probs])
    return ops.tsdf_icp_batch((S, N), [_t(p[1]) for p in probs], g=_g(np.stack([p[2] for p in probs])), origin=origin, voxel=h, trunc=trunc,
                              trace=True, packed=packed, **kw)


def test_icp_batch_is_the_single_op_in_any_order_and_run():
    probs, origin, h, trunc = _icp_batch()
    P = len(probs)
    assert P == 7
    kw = {"max_iter": 12}
    res = [_host(x) for x in _run_icp_batch(probs, origin, h, trunc, **kw)]
    alone = [_icp(p[0], p[1], p[2], origin, h, trunc, **kw) for p in probs]
    for p in range(P):
        _identical(res[p], alone[p], f"problem {p} alone")
    rev = [_host(x) for x in _run_icp_batch(probs[::-1], origin, h, trunc, **kw)]
    again = [_host(x) for x in _run_icp_batch(probs, origin, h, trunc, **kw)]
    for p in range(P):
        _identical(rev[P - 1 - p], res[p], f"problem {p} reversed")
        _identical(again[p], res[p], f"problem {p} again")
    iters, stops = [x["iters"] for x in res], [x["stop"] for x in res]
    print("batch iters", iters, "stop", stops)
    assert stops[:3] == [tso.STARVED, tso.STARVED, tso.DEGENERATE] and iters[:3] == [0, 0, 0]
    assert len(set(iters)) >= 3 and min(iters[3:]) >= 1, iters           # problems stop at different k: the stopped ones stay frozen
    cut = sorted(set(iters[3:]))[1]                                      # whoever stopped before `cut` keeps its bits while the others run on
    short = [_host(x) for x in _run_icp_batch(probs, origin, h, trunc, max_iter=cut)]
    assert sum(x["iters"] < cut for x in res[3:]) >= 1
    for p in range(P):
        if res[p]["iters"] < cut:
            _identical({k: v for k, v in short[p].items() if "trace" not in k}, res[p], f"problem {p}, a shorter run")
            assert np.array_equal(_bits(short[p]["g_trace"][:res[p]["iters"] + 1]), _bits(res[p]["g_trace"][:res[p]["iters"] + 1]))
    _steps(probs[5][0], probs[5][1], probs[5][2], origin, h, trunc, res[5], what="batch problem 5", **kw)
    _final(probs[6][0], probs[6][1], origin, h, trunc, res[6], what="batch problem 6")
    pk = _run_icp_batch(probs, origin, h, trunc, packed=True, **kw)      # the packed form: the same result
    assert pk["b_off"].tolist() == np.cumsum([0] + [p[1].shape[0] for p in probs]).tolist() and tuple(pk["g"].shape) == (P, 3, 4)
    assert pk["stop"].dtype == np.int32 and pk["stop"].tolist() == stops and pk["iters"].tolist() == iters
    assert np.array_equal(_bits(pk["g"]), _bits(np.stack([x["g"] for x in res]))) and np.array_equal(pk["counts"], np.stack([x["counts"] for x in res]))
    assert np.array_equal(_b64(pk["phi"]), _b64(np.concatenate([x["phi"] for x in res]))) and pk["sum_phi2"].tolist() == [x["sum_phi2"] for x in res]


def test_icp_errors_name_the_problem():
    from livingscenes_amd import _lib, ops
    probs, origin, h, trunc = _icp_batch()
    S = torch.stack([_state(p[0])[0] for p in probs])
    N = torch.stack([_state(p[0])[1] for p in probs])
    Bs = [_t(p[1]) for p in probs]
    with pytest.raises(_lib.LsError, match="problem 4.*trunc"):
        ops.tsdf_icp_batch((S, N), Bs, origin=origin, voxel=h, trunc=[trunc] * 4 + [float("nan")] + [trunc] * 2)
    for kw, word in (({"max_iter": -1}, "max_iter"), ({"min_matched": 2}, "min_matched"), ({"rel_thr": -1.0}, "rel_thr")):
        with pytest.raises(_lib.LsError, match=word):
            ops.tsdf_icp_batch((S, N), Bs, origin=origin, voxel=h, trunc=trunc, **kw)
        with pytest.raises(_lib.LsError, match=word):
            ops.tsdf_icp((S[4], N[4]), Bs[4], origin=origin, voxel=h, trunc=trunc, **kw)
    with pytest.raises(_lib.LsError, match="no CPU fallback"):
        ops.tsdf_icp((S[4], N[4]), torch.zeros(3, 3), origin=origin, voxel=h, trunc=trunc)
    with pytest.raises(ValueError):
        ops.tsdf_icp_batch((S, N), Bs[:-1], origin=origin, voxel=h, trunc=trunc)


# ------------------------------------------------------------------------------------------------ a recovery check on fused partial views
RECOVERY_SEEDS = (0, 1, 2, 6)


def _angle(g):
    R = np.asarray(g, np.float64)[:, :3]
    return float(np.degrees(np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))))


def test_recovery_on_fused_partial_views():
    """A condition, not a measurement: 4 synth shapes rendered by make_partial_views(with_depth=True) and fused at res 32; the
    observation is one view's depth_points; the start is 2 degrees and trunc / 2 off the true pose (the identity); the final rotation
    error and the final rms phi are both below their starting values for every shape.  The NumPy twin alone must meet this on the same
    data (the precondition, asserted first); then the device, whose loop is held to the twin step by step above.  The seeds were chosen
    with the twin alone: of the seeds 0 .. 23 the twin lowers rms phi on all 24 but the rotation error only on 13 (0, 1, 2, 6, 12, 13,
    14, 18 - 23) -- on the others a state fused from three views lets the partial view slide to a pose that fits the field better and
    the truth worse (2 degrees -> 2.3 .. 14.0).  That is what the loop does on such states, not a defect of the kernels, and it is why
    no setting is recommended."""
    from livingscenes_amd import ops, render, synth
    from livingscenes_amd.lib_more.more_solver import More_Solver
    dev = _dev()
    parts = synth.make_partial_views(RECOVERY_SEEDS, 3, res=32, with_depth=True, device=dev)
    clouds = [torch.cat(p["clouds"]) for p in parts]
    grids = More_Solver._fusion_grids(clouds, 32, 4)
    S, N = ops.tsdf_state(len(parts), grids["dims"], dev)
    ops.depth_fuse_batch((S, N), [p["depth"] for p in parts], [p["intrinsics"] for p in parts], [p["world_to_cam"] for p in parts],
                         origin=grids["origin"], voxel=grids["voxel"], trunc=grids["trunc"])
    Bs, g0s = [], []
    for k, p in enumerate(parts):
        pts, _ = ops.depth_points(p["depth"][:1], p["intrinsics"], torch.from_numpy(render.cam_to_world(p["poses"][0])[None]).to(dev))[0]
        assert torch.equal(pts, p["clouds"][0])                           # the first view's back-projection, in the shape's frame
        Bs.append(pts)
        g0s.append(_start(pts.double().mean(0).cpu().numpy(), 2.0, 0.5 * float(grids["trunc"][k]), RECOVERY_SEEDS[k]))
    res = ops.tsdf_icp_batch((S, N), Bs, g=_g(np.stack(g0s)), origin=grids["origin"], voxel=grids["voxel"], trunc=grids["trunc"], trace=True)
    Sh, Nh = S.cpu().numpy(), N.cpu().numpy()
    for k, r in enumerate(res):
        r = _host(r)
        o, h, tr = grids["origin"][k].numpy(), float(grids["voxel"][k]), float(grids["trunc"][k])
        tw = tso.icp((Sh[k], Nh[k]), Bs[k].cpu().numpy(), g0s[k], o, h, tr)
        rms = lambda f, w, q: float(np.sqrt(q / w)) if w else float("nan")   # noqa: E731
        t0, t1 = rms(*tw["stat_trace"][0]), rms(*tw["stat_trace"][-1])
        print(f"shape {k}: twin iters {tw['iters']} stop {tw['stop']} angle {_angle(g0s[k]):.3f} -> {_angle(tw['g']):.3f} deg, rms phi {t0:.3e} -> {t1:.3e}; "
              f"device iters {r['iters']} stop {r['stop']} angle {_angle(r['g']):.3f} deg, sampled {r['counts'][2]} of {r['counts'][0]}")
        assert _angle(tw["g"]) < _angle(g0s[k]) and t1 < t0, (k, "the twin alone misses the condition: choose other seeds")
        st = r["stat_trace"]
        d0, d1 = rms(*st[0]), rms(*st[r["iters"]])
        assert _angle(r["g"]) < _angle(g0s[k]) and d1 < d0, (k, _angle(r["g"]), d0, d1)
        assert r["iters"] >= 1 and r["stop"] in (tso.CONVERGED, tso.MAX_ITER)


# ------------------------------------------------------------------------------------------------ the layers above
def test_refine_on_fusion_batch():
    from livingscenes_amd import ops
    from livingscenes_amd.lib_math.torch_se3 import inverse
    solver = _solver(object())
    box, origin, h, trunc, centre = _solid("box")
    blank = tuple(np.zeros_like(t) for t in box)
    states = [box, box, blank]
    S = torch.stack([_state(s)[0] for s in states])
    N = torch.stack([_state(s)[1] for s in states])
    fusion = {"sum": S, "n": N, "origin": torch.from_numpy(np.tile(origin, (3, 1))), "voxel": torch.full((3,), h, dtype=torch.float64),
              "trunc": torch.full((3,), trunc, dtype=torch.float64)}
    news, Ts = [], []
    for k in range(3):
        g = _start(centre, 1.5 + k, 0.3 * trunc, 20 + k).astype(np.float64)
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = g[:, :3].T, -g[:, :3].T @ g[:, 3]           # memory -> rescan: the inverse of the pose the operator starts from
        news.append(_t(_box_points(500 + 10 * k, 30 + k)))
        Ts.append(T.astype(F))
    Ts[2] = Ts[2] + F(0.125)                                              # a starved slot keeps whatever T it came with, bit for bit
    T = torch.from_numpy(np.stack(Ts)).to(_dev())
    T2, info = solver._refine_on_fusion_batch(fusion, news, T, max_iter=30)
    assert set(info) == {"g", "stop", "iters", "sampled", "rms_phi", "counts"} and tuple(T2.shape) == (3, 4, 4)
    want = ops.tsdf_icp_batch((S, N), news, g=inverse(T), origin=fusion["origin"], voxel=fusion["voxel"], trunc=fusion["trunc"], max_iter=30, packed=True)
    assert torch.equal(info["g"], want["g"]) and info["stop"].tolist() == want["stop"].tolist() and info["iters"].tolist() == want["iters"].tolist()
    assert info["iters"][2] == 0 and info["stop"][2] == tso.STARVED and np.array_equal(_bits(T2[2]), _bits(T[2])) and info["sampled"][2] == 0.0
    assert np.isnan(info["rms_phi"][2])
    for k in range(2):
        print(f"pair {k}: iters {info['iters'][k]} stop {info['stop'][k]} sampled {info['sampled'][k]:.3f} rms phi {info['rms_phi'][k]:.3e}")
        assert info["iters"][k] >= 1 and np.array_equal(_bits(T2[k, :3]), _bits(inverse(info["g"][k:k + 1])[0]))
        assert info["sampled"][k] == want["counts"][k][2] / want["counts"][k][0] and info["rms_phi"][k] == float(np.sqrt(want["sum_phi2"][k] / want["counts"][k][2]))
    T3, _ = solver._refine_on_fusion_batch(fusion, news, T[:, :3], min_obs=2, max_iter=3)
    assert tuple(T3.shape) == (3, 4, 4)
    with pytest.raises(ValueError, match="observations"):
        solver._refine_on_fusion_batch(fusion, news[:2], T)


def test_solve_sequence_refine_metric_tsdf(small_prior, monkeypatch):
    from livingscenes_amd.lib_more import more_solver
    from test_hip_depth_fuse import _fusion_scene, _part_views
    solver = _solver(small_prior)
    n, h, res = 3, 0.02, 32
    parts, ref, rescan = _fusion_scene(n)
    views = [_part_views(p) for p in parts]
    dev = _dev()
    monkeypatch.setattr(solver, "_solve_object_matching", lambda *a, **k: {"matches0": torch.arange(n, device=dev)})
    off = [np.concatenate([_start(ref[i].double().mean(0).cpu().numpy(), 1.0, 0.01, i), [[0, 0, 0, 1]]]).astype(F) for i in range(n)]
    Rt = torch.from_numpy(np.stack(off)).to(dev)                          # memory -> rescan: a degree and a centimetre off the truth
    monkeypatch.setattr(solver, "_solve_pairwise_registration_batch",
                        lambda src, tgt, **k: (Rt[:len(src), :3, :3].contiguous(), Rt[:len(src), :3, 3:].contiguous()))
    seen = {"refine": [], "accumulate": [], "fuse": [], "overlap": []}
    for name, key in (("_refine_on_fusion_batch", "refine"), ("_accumulate_batch", "accumulate"), ("_fuse_batch", "fuse"), ("_overlap_batch", "overlap")):
        def spy(*a, _real=getattr(solver, name), _key=key, **kw):
            out = _real(*a, **kw)
            seen[_key].append((a, kw, out))
            return out
        monkeypatch.setattr(solver, name, spy)
    scene = dict(_scene(ref), views=views)
    base_steps, base = more_solver.solve_sequence(solver, scene, [dict(_scene(rescan), views=views)], voxel=h, fuse_res=res, fuse_empty="free")
    assert not seen["refine"] and set(base_steps[0]) == STEP_KEYS | {"n_fused_views"}
    again_steps, again = more_solver.solve_sequence(solver, scene, [dict(_scene(rescan), views=views)], voxel=h, fuse_res=res, fuse_empty="free",
                                                    refine_metric="point")
    _step_values_equal(again_steps[0], base_steps[0])                     # without the new option: equal to what it was
    assert torch.equal(again["fusion"]["sum"], base["fusion"]["sum"]) and torch.equal(again["fusion"]["n"], base["fusion"]["n"])
    for k in seen:
        seen[k].clear()
    steps, memory = more_solver.solve_sequence(solver, scene, [dict(_scene(rescan), views=views), dict(_scene(rescan), views=views)], voxel=h,
                                               fuse_res=res, fuse_empty="free", refine_metric="tsdf", overlap_radius=0.04, min_overlap=0.0)
    assert len(seen["refine"]) == 2 and len(steps) == 2                   # one refinement call per step
    for k, st in enumerate(steps):
        assert set(st) == STEP_KEYS | GATE_KEYS | REFINE_KEYS | {"n_fused_views"}
        (fusion, pcs, T_in), kw, (T_out, info) = seen["refine"][k]
        assert fusion["sum"].shape[0] == n and len(pcs) == n and kw == {"min_obs": 1}
        g_out = info["g"]
        for i in range(n):
            assert st["refine_stop"][i] in (0, 1, 2, 3) and st["refine_iters"][i] == int(info["iters"][i]) and 0.0 <= st["overlap"][i] <= 1.0
            assert torch.equal(st["registration_init"][i], Rt[i:i + 1]) and torch.equal(st["registration"][i], T_out[i:i + 1])
            print(f"step {k} slot {i}: tsdf refinement iters {st['refine_iters'][i]} stop {st['refine_stop'][i]} overlap {st['overlap'][i]:.3f}")
            if st["refine_iters"][i] == 0:                                # no fallback: the pose the pair came with
                assert torch.equal(st["registration"][i], st["registration_init"][i])
        assert any(it >= 1 for it in st["refine_iters"]), st["refine_iters"]
        # the gate searched on its own, and the merge and the fuse received the refined pose
        assert torch.equal(seen["overlap"][k][1]["g"], g_out) and seen["overlap"][k][0][2] is None
        merge = [c for c in seen["accumulate"] if c[1].get("g") is not None][k]
        assert torch.equal(merge[1]["g"], g_out)
        fuse = [c for c in seen["fuse"] if c[1].get("g") is not None][k]
        assert torch.equal(fuse[1]["g"].to(torch.float32), g_out.to(torch.float32)[:, :3]) and fuse[1].get("T") is None
    assert set(memory) == set(base) and len(memory["clouds"]) == n
    monkeypatch.undo()
