"""GPU tests of the scene memory's trimmed ICP (csrc/cloudnear.hip: ls_cloud_icp_f32 / ls_cloud_icp_batch_f32; ops.cloud_icp / cloud_icp_batch)
and of the layers on top of it (More_Solver._refine_on_memory_batch, solve_sequence(refine_radius=...)).

The operator is held to tests/icp_oracle.py STEP BY STEP (_steps): the device's trace gives its pose g_k at every iteration; the twin's search at
that g_k must give the same f_k and n_k as integers, and S_k within n_k 2^-52 S_k of the twin's math.fsum (the bound
tests/test_hip_cloud_nearest.py derives for a float64 sum of n non-negative terms against the correctly rounded one).  The twin's float64
update from its own correspondences then gives g_{k+1}: R must agree within 2^-23 per entry and t_a within 2^-23 (|t_a| + sum_b |mu_x b|).
Both sides solve in float64, so for a well-conditioned problem they differ by some 1e-13, far below an fp32 ulp; the two fp32 roundings can
then differ by one ulp at a rounding boundary (<= 2^-24 for |R| < 1; the products R mu_x carry it into t), and one more ulp is allowed.
"Well-conditioned" is asserted on the twin's H: sigma_0 / (sigma_1 + sigma_2) < 1e3 -- the rotation's sensitivity to a perturbation of H
is 1 / (sigma_1 + sigma_2), the smallest sum of two singular values, so a planar matched set (sigma_2 = 0: three points) is well-conditioned
and a collinear one is not; that one is a case of its own.  stop and iters must equal the stop rule re-evaluated in Python float64 from the
device's own traced (f, n, S): the same expression, so the same decision.  The final search is compared bit for bit with
ops.cloud_nearest at g_out and with the twin.  Between the single op and the batch every output is compared bit for bit.  The
solve_sequence tests run untrained weights with the registration replaced by perturbed ground truth, and make no accuracy claim."""
import math

import numpy as np
import pytest
import torch

import icp_oracle as io
import merge_oracle as mo
import nearest_oracle as no
from cloud_testlib import (CODE_KEYS, GATE_KEYS, REFINE_KEYS, STEP_KEYS, TILE, F, _bits, _dev, _g, _scene, _solver, _t,
                           small_prior)  # noqa: F401 (small_prior is a fixture)
from livingscenes_amd import synth
from test_cloud_icp_cpu import _inv, _pose, _rot, twin_bound, twin_case

pytestmark = pytest.mark.gpu


def _host(res):
    """a result dict of ops.cloud_icp with its tensors on the host"""
    assert res["g"].dtype == torch.float32 and tuple(res["g"].shape) == (3, 4) and res["idx"].dtype == torch.int32
    assert isinstance(res["stop"], int) and isinstance(res["iters"], int) and isinstance(res["sum_d2"], float)
    assert res["counts"].dtype == np.int64 and res["counts"].shape == (3,)
    return {k: v.cpu().numpy() if torch.is_tensor(v) else v for k, v in res.items()}


def _single(A, B, g0, r, trace=True, **kw):
    from livingscenes_amd import ops
    return _host(ops.cloud_icp(_t(A), _t(B), g=_g(g0), radius=r, trace=trace, **kw))


def _compose(d, g):
    """d o g for [3,4] poses in float64"""
    return np.concatenate([d[:, :3] @ g[:, :3], d[:, :3] @ g[:, 3:] + d[:, 3:]], 1)


def _identical(x, y, what=""):
    """two device results of one problem: every output the same bits"""
    assert x["stop"] == y["stop"] and x["iters"] == y["iters"], (what, x["stop"], y["stop"], x["iters"], y["iters"])
    assert np.array_equal(_bits(x["g"]), _bits(y["g"])), (what, "g")
    assert np.array_equal(x["idx"], y["idx"]) and np.array_equal(_bits(x["d2"]), _bits(y["d2"])) and np.array_equal(x["counts"], y["counts"]), what
    assert np.float64(x["sum_d2"]).view(np.uint64) == np.float64(y["sum_d2"]).view(np.uint64), (what, x["sum_d2"], y["sum_d2"])
    if "g_trace" in x and "g_trace" in y:
        k = x["iters"] + 1
        assert np.array_equal(_bits(x["g_trace"][:k]), _bits(y["g_trace"][:k])), (what, "g_trace")
        assert np.array_equal(x["stat_trace"][:k].view(np.uint64), y["stat_trace"][:k].view(np.uint64)), (what, "stat_trace")


def _steps(A, B, g0, r, res, max_iter=100, rel_thr=1e-6, min_matched=3, what=""):
    """the per-step check of the module docstring -> the device's E_k, k <= iters"""
    A, B = np.asarray(A, np.float32).reshape(-1, 3), np.asarray(B, np.float32).reshape(-1, 3)
    iters, stop = res["iters"], res["stop"]
    assert 0 <= iters <= max_iter, (what, iters)
    gt, st = res["g_trace"].reshape(-1, 3, 4), res["stat_trace"]
    assert gt.shape[0] == st.shape[0] == max_iter + 1
    assert np.array_equal(_bits(gt[0]), _bits(io.pose0(g0))), (what, "g_0 is g0 (None: the identity matrix)")
    assert np.array_equal(_bits(res["g"]), _bits(gt[iters])), (what, "g_out is g_k of the stop")
    assert not _bits(gt[iters + 1:]).any() and not st[iters + 1:].any(), (what, "trace rows past the stop are left alone")
    E, E_prev = [], 0.0
    for k in range(iters + 1):
        tw = io.step(A, B, gt[k], r)
        f, n, S = st[k]
        assert (f, n) == (tw["f"], tw["n"]), (what, k, "f, n", f, n, tw["f"], tw["n"])
        assert abs(S - tw["S"]) <= tw["n"] * 2.0 ** -52 * tw["S"], (what, k, "S", S, tw["S"])
        E.append(io.cost(int(f), int(n), float(S), r))
        why = io.stop_rule(k, int(n), E[k], E_prev, max_iter, rel_thr, min_matched)
        if k < iters:
            assert why is None, (what, k, "the device went on where the rule stops", why)
            assert tw["g_next"] is not None, (what, k)
            sg = np.linalg.svd(tw["H"], compute_uv=False)
            assert sg[0] / (sg[1] + sg[2]) < 1e3, (what, k, "the twin's H is ill-conditioned: a case of its own", sg)
            Rd, td, Rt, tt = gt[k + 1][:, :3], gt[k + 1][:, 3], tw["g_next"][:, :3], tw["g_next"][:, 3]
            assert np.abs(Rd.astype(np.float64) - Rt).max() <= 2.0 ** -23, (what, k, "R", np.abs(Rd.astype(np.float64) - Rt).max())
            tol = 2.0 ** -23 * (np.abs(tt.astype(np.float64)) + np.abs(tw["mu_x"]).sum())
            assert (np.abs(td.astype(np.float64) - tt) <= tol).all(), (what, k, "t", td, tt, tol)
            E_prev = E[k]
        else:
            if why is None:                                              # the rule goes on: only a failed solve stops here
                assert stop == io.DEGENERATE and tw["g_next"] is None, (what, k, stop)
            else:
                assert stop == why, (what, k, stop, why)
    return E


def _final(A, B, r, res, what=""):
    """the final search: bit for bit ops.cloud_nearest at g_out, and the twin's"""
    from livingscenes_amd import ops
    A, B = np.asarray(A, np.float32).reshape(-1, 3), np.asarray(B, np.float32).reshape(-1, 3)
    idx, d2, counts, s = ops.cloud_nearest(_t(A), _t(B), g=_g(res["g"]), radius=r)
    assert np.array_equal(res["idx"], idx.cpu().numpy()) and np.array_equal(_bits(res["d2"]), _bits(d2)), (what, "final nn")
    assert np.array_equal(res["counts"], counts), (what, res["counts"], counts)
    assert np.float64(res["sum_d2"]).view(np.uint64) == np.float64(s).view(np.uint64), (what, res["sum_d2"], s)
    tw = no.nearest(A, B, res["g"], r)
    assert np.array_equal(res["idx"], tw[0]) and np.array_equal(_bits(res["d2"]), _bits(tw[1])) and np.array_equal(res["counts"], tw[2]), what
    assert abs(res["sum_d2"] - tw[3]) <= int(tw[2][1]) * 2.0 ** -52 * tw[3], (what, res["sum_d2"], tw[3])


# ------------------------------------------------------------------------------------------------ size edges, P = 1
SIZES = [(0, 0), (0, 5), (5, 0), (2, 2), (3, 3), (300, 255), (300, 256), (300, 257), (TILE // 2, 300), (TILE // 2 + 1, 300), (TILE + 1, 513),
         (2 ** 13 + 1, 2 ** 13 + 1)]


def _edge_problem(a, b, posed):
    """b noisy rows of a random cloud of a rows, off their place by a small rigid motion -> (A, B, g0, r)"""
    rng = np.random.default_rng(1000 * a + b + posed)
    A = rng.uniform(-0.4, 0.4, (a, 3)).astype(np.float32)
    rows = rng.permutation(a)[:b] if b <= a else rng.integers(0, max(a, 1), b)   # distinct rows while they last: three of them span a plane
    pts = A[rows] + rng.normal(0, 0.002, (b, 3)) if a else rng.uniform(-0.4, 0.4, (b, 3))
    off = _pose([1, -2, 1], 1.0, [0.006, -0.004, 0.005])                 # what the ICP has to undo: up to ~0.02 at the corners
    g_true = _pose(rng.standard_normal(3), 40.0, rng.uniform(-0.5, 0.5, 3)) if posed else _pose([0, 0, 1], 0.0, [0, 0, 0])
    B = (pts @ _inv(_compose(off, g_true))[:, :3].T + _inv(_compose(off, g_true))[:, 3]).astype(np.float32)
    return A, B, (g_true.astype(np.float32) if posed else None), 0.05


@pytest.mark.parametrize("posed", (False, True))
@pytest.mark.parametrize("a,b", SIZES)
def test_size_edges(a, b, posed):
    assert TILE == 4096
    A, B, g0, r = _edge_problem(a, b, posed)
    res = _single(A, B, g0, r, max_iter=5)
    _steps(A, B, g0, r, res, max_iter=5, what=f"{a}x{b}")
    _final(A, B, r, res, f"{a}x{b}")
    if min(a, b) <= 2:
        assert res["stop"] == io.STARVED and res["iters"] == 0 and np.array_equal(_bits(res["g"]), _bits(io.pose0(g0)))
        assert res["counts"][1] <= 2
    else:
        assert res["iters"] >= 1 and res["stop"] in (io.CONVERGED, io.MAX_ITER)
        untraced = _single(A, B, g0, r, trace=False, max_iter=5)         # the trace is an observer: the same bits without it
        assert "g_trace" not in untraced
        _identical(untraced, res, f"{a}x{b} untraced")
    zero = _single(A, B, g0, r, max_iter=0)                              # max_iter 0: one search, no update
    assert zero["iters"] == 0 and zero["stop"] == (io.MAX_ITER if zero["counts"][1] >= 3 else io.STARVED)
    assert np.array_equal(_bits(zero["g"]), _bits(io.pose0(g0)))
    _final(A, B, r, zero, f"{a}x{b} max_iter 0")


# ------------------------------------------------------------------------------------------------ twins: one update recovers the pose
def test_twins():
    A, B, g0, r, rows = twin_case()
    first = io.step(A, B, g0, r)
    assert np.array_equal(first["idx"][:700], rows) and (first["idx"][700:] == -1).all()       # every first correspondence is the true twin
    one = _single(A, B, g0, r, max_iter=1)
    _steps(A, B, g0, r, one, max_iter=1, what="twins, one update")
    assert one["iters"] == 1 and one["stop"] == io.MAX_ITER
    res = _single(A, B, g0, r)
    _steps(A, B, g0, r, res, what="twins")
    _final(A, B, r, res, "twins")
    assert res["stop"] == io.CONVERGED and res["iters"] >= 1
    for out in (one, res):
        err = np.abs(io.images(B[:700], out["g"]).astype(np.float64) - A[rows]).max()
        print(f"twins: iters {out['iters']}: max |g_out x - a| = {err:.3e}, bound {twin_bound(A, B, out['g']):.3e}")
        assert err <= twin_bound(A, B, out["g"]), (err, twin_bound(A, B, out["g"]))
        assert np.array_equal(out["idx"][:700], rows) and (out["idx"][700:] == -1).all() and out["counts"].tolist() == [800, 700, 700]


# ------------------------------------------------------------------------------------------------ several iterations
def iter_case():
    """a synth shape merged at voxel 0.01 (the memory) against an independent, noisy resampling of its half x > 0 under a pose, plus a patch
    of surface the memory lacks; g0 off by 2 degrees and 0.015; r = 0.03 -> (A, B, g0, r, g_true)"""
    full = synth.canonical_shape(5200, 3).astype(np.float32)
    A, _ = mo.merge(full, full[:0], None, 0.01)
    rng = np.random.default_rng(23)
    other = synth.canonical_shape(6001, 3)                               # another N: another draw of the same shape
    mid = 0.5 * (full[:, 0].max() + full[:, 0].min())
    half = other[other[:, 0] > mid]
    lo, hi = full.min(0).astype(np.float64), full.max(0).astype(np.float64)
    patch = np.stack([rng.uniform(mid, hi[0], 400), rng.uniform(lo[1], hi[1], 400), np.full(400, hi[2] + 0.1)], 1)   # 0.1 > r above the shape
    pts = np.concatenate([half + rng.normal(0, 0.002, half.shape), patch])
    g_true = _pose([2, -1, 1], 70.0, [0.8, -0.3, 0.5])                   # takes B into the memory's frame
    gi = _inv(g_true)
    B = (pts @ gi[:, :3].T + gi[:, 3]).astype(np.float32)
    c = half.mean(0)
    dR = _rot([1, 1, -1], 2.0)
    shift = 0.015 * np.array([2.0, -1.0, 2.0]) / 3.0
    delta = np.concatenate([dR, (c - dR @ c + shift).reshape(3, 1)], 1)  # 2 degrees about the view's centroid, then 0.015
    return A, B, _compose(delta, g_true).astype(np.float32), 0.03, g_true


def test_several_iterations():
    A, B, g0, r, g_true = iter_case()
    assert 3000 < A.shape[0] <= 8200 and 2000 < B.shape[0] <= 8200
    res = _single(A, B, g0, r, max_iter=15)
    E = _steps(A, B, g0, r, res, max_iter=15, what="several iterations")
    _final(A, B, r, res, "several iterations")
    assert res["iters"] >= 2 and res["stop"] in (io.CONVERGED, io.MAX_ITER)
    assert all(E[k] < E[k - 1] for k in range(1, res["iters"])), E      # strictly down until the stop
    assert E[-1] <= E[0]
    truth = io.images(B, g_true.astype(np.float32)).astype(np.float64)
    dist = lambda g: float(np.linalg.norm(io.images(B, g).astype(np.float64) - truth, axis=1).mean())
    twin = io.icp(A, B, g0, r, max_iter=15)
    print(f"several iterations: device iters {res['iters']} stop {res['stop']} E0 {E[0]:.6e} E_end {E[-1]:.6e}; mean distance to the true-pose "
          f"images {dist(g0):.6f} -> {dist(res['g']):.6f}; twin iters {twin['iters']} stop {twin['stop']} E_end {twin['E'][-1]:.6e} "
          f"distance {dist(twin['g']):.6f}")
    assert dist(res["g"]) < dist(g0)


# ------------------------------------------------------------------------------------------------ rows that must be ignored
def test_non_finite_rows_are_ignored():
    A, B, g0, r = _edge_problem(600, 500, True)
    res = _single(A, B, g0, r, max_iter=5)
    A2 = np.concatenate([F([[np.nan, 0, 0], [0, np.inf, 0]]), A, F([[-np.inf, np.nan, 1]])])
    B2 = np.concatenate([B[:100], F([[0, 0, np.nan], [np.inf, np.inf, np.inf]]), B[100:], F([[1, -np.inf, 1]])])
    got = _single(A2, B2, g0, r, max_iter=5)
    _steps(A2, B2, g0, r, got, max_iter=5, what="non-finite")
    _final(A2, B2, r, got, "non-finite")
    assert got["iters"] >= 1 and res["iters"] >= 1 and got["counts"][0] == 500 and got["counts"][1] > 400
    assert (got["idx"][[100, 101, 502]] == -1).all() and not set(got["idx"].tolist()) & {0, 1, 602}
    assert np.abs(got["g"] - res["g"]).max() < 1e-3                     # the same problem between the rows that are ignored
    nothing = _single(np.full((300, 3), np.nan, np.float32), B, g0, r, max_iter=5)
    assert nothing["stop"] == io.STARVED and nothing["iters"] == 0 and nothing["counts"].tolist() == [500, 0, 0]
    bad_pose = g0.copy()
    bad_pose[1, 3] = np.nan                                              # every query non-finite: f = 0, E = 0, starved
    nothing = _single(A, B, bad_pose, r, max_iter=5)
    assert nothing["stop"] == io.STARVED and nothing["counts"].tolist() == [0, 0, 0] and np.array_equal(_bits(nothing["g"]), _bits(bad_pose))


def test_collinear_matches_are_degenerate():
    A = np.zeros((40, 3), np.float32)
    A[:, 0] = np.arange(40) * 0.01                                       # on the x axis: H is exactly of rank 1
    B = A + F([0.002, 0, 0])
    for g0 in (None, F([[1, 0, 0, 0.001], [0, 1, 0, 0], [0, 0, 1, 0]])):
        res = _single(A, B, g0, 0.02, max_iter=5)
        _steps(A, B, g0, 0.02, res, max_iter=5, what="collinear")
        _final(A, B, 0.02, res, "collinear")
        assert res["stop"] == io.DEGENERATE and res["iters"] == 0 and res["counts"][1] == 40
        assert np.array_equal(_bits(res["g"]), _bits(io.pose0(g0)))
    A2 = np.concatenate([A, F([[0.1, 0.05, 0.02], [0.3, -0.04, 0.03]])])  # two points off the axis: a rotation again
    res = _single(A2, A2 + F([0.002, 0, 0]), None, 0.02, max_iter=5)
    _steps(A2, A2 + F([0.002, 0, 0]), None, 0.02, res, max_iter=5, what="off the axis")
    assert res["stop"] != io.DEGENERATE and res["iters"] >= 1


# ------------------------------------------------------------------------------------------------ the ragged batch
@pytest.fixture(scope="module")
def batch():
    rng = np.random.default_rng(31)
    tA, tB, tg, tr, _ = twin_case()
    iA, iB, ig, ir, _ = iter_case()
    r1 = _edge_problem(700, 257, True)
    r2 = _edge_problem(1025, 2000, True)
    eye = io.IDENTITY
    probs = [(np.zeros((0, 3), F), rng.uniform(-1, 1, (300, 3)).astype(F), eye, 0.05),          # an empty A
             (rng.uniform(-1, 1, (300, 3)).astype(F), np.zeros((0, 3), F), eye, 0.05),          # an empty B
             (F([[0, 0, 0], [0.5, 0, 0], [0, 0.5, 0], [0.3, 0.3, 0.3]]), F([[0.001, 0, 0], [0.5, 0.001, 0], [9, 9, 9]]), eye, 0.02),   # starved
             (tA, tB, tg, float(tr)), (iA, iB, ig, ir), (r1[0], r1[1], r1[2], 0.05), (r2[0], r2[1], r2[2], 0.04)]
    return probs


def _run_batch(probs, packed=False, **kw):
    from livingscenes_amd import ops
    return ops.cloud_icp_batch([_t(p[0]) for p in probs], [_t(p[1]) for p in probs], g=_g(np.stack([p[2] for p in probs])),
                               radius=[p[3] for p in probs], trace=True, packed=packed, **kw)


def test_batch_is_the_single_op_in_any_order_and_run(batch):
    P = len(batch)
    assert P == 7
    kw = {"max_iter": 12}
    res = [_host(x) for x in _run_batch(batch, **kw)]
    alone = [_single(*p, **kw) for p in batch]
    for p in range(P):
        _identical(res[p], alone[p], f"problem {p} alone")
    rev = [_host(x) for x in _run_batch(batch[::-1], **kw)]
    again = [_host(x) for x in _run_batch(batch, **kw)]
    for p in range(P):
        _identical(rev[P - 1 - p], res[p], f"problem {p} reversed")
        _identical(again[p], res[p], f"problem {p} again")
    iters = [x["iters"] for x in res]
    assert [x["stop"] for x in res[:3]] == [io.STARVED] * 3 and iters[:3] == [0, 0, 0] and res[2]["counts"][1] == 2
    assert len(set(iters)) >= 3 and min(iters[3:]) >= 1, iters           # problems stop at different k: the stopped ones stay frozen
    print("batch iters", iters, "stop", [x["stop"] for x in res])
    _steps(batch[5][0], batch[5][1], batch[5][2], batch[5][3], res[5], what="batch problem 5", **kw)
    _final(batch[6][0], batch[6][1], batch[6][3], res[6], "batch problem 6")
    pk = _run_batch(batch, packed=True, **kw)                            # the packed form: the same result
    assert pk["b_off"].tolist() == np.cumsum([0] + [p[1].shape[0] for p in batch]).tolist() and tuple(pk["g"].shape) == (P, 3, 4)
    assert pk["stop"].dtype == np.int32 and pk["stop"].tolist() == [x["stop"] for x in res] and pk["iters"].tolist() == iters
    assert np.array_equal(_bits(pk["g"]), _bits(np.stack([x["g"] for x in res]))) and np.array_equal(pk["counts"], np.stack([x["counts"] for x in res]))
    assert np.array_equal(pk["idx"].cpu().numpy(), np.concatenate([x["idx"] for x in res])) and pk["sum_d2"].tolist() == [x["sum_d2"] for x in res]


def test_errors_name_the_problem(batch):
    from livingscenes_amd import _lib, ops
    tA, tB = [_t(p[0]) for p in batch], [_t(p[1]) for p in batch]
    rs = [p[3] for p in batch]
    with pytest.raises(_lib.LsError, match="problem 4.*radius"):
        ops.cloud_icp_batch(tA, tB, radius=rs[:4] + [float("nan")] + rs[5:])
    for kw, word in (({"max_iter": -1}, "max_iter"), ({"min_matched": 2}, "min_matched"), ({"rel_thr": -1.0}, "rel_thr"), ({"rel_thr": float("nan")}, "rel_thr")):
        with pytest.raises(_lib.LsError, match=word):
            ops.cloud_icp_batch(tA, tB, radius=rs, **kw)
        with pytest.raises(_lib.LsError, match=word):
            ops.cloud_icp(tA[3], tB[3], radius=0.02, **kw)
    with pytest.raises(_lib.LsError, match="no CPU fallback"):
        ops.cloud_icp(torch.zeros(3, 3), torch.zeros(3, 3), radius=0.1)
    with pytest.raises(ValueError):
        ops.cloud_icp(tA[3], tB[3], g=torch.eye(3, device=_dev()), radius=0.1)
    with pytest.raises(ValueError):
        ops.cloud_icp_batch(tA, tB[:-1], radius=0.1)


# ------------------------------------------------------------------------------------------------ the layers above


def _pose_error(T, T_true, pts):
    """mean distance between the images of pts under two memory -> rescan transforms [4,4]"""
    T, T_true = T.double().cpu().numpy(), T_true.double().cpu().numpy()
    p = pts.double().cpu().numpy()
    return float(np.linalg.norm((p @ T[:3, :3].T + T[:3, 3]) - (p @ T_true[:3, :3].T + T_true[:3, 3]), axis=1).mean())


def _perturbed(T_true, k, centre):
    """a ground-truth transform [4,4] (numpy float64, memory -> rescan) off by 1.5 degrees about `centre` (memory frame) and 0.01"""
    d = np.eye(4)
    dR = _rot([1, k + 1, -1], 1.5)
    d[:3, :3], d[:3, 3] = dR, centre - dR @ centre + [0.006, -0.006, 0.005]
    return T_true @ d


def test_refine_on_memory_batch():
    from livingscenes_amd.lib_math.torch_se3 import inverse
    d = _dev()
    solver = _solver(object())
    rng = np.random.default_rng(41)
    mems, news, Ts, Tt = [], [], [], []
    for k, seed in enumerate((3, 4, 5)):
        full = synth.canonical_shape(6000, seed).astype(np.float32)
        mem, _ = mo.merge(full, full[:0], None, 0.01)
        other = synth.canonical_shape(3001, seed)
        view = other[other[:, 0] > np.median(other[:, 0]) - 0.05]
        view = view + rng.normal(0, 0.001, view.shape)
        T_true = np.eye(4)
        T_true[:3] = _pose(rng.standard_normal(3), 50.0 + 20 * k, rng.uniform(-1, 1, 3))      # memory -> rescan
        mems.append(_t(mem)), news.append(_t((view @ T_true[:3, :3].T + T_true[:3, 3]).astype(np.float32)))
        Tt.append(torch.from_numpy(T_true).to(d)), Ts.append(_perturbed(T_true, k, mem.astype(np.float64).mean(0)).astype(np.float32))
    mems.append(_t(np.zeros((0, 3), F))), news.append(news[0].clone())   # an empty memory: starved, the slot keeps its T
    Ts.append(Ts[0] + F(0.125))                                          # not even a rigid motion: it must come back bit for bit
    T = torch.from_numpy(np.stack(Ts)).to(d)
    for Tin in (T, T[:, :3].contiguous()):
        T2, info = solver._refine_on_memory_batch(mems, news, Tin, 0.04, max_iter=30)
        assert tuple(T2.shape) == (4, 4, 4) and T2.dtype == torch.float32
        assert set(info) == {"g", "stop", "iters", "overlap", "rmse", "memory_seen", "counts", "nn_idx"}
        assert info["iters"][3] == 0 and info["stop"][3] == io.STARVED and np.array_equal(_bits(T2[3, :3]), _bits(Tin[3, :3]))
        assert T2[3, 3].tolist() == [0, 0, 0, 1] or np.array_equal(_bits(T2[3]), _bits(Tin[3]))
        assert np.array_equal(_bits(info["g"][3]), _bits(inverse(Tin)[3]))                      # g_out is the g0 the operator received
        for k in range(3):
            before, after = _pose_error(T[k], Tt[k], mems[k]), _pose_error(T2[k], Tt[k], mems[k])
            print(f"pair {k}: iters {info['iters'][k]} stop {info['stop'][k]} pose error {before:.5f} -> {after:.5f} overlap {info['overlap'][k]:.3f}")
            assert info["iters"][k] >= 1 and after < before
            assert np.array_equal(_bits(T2[k, :3]), _bits(inverse(info["g"][k:k + 1])[0]))    # T' is inverse(g_out)
    # the figures are those of _overlap_batch at g_out and this radius; g= reaches the merge and the search without an inverse
    ov = solver._overlap_batch(mems, news, None, radius=0.04, g=info["g"])
    for key in ("overlap", "memory_seen"):
        assert ov[key] == info[key]
    assert all(a == b or (math.isnan(a) and math.isnan(b)) for a, b in zip(ov["rmse"], info["rmse"]))
    assert all(np.array_equal(a, b) for a, b in zip(ov["counts"], info["counts"]))
    assert all(torch.equal(a, b) for a, b in zip(ov["nn_idx"], info["nn_idx"]))
    by_T = solver._accumulate_batch(mems[:3], news[:3], T2[:3], voxel=0.01)
    by_g = solver._accumulate_batch(mems[:3], news[:3], None, voxel=0.01, g=info["g"][:3])
    assert all(abs(a.shape[0] - b.shape[0]) <= 0.02 * a.shape[0] for a, b in zip(by_T, by_g))   # inverse(inverse(g)) is g up to rounding
    for f in (solver._accumulate_batch, solver._overlap_batch):
        with pytest.raises(ValueError, match="not both"):
            f(mems, news, T, g=info["g"])
    with pytest.raises(ValueError):
        solver._refine_on_memory_batch(mems, news[:1], T, 0.04)
    with pytest.raises(ValueError):
        solver._refine_on_memory_batch(mems, news, None, 0.04)


def _counted(monkeypatch, solver, truth):
    """every memory slot matched to the rescan instance of its index, the registration replaced by perturbed ground truth -- truth(pc1, pc2)
    -> [4,4] float64 memory -> rescan -- and the calls counted"""
    calls = {"registration": 0, "overlap": 0, "accumulate": 0, "refine": 0}
    monkeypatch.setattr(solver, "_solve_object_matching",
                        lambda src, tgt, method: {"matches0": torch.arange(src["z_inv"].shape[0], device=src["z_inv"].device)})

    def registration(pcs1, pcs2, icp=True):
        calls["registration"] += 1
        T = np.stack([_perturbed(truth(a, b), k, a.double().mean(0).cpu().numpy()) for k, (a, b) in enumerate(zip(pcs1, pcs2))]).astype(np.float32)
        T = torch.from_numpy(T).to(pcs1[0].device)
        return T[:, :3, :3].contiguous(), T[:, :3, 3:].contiguous()
    monkeypatch.setattr(solver, "_solve_pairwise_registration_batch", registration)
    for name, key in (("_overlap_batch", "overlap"), ("_accumulate_batch", "accumulate"), ("_refine_on_memory_batch", "refine")):
        def counted(*a, _real=getattr(solver, name), _key=key, **kw):
            calls[_key] += 1
            return _real(*a, **kw)
        monkeypatch.setattr(solver, name, counted)
    return calls


def _step_values_equal(st, st0):
    for key in STEP_KEYS - {"codes", "registration", "ref_pc_lst", "rescan_pc_lst", "matches"}:
        assert st[key] == st0[key], key
    assert torch.equal(st["matches"], st0["matches"])
    for key in ("ref_pc_lst", "rescan_pc_lst"):
        assert all(torch.equal(a, b) for a, b in zip(st[key], st0[key])), key
    for a, b in zip(st["registration"], st0["registration"]):
        assert (a is None and b is None) or torch.equal(a, b)
    for a, b in zip(st["codes"], st0["codes"]):
        assert (a is None and b is None) or all(torch.equal(a[k], b[k]) for k in CODE_KEYS)


def test_solve_sequence_refine_radius(small_prior, monkeypatch):
    from livingscenes_amd.lib_more import more_solver
    solver = _solver(small_prior)
    n, h = 4, 0.02
    pair = synth.make_scene_pair(n, 700, seed=71, noise=0.002)
    ref, rescan = _scene(pair["ref"]), _scene(pair["rescan"])
    gt = (pair["rescan_T"].double() @ torch.linalg.inv(pair["ref_T"].double())).numpy()      # [n,4,4] reference -> rescan
    ref_pts = pair["ref"].numpy()

    def truth(pc1, pc2):
        """the ground truth of the instance a memory cloud belongs to: the merge keeps the first row of the reference cloud"""
        return gt[next(i for i in range(n) if (ref_pts[i, 0] == pc1[0].cpu().numpy()).all())]

    calls = _counted(monkeypatch, solver, truth)
    steps0, memory0 = more_solver.solve_sequence(solver, ref, [rescan], voxel=h)              # refine_radius None: exactly today's step
    assert set(steps0[0]) == STEP_KEYS and calls["refine"] == 0 and calls["overlap"] == 0
    again0, _ = more_solver.solve_sequence(solver, ref, [rescan], voxel=h, refine_radius=None)
    _step_values_equal(again0[0], steps0[0])
    base = dict(calls)
    steps, memory = more_solver.solve_sequence(solver, ref, [rescan], voxel=h, refine_radius=0.04, overlap_radius=0.04, min_overlap=0.0)
    st, st0 = steps[0], steps0[0]
    assert set(st) == STEP_KEYS | GATE_KEYS | REFINE_KEYS
    assert calls["refine"] == base["refine"] + 1 and calls["overlap"] == base["overlap"], "equal radii: the refinement's search is the gate's"
    assert calls["registration"] == base["registration"] + 1
    m0 = st["matches"].tolist()
    slots = list(range(n))
    assert m0 == slots
    good = 0
    for i in range(n):
        assert torch.equal(st["registration_init"][i], st0["registration"][i]) and st["registration"][i].shape == (1, 4, 4)
        assert st["refine_stop"][i] in (0, 1, 2, 3) and st["refine_iters"][i] >= 0 and 0.0 <= st["overlap"][i] <= 1.0
        if st["refine_iters"][i] == 0:
            assert torch.equal(st["registration"][i], st["registration_init"][i])
        T_true = torch.from_numpy(gt[i])                                 # the refinement must come nearer the truth
        before = _pose_error(st["registration_init"][i][0], T_true, st["ref_pc_lst"][i])
        after = _pose_error(st["registration"][i][0], T_true, st["ref_pc_lst"][i])
        print(f"slot {i}: iters {st['refine_iters'][i]} stop {st['refine_stop'][i]} pose error {before:.5f} -> {after:.5f}")
        assert st["refine_iters"][i] >= 1 and after < before
        good += 1
    assert good == n
    base = dict(calls)
    steps2, _ = more_solver.solve_sequence(solver, ref, [rescan], voxel=h, refine_radius=0.04, overlap_radius=0.03)
    assert calls["refine"] == base["refine"] + 1 and calls["overlap"] == base["overlap"] + 1, "other radii: one search at g_out"
    for i in slots:
        assert torch.equal(steps2[0]["registration"][i], st["registration"][i]) and steps2[0]["overlap"][i] <= st["overlap"][i]
    steps3, _ = more_solver.solve_sequence(solver, ref, [rescan], voxel=h, refine_radius=0.04)     # no gate: no gate keys
    assert set(steps3[0]) == STEP_KEYS | REFINE_KEYS and steps3[0]["merged_sizes"] == st["merged_sizes"]
