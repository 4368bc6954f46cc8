"""GPU tests of the scene memory's normals and point-to-plane ICP (csrc/cloudnear.hip: ls_cloud_normals_f32 / ls_cloud_icp_plane_f32 and their
batch forms; ops.cloud_normals*, ops.cloud_icp_plane*) and of the layers on top (More_Solver._memory_normals_batch,
_refine_on_memory_batch(metric="plane"), solve_sequence(refine_metric="plane")).

Normals.  nbr_cnt, both counts and the valid mask are integers and must EQUAL those of tests/normals_oracle.py: the moments are int64 sums of
the same integers on both sides, the covariance is the same float64 expression of them (the same bits), and the validity rule is a
comparison of eigenvalues that the inputs keep away from its threshold (asserted on the twin: l1 / l2 outside [2^-44, 2^-36]).  The
eigenvectors come from two float64 solvers (Jacobi on the device, LAPACK in the twin).  A backward-stable solver returns the eigenvector of
C + dC with |dC| <= c 2^-52 |C| for a small c; the eigenvector of l0 then moves by at most |dC| / (l1 - l0), and the tests assert
(l1 - l0) / l2 >= 1e-3 on the twin, so the two float64 normals differ by about c 1e3 2^-52 < 1e-11 per component.  Each side then rounds
once to fp32: |n| <= 1, so an fp32 ulp is at most 2^-24 and the two roundings of values 1e-11 apart differ by at most one ulp.  One more
ulp is allowed: |n_dev - n_twin| <= 2^-23, after aligning the sign with the twin's (the sign rule itself is checked on the device's output
wherever its two largest magnitudes differ by more than 2^-20, far above both effects).  variation = l0 / (l0 + l1 + l2): an eigenvalue moves
by at most |dC| <= c 2^-52 l2 and the denominator is at least l2, so the float64 values differ by a few 2^-52 ABSOLUTE -- 2^-45 allows for
c up to 128 -- and the fp32 roundings add one ulp of the value, 2^-23 v, with one more allowed: 2^-22 twin + 2^-45.

Plane ICP.  Held to tests/plane_icp_oracle.py STEP BY STEP like tests/test_hip_cloud_icp.py: at every traced g_k the twin's search must give the
same f, n, w as integers, S within n 2^-52 S and Q within w 2^-52 Q of the twin's math.fsum (sums of non-negative terms that are the same
float64 values on both sides).  The twin's update from its own correspondences gives g_{k+1}: R within 2^-23 per entry, t_a within
2^-23 (|t_a| + sum_b |c_b|) with c the centroid of the posed planar queries -- the bound of the point ICP's test with the lever arm of this
update: both sides solve in float64 and round once, an ulp of rotation moves a point at c by ulp |c|.  The conditioning is asserted on the
twin: the smallest Cholesky pivot ratio >= 1e-8 (or the exact degenerate case), so the float64 solutions agree far below an fp32 ulp.
stop / iters are re-derived from the device's own traced statistics; the final search is compared bit for bit with ops.cloud_nearest."""
import numpy as np
import pytest
import torch

import icp_oracle as io
import nearest_oracle as no
import normals_oracle as nmo
import plane_icp_oracle as po
from cloud_testlib import (GATE_KEYS, REFINE_KEYS, STEP_KEYS, TILE, F, _bits, _dev, _g, _scene, _solver, _t,
                           small_prior)  # noqa: F401 (small_prior is a fixture)
from livingscenes_amd import synth
from test_cloud_icp_cpu import _inv, _pose, _rot
from test_cloud_plane_cpu import OFFSET, SHEET_R, eigen_gap_ok, hand_cases, sheet, surface_case
from test_hip_cloud_icp import _compose, _counted, _perturbed, _step_values_equal

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ normals
def _normals(A, r=SHEET_R, min_nbrs=5):
    from livingscenes_amd import ops
    n, c, v, counts = ops.cloud_normals(_t(A), radius=r, min_nbrs=min_nbrs)
    assert n.dtype == torch.float32 and c.dtype == torch.int32 and v.dtype == torch.float32 and counts.dtype == np.int64
    A = np.asarray(A).reshape(-1, 3)
    assert tuple(n.shape) == (A.shape[0], 3) and tuple(c.shape) == tuple(v.shape) == (A.shape[0],) and counts.shape == (2,)
    return {"normals": n.cpu().numpy(), "nbr_cnt": c.cpu().numpy(), "variation": v.cpu().numpy(), "counts": counts}


def _check_normals(got, tw, what="", gap=True):
    """the comparison of the module docstring; no row is skipped"""
    assert np.array_equal(got["nbr_cnt"], tw["nbr_cnt"]), (what, "nbr_cnt")
    assert np.array_equal(got["counts"], tw["counts"]), (what, got["counts"], tw["counts"])
    valid = (got["normals"] != 0).any(1)
    assert np.array_equal(valid, tw["valid"]), (what, "valid", np.flatnonzero(valid != tw["valid"])[:5])
    assert not got["variation"][~valid].any()
    if gap:
        assert eigen_gap_ok(tw), (what, "the inputs do not meet the eigen-gap condition")
    nd, nt = got["normals"].astype(np.float64), tw["normals"].astype(np.float64)
    sign = np.where((nd * nt).sum(1) < 0, -1.0, 1.0)[:, None]
    err = np.abs(nd * sign - nt).max() if nd.size else 0.0
    assert err <= 2.0 ** -23, (what, "normal", err)
    mag = np.sort(np.abs(nd[valid]), axis=1)
    clear = mag[:, 2] - mag[:, 1] > 2.0 ** -20
    big = np.argmax(np.abs(nd[valid]), axis=1)
    assert (nd[valid][np.arange(big.size), big][clear] > 0).all(), (what, "the sign rule")
    assert (sign[valid][clear] == 1.0).all(), (what, "the sign agrees with the twin's where the rule is unambiguous")
    vd, vt = got["variation"].astype(np.float64), tw["variation"].astype(np.float64)
    assert (np.abs(vd - vt) <= 2.0 ** -22 * np.abs(vt) + 2.0 ** -45).all(), (what, "variation", np.abs(vd - vt).max())
    assert np.allclose(np.linalg.norm(nd[valid], axis=1), 1.0, rtol=0, atol=2.0 ** -22)


NORMAL_SIZES = [0, 1, 2, 4, 5, 255, 256, 257, TILE // 2, TILE // 2 + 1, TILE + 1, 2 ** 13 + 1]


@pytest.mark.parametrize("a", NORMAL_SIZES)
def test_normals_size_edges(a):
    assert TILE == 4096
    A = sheet(a, seed=a % 3)
    got, tw = _normals(A), nmo.normals(A, F(SHEET_R), 5)
    _check_normals(got, tw, f"a = {a}")
    assert got["counts"][0] == a
    if a >= 255:
        assert got["counts"][1] >= 0.99 * a
    if a < 5:
        assert got["counts"][1] == 0 and not got["normals"].any()
    lo = _normals(A, min_nbrs=1)                                        # the count rule off: the rank rule alone
    _check_normals(lo, nmo.normals(A, F(SHEET_R), 1), f"a = {a}, min_nbrs 1")


def test_normals_one_crowded_cell():
    """5 000 jittered points in one cell: every row has 5 000 neighbours, the second moments reach 5 000 * 2^30"""
    rng = np.random.default_rng(5)
    A = (OFFSET + [0.0151, 0.0149, 0.015] + rng.uniform(-0.004, 0.004, (5000, 3)) * [1, 1, 0.1]).astype(np.float32)
    got, tw = _normals(A), nmo.normals(A, F(SHEET_R), 5)
    assert (tw["nbr_cnt"] == 5000).all() and np.abs(tw["s2"]).max() > 2 ** 31 and np.unique(nmo.cells(A, F(SHEET_R))[0], axis=0).shape[0] == 1
    _check_normals(got, tw, "one cell")
    assert got["counts"].tolist() == [5000, 5000]


def test_normals_far_from_the_origin():
    A = sheet(2049, seed=1) + F([300.0, -300.0, 300.0])                  # an fp32 ulp is 3e-5 here: a thousandth of r
    got, tw = _normals(A), nmo.normals(A, F(SHEET_R), 5)
    _check_normals(got, tw, "300 m")
    assert got["counts"][1] > 1900


def test_normals_ignore_non_finite_rows():
    A = sheet(600, seed=2)
    A2 = np.concatenate([F([[np.nan, 0, 0], [0, np.inf, 0]]), A[:300], F([[-np.inf, np.nan, 1]]), A[300:]])
    got, tw = _normals(A2), nmo.normals(A2, F(SHEET_R), 5)
    _check_normals(got, tw, "non-finite")
    assert got["counts"][0] == 600 and got["nbr_cnt"][[0, 1, 302]].tolist() == [0, 0, 0] and not got["normals"][[0, 1, 302]].any()
    clean = _normals(A)
    keep = np.r_[2:302, 303:603]
    for k in ("normals", "nbr_cnt", "variation"):
        assert np.array_equal(_bits(got[k][keep]), _bits(clean[k])), k   # the same rows between the ones that are ignored
    nothing = _normals(np.full((300, 3), np.nan, np.float32))
    assert nothing["counts"].tolist() == [0, 0] and not nothing["nbr_cnt"].any() and not nothing["normals"].any()


def test_normals_hand_written():
    for name, A, r, k, valid, n0 in hand_cases():
        got = _normals(A, r, k)
        _check_normals(got, nmo.normals(A, F(r), k), name, gap=False)
        assert (got["normals"] != 0).any(1).tolist() == valid, name
        if n0 is not None:
            assert np.array_equal(got["normals"], np.tile(F(n0), (len(A), 1))) and not got["variation"].any(), name
    n = _normals(hand_cases()[4][1], 0.03, 5)["normals"][0]             # two equal magnitudes: the first is positive
    assert abs(abs(n[0]) - abs(n[2])) <= 2.0 ** -23 and n[0] * n[2] < 0 and ((n[0] > 0) if abs(n[0]) >= abs(n[2]) else (n[2] > 0)), n


def test_normals_batch_is_the_single_op():
    from livingscenes_amd import _lib, ops
    clouds = [sheet(700, 0), np.zeros((0, 3), F), sheet(257, 1), hand_cases()[1][1], sheet(2 ** 12 + 5, 2), np.zeros((0, 3), F), sheet(5, 0)]
    radii = [0.03, 0.05, 0.04, 0.03, 0.03, 0.02, 0.03]
    res = ops.cloud_normals_batch([_t(c) for c in clouds], radius=radii)
    alone = [ops.cloud_normals(_t(c), radius=r) for c, r in zip(clouds, radii)]
    rev = ops.cloud_normals_batch([_t(c) for c in clouds[::-1]], radius=radii[::-1])[::-1]
    for p in range(7):
        for other in (alone[p], rev[p]):
            assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(res[p][:3], other[:3])), p
            assert np.array_equal(res[p][3], other[3]), p
        tw = nmo.normals(clouds[p], F(radii[p]), 5)
        _check_normals({"normals": res[p][0].cpu().numpy(), "nbr_cnt": res[p][1].cpu().numpy(), "variation": res[p][2].cpu().numpy(),
                        "counts": res[p][3]}, tw, f"problem {p}", gap=p != 3)
    assert res[3][3].tolist() == [7, 0] and res[1][3].tolist() == [0, 0]
    n, c, v, counts, off = ops.cloud_normals_batch([_t(c) for c in clouds], radius=radii, packed=True)
    assert off.tolist() == np.cumsum([0] + [len(c) for c in clouds]).tolist() and tuple(counts.shape) == (7, 2)
    assert torch.equal(n, torch.cat([x[0] for x in res])) and torch.equal(c, torch.cat([x[1] for x in res]))
    with pytest.raises(_lib.LsError, match="problem 4.*radius"):
        ops.cloud_normals_batch([_t(c) for c in clouds], radius=radii[:4] + [float("nan")] + radii[5:])
    with pytest.raises(_lib.LsError, match="min_nbrs"):
        ops.cloud_normals(_t(clouds[0]), radius=0.03, min_nbrs=0)
    with pytest.raises(_lib.LsError, match="no CPU fallback"):
        ops.cloud_normals(torch.zeros(3, 3), radius=0.1)


# ------------------------------------------------------------------------------------------------ plane ICP, P = 1
def _host(res):
    assert res["g"].dtype == torch.float32 and tuple(res["g"].shape) == (3, 4) and res["idx"].dtype == torch.int32
    assert all(isinstance(res[k], int) for k in ("stop", "iters", "planar")) and isinstance(res["sum_d2"], float) and isinstance(res["sum_rho2"], float)
    return {k: v.cpu().numpy() if torch.is_tensor(v) else v for k, v in res.items()}


def _single(A, N, B, g0, r, trace=True, **kw):
    from livingscenes_amd import ops
    return _host(ops.cloud_icp_plane(_t(A), _t(N), _t(B), g=_g(g0), radius=r, trace=trace, **kw))


def _identical(x, y, what=""):
    assert (x["stop"], x["iters"], x["planar"]) == (y["stop"], y["iters"], y["planar"]), (what, x["stop"], y["stop"], x["iters"], y["iters"])
    assert np.array_equal(_bits(x["g"]), _bits(y["g"])), (what, "g")
    assert np.array_equal(x["idx"], y["idx"]) and np.array_equal(_bits(x["d2"]), _bits(y["d2"])) and np.array_equal(x["counts"], y["counts"]), what
    for k in ("sum_d2", "sum_rho2"):
        assert np.float64(x[k]).view(np.uint64) == np.float64(y[k]).view(np.uint64), (what, k, x[k], y[k])
    if "g_trace" in x and "g_trace" in y:
        k = x["iters"] + 1
        assert np.array_equal(_bits(x["g_trace"][:k]), _bits(y["g_trace"][:k])), (what, "g_trace")
        assert np.array_equal(x["stat_trace"][:k].view(np.uint64), y["stat_trace"][:k].view(np.uint64)), (what, "stat_trace")


def _steps(A, N, B, g0, r, res, max_iter=100, rel_thr=1e-6, min_matched=6, what=""):
    """the per-step check of the module docstring -> the device's E_k, k <= iters"""
    A, N, B = (np.asarray(X, np.float32).reshape(-1, 3) for X in (A, N, B))
    iters, stop = res["iters"], res["stop"]
    assert 0 <= iters <= max_iter, (what, iters)
    gt, st = res["g_trace"].reshape(-1, 3, 4), res["stat_trace"]
    assert gt.shape[0] == st.shape[0] == max_iter + 1 and st.shape[1] == 5
    assert np.array_equal(_bits(gt[0]), _bits(io.pose0(g0))), (what, "g_0 is g0 (None: the identity matrix)")
    assert np.array_equal(_bits(res["g"]), _bits(gt[iters])), (what, "g_out is g_k of the stop")
    assert not _bits(gt[iters + 1:]).any() and not st[iters + 1:].any(), (what, "trace rows past the stop are left alone")
    E, E_prev = [], 0.0
    for k in range(iters + 1):
        R = gt[k][:, :3].astype(np.float64)
        if np.isfinite(R).all() and k > 0:
            assert np.abs(R @ R.T - np.eye(3)).max() <= 2.0 ** -22, (what, k, "g_k is orthonormal to fp32 rounding")
        tw = po.step(A, N, B, gt[k], r)
        f, n, S, w, Q = st[k]
        assert (f, n, w) == (tw["f"], tw["n"], tw["w"]), (what, k, "f, n, w", f, n, w, tw["f"], tw["n"], tw["w"])
        assert abs(S - tw["S"]) <= tw["n"] * 2.0 ** -52 * tw["S"], (what, k, "S", S, tw["S"])
        assert abs(Q - tw["Q"]) <= tw["w"] * 2.0 ** -52 * tw["Q"], (what, k, "Q", Q, tw["Q"])
        E.append(io.cost(int(f), int(w), float(Q), r))
        why = po.stop_rule(k, int(w), E[k], E_prev, max_iter, rel_thr, min_matched)
        if k < iters:
            assert why is None, (what, k, "the device went on where the rule stops", why)
            assert tw["g_next"] is not None and tw["pivot"] >= 1e-8, (what, k, "the twin's M is ill-conditioned: a case of its own", tw["pivot"])
            Rd, td, Rt, tt = gt[k + 1][:, :3], gt[k + 1][:, 3], tw["g_next"][:, :3], tw["g_next"][:, 3]
            assert np.abs(Rd.astype(np.float64) - Rt).max() <= 2.0 ** -23, (what, k, "R", np.abs(Rd.astype(np.float64) - Rt).max())
            c = io.images(B, gt[k])[po.planar_mask(N, tw["idx"])].astype(np.float64).mean(0)
            tol = 2.0 ** -23 * (np.abs(tt.astype(np.float64)) + np.abs(c).sum())
            assert (np.abs(td.astype(np.float64) - tt) <= tol).all(), (what, k, "t", td, tt, tol)
            E_prev = E[k]
        else:
            assert (res["planar"], res["sum_rho2"]) == (int(w), float(Q)), (what, "the final (w, Q)")
            if why is None:                                              # the rule goes on: only a failed solve stops here
                assert stop == po.DEGENERATE and tw["g_next"] is None, (what, k, stop)
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


def _memory(a, seed=0):
    """a sheet and the device's own normals of it: the twin is fed the device's array"""
    A = sheet(a, seed)
    return A, _normals(A)["normals"]


def _view(A, b, seed, posed=True):
    """b noisy rows of A, off their place by a small rigid motion about the cloud's centre -> (B, g0)"""
    rng = np.random.default_rng(900 + 7 * b + seed)
    rows = rng.permutation(A.shape[0])[:b] if b <= A.shape[0] else rng.integers(0, A.shape[0], b)
    pts = A[rows].astype(np.float64) + rng.normal(0, 0.001, (b, 3))
    c = A.astype(np.float64).mean(0)
    dR = _rot([1, -2, 1], 1.0)
    off = np.concatenate([dR, (c - dR @ c + [0.004, -0.003, 0.004]).reshape(3, 1)], 1)     # what the ICP has to undo
    g_true = _pose(rng.standard_normal(3), 40.0, rng.uniform(-0.5, 0.5, 3)) if posed else _pose([0, 0, 1], 0.0, [0, 0, 0])
    gi = _inv(_compose(off, g_true))
    B = (pts @ gi[:, :3].T + gi[:, 3]).astype(np.float32)
    return B, (g_true.astype(np.float32) if posed else None)


QUERY_SIZES = [0, 5, 255, 256, 257, 513, 2 ** 13 + 1]


@pytest.mark.parametrize("posed", (False, True))
@pytest.mark.parametrize("b", QUERY_SIZES)
def test_plane_icp_size_edges(b, posed):
    A, N = _memory(2 ** 13 + 1 if b > 2049 else 2049, seed=1)
    B, g0 = _view(A, b, int(posed), posed)
    r = SHEET_R
    res = _single(A, N, B, g0, r, max_iter=4)
    _steps(A, N, B, g0, r, res, max_iter=4, what=f"b = {b}")
    _final(A, B, r, res, f"b = {b}")
    if b <= 5:
        assert res["stop"] == po.STARVED and res["iters"] == 0 and np.array_equal(_bits(res["g"]), _bits(io.pose0(g0))) and res["planar"] <= 5
    else:
        assert res["iters"] >= 1 and res["stop"] in (po.CONVERGED, po.MAX_ITER)
        untraced = _single(A, N, B, g0, r, trace=False, max_iter=4)     # the trace is an observer: the same bits without it
        assert "g_trace" not in untraced
        _identical(untraced, res, f"b = {b} untraced")
    zero = _single(A, N, B, g0, r, max_iter=0)                          # max_iter 0: one search, no update
    assert zero["iters"] == 0 and zero["stop"] == (po.MAX_ITER if zero["planar"] >= 6 else po.STARVED)
    assert np.array_equal(_bits(zero["g"]), _bits(io.pose0(g0)))
    _final(A, B, r, zero, f"b = {b} max_iter 0")


def test_plane_icp_converges_on_a_surface():
    A, B, g0, r, g_true = surface_case()
    N = _normals(A, r)["normals"]
    res = _single(A, N, B, g0, r)
    E = _steps(A, N, B, g0, r, res, what="surface")
    _final(A, B, r, res, "surface")
    truth = io.images(B, g_true.astype(np.float32)).astype(np.float64)
    dist = lambda g: float(np.linalg.norm(io.images(B, g).astype(np.float64) - truth, axis=1).mean())
    print(f"surface: iters {res['iters']} stop {res['stop']} E {E[0]:.4e} -> {E[-1]:.4e}; distance to the true-pose images {dist(g0):.3e} -> "
          f"{dist(res['g']):.3e}; planar {res['planar']} of {res['counts'][1]} matched")
    assert res["stop"] == po.CONVERGED and 2 <= res["iters"] <= 20 and dist(res["g"]) < 0.1 * dist(g0)
    one = _single(A, N, B, g0, r, max_iter=1)                           # MAX_ITER: one update, then the stop at k = 1
    _steps(A, N, B, g0, r, one, max_iter=1, what="surface, one update")
    assert one["stop"] == po.MAX_ITER and one["iters"] == 1
    assert np.array_equal(_bits(one["g"]), _bits(res["g_trace"].reshape(-1, 3, 4)[1]))


def test_plane_icp_starved_by_the_planar_count():
    A, N = _memory(2049, seed=2)
    B, g0 = _view(A, 600, 3)
    few = np.zeros_like(N)
    few[:4] = N[:4]                                                      # four rows keep a normal: w <= 4 whatever n is
    res = _single(A, few, B, g0, SHEET_R, max_iter=5)
    _steps(A, few, B, g0, SHEET_R, res, max_iter=5, what="starved by w")
    _final(A, B, SHEET_R, res, "starved by w")
    assert res["stop"] == po.STARVED and res["iters"] == 0 and res["counts"][1] > 500 and res["planar"] <= 4
    assert np.array_equal(_bits(res["g"]), _bits(g0))
    nan_pose = g0.copy()
    nan_pose[1, 3] = np.nan                                              # every query non-finite: f = 0, E = 0, starved
    nothing = _single(A, N, B, nan_pose, SHEET_R, max_iter=5)
    assert nothing["stop"] == po.STARVED and nothing["counts"].tolist() == [0, 0, 0] and nothing["planar"] == 0 and nothing["sum_rho2"] == 0.0


def test_plane_icp_degenerate_on_a_plane():
    rng = np.random.default_rng(1)
    A = (np.concatenate([rng.uniform(-0.2, 0.2, (1500, 2)), np.zeros((1500, 1))], 1) + OFFSET).astype(F)
    B = A[:700] + F([0.001, -0.001, 0.004])
    for N in (np.tile(F([[0, 0, 1]]), (1500, 1)), _normals(A)["normals"]):       # hand-set normals, and the device's own: all (0, 0, 1)
        assert np.array_equal(N[(N != 0).any(1)], np.tile(F([[0, 0, 1]]), (int((N != 0).any(1).sum()), 1)))
        for g0 in (None, F([[1, 0, 0, 0.001], [0, 1, 0, 0], [0, 0, 1, 0]])):
            res = _single(A, N, B, g0, SHEET_R, max_iter=5)
            _steps(A, N, B, g0, SHEET_R, res, max_iter=5, what="one plane")
            _final(A, B, SHEET_R, res, "one plane")
            assert res["stop"] == po.DEGENERATE and res["iters"] == 0 and res["planar"] >= 600
            assert np.array_equal(_bits(res["g"]), _bits(io.pose0(g0)))


def test_plane_icp_ignores_non_finite_rows():
    A, N = _memory(2049, seed=0)
    B, g0 = _view(A, 500, 5)
    res = _single(A, N, B, g0, SHEET_R, max_iter=4)
    A2 = np.concatenate([F([[np.nan, 0, 0], [0, np.inf, 0]]), A, F([[-np.inf, np.nan, 1]])])
    N2 = np.concatenate([F([[0, 0, 1], [0, 0, 1]]), N, F([[0, 1, 0]])])
    B2 = np.concatenate([B[:100], F([[0, 0, np.nan], [np.inf, np.inf, np.inf]]), B[100:], F([[1, -np.inf, 1]])])
    got = _single(A2, N2, B2, g0, SHEET_R, max_iter=4)
    _steps(A2, N2, B2, g0, SHEET_R, got, max_iter=4, what="non-finite")
    _final(A2, B2, SHEET_R, got, "non-finite")
    assert got["iters"] >= 1 and got["counts"][0] == 500 and (got["idx"][[100, 101, 502]] == -1).all()
    assert got["iters"] == res["iters"] and np.abs(got["g"] - res["g"]).max() < 1e-4


# ------------------------------------------------------------------------------------------------ the ragged batch
@pytest.fixture(scope="module")
def batch():
    rng = np.random.default_rng(31)
    sA, sB, sg, sr, _ = surface_case()
    eye = io.IDENTITY
    m1, m2, m3 = _memory(700, 0), _memory(2049, 1), _memory(1025, 2)
    flat = (np.concatenate([rng.uniform(-0.2, 0.2, (400, 2)), np.zeros((400, 1))], 1) + OFFSET).astype(F)
    probs = [(np.zeros((0, 3), F), np.zeros((0, 3), F), rng.uniform(-1, 1, (300, 3)).astype(F), eye, 0.05),         # an empty A
             (m1[0], m1[1], np.zeros((0, 3), F), eye, 0.05),                                                          # an empty B
             (flat, np.tile(F([[0, 0, 1]]), (400, 1)), flat[:200] + F([0.001, 0, 0.003]), eye, 0.03),                 # degenerate
             (sA, _normals(sA, sr)["normals"], sB, sg, float(sr))]
    for (A, N), b, r in ((m1, 257, 0.03), (m2, 2000, 0.04), (m3, 600, 0.025)):
        B, g0 = _view(A, b, 1)
        probs.append((A, N, B, g0, r))
    return probs


def _run_batch(probs, packed=False, **kw):
    from livingscenes_amd import ops
    return ops.cloud_icp_plane_batch([_t(p[0]) for p in probs], [_t(p[1]) for p in probs], [_t(p[2]) for p in probs],
                                     g=_g(np.stack([p[3] for p in probs])), radius=[p[4] for p in probs], trace=True, packed=packed, **kw)


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
    iters, stops = [x["iters"] for x in res], [x["stop"] for x in res]
    print("batch iters", iters, "stop", stops)
    assert stops[:3] == [po.STARVED, po.STARVED, po.DEGENERATE] and iters[:3] == [0, 0, 0]
    assert len(set(iters)) >= 3 and min(iters[3:]) >= 1, iters           # problems stop at different k: the stopped ones stay frozen
    cut = sorted(set(iters[3:]))[1]                                      # whoever stopped before `cut` keeps its bits while the others run on
    short = [_host(x) for x in _run_batch(batch, max_iter=cut)]
    assert sum(x["iters"] < cut for x in res[3:]) >= 1
    for p in range(P):
        if res[p]["iters"] < cut:
            _identical({k: v for k, v in short[p].items() if "trace" not in k}, res[p], f"problem {p}, a shorter run")
            assert np.array_equal(_bits(short[p]["g_trace"][:res[p]["iters"] + 1]), _bits(res[p]["g_trace"][:res[p]["iters"] + 1]))
    _steps(*batch[5], res[5], what="batch problem 5", **kw)
    _final(batch[6][0], batch[6][2], batch[6][4], res[6], "batch problem 6")
    pk = _run_batch(batch, packed=True, **kw)                            # the packed form: the same result
    assert pk["b_off"].tolist() == np.cumsum([0] + [p[2].shape[0] for p in batch]).tolist() and tuple(pk["g"].shape) == (P, 3, 4)
    assert pk["stop"].dtype == np.int32 and pk["stop"].tolist() == stops and pk["iters"].tolist() == iters
    assert pk["planar"].tolist() == [x["planar"] for x in res] and pk["sum_rho2"].tolist() == [x["sum_rho2"] for x in res]
    assert np.array_equal(_bits(pk["g"]), _bits(np.stack([x["g"] for x in res]))) and np.array_equal(pk["counts"], np.stack([x["counts"] for x in res]))
    assert np.array_equal(pk["idx"].cpu().numpy(), np.concatenate([x["idx"] for x in res])) and pk["sum_d2"].tolist() == [x["sum_d2"] for x in res]


def test_errors_name_the_problem(batch):
    from livingscenes_amd import _lib, ops
    tA, tN, tB = ([_t(p[k]) for p in batch] for k in range(3))
    rs = [p[4] for p in batch]
    with pytest.raises(_lib.LsError, match="problem 4.*radius"):
        ops.cloud_icp_plane_batch(tA, tN, tB, radius=rs[:4] + [float("nan")] + rs[5:])
    for kw, word in (({"max_iter": -1}, "max_iter"), ({"min_matched": 2}, "min_matched"), ({"rel_thr": -1.0}, "rel_thr")):
        with pytest.raises(_lib.LsError, match=word):
            ops.cloud_icp_plane_batch(tA, tN, tB, radius=rs, **kw)
        with pytest.raises(_lib.LsError, match=word):
            ops.cloud_icp_plane(tA[4], tN[4], tB[4], radius=0.03, **kw)
    with pytest.raises(_lib.LsError, match="no CPU fallback"):
        ops.cloud_icp_plane(torch.zeros(3, 3), torch.zeros(3, 3), torch.zeros(3, 3), radius=0.1)
    with pytest.raises(ValueError, match="one normal row per kept row"):
        ops.cloud_icp_plane(tA[4], tN[4][:-1], tB[4], radius=0.1)
    with pytest.raises(ValueError):
        ops.cloud_icp_plane_batch(tA, tN[:-1], tB, radius=0.1)


# ------------------------------------------------------------------------------------------------ the layers above
def test_refine_on_memory_batch_plane():
    from livingscenes_amd import ops
    from livingscenes_amd.lib_math.torch_se3 import inverse
    d = _dev()
    solver = _solver(object())
    mems, news, Ts = [], [], []
    for k, seed in enumerate((5, 6)):
        A, B, g0, r, g_true = surface_case(seed=seed)
        T_true = np.eye(4)
        T_true[:3] = _inv(g_true)                                        # memory -> rescan
        mems.append(_t(A)), news.append(_t(B))
        Ts.append(_perturbed(T_true, k, A.astype(np.float64).mean(0)).astype(np.float32))
    mems.append(_t(np.zeros((0, 3), F))), news.append(news[0].clone())   # an empty memory: starved, the slot keeps its T
    Ts.append(Ts[0] + F(0.125))
    T = torch.from_numpy(np.stack(Ts)).to(d)
    nrm = solver._memory_normals_batch(mems)
    direct = ops.cloud_normals_batch(mems, radius=0.03)                  # the derived default: 3 * 0.01
    assert all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) and np.array_equal(x[3], y[3]) for x, y in zip(nrm, direct))
    T2, info = solver._refine_on_memory_batch(mems, news, T, 0.03, metric="plane", max_iter=30)
    assert set(info) == {"g", "stop", "iters", "overlap", "rmse", "memory_seen", "counts", "nn_idx", "planar"}
    want = ops.cloud_icp_plane_batch(mems, [x[0] for x in direct], news, g=inverse(T), radius=0.03, max_iter=30, packed=True)
    assert torch.equal(info["g"], want["g"]) and info["stop"].tolist() == want["stop"].tolist() and info["iters"].tolist() == want["iters"].tolist()
    assert info["planar"].tolist() == want["planar"].tolist()
    assert info["iters"][2] == 0 and info["stop"][2] == po.STARVED and np.array_equal(_bits(T2[2, :3]), _bits(T[2, :3]))
    for k in range(2):
        print(f"pair {k}: iters {info['iters'][k]} stop {info['stop'][k]} planar {info['planar'][k]} overlap {info['overlap'][k]:.3f}")
        assert info["iters"][k] >= 1 and np.array_equal(_bits(T2[k, :3]), _bits(inverse(info["g"][k:k + 1])[0]))
    ov = solver._overlap_batch(mems, news, None, radius=0.03, g=info["g"])
    assert ov["overlap"] == info["overlap"] and all(np.array_equal(a, b) for a, b in zip(ov["counts"], info["counts"]))
    wide, _ = solver._refine_on_memory_batch(mems, news, T, 0.03, metric="plane", normal_radius=0.05, max_iter=30)
    assert tuple(wide.shape) == (3, 4, 4)
    with pytest.raises(ValueError, match="metric"):
        solver._refine_on_memory_batch(mems, news, T, 0.03, metric="surface")


def test_solve_sequence_refine_metric(small_prior, monkeypatch):
    from livingscenes_amd.lib_more import more_solver
    solver = _solver(small_prior)
    n, h = 4, 0.02
    pair = synth.make_scene_pair(n, 700, seed=71, noise=0.002)
    ref, rescan = _scene(pair["ref"]), _scene(pair["rescan"])
    gt = (pair["rescan_T"].double() @ torch.linalg.inv(pair["ref_T"].double())).numpy()
    ref_pts = pair["ref"].numpy()

    def truth(pc1, pc2):
        return gt[next(i for i in range(n) if (ref_pts[i, 0] == pc1[0].cpu().numpy()).all())]

    calls = _counted(monkeypatch, solver, truth)
    base, _ = more_solver.solve_sequence(solver, ref, [rescan], voxel=h, refine_radius=0.04)
    point, _ = more_solver.solve_sequence(solver, ref, [rescan], voxel=h, refine_radius=0.04, refine_metric="point", normal_radius=0.1)
    assert set(point[0]) == set(base[0]) == STEP_KEYS | REFINE_KEYS
    _step_values_equal(point[0], base[0])                                # "point" is the path without the new arguments, bit for bit
    for key in ("refine_stop", "refine_iters"):
        assert point[0][key] == base[0][key]
    assert all(torch.equal(a, b) for a, b in zip(point[0]["registration_init"], base[0]["registration_init"]))
    before = dict(calls)
    steps, memory = more_solver.solve_sequence(solver, ref, [rescan], voxel=h, refine_radius=0.04, refine_metric="plane", normal_radius=0.1,
                                               overlap_radius=0.04, min_overlap=0.0)
    st = steps[0]
    assert set(st) == STEP_KEYS | GATE_KEYS | REFINE_KEYS
    assert calls["refine"] == before["refine"] + 1 and calls["overlap"] == before["overlap"] and calls["registration"] == before["registration"] + 1
    for i in range(n):
        assert st["refine_stop"][i] in (0, 1, 2, 3) and st["refine_iters"][i] >= 0 and 0.0 <= st["overlap"][i] <= 1.0
        assert torch.equal(st["registration_init"][i], base[0]["registration_init"][i])
        print(f"slot {i}: plane refinement iters {st['refine_iters'][i]} stop {st['refine_stop'][i]} overlap {st['overlap'][i]:.3f}")
        if st["refine_iters"][i] == 0:                                   # no fallback: the pose the pair came with
            assert torch.equal(st["registration"][i], st["registration_init"][i])
    assert len(memory["clouds"]) == n
    with pytest.raises(ValueError, match="refine_radius"):
        more_solver.solve_sequence(solver, ref, [rescan], voxel=h, refine_metric="plane")
