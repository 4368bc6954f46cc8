"""GPU tests of the scene memory's projection onto local planes (csrc/cloudnear.hip: ls_cloud_project_f32 / ls_cloud_project_batch_f32;
ops.cloud_project*) and of the layers on top (More_Solver._consolidate_batch, solve_sequence(consolidate=True)).

Integers.  nbr-derived quantities are int64 sums of the same integers on both sides, the covariance is the same float64 expression of them
(the same bits), and the validity rule is a comparison of eigenvalues that the inputs keep away from its threshold (eigen_gap_ok of
tests/test_cloud_plane_cpu.py, asserted on the twin).  So `state` and `counts` must EQUAL those of tests/project_oracle.py wherever no limit
is set; where a test sets a limit it first asserts on the twin that no row's variation or distance lies within the bounds below of it.

Floats.  The eigenvectors come from two float64 solvers (Jacobi on the device, LAPACK in the twin).  A backward-stable solver returns the
eigenvector of C + dC with |dC| <= c 2^-52 |C|; the eigenvector of l0 then moves by at most |dC| / (l1 - l0), and eigen_gap_ok asserts
(l1 - l0) / l2 >= 1e-3, so the float64 unit normals differ -- up to the sign, which the result does not depend on -- by at most
EPS_N = 2^-35 per component (c up to 128, the allowance of the normals' tests).  The offset d is the same bits on both sides, |d_k| <= r
(|q| <= 2^15 in units of r 2^-15), so
  s         = (d_0 n_0 + d_1 n_1) + d_2 n_2 differs by at most E_s = 3 r (EPS_N + 2^-51): the normal's error and five float64 roundings
  shift     = float32(|s|): two roundings of values E_s apart differ by at most E_s plus one fp32 ulp of the value, 2^-23 |s|
  out_pts_k = float32(A_k - s n_k): the float64 values differ by at most E_x = E_s + 2 r EPS_N + 2^-51 (|A_k| + 2 r) (|n_k| <= 1,
              |s| <= sqrt(3) r < 2 r, two roundings); E_x is about 1e-12, five orders below an fp32 ulp of a coordinate of order 1, so
              the two fp32 roundings agree except where the value sits at a rounding tie: at most E_x plus ONE ulp of the coordinate
  sum_shift2  a float64 sum of `moved` non-negative terms: within moved 2^-52 S of math.fsum of its own terms, the bound the ICP tests use
              for S; the terms s^2 themselves differ by at most 2 |s| E_s + E_s^2 each, which is added
None of these is fitted to an observed error.  Batches, reversed batches and second runs are compared bit for bit with the single operator.

Consolidation.  The merge is integer-exact, so More_Solver._consolidate_batch is compared, rows and order, with merge_oracle.merge of the
DEVICE's own projected points: a 1-ulp difference between the twin's points and the device's could move a point across a voxel face."""
import math

import numpy as np
import pytest
import torch

import merge_oracle as mo
import project_oracle as pjo
from cloud_testlib import CODE_KEYS, F, _bits, _scene, _solver, _t, small_prior  # noqa: F401 (small_prior is a fixture)
from livingscenes_amd import synth
from test_cloud_plane_cpu import SHEET_R, eigen_gap_ok, hand_cases, sheet
from test_cloud_project_cpu import lattice, lifted, noisy_sphere_memory

pytestmark = pytest.mark.gpu

INF = float("inf")
EPS_N = 2.0 ** -35


def _project(A, r=SHEET_R, min_nbrs=5, max_variation=1 / 3, max_shift=INF):
    from livingscenes_amd import ops
    pts, state, shift, counts, sum2 = ops.cloud_project(_t(A), radius=r, min_nbrs=min_nbrs, max_variation=max_variation, max_shift=max_shift)
    a = np.asarray(A).reshape(-1, 3).shape[0]
    assert pts.dtype == torch.float32 and state.dtype == torch.int32 and shift.dtype == torch.float32 and counts.dtype == np.int64
    assert tuple(pts.shape) == (a, 3) and tuple(state.shape) == tuple(shift.shape) == (a,) and counts.shape == (4,) and isinstance(sum2, float)
    return {"points": pts.cpu().numpy(), "state": state.cpu().numpy(), "shift": shift.cpu().numpy(), "counts": counts, "sum_shift2": sum2}


def _bounds(A, r, tw):
    """E_s and E_x [a,3] of the module docstring"""
    r = float(r)
    e_s = 3 * r * (EPS_N + 2.0 ** -51)
    return e_s, e_s + 2 * r * EPS_N + 2.0 ** -51 * (np.abs(A.astype(np.float64)) + 2 * r)


def _limits_clear(tw, r, max_variation, max_shift, A):
    """the condition on the inputs under which a limit decides the same way on both sides"""
    e_s, _ = _bounds(A, r, tw)
    plane = tw["state"] >= pjo.HELD
    mv, ms = float(np.float32(max_variation)), float(np.float32(max_shift))
    var_ok = (np.abs(tw["variation"][plane] - mv) > 2.0 ** -44) | (tw["variation"][plane] == 0.0) if mv < 1 / 3 else True
    s_abs = np.abs(tw["s"][plane])
    s_ok = (np.abs(s_abs - ms) > e_s) | (s_abs == 0.0) if ms < INF else True
    return bool(np.all(var_ok) and np.all(s_ok))


def _check(got, tw, A, r, what="", gap=True):
    """the comparison of the module docstring; no row is skipped"""
    A = np.ascontiguousarray(A, dtype=np.float32).reshape(-1, 3)
    if gap:
        ntw = {"lam": tw["lam"], "valid": tw["state"] >= pjo.HELD}
        assert eigen_gap_ok(ntw), (what, "the inputs do not meet the eigen-gap condition")
    assert np.array_equal(got["state"], tw["state"]), (what, "state", np.flatnonzero(got["state"] != tw["state"])[:5])
    assert np.array_equal(got["counts"], tw["counts"]), (what, got["counts"], tw["counts"])
    e_s, e_x = _bounds(A, r, tw)
    st = tw["state"]
    fixed = st != pjo.MOVED
    assert np.array_equal(_bits(got["points"][fixed]), _bits(A[fixed])), (what, "a row that is not moved is the input bit for bit")
    assert not got["shift"][st < pjo.HELD].any(), (what, "shift of a row without a plane")
    sd, stw = got["shift"].astype(np.float64), tw["shift"].astype(np.float64)
    assert (np.abs(sd - stw) <= e_s + 2.0 ** -23 * stw).all(), (what, "shift", np.abs(sd - stw).max())
    pd, pt = got["points"].astype(np.float64), tw["points"].astype(np.float64)
    with np.errstate(invalid="ignore"):
        bad = np.abs(pd - pt) > e_x + np.spacing(np.abs(tw["points"])).astype(np.float64)
    assert not bad[st == pjo.MOVED].any(), (what, "points", np.abs(pd - pt)[st == pjo.MOVED].max())
    moved = int(tw["counts"][3])
    s_abs = np.abs(tw["s"][st == pjo.MOVED])
    S = math.fsum((s_abs * s_abs).tolist())
    tol = moved * 2.0 ** -52 * S + float((2 * s_abs * e_s + e_s * e_s).sum())
    assert abs(got["sum_shift2"] - S) <= tol, (what, "sum_shift2", got["sum_shift2"], S, tol)
    # and against the device's own rows: the float64 sum of the squares of its fp32 shifts, each within 2^-23 of its s^2
    own = math.fsum((sd[st == pjo.MOVED] ** 2).tolist())
    assert abs(got["sum_shift2"] - own) <= 2.0 ** -22 * own + moved * 2.0 ** -52 * own, (what, "sum_shift2 against the shifts")


# ------------------------------------------------------------------------------------------------ the device against the twin
PROJECT_SIZES = [0, 1, 4, 5, 255, 256, 257, 513, 3001]


@pytest.mark.parametrize("a", PROJECT_SIZES)
def test_project_size_edges(a):
    A = sheet(a, seed=a % 3)
    got, tw = _project(A), pjo.project(A, F(SHEET_R), 5)
    _check(got, tw, A, SHEET_R, f"a = {a}")
    from livingscenes_amd import ops
    nbr = ops.cloud_normals(_t(A), radius=SHEET_R)[1].cpu().numpy()     # the operator returns no neighbour counts: the normals' are its own
    assert np.array_equal(nbr, tw["nbr_cnt"]) and np.array_equal(got["state"] >= pjo.HELD, nbr >= 5)
    assert got["counts"].sum() == a and got["counts"][0] == 0
    if a >= 255:
        assert got["counts"][3] >= 0.99 * a and got["sum_shift2"] > 0 and (got["points"] != A).any()
    if a < 5:
        assert got["counts"].tolist() == [0, a, 0, 0] and got["sum_shift2"] == 0.0
    lo = _project(A, min_nbrs=1)                                        # the count rule off: the rank rule alone
    _check(lo, pjo.project(A, F(SHEET_R), 1), A, SHEET_R, f"a = {a}, min_nbrs 1")


def test_project_limits_on_a_surface():
    A = sheet(3001)
    for mv, ms in ((0.0015, INF), (1 / 3, 0.0004), (0.0015, 0.0004)):
        tw = pjo.project(A, F(SHEET_R), 5, mv, ms)
        assert _limits_clear(tw, SHEET_R, mv, ms, A), "a row sits at a limit: choose another"
        assert tw["counts"][2] > 100 and tw["counts"][3] > 100             # the limit holds some rows and lets others move
        _check(_project(A, max_variation=mv, max_shift=ms), tw, A, SHEET_R, f"limits {mv}, {ms}")


def test_project_one_crowded_cell():
    """5 000 jittered points in one cell: every row has 5 000 neighbours, the second moments reach 5 000 * 2^30"""
    rng = np.random.default_rng(5)
    A = (np.array([3.0151, -1.9851, 0.515]) + rng.uniform(-0.004, 0.004, (5000, 3)) * [1, 1, 0.1]).astype(np.float32)
    tw = pjo.project(A, F(SHEET_R), 5)
    assert (tw["nbr_cnt"] == 5000).all() and np.unique(mo.cells(A, F(SHEET_R))[0], axis=0).shape[0] == 1
    got = _project(A)
    _check(got, tw, A, SHEET_R, "one cell")
    assert got["counts"].tolist() == [0, 0, 0, 5000]


def test_project_far_from_the_origin():
    """the cloud on a grid of 2^-15, so that 300 m more on every axis is exact in fp32: the offsets, the integer moments and with them s
    are the same numbers, and the twin confirms that the shifted cells change no neighbourhood -- state and shift must be the same BITS,
    and a moved row lands where it landed plus 300 m, to half an ulp there (2^-16) and half an ulp here (2^-23)"""
    A = (np.round(sheet(2049, seed=1).astype(np.float64) * 2 ** 15) / 2 ** 15).astype(np.float32)
    T = np.array([300.0, -300.0, 300.0])
    far = (A.astype(np.float64) + T).astype(np.float32)
    assert np.array_equal(far.astype(np.float64), A.astype(np.float64) + T)
    tw, tw_far = pjo.project(A, F(SHEET_R), 5), pjo.project(far, F(SHEET_R), 5)
    assert np.array_equal(tw["nbr_cnt"], tw_far["nbr_cnt"]) and np.array_equal(tw["s"], tw_far["s"])
    got, got_far = _project(A), _project(far)
    _check(got, tw, A, SHEET_R, "near")
    _check(got_far, tw_far, far, SHEET_R, "300 m")
    assert np.array_equal(got["state"], got_far["state"]) and np.array_equal(_bits(got["shift"]), _bits(got_far["shift"]))
    assert got["sum_shift2"] == got_far["sum_shift2"] and got["counts"][3] > 1900
    assert np.abs(got_far["points"].astype(np.float64) - (got["points"].astype(np.float64) + T)).max() <= 2.0 ** -16 + 2.0 ** -23


def test_project_ignores_non_finite_rows():
    A = sheet(600, seed=2)
    A2 = np.concatenate([F([[np.nan, 0, 0], [0, np.inf, 0]]), A[:300], F([[-np.inf, np.nan, 1]]), A[300:]])
    got, tw = _project(A2), pjo.project(A2, F(SHEET_R), 5)
    bad = [0, 1, 302]
    finite = np.setdiff1d(np.arange(603), bad)
    assert got["state"][bad].tolist() == [0, 0, 0] and not got["shift"][bad].any() and got["counts"][0] == 3
    assert np.array_equal(_bits(got["points"][bad]), _bits(A2[bad]))    # NaN payloads and infinities pass through bit for bit
    _check(got, tw, A2, SHEET_R, "non-finite")
    clean = _project(A)
    for k in ("points", "state", "shift"):
        assert np.array_equal(_bits(got[k][finite]), _bits(clean[k])), k  # the same rows between the ones that are ignored
    nothing = _project(np.full((300, 3), np.nan, np.float32))
    assert nothing["counts"].tolist() == [300, 0, 0, 0] and nothing["sum_shift2"] == 0.0 and not nothing["shift"].any()


def test_project_hand_written():
    A = lattice()
    got = _project(A, 0.03)
    _check(got, pjo.project(A, F(0.03), 5), A, 0.03, "lattice", gap=False)
    assert got["counts"].tolist() == [0, 0, 0, 81] and not got["shift"].any() and got["sum_shift2"] == 0.0
    assert np.array_equal(_bits(got["points"]), _bits(A))               # a fixed point, bit for bit
    assert _project(A, 0.03, max_variation=0.0, max_shift=0.0)["counts"].tolist() == [0, 0, 0, 81]
    for name, B, r, k, valid, _ in hand_cases():
        got = _project(B, r, k)
        _check(got, pjo.project(B, F(r), k), B, r, name, gap=False)
        if not any(valid):                                              # collinear, coincident, m = min_nbrs - 1
            assert got["state"].tolist() == [1] * len(B) and np.array_equal(_bits(got["points"]), _bits(B)), name
    L, i = lifted()
    free, held = _project(L, 0.03), _project(L, 0.03, max_shift=0.0)
    _check(free, pjo.project(L, F(0.03), 5), L, 0.03, "lifted", gap=False)
    _check(held, pjo.project(L, F(0.03), 5, 1 / 3, 0.0), L, 0.03, "lifted, held", gap=False)
    assert free["state"].tolist() == [3] * 81 and held["state"][i] == 2 and np.array_equal(_bits(held["points"]), _bits(L))
    assert 0.002 < free["shift"][i] < 0.004 and abs(free["points"][i, 2]) < 0.002 and held["shift"][i] == free["shift"][i]
    S = sheet(257)
    none = _project(S, max_variation=0.0)                               # holds everything that is not exactly planar
    assert none["counts"][3] == 0 and none["counts"][2] > 250 and np.array_equal(_bits(none["points"]), _bits(S)) and none["sum_shift2"] == 0.0


# ------------------------------------------------------------------------------------------------ a ragged batch
def test_batch_is_the_single_op_reversed_and_again():
    from livingscenes_amd import _lib, ops
    clouds = [sheet(700, 0), np.zeros((0, 3), F), sheet(257, 1), hand_cases()[1][1], sheet(2 ** 12 + 5, 2), sheet(1, 0), sheet(513, 0)]
    radii = [0.03, 0.05, 0.04, 0.03, 0.03, 0.02, 0.03]
    kw = {"max_variation": 0.0015, "max_shift": 0.0006}
    res = ops.cloud_project_batch([_t(c) for c in clouds], radius=radii, **kw)
    alone = [ops.cloud_project(_t(c), radius=r, **kw) for c, r in zip(clouds, radii)]
    rev = ops.cloud_project_batch([_t(c) for c in clouds[::-1]], radius=radii[::-1], **kw)[::-1]
    again = ops.cloud_project_batch([_t(c) for c in clouds], radius=radii, **kw)
    for p in range(7):
        for other in (alone[p], rev[p], again[p]):
            assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(res[p][:3], other[:3])), p
            assert np.array_equal(res[p][3], other[3]) and res[p][4] == other[4], p
        assert res[p][3].sum() == len(clouds[p])
    assert res[1][3].tolist() == [0, 0, 0, 0] and res[3][3].tolist() == [0, 7, 0, 0] and res[5][3].tolist() == [0, 1, 0, 0]
    assert all(res[p][3][2] > 20 and res[p][3][3] > 20 and res[p][4] > 0 for p in (0, 2, 4, 6))   # the limits hold some rows, others move
    free = ops.cloud_project_batch([_t(c) for c in clouds], radius=radii)
    for p in (0, 2, 4, 6):
        got = {"points": free[p][0].cpu().numpy(), "state": free[p][1].cpu().numpy(), "shift": free[p][2].cpu().numpy(), "counts": free[p][3],
               "sum_shift2": free[p][4]}
        _check(got, pjo.project(clouds[p], F(radii[p]), 5), clouds[p], radii[p], f"problem {p}")
    pts, state, shift, counts, sums, off = ops.cloud_project_batch([_t(c) for c in clouds], radius=radii, packed=True, **kw)
    assert off.tolist() == np.cumsum([0] + [len(c) for c in clouds]).tolist() and tuple(counts.shape) == (7, 4) and tuple(sums.shape) == (7,)
    assert torch.equal(pts, torch.cat([x[0] for x in res])) and torch.equal(state, torch.cat([x[1] for x in res]))
    assert torch.equal(shift, torch.cat([x[2] for x in res]))
    with pytest.raises(_lib.LsError, match="problem 4.*radius"):
        ops.cloud_project_batch([_t(c) for c in clouds], radius=radii[:4] + [float("nan")] + radii[5:])
    with pytest.raises(_lib.LsError, match="max_shift"):
        ops.cloud_project(_t(clouds[0]), radius=0.03, max_shift=-1.0)
    with pytest.raises(_lib.LsError, match="max_variation"):
        ops.cloud_project(_t(clouds[0]), radius=0.03, max_variation=float("nan"))
    with pytest.raises(_lib.LsError, match="no CPU fallback"):
        ops.cloud_project(torch.zeros(3, 3), radius=0.1)


# ------------------------------------------------------------------------------------------------ the layers above
def test_consolidate_batch_is_the_merge_of_the_device_projection():
    from livingscenes_amd import ops
    sphere, centre = noisy_sphere_memory()
    mems = [_t(sphere), _t(sheet(3001)), _t(np.zeros((0, 3), F)), _t(hand_cases()[1][1])]
    h = 0.01
    solver = _solver(object(), {"accumulate": {"voxel_size": h}})
    clouds, info = solver._consolidate_batch(mems)
    proj = ops.cloud_project_batch(mems, radius=0.03)                    # the derived default: 3 * 0.01
    assert set(info) == {"rows_before", "rows_after", "moved", "held", "no_plane", "rms_shift"} and all(len(v) == 4 for v in info.values())
    for p in range(4):
        want, _ = mo.merge(proj[p][0].cpu().numpy(), np.zeros((0, 3), F), None, h)
        assert np.array_equal(_bits(clouds[p]), _bits(want)), p          # rows and order
        assert info["rows_before"][p] == mems[p].shape[0] and info["rows_after"][p] == want.shape[0]
        assert [info[k][p] for k in ("no_plane", "held", "moved")] == proj[p][3][1:].tolist()
        rms = math.sqrt(proj[p][4] / info["moved"][p]) if info["moved"][p] else float("nan")
        assert info["rms_shift"][p] == rms or (math.isnan(rms) and math.isnan(info["rms_shift"][p]))
    assert info["rows_after"][0] < info["rows_before"][0] and info["held"] == [0, 0, 0, 0] and info["no_plane"][3] == 7
    assert math.isnan(info["rms_shift"][2]) and math.isnan(info["rms_shift"][3]) and info["rows_after"][2] == 0
    # the quality condition of the CPU tests on the device's own output, at the radius of those tests and an explicit voxel
    tight, t_info = solver._consolidate_batch(mems[:1], radius=0.02, voxel=h, max_shift=INF)
    rms = lambda X: float(np.sqrt(np.mean((np.linalg.norm(X.astype(np.float64) - centre, axis=1) - 0.15) ** 2)))
    assert rms(tight[0].cpu().numpy()) < 0.5 * rms(sphere) and 0.5 * 0.002 < t_info["rms_shift"][0] < 2 * 0.002
    limited, l_info = solver._consolidate_batch(mems[:2], max_variation=0.0015, max_shift=0.0004)
    assert l_info["held"][1] > 0 and l_info["moved"][1] > 0 and l_info["held"][1] + l_info["moved"][1] + l_info["no_plane"][1] == 3001


def test_solve_sequence_consolidates_once_after_the_last_rescan(small_prior, monkeypatch):
    from livingscenes_amd.lib_more import more_solver
    solver = _solver(small_prior)
    n, h = 4, 0.02
    s1, s2 = synth.make_scene_pair(n, 700, seed=71, noise=0.002), synth.make_scene_pair(n, 500, seed=71, noise=0.004)
    ref, rescans = _scene(s1["ref"]), [_scene(s1["rescan"]), _scene(s2["rescan"])]
    plain_steps, plain = more_solver.solve_sequence(solver, ref, rescans, voxel=h)
    off_steps, off = more_solver.solve_sequence(solver, ref, rescans, voxel=h, consolidate=False, consolidate_radius=0.05,
                                                consolidate_max_variation=0.1, consolidate_max_shift=0.01)
    # consolidate=False: every returned object is what it is without the arguments
    assert set(off) == set(plain) == {"clouds", "codes", "meshes"} and len(off_steps) == len(plain_steps)
    for i in range(n):
        assert torch.equal(off["clouds"][i], plain["clouds"][i]), i
    for key in CODE_KEYS:
        assert torch.equal(off["codes"][key], plain["codes"][key]), key
    for a, b in zip(off_steps, plain_steps):
        assert set(a) == set(b) and a["merged_sizes"] == b["merged_sizes"] and torch.equal(a["matches"], b["matches"])

    calls, events, forced = [], [], 1

    def spy(mem_pcs, *args, _real=solver._consolidate_batch, **kw):
        calls.append((len(mem_pcs), kw))
        events.append("consolidate")
        clouds, info = _real(mem_pcs, *args, **kw)
        clouds[forced] = clouds[forced][:100]                            # below n_input_point = 128: the slot must keep its cloud and code
        return clouds, info
    monkeypatch.setattr(solver, "_consolidate_batch", spy)

    def encode(model, clouds, _real=more_solver._encode_clouds):
        events.append(f"encode {len(clouds)}")
        return _real(model, clouds)
    monkeypatch.setattr(more_solver, "_encode_clouds", encode)
    steps, memory = more_solver.solve_sequence(solver, ref, rescans, voxel=h, consolidate=True)
    monkeypatch.undo()
    # ONE call over all slots, after the last rescan, then ONE encoder batch of the slots that took their consolidated cloud
    assert len(calls) == 1 and calls[0][0] == n and events[-2:] == ["consolidate", f"encode {n - 1}"] and len(events) >= 3
    assert calls[0][1] == {"radius": None, "voxel": h, "max_variation": 1 / 3, "max_shift": INF}
    for a, b in zip(steps, plain_steps):                                 # the steps do not know of it
        assert a["merged_sizes"] == b["merged_sizes"] and torch.equal(a["matches"], b["matches"])
        assert all(torch.equal(x, y) for x, y in zip(a["ref_pc_lst"], b["ref_pc_lst"]))
    want, info = solver._consolidate_batch(plain["clouds"], voxel=h)
    cons = memory["consolidation"]
    assert cons["kept_as_is"] == [forced] and {k: cons[k] for k in info} == info and set(cons) == set(info) | {"kept_as_is"}
    assert all(info["moved"][i] > 0 for i in range(n)) and all(r >= 128 for r in info["rows_after"])
    for i in range(n):
        if i == forced:
            assert torch.equal(memory["clouds"][i], plain["clouds"][i])
            for key in CODE_KEYS:
                assert torch.equal(memory["codes"][key][i], plain["codes"][key][i]), (i, key)
        else:
            c = memory["clouds"][i]
            assert torch.equal(c, want[i]) and not torch.equal(c, plain["clouds"][i][: c.shape[0]])
            direct = small_prior.encode_fps(c.T[None].contiguous(), torch.ones(1, 1, c.shape[0], dtype=torch.bool, device=c.device))
            for key in CODE_KEYS:
                assert torch.equal(memory["codes"][key][i], direct[key][0]), (i, key)
