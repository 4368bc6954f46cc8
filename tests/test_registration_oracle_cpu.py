"""CPU side of the registration ladders (tests/tools/registration_vs_float64.py; the GPU side is tests/test_hip_registration_f64.py): the inputs
meet their preconditions, the float64 oracles of tests/registration_oracle.py reproduce the committed reference outputs, and the rule catches a
planted wrong answer.  No GPU, nothing from the library."""
import importlib.util
import os

import numpy as np
import pytest

TOOL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools", "registration_vs_float64.py")


def _load():
    spec = importlib.util.spec_from_file_location("registration_vs_float64", TOOL)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


lad = _load()   # one module object: the references it caches serve every test of this file
ro = lad.ro
F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------ the preconditions
def test_every_input_of_the_ladders_meets_its_preconditions():
    """Kabsch, pseudo-points, residual matrix: gap >= 0.01 and e32_min <= e32 <= 1e-5 for every problem and measure.  ICP: icp_well_posed -- the
    certificate, the float32 oracle on the float64 trajectory (iteration count and final assignment), e32 in range.  Prints what the history
    records: the range of e32 and, per ICP case, e32 and the smallest certificate margin."""
    lines, bad = lad.cpu_report()
    print("\n".join(lines))
    assert not bad, f"{len(bad)} failures:\n" + "\n".join(bad[:20])


def test_the_ladders_reach_what_they_are_for():
    """every n and b of the Kabsch ladder with every kind and weights; the pseudo-point widths on both sides of 256 with every selector form, a
    negative and a repeated entry in each; both ICP families: every slot count of a thread, both sides of 64 KB of LDS, the advertised maxima,
    trajectories of 2 up to at least 5 iterations, n < m and n > m"""
    kb = lad.kabsch_ladder()
    assert len(kb) == len({c[0] for c in kb}) == 10 * 4 * 4 * 3
    assert {c[1] for c in kb} == {3, 4, 63, 64, 65, 255, 256, 257, 320, 1000} and {c[2] for c in kb} == {1, 3, 4, 5}
    x1, _, w, raw = lad.kabsch_inputs(next(c for c in kb if c[1] == 65 and c[4] == "raw_zeros"))
    assert raw and int((w == 0).sum(1).min()) == 65 // 3 and abs(float(w.sum(1).max()) - 1.0) > 0.1          # zeroed, not renormalised
    assert float(np.abs(lad.kabsch_inputs(next(c for c in kb if c[3] == "far"))[0].mean(1) - np.array([10, -7, 3])).max()) < 1.5
    for _, (s1, s2) in lad.CODE_SELECTORS.items():
        for sel in (s1, s2):
            assert sel is None or (min(sel) < 0 and len(set(sel)) < len(sel) and max(sel) < lad.CODE_SETS)
    assert {len(r) % 4 for r in (lad.codes_reference(c) for c in lad.codes_ladder())} == {1, 2, 3}           # partly filled last workgroups
    assert any((0 in nm) for c in lad.resmat_ladder() for nm in c[1])
    icp = lad.icp_ladder()
    assert {(c[2] + 1023) // 1024 for c in icp} == {1, 2, 3, 4} and {c[3] * 12 > 65536 for c in icp} == {False, True}
    assert max(c[2] for c in icp) == lad.ICP_N_MAX and max(c[3] for c in icp) == lad.ICP_M_MAX
    assert any(c[2] < c[3] for c in icp) and any(c[2] > c[3] for c in icp)
    its = [lad.icp_reference(c)["ref"].iterations for c in icp if c[1] == "dynamic"]
    assert min(its) >= 2 and max(its) >= 5 and len(set(its)) >= 3, its
    assert len(set(lad.icp_batch_inputs()[4])) == 3


# ------------------------------------------------------------------------------------------------ the oracles
def test_the_kabsch_oracle_reproduces_the_committed_reference_outputs(golden):
    """tests/golden/registration.npz holds the reference implementation's float32 outputs on 32 isotropic problems of 256 points, 16 of them
    with a reflected target, without and with weights.  They are one more float32 evaluation of the function the oracle states, so they are
    held to the rule the kernels are held to: over the 32 problems, err <= min(16 x e32, 1e-4) per measure, e32 this module's float32 side."""
    g = golden("registration")
    for tag, w in (("", None), ("w", g["kab_w"])):
        err, e32 = dict.fromkeys(lad.KB_MEASURES, 0.0), dict.fromkeys(lad.KB_MEASURES, 0.0)
        for p in range(g["kab_x1"].shape[0]):
            x1, x2 = g["kab_x1"][p], g["kab_x2"][p]
            r64, r32 = (ro.kabsch(x1, x2, None if w is None else w[p], dtype=d) for d in (F64, F32))
            s = lad.scale_of(x1, x2)
            for k, v in lad.kabsch_errs((g["kab_R" + tag][p], g["kab_t" + tag][p], g["kab_res" + tag][p]), r64, s).items():
                err[k] = max(err[k], v)
            for k, v in lad.kabsch_errs(r32, r64, s).items():
                e32[k] = max(e32[k], v)
            assert abs(float(np.linalg.det(r64[0])) - 1.0) < 1e-12
        print(f"golden{tag}: err {err}  e32 {e32}")
        for k in err:
            assert err[k] <= lad.bound(e32[k]), (tag, k, err[k], e32[k])


def test_the_entry_wrappers_of_the_kabsch_oracle():
    """pseudo-points are the float32 sums, a negative selector reads set 0, the default pairing is p with p; the residual matrix is the mean
    residual of every pair"""
    z1, t1, z2, t2, _, _ = lad.codes_inputs(lad.codes_ladder()[0])
    p1, p2 = ro.pseudo_points(z1, t1), ro.pseudo_points(z2, t2)
    assert p1.dtype == F32 and np.array_equal(p1[2], (z1[2] + t1[2]).astype(F32))
    out = ro.kabsch_codes(z1, t1, z2, t2, sel1=np.array([4, -3]), sel2=np.array([-1, 5]))
    for got, (a, b) in zip(out, ((4, 0), (0, 5))):
        want = ro.kabsch(p1[a], p2[b])
        assert all(np.array_equal(x, y) for x, y in zip(got, want))
    assert np.array_equal(ro.kabsch_codes(z1, t1, z2, t2)[3][0], ro.kabsch(p1[3], p2[3])[0])
    M, gap = ro.residual_matrix(p1[:2], p2[:3])
    assert M.shape == (2, 3) and M[1, 2] == ro.kabsch(p1[1], p2[2])[3] and gap >= lad.GAP_MIN


def test_the_nearest_neighbour_search_is_exact_and_takes_the_first_of_equals():
    rng = np.random.default_rng(5)
    Q, Y = rng.standard_normal((300, 3)), rng.standard_normal((77, 3))
    Y[40] = Y[11]                                    # two equal targets: the first wins
    Q[7] = Y[11] + 1e-9
    nn, d1, d2 = ro.nearest2(Q, Y, chunk=64)
    d = ((Q[:, None, :] - Y[None, :, :]) ** 2).sum(2)
    assert np.array_equal(nn, d.argmin(1)) and nn[7] == 11
    srt = np.sort(d, axis=1)
    assert np.array_equal(d1, srt[:, 0]) and np.array_equal(d2, srt[:, 1]) and d2[7] == d1[7]


def test_the_icp_oracle_agrees_with_the_restated_reference():
    """oracle/more.py::iterative_closest_point (float32 torch, the canonical distance) on a certified input ends on the same assignment after
    the same number of iterations: its pose is a float32 evaluation like any other and is held to the rule"""
    import torch
    from oracle import more
    case = next(c for c in lad.icp_ladder() if (c[2], c[3]) == (200, 200))
    X, Y, R0, T0 = (torch.from_numpy(a)[None] for a in lad.icp_inputs(case))
    R, T, rmse, it, converged = more.iterative_closest_point(X, Y, R0, T0)
    r = lad.icp_reference(case)
    assert converged and it == r["ref"].iterations
    bad = []
    lad.judge(case[0], lad.icp_errs((R[0].numpy(), T[0].numpy(), float(rmse[0])), (r["ref"].R, r["ref"].T, r["ref"].rmse), r["s"]), r["e32"], bad)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ the certificate
def test_the_certificate_says_no_where_the_trajectory_is_not_pinned():
    case = next(c for c in lad.icp_ladder() if (c[2], c[3]) == (255, 256))
    r = lad.icp_reference(case)
    tr, c = r["ref"].trace, r["ref"].c
    assert ro.icp_certificate(tr, c, r["e32_pose"])
    assert not ro.icp_certificate(tr, c, 1e-3)                       # a pose error this large moves points across bisectors
    assert not ro.icp_certificate(tr[:-1], c, r["e32_pose"])          # the last iteration does not repeat the one before: rel is not exactly 0
    slow = [dict(t) for t in tr]
    slow[1]["rel"] = 5e-5                                             # a stop test within a hundred thresholds of firing
    assert not ro.icp_certificate(slow, c, r["e32_pose"])
    flat = [dict(t) for t in tr]
    flat[0]["gap"] = 0.005
    assert not ro.icp_certificate(flat, c, r["e32_pose"])
    near = [dict(t) for t in tr]
    near[2] = dict(near[2], d2=near[2]["d1"] * (1 + 1e-7))           # a second neighbour as good as the first, to rounding
    assert not ro.icp_certificate(near, c, r["e32_pose"])
    X, Y, R0, T0 = lad.icp_inputs(case)
    assert not ro.icp_certificate(ro.icp(X, Y, R0, T0, max_iter=1).trace, c, r["e32_pose"])


# ------------------------------------------------------------------------------------------------ planted wrong answers
def _caught(key, errs, e32):
    bad = []
    lad.judge(key, errs, e32, bad)
    return bad


@pytest.mark.parametrize("n", [65, 257, 1000])
def test_the_rule_catches_a_planted_kabsch_error(n):
    """a float32 evaluation that forgets the last point (the off-by-one of a guard), and the transposed rotation with its consistent t and
    residuals: each breaks the rule in every kind of cloud, while the honest float32 evaluation passes it"""
    for kind in lad.KB_KINDS:
        case = next(c for c in lad.kabsch_ladder() if c[1:] == (n, 5, kind, "random"))
        x1, x2, w, raw = lad.kabsch_inputs(case)
        r = lad.kabsch_reference(case)[4]
        a, b, wp = x1[4], x2[4], w[4]
        assert not _caught("honest", lad.kabsch_errs(ro.kabsch(a, b, wp, raw, dtype=F32), r["ref"], r["s"]), r["e32"])
        R, t = ro.kabsch(a[:-1], b[:-1], wp[:-1], raw, dtype=F32)[:2]
        res = np.linalg.norm(a @ R.T + t - b, axis=1)
        assert _caught("last point dropped", lad.kabsch_errs((R, t, res), r["ref"], r["s"]), r["e32"]), (n, kind)
        R = r["ref"][0].T
        t = b.mean(0) - R @ a.mean(0)
        assert _caught("transposed", lad.kabsch_errs((R, t, np.linalg.norm(a @ R.T + t - b, axis=1)), r["ref"], r["s"]), r["e32"]), (n, kind)


def test_the_rule_catches_a_planted_residual_matrix_error():
    """the mean over n - 1 residuals divided by n, in the last entry of the last problem of the batch"""
    case = next(c for c in lad.resmat_ladder() if c[3] and c[2] == 257)
    src, tgt = lad.resmat_inputs(case)[-1]
    r = lad.resmat_reference(case)[-1]
    out = r["ref"].copy()
    assert not _caught("exact", lad.resmat_err(out, r), r["e32"])
    out[-1, -1] = ro.kabsch(src[-1], tgt[-1])[2][:-1].sum() / 257
    assert _caught("short mean", lad.resmat_err(out, r), r["e32"])


@pytest.mark.parametrize("nm", [(4096, 600), (700, 10240), (255, 256)])
def test_the_rule_catches_one_moved_match(nm):
    """the float64 alignment onto the oracle's final assignment with ONE point matched to its second neighbour -- at n = 4096 the smallest
    change of a pose a wrong match can make in the ladder -- breaks the rule in R or T; with the right assignment it passes"""
    case = next(c for c in lad.icp_ladder() if (c[2], c[3]) == nm)
    X, Y, _, _ = (a.astype(F64) for a in lad.icp_inputs(case))
    r = lad.icp_reference(case)

    def pose(nn):
        mx, my = X.mean(0), Y[nn].mean(0)
        R, _ = ro._rotation((X - mx).T @ (Y[nn] - my) / len(X), True)
        T = my - mx @ R
        return R, T, float(np.sqrt((((X @ R + T) - Y[nn]) ** 2).sum(1).mean()))
    nn = r["ref"].assignment.copy()
    ref = (r["ref"].R, r["ref"].T, r["ref"].rmse)
    assert not _caught("right", lad.icp_errs(pose(nn), ref, r["s"]), r["e32"])
    q = (X @ r["ref"].R + r["ref"].T)[-1]
    d = ((q - Y) ** 2).sum(1)
    d[nn[-1]] = np.inf
    nn[-1] = int(d.argmin())
    assert _caught("moved", lad.icp_errs(pose(nn), ref, r["s"]), r["e32"])
