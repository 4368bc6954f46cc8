"""CPU-only tests (-m "not gpu") of the scene memory's normals and point-to-plane ICP: the NumPy definitions (tests/normals_oracle.py,
tests/plane_icp_oracle.py) against their literal readings, the hand-written cases of the definition, the plane twin against the point twin
on a surface, and what the C entry points decide on the host before any HIP call (the exported symbols, the workspace sizes, the argument
errors that name the problem).  The shared generator of tests/test_hip_cloud_plane.py (`sheet`, `surface_case`) lives here."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import icp_oracle as io
import merge_oracle as mo
import normals_oracle as nmo
import plane_icp_oracle as po
from test_cloud_icp_cpu import _inv, _pose, _rot

REPO = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
NAMES = ("ls_cloud_normals_workspace_bytes", "ls_cloud_normals_f32", "ls_cloud_normals_batch_workspace_bytes", "ls_cloud_normals_batch_f32",
         "ls_cloud_icp_plane_workspace_bytes", "ls_cloud_icp_plane_f32", "ls_cloud_icp_plane_batch_workspace_bytes",
         "ls_cloud_icp_plane_batch_f32")
F = np.float32
OFFSET = np.array([3.0, -2.0, 0.5])
SHEET_R = 0.03


def sheet(a, seed=0):
    """the wavy sheet of the issue: z = 0.02 sin(20 x) cos(15 y) + U(+-0.001), (x, y) uniform on a square of side max(0.01 sqrt(a), 0.03),
    offset by (3, -2, 0.5); r = 0.03 -> [a,3] float32"""
    rng = np.random.default_rng(7000 + 10 * a + seed)
    side = max(0.01 * np.sqrt(a), 0.03)
    xy = rng.uniform(0, side, (a, 2))
    z = 0.02 * np.sin(20 * xy[:, 0]) * np.cos(15 * xy[:, 1]) + rng.uniform(-0.001, 0.001, a)
    return (np.concatenate([xy, z[:, None]], 1) + OFFSET).astype(np.float32)


def eigen_gap_ok(tw):
    """the condition on the inputs under which the device's normals are comparable with the twin's: on every row whose neighbourhood is
    not a single point (l2 > 0; with l2 == 0 the integer moments make C exactly zero on both sides), l1 / l2 outside [2^-44, 2^-36], so the
    rank rule decides the same way; on every row the twin finds valid, (l1 - l0) / l2 >= 1e-3, so the eigenvector is well determined"""
    lam = tw["lam"]
    top = lam[:, 2] > 0
    ratio = lam[top, 1] / lam[top, 2]
    v = tw["valid"]
    return bool(not ((ratio >= 2.0 ** -44) & (ratio <= 2.0 ** -36)).any() and ((lam[v, 1] - lam[v, 0]) / lam[v, 2] >= 1e-3).all())


def _box_surface(rng, n, lo, hi):
    """n points on the surface of the box [lo, hi], faces chosen by area"""
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    e = hi - lo
    area = np.array([e[1] * e[2], e[0] * e[2], e[0] * e[1]])
    axis = rng.choice(3, n, p=area / area.sum())
    pts = rng.uniform(lo, hi, (n, 3))
    pts[np.arange(n), axis] = np.where(rng.random(n) < 0.5, lo[axis], hi[axis])
    return pts


def _chair(rng, n):
    """a chair-like union of boxes sampled on its surfaces: a seat, a back and four legs"""
    boxes = [([0, 0, 0.4], [0.5, 0.5, 0.45]), ([0, 0.45, 0.45], [0.5, 0.5, 1.0])]
    boxes += [([x, y, 0], [x + 0.05, y + 0.05, 0.4]) for x in (0, 0.45) for y in (0, 0.45)]
    area = np.array([2 * (e[0] * e[1] + e[1] * e[2] + e[0] * e[2]) for e in (np.subtract(hi, lo) for lo, hi in boxes)])
    return np.concatenate([_box_surface(rng, int(n * w), lo, hi) for w, (lo, hi) in zip(area / area.sum(), boxes)])


def surface_case(n_mem=60000, n_obs=1500, seed=5):
    """the prototype's kind of case: the memory = a chair-like union of boxes offset by (3, -2, 0.5), merged at voxel 0.01; the observation
    = its half x > centre resampled with sigma = 0.002 noise, under a pose; g0 off by 2 degrees and about 0.015; r = 0.03
    -> (A, B, g0, r, g_true)"""
    rng = np.random.default_rng(seed)
    full = (_chair(rng, n_mem) + OFFSET).astype(np.float32)
    A, _ = mo.merge(full, full[:0], None, 0.01)
    other = _chair(rng, 4 * n_obs) + OFFSET
    half = other[other[:, 0] > OFFSET[0] + 0.25][:n_obs]
    pts = half + rng.normal(0, 0.002, half.shape)
    g_true = _pose([2, -1, 1], 70.0, [0.8, -0.3, 0.5])                   # takes B into the memory's frame
    gi = _inv(g_true)
    B = (pts @ gi[:, :3].T + gi[:, 3]).astype(np.float32)
    c = half.mean(0)
    dR = _rot([1, 1, -1], 2.0)
    shift = 0.015 * np.array([2.0, -1.0, 2.0]) / 3.0
    delta = np.concatenate([dR, (c - dR @ c + shift).reshape(3, 1)], 1)  # 2 degrees about the view's centroid, then 0.015
    g0 = np.concatenate([delta[:, :3] @ g_true[:, :3], delta[:, :3] @ g_true[:, 3:] + delta[:, 3:]], 1).astype(np.float32)
    return A, B, g0, F(SHEET_R), g_true


# ------------------------------------------------------------------------------------------------ the normals twin against itself
def _same_moments(x, y):
    return all(np.array_equal(x[k], y[k]) for k in ("nbr_cnt", "s1", "s2", "counts", "valid")) and \
        np.array_equal(x["normals"].view(np.uint32), y["normals"].view(np.uint32)) and \
        np.array_equal(x["variation"].view(np.uint32), y["variation"].view(np.uint32))


@pytest.mark.parametrize("seed", range(6))
def test_normals_equal_the_literal_reading(seed):
    rng = np.random.default_rng(seed)
    a = int(rng.integers(20, 90))
    A = rng.uniform(-0.3, 0.3, (a, 3)).astype(np.float32)
    A[:, 2] *= 0.1
    if seed % 2:
        A[0], A[5] = [np.nan, 0, 0], [0, np.inf, 0]
    r = F((0.1, 0.25)[seed % 2])
    got, want = nmo.normals(A, r, 3), nmo.normals_brute(A, r, 3)
    assert _same_moments(got, want)
    assert got["counts"][0] == a - 2 * (seed % 2) and got["counts"][1] >= 1
    if seed % 2:
        assert got["nbr_cnt"][0] == 0 and got["nbr_cnt"][5] == 0 and not got["normals"][[0, 5]].any()
    v = got["valid"]
    assert np.allclose(np.linalg.norm(got["normals"][v].astype(np.float64), axis=1), 1.0, atol=2.0 ** -23)
    assert not got["normals"][~v].any() and not got["variation"][~v].any()


def test_normals_radius_boundary_and_cell_rule():
    # d2 == r2 exactly is a neighbour: r = 0.25, rows 0.25 apart in adjacent cells
    A = F([[0.0, 0, 0], [0.25, 0, 0], [0.0, 0.25, 0], [0.25, 0.25, 0.0], [0.125, 0.125, 0]])
    for f in (nmo.normals, nmo.normals_brute):
        out = f(A, F(0.25), 3)
        assert out["nbr_cnt"].tolist() == [4, 4, 4, 4, 5]                # the diagonal is farther than r
        assert out["s1"][0].tolist() == [-32768 - 16384, -32768 - 16384, 0]
    # the cell-rule edge case of nearest_oracle: d2 == r2 but the cells are -1 and 1
    A = F([[-1e-30, 0, 0], [0.25, 0, 0]])
    for f in (nmo.normals, nmo.normals_brute):
        assert f(A, F(0.25), 1)["nbr_cnt"].tolist() == [1, 1]


def hand_cases():
    """(name, A, r, min_nbrs, expected valid mask or None, expected normal of row 0 or None)"""
    plane = F([[0, 0, 0], [0.01, 0, 0], [-0.01, 0, 0], [0, 0.01, 0], [0, -0.01, 0]]) + F([3, -2, 0.5])
    line = (np.arange(7)[:, None] * F([0.004, 0.004, 0.004])).astype(F)
    same = np.tile(F([[1.5, 2.5, -0.5]]), (6, 1))
    tilted = F([[0, 0, 0], [0.01, 0, 0.01], [-0.01, 0, -0.01], [0, 0.01, 0], [0, -0.01, 0]])       # the plane x - z = 0
    return [("coplanar", plane, 0.03, 5, [True] * 5, [0, 0, 1]), ("collinear", line, 0.03, 3, [False] * 7, None),
            ("coincident", same, 0.03, 3, [False] * 6, None), ("one short", plane, 0.03, 6, [False] * 5, None),
            ("sign: the first of two equal magnitudes", tilted, 0.03, 5, [True] * 5, None)]


def test_normals_hand_written():
    for name, A, r, k, valid, n0 in hand_cases():
        for f in (nmo.normals, nmo.normals_brute):
            out = f(A, F(r), k)
            assert out["valid"].tolist() == valid, name
            if n0 is not None:
                assert np.array_equal(out["normals"], np.tile(F(n0), (len(A), 1))) and not out["variation"].any(), name
    out = nmo.normals(hand_cases()[4][1], F(0.03), 5)
    n = out["normals"][0]
    assert abs(abs(n[0]) - abs(n[2])) <= 2.0 ** -23 and abs(n[1]) < 1e-6 and n[0] * n[2] < 0, n
    assert (n[0] > 0) if abs(n[0]) >= abs(n[2]) else (n[2] > 0), n
    # the sign rule where the largest component is unambiguous: normals of planes facing down come out facing the positive side
    rng = np.random.default_rng(3)
    for axis in ([0.2, -0.3, -0.9], [-0.8, 0.1, 0.2], [0.1, -0.9, 0.3]):
        nrm = np.asarray(axis) / np.linalg.norm(axis)
        u = np.cross(nrm, [1, 0, 0])
        u /= np.linalg.norm(u)
        v = np.cross(nrm, u)
        st = rng.uniform(-0.02, 0.02, (40, 2))
        A = (st[:, :1] * u + st[:, 1:] * v).astype(F)
        got = nmo.normals(A, F(0.03), 5)
        big = int(np.argmax(np.abs(nrm)))
        assert got["valid"].all() and (got["normals"][:, big] > 0).all()
        assert np.abs(got["normals"] - np.sign(nrm[big]) * nrm).max() < 1e-3


@pytest.mark.parametrize("a", (255, 256, 257, 2049))
def test_sheet_meets_the_eigen_gap_condition(a):
    for seed in range(3):
        tw = nmo.normals(sheet(a, seed), F(SHEET_R), 5)
        # a corner row can have fewer than min_nbrs neighbours (a quarter of the 28 a ball holds, less the draw): invalid by the count
        # alone, never by the rank rule, and the condition holds on it too
        assert np.array_equal(tw["valid"], tw["nbr_cnt"] >= 5) and tw["valid"].mean() >= 0.99 and tw["counts"][0] == a
        assert 3 <= tw["nbr_cnt"].min() and tw["nbr_cnt"].max() <= 60
        assert eigen_gap_ok(tw)


# ------------------------------------------------------------------------------------------------ the plane twin against itself
@pytest.mark.parametrize("seed", range(6))
def test_plane_step_equals_literal_reading(seed):
    rng = np.random.default_rng(50 + seed)
    a, b = int(rng.integers(30, 60)), int(rng.integers(20, 50))
    A = rng.uniform(-0.5, 0.5, (a, 3)).astype(np.float32)
    N = rng.standard_normal((a, 3))
    N = (N / np.linalg.norm(N, axis=1, keepdims=True)).astype(np.float32)
    N[rng.integers(0, a, 5)] = 0                                         # rows without a normal
    B = (A[rng.integers(0, a, b)] + rng.normal(0, 0.02, (b, 3))).astype(np.float32)
    if seed % 2:
        A[0], B[1] = [np.nan, 0, 0], [0, np.inf, 0]
    g = io.pose0(None if seed % 3 == 0 else _pose([1, 1, 0], 3.0, [0.01, 0.0, -0.01]).astype(np.float32))
    r = F((0.1, 0.25)[seed % 2])
    got, want = po.step(A, N, B, g, r), po.step_brute(A, N, B, g, r)
    assert np.array_equal(got["idx"], want["idx"]) and np.array_equal(got["d2"].view(np.uint32), want["d2"].view(np.uint32))
    for k in ("f", "n", "S", "w", "Q", "E"):
        assert got[k] == want[k], k
    assert 6 <= got["w"] <= got["n"] and np.array_equal(got["M"], want["M"]) and np.array_equal(got["b"], want["b"])
    assert np.array_equal(got["g_next"].view(np.uint32), want["g_next"].view(np.uint32))
    R = got["g_next"][:, :3].astype(np.float64)
    assert np.abs(R @ R.T - np.eye(3)).max() <= 2.0 ** -22 and np.linalg.det(R) > 0.999
    assert got["E"] == io.cost(got["f"], got["w"], got["Q"], r)


def test_plane_query_at_exactly_r_and_cell_rule():
    N = F([[0, 0, 1], [0, 0, 1]])
    for A, B, n in ((F([[0, 0, 0], [5, 5, 5]]), F([[0.25, 0, 0]]), 1), (F([[-1e-30, 0, 0], [5, 5, 5]]), F([[0.25, 0, 0]]), 0)):
        got, want = po.step(A, N, B, io.IDENTITY, F(0.25)), po.step_brute(A, N, B, io.IDENTITY, F(0.25))
        assert got["n"] == want["n"] == n and got["w"] == want["w"] == n and got["Q"] == want["Q"] == 0.0


def test_exp_and_cholesky_hand_written():
    R, t = po.se3_exp(np.array([1.0, 2.0, 3.0, 0.0, 0.0, 0.0]))
    assert np.array_equal(R, np.eye(3)) and t.tolist() == [1.0, 2.0, 3.0]
    R, t = po.se3_exp(np.array([1.0, 0.0, 0.0, 0.0, 0.0, np.pi / 2]))   # a quarter turn about z: the translation follows the arc
    assert np.allclose(R, [[0, -1, 0], [1, 0, 0], [0, 0, 1]], atol=1e-15) and np.allclose(t, [2 / np.pi, 2 / np.pi, 0], atol=1e-15)
    rng = np.random.default_rng(0)
    X = rng.standard_normal((6, 6))
    M, b = X @ X.T + np.eye(6), rng.standard_normal(6)
    xi, ratio = po.cholesky_solve(M, b)
    assert np.allclose(M @ xi, b, atol=1e-12) and 0 < ratio <= 1
    M[5], M[:, 5] = M[4], M[:, 4]
    M[5, 5] = M[4, 4]
    assert po.cholesky_solve(M, b)[0] is None                            # two equal rows: the last pivot is zero
    assert po.cholesky_solve(np.full((6, 6), np.nan), b)[0] is None
    assert po.stop_rule(0, 5, 0.1, 0.0, 5, 1e-6, 6) == po.STARVED and po.stop_rule(0, 6, 0.1, 0.0, 5, 1e-6, 6) is None
    assert po.stop_rule(3, 6, 0.2, 0.1, 5, 1e-6, 6) == po.CONVERGED      # a step that raised E ends the loop


def test_parallel_normals_are_degenerate():
    rng = np.random.default_rng(1)
    A = np.concatenate([rng.uniform(-0.2, 0.2, (200, 2)), np.zeros((200, 1))], 1).astype(F) + F([3, -2, 0.5])
    N = np.tile(F([[0, 0, 1]]), (200, 1))
    B = A[:80] + F([0.001, -0.001, 0.004])
    out = po.icp(A, N, B, None, F(0.03), max_iter=5)
    assert out["stop"] == po.DEGENERATE and out["iters"] == 0 and np.array_equal(out["g"], io.IDENTITY) and out["planar"] == 80


# the iterations observed on surface_case with the defaults (rel_thr 1e-6): recorded after they were seen, the point twin first
SURFACE_ITERS = {"point": 48, "plane": 6}


def test_plane_twin_needs_fewer_iterations_on_a_surface():
    A, B, g0, r, g_true = surface_case()
    tw = nmo.normals(A, r, 5)
    assert tw["valid"].mean() > 0.95
    point = io.icp(A, B, g0, r)
    plane = po.icp(A, tw["normals"], B, g0, r)
    truth = io.images(B, g_true.astype(np.float32)).astype(np.float64)
    dist = lambda g: float(np.linalg.norm(io.images(B, g).astype(np.float64) - truth, axis=1).mean())
    print(f"surface case: a {A.shape[0]} b {B.shape[0]}; point: iters {point['iters']} stop {point['stop']} distance {dist(point['g']):.3e}; "
          f"plane: iters {plane['iters']} stop {plane['stop']} distance {dist(plane['g']):.3e}; start {dist(g0):.3e}")
    assert point["stop"] == io.CONVERGED and plane["stop"] == po.CONVERGED
    for g in plane["g_trace"]:
        R = np.asarray(g)[:, :3].astype(np.float64)
        assert np.abs(R @ R.T - np.eye(3)).max() <= 2.0 ** -22
    assert (point["iters"], plane["iters"]) == (SURFACE_ITERS["point"], SURFACE_ITERS["plane"])
    assert plane["iters"] < point["iters"]
    assert dist(plane["g"]) < 0.1 * dist(g0) and dist(point["g"]) < 0.1 * dist(g0)


# ------------------------------------------------------------------------------------------------ the library, host side only
def test_symbols_and_bindings():
    from livingscenes_amd import _lib, ops
    from livingscenes_amd.lib_more.more_solver import More_Solver, solve_sequence
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "livingscenes_hip.h")).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and name + "(" in header, name
    assert header.count("EXTENSION BEYOND THE RELEASED REFERENCE") + header.count("EXTENSION BEYOND THE\n * RELEASED REFERENCE") + \
        header.count("AN\n * EXTENSION BEYOND THE RELEASED REFERENCE") >= 5
    assert int(lib.ls_version()) == _lib.ABI_VERSION == 107
    sig = inspect.signature(ops.cloud_normals).parameters
    assert sig["min_nbrs"].default == 5 and sig["radius"].default is inspect.Parameter.empty
    assert "not tuned" in ops.cloud_normals.__doc__.lower() and "not tuned" in ops.cloud_normals_batch.__doc__.lower()
    sig = inspect.signature(ops.cloud_icp_plane).parameters
    assert list(sig)[:4] == ["A", "N", "B", "g"]
    assert (sig["max_iter"].default, sig["rel_thr"].default, sig["min_matched"].default, sig["trace"].default) == (100, 1e-6, 6, False)
    assert inspect.signature(ops.cloud_icp_plane_batch).parameters["packed"].default is False
    assert inspect.signature(ops.cloud_normals_batch).parameters["packed"].default is False
    sig = inspect.signature(More_Solver._memory_normals_batch).parameters
    assert sig["radius"].default is None and sig["min_nbrs"].default == 5
    sig = inspect.signature(More_Solver._refine_on_memory_batch).parameters
    assert sig["metric"].default == "point" and sig["normal_radius"].default is None
    sig = inspect.signature(solve_sequence).parameters
    assert sig["refine_metric"].default == "point" and sig["normal_radius"].default is None


def test_solve_sequence_refuses_plane_without_a_radius():
    from livingscenes_amd.lib_more.more_solver import solve_sequence
    with pytest.raises(ValueError, match="refine_radius"):
        solve_sequence(None, None, [], refine_metric="plane")
    with pytest.raises(ValueError, match="refine_metric"):
        solve_sequence(None, None, [], refine_radius=0.04, refine_metric="surface")


def test_workspace_sizes():
    from livingscenes_amd import _lib
    lib = _lib.load()
    nrm, nrm_batch = lib.ls_cloud_normals_workspace_bytes, lib.ls_cloud_normals_batch_workspace_bytes
    one, batch = lib.ls_cloud_icp_plane_workspace_bytes, lib.ls_cloud_icp_plane_batch_workspace_bytes
    point, point_batch = lib.ls_cloud_icp_workspace_bytes, lib.ls_cloud_icp_batch_workspace_bytes
    assert nrm(-1) == 0 and nrm(2 ** 31) == 0 and nrm_batch(0, 1) == 0 and nrm_batch(1, -1) == 0 and nrm_batch(2, 2 ** 31) == 0
    assert one(-1, 0) == 0 and one(0, -1) == 0 and one(2 ** 31 - 1, 1) == 0 and batch(0, 1, 1) == 0 and batch(2, 2 ** 30, 2 ** 30) == 0
    assert nrm(0) > 0 and nrm(0) % 256 == 0 and one(0, 0) > 0 and one(0, 0) % 256 == 0
    grid = (0, 1, 100, 4096, 4097, 60000)
    sizes = [nrm(n) for n in grid]
    assert sizes == sorted(sizes) and sizes[-1] > sizes[0] and all(v % 256 == 0 for v in sizes)
    assert all(nrm(n) == lib.ls_cloud_nearest_workspace_bytes(n, 0) for n in grid)                 # the search's grid and nothing else
    assert all(nrm_batch(3, n) == lib.ls_cloud_nearest_batch_workspace_bytes(3, n, 0) for n in grid)
    for fixed in (0, 1000):
        in_a, in_b = [one(n, fixed) for n in grid], [one(fixed, n) for n in grid]
        assert in_a == sorted(in_a) and in_a[-1] > in_a[0] and in_b == sorted(in_b) and in_b[-1] > in_b[0]
        assert all(v % 256 == 0 for v in in_a + in_b)
    # the point ICP's bytes, then 13 more float64 and one int per chunk of 256 queries: the larger record takes up to 255 bytes of padding
    # the point layout ended with, and the one new piece is padded to 256 bytes
    for a, b in ((0, 0), (1000, 2000), (60000, 60000)):
        extra = (13 * 8 + 4) * (b // 256 + 1)
        assert point(a, b) + extra - 255 <= one(a, b) <= point(a, b) + extra + 2 * 256, (a, b)
    for P in (1, 6):
        extra = (13 * 8 + 4) * (2000 // 256 + P)
        assert point_batch(P, 1000, 2000) + extra - 255 <= batch(P, 1000, 2000) <= point_batch(P, 1000, 2000) + extra + 2 * 256
        assert batch(P, 1000, 2000) >= one(1000, 2000) and batch(P, 1000, 2000) % 256 == 0


def _plane_batch(lib, P, a_total, a_off, b_total, b_off, radius, max_iter=5, rel_thr=1e-6, min_matched=6, ws_bytes=64):
    """the batch entry with host arrays and made-up buffers: only for calls the host checks refuse before anything is dereferenced"""
    buf = (ctypes.c_float * 16)()
    ao, bo = np.asarray(a_off, np.int64), np.asarray(b_off, np.int64)
    rd = np.asarray(radius, np.float32)
    rc = lib.ls_cloud_icp_plane_batch_f32(P, buf, buf, a_total, ao.ctypes.data, buf, b_total, bo.ctypes.data, None, rd.ctypes.data, max_iter,
                                          rel_thr, min_matched, buf, buf, buf, buf, buf, buf, buf, buf, buf, None, None, None, buf, ws_bytes, None)
    return rc, lib.ls_last_error().decode()


def _normals_batch(lib, P, a_total, a_off, radius, min_nbrs=5, ws_bytes=64):
    buf = (ctypes.c_float * 16)()
    ao, rd = np.asarray(a_off, np.int64), np.asarray(radius, np.float32)
    rc = lib.ls_cloud_normals_batch_f32(P, buf, a_total, ao.ctypes.data, rd.ctypes.data, min_nbrs, buf, buf, buf, buf, None, buf, ws_bytes, None)
    return rc, lib.ls_last_error().decode()


def test_argument_errors_name_the_problem():
    from livingscenes_amd import _lib
    lib = _lib.load()
    INVALID = -1
    for call, sizes in ((_plane_batch, (3, [0, 1, 2, 3])), (_normals_batch, ())):
        name = "cloud_icp_plane_batch" if sizes else "cloud_normals_batch"
        rc, msg = call(lib, 3, 30, [0, 10, 5, 30], *sizes, [0.1, 0.1, 0.1])
        assert rc == INVALID and name in msg and "problem 1" in msg and "a_off" in msg and "decreases" in msg, msg
        rc, msg = call(lib, 3, 30, [0, 10, 20, 29], *sizes, [0.1, 0.1, 0.1])
        assert rc == INVALID and "problem 2" in msg and "a_off" in msg and "ends at 29" in msg, msg
        rc, msg = call(lib, 3, 30, [1, 10, 20, 30], *sizes, [0.1, 0.1, 0.1])
        assert rc == INVALID and "a_off[0]" in msg, msg
        for bad in (0.0, -0.5, float("nan"), float("inf"), 1e-45, 1e-30, 1e30):
            rc, msg = call(lib, 3, 30, [0, 10, 20, 30], *sizes, [0.1, 0.1, bad])
            assert rc == INVALID and "problem 2" in msg and "radius" in msg, (bad, msg)
        rc, msg = call(lib, 0, 0, [0], *((0, [0]) if sizes else ()), [0.1])
        assert rc == INVALID and "P must be" in msg
    rc, msg = _plane_batch(lib, 3, 30, [0, 10, 20, 30], 3, [0, 2, 1, 3], [0.1, 0.1, 0.1])
    assert rc == INVALID and "problem 1" in msg and "b_off" in msg and "decreases" in msg, msg
    good = (2, 10, [0, 5, 10], 4, [0, 2, 4], [0.1, 0.2])
    rc, msg = _plane_batch(lib, *good, max_iter=-1)
    assert rc == INVALID and "max_iter" in msg, msg
    for bad in (2, 0, -1):
        rc, msg = _plane_batch(lib, *good, min_matched=bad)
        assert rc == INVALID and "min_matched" in msg, msg
    for bad in (-1e-9, float("nan"), float("inf")):
        rc, msg = _plane_batch(lib, *good, rel_thr=bad)
        assert rc == INVALID and "rel_thr" in msg, (bad, msg)
    rc, msg = _plane_batch(lib, *good, max_iter=0, rel_thr=0.0)              # all in order: only the workspace (64 bytes) is short
    assert rc == -3 and "workspace" in msg and "ls_cloud_icp_plane_batch_workspace_bytes" in msg, msg
    rc, msg = _plane_batch(lib, *good, ws_bytes=lib.ls_cloud_icp_batch_workspace_bytes(2, 10, 4))      # the point ICP's size is too short
    assert rc == -3 and "workspace" in msg, msg
    for bad in (0, -3):
        rc, msg = _normals_batch(lib, 2, 10, [0, 5, 10], [0.1, 0.2], min_nbrs=bad)
        assert rc == INVALID and "min_nbrs" in msg, msg
    rc, msg = _normals_batch(lib, 2, 10, [0, 5, 10], [0.1, 0.2])
    assert rc == -3 and "workspace" in msg and "ls_cloud_normals_batch_workspace_bytes" in msg, msg
    buf = (ctypes.c_float * 16)()
    one = lambda radius, min_nbrs, ws, n: lib.ls_cloud_normals_f32(buf, 3, ctypes.c_float(radius), min_nbrs, buf, buf, buf, buf, None, ws, n, None)
    for args, word in (((-1.0, 5), "radius"), ((float("nan"), 5), "radius"), ((0.1, 0), "min_nbrs")):
        assert one(*args, buf, 64) == INVALID and word in lib.ls_last_error().decode(), word
    assert one(0.1, 5, None, 0) == -3 and "workspace" in lib.ls_last_error().decode()
    plane = lambda radius, max_iter, rel_thr, min_matched, N, ws, n: lib.ls_cloud_icp_plane_f32(
        buf, N, 3, buf, 2, None, ctypes.c_float(radius), max_iter, rel_thr, min_matched, buf, buf, buf, buf, buf, buf, buf, buf, buf, None, None, None,
        ws, n, None)
    for args, word in (((-1.0, 5, 1e-6, 6), "radius"), ((0.1, -2, 1e-6, 6), "max_iter"), ((0.1, 5, -1.0, 6), "rel_thr"), ((0.1, 5, 1e-6, 2), "min_matched")):
        assert plane(*args, buf, buf, 64) == INVALID and word in lib.ls_last_error().decode(), word
    assert plane(0.1, 5, 1e-6, 6, None, buf, 64) == INVALID and "null N" in lib.ls_last_error().decode()
    assert plane(0.1, 5, 1e-6, 6, buf, None, 0) == -3 and "workspace" in lib.ls_last_error().decode()
