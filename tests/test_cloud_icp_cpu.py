"""CPU-only tests (-m "not gpu") of the scene memory's trimmed ICP: the NumPy definition (tests/icp_oracle.py) against a literal reading of one
iteration, the monotone cost of the oracle's own loop, the twin case of tests/test_hip_cloud_icp.py on the oracle alone, and what the C entry
points decide on the host before any HIP call (the exported symbols, the workspace sizes, the argument errors that name the problem)."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import icp_oracle as io

REPO = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
NAMES = ("ls_cloud_icp_workspace_bytes", "ls_cloud_icp_f32", "ls_cloud_icp_batch_workspace_bytes", "ls_cloud_icp_batch_f32")
F = np.float32


def _rot(axis, deg):
    axis = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    a = np.deg2rad(deg)
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K


def _pose(axis, deg, t):
    return np.concatenate([_rot(axis, deg), np.asarray(t, dtype=np.float64).reshape(3, 1)], 1)


def _inv(g):
    g = np.asarray(g, dtype=np.float64)
    return np.concatenate([g[:, :3].T, -g[:, :3].T @ g[:, 3:]], 1)


def twin_case():
    """the twin case of the issue: A = 2 000 lattice points of pitch 0.02 jittered by < 0.004 (minimum spacing > 0.012); B = 700 rows of A
    under a pose, rounded to fp32, plus 100 rows farther than 3 r from every row of A; g0 = the true pose perturbed so that no point moves
    more than 0.005; r = 0.02 -> (A, B, g0, r, rows: the row of A behind each of the first 700 rows of B)"""
    rng = np.random.default_rng(11)
    ii = np.stack(np.meshgrid(np.arange(20), np.arange(10), np.arange(10), indexing="ij"), -1).reshape(-1, 3)
    A = (ii * 0.02 + rng.uniform(-0.0039, 0.0039, ii.shape)).astype(np.float32)         # |jitter| < 0.004 per axis: spacing > 0.012
    rows = rng.permutation(2000)[:700]
    g_true = _pose([1, 2, 3], 25.0, [0.3, -0.2, 0.1])                                    # takes B into A's frame
    far = (rng.uniform(0, 0.2, (100, 3)) + [0.0, 0.0, 0.5]).astype(np.float32)          # in A's frame: > 0.3 from every row of A
    B = io.no.transform(np.concatenate([A[rows], far]), _inv(g_true).astype(np.float32))
    c = A.astype(np.float64).mean(0)
    dR = _rot([3, -1, 2], 0.5)                                                           # 0.5 deg about the centroid: < 0.0025 at 0.27
    delta = np.concatenate([dR, (c - dR @ c + [0.001, -0.001, 0.001]).reshape(3, 1)], 1)
    g0 = np.concatenate([delta[:, :3] @ g_true[:, :3], delta[:, :3] @ g_true[:, 3:] + delta[:, 3:]], 1).astype(np.float32)
    return A, B, g0, F(0.02), rows


def twin_bound(A, B, g):
    """8 * 2^-24 * (the largest coordinate or translation magnitude): one rounding each from R, from t and from generating B, each through
    three products and a sum, rounded up"""
    return 8 * 2.0 ** -24 * max(np.abs(A).max(), np.abs(B[np.isfinite(B).all(1)]).max(), np.abs(np.asarray(g)[:, 3]).max())


# ------------------------------------------------------------------------------------------------ the oracle against itself
@pytest.mark.parametrize("seed", range(6))
def test_step_equals_literal_reading(seed):
    rng = np.random.default_rng(seed)
    a, b = int(rng.integers(4, 50)), int(rng.integers(4, 50))
    A = rng.uniform(-0.5, 0.5, (a, 3)).astype(np.float32)
    B = (A[rng.integers(0, a, b)] + rng.normal(0, 0.02, (b, 3))).astype(np.float32)
    if seed % 2:
        A[0] = [np.nan, 0, 0]
        B[1] = [0, np.inf, 0]
    g = io.pose0(None if seed % 3 == 0 else _pose([1, 1, 0], 3.0, [0.01, 0.0, -0.01]).astype(np.float32))
    r = F((0.1, 0.25)[seed % 2])
    got, want = io.step(A, B, g, r), io.step_brute(A, B, g, r)
    assert np.array_equal(got["idx"], want["idx"]) and np.array_equal(got["d2"].view(np.uint32), want["d2"].view(np.uint32))
    assert (got["f"], got["n"], got["S"], got["E"]) == (want["f"], want["n"], want["S"], want["E"])
    assert got["n"] >= 3
    assert np.allclose(got["H"], want["H"], rtol=0, atol=1e-15 * got["n"])
    assert np.array_equal(got["g_next"].view(np.uint32), want["g_next"].view(np.uint32)) or np.abs(got["g_next"] - want["g_next"]).max() <= 2.0 ** -23
    R = got["g_next"][:, :3].astype(np.float64)
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-6 and np.linalg.det(R) > 0.999


def test_cost_and_stop_rule_hand_written():
    assert io.cost(0, 0, 0.0, F(0.5)) == 0.0
    assert io.cost(4, 2, 0.125, F(0.5)) == (0.125 + 2 * 0.25) / 4
    assert io.stop_rule(0, 2, 0.1, 0.0, 5, 1e-6, 3) == io.STARVED
    assert io.stop_rule(0, 3, 0.1, 0.0, 0, 1e-6, 3) == io.MAX_ITER            # k = 0 never converges: there is no previous cost
    assert io.stop_rule(0, 3, 0.1, 0.0, 5, 1e-6, 3) is None
    assert io.stop_rule(2, 3, 0.1, 0.1, 5, 0.0, 3) == io.CONVERGED            # no decrease at rel_thr 0
    assert io.stop_rule(2, 3, 0.05, 0.1, 2, 1e-6, 3) == io.MAX_ITER
    assert io.stop_rule(2, 2, 0.05, 0.1, 2, 1e-6, 3) == io.STARVED            # the order of the tests
    assert (io.CONVERGED, io.MAX_ITER, io.STARVED, io.DEGENERATE) == (0, 1, 2, 3)


def test_collinear_matches_are_degenerate():
    A = np.zeros((6, 3), np.float32)
    A[:, 0] = np.arange(6) * 0.01
    B = A + F([0.002, 0, 0])
    out = io.icp(A, B, None, F(0.02), max_iter=5)
    assert out["stop"] == io.DEGENERATE and out["iters"] == 0 and np.array_equal(out["g"], io.IDENTITY)


@pytest.mark.parametrize("seed", range(3))
def test_oracle_cost_never_rises(seed):
    rng = np.random.default_rng(100 + seed)
    A = rng.uniform(-0.5, 0.5, (600, 3)).astype(np.float32)
    A[:, 2] *= 0.2
    sel = A[:, 0] > -0.1                                                        # a partial view of A, noisy, under a pose
    g_true = _pose([0, 1, 1], 10.0 + 5 * seed, [0.2, 0.1, -0.3])
    B = io.no.transform((A[sel] + rng.normal(0, 0.003, (int(sel.sum()), 3))).astype(np.float32), _inv(g_true).astype(np.float32))
    d = _pose([1, 0, 0], 2.0, [0.01, -0.01, 0.005])
    g0 = np.concatenate([d[:, :3] @ g_true[:, :3], d[:, :3] @ g_true[:, 3:] + d[:, 3:]], 1).astype(np.float32)
    out = io.icp(A, B, g0, F(0.05), max_iter=30, rel_thr=1e-6)
    E = out["E"]
    assert out["iters"] >= 2 and out["stop"] in (io.CONVERGED, io.MAX_ITER)
    # neither step can raise the truncated cost in exact arithmetic; the fp32 pose and fp32 d2 add relative rounding of a few 2^-24 per term
    assert all(E[k + 1] <= E[k] * (1 + 1e-5) for k in range(len(E) - 1)), E
    assert E[-1] < E[0]
    if out["stop"] == io.CONVERGED:
        assert E[-2] - E[-1] <= 1e-6 * E[-2] and all(E[k - 1] - E[k] > 1e-6 * E[k - 1] for k in range(1, len(E) - 1))


def test_twin_case_on_the_oracle():
    A, B, g0, r, rows = twin_case()
    d = np.linalg.norm(A[:, None, :].astype(np.float64) - A[None].astype(np.float64), axis=-1)
    assert (d + np.eye(2000)).min() > 0.012
    first = io.step(A, B, g0, r)
    moved = np.linalg.norm(io.images(B[:700], g0).astype(np.float64) - A[rows], axis=1).max()
    assert moved <= 0.005, moved
    assert np.array_equal(first["idx"][:700], rows) and (first["idx"][700:] == -1).all()      # every first correspondence is the true twin
    far = io.images(B[700:], g0).astype(np.float64)
    assert np.linalg.norm(far[:, None] - A[None].astype(np.float64), axis=-1).min() > 3 * float(r)
    out = io.icp(A, B, g0, r, max_iter=100, rel_thr=1e-6)
    assert out["stop"] == io.CONVERGED and out["iters"] >= 1
    err = np.abs(io.images(B[:700], out["g"]).astype(np.float64) - A[rows]).max()
    one = np.abs(io.images(B[:700], first["g_next"]).astype(np.float64) - A[rows]).max()
    assert one <= twin_bound(A, B, first["g_next"]), (one, twin_bound(A, B, first["g_next"]))
    assert err <= twin_bound(A, B, out["g"]), (err, twin_bound(A, B, out["g"]))
    assert (out["idx"][700:] == -1).all() and out["counts"].tolist() == [800, 700, 700]


# ------------------------------------------------------------------------------------------------ solve_sequence, host side
def test_sequence_plan_is_unchanged_and_refine_radius_defaults_to_none():
    from livingscenes_amd.lib_more.more_solver import More_Solver, sequence_plan, solve_sequence
    m0 = [3, -1, 0, -1, 1]
    assert sequence_plan(5, m0, 5) == {"pairs": [(0, 3), (2, 0), (4, 1)], "updated": [0, 2, 4], "reencode": [0, 2, 4], "unmatched_new": [2, 4]}
    assert list(inspect.signature(sequence_plan).parameters) == ["n_mem", "matches0", "n_new", "n_new_points", "accepted"]
    sig = inspect.signature(solve_sequence).parameters
    assert sig["refine_radius"].default is None and sig["overlap_radius"].default is None and sig["min_overlap"].default is None
    for f in (More_Solver._accumulate_batch, More_Solver._overlap_batch):
        assert inspect.signature(f).parameters["g"].default is None
    assert inspect.signature(More_Solver._refine_on_memory_batch).parameters["radius"].default is inspect.Parameter.empty


# ------------------------------------------------------------------------------------------------ the library, host side only
def test_symbols_and_bindings():
    from livingscenes_amd import _lib, ops
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "livingscenes_hip.h")).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and name + "(" in header, name
    for k, name in enumerate(("LS_ICP_CONVERGED", "LS_ICP_MAX_ITER", "LS_ICP_STARVED", "LS_ICP_DEGENERATE")):
        assert f"#define {name} {k} " in header and ops.ICP_STOP[k] == name[7:].lower()
    assert "EXTENSION BEYOND THE\n * RELEASED REFERENCE" in header or "EXTENSION BEYOND THE RELEASED REFERENCE" in header
    assert callable(ops.cloud_icp) and callable(ops.cloud_icp_batch)
    sig = inspect.signature(ops.cloud_icp).parameters
    assert (sig["max_iter"].default, sig["rel_thr"].default, sig["min_matched"].default, sig["trace"].default) == (100, 1e-6, 3, False)
    assert sig["radius"].default is inspect.Parameter.empty
    assert int(lib.ls_version()) == _lib.ABI_VERSION == 107


def test_workspace_sizes():
    from livingscenes_amd import _lib
    lib = _lib.load()
    one, batch = lib.ls_cloud_icp_workspace_bytes, lib.ls_cloud_icp_batch_workspace_bytes
    near, near_batch = lib.ls_cloud_nearest_workspace_bytes, lib.ls_cloud_nearest_batch_workspace_bytes
    assert one(-1, 0) == 0 and one(0, -1) == 0 and one(2 ** 31 - 1, 1) == 0 and batch(0, 1, 1) == 0 and batch(2, 2 ** 30, 2 ** 30) == 0
    assert batch(-1, 1, 1) == 0 and batch(1, -1, 1) == 0 and batch(1, 1, -1) == 0
    assert one(0, 0) > 0 and one(0, 0) % 256 == 0
    grid = (0, 1, 100, 4096, 4097, 60000)
    for fixed in (0, 1000):
        in_a, in_b = [one(n, fixed) for n in grid], [one(fixed, n) for n in grid]
        assert in_a == sorted(in_a) and in_a[-1] > in_a[0] and in_b == sorted(in_b) and in_b[-1] > in_b[0]
        assert all(v % 256 == 0 for v in in_a + in_b)
    # the search's bytes, then the pose (48) and the previous cost (8) per problem and one record of 15 float64 per chunk of 256 queries;
    # three more pieces, each padded to 256 bytes
    for a, b in ((0, 0), (1000, 2000), (60000, 60000)):
        extra = 56 + 120 * (b // 256 + 1)
        assert near(a, b) + extra <= one(a, b) <= near(a, b) + extra + 3 * 256, (a, b)
    for P in (1, 6):
        extra = 56 * P + 120 * (2000 // 256 + P)
        assert near_batch(P, 1000, 2000) + extra <= batch(P, 1000, 2000) <= near_batch(P, 1000, 2000) + extra + 3 * 256
        assert batch(P, 1000, 2000) >= one(1000, 2000) and batch(P, 1000, 2000) % 256 == 0


def _call_batch(lib, P, a_total, a_off, b_total, b_off, radius, max_iter=5, rel_thr=1e-6, min_matched=3, ws_bytes=64):
    """the batch entry with host arrays and made-up buffers: only for calls the host checks refuse before anything is dereferenced"""
    buf = (ctypes.c_float * 16)()
    ao, bo = np.asarray(a_off, np.int64), np.asarray(b_off, np.int64)
    rd = np.asarray(radius, np.float32)
    rc = lib.ls_cloud_icp_batch_f32(P, buf, a_total, ao.ctypes.data, buf, b_total, bo.ctypes.data, None, rd.ctypes.data, max_iter, rel_thr,
                                    min_matched, buf, buf, buf, buf, buf, buf, buf, None, None, None, buf, ws_bytes, None)
    return rc, lib.ls_last_error().decode()


def test_argument_errors_name_the_problem():
    from livingscenes_amd import _lib
    lib = _lib.load()
    INVALID = -1
    rc, msg = _call_batch(lib, 3, 30, [0, 10, 5, 30], 3, [0, 1, 2, 3], [0.1, 0.1, 0.1])
    assert rc == INVALID and "cloud_icp_batch" in msg and "problem 1" in msg and "a_off" in msg and "decreases" in msg, msg
    rc, msg = _call_batch(lib, 3, 30, [0, 10, 20, 30], 3, [0, 2, 1, 3], [0.1, 0.1, 0.1])
    assert rc == INVALID and "problem 1" in msg and "b_off" in msg and "decreases" in msg, msg
    rc, msg = _call_batch(lib, 3, 30, [0, 10, 20, 29], 3, [0, 1, 2, 3], [0.1, 0.1, 0.1])
    assert rc == INVALID and "problem 2" in msg and "a_off" in msg and "ends at 29" in msg, msg
    rc, msg = _call_batch(lib, 3, 30, [1, 10, 20, 30], 3, [0, 1, 2, 3], [0.1, 0.1, 0.1])
    assert rc == INVALID and "a_off[0]" in msg, msg
    for bad in (0.0, -0.5, float("nan"), float("inf"), 1e-45, 1e-30, 1e30):
        rc, msg = _call_batch(lib, 3, 30, [0, 10, 20, 30], 3, [0, 1, 2, 3], [0.1, 0.1, bad])
        assert rc == INVALID and "problem 2" in msg and "radius" in msg, (bad, msg)
    rc, msg = _call_batch(lib, 0, 0, [0], 0, [0], [0.1])
    assert rc == INVALID and "P must be" in msg
    good = (2, 10, [0, 5, 10], 4, [0, 2, 4], [0.1, 0.2])
    rc, msg = _call_batch(lib, *good, max_iter=-1)
    assert rc == INVALID and "max_iter" in msg, msg
    for bad in (2, 0, -1):
        rc, msg = _call_batch(lib, *good, min_matched=bad)
        assert rc == INVALID and "min_matched" in msg, msg
    for bad in (-1e-9, float("nan"), float("inf")):
        rc, msg = _call_batch(lib, *good, rel_thr=bad)
        assert rc == INVALID and "rel_thr" in msg, (bad, msg)
    rc, msg = _call_batch(lib, *good, max_iter=0, rel_thr=0.0)                   # all in order: only the workspace (64 bytes) is short
    assert rc == -3 and "workspace" in msg and "ls_cloud_icp_batch_workspace_bytes" in msg, msg
    rc, msg = _call_batch(lib, *good, ws_bytes=lib.ls_cloud_nearest_batch_workspace_bytes(2, 10, 4))    # the search's size is too short
    assert rc == -3 and "workspace" in msg, msg
    buf = (ctypes.c_float * 16)()
    one = lambda radius, max_iter, rel_thr, min_matched, ws, n: lib.ls_cloud_icp_f32(
        buf, 3, buf, 2, None, ctypes.c_float(radius), max_iter, rel_thr, min_matched, buf, buf, buf, buf, buf, buf, buf, None, None, None, ws, n, None)
    for args, word in (((-1.0, 5, 1e-6, 3), "radius"), ((0.1, -2, 1e-6, 3), "max_iter"), ((0.1, 5, -1.0, 3), "rel_thr"), ((0.1, 5, 1e-6, 2), "min_matched")):
        assert one(*args, buf, 64) == INVALID and word in lib.ls_last_error().decode(), word
    assert one(0.1, 5, 1e-6, 3, None, 0) == -3 and "workspace" in lib.ls_last_error().decode()
