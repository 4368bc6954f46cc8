"""CPU-only tests (-m "not gpu") of the scene memory's radius search: the NumPy definition (tests/nearest_oracle.py) against a literal O(a b)
reading of the neighbour rule, the hand-written cases of the definition, the `accepted` bookkeeping of solve_sequence, and what the C entry
points decide on the host before any HIP call (the exported symbols, the workspace sizes, the argument errors that name the problem)."""
import ctypes
import math
import os

import numpy as np
import pytest

import nearest_oracle as no

REPO = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
NAMES = ("ls_cloud_nearest_workspace_bytes", "ls_cloud_nearest_f32", "ls_cloud_nearest_batch_workspace_bytes", "ls_cloud_nearest_batch_f32")
F = np.float32


def _same(got, want):
    assert got[0].dtype == np.int32 and np.array_equal(got[0], want[0])
    assert got[1].dtype == np.float32 and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    assert got[2].dtype == np.int64 and np.array_equal(got[2], want[2])
    assert got[3] == want[3]


def _rot(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    return q * np.sign(np.linalg.det(q))


def _pose(rng):
    return np.concatenate([_rot(rng), rng.uniform(-1, 1, (3, 1))], 1).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the twin against the literal rule
@pytest.mark.parametrize("seed", range(12))
def test_vectorised_oracle_equals_brute_force(seed):
    rng = np.random.default_rng(seed)
    a, b = int(rng.integers(0, 60)), int(rng.integers(0, 60))
    r = F((0.25, 0.1, 0.37)[seed % 3])
    A = rng.uniform(-1, 1, (a, 3)).astype(np.float32)
    B = rng.uniform(-1, 1, (b, 3)).astype(np.float32)
    if a >= 8:
        A[1] = A[0]                                          # duplicates
        A[2] = [-0.0, 0.0, -0.0]                             # the origin with signed zeros: cell (0, 0, 0)
        A[3] = [0.0, -0.0, 0.0]
        A[4] = F([2, -3, 1]) * r                             # exactly on cell faces, either sign
        A[5] = F([-2, 3, -1]) * r
        A[6] = [np.nan, 0.0, 0.0]
        A[7] = [0.1, -np.inf, 0.2]
    if b >= 8:
        B[0] = [np.inf, 0.0, 0.0]
        B[1] = B[2]
        B[3] = [0.5, np.nan, 0.5]
        B[6] = F([1, -3, 1]) * r                             # on faces, one cell from A[4]
        B[7] = [0.0, 0.0, -0.0]
    g = None if seed % 2 else _pose(rng)
    if g is None and a >= 2 and b >= 6:
        B[4], B[5] = A[0], A[a - 1]                          # queries that repeat targets
    got = no.nearest(A, B, g, r)
    _same(got, no.nearest_brute(A, B, g, r))
    if g is None and a >= 8 and b >= 8:
        assert got[0][4] == 0 and got[1][4] == 0.0           # the duplicate target with the lower index
        assert got[0][0] == got[0][3] == -1 and np.isinf(got[1][0])
        assert got[0][7] == 2 and got[2][0] == b - 2


def test_radius_reached_across_two_cells_is_no_neighbour():
    # d2 == r2 == 0.0625, but the cells are -1 and 1: the cell condition is part of the definition
    A, B, r = F([[-1e-30, 0, 0]]), F([[0.25, 0, 0]]), F(0.25)
    for f in (no.nearest, no.nearest_brute):
        idx, d2, counts, s = f(A, B, None, r)
        assert idx.tolist() == [-1] and np.isinf(d2[0]) and counts.tolist() == [1, 0, 0] and s == 0.0
    assert no._d2(B[0], A[0]) == r * r == F(0.0625)


def test_radius_is_inclusive_within_adjacent_cells():
    r = F(0.25)
    up = np.nextafter(F(0.25), F(1))
    A = F([[0, 0, 0]])
    B = F([[0.25, 0, 0], [up, 0, 0], [-0.25, 0, 0]])          # cells 1, 1, -1 against cell 0
    for f in (no.nearest, no.nearest_brute):
        idx, d2, counts, s = f(A, B, None, r)
        assert idx.tolist() == [0, -1, 0] and d2[0] == d2[2] == F(0.0625) and np.isinf(d2[1])
        assert counts.tolist() == [3, 2, 1] and s == 0.125


def test_ties_go_to_the_lowest_index():
    A = F([[9, 9, 9], [0.1, 0, 0], [-0.1, 0, 0], [0, 0.1, 0], [0.1, 0, 0]])
    for f in (no.nearest, no.nearest_brute):
        idx, d2, counts, _ = f(A, F([[0, 0, 0]]), None, F(0.25))
        assert idx.tolist() == [1] and d2[0] == F(0.1) * F(0.1) and counts.tolist() == [1, 1, 1]
        idx, _, _, _ = f(A[::-1], F([[0, 0, 0]]), None, F(0.25))
        assert idx.tolist() == [0]


def test_clamped_cells_are_shared():
    A = F([[1e12, 1e12, 1e12]])
    B = F([[1e12, 1e12, 1e12], [-1e12, 0, 0]])
    for f in (no.nearest, no.nearest_brute):
        idx, d2, counts, _ = f(A, B, None, F(0.5))
        assert idx.tolist() == [0, -1] and d2[0] == 0.0 and counts.tolist() == [2, 1, 1]


def test_pose_and_sum():
    rng = np.random.default_rng(5)
    A = rng.uniform(-1, 1, (300, 3)).astype(np.float32)
    g = _pose(rng)
    gi = np.concatenate([g[:, :3].T, -g[:, :3].T @ g[:, 3:]], 1).astype(np.float32)
    B = no.transform(A, gi)                                  # g takes B back onto A up to rounding
    idx, d2, counts, s = no.nearest(A, B, g, F(0.01))
    assert np.array_equal(idx, np.arange(300)) and counts.tolist() == [300, 300, 300] and d2.max() < 1e-10
    assert s == math.fsum(float(v) for v in d2)
    idx, d2, counts, s = no.nearest(A, A, None, F(1e-4))     # no pose: the bits of B, so every distance is +0.0
    assert np.array_equal(idx, np.arange(300)) and not d2.view(np.uint32).any() and s == 0.0


# ------------------------------------------------------------------------------------------------ the bookkeeping of solve_sequence
def test_sequence_plan_accepted_hand_written():
    from livingscenes_amd.lib_more.more_solver import sequence_plan
    m0 = [3, -1, 0, -1, 1]
    base = sequence_plan(5, m0, 5)
    assert set(base) == {"pairs", "updated", "reencode", "unmatched_new"}                    # accepted=None: exactly today's dict
    assert sequence_plan(5, m0, 5, accepted=None) == base
    assert sequence_plan(5, m0, 5, [7, 0, 1], accepted=None) == sequence_plan(5, m0, 5, [7, 0, 1])
    p = sequence_plan(5, m0, 5, accepted=[True, False, True])
    assert p["pairs"] == base["pairs"] == [(0, 3), (2, 0), (4, 1)] and p["unmatched_new"] == base["unmatched_new"] == [2, 4]
    assert p["updated"] == [0, 4] and p["reencode"] == [0, 4] and p["rejected"] == [2]
    p = sequence_plan(5, m0, 5, n_new_points=[0, 9], accepted=[True, False, True])           # one count per ACCEPTED pair
    assert p["updated"] == [0, 4] and p["reencode"] == [4] and p["rejected"] == [2]
    p = sequence_plan(5, m0, 5, accepted=[True, True, True])
    assert p["updated"] == [0, 2, 4] and p["rejected"] == []
    p = sequence_plan(5, m0, 5, n_new_points=[], accepted=[False, False, False])
    assert p["updated"] == [] and p["reencode"] == [] and p["rejected"] == [0, 2, 4]
    p = sequence_plan(3, [-1, -1, -1], 2, accepted=[])
    assert p["pairs"] == [] and p["rejected"] == []
    for bad in (lambda: sequence_plan(5, m0, 5, accepted=[True, False]),
                lambda: sequence_plan(5, m0, 5, n_new_points=[1, 2, 3], accepted=[True, False, True])):
        with pytest.raises(ValueError):
            bad()


# ------------------------------------------------------------------------------------------------ the library, host side only
def test_symbols_bindings_and_sources():
    from livingscenes_amd import _lib, ops
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "livingscenes_hip.h")).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and name + "(" in header, name
    build = __import__("livingscenes_amd.build", fromlist=["SOURCES"])
    assert "cloudnear.hip" in build.SOURCES and build.PACKED_FP32_GUARD["cloudnear.hip"] == []
    assert callable(ops.cloud_nearest) and callable(ops.cloud_nearest_batch)
    assert int(lib.ls_version()) == _lib.ABI_VERSION == 107


def test_workspace_sizes():
    from livingscenes_amd import _lib
    lib = _lib.load()
    one, batch = lib.ls_cloud_nearest_workspace_bytes, lib.ls_cloud_nearest_batch_workspace_bytes
    assert one(-1, 0) == 0 and one(0, -1) == 0 and one(2 ** 31 - 1, 1) == 0 and batch(0, 1, 1) == 0 and batch(2, 2 ** 30, 2 ** 30) == 0
    assert batch(-1, 1, 1) == 0 and batch(1, -1, 1) == 0 and batch(1, 1, -1) == 0
    assert one(0, 0) > 0 and one(0, 0) % 256 == 0
    grid = (0, 1, 100, 4096, 4097, 60000)
    for fixed in (0, 1000):
        in_a, in_b = [one(n, fixed) for n in grid], [one(fixed, n) for n in grid]
        assert in_a == sorted(in_a) and in_a[-1] > in_a[0] and in_b == sorted(in_b) and in_b[-1] > in_b[0]
        assert all(v % 256 == 0 for v in in_a + in_b)
    # per target row: cell 12, table 8, count 8, start 8, slot record 32, slot 4, rank 4, member 16, hit flag 1 = 93 bytes, plus 4 bytes of
    # scan block sums per 2048 rows; per chunk of 256 query rows: a float64 and two int32 = 16 bytes; 17 pieces, each padded to 256 bytes
    a, b = 60000, 60000
    rows = 93 * a + 4 * math.ceil(2 * a / 4096) + 16 * (b // 256 + 1)
    assert rows <= one(a, b) <= rows + 17 * 256
    assert one(a, b) <= 96 * a + b // 16 + 17 * 256
    assert one(0, 10 ** 6) <= 10 ** 6 // 16 + 17 * 256                       # the queries cost the partial sums alone
    assert batch(6, 1000, 2000) >= one(1000, 2000) and batch(6, 1000, 2000) % 256 == 0
    assert batch(1, 1000, 2000) >= one(1000, 2000)


def _call_batch(lib, P, a_total, a_off, b_total, b_off, radius):
    """the batch entry with host arrays and made-up buffers: only for calls the host checks refuse before anything is dereferenced"""
    buf = (ctypes.c_float * 16)()
    ao, bo = np.asarray(a_off, np.int64), np.asarray(b_off, np.int64)
    rd = np.asarray(radius, np.float32)
    rc = lib.ls_cloud_nearest_batch_f32(P, buf, a_total, ao.ctypes.data, buf, b_total, bo.ctypes.data, None, rd.ctypes.data, buf, buf, buf, buf, None,
                                        buf, 64, None)
    return rc, lib.ls_last_error().decode()


def test_argument_errors_name_the_problem():
    from livingscenes_amd import _lib
    lib = _lib.load()
    INVALID = -1
    rc, msg = _call_batch(lib, 3, 30, [0, 10, 5, 30], 3, [0, 1, 2, 3], [0.1, 0.1, 0.1])
    assert rc == INVALID and "problem 1" in msg and "a_off" in msg and "decreases" in msg, msg
    rc, msg = _call_batch(lib, 3, 30, [0, 10, 20, 30], 3, [0, 2, 1, 3], [0.1, 0.1, 0.1])
    assert rc == INVALID and "problem 1" in msg and "b_off" in msg and "decreases" in msg, msg
    rc, msg = _call_batch(lib, 3, 30, [0, 10, 20, 29], 3, [0, 1, 2, 3], [0.1, 0.1, 0.1])
    assert rc == INVALID and "problem 2" in msg and "a_off" in msg and "ends at 29" in msg, msg
    rc, msg = _call_batch(lib, 3, 30, [0, 10, 20, 30], 3, [0, 1, 2, 4], [0.1, 0.1, 0.1])
    assert rc == INVALID and "problem 2" in msg and "b_off" in msg and "ends at 4" in msg, msg
    rc, msg = _call_batch(lib, 3, 30, [1, 10, 20, 30], 3, [0, 1, 2, 3], [0.1, 0.1, 0.1])
    assert rc == INVALID and "a_off[0]" in msg, msg
    for bad in (0.0, -0.5, float("nan"), float("inf"), 1e-45, 1e-30, 1e30):    # 1e-45: 1 / r overflows; 1e-30: r r is 0; 1e30: r r overflows
        rc, msg = _call_batch(lib, 3, 30, [0, 10, 20, 30], 3, [0, 1, 2, 3], [0.1, 0.1, bad])
        assert rc == INVALID and "problem 2" in msg and "radius" in msg, (bad, msg)
    rc, msg = _call_batch(lib, 0, 0, [0], 0, [0], [0.1])
    assert rc == INVALID and "P must be" in msg
    rc, msg = _call_batch(lib, 1, 2 ** 31 - 1, [0, 2 ** 31 - 1], 1, [0, 1], [0.1])
    assert rc == INVALID and "exceed" in msg
    rc, msg = _call_batch(lib, 2, 10, [0, 5, 10], 4, [0, 2, 4], [0.1, 0.2])       # all in order: only the workspace (64 bytes) is short
    assert rc == -3 and "workspace" in msg, msg
    buf = (ctypes.c_float * 16)()
    rc = lib.ls_cloud_nearest_f32(buf, 3, buf, 2, None, ctypes.c_float(-1.0), buf, buf, buf, buf, None, buf, 64, None)
    assert rc == INVALID and "radius" in lib.ls_last_error().decode()
    rc = lib.ls_cloud_nearest_f32(buf, 3, buf, 2, None, ctypes.c_float(0.1), buf, buf, buf, buf, None, None, 0, None)
    assert rc == -3 and "workspace" in lib.ls_last_error().decode()
