"""CPU-only tests (-m "not gpu") of the scene-memory merge: the NumPy definition (tests/merge_oracle.py) against a literal O(n^2) reading of
the keep rule, the index bookkeeping of solve_sequence, and what the C entry points decide on the host before any HIP call (the exported
symbols, the workspace sizes, the argument errors that name the problem)."""
import ctypes
import os

import numpy as np
import pytest

import merge_oracle as mo

REPO = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
NAMES = ("ls_cloud_merge_workspace_bytes", "ls_cloud_merge_f32", "ls_cloud_merge_batch_workspace_bytes", "ls_cloud_merge_batch_f32")


def _same(got, want):
    assert got[1].dtype == np.int32 and np.array_equal(got[1], want[1])
    assert got[0].dtype == np.float32 and np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))


def _rot(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    return q * np.sign(np.linalg.det(q))


def _pose(rng):
    return np.concatenate([_rot(rng), rng.uniform(-1, 1, (3, 1))], 1).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the oracle against the literal rule
@pytest.mark.parametrize("seed", range(12))
def test_vectorised_oracle_equals_brute_force(seed):
    rng = np.random.default_rng(seed)
    a, b = int(rng.integers(0, 60)), int(rng.integers(0, 60))
    h = np.float32((0.25, 0.1, 0.37)[seed % 3])
    A = rng.uniform(-1, 1, (a, 3)).astype(np.float32)
    B = rng.uniform(-1, 1, (b, 3)).astype(np.float32)
    if a >= 8:
        A[1] = A[0]                                          # duplicates
        A[2] = [-0.0, 0.0, -0.0]                             # the origin with signed zeros: cell (0, 0, 0)
        A[3] = [0.0, -0.0, 0.0]
        A[4] = np.float32([2, -3, 1]) * h                    # exactly on cell faces, either sign
        A[5] = np.float32([-2, 3, -1]) * h
        A[6] = [np.nan, 0.0, 0.0]
        A[7] = [0.1, -np.inf, 0.2]
    if b >= 4:
        B[0] = [np.inf, 0.0, 0.0]
        B[1] = B[2]
        B[3] = [0.5, np.nan, 0.5]
    g = None if seed % 2 else _pose(rng)
    if g is None and a >= 2 and b >= 6:
        B[4], B[5] = A[0], A[a - 1]                          # new points that repeat kept ones
    _same(mo.merge(A, B, g, h), mo.merge_brute(A, B, g, h))


def test_oracle_properties():
    rng = np.random.default_rng(100)
    A = rng.uniform(-1, 1, (200, 3)).astype(np.float32)
    B = rng.uniform(-1, 1, (150, 3)).astype(np.float32)
    h = 0.2
    pts, src = mo.merge(A, B, None, h)
    assert 0 < pts.shape[0] < 350 and (np.diff(src) > 0).all()
    _same(mo.merge(pts, B[:0], None, h), (pts, np.arange(pts.shape[0], dtype=np.int32)))     # merge(merge(A, B), {}) == merge(A, B)
    again, src2 = mo.merge(pts, B, None, h)                                                  # nothing of B is new the second time
    assert np.array_equal(again.view(np.uint32), pts.view(np.uint32)) and (src2 < pts.shape[0]).all()
    # -0.0 and +0.0 share cell 0; floor sends -tiny to cell -1; the clamp collects everything beyond 2^30 cells
    c, valid = mo.cells(np.float32([[-0.0, 0.0, -1e-30], [3e9, -3e9, 2.0 ** 30], [1e38, np.nan, 0.0]]), np.float32(0.5))
    assert valid.tolist() == [True, True, False]
    assert c[0].tolist() == [0, 0, -1] and c[1].tolist() == [2 ** 30, -2 ** 30, 2 ** 30]
    # the transform is the stated expression, one rounding per operation
    g = _pose(rng)
    x = B[7]
    want = [np.float32(np.float32(np.float32(np.float32(g[r, 0] * x[0]) + np.float32(g[r, 1] * x[1])) + np.float32(g[r, 2] * x[2])) + g[r, 3])
            for r in range(3)]
    assert mo.transform(B, g)[7].tolist() == [float(w) for w in want]


# ------------------------------------------------------------------------------------------------ the bookkeeping of solve_sequence
def test_sequence_plan_hand_written():
    from livingscenes_amd.lib_more.more_solver import sequence_plan
    p = sequence_plan(4, [0, 1, 2, 3], 4)                                   # all matched
    assert p["pairs"] == [(0, 0), (1, 1), (2, 2), (3, 3)] and p["updated"] == [0, 1, 2, 3] and p["unmatched_new"] == []
    assert p["reencode"] == [0, 1, 2, 3]
    p = sequence_plan(3, [-1, -1, -1], 2)                                   # none matched
    assert p["pairs"] == [] and p["updated"] == [] and p["reencode"] == [] and p["unmatched_new"] == [0, 1]
    p = sequence_plan(5, [3, -1, 0, -1, 1], 5)                              # -1 in the middle, a permutation, rescan instances left over
    assert p["pairs"] == [(0, 3), (2, 0), (4, 1)] and p["updated"] == [0, 2, 4] and p["unmatched_new"] == [2, 4]
    p = sequence_plan(5, [3, -1, 0, -1, 1], 5, n_new_points=[7, 0, 1])      # only the slots that grew are encoded again
    assert p["reencode"] == [0, 4] and p["updated"] == [0, 2, 4]
    assert sequence_plan(0, [], 3)["unmatched_new"] == [0, 1, 2] and sequence_plan(2, [1, -1])["unmatched_new"] is None
    import torch
    assert sequence_plan(3, torch.tensor([2, -1, 0]).tolist(), 3)["pairs"] == [(0, 2), (2, 0)]
    for bad in (lambda: sequence_plan(3, [0, 1], 2), lambda: sequence_plan(3, [1, -1, 1], 2), lambda: sequence_plan(2, [0, 2], 2),
                lambda: sequence_plan(2, [0, 1], 2, n_new_points=[1])):
        with pytest.raises(ValueError):
            bad()


# ------------------------------------------------------------------------------------------------ the library, host side only
def test_symbols_bindings_and_sources():
    from livingscenes_amd import _lib, ops
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "livingscenes_hip.h")).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and name + "(" in header, name
    assert "cloudmerge.hip" in __import__("livingscenes_amd.build", fromlist=["SOURCES"]).SOURCES
    assert callable(ops.cloud_merge) and callable(ops.cloud_merge_batch)
    assert int(lib.ls_version()) == _lib.ABI_VERSION == 107


def test_workspace_sizes():
    from livingscenes_amd import _lib
    lib = _lib.load()
    one, batch = lib.ls_cloud_merge_workspace_bytes, lib.ls_cloud_merge_batch_workspace_bytes
    assert one(-1, 0) == 0 and one(0, -1) == 0 and one(2 ** 31 - 1, 1) == 0 and batch(0, 1, 1) == 0 and batch(2, 2 ** 30, 2 ** 30) == 0
    assert one(0, 0) > 0 and one(0, 0) % 256 == 0
    sizes = [one(n, n) for n in (0, 1, 100, 4096, 4097, 60000)]
    assert sizes == sorted(sizes) and sizes[-1] > sizes[0]
    assert one(60000, 60000) == one(120000, 0) == one(0, 120000)            # a function of the candidates alone
    # 32 bytes per candidate (cell 12, table 8, slot 4, keep 4, rank 4) plus the scan's block sums and the fixed pieces
    assert 32 * 120000 <= one(60000, 60000) <= 32 * 120000 + 16 * 256
    assert batch(6, 1000, 2000) >= one(1000, 2000) and batch(6, 1000, 2000) % 256 == 0


def _call_batch(lib, P, a_total, a_off, b_total, b_off, voxel):
    """the batch entry with host arrays and made-up buffers: only for calls the host checks refuse before anything is dereferenced"""
    buf = (ctypes.c_float * 16)()
    ao, bo = np.asarray(a_off, np.int64), np.asarray(b_off, np.int64)
    vx = np.asarray(voxel, np.float32)
    rc = lib.ls_cloud_merge_batch_f32(P, buf, a_total, ao.ctypes.data, buf, b_total, bo.ctypes.data, None, vx.ctypes.data, buf, buf, buf, None, buf, 64,
                                      None)
    return rc, lib.ls_last_error().decode()


def test_argument_errors_name_the_problem():
    from livingscenes_amd import _lib
    lib = _lib.load()
    INVALID = -1
    rc, msg = _call_batch(lib, 3, 30, [0, 10, 5, 30], 3, [0, 1, 2, 3], [0.1, 0.1, 0.1])
    assert rc == INVALID and "problem 1" in msg and "a_off" in msg and "decreases" in msg, msg
    rc, msg = _call_batch(lib, 3, 30, [0, 10, 20, 30], 3, [0, 1, 2, 4], [0.1, 0.1, 0.1])
    assert rc == INVALID and "problem 2" in msg and "b_off" in msg and "ends at 4" in msg, msg
    rc, msg = _call_batch(lib, 3, 30, [1, 10, 20, 30], 3, [0, 1, 2, 3], [0.1, 0.1, 0.1])
    assert rc == INVALID and "a_off[0]" in msg, msg
    for bad in (0.0, -0.5, float("nan"), float("inf"), 1e-45):
        rc, msg = _call_batch(lib, 3, 30, [0, 10, 20, 30], 3, [0, 1, 2, 3], [0.1, 0.1, bad])
        assert rc == INVALID and "problem 2" in msg and "voxel" in msg, (bad, msg)
    rc, msg = _call_batch(lib, 0, 0, [0], 0, [0], [0.1])
    assert rc == INVALID and "P must be" in msg
    rc, msg = _call_batch(lib, 1, 2 ** 31 - 1, [0, 2 ** 31 - 1], 1, [0, 1], [0.1])
    assert rc == INVALID and "exceed" in msg
    rc, msg = _call_batch(lib, 2, 10, [0, 5, 10], 4, [0, 2, 4], [0.1, 0.2])       # all in order: only the workspace (64 bytes) is short
    assert rc == -3 and "workspace" in msg, msg
    buf = (ctypes.c_float * 16)()
    rc = lib.ls_cloud_merge_f32(buf, 3, buf, 2, None, ctypes.c_float(-1.0), buf, buf, buf, None, buf, 64, None)
    assert rc == INVALID and "voxel" in lib.ls_last_error().decode()
