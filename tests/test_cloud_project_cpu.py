"""CPU-only tests (-m "not gpu") of the scene memory's projection onto local planes: the NumPy definition (tests/project_oracle.py) against
its literal reading, the hand-written cases of the definition, the quality condition of the consolidation on the twin, and what the C entry
points decide on the host before any HIP call (the exported symbols, the workspace sizes, every refusal).  The shared generators of
tests/test_hip_cloud_project.py (`lattice`, `lifted`, `noisy_sphere_memory`) live here.

The quality condition.  A sphere of radius 0.15 m, sigma = 0.002 noise, voxel 0.01 m, 4 000 points per scan, one reference scan and three
rescans merged at the true pose (merge_oracle), one projection at r = 0.02: the RMS distance of the kept rows to the sphere must fall
below 0.5 x what it was.  The bound is the issue's: its larger experiment (radius 0.4 m, 20 000 points, five rescans) gives 0.24, and 0.5
leaves a factor two for this smaller, sparser cloud.  The figure of this cloud is printed by the test."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import merge_oracle as mo
import project_oracle as pjo
from test_cloud_plane_cpu import hand_cases, sheet

REPO = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
NAMES = ("ls_cloud_project_workspace_bytes", "ls_cloud_project_f32", "ls_cloud_project_batch_workspace_bytes", "ls_cloud_project_batch_f32")
F = np.float32
INF = float("inf")


def lattice(n=9, step=0.01, origin=(3.0, -2.0, 0.0)):
    """an axis-aligned n x n lattice on z = 0: every offset has q_z = 0, so the covariance has an exactly zero row and column"""
    g = np.arange(n) * step
    xy = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    return (np.concatenate([xy, np.zeros((n * n, 1))], 1) + np.asarray(origin)).astype(F)


def lifted(n=9, lift=0.004):
    """the lattice with its centre row lifted off the plane -> (A, the row)"""
    A = lattice(n)
    i = (n // 2) * n + n // 2
    A[i, 2] = F(lift)
    return A, i


def noisy_sphere_memory(radius=0.15, per_scan=4000, rescans=3, sigma=0.002, voxel=0.01, seed=11):
    """the memory of the experiment: scans of a sphere with Gaussian noise, merged at the true pose one after the other -> (A, centre)"""
    rng = np.random.default_rng(seed)
    centre = np.array([3.0, -2.0, 0.5])

    def scan():
        d = rng.standard_normal((per_scan, 3))
        return (centre + radius * d / np.linalg.norm(d, axis=1, keepdims=True) + rng.normal(0, sigma, (per_scan, 3))).astype(F)
    A, _ = mo.merge(scan(), np.zeros((0, 3), F), None, voxel)
    for _ in range(rescans):
        A, _ = mo.merge(A, scan(), None, voxel)
    return A, centre


def _same(x, y):
    return all(np.array_equal(x[k], y[k]) for k in ("state", "counts", "nbr_cnt")) and x["sum_shift2"] == y["sum_shift2"] and \
        np.array_equal(x["points"].view(np.uint32), y["points"].view(np.uint32)) and \
        np.array_equal(x["shift"].view(np.uint32), y["shift"].view(np.uint32))


# ------------------------------------------------------------------------------------------------ the twin against itself
@pytest.mark.parametrize("seed", range(6))
def test_project_equals_the_literal_reading(seed):
    rng = np.random.default_rng(100 + seed)
    a = int(rng.integers(40, 300 if seed == 5 else 120))                 # seed 5: more than one chunk of 256 rows
    A = rng.uniform(-0.3, 0.3, (a, 3)).astype(F)
    A[:, 2] *= 0.1
    if seed % 2:
        A[0], A[5] = [np.nan, 0, 0], [0, np.inf, 0]
    r = F((0.1, 0.25)[seed % 2])
    limits = ((1 / 3, INF), (0.008, INF), (1 / 3, 0.004))[seed % 3]
    got, want = pjo.project(A, r, 3, *limits), pjo.project_brute(A, r, 3, *limits)
    assert _same(got, want)
    st = got["state"]
    assert got["counts"].tolist() == [int((st == k).sum()) for k in range(4)] and got["counts"].sum() == a
    assert got["counts"][0] == 2 * (seed % 2) and got["counts"][3] >= 1
    if seed % 3:
        assert got["counts"][2] >= 1                                     # the limit holds some row
    fixed = st != pjo.MOVED
    assert np.array_equal(got["points"][fixed].view(np.uint32), A[fixed].view(np.uint32))
    assert not got["shift"][st < pjo.HELD].any()
    # a moved row lies on its plane: what is left of its distance is the fp32 rounding of three coordinates
    mv = st == pjo.MOVED
    left = np.abs(((got["points"][mv].astype(np.float64) - A[mv]) * got["n"][mv]).sum(1) + got["s"][mv])
    assert left.max() <= 3 * 2.0 ** -24 * np.abs(A[mv]).max()


def test_project_radius_boundary_and_cell_rule():
    # d2 == r2 exactly is a neighbour: r = 0.25, rows 0.25 apart in adjacent cells
    A = F([[0.0, 0, 0], [0.25, 0, 0], [0.0, 0.25, 0], [0.25, 0.25, 0.0], [0.125, 0.125, 0]])
    for f in (pjo.project, pjo.project_brute):
        out = f(A, F(0.25), 3)
        assert out["nbr_cnt"].tolist() == [4, 4, 4, 4, 5] and out["state"].tolist() == [3] * 5 and not out["shift"].any()
    # the cell-rule edge case of the search: d2 == r2 but the cells are -1 and 1
    A = F([[-1e-30, 0, 0], [0.25, 0, 0]])
    for f in (pjo.project, pjo.project_brute):
        out = f(A, F(0.25), 1)
        assert out["nbr_cnt"].tolist() == [1, 1] and out["state"].tolist() == [1, 1]


def test_chunk_rule_hand_written():
    assert pjo.chunk_rule(np.zeros(0)) == 0.0 and pjo.chunk_rule(np.array([0.5])) == 0.5
    v = np.zeros(257)
    v[0], v[128], v[255], v[256] = 1.0, 2.0 ** -53, 2.0 ** -53, 2.0 ** -53
    # the tree adds row 128 to row 0 first (lost), row 255 to row 127 and that only at the end (lost again); the second chunk is added last
    assert pjo.chunk_rule(v) == 1.0
    # rows 127 and 255 meet before they meet row 0, so 2^-52 survives the first chunk; the second chunk's 2^-53 is then a tie that rounds
    # to the even neighbour above
    v[127] = 2.0 ** -53
    assert pjo.chunk_rule(v) == 1.0 + 2.0 ** -51
    assert pjo.chunk_rule(v[:256]) == 1.0 + 2.0 ** -52


# ------------------------------------------------------------------------------------------------ hand-written cases
def test_lattice_is_a_fixed_point():
    A = lattice()
    for f in (pjo.project, pjo.project_brute):
        out = f(A, F(0.03), 5)
        assert out["state"].tolist() == [3] * len(A) and out["counts"].tolist() == [0, 0, 0, len(A)]
        assert not out["shift"].any() and out["sum_shift2"] == 0.0
        assert np.array_equal(out["points"].view(np.uint32), A.view(np.uint32))


def test_rows_without_a_plane_stay():
    for name, A, r, k, valid, _ in hand_cases():
        if any(valid):
            continue                                                     # collinear, coincident, m = min_nbrs - 1
        for f in (pjo.project, pjo.project_brute):
            out = f(A, F(r), k)
            assert out["state"].tolist() == [1] * len(A), name
            assert not out["shift"].any() and np.array_equal(out["points"].view(np.uint32), A.view(np.uint32)), name
    A = np.concatenate([lattice(), F([[np.nan, 0, 0], [0, -np.inf, 0]])])
    out = pjo.project(A, F(0.03), 5)
    assert out["state"][-2:].tolist() == [0, 0] and out["counts"].tolist() == [2, 0, 0, len(A) - 2]
    assert np.array_equal(out["points"].view(np.uint32), A.view(np.uint32))


def test_lifted_row_and_max_shift():
    A, i = lifted()
    for f in (pjo.project, pjo.project_brute):
        free, held = f(A, F(0.03), 5, 1 / 3, INF), f(A, F(0.03), 5, 1 / 3, 0.0)
        assert free["state"].tolist() == [3] * len(A)
        assert 0.5 * 0.004 < free["shift"][i] < 0.004 and abs(free["points"][i, 2]) < 0.5 * 0.004      # most of the way back to the plane
        assert held["state"][i] == 2 and held["shift"][i] == free["shift"][i] and np.array_equal(held["points"][i], A[i])
        # at max_shift = 0 a row moves iff its distance is exactly 0: the rows that do not see the lifted one
        near = free["shift"] > 0
        assert near[i] and 5 <= near.sum() < len(A)
        assert np.array_equal(held["state"], np.where(near, 2, 3)) and np.array_equal(held["points"].view(np.uint32), A.view(np.uint32))
        assert held["sum_shift2"] == 0.0 and free["sum_shift2"] > float(free["shift"][i]) ** 2


def test_max_variation_zero_holds_what_is_not_exactly_planar():
    A = sheet(257)
    out, free = pjo.project(A, F(0.03), 5, 0.0, INF), pjo.project(A, F(0.03), 5)
    assert out["counts"][3] == 0 and out["counts"][2] == free["counts"][3] > 250 and out["counts"][1] == free["counts"][1]
    assert np.array_equal(out["points"].view(np.uint32), A.view(np.uint32)) and np.array_equal(out["shift"], free["shift"])
    assert (free["variation"] <= 1 / 3).all() and np.float32(1 / 3) >= free["variation"].max()          # 1/3 holds nothing
    flat = pjo.project(lattice(), F(0.03), 5, 0.0, 0.0)                  # exactly planar: variation 0 and distance 0 pass both limits
    assert flat["counts"].tolist() == [0, 0, 0, 81]


def test_one_projection_halves_the_noise_of_a_sphere():
    A, centre = noisy_sphere_memory()
    rms = lambda X: float(np.sqrt(np.mean((np.linalg.norm(X.astype(np.float64) - centre, axis=1) - 0.15) ** 2)))
    out = pjo.project(A, F(0.02), 5)
    merged, _ = mo.merge(out["points"], np.zeros((0, 3), F), None, 0.01)
    before, after = rms(A), rms(out["points"])
    print(f"sphere memory: {A.shape[0]} rows, rms {before:.3e}; projected once at r = 0.02: rms {after:.3e} (ratio {after / before:.3f}), "
          f"moved {out['counts'][3]}, no plane {out['counts'][1]}; merged again at 0.01: {merged.shape[0]} rows, rms {rms(merged):.3e}")
    assert 0.8 * 0.002 < before < 1.2 * 0.002                            # the memory carries the noise of its scans
    assert after < 0.5 * before
    assert merged.shape[0] < A.shape[0] and rms(merged) < 0.5 * before


# ------------------------------------------------------------------------------------------------ the library, host side only
def test_symbols_and_bindings():
    from livingscenes_amd import _lib, ops
    from livingscenes_amd.lib_more.more_solver import More_Solver, solve_sequence
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "livingscenes_hip.h")).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and name + "(" in header, name
    assert int(lib.ls_version()) == _lib.ABI_VERSION == 107
    for f in (ops.cloud_project, ops.cloud_project_batch):
        sig = inspect.signature(f).parameters
        assert sig["radius"].default is inspect.Parameter.empty and sig["radius"].kind is inspect.Parameter.KEYWORD_ONLY
        assert (sig["min_nbrs"].default, sig["max_variation"].default, sig["max_shift"].default) == (5, 1 / 3, INF)
        assert "no limit" in f.__doc__.lower() and "by construction" in f.__doc__
    assert inspect.signature(ops.cloud_project_batch).parameters["packed"].default is False
    sig = inspect.signature(More_Solver._consolidate_batch).parameters
    assert [sig[k].default for k in ("radius", "voxel", "min_nbrs", "max_variation", "max_shift")] == [None, None, 5, 1 / 3, INF]
    assert "derived" in More_Solver._consolidate_batch.__doc__.lower() and "not tuned" in More_Solver._consolidate_batch.__doc__.lower()
    sig = inspect.signature(solve_sequence).parameters
    assert [sig[k].default for k in ("consolidate", "consolidate_radius", "consolidate_max_variation", "consolidate_max_shift")] == \
        [False, None, 1 / 3, INF]
    doc = solve_sequence.__doc__
    assert "CPU EXPERIMENT" in doc and "8.4e-4" in doc and "1.78e-3" in doc and "_consolidate_batch" in doc and "own risk" in doc


def test_workspace_sizes():
    from livingscenes_amd import _lib
    lib = _lib.load()
    one, batch = lib.ls_cloud_project_workspace_bytes, lib.ls_cloud_project_batch_workspace_bytes
    nrm, nrm_batch = lib.ls_cloud_normals_workspace_bytes, lib.ls_cloud_normals_batch_workspace_bytes
    assert one(-1) == 0 and one(2 ** 31) == 0 and batch(0, 1) == 0 and batch(1, -1) == 0 and batch(2, 2 ** 31) == 0
    assert one(0) > 0 and one(0) % 256 == 0
    grid = (0, 1, 100, 255, 256, 257, 4096, 4097, 60000, 3840000)
    sizes = [one(n) for n in grid]
    assert sizes == sorted(sizes) and sizes[-1] > sizes[0] and all(v % 256 == 0 for v in sizes)
    # the normals' layout plus 8 bytes per chunk of 256 rows, in a piece that is padded to 256 bytes like every other
    for n in grid:
        assert nrm(n) + 8 * (n // 256) - 255 <= one(n) <= nrm(n) + 8 * (n // 256) + 256, n
        for P in (1, 7):
            assert nrm_batch(P, n) + 8 * (n // 256) - 255 <= batch(P, n) <= nrm_batch(P, n) + 8 * (n // 256) + 256, (P, n)
            assert batch(P, n) >= one(n) and batch(P, n) % 256 == 0
    assert [batch(P, 1000) for P in (1, 2, 64)] == sorted(batch(P, 1000) for P in (1, 2, 64))


def _batch(lib, P, a_total, a_off, radius, min_nbrs=5, max_variation=1 / 3, max_shift=INF, ws_bytes=64, alias=False):
    """the batch entry with host arrays and made-up buffers: only for calls the host checks refuse before anything is dereferenced"""
    A, out, buf = (ctypes.c_float * 4096)(), (ctypes.c_float * 4096)(), (ctypes.c_float * 4096)()
    ao, rd = np.asarray(a_off, np.int64), np.asarray(radius, np.float32)
    rc = lib.ls_cloud_project_batch_f32(P, A, a_total, ao.ctypes.data, rd.ctypes.data, min_nbrs, max_variation, max_shift, A if alias else out, buf,
                                        buf, buf, buf, None, buf, ws_bytes, None)
    return rc, lib.ls_last_error().decode()


def _one(lib, a=3, radius=0.1, min_nbrs=5, max_variation=1 / 3, max_shift=INF, ws=True, ws_bytes=64, alias=None):
    """the single entry likewise; alias = k: out_pts starts k floats into A"""
    A, out, buf = (ctypes.c_float * 4096)(), (ctypes.c_float * 4096)(), (ctypes.c_float * 4096)()
    dst = out if alias is None else ctypes.c_void_p(ctypes.addressof(A) + 4 * alias)
    rc = lib.ls_cloud_project_f32(A, a, radius, min_nbrs, max_variation, max_shift, dst, buf, buf, buf, buf, None, buf if ws else None, ws_bytes, None)
    return rc, lib.ls_last_error().decode()


def test_every_host_refusal():
    from livingscenes_amd import _lib
    lib = _lib.load()
    INVALID, WORKSPACE = -1, -3
    name = "cloud_project_batch"
    rc, msg = _batch(lib, 3, 30, [0, 10, 5, 30], [0.1, 0.1, 0.1])
    assert rc == INVALID and name in msg and "problem 1" in msg and "a_off" in msg and "decreases" in msg, msg
    rc, msg = _batch(lib, 3, 30, [0, 10, 20, 29], [0.1, 0.1, 0.1])
    assert rc == INVALID and "problem 2" in msg and "ends at 29" in msg, msg
    rc, msg = _batch(lib, 3, 30, [1, 10, 20, 30], [0.1, 0.1, 0.1])
    assert rc == INVALID and "a_off[0]" in msg, msg
    for bad in (0.0, -0.5, float("nan"), INF, 1e-45, 1e-30, 1e30):
        rc, msg = _batch(lib, 3, 30, [0, 10, 20, 30], [0.1, 0.1, bad])
        assert rc == INVALID and name in msg and "problem 2" in msg and "radius" in msg, (bad, msg)
        rc, msg = _one(lib, radius=bad)
        assert rc == INVALID and "radius" in msg, (bad, msg)
    rc, msg = _batch(lib, 0, 0, [0], [0.1])
    assert rc == INVALID and "P must be" in msg
    good = (2, 10, [0, 5, 10], [0.1, 0.2])
    for call in (lambda **kw: _batch(lib, *good, **kw), lambda **kw: _one(lib, **kw)):
        for bad in (0, -3):
            rc, msg = call(min_nbrs=bad)
            assert rc == INVALID and "min_nbrs" in msg, msg
        for bad in (float("nan"), -1e-9, -INF):
            rc, msg = call(max_variation=bad)
            assert rc == INVALID and "max_variation" in msg, (bad, msg)
            rc, msg = call(max_shift=bad)
            assert rc == INVALID and "max_shift" in msg, (bad, msg)
        rc, msg = call(max_variation=0.0, max_shift=0.0)                 # both limits at their least, +inf and 5.0 too: only the workspace is short
        assert rc == WORKSPACE and "workspace" in msg, msg
        rc, msg = call(max_variation=5.0, max_shift=INF)
        assert rc == WORKSPACE and "workspace" in msg, msg
    rc, msg = _batch(lib, *good, alias=True)
    assert rc == INVALID and "out_pts" in msg and "overlaps A" in msg, msg
    rc, msg = _one(lib, alias=0)
    assert rc == INVALID and "out_pts" in msg and "overlaps A" in msg, msg
    rc, msg = _one(lib, a=3, alias=8)                                    # out_pts starts inside A's nine floats
    assert rc == INVALID and "overlaps A" in msg, msg
    rc, msg = _one(lib, a=3, alias=9)                                    # right behind A: no overlap, only the workspace is short
    assert rc == WORKSPACE, msg
    rc, msg = _batch(lib, *good)
    assert rc == WORKSPACE and "ls_cloud_project_batch_workspace_bytes(2, 10)" in msg, msg
    rc, msg = _batch(lib, *good, ws_bytes=lib.ls_cloud_project_batch_workspace_bytes(2, 10) - 1)
    assert rc == WORKSPACE and "workspace" in msg, msg
    rc, msg = _one(lib, ws=False, ws_bytes=0)
    assert rc == WORKSPACE and "ls_cloud_project_workspace_bytes(3)" in msg, msg
    rc, msg = _one(lib, a=-1)
    assert rc == INVALID and "negative" in msg, msg
