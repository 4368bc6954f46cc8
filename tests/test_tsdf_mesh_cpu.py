"""CPU-only tests (-m "not gpu") of the scene memory's mesh of a fused state (include/livingscenes_hip.h: ls_tsdf_mesh_f64): the property
of the triangle table the local rule rests on; the rule (tests/tsdf_mesh_oracle.py) against fuse_oracle.compact; csrc/tsdfmesh_plan.h --
compiled on its own with the host compiler and run through all five passes by tests/tools/tsdfmesh_plan_run.cpp, plain and under
AddressSanitizer / UBSan -- against fuse_oracle.mesh by equality; what the C entry points decide on the host before any HIP call; and the
fused sphere.  The states and the size edges of tests/test_hip_tsdf_mesh.py live here."""
import ctypes
import functools
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, ".."))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import fuse_oracle as fo          # noqa: E402
import tsdf_mesh_oracle as tmo    # noqa: E402
from oracle import mcubes as om   # noqa: E402

NAMES = ("ls_tsdf_mesh_workspace_bytes", "ls_tsdf_mesh_f64", "ls_tsdf_mesh_batch_workspace_bytes", "ls_tsdf_mesh_batch_f64")
NAN, INF = float("nan"), float("inf")
PER_BLOCK = 4096                  # MESH_PER_BLOCK of csrc/tsdfmesh_plan.h, asserted below against the header itself

# the states whose figures are written down: (dims, min_obs) -> (kept cubes, all cubes, carried, created, faces)
FIGURES = {((20, 21, 22), 1): (5316, 7980, 11967, 14259, 17019), ((17, 17, 17), 1): (2678, 4096, 6485, 7695, 8677), ((5, 7, 11), 1): (163, 240, 493, None, 556),
           ((20, 21, 22), 2): (137, 7980, 701, None, 435)}
# the size edges: one cube; 63 / 64 / 65 cubes; one short of, exactly and one over the cubes per workgroup of the count pass; three unequal dims
EDGE_DIMS = ((2, 2, 2), (2, 2, 64), (2, 2, 65), (2, 2, 66), (16, 22, 14), (17, 17, 17), (2, 18, 242), (5, 7, 11), (20, 21, 22))
ORIGIN, VOXEL = np.array([-0.31, 0.17, 1.003]), 0.0137


@functools.lru_cache(maxsize=None)
def state_of(dims, seed=0):
    return tmo.random_state(seed, dims)


@functools.lru_cache(maxsize=None)
def expected(dims, min_obs, seed=0):
    """the expected mesh of the seeded state, computed once and shared: (vertices, faces, stats)"""
    v, f = tmo.mesh(state_of(dims, seed), ORIGIN, VOXEL, min_obs)
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f, tmo.analyse(state_of(dims, seed), min_obs)["stats"]


def test_size_edges_are_the_edges():
    cubes = [int(np.prod([d - 1 for d in dims])) for dims in EDGE_DIMS]
    assert cubes[:7] == [1, 63, 64, 65, PER_BLOCK - 1, PER_BLOCK, PER_BLOCK + 1]
    assert len(set(EDGE_DIMS[7])) == 3 and len(set(EDGE_DIMS[8])) == 3


# ------------------------------------------------------------------------------------------------ the table and the rule
def test_every_pattern_names_exactly_its_crossed_edges():
    """what "carried iff a kept cube around the edge" rests on: the triangles of a pattern name every crossed edge of the cube, and no other"""
    tri, edge_table = om._tables()
    differ = 0
    for cfg in range(256):
        named = set(int(e) for e in tri[cfg] if e >= 0)
        crossed = set(e for e in range(12) if ((cfg >> om.EDGE_A[e]) & 1) != ((cfg >> om.EDGE_B[e]) & 1))
        assert crossed == set(e for e in range(12) if (edge_table[cfg] >> e) & 1)
        differ += named != crossed
    assert differ == 0
    # the table the library compiles is the oracle's
    text = open(os.path.join(REPO, "livingscenes_amd", "csrc", "mc_tables.h")).read().split("MC_TRI_TABLE[256][16] = {")[1].split("};")[0]
    rows = np.array([int(t) for t in text.replace("{", " ").replace("}", " ").replace(",", " ").split()]).reshape(256, 16)
    assert np.array_equal(rows, tri)


@pytest.mark.parametrize("key", sorted(FIGURES))
def test_the_rule_is_the_compaction_and_the_figures_hold(key):
    dims, min_obs = key
    state = state_of(dims)
    a = tmo.analyse(state, min_obs)
    verts, faces = fo.masked_marching_cubes(a["D"], a["valid"], 0.0)
    used = np.zeros(len(verts), bool)
    used[faces.reshape(-1)] = True                                  # "named by some kept face", as fuse_oracle.compact has it
    assert np.array_equal(tmo.carried_in_creation_order(a), used)
    v1, f1 = tmo.mesh_by_rule(state, ORIGIN, VOXEL, min_obs)
    v2, f2, stats = expected(dims, min_obs)
    assert np.array_equal(v1.view(np.int64), v2.view(np.int64)) and np.array_equal(f1, f2)
    kept, cubes, carried, created, nf = FIGURES[key]
    assert (int(a["kept"].sum()), a["kept"].size, int(a["carried"].sum()), len(f2)) == (kept, cubes, carried, nf)
    assert created is None or int(a["creates"].sum()) == created
    assert stats[0] == kept and stats[2] == a["valid"].sum()
    # both ends of a carried edge are valid, and a carried vertex may be owned by a dropped cube
    cx, cy, cz = a["kept"].shape
    for e in range(12):
        for corner in (om.EDGE_A[e], om.EDGE_B[e]):
            dx, dy, dz = om.CORNER[corner]
            assert a["valid"][dx:dx + cx, dy:dy + cy, dz:dz + cz][a["carried"][..., e]].all()
    assert (a["carried"].any(-1) & ~a["kept"]).any()
    if min_obs == 2:
        owners = a["carried"].any(-1)
        assert (owners & ~a["kept"]).sum() > (owners & a["kept"]).sum()       # the sparse mesh: most owners of carried vertices are dropped cubes


def test_coverage_of_the_gpu_states():
    """what tests/test_hip_tsdf_mesh.py asserts again before it compares: the big states reach all 256 patterns in kept cubes, drop vertices, and have faces"""
    for dims in ((20, 21, 22), (17, 17, 17)):
        a = tmo.analyse(state_of(dims), 1)
        assert len(np.unique(a["cfg"][a["kept"]])) == 256
        assert 0 < a["carried"].sum() < a["creates"].sum()
    for dims in EDGE_DIMS:
        for min_obs in (1, 2):
            assert expected(dims, min_obs)[1].min(initial=0) >= 0


# ------------------------------------------------------------------------------------------------ tsdfmesh_plan.h, all five passes on the host
def _compile(out, flags):
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *flags, "-I",
                    os.path.join(REPO, "livingscenes_amd", "csrc"), os.path.join(HERE, "tools", "tsdfmesh_plan_run.cpp"), "-o", out], check=True)
    return out


@pytest.fixture(scope="module")
def runners(tmp_path_factory):
    d = tmp_path_factory.mktemp("tsdfmesh_plan")
    return {"plain": _compile(str(d / "run"), ["-O1"]),
            "sanitized": _compile(str(d / "run_san"), ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])}


def run_plan(exe, state, origin, voxel, min_obs):
    S, N = state
    text = " ".join([*(str(d) for d in S.shape), str(min_obs), *(float(t).hex() for t in origin), float(voxel).hex()]) + "\n"
    text += " ".join(map(str, S.reshape(-1).tolist())) + "\n" + " ".join(map(str, N.reshape(-1).tolist())) + "\n"
    out = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    lines = out.stdout.splitlines()
    nv, nf, *stats = (int(t) for t in lines[0].split())
    assert len(lines) == 1 + nv + nf
    verts = np.array([[float.fromhex(t) for t in line.split()] for line in lines[1:1 + nv]], np.float64).reshape(nv, 3)
    faces = np.array([[int(t) for t in line.split()] for line in lines[1 + nv:]], np.int64).reshape(nf, 3)
    return verts, faces, np.array(stats, np.int64)


def _same(got, want):
    gv, gf, gs = got
    wv, wf, ws = want
    assert gv.shape == wv.shape and gf.shape == wf.shape, (gv.shape, wv.shape, gf.shape, wf.shape)
    assert not np.isnan(gv).any() and (gf >= 0).all() and (gf < max(len(gv), 1)).all()
    assert np.array_equal(gf, wf)
    assert np.array_equal(gv.view(np.int64), wv.view(np.int64))              # bitwise
    assert np.array_equal(gs, ws)


def test_header_constants(runners):
    out = subprocess.run([runners["plain"]], input="constants\n", capture_output=True, text=True, check=True).stdout.split()
    assert [int(t) for t in out] == [256, 16, PER_BLOCK, 65535]


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_host_program_equals_the_oracle(runners, which):
    """every size edge and both min_obs; the sanitised build is the same program with its own main: nothing is preloaded"""
    for dims in EDGE_DIMS:
        for min_obs in (1, 2):
            _same(run_plan(runners[which], state_of(dims), ORIGIN, VOXEL, min_obs), expected(dims, min_obs))
    # no cube, no valid sample, everything valid and on one side, a flat D (f1 == f2 never crossed; 0 against 0 is no crossing)
    S, N = state_of((5, 7, 11))
    for state in ((S[:1], N[:1]), (S[:, :1], N[:, :1]), (S, np.zeros_like(N)), (np.abs(S) + 1, np.maximum(N, 1)), (np.zeros_like(S), np.ones_like(N))):
        state = tuple(np.ascontiguousarray(t) for t in state)
        v, f = tmo.mesh(state, ORIGIN, VOXEL, 1)
        _same(run_plan(runners[which], state, ORIGIN, VOXEL, 1), (v, f, tmo.analyse(state, 1)["stats"] if min(state[0].shape) >= 2 else
                                                               np.array([0, 0, (state[1] >= 1).sum()])))
    # zeros on the surface: D == 0 counts as inside, an edge between 0 and a positive value puts its vertex ON the sample
    rng = np.random.default_rng(5)
    N = np.ones((6, 5, 4), np.int32)
    S = (rng.integers(-2, 3, size=N.shape) * 4096).astype(np.int32)
    v, f = tmo.mesh((S, N), ORIGIN, VOXEL, 1)
    assert len(f) > 0 and (S == 0).any()
    _same(run_plan(runners[which], (S, N), ORIGIN, VOXEL, 1), (v, f, tmo.analyse((S, N), 1)["stats"]))


def test_sphere_vertices_lie_within_a_cube_diagonal(runners):
    """the fused 4-view sphere of test_depth_fuse_cpu: every vertex of the host program's mesh within sqrt(3) h of the sphere"""
    from test_depth_fuse_cpu import sphere_state
    (S, N), origin, h = sphere_state()
    verts, faces, stats = run_plan(runners["plain"], (S, N), origin, h, 1)
    wv, wf = fo.mesh((S, N), origin, h)
    assert np.array_equal(verts.view(np.int64), wv.view(np.int64)) and np.array_equal(faces, wf)
    err = np.abs(np.linalg.norm(verts, axis=1) - 0.4)
    print(f"sphere: {len(verts)} vertices, {len(faces)} faces, kept {stats[0]}, dropped with a crossing {stats[1]}, max error {err.max() / h:.3f} h")
    assert len(faces) > 1000 and len(np.unique(faces)) == len(verts)
    assert err.max() <= np.sqrt(3) * h


# ------------------------------------------------------------------------------------------------ the library, host side only
def test_symbols_and_bindings():
    from livingscenes_amd import _lib, build, ops
    from livingscenes_amd.lib_more.more_solver import More_Solver, solve_sequence
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "livingscenes_hip.h")).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and name + "(" in header, name
        res, args = _lib.SIGNATURES[name]
        assert getattr(lib, name).restype is res and list(getattr(lib, name).argtypes) == list(args)
    assert len(_lib.SIGNATURES["ls_tsdf_mesh_f64"][1]) == 17 and len(_lib.SIGNATURES["ls_tsdf_mesh_batch_f64"][1]) == 18
    assert int(lib.ls_version()) == _lib.ABI_VERSION == 107 and "#define LS_ABI_VERSION 107" in header
    assert "ls_tsdf_mesh_f64 / ls_tsdf_mesh_batch_f64" in header.split("#define LS_ABI_VERSION")[0]
    assert "tsdfmesh.hip" in build.SOURCES and build.PACKED_FP32_GUARD["tsdfmesh.hip"] == []
    plan_h = open(os.path.join(REPO, "livingscenes_amd", "csrc", "tsdfmesh_plan.h")).read()
    assert "#include <hip" not in plan_h and '#include "ls_' not in plan_h and "contract(off)" in plan_h and "fuse_value" in plan_h
    kernels = open(os.path.join(REPO, "livingscenes_amd", "csrc", "tsdfmesh.hip")).read()
    assert "__constant__" not in kernels and "mc_launch" not in kernels and "hipMalloc" not in kernels and "Synchronize" not in kernels
    assert kernels.count("LS_MESH_PASS(\"") == 6                              # one per launch (classify twice: with and without cubes)
    for f, batch in ((ops.tsdf_mesh, False), (ops.tsdf_mesh_batch, True)):
        sig = inspect.signature(f).parameters
        assert list(sig)[0] == "state" and sig["min_obs"].default == 1 and ("packed" in sig) == batch
        for k in ("origin", "voxel"):
            assert sig[k].default is inspect.Parameter.empty and sig[k].kind is inspect.Parameter.KEYWORD_ONLY
        assert "NO min_obs IS RECOMMENDED" in f.__doc__
    assert inspect.signature(More_Solver._observed_mesh_batch).parameters["min_obs"].default == 1
    sig = inspect.signature(solve_sequence).parameters
    assert [sig[k].default for k in ("fuse_mesh", "fuse_min_obs")] == [False, 1]
    assert "observed_meshes" in solve_sequence.__doc__ and "NOT BUILT YET" not in solve_sequence.__doc__


def test_workspace_sizes():
    from livingscenes_amd import _lib
    lib = _lib.load()
    one, batch = lib.ls_tsdf_mesh_workspace_bytes, lib.ls_tsdf_mesh_batch_workspace_bytes
    assert one(0, 4, 4) == 0 and one(4, -1, 4) == 0 and one(4, 4, 0) == 0 and one(524, 524, 524) == 0 and one(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1) == 0
    assert batch(0, 4, 4, 4) == 0 and batch(-1, 4, 4, 4) == 0 and batch(65536, 2, 2, 2) == 0 and batch(65535, 2, 2, 2) > 0
    assert one(523, 523, 523) > 0 and 15 * 523 ** 3 < 2 ** 31 <= 15 * 524 ** 3
    assert batch(64, 130, 130, 130) > 0 and batch(64, 131, 131, 131) == 0 and 15 * 64 * 130 ** 3 < 2 ** 31 <= 15 * 64 * 131 ** 3
    assert one(1, 5, 5) == one(5, 1, 5) == one(5, 5, 1) == 256
    for dims in ((2, 2, 2), (17, 17, 17), (2, 18, 242), (64, 64, 64)):
        cubes = int(np.prod([d - 1 for d in dims]))
        nblk = -(-cubes // PER_BLOCK)
        for P in (1, 3, 64):
            a256 = lambda x: -(-x // 256) * 256                                # noqa: E731
            want = 2 * a256(2 * P * cubes) + 2 * a256(4 * P * cubes) + a256(8 * (P * nblk + 1)) + a256(32 * P)
            assert batch(P, *dims) == want and (P != 1 or one(*dims) == want)


GOOD = dict(P=2, nx=4, ny=4, nz=4, min_obs=1, cap_v=0, cap_f=0)


def _call(lib, single=False, origin=None, voxel=None, ws=True, ws_bytes=0, null=(), with_outputs=(True, True), **kw):
    """the entries with made-up buffers: only for calls the host checks refuse before anything is dereferenced"""
    s = dict(GOOD, **kw)
    P = 1 if single else s["P"]
    state, buf = (ctypes.c_int * 4096)(), (ctypes.c_double * 4096)()
    o = np.ascontiguousarray(np.zeros((max(P, 1), 3)) if origin is None else origin, np.float64)
    h = np.ascontiguousarray(np.full(max(P, 1), 0.01) if voxel is None else voxel, np.float64)
    b = {k: (None if k in null else state) for k in ("sum", "n")}
    b.update({k: (None if k in null else buf) for k in ("off", "stats")})
    optr = None if "origin" in null else o.ctypes.data
    V, F = (buf if w else None for w in with_outputs)
    tail = (V, s["cap_v"], F, s["cap_f"], b["off"], b["stats"], buf if ws else None, ws_bytes, None)
    if single:
        rc = lib.ls_tsdf_mesh_f64(b["sum"], b["n"], s["nx"], s["ny"], s["nz"], s["min_obs"], optr, float(h[0]), *tail)
    else:
        rc = lib.ls_tsdf_mesh_batch_f64(P, b["sum"], b["n"], s["nx"], s["ny"], s["nz"], s["min_obs"], optr, None if "voxel" in null else h.ctypes.data, *tail)
    return rc, lib.ls_last_error().decode()


def test_every_host_refusal():
    from livingscenes_amd import _lib
    lib = _lib.load()
    INVALID, WORKSPACE = -1, -3
    for single, name in ((False, "tsdf_mesh_batch"), (True, "tsdf_mesh")):
        call = functools.partial(_call, lib, single)
        for dims in (dict(nx=0), dict(ny=-1), dict(nz=0)):
            rc, msg = call(**dims)
            assert rc == INVALID and msg.startswith(name + ":") and "dims must be at least 1" in msg, msg
        rc, msg = call(nx=524, ny=524, nz=524)
        assert rc == INVALID and "reaches 2^31" in msg, msg
        rc, msg = call(nx=2 ** 31 - 1, ny=2 ** 31 - 1, nz=2 ** 31 - 1)
        assert rc == INVALID and "reaches 2^31" in msg, msg
        for bad in (0, -3):
            rc, msg = call(min_obs=bad)
            assert rc == INVALID and "min_obs must be >= 1" in msg, msg
        for bad in (0.0, -0.01, NAN, INF):
            rc, msg = call(voxel=[0.01, bad][-1:] if single else [0.01, bad])
            assert rc == INVALID and f"problem {0 if single else 1}" in msg and "voxel must be finite and > 0" in msg, (bad, msg)
        for bad in (NAN, INF, -INF):
            o = np.zeros((1 if single else 2, 3))
            o[-1, 1] = bad
            rc, msg = call(origin=o)
            assert rc == INVALID and f"problem {0 if single else 1}" in msg and "origin must be finite" in msg, (bad, msg)
        for caps in (dict(cap_v=-1), dict(cap_f=-1)):
            rc, msg = call(**caps)
            assert rc == INVALID and "negative capacity" in msg, msg
        for k in ("sum", "n", "off"):
            rc, msg = call(null=(k,))
            assert rc == INVALID and "null sum / n / off_out" in msg, (k, msg)
        rc, msg = call(null=("origin",))
        assert rc == INVALID and "null origin / voxel" in msg, msg
        for outs in ((True, False), (False, True)):
            rc, msg = call(with_outputs=outs)
            assert rc == INVALID and "given together" in msg, msg
        # the accepted extremes: only the workspace is short, and the error names the query
        rc, msg = call(voxel=[1e-300] * 2, min_obs=2 ** 31 - 1, null=("stats",), with_outputs=(False, False))
        assert rc == WORKSPACE and f"ls_{name}_workspace_bytes" in msg, msg
        rc, msg = call(ws=False, ws_bytes=1 << 30)
        assert rc == WORKSPACE, msg
        need = lib.ls_tsdf_mesh_workspace_bytes(4, 4, 4) if single else lib.ls_tsdf_mesh_batch_workspace_bytes(2, 4, 4, 4)
        rc, msg = call(ws_bytes=need - 1)
        assert rc == WORKSPACE and f"{need - 1} < required {need}" in msg, msg
    for P in (0, -1, 65536):
        rc, msg = _call(lib, P=P)
        assert rc == INVALID and "outside 1..65535" in msg, msg
    rc, msg = _call(lib, P=64, nx=131, ny=131, nz=131)
    assert rc == INVALID and "15 * P * nx * ny * nz" in msg and "reaches 2^31" in msg, msg
    rc, msg = _call(lib, null=("voxel",))
    assert rc == INVALID and "null origin / voxel" in msg, msg
