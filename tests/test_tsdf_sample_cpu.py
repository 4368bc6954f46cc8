"""CPU-only tests (-m "not gpu") of the scene memory's sampling of a fused state and of the registration on it
(include/livingscenes_hip.h: ls_tsdf_sample_f32, ls_tsdf_icp_f32): csrc/tsdfsample_plan.h -- compiled on its own with the host compiler and
run by tests/tools/tsdf_sample_plan_run.cpp, plain and under AddressSanitizer / UBSan -- against tests/tsdf_sample_oracle.py by equality;
the twin's gradient against a central difference of the twin's own value; what the C entry points decide on the host before any HIP call;
the bindings; and solve_sequence's two new refusals.  The states, the grids and the queries of tests/test_hip_tsdf_icp.py live here.

States.  Per dims a fused sphere and a fused box (analytic depth maps through fuse_oracle.fuse on a dyadic grid, so that a row ON a
face of the grid is an exact fp32 number) and a hand-made state with holes and a block of saturated free space on a grid that is not
dyadic.  Queries: 513 rows per (state, min_obs), every shorter count a prefix.  A grid of dims (2,2,2) has ONE cell, which is SAMPLED or
UNSEEN as a whole: there the three query states cannot meet in one state, and the precondition asked of it is OUT plus the cell's own
state, with both SAMPLED and UNSEEN reached over the kinds and min_obs; every other (state, min_obs) holds all three."""
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
import fuse_oracle as fo               # noqa: E402
import tsdf_sample_oracle as tso       # noqa: E402
from test_depth_fuse_cpu import _look_at, _rot, _sphere_depth   # noqa: E402

NAMES = ("ls_tsdf_sample_workspace_bytes", "ls_tsdf_sample_f32", "ls_tsdf_sample_batch_workspace_bytes", "ls_tsdf_sample_batch_f32",
         "ls_tsdf_icp_workspace_bytes", "ls_tsdf_icp_f32", "ls_tsdf_icp_batch_workspace_bytes", "ls_tsdf_icp_batch_f32")
F = np.float32
NAN, INF = float("nan"), float("inf")
DIMS = ((2, 2, 2), (2, 3, 5), (9, 8, 7), (17, 16, 33))
KINDS = ("sphere", "box", "holes")
COUNTS = (1, 255, 256, 257, 513)
BOX_HALF = np.array([0.22, 0.3, 0.38])
VIEWS = 2


def grid_of(kind, dims):
    """-> (origin [3], voxel, trunc).  sphere / box: h a power of two with the longest side about 1, the grid centred on a dyadic point:
    origin + h k is exact in fp32 for every lattice index k.  holes: the grid of the mesh tests, not dyadic."""
    if kind == "holes":
        return np.array([-0.31, 0.17, 1.003]), 0.0137, 3 * 0.0137
    h = 2.0 ** -int(round(np.log2(max(dims) - 1)))
    centre = np.array([0.1875, -0.3125, 1.0])
    return centre - h * (np.array(dims) - 1) / 2, h, (1.0 if max(dims) <= 5 else 2.0) * h


def _box_depth(E, K, H, W, half):
    """the analytic z-depth of the box |x_a| <= half_a at the origin (slabs), 0 where the ray misses it"""
    fx, fy, cx, cy = K
    py, px = np.mgrid[0:H, 0:W]
    d = np.stack([(px - cx) / fx, (py - cy) / fy, np.ones((H, W))], -1)
    R, t = E[:, :3], E[:, 3]
    o, dw = -R.T @ t, d @ R
    with np.errstate(all="ignore"):
        t0, t1 = (-half - o) / dw, (half - o) / dw
    near, far = np.minimum(t0, t1).max(-1), np.maximum(t0, t1).min(-1)
    return np.where((near <= far) & (near > 0), near, 0.0).astype(F)


@functools.lru_cache(maxsize=None)
def state_of(kind, dims):
    """-> ((sum, n), origin, voxel, trunc), computed once and shared; read-only"""
    origin, h, trunc = grid_of(kind, dims)
    if kind == "holes":
        rng = np.random.default_rng(sum(dims))
        N = rng.choice([0, 1, 2, 3], size=dims, p=[.04, .06, .45, .45])
        S = rng.integers(-16384, 16385, size=dims) * N
        far = (slice(None), slice(None), slice(dims[2] // 2, None))        # a slab of saturated free space (observed, D = +1 exactly) ...
        N[far] = np.maximum(N[far], 2)
        S[far] = 16384 * N[far]
        if max(dims) > 2:
            N[tuple(d - 1 for d in dims)] = 0                               # ... with one unobserved corner in it
            S[tuple(d - 1 for d in dims)] = 0
        else:
            N = np.maximum(N, 1)                                            # the one-cell grid: its cell observed
        state = (S.astype(np.int32), N.astype(np.int32))
    else:
        rng = np.random.default_rng(7)
        K = np.array([100.0, 100.0, 50.0, 50.0])
        rots = []
        while len(rots) < VIEWS:                                          # cameras on one side: the object's shadow stays unobserved
            R = _rot(rng)
            if R[2, 2] > 0.6:
                rots.append(R)
        E = np.stack([_look_at(R) for R in rots])                         # the object's frame: its centre at 0
        depth = np.stack([_sphere_depth(e, K, 100, 100, 0.4) if kind == "sphere" else _box_depth(e, K, 100, 100, BOX_HALF) for e in E])
        centre = origin + h * (np.array(dims) - 1) / 2
        Eg = E.copy()
        Eg[:, :, 3] -= E[:, :, :3] @ centre                               # the same cameras from the grid's frame
        state = fo.new_state(dims)
        fo.fuse(state, depth, np.tile(K, (VIEWS, 1)), Eg, origin, h, trunc, empty="free")   # a ray that hits nothing saw free space
    for t in state:
        t.setflags(write=False)
    return state, origin, h, trunc


@functools.lru_cache(maxsize=None)
def queries_of(kind, dims, min_obs):
    """513 fp32 rows in the grid's frame: row 0 inside the grid; rows exactly on the low and the far face of every axis and one ulp
    outside and inside each; lattice points; NaN and +-inf rows; rows in cells with exactly one invalid corner, in SAMPLED cells and in
    cells of saturated free space (where the state has such cells); rows far outside; the rest uniform over the grid and half a voxel
    around it.  Shuffled behind row 0, so every prefix is a mix."""
    (S, N), origin, h, _ = state_of(kind, dims)
    rng = np.random.default_rng(1000 * min_obs + sum(dims) + len(kind))
    n = np.array(dims)
    D, valid = tso.corner_values((S, N), min_obs)
    cells = tuple(d - 1 for d in dims)
    bad = np.zeros(cells, np.int64)
    sat = np.ones(cells, bool)
    for a in range(2):
        for b in range(2):
            for c in range(2):
                sl = (slice(a, a + cells[0]), slice(b, b + cells[1]), slice(c, c + cells[2]))
                bad += ~valid[sl]
                sat &= valid[sl] & (D[sl] == 1.0)
    rows = []

    def at(u):
        rows.append((origin + h * np.asarray(u, np.float64)).astype(F))

    def inside_cells(mask, count):
        where = np.argwhere(mask)
        for c in where[rng.permutation(len(where))[:count]]:
            at(c + rng.uniform(0.05, 0.95, 3))

    inside_cells(bad == 0, 24)
    inside_cells(bad == 1, 24)
    inside_cells(bad >= 1, 24)
    inside_cells(sat, 12)
    for a in range(3):
        for face in (0.0, float(n[a] - 1)):
            for _ in range(2):
                u = rng.uniform(0, 1, 3) * (n - 1)
                u[a] = face
                at(u)
                on = rows[-1]
                for toward in (-INF, INF):
                    step = on.copy()
                    step[a] = np.nextafter(on[a], F(toward))
                    rows.append(step)
    for k in (np.zeros(3), n - 1.0, np.array([0.0, n[1] - 1.0, 0.0]), *(np.floor(rng.uniform(0, 1, (12, 3)) * n))):
        at(k)
    rows += [F([NAN, 0, 0]), F([origin[0], INF, origin[2]]), F([origin[0], origin[1], -INF]), F([NAN, INF, -INF])]
    for far in (-1e6, 1e6, 3e38):
        at(rng.uniform(0, 1, 3) * (n - 1) + [far / h, 0, 0])
    first = (origin + h * (np.argwhere(bad < 9)[0] + 0.5)).astype(F)
    rest = np.stack(rows)
    fill = (origin + h * (rng.uniform(0.0, 1.0, (512 - len(rest), 3)) * n - 0.5)).astype(F)
    rest = np.concatenate([rest, fill])[rng.permutation(512)]
    B = np.concatenate([first[None], rest])
    assert B.shape == (513, 3) and B.dtype == F
    B.setflags(write=False)
    return B


def pose_of(seed):
    """a rigid fp32 pose [3,4] a few degrees and centimetres off the identity"""
    rng = np.random.default_rng(seed)
    w = rng.normal(size=3)
    w *= np.deg2rad(7.0) / np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    th = np.linalg.norm(w)
    R = np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)
    return np.concatenate([R, rng.uniform(-0.05, 0.05, (3, 1))], 1).astype(F)


def unposed(B, g):
    """rows that g takes (about) onto B: B under the inverse of g, rounded to fp32"""
    g = g.astype(np.float64)
    with np.errstate(all="ignore"):
        return ((B.astype(np.float64) - g[:, 3]) @ g[:, :3]).astype(F)


@functools.lru_cache(maxsize=None)
def expected(kind, dims, min_obs, posed):
    """the twin's sample of the 513 queries, computed once and shared -> (B, g, dict)"""
    state, origin, h, trunc = state_of(kind, dims)
    B, g = queries_of(kind, dims, min_obs), None
    if posed:
        g = pose_of(sum(dims))
        B = unposed(B, g)
    return B, g, tso.sample(state, B, g, origin, h, trunc, min_obs)


def test_every_state_holds_every_query_state():
    one_cell = set()
    for kind in KINDS:
        for dims in DIMS:
            for min_obs in (1, 2):
                for posed in (False, True):
                    s = expected(kind, dims, min_obs, posed)[2]
                    have = set(np.unique(s["state"]).tolist())
                    if dims == (2, 2, 2):
                        assert tso.OUT in have and len(have) == 2, (kind, min_obs, have)
                        one_cell |= have
                    else:
                        assert have == {tso.OUT, tso.UNSEEN, tso.SAMPLED}, (kind, dims, min_obs, posed, have)
                    assert (s["counts"][0] <= 509 if posed else s["counts"][0] == 509) and s["counts"][1] == (s["state"] != tso.OUT).sum()
                if max(dims) > 5:
                    s = expected(kind, dims, min_obs, False)[2]
                    sampled = s["state"] == tso.SAMPLED
                    assert (sampled & (s["phi"] == state_of(kind, dims)[3]) & ~s["grad"].any(1)).any(), (kind, dims, min_obs, "saturated free space")
                    assert (np.abs(s["phi"][sampled]) < 0.5 * state_of(kind, dims)[3]).any() or kind == "holes", (kind, dims, "near the surface")
    assert one_cell == {tso.OUT, tso.UNSEEN, tso.SAMPLED}


def test_the_faces_belong_to_the_grid_and_one_ulp_outside_does_not():
    for dims in DIMS:
        (S, N), origin, h, trunc = state_of("sphere", dims)
        n = np.array(dims)
        for a in range(3):
            for face, out in ((0.0, -INF), (float(n[a] - 1), INF)):
                u = (n - 1) * 0.37
                u[a] = face
                on = (origin + h * u).astype(F)
                assert float(on[a]) == origin[a] + h * face                    # the dyadic grid: the face is an fp32 number
                off = on.copy()
                off[a] = np.nextafter(on[a], F(out))
                s = tso.sample((S, N), np.stack([on, off]), None, origin, h, trunc)
                assert s["state"][0] != tso.OUT and s["state"][1] == tso.OUT, (dims, a, face)
        s = tso.sample((S, N), (origin + h * (n - 1.0)).astype(F)[None], None, origin, h, trunc)     # the far corner: the last cell, f = 1
        if s["state"][0] == tso.SAMPLED:
            D = tso.corner_values((S, N), 1)[0]
            assert s["phi"][0] == trunc * D[-1, -1, -1] or abs(s["phi"][0] - trunc * D[-1, -1, -1]) <= 2.0 ** -50 * trunc


def test_lattice_points_read_the_sample():
    """at a lattice point the interpolant is the sample itself: f = 0 leaves a + 0 * (b - a) = a on every axis, exactly"""
    (S, N), origin, h, trunc = state_of("sphere", (9, 8, 7))
    D, valid = tso.corner_values((S, N), 1)
    idx = np.argwhere(np.ones((8, 7, 6), bool))
    s = tso.sample((S, N), (origin + h * idx).astype(F), None, origin, h, trunc)
    m = s["state"] == tso.SAMPLED
    assert m.sum() > 20
    assert np.array_equal(s["phi"][m], trunc * D[idx[m, 0], idx[m, 1], idx[m, 2]])


def test_gradient_is_the_central_difference_of_the_value():
    """The interpolant is affine in every f_a with the other two held, so the central difference (v(f + e) - v(f - e)) / (2 e) of the
    twin's own value has NO truncation error; what is left is rounding.  One lerp a + f (b - a) of values bounded by m = max |D| commits
    at most 3 roundings of numbers <= 3 m: 9 u m with u = 2^-53; three levels of lerps (errors pass through a lerp with factor <= 1):
    27 u m for D_interp, so the difference quotient is off by at most 27 u m / e.  The gradient's G_a is two levels of lerps of
    differences bounded by 2 m, plus the difference itself: (1 + 2 * 9) u 2 m = 38 u m.  Bound: (27 / e + 38) u m, in units of D per
    cell; the same bound times trunc / h in metres per metre.  The test is not vacuous: across the cell the slope along an axis changes
    by the mixed second differences of D, and the test asserts that this change, over the offsets it uses, exceeds the bound a
    thousandfold -- a gradient taken at the wrong place in the cell would fail."""
    u = 2.0 ** -53
    e = 2.0 ** -12
    for kind, dims in (("sphere", (17, 16, 33)), ("box", (9, 8, 7)), ("holes", (9, 8, 7))):
        (S, N), origin, h, trunc = state_of(kind, dims)
        D, valid = tso.corner_values((S, N), 1)
        rng = np.random.default_rng(3)
        cells = np.argwhere(np.ones(tuple(d - 1 for d in dims), bool))
        cells = cells[rng.permutation(len(cells))[:300]]
        D8 = np.stack([np.stack([np.stack([D[cells[:, 0] + a, cells[:, 1] + b, cells[:, 2] + c] for c in range(2)], -1) for b in range(2)], -2)
                       for a in range(2)], -3)
        assert D8.shape == (300, 2, 2, 2)
        f = rng.uniform(0.1, 0.9, (300, 3))
        v, G = tso.interpolate(D8, f)
        m = np.abs(D8).reshape(300, -1).max(1)
        bound = (27 / e + 38) * u * m
        mixed = 0.0
        for a in range(3):
            fp, fm = f.copy(), f.copy()
            fp[:, a] += e
            fm[:, a] -= e
            cd = (tso.interpolate(D8, fp)[0] - tso.interpolate(D8, fm)[0]) / (fp[:, a] - fm[:, a])
            assert (np.abs(cd - G[:, a]) <= bound).all(), (kind, a, np.abs(cd - G[:, a]).max(), bound.min())
            other = f.copy()
            other[:, (a + 1) % 3] = 1.0 - other[:, (a + 1) % 3]                  # the same cell, another place in it
            mixed = max(mixed, np.abs(tso.interpolate(D8, other)[1][:, a] - G[:, a]).max())
        assert mixed > 1000 * bound.max(), (kind, mixed, bound.max())
        # and in metres: the twin's sample against the same quotient taken through its own queries' f
        y = (origin + h * (cells + f)).astype(F)
        s = tso.sample((S, N), y, None, origin, h, trunc)
        uu = (y.astype(np.float64) - origin) / h
        ff = uu - np.minimum(np.floor(uu), np.array(dims) - 2)
        v2, G2 = tso.interpolate(D8, ff)
        ok = s["state"] == tso.SAMPLED
        assert ok.sum() > 50 and s["grad"][ok].any(1).sum() > 10
        assert np.array_equal(s["phi"][ok], trunc * v2[ok]) and np.array_equal(s["grad"][ok], (trunc / h) * G2[ok])


# ------------------------------------------------------------------------------------------------ tsdfsample_plan.h on the host
def _compile(out, flags):
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *flags, "-I",
                    os.path.join(REPO, "livingscenes_amd", "csrc"), os.path.join(HERE, "tools", "tsdf_sample_plan_run.cpp"), "-o", out], check=True)
    return out


@pytest.fixture(scope="module")
def runners(tmp_path_factory):
    d = tmp_path_factory.mktemp("tsdf_sample_plan")
    return {"plain": _compile(str(d / "run"), ["-O1"]),
            "sanitized": _compile(str(d / "run_san"), ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])}


def _hex(values):
    return " ".join(float(v).hex() for v in np.asarray(values).reshape(-1))


def run_plan(exe, state, B, g, origin, voxel, trunc, min_obs):
    S, N = state
    text = " ".join(map(str, [*S.shape, min_obs, int(g is not None), len(B)])) + "\n" + _hex([*origin, voxel, trunc]) + "\n"
    if g is not None:
        text += _hex(g) + "\n"
    text += " ".join(map(str, S.reshape(-1).tolist())) + "\n" + " ".join(map(str, N.reshape(-1).tolist())) + "\n" + _hex(B) + "\n"
    out = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    lines = out.stdout.splitlines()
    assert len(lines) == len(B) + 2
    rows = [line.split() for line in lines[:len(B)]]
    st = np.array([int(r[0]) for r in rows], np.uint8)
    vals = np.array([[float.fromhex(t) for t in r[1:]] for r in rows], np.float64).reshape(len(B), 4)
    return {"state": st, "phi": vals[:, 0], "grad": vals[:, 1:], "counts": np.array(lines[-2].split(), np.int64),
            "record": np.array([float.fromhex(t) for t in lines[-1].split()])}


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def test_header_constants(runners):
    out = subprocess.run([runners["plain"]], input="constants\n", capture_output=True, text=True, check=True).stdout.split()
    assert [int(t) for t in out] == [tso.CHUNK, tso.WAVE, 6, 28, 3, 3]


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_host_program_equals_the_twin(runners, which):
    """every state, both min_obs, with and without a pose; the sanitised build is the same program with its own main: nothing is preloaded"""
    for kind in KINDS:
        for dims in DIMS:
            state, origin, h, trunc = state_of(kind, dims)
            for min_obs in (1, 2):
                for posed in (False, True):
                    B, g, want = expected(kind, dims, min_obs, posed)
                    for b in (513, 257) if posed else (513,):
                        tw = want if b == 513 else tso.sample(state, B[:b], g, origin, h, trunc, min_obs)
                        got = run_plan(runners[which], state, B[:b], g, origin, h, trunc, min_obs)
                        what = (kind, dims, min_obs, posed, b)
                        assert np.array_equal(got["state"], tw["state"]), what
                        assert np.array_equal(_bits(got["phi"]), _bits(tw["phi"])) and np.array_equal(_bits(got["grad"]), _bits(tw["grad"])), what
                        assert np.array_equal(got["counts"], tw["counts"]), what
                        rec = tso.record(tw)
                        assert np.array_equal(_bits(got["record"]), _bits(rec)), what
                        assert got["record"][0] == tw["sum_phi2"]
    # a dimension below 2 has no cell; an all-zero state has no observed corner
    S, N = state_of("holes", (9, 8, 7))[0]
    _, origin, h, trunc = state_of("holes", (9, 8, 7))
    B = queries_of("holes", (9, 8, 7), 1)
    for state in ((S[:1], N[:1]), (S[:, :1], N[:, :1]), (np.zeros_like(S), np.zeros_like(N))):
        state = tuple(np.ascontiguousarray(t) for t in state)
        tw = tso.sample(state, B, None, origin, h, trunc, 1)
        got = run_plan(runners[which], state, B, None, origin, h, trunc, 1)
        assert np.array_equal(got["state"], tw["state"]) and tw["counts"][2] == 0 and not got["record"].any()
        assert (got["phi"] == trunc).all() and not got["grad"].any() and np.array_equal(got["counts"], tw["counts"])
        assert (tw["counts"][1] == 0) == (min(state[0].shape) < 2)


def test_chunk_sum_is_the_stated_tree():
    rng = np.random.default_rng(0)
    v = rng.uniform(0, 1, 700)
    parts = []
    for c in range(0, 700, 256):
        w = np.zeros(256)
        w[:len(v[c:c + 256])] = v[c:c + 256]
        waves = []
        for k in range(4):
            lane = w[64 * k:64 * k + 64].tolist()
            o = 32
            while o:
                for l in range(o):
                    lane[l] = lane[l] + lane[l + o]
                o //= 2
            waves.append(lane[0])
        parts.append((waves[0] + waves[1]) + (waves[2] + waves[3]))
    total = 0.0
    for p in parts:
        total += p
    assert tso.chunk_sum(v) == total and abs(total - v.sum()) < 1e-10 and tso.chunk_sum([]) == 0.0


def test_the_twin_registers_a_sphere_cap():
    """the loop of the twin on the fused sphere: points of the sphere seen from one side, started 2 degrees and trunc / 2 off, end closer"""
    dims = (17, 16, 33)
    state, origin, h, trunc = state_of("sphere", dims)
    centre = origin + h * (np.array(dims) - 1) / 2
    rng = np.random.default_rng(4)
    d = rng.normal(size=(3000, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    pts = centre + 0.4 * d
    s0 = tso.sample(state, pts.astype(F), None, origin, h, trunc)
    pts = pts[s0["state"] == tso.SAMPLED][:350]
    assert len(pts) == 350
    g_off = pose_of(11).astype(np.float64)
    g_off[:, 3] = 0.3 * trunc * np.array([0.6, -0.5, 0.62]) + centre - g_off[:, :3] @ centre
    res = tso.icp(state, pts.astype(F), g_off.astype(F), origin, h, trunc, max_iter=10)
    rms = [np.sqrt(q / max(w, 1)) for _, w, q in res["stat_trace"]]
    assert res["iters"] >= 2 and res["stop"] in (tso.CONVERGED, tso.MAX_ITER) and rms[-1] < 0.5 * rms[0], (res["iters"], res["stop"], rms)
    t_err = lambda g: np.linalg.norm(g[:, :3].astype(np.float64) @ centre + g[:, 3] - centre)   # noqa: E731
    assert t_err(res["g"]) < 0.5 * t_err(g_off), (t_err(res["g"]), t_err(g_off))               # a sphere fixes the translation, not the rotation


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
    assert [len(_lib.SIGNATURES[n][1]) for n in NAMES] == [4, 20, 5, 22, 4, 28, 5, 30]
    assert int(lib.ls_version()) == _lib.ABI_VERSION == 107 and "#define LS_ABI_VERSION 107" in header
    assert "ls_tsdf_sample_f32 / ls_tsdf_sample_batch_f32, ls_tsdf_icp_f32 / ls_tsdf_icp_batch_f32" in header.split("#define LS_ABI_VERSION")[0]
    assert "tsdficp.hip" in build.SOURCES and build.PACKED_FP32_GUARD["tsdficp.hip"] == []
    csrc = os.path.join(REPO, "livingscenes_amd", "csrc")
    plan_h = open(os.path.join(csrc, "tsdfsample_plan.h")).read()
    assert "#include <hip" not in plan_h and '#include "ls_' not in plan_h and "contract(off)" in plan_h and "fuse_value" in plan_h
    kernels = open(os.path.join(csrc, "tsdficp.hip")).read()
    assert "hipMalloc" not in kernels and "Synchronize" not in kernels and "atomicAdd" not in kernels and "atomicCAS" not in kernels
    assert kernels.count("LS_TSDF_PASS(\"") == 5 and "plane_update" in kernels and "pose_row" in kernels
    shared, near = open(os.path.join(csrc, "se3_gn.h")).read(), open(os.path.join(csrc, "cloudnear.hip")).read()
    assert "bool plane_update(" in shared and "double wave_tree_f64(" in shared
    assert "bool plane_update(" not in near and "double wave_tree_f64(" not in near and '#include "se3_gn.h"' in near
    for f, batch, icp in ((ops.tsdf_sample, False, False), (ops.tsdf_sample_batch, True, False), (ops.tsdf_icp, False, True),
                          (ops.tsdf_icp_batch, True, True)):
        sig = inspect.signature(f).parameters
        assert list(sig)[:3] == ["state", "Bs" if batch else "B", "g"] and sig["min_obs"].default == 1 and ("packed" in sig) == batch
        for k in ("origin", "voxel", "trunc"):
            assert sig[k].default is inspect.Parameter.empty and sig[k].kind is inspect.Parameter.KEYWORD_ONLY
        if icp:
            assert [sig[k].default for k in ("max_iter", "rel_thr", "min_matched", "trace")] == [100, 1e-6, 6, False]
            assert "inherited, not tuned" in f.__doc__.lower()
    sig = inspect.signature(More_Solver._refine_on_fusion_batch).parameters
    assert list(sig)[:4] == ["self", "fusion", "new_pcs", "T"] and sig["min_obs"].default == 1
    assert "tsdf" in solve_sequence.__doc__ and "_refine_on_fusion_batch" in solve_sequence.__doc__


def test_solve_sequence_refuses_tsdf_without_a_fusion_or_with_a_radius():
    from livingscenes_amd.lib_more.more_solver import solve_sequence
    with pytest.raises(ValueError, match="fuse_res"):
        solve_sequence(None, None, [], refine_metric="tsdf")
    with pytest.raises(ValueError, match="refine_radius"):
        solve_sequence(None, None, [], refine_metric="tsdf", fuse_res=32, refine_radius=0.05)
    with pytest.raises(ValueError, match="refine_metric"):
        solve_sequence(None, None, [], refine_metric="surface", fuse_res=32)


def test_workspace_sizes():
    from livingscenes_amd import _lib
    lib = _lib.load()
    a256 = lambda x: -(-x // 256) * 256                                        # noqa: E731
    for name, icp in (("ls_tsdf_sample", False), ("ls_tsdf_icp", True)):
        one, batch = getattr(lib, name + "_workspace_bytes"), getattr(lib, name + "_batch_workspace_bytes")
        assert one(0, 4, 4, 10) == 0 and one(4, -1, 4, 10) == 0 and one(4, 4, 4, -1) == 0 and one(4, 4, 4, 2 ** 31) == 0 and one(2048, 1024, 1024, 1) == 0
        assert batch(0, 4, 4, 4, 10) == 0 and batch(64, 512, 256, 256, 10) == 0 and batch(63, 512, 256, 256, 10) > 0
        for P, b in ((1, 0), (1, 1), (1, 256), (1, 257), (5, 1028), (64, 64 * 60000)):
            chunks = b // 256 + P
            want = a256(8 * (2 * (P + 1) + 6 * P)) + a256(8 * chunks) + a256(12 * chunks)
            if icp:
                want += a256(48 * P) + a256(8 * P) + a256(8 * 28 * chunks)
            assert batch(P, 8, 8, 8, b) == want and (P != 1 or one(8, 8, 8, b) == want), (name, P, b)


GOOD = dict(P=2, nx=4, ny=4, nz=4, min_obs=1, b=8, max_iter=3, rel_thr=1e-6, min_matched=6)


def _call(lib, icp, single=False, origin=None, voxel=None, trunc=None, b_off=None, ws=True, ws_bytes=0, null=(), **kw):
    """the entries with made-up buffers: only for calls the host checks refuse before anything is dereferenced"""
    s = dict(GOOD, **kw)
    P = 1 if single else s["P"]
    ints, buf = (ctypes.c_int * 4096)(), (ctypes.c_double * 4096)()
    o = np.ascontiguousarray(np.zeros((max(P, 1), 3)) if origin is None else origin, np.float64)
    h = np.ascontiguousarray(np.full(max(P, 1), 0.01) if voxel is None else voxel, np.float64)
    tr = np.ascontiguousarray(np.full(max(P, 1), 0.04) if trunc is None else trunc, np.float64)
    bo = np.ascontiguousarray(np.linspace(0, s["b"], max(P, 1) + 1).astype(np.int64) if b_off is None else b_off, np.int64)
    p = {k: (None if k in null else (ints if k in ("sum", "n", "stop", "iters") else buf))
         for k in ("sum", "n", "B", "phi", "grad", "state", "counts", "sum_phi2", "g_out", "stop", "iters")}
    optr = None if "origin" in null else o.ctypes.data
    outs = (p["phi"], p["grad"], p["state"], p["counts"], p["sum_phi2"])
    tail = (buf if ws else None, ws_bytes, None)
    loop = (s["max_iter"], s["rel_thr"], s["min_matched"], p["g_out"], p["stop"], p["iters"]) if icp else ()
    trace = (None, None) if icp else ()
    name = "ls_tsdf_icp" if icp else "ls_tsdf_sample"
    if single:
        rc = getattr(lib, name + "_f32")(p["sum"], p["n"], s["nx"], s["ny"], s["nz"], s["min_obs"], optr, float(h[0]), float(tr[0]), p["B"], s["b"], None,
                                         *loop, *outs, *trace, *tail)
    else:
        rc = getattr(lib, name + "_batch_f32")(P, p["sum"], p["n"], s["nx"], s["ny"], s["nz"], s["min_obs"], optr, None if "voxel" in null else h.ctypes.data,
                                               tr.ctypes.data, p["B"], s["b"], None if "b_off" in null else bo.ctypes.data, None, *loop, *outs, *trace,
                                               *tail)
    return rc, lib.ls_last_error().decode()


def test_every_host_refusal():
    from livingscenes_amd import _lib
    lib = _lib.load()
    INVALID, WORKSPACE = -1, -3
    for icp in (False, True):
        for single in (False, True):
            name = ("tsdf_icp" if icp else "tsdf_sample") + ("" if single else "_batch")
            call = functools.partial(_call, lib, icp, single)
            last = 0 if single else 1
            for dims in (dict(nx=0), dict(ny=-1), dict(nz=0)):
                rc, msg = call(**dims)
                assert rc == INVALID and msg.startswith(name + ":") and "dims must be at least 1" in msg, msg
            rc, msg = call(nx=2048, ny=1024, nz=1024)
            assert rc == INVALID and "reaches 2^31" in msg, msg
            for bad in (0, -3):
                rc, msg = call(min_obs=bad)
                assert rc == INVALID and "min_obs must be >= 1" in msg, msg
            rc, msg = call(b=-1)
            assert rc == INVALID and "negative size" in msg, msg
            for bad in (0.0, -0.01, NAN, INF):
                rc, msg = call(voxel=[0.01, bad][-1:] if single else [0.01, bad])
                assert rc == INVALID and f"problem {last}" in msg and "voxel must be finite and > 0" in msg, (bad, msg)
                rc, msg = call(trunc=[0.04, bad][-1:] if single else [0.04, bad])
                assert rc == INVALID and f"problem {last}" in msg and "trunc must be finite and > 0" in msg, (bad, msg)
            rc, msg = call(voxel=[1e-300] * (last + 1), trunc=[1e300] * (last + 1))
            assert rc == INVALID and "problem 0" in msg and "trunc / voxel overflows" in msg, msg
            for bad in (NAN, INF, -INF):
                o = np.zeros((last + 1, 3))
                o[-1, 1] = bad
                rc, msg = call(origin=o)
                assert rc == INVALID and f"problem {last}" in msg and "origin must be finite" in msg, (bad, msg)
            for k in ("sum", "n"):
                rc, msg = call(null=(k,))
                assert rc == INVALID and "null sum / n" in msg, (k, msg)
            rc, msg = call(null=("origin",))
            assert rc == INVALID and "null origin / voxel / trunc" in msg, msg
            for k in ("B", "phi", "grad", "state"):
                rc, msg = call(null=(k,))
                assert rc == INVALID and "null B / phi / grad / state" in msg, (k, msg)
            for k in ("counts", "sum_phi2"):
                rc, msg = call(null=(k,))
                assert rc == INVALID and "null counts / sum_phi2" in msg, (k, msg)
            if icp:
                for kw, word in ((dict(max_iter=-1), "max_iter must be >= 0"), (dict(max_iter=2 ** 31 - 1), "do not fit an int"),
                                 (dict(rel_thr=-1.0), "rel_thr"), (dict(rel_thr=NAN), "rel_thr"), (dict(min_matched=2), "min_matched must be >= 3")):
                    rc, msg = call(**kw)
                    assert rc == INVALID and word in msg, (kw, msg)
                for k in ("g_out", "stop", "iters"):
                    rc, msg = call(null=(k,))
                    assert rc == INVALID and "null g_out / stop / iters" in msg, (k, msg)
            # the accepted extremes: only the workspace is short, and the error names the query
            rc, msg = call(voxel=[1e-300] * (last + 1), trunc=[1e-300] * (last + 1), min_obs=2 ** 31 - 1)
            assert rc == WORKSPACE and f"ls_{name}_workspace_bytes" in msg, msg
            rc, msg = call(ws=False, ws_bytes=1 << 30)
            assert rc == WORKSPACE, msg
            need = getattr(lib, f"ls_{name}_workspace_bytes")(*(() if single else (2,)), 4, 4, 4, 8)
            rc, msg = call(ws_bytes=need - 1)
            assert rc == WORKSPACE and f"{need - 1} < required {need}" in msg, msg
    for icp in (False, True):
        for P in (0, -1):
            rc, msg = _call(lib, icp, P=P)
            assert rc == INVALID and "P must be at least 1" in msg, msg
        rc, msg = _call(lib, icp, b_off=[0, 9, 8])
        assert rc == INVALID and "problem 1" in msg and "decreases" in msg, msg
        rc, msg = _call(lib, icp, b_off=[0, 3, 7])
        assert rc == INVALID and "disagrees with the total" in msg, msg
        rc, msg = _call(lib, icp, null=("b_off",))
        assert rc == INVALID and "null b_off" in msg, msg
        rc, msg = _call(lib, icp, null=("voxel",))
        assert rc == INVALID and "null origin / voxel / trunc" in msg, msg
