"""CPU-only tests (-m "not gpu") of the scene memory's depth fusion (include/livingscenes_hip.h: ls_depth_fuse_f32, ls_tsdf_volume_f64):
the hand cases of the definition; csrc/fuse_plan.h -- compiled on its own with the host compiler -- against
the NumPy twin (tests/fuse_oracle.py) per step and per class; the properties of the twin (order, splits, a plane, a sphere); and what the
C entry points decide on the host before any HIP call (the exported symbols, the workspace sizes, every refusal).  The shared generators
of tests/test_hip_depth_fuse.py (`fuse_problem`, `gpu_cases`) live here.  The kernels are held to the twin by equality there."""
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
import fuse_oracle as fo     # noqa: E402
import render_oracle as ro   # noqa: E402

NAMES = ("ls_depth_fuse_workspace_bytes", "ls_depth_fuse_f32", "ls_depth_fuse_batch_workspace_bytes", "ls_depth_fuse_batch_f32", "ls_tsdf_volume_f64")
F = np.float32
NAN, INF = float("nan"), float("inf")
EYE = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)

# the size edges of the kernel: voxel counts where a wave of 64 or a chunk of 256 is full, one short and one over
GPU_DIMS = ((1, 1, 1), (3, 3, 7), (4, 4, 4), (5, 13, 1), (3, 5, 17), (4, 8, 8), (257, 1, 1), (16, 16, 16), (17, 16, 16))
GPU_IMAGES = ((1, 1), (5, 7), (16, 16), (100, 100))       # (H, W)
GPU_VIEWS = (0, 1, 3)


# ------------------------------------------------------------------------------------------------ shared generators
def fuse_problem(rng, dims, V, H, W):
    """a grid of `dims` samples about one unit wide around the origin, V cameras that look at it from 0.35 .. 1.8 away (the first one
    always from 0.4: it stands inside or next to the grid, so voxels lie behind it or beside its image), depth images of a noisy sheet
    at the camera's distance with holes, negative, NaN and inf pixels -> dict(origin [3], voxel, trunc, depth [V,H,W] f32, K [V,4],
    E [V,3,4]).  f = 1.5 W: the image is narrower than the grid."""
    h = 1.0 / max(dims)
    origin = np.array([-h * (d - 1) / 2 for d in dims]) + rng.uniform(-0.01, 0.01, 3)
    E, dist = np.zeros((V, 3, 4)), np.zeros(V)
    for v in range(V):
        d = rng.standard_normal(3)
        dist[v] = rng.uniform(0.35, 0.45) if v == 0 else rng.uniform(0.4, 1.8)   # the first stands in or at the grid: voxels beside and behind it
        E[v] = ro.world_to_cam(ro.look_at_pose(dist[v] * d / np.linalg.norm(d)))
    K = np.tile([1.5 * W, 1.5 * W, (W - 1) / 2.0, (H - 1) / 2.0], (V, 1)) + rng.uniform(-0.3, 0.3, (V, 4))
    depth = (dist[:, None, None] + 0.25 * rng.standard_normal((V, H, W))).astype(F)
    hole = rng.random((V, H, W))
    depth[hole < 0.15] = 0.0
    depth[(hole > 0.15) & (hole < 0.17)] = -1.0
    depth[(hole > 0.17) & (hole < 0.18)] = NAN
    depth[(hole > 0.18) & (hole < 0.19)] = INF
    return dict(origin=origin, voxel=h, trunc=0.12, depth=depth, K=K, E=E)


def reaches_every_class(dims, V, H, W, vc):
    """what the size-edge problems are chosen for: from 255 voxels up and with a view, a non-zero count in every class but SATURATED.
    The one thing that is impossible: ONE view of a 1 x 1 image has one depth, so it cannot be both EMPTY and not; there the pixel is
    chosen to hold a depth, and OUT, OCCLUDED, NEAR and FREE are all asked for.  Three views of 1 x 1 reach every class like any image."""
    if V == 0 or np.prod(dims) < 255:
        return True
    tot = vc.sum(0)
    want = [fo.OUT, fo.OCCLUDED, fo.NEAR, fo.FREE] if (H, W, V) == (1, 1, 1) else [fo.OUT, fo.EMPTY, fo.OCCLUDED, fo.NEAR, fo.FREE]
    return bool((tot[want] > 0).all() and tot[fo.SATURATED] == 0)


@functools.lru_cache(maxsize=None)
def gpu_cases(dims):
    """the problems of one grid size in tests/test_hip_depth_fuse.py: (V, (H, W), problem), seeded by the sizes alone.  A line of voxels
    meets few pixels of a small image, so a draw can miss a class: the first draw of (sizes, salt), salt = 0, 1, ..., that
    reaches_every_class under the twin is the problem."""
    out = []
    for V in GPU_VIEWS:
        for H, W in GPU_IMAGES:
            for salt in range(1024):
                rng = np.random.Generator(np.random.Philox(key=[dims[0] * 10000 + dims[1] * 100 + dims[2], (V * 1000 + H * 10 + W % 10) * 1024 + salt]))
                pr = fuse_problem(rng, dims, V, H, W)
                if reaches_every_class(dims, V, H, W, run_twin(dims, pr)[1]):
                    break
            else:
                raise AssertionError(f"no draw of {dims}, {V} views, {H} x {W} reaches every class")
            out.append((V, (H, W), pr))
    return out


def run_twin(dims, pr, empty="unknown", state=None):
    state = fo.new_state(dims) if state is None else state
    vc = fo.fuse(state, pr["depth"], pr["K"], pr["E"], pr["origin"], pr["voxel"], pr["trunc"], empty)
    return state, vc


# ------------------------------------------------------------------------------------------------ the hand cases
def _one_voxel(x, depth, empty="unknown", trunc=0.04, znear=0.05, K=(4.0, 4.0, 2.0, 2.0)):
    """one voxel at x under the identity camera and one view -> (class, sum, n)"""
    state = fo.new_state((1, 1, 1))
    vc = fo.fuse(state, depth[None], np.array([K]), EYE[None], np.array(x, np.float64), 1.0, trunc, empty, znear)
    assert vc.sum() == 1
    return int(np.flatnonzero(vc[0])[0]), int(state[0][0, 0, 0]), int(state[1][0, 0, 0])


def test_hand_cases_worked_out_by_hand():
    """identity camera, a constant depth image d = 1.0 (5 x 5, f = 4, c = 2: the axis meets pixel (2, 2)), trunc = 0.04"""
    one = np.ones((5, 5), F)
    for z, cls, q in ((0.90, fo.FREE, 16384), (0.99, fo.NEAR, 4096), (1.00, fo.NEAR, 0), (1.03, fo.NEAR, -12288)):
        for empty in ("unknown", "free"):
            assert _one_voxel((0, 0, z), one, empty) == (cls, q, 1), (z, empty)
    assert _one_voxel((0, 0, 1.05), one) == (fo.OCCLUDED, 0, 0)
    assert _one_voxel((0, 0, 0.04), one) == (fo.OUT, 0, 0)                       # behind znear = 0.05
    assert _one_voxel((0, 0, -1.0), one) == (fo.OUT, 0, 0)                       # behind the camera
    assert _one_voxel((0, 0, 0.05), one)[0] == fo.FREE                           # c.z == znear stays in
    assert _one_voxel((1.0, 0, 1.0), one) == (fo.OUT, 0, 0)                      # u = 6: outside the 5-pixel image
    assert _one_voxel((-0.625, 0, 1.0), one)[0] == fo.NEAR                       # u = -0.5 exactly: qx = 0
    assert _one_voxel((0.625, 0, 1.0), one) == (fo.OUT, 0, 0)                    # u = 4.5 exactly: qx = 5 = W
    assert _one_voxel((NAN, 0, 1.0), one) == (fo.OUT, 0, 0)
    for bad in (0.0, -1.0, NAN):                                                 # a pixel that hit nothing, under both modes
        hole = one.copy()
        hole[2, 2] = bad
        assert _one_voxel((0, 0, 0.99), hole, "unknown") == (fo.EMPTY, 0, 0), bad
        assert _one_voxel((0, 0, 0.99), hole, "free") == (fo.FREE, 16384, 1), bad
        assert _one_voxel((0, 0, 1.5), hole, "free") == (fo.FREE, 16384, 1), bad   # no depth to be occluded by
    far = one.copy()
    far[2, 2] = INF
    assert _one_voxel((0, 0, 0.99), far) == (fo.FREE, 16384, 1)
    # s == trunc is NEAR with t = 1, s == -trunc is taken with t = -1, one ulp further is occluded (representable: d = 1, trunc = 0.25)
    assert _one_voxel((0, 0, 0.75), one, trunc=0.25) == (fo.NEAR, 16384, 1)
    assert _one_voxel((0, 0, np.nextafter(0.75, 0)), one, trunc=0.25) == (fo.FREE, 16384, 1)
    assert _one_voxel((0, 0, 1.25), one, trunc=0.25) == (fo.NEAR, -16384, 1)
    assert _one_voxel((0, 0, np.nextafter(1.25, 2)), one, trunc=0.25) == (fo.OCCLUDED, 0, 0)


def test_saturation_and_volume_of_the_twin():
    one = np.ones((3, 5, 5), F)
    K, E = np.tile([4.0, 4.0, 2.0, 2.0], (3, 1)), np.tile(EYE, (3, 1, 1))
    for n0, want_n, want_counts in ((65534, 65535, [fo.NEAR, fo.SATURATED, fo.SATURATED]), (65535, 65535, [fo.SATURATED] * 3), (0, 3, [fo.NEAR] * 3)):
        state = (np.full((1, 1, 1), 7, np.int32), np.full((1, 1, 1), n0, np.int32))
        vc = fo.fuse(state, one, K, E, np.array([0, 0, 0.99]), 1.0, 0.04)
        assert state[1][0, 0, 0] == want_n and state[0][0, 0, 0] == 7 + 4096 * (want_n - n0)
        assert [int(np.flatnonzero(r)[0]) for r in vc] == want_counts
    S = np.array([[[0, 4096, -8192, 5, 16384 * 3]]], np.int32)
    N = np.array([[[0, 1, 2, 1, 3]]], np.int32)
    D, valid, counts = fo.volume((S, N), 1)
    assert D.tolist() == [[[1.0, 0.25, -0.25, 5 / 16384, 1.0]]] and valid.tolist() == [[[False, True, True, True, True]]] and counts.tolist() == [4, 1, 1]
    D, valid, counts = fo.volume((S, N), 2)
    assert D.tolist() == [[[1.0, 1.0, -0.25, 1.0, 1.0]]] and valid.sum() == 2 and counts.tolist() == [2, 1, 1]


# ------------------------------------------------------------------------------------------------ fuse_plan.h against the twin
@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fuse_plan") / "fuse_plan_dump")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", "-I",
                    os.path.join(REPO, "livingscenes_amd", "csrc"), os.path.join(HERE, "tools", "fuse_plan_dump.cpp"), "-o", exe], check=True)

    def run(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(lines)
        return [line.split() for line in out]
    return run


def _hex(values):
    return " ".join(float(t).hex() for t in np.asarray(values, np.float64).reshape(-1))


def test_fuse_plan_header_equals_the_twin(plan):
    assert [int(t) for t in plan(["constants"])[0]] == [fo.OUT, fo.EMPTY, fo.OCCLUDED, fo.NEAR, fo.FREE, fo.SATURATED, 256, fo.SCALE, fo.MAX_OBS, 5]
    rng = np.random.Generator(np.random.Philox(key=[31, 5]))
    # step 1: the positions
    lines, want = [], []
    for _ in range(200):
        o, h, i = rng.uniform(-2, 2), rng.uniform(1e-3, 0.1), int(rng.integers(0, 500))
        lines.append(f"pos {float(o).hex()} {float(h).hex()} {i}")
        want.append(float(np.float64(o) + np.float64(h) * np.float64(i)))
    assert [float.fromhex(g[0]) for g in plan(lines)] == want
    # steps 1 - 6 per voxel and view, both modes
    lines, want = [], []
    for dims, (H, W) in (((3, 3, 7), (5, 7)), ((4, 4, 4), (1, 1)), ((5, 13, 1), (16, 16)), ((6, 6, 6), (3, 3))):
        pr = fuse_problem(rng, dims, 3, H, W)
        x = fo.positions(dims, pr["origin"], pr["voxel"])
        X = np.stack([a.reshape(-1) for a in x], 1)
        for v in range(3):
            for eif in (0, 1):
                cls, q = fo.view_classes(x, pr["depth"][v], pr["K"][v], pr["E"][v], pr["trunc"], bool(eif))
                head = f"view {W} {H} {eif} {float(pr['trunc']).hex()} {float(0.05).hex()} {_hex(pr['E'][v])} {_hex(pr['K'][v])}"
                img = _hex(pr["depth"][v])
                lines += [f"{head} {_hex(p)} {img}" for p in X]
                want += list(zip(cls.reshape(-1).tolist(), q.reshape(-1).tolist()))
    got = [(int(g[0]), int(g[1])) for g in plan(lines)]
    wrong = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not wrong, wrong[:5]
    hist = np.bincount([w[0] for w in want], minlength=6)
    print(f"{len(want)} (voxel, view) cases, classes {hist.tolist()}")
    assert (hist[:5] >= 20).all() and hist[5] == 0, "a class the cases hardly reach"
    # steps 4 - 6 alone, around the edges of the band
    lines, want = [], []
    for d in (1.0, 0.0, -1.0, NAN, INF, 0.5):
        for z in (0.75, np.nextafter(0.75, 0), 1.25, np.nextafter(1.25, 2), 1.0, 0.9, 1.1, 0.3):
            for eif in (0, 1):
                lines.append(f"dist {float(d).hex() if np.isfinite(d) else d} {float(z).hex()} {float(0.25).hex()} {eif}")
                dd = np.float64(F(d))
                if not dd > 0:
                    want.append((fo.FREE, fo.SCALE) if eif else (fo.EMPTY, 0))
                else:
                    s = dd - z
                    want.append((fo.OCCLUDED, 0) if s < -0.25 else (fo.NEAR if s <= 0.25 else fo.FREE, int(np.floor(min(s, 0.25) / 0.25 * 16384 + 0.5))))
    assert [(int(g[0]), int(g[1])) for g in plan(lines)] == want


def test_fuse_plan_update_value_and_checks(plan):
    cases = [(c, q, s, n) for c in range(5) for q in (-16384, 0, 77) for s in (0, -5) for n in (0, 1, 65534, 65535)]
    want = []
    for c, q, s, n in cases:
        if c not in (fo.NEAR, fo.FREE):
            want.append([c, s, n])
        elif n == 65535:
            want.append([fo.SATURATED, s, n])
        else:
            want.append([c, s + q, n + 1])
    assert [[int(t) for t in g] for g in plan([f"update {c} {q} {s} {n}" for c, q, s, n in cases])] == want
    cases = [(s, n, m) for s in (0, 1, -16384, 12345, -(2 ** 30) + 1, 2 ** 30 - 1) for n in (0, 1, 2, 3, 65535) for m in (1, 2, 3)]
    got = plan([f"value {s} {n} {m}" for s, n, m in cases])
    for (s, n, m), g in zip(cases, got):
        D, valid, _ = fo.volume((np.array([[[s]]], np.int32), np.array([[[n]]], np.int32)), m)
        assert int(g[0]) == int(valid[0, 0, 0]) and float.fromhex(g[1]) == D[0, 0, 0], (s, n, m, g)
        if not valid[0, 0, 0]:
            assert float.fromhex(g[1]).hex() == (1.0).hex()
    sizes = [((1, 1, 1, 1), 1), ((0, 4, 4, 4), 0), ((1, 0, 4, 4), 0), ((1, 4, -1, 4), 0), ((1, 4, 4, 0), 0), ((1, 1290, 1290, 1290), 1),
             ((1, 1291, 1291, 1291), 0), ((8, 640, 640, 640), 1), ((8, 645, 645, 645), 1), ((8, 646, 646, 646), 0), ((64, 64, 64, 64), 1),
             ((2 ** 31 - 1, 1, 1, 1), 1), ((2 ** 31 - 1, 2, 1, 1), 0), ((1, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1), 0), ((2, 2 ** 30, 1, 1), 0),
             ((1, 2 ** 30, 1, 1), 1)]
    assert [int(g[0]) for g in plan([f"sizes {a} {b} {c} {d}" for (a, b, c, d), _ in sizes])] == [w for _, w in sizes]
    for (P, nx, ny, nz), w in sizes:
        assert w == int(min(P, nx, ny, nz) >= 1 and P * nx * ny * nz < 2 ** 31)
    good = [0.1, -0.2, 0.3, 0.01, 0.04]
    lines, want = [f"grid {_hex(good)}"], [0]
    for field, idx, bads in ((1, (0, 1, 2), (NAN, INF, -INF)), (2, (3,), (0.0, -0.01, NAN, INF)), (3, (4,), (0.0, -1.0, NAN, INF, -INF))):
        for i in idx:
            for b in bads:
                a = list(good)
                a[i] = b
                lines.append("grid " + " ".join(float(t).hex() if np.isfinite(t) else str(t) for t in a))
                want.append(field)
    lines += [f"grid {_hex([1e300, -1e300, 0.0, 1e-300, 1e300])}"]
    want += [0]
    assert [int(g[0]) for g in plan(lines)] == want
    assert [int(g[0]) for g in plan([f"scalars {float(0.05).hex()} 0", f"scalars {float(1e-300).hex()} 1", "scalars 0x0p+0 0", "scalars -0x1p+0 0",
                                     "scalars nan 0", "scalars inf 1", f"scalars {float(0.05).hex()} 2", f"scalars {float(0.05).hex()} -1"])] == \
        [0, 0, 1, 1, 1, 1, 2, 2]
    assert [[int(t) for t in g] for g in plan(["pieces 1", "pieces 5", "pieces 64"])] == [[2, 5], [6, 25], [65, 320]]


# ------------------------------------------------------------------------------------------------ properties of the twin
def test_gpu_cases_reach_every_class():
    """From 255 voxels up, every random problem of tests/test_hip_depth_fuse.py that has a view puts a non-zero count in every class but
    SATURATED (empty pixels skipped; ONE view of a 1 x 1 image cannot be EMPTY as well: see reaches_every_class).  Printed: the totals per grid size."""
    for dims in GPU_DIMS:
        total = np.zeros(6, np.int64)
        for V, (H, W), pr in gpu_cases(dims):
            _, vc = run_twin(dims, pr)
            assert vc.shape == (V, 6) and (vc.sum(1) == np.prod(dims)).all()
            _, vf = run_twin(dims, pr, "free")
            assert not vf[:, fo.EMPTY].any() and np.array_equal(vf[:, fo.FREE], vc[:, fo.FREE] + vc[:, fo.EMPTY])
            total += vc.sum(0)
            if V and np.prod(dims) >= 255:
                tot = vc.sum(0)
                must = [fo.OUT, fo.OCCLUDED, fo.NEAR, fo.FREE] if (H, W, V) == (1, 1, 1) else [fo.OUT, fo.EMPTY, fo.OCCLUDED, fo.NEAR, fo.FREE]
                assert (tot[must] > 0).all() and tot[fo.SATURATED] == 0, (dims, V, H, W, tot)
        print(dims, total.tolist())


def test_order_and_splits_do_not_change_the_state():
    rng = np.random.Generator(np.random.Philox(key=[2, 9]))
    dims = (6, 7, 8)
    pr = fuse_problem(rng, dims, 5, 16, 16)
    for empty in ("unknown", "free"):
        (S, N), vc = run_twin(dims, pr, empty)
        assert N.max() >= 3 and (S != 0).any()
        for perm in ([4, 3, 2, 1, 0], [2, 0, 4, 1, 3]):
            q = dict(pr, depth=pr["depth"][perm], K=pr["K"][perm], E=pr["E"][perm])
            (S2, N2), vc2 = run_twin(dims, q, empty)
            assert np.array_equal(S, S2) and np.array_equal(N, N2) and np.array_equal(vc2, vc[perm])
        for cut in (0, 1, 2, 5):
            state = fo.new_state(dims)
            parts = [run_twin(dims, dict(pr, depth=pr["depth"][a:b], K=pr["K"][a:b], E=pr["E"][a:b]), empty, state)[1] for a, b in ((0, cut), (cut, 5))]
            assert np.array_equal(S, state[0]) and np.array_equal(N, state[1]) and np.array_equal(np.concatenate(parts), vc)


def test_a_plane_is_met_within_the_rounding_of_q():
    """A fronto-parallel plane z = d0 (a constant depth image under the identity camera) and voxel columns along the optical axis.  In
    the band t = (d0 - z) / trunc is linear in z; the state keeps q = round(16384 t), so D = t + e with |e| <= 1 / 32768: a distance
    error of eps = trunc / 32768.  Marching cubes puts the vertex of an edge (z1, z2 = z1 + h) at z1 + h D1 / (D1 - D2); with
    a = t1 / (t1 - t2) in [0, 1] and t1 - t2 = h / trunc its error is h ((1 - a) e1 + a e2) / (h / trunc + e1 - e2), at most
    eps / (1 - 2 trunc / (32768 h)) = 1.0003 eps at trunc = 4 h -- below the DERIVED bound 2 eps, which also covers the float64 rounding
    of z and s (1e-16).  D does not depend on x and y, so only edges along z are crossed.  The test grants twice the derived bound:
    trunc / 8192.  One view, and three views of the same plane (the average of equal values)."""
    dims, h, d0 = (5, 4, 24), 0.01, 1.0037
    trunc, origin = 4 * h, np.array([-0.02, -0.015, 0.9])
    K = np.array([[60.0, 60.0, 49.5, 49.5]])
    for V in (1, 3):
        state = fo.new_state(dims)
        vc = fo.fuse(state, np.full((V, 100, 100), d0, F), np.tile(K, (V, 1)), np.tile(EYE, (V, 1, 1)), origin, h, trunc)
        assert not vc[:, fo.OUT].any() and vc[:, fo.NEAR].all() and vc[:, fo.FREE].all() and vc[:, fo.OCCLUDED].all()
        verts, faces = fo.mesh(state, origin, h)
        raw, _ = fo.mesh(state, origin, h, do_compact=False)
        err = np.abs(verts[:, 2] - np.float64(F(d0))).max()
        print(f"plane, {V} view(s): {len(verts)} vertices, {len(faces)} faces, max |z - d0| = {err:.3e}, eps = {trunc / 32768:.3e}")
        assert len(faces) == 2 * (dims[0] - 1) * (dims[1] - 1) and len(verts) >= dims[0] * dims[1]   # one layer of cubes, two triangles each
        assert len(raw) > len(verts)              # unmasked, the band's far end (D = -1 next to +1) makes vertices too: the mask drops their faces
        assert err <= trunc / 8192
        assert err <= 2 * trunc / 32768, "the twin alone misses the derived bound"


def _rot(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _look_at(R):
    t = -1.5 * R[:, 2]
    return np.concatenate([R.T, (-R.T @ t)[:, None]], 1)


def _sphere_depth(E, K, H, W, r):
    """the analytic z-depth of a sphere of radius r at the origin, 0 where the ray misses it"""
    fx, fy, cx, cy = K
    py, px = np.mgrid[0:H, 0:W]
    d = np.stack([(px - cx) / fx, (py - cy) / fy, np.ones((H, W))], -1)
    R, t = E[:, :3], E[:, 3]
    o, dw = -R.T @ t, d @ R
    a, b, c = (dw * dw).sum(-1), 2 * (dw @ o), o @ o - r * r
    disc = b * b - 4 * a * c
    return np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), 0.0).astype(F)


@functools.lru_cache(maxsize=None)
def sphere_state(views=4, res=40, r=0.4):
    """a CPU experiment on the twin alone (the library has no masked marching cubes yet: the twin shows why one is needed): analytic depth maps of a sphere, 100 x 100, f = 100, cameras at 1.5, h = 1 / (res - 1), trunc = 4 h"""
    rng = np.random.default_rng(0)
    _rot(rng)                                                                    # the experiment's one-view round comes first
    h, origin = 1.0 / (res - 1), np.array([-0.5] * 3)
    K = np.array([100.0, 100.0, 50.0, 50.0])
    E = np.stack([_look_at(_rot(rng)) for _ in range(views)])
    depth = np.stack([_sphere_depth(e, K, 100, 100, r) for e in E])
    state = fo.new_state((res,) * 3)
    fo.fuse(state, depth, np.tile(K, (views, 1)), E, origin, h, 4 * h)
    return state, origin, h


def test_the_sphere_needs_the_mask():
    """Masked, every referenced vertex lies within sqrt(3) h of the sphere (a cube's diagonal: the surface crosses every cube that emits
    a face; 0.95 h observed).  Unmasked -- unobserved samples read +1 -- a second shell appears where the truncation band ends: at least
    one vertex lies farther than trunc - h from the sphere."""
    (S, N), origin, h = sphere_state()
    r, trunc = 0.4, 4 * h
    verts, faces = fo.mesh((S, N), origin, h)
    D, valid, counts = fo.volume((S, N))
    uv, uf = fo.masked_marching_cubes(D, None)
    uv = (uv - 0.5) * h + origin
    err = np.abs(np.linalg.norm(verts, axis=1) - r)
    uerr = np.abs(np.linalg.norm(uv[np.unique(uf)], axis=1) - r)
    print(f"sphere, 4 views: observed {counts[0] / N.size:.3f}; masked {len(faces)} faces, max error {err.max():.4f} ({err.max() / h:.2f} h), rms "
          f"{np.sqrt((err ** 2).mean()):.4f}; unmasked {len(uf)} faces, max error {uerr.max():.4f} (trunc {trunc:.4f})")
    assert len(faces) > 1000 and len(uf) > len(faces)
    assert err.max() <= np.sqrt(3) * h
    assert uerr.max() > trunc - h
    # the masked faces are a subsequence of the unmasked ones and every vertex is created either way
    raw_v, raw_f = fo.masked_marching_cubes(D, valid)
    assert len(raw_v) == len(uv) and len(raw_f) == len(faces)
    keep = np.repeat(fo.cube_ok(valid), fo.triangles_per_cube(D, 0.0))
    assert np.array_equal(raw_f, uf[keep])


def test_fusion_grid_of_the_twin():
    cloud = np.array([[0.0, 0.0, 0.0], [1.0, 0.5, 0.25]])
    origin, h, trunc = fo.fusion_grid(cloud, 19, 4)
    assert h == 0.1 and trunc == 0.4 and np.allclose(origin, [0.5 - 0.9, 0.25 - 0.9, 0.125 - 0.9], atol=1e-15)
    assert origin[0] + 4 * h <= 0.0 + 1e-15 and origin[0] + 14 * h >= 1.0 - 1e-15          # the box keeps its band inside
    with pytest.raises(ValueError):
        fo.fusion_grid(cloud, 9, 4)


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
    assert len(_lib.SIGNATURES["ls_depth_fuse_f32"][1]) == 20 and len(_lib.SIGNATURES["ls_depth_fuse_batch_f32"][1]) == 22
    assert len(_lib.SIGNATURES["ls_tsdf_volume_f64"][1]) == 11
    assert int(lib.ls_version()) == _lib.ABI_VERSION == 107 and "#define LS_ABI_VERSION 107" in header
    assert "ls_depth_fuse_f32 / ls_depth_fuse_batch_f32" in header.split("#define LS_ABI_VERSION")[0]
    for text in ("x_a = origin_a + h * (double)i_a", "s = d - c.z", "q = (int) floor(t * 16384 + 0.5)", "SATURATED, and skipped, if n == 65535",
                 "THE UPDATE IS INTEGER", "EXACTLY +1.0", "1 memset (view_counts)"):
        assert text in header, text
    assert "depthfuse.hip" in build.SOURCES and build.PACKED_FP32_GUARD["depthfuse.hip"] == []
    plan_h = open(os.path.join(REPO, "livingscenes_amd", "csrc", "fuse_plan.h")).read()
    assert "#include <hip" not in plan_h and '#include "ls_' not in plan_h and "carve_pixel" in plan_h and "contract(off)" in plan_h
    for f in (ops.depth_fuse, ops.depth_fuse_batch):
        sig = inspect.signature(f).parameters
        assert list(sig)[:4] == ["state", "depth" if f is ops.depth_fuse else "depths", "intrinsics", "world_to_cam"]
        for k in ("origin", "voxel", "trunc"):
            assert sig[k].default is inspect.Parameter.empty and sig[k].kind is inspect.Parameter.KEYWORD_ONLY
        assert [sig[k].default for k in ("empty", "znear")] == ["unknown", 0.05]
    assert ops.FUSE_CLASS == ("out", "empty", "occluded", "near", "free", "saturated")
    assert inspect.signature(ops.tsdf_volume).parameters["min_obs"].default == 1
    sig = inspect.signature(More_Solver._fuse_batch).parameters
    assert list(sig)[1:5] == ["fusion", "views", "T", "g"] and [sig[k].default for k in ("empty", "znear")] == ["unknown", 0.05]
    assert inspect.signature(More_Solver._fusion_grids).parameters["trunc_voxels"].default == 4
    sig = inspect.signature(solve_sequence).parameters
    assert [sig[k].default for k in ("fuse_res", "fuse_trunc_voxels", "fuse_empty")] == [None, 4, "unknown"]
    assert "UNMEASURED" in solve_sequence.__doc__ and "NO fuse_res IS RECOMMENDED" in solve_sequence.__doc__


def test_fusion_grids_on_the_host():
    import torch
    from livingscenes_amd.lib_more.more_solver import More_Solver
    rng = np.random.default_rng(3)
    clouds = [rng.uniform(-0.4, 0.6, (50, 3)).astype(F) * s for s in (1.0, 0.3)]
    for res, tv in ((16, 4), (10, 4), (40, 2)):
        g = More_Solver._fusion_grids([torch.from_numpy(c) for c in clouds], res, tv)
        assert g["dims"] == (res,) * 3 and g["origin"].dtype == g["voxel"].dtype == g["trunc"].dtype == torch.float64
        for p, c in enumerate(clouds):
            origin, h, trunc = fo.fusion_grid(c, res, tv)
            assert np.array_equal(g["origin"][p].numpy(), origin) and float(g["voxel"][p]) == h and float(g["trunc"][p]) == trunc
            lo, hi = c.astype(np.float64).min(0), c.astype(np.float64).max(0)
            assert (origin + trunc <= lo + 1e-12).all() and (origin + h * (res - 1) - trunc >= hi - 1e-12).all()   # the band stays inside
    for res, tv in ((9, 4), (3, 1), (16, 0)):
        with pytest.raises(ValueError, match="res must be at least"):
            More_Solver._fusion_grids([torch.from_numpy(clouds[0])], res, tv)


def test_workspace_sizes():
    from livingscenes_amd import _lib
    lib = _lib.load()
    one, batch = lib.ls_depth_fuse_workspace_bytes, lib.ls_depth_fuse_batch_workspace_bytes
    assert one(0, 4, 4, 1) == 0 and one(4, 0, 4, 1) == 0 and one(4, 4, -1, 1) == 0 and one(4, 4, 4, -1) == 0 and one(4, 4, 4, 2 ** 31) == 0
    assert one(1291, 1291, 1291, 1) == 0 and one(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 1) == 0
    assert batch(0, 4, 4, 4, 1) == 0 and batch(-1, 4, 4, 4, 1) == 0 and batch(8, 646, 646, 646, 1) == 0 and batch(2, 4, 4, 4, -1) == 0
    assert one(1, 1, 1, 0) > 0 and one(1290, 1290, 1290, 2 ** 31 - 1) > 0 and batch(8, 645, 645, 645, 0) > 0
    for dims in ((1, 1, 1), (4, 8, 8), (64, 64, 64), (17, 16, 16)):
        for views in (0, 1, 8, 1000):
            assert one(*dims, views) == one(1, 1, 1, 0) == batch(1, *dims, views)       # the state and the views are read where they lie
            for P in (1, 5, 64, 4096):
                got = batch(P, *dims, views)
                assert got % 256 == 0 and 8 * (6 * P + 1) <= got < 8 * (6 * P + 1) + 256
    sizes = [batch(P, 16, 16, 16, 8) for P in (1, 2, 64, 4096)]
    assert sizes == sorted(sizes) and sizes[-1] > sizes[0]


GOOD = dict(nx=4, ny=4, nz=4, origin=(0.0, 0.0, 0.0), voxel=0.01, trunc=0.04, views=2, H=4, W=4, znear=0.05, empty_is_free=0)


def _bufs():
    return (ctypes.c_int * 4096)(), (ctypes.c_float * 4096)()


def _one(lib, ws=True, ws_bytes=0, null=(), **kw):
    """the single entry with made-up buffers: only for calls the host checks refuse before anything is dereferenced"""
    s = dict(GOOD, **kw)
    state, buf = _bufs()
    b = {k: (None if k in null else buf) for k in ("depth", "K", "E", "view_counts")}
    b.update({k: (None if k in null else state) for k in ("sum", "n")})
    o = None if "origin" in null else np.asarray(s["origin"], np.float64).ctypes.data
    rc = lib.ls_depth_fuse_f32(b["sum"], b["n"], s["nx"], s["ny"], s["nz"], o, s["voxel"], s["trunc"], b["depth"], s["views"], s["H"], s["W"],
                               b["K"], b["E"], s["znear"], s["empty_is_free"], b["view_counts"], buf if ws else None, ws_bytes, None)
    return rc, lib.ls_last_error().decode()


def _batch(lib, P=2, view_off=(0, 1, 2), origin=None, voxel=None, trunc=None, ws_bytes=0, **kw):
    s = dict(GOOD, **kw)
    state, buf = _bufs()
    o = np.ascontiguousarray(np.zeros((max(P, 1), 3)) if origin is None else origin, np.float64)
    h = np.ascontiguousarray(np.full(max(P, 1), 0.01) if voxel is None else voxel, np.float64)
    t = np.ascontiguousarray(np.full(max(P, 1), 0.04) if trunc is None else trunc, np.float64)
    vo = np.asarray(view_off, np.int64)
    rc = lib.ls_depth_fuse_batch_f32(P, state, state, s["nx"], s["ny"], s["nz"], o.ctypes.data, h.ctypes.data, t.ctypes.data, buf, s["views"],
                                     vo.ctypes.data, s["H"], s["W"], buf, buf, s["znear"], s["empty_is_free"], buf, buf, ws_bytes, None)
    return rc, lib.ls_last_error().decode()


def test_every_host_refusal():
    from livingscenes_amd import _lib
    lib = _lib.load()
    INVALID, WORKSPACE = -1, -3
    for call, name in ((lambda **kw: _batch(lib, **kw), "depth_fuse_batch"), (lambda **kw: _one(lib, **kw), "depth_fuse")):
        for bad in (0.0, -0.5, NAN, INF):
            rc, msg = call(znear=bad)
            assert rc == INVALID and name in msg and "znear must be finite and > 0" in msg, (bad, msg)
        for bad in (2, -1):
            rc, msg = call(empty_is_free=bad)
            assert rc == INVALID and "empty_is_free must be 0 or 1" in msg, (bad, msg)
        for H, W in ((0, 4), (4, 0), (-1, 4)):
            rc, msg = call(H=H, W=W)
            assert rc == INVALID and "at least one pixel" in msg, msg
        for dims in (dict(nx=0), dict(ny=-1), dict(nz=0)):
            rc, msg = call(**dims)
            assert rc == INVALID and "dims must be at least 1" in msg, msg
        rc, msg = call(nx=1291, ny=1291, nz=1291)
        assert rc == INVALID and "reaches 2^31" in msg, msg
        rc, msg = call(znear=1e-300, empty_is_free=1)                  # the accepted extremes: only the workspace is short
        assert rc == WORKSPACE and "workspace" in msg and f"ls_{name}_workspace_bytes" in msg, msg
    # the grid, per problem: the error names it
    for field, text, bads in (("voxel", "voxel must be finite and > 0", (0.0, -0.01, NAN, INF)), ("trunc", "trunc must be finite and > 0", (0.0, -1.0, NAN, INF))):
        for bad in bads:
            rc, msg = _batch(lib, **{field: [0.01, bad]})
            assert rc == INVALID and "problem 1" in msg and text in msg, (bad, msg)
            rc, msg = _one(lib, **{field: bad})
            assert rc == INVALID and "problem 0" in msg and text in msg, (bad, msg)
    for bad in (NAN, INF, -INF):
        o = np.zeros((2, 3))
        o[1, 2] = bad
        rc, msg = _batch(lib, origin=o)
        assert rc == INVALID and "problem 1" in msg and "origin must be finite" in msg, (bad, msg)
        rc, msg = _one(lib, origin=(0.0, bad, 0.0))
        assert rc == INVALID and "origin must be finite" in msg, (bad, msg)
    rc, msg = _batch(lib, P=3, view_off=[0, 2, 1, 2])
    assert rc == INVALID and "problem 1" in msg and "view_off" in msg and "decreases" in msg, msg
    rc, msg = _batch(lib, P=2, view_off=[0, 1, 3])
    assert rc == INVALID and "view_off" in msg and "ends at 3" in msg, msg
    rc, msg = _batch(lib, P=2, view_off=[1, 1, 2])
    assert rc == INVALID and "view_off[0]" in msg, msg
    rc, msg = _batch(lib, P=0, view_off=[0])
    assert rc == INVALID and "P must be" in msg, msg
    rc, msg = _batch(lib, P=8, nx=646, ny=646, nz=646, view_off=[0] * 8 + [2])
    assert rc == INVALID and "reaches 2^31" in msg, msg
    rc, msg = _one(lib, views=-1)
    assert rc == INVALID and "negative" in msg, msg
    rc, msg = _one(lib, views=2 ** 31)
    assert rc == INVALID and "views exceed" in msg, msg
    for k in ("sum", "n"):
        rc, msg = _one(lib, null=(k,))
        assert rc == INVALID and "null sum / n" in msg, (k, msg)
    rc, msg = _one(lib, null=("origin",))
    assert rc == INVALID and "null origin / voxel / trunc" in msg, msg
    for k in ("depth", "K", "E", "view_counts"):
        rc, msg = _one(lib, null=(k,))
        assert rc == INVALID and "null depth / intrinsics / world_to_cam / view_counts" in msg, (k, msg)
    rc, msg = _one(lib, views=0, null=("depth", "K", "E", "view_counts"))       # no views: their arrays may be null, only the workspace is short
    assert rc == WORKSPACE, msg
    rc, msg = _one(lib, ws=False, ws_bytes=1 << 20)
    assert rc == WORKSPACE, msg
    rc, msg = _batch(lib, ws_bytes=lib.ls_depth_fuse_batch_workspace_bytes(2, 4, 4, 4, 2) - 1)
    assert rc == WORKSPACE and "workspace" in msg, msg
    # the volume
    state, buf = _bufs()
    vol = lib.ls_tsdf_volume_f64
    for args, text in (((0, 4, 4, 4, 1), "B must be at least 1"), ((1, 0, 4, 4, 1), "dims must be at least 1"), ((1, 4, 4, 4, 0), "min_obs must be >= 1"),
                       ((1, 4, 4, 4, -2), "min_obs must be >= 1"), ((8, 646, 646, 646, 1), "reaches 2^31")):
        assert vol(state, state, *args, buf, buf, buf, None) == INVALID and text in lib.ls_last_error().decode(), args
    for k in range(5):
        ptrs = [state, state, buf, buf, buf]
        ptrs[k] = None
        assert vol(ptrs[0], ptrs[1], 1, 4, 4, 4, 1, ptrs[2], ptrs[3], ptrs[4], None) == INVALID and "null sum / n / volume_out" in lib.ls_last_error().decode()
