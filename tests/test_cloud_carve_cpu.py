"""CPU-only tests (-m "not gpu") of the scene memory's carve (include/livingscenes_hip.h: ls_cloud_carve_f32): csrc/carve_plan.h -- compiled
on its own with the host compiler -- against the NumPy twin (tests/carve_oracle.py), state for state, on random and hand-made (point,
view) cases; the properties of the twin on a rendered scene; and what the C entry points decide on the host before any HIP call (the
exported symbols, the workspace sizes, every refusal).  The shared generators of tests/test_hip_cloud_carve.py (`hand_cases`,
`carve_scene`, `random_problem`) live here.  The kernels are held to the twin by equality in tests/test_hip_cloud_carve.py.

The scene: an icosphere (level 3, r 0.3) on a thin slab with two legs, three 100 x 100 views (f = 100, cameras 1.5 from the origin)
rendered by tests/render_oracle.py, 4 000 points sampled on the faces.  Figures of this scene, printed by the tests: with window 1, tol
0.01 and empty pixels free NO true surface sample is called free in any view (window 0: 776 are, 480 would be dropped); of a copy
displaced by (0.12, 0.05, -0.08) 2 659 of 4 000 rows are dropped with empty pixels free and 1 303 with empty pixels unknown."""
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
import carve_oracle as co    # noqa: E402
import render_oracle as ro   # noqa: E402

NAMES = ("ls_cloud_carve_workspace_bytes", "ls_cloud_carve_f32", "ls_cloud_carve_batch_workspace_bytes", "ls_cloud_carve_batch_f32")
F = np.float32
NAN, INF = float("nan"), float("inf")
EYE = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)


def _below(x):
    return np.nextafter(F(x), F(-np.inf))


def _above(x):
    return np.nextafter(F(x), F(np.inf))


# ------------------------------------------------------------------------------------------------ shared generators
def hand_cases():
    """The hand-made cases of the definition -> list of (name, A [a,3] f32, depth [V,H,W] f32, K [V,4], E [V,3,4], kw, expected) with kw =
    dict(tol, znear) and expected = {(window, empty_is_free): {row: state}} for the rows whose state is worked out by hand.  The camera
    is the identity, so c = x exactly; fx = fy = 4 and cx, cy are multiples of 1/2, so at z = 1 every u and v is exact."""
    cases = []
    # 1. the edges of step 3 and the near plane, on a 5 x 7 image of depth 1 (W = 5, H = 7)
    K = np.array([[4.0, 4.0, 1.5, 2.5]])
    depth = np.ones((1, 7, 5), F)
    rows = [(-0.5, 0, 1), (_below(-0.5), 0, 1),          # u = -0.5 exactly: qx = 0, inside; one ulp further left: out
            (0.75, 0, 1), (_below(0.75), 0, 1),          # u = W - 0.5 exactly: qx = W, out; one ulp below: qx = W - 1
            (0, -0.75, 1), (0, _below(-0.75), 1),        # v = -0.5
            (0, 1.0, 1), (0, _below(1.0), 1),            # v = H - 0.5
            (0, 0, 0.5), (0, 0, _below(0.5)),            # c.z == znear stays in; one ulp nearer: out
            (0, 0, -1.0), (0.1, 0.1, -0.3), (0, 0, 0.0), (0, 0, -0.0),      # behind the camera and on its plane
            (NAN, 0, 1), (0, NAN, 1), (0, 0, NAN), (INF, 0, 1), (0, -INF, 1), (0, 0, INF), (NAN, INF, -INF)]
    exp = {r: co.OUT for r in (1, 2, 5, 6, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20)}
    exp.update({0: co.SEEN, 3: co.SEEN, 4: co.SEEN, 7: co.SEEN, 8: co.FREE})
    cases.append(("edges", np.array(rows, F), depth, K, EYE[None], dict(tol=0.25, znear=0.5), {(k, e): exp for k in (0, 1, 2) for e in (0, 1)}))
    # 2. c.z == lo and c.z == hi with representable values: d 1.0, tol 0.25, z 0.75 and 1.25 and their neighbours (window 0: one pixel)
    rows = [(0, 0, 0.75), (0, 0, _below(0.75)), (0, 0, 1.25), (0, 0, _above(1.25)), (0, 0, 1.0)]
    exp = {0: co.SEEN, 1: co.FREE, 2: co.SEEN, 3: co.OCCLUDED, 4: co.SEEN}
    cases.append(("bounds", np.array(rows, F), depth, K, EYE[None], dict(tol=0.25, znear=0.05), {(k, e): exp for k in (0, 1, 2) for e in (0, 1)}))
    # 3. NaN, inf, negative and zero depth, each in the middle of a 3 x 3 block of its own kind on a 9 x 9 image, and a block of depth 2;
    #    rows at z = 1 over the five block centres
    depth = np.ones((1, 9, 9), F)
    K9 = np.array([[4.0, 4.0, 4.0, 4.0]])
    for (y, x), v in {(1, 1): NAN, (1, 4): INF, (1, 7): -1.0, (4, 1): 0.0, (4, 4): 2.0}.items():
        depth[0, y - 1:y + 2, x - 1:x + 2] = v
    centre = lambda y, x: ((x - 4) / 4.0, (y - 4) / 4.0, 1.0)
    rows = [centre(1, 1), centre(1, 4), centre(1, 7), centre(4, 1), centre(4, 4), centre(7, 7)]
    e0 = {0: co.MIXED, 1: co.FREE, 2: co.MIXED, 3: co.MIXED, 4: co.FREE, 5: co.SEEN}     # empty pixels unknown: neither front nor behind
    e1 = {0: co.FREE, 1: co.FREE, 2: co.FREE, 3: co.FREE, 4: co.FREE, 5: co.SEEN}        # empty pixels free
    cases.append(("depths", np.array(rows, F), depth, K9, EYE[None], dict(tol=0.25, znear=0.05),
                  {(0, 0): e0, (1, 0): e0, (0, 1): e1, (1, 1): e1}))
    # 4. windows that reach outside the image: every pixel of a 3 x 3 image whose centre alone is far (window 2 covers the image from
    #    anywhere), rows at z = 1 in front of the rim (depth 1: seen at window 0) and of the centre (depth 3: free at window 0)
    depth = np.ones((1, 3, 3), F)
    depth[0, 1, 1] = 3.0
    K3 = np.array([[4.0, 4.0, 1.0, 1.0]])
    rows = [((x - 1) / 4.0, (y - 1) / 4.0, 1.0) for y in range(3) for x in range(3)]
    w0 = {r: (co.FREE if r == 4 else co.SEEN) for r in range(9)}
    w12 = {r: co.SEEN for r in range(9)}
    cases.append(("tiny", np.array(rows, F), depth, K3, EYE[None], dict(tol=0.25, znear=0.05),
                  {(0, 0): w0, (0, 1): w0, (1, 0): w12, (1, 1): w12, (2, 0): w12, (2, 1): w12}))
    # 5. the same image, the rows pushed behind the rim and in front of the centre: occluded or free at window 0; every larger window
    #    holds the centre (in front of it) and rim pixels (behind them): mixed
    rows = [((x - 1) / 4.0 * 2.0, (y - 1) / 4.0 * 2.0, 2.0) for y in range(3) for x in range(3)]
    w0 = {r: (co.FREE if r == 4 else co.OCCLUDED) for r in range(9)}
    w12 = {r: co.MIXED for r in range(9)}
    cases.append(("tiny_behind", np.array(rows, F), depth, K3, EYE[None], dict(tol=0.25, znear=0.05),
                  {(0, 0): w0, (0, 1): w0, (1, 0): w12, (1, 1): w12, (2, 0): w12, (2, 1): w12}))
    return cases


def _box(lo, hi):
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    V = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
    Fc = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]])
    return V, Fc


def sample_faces(V, Fc, n, rng):
    """n points on the faces, a face chosen by its area -> float32 [n,3]"""
    tri = V[Fc]
    area = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    f = rng.choice(len(Fc), n, p=area / area.sum())
    u, v = rng.random(n), rng.random(n)
    flip = u + v > 1
    u[flip], v[flip] = 1 - u[flip], 1 - v[flip]
    return (tri[f, 0] + u[:, None] * (tri[f, 1] - tri[f, 0]) + v[:, None] * (tri[f, 2] - tri[f, 0])).astype(F)


DISPLACEMENT = F([0.12, 0.05, -0.08])


@functools.lru_cache(maxsize=None)
def carve_scene(n_points=4000):
    """the icosphere-and-boxes scene -> dict(V, F, depth [3,100,100], K [3,4], E [3,3,4], M [3,3,4] camera -> world, points [n,3] f32 on the faces)"""
    sv, sf = ro.icosphere(3, 0.3)
    parts = [(sv + [0, 0, 0.3], sf), _box([-0.4, -0.3, -0.04], [0.4, 0.3, 0.0]), _box([-0.35, -0.05, -0.4], [-0.25, 0.05, -0.04]),
             _box([0.25, -0.05, -0.4], [0.35, 0.05, -0.04])]
    V = np.concatenate([v for v, _ in parts])
    base = np.cumsum([0] + [len(v) for v, _ in parts[:-1]])
    Fc = np.concatenate([f + b for (_, f), b in zip(parts, base)])
    poses = [ro.look_at_pose(1.5 * np.array(e) / np.linalg.norm(e)) for e in ([0.3, 0.5, 1.2], [-1.0, 0.4, -0.6], [0.9, -1.0, 0.2])]
    E, M = np.stack([ro.world_to_cam(p) for p in poses]), np.stack([ro.cam_to_world(p) for p in poses])
    K = np.tile([100.0, 100.0, 50.0, 50.0], (3, 1))
    depth, _, counts = ro.render(V, Fc, E, K, 100, 100)
    assert (counts[:, 0] > 1500).all() and not counts[:, 2:].any()
    return dict(V=V, F=Fc, depth=depth, K=K, E=E, M=M, points=sample_faces(V, Fc, n_points, np.random.default_rng(5)))


def random_problem(rng, a, V, H, W, bad_rows=True):
    """a rows around the origin, V cameras about 1.5 away that look at it, depth images of a wavy sheet through the origin with holes,
    negative, NaN and inf pixels -> (A [a,3] f32, depth [V,H,W] f32, K [V,4], E [V,3,4]).  f = W, so the image spans the cloud."""
    A = rng.uniform(-0.5, 0.5, (a, 3)).astype(F)
    if bad_rows and a >= 8:
        A[a // 2], A[a // 3], A[a - 1] = [NAN, 0, 0], [0, INF, 0], [0, 0, 40.0]
        A[1] = [0, 0, -3.0]                                                # behind some camera, in front of another
    E = np.zeros((V, 3, 4))
    for v in range(V):
        d = rng.standard_normal(3)
        E[v] = ro.world_to_cam(ro.look_at_pose(rng.uniform(1.2, 1.8) * d / np.linalg.norm(d)))
    K = np.tile([float(W), float(W), (W - 1) / 2.0, (H - 1) / 2.0], (V, 1)) + rng.uniform(-0.3, 0.3, (V, 4))
    depth = (1.5 + 0.3 * rng.standard_normal((V, H, W))).astype(F)
    hole = rng.random((V, H, W))
    depth[hole < 0.15] = 0.0
    depth[(hole > 0.15) & (hole < 0.17)] = -1.0
    depth[(hole > 0.17) & (hole < 0.18)] = NAN
    depth[(hole > 0.18) & (hole < 0.19)] = INF
    return A, depth, K, E


# ------------------------------------------------------------------------------------------------ the twin on the hand-made cases
def test_hand_cases_have_the_states_worked_out_by_hand():
    reached = set()
    for name, A, depth, K, E, kw, expected in hand_cases():
        for (k, eif), exp in expected.items():
            st = co.view_states(A, depth[0], K[0], E[0], kw["tol"], k, bool(eif), kw["znear"])
            wrong = {r: (int(st[r]), s) for r, s in exp.items() if st[r] != s}
            assert not wrong, (name, k, eif, wrong)
            reached |= set(st.tolist())
    assert reached == {co.OUT, co.SEEN, co.FREE, co.OCCLUDED, co.MIXED}


def test_the_keep_rule_and_the_outputs():
    name, A, depth, K, E, kw, _ = hand_cases()[2]
    for empty in ("unknown", "free"):
        for min_free, max_seen in ((1, 0), (2, 0), (1, 1)):
            r = co.carve(A, depth, K, E, window=0, min_free=min_free, max_seen=max_seen, empty=empty, **kw)
            assert np.array_equal(r["dropped"], (r["free"] >= min_free) & (r["seen"] <= max_seen))
            assert np.array_equal(r["points"].view(np.uint32), A[~r["dropped"]].view(np.uint32)) and np.array_equal(r["src"], np.flatnonzero(~r["dropped"]))
            assert r["view_counts"].sum() == len(A) * depth.shape[0] and r["counts"][2] == r["dropped"].sum()
            assert (r["dropped"].sum() > 0) == (min_free == 1)             # one view: no row is free twice
    with pytest.raises(ValueError):
        co.carve(A, depth, K, E, 0.1, empty="maybe")


# ------------------------------------------------------------------------------------------------ carve_plan.h against the twin
@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("carve_plan") / "carve_plan_dump")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", "-I",
                    os.path.join(REPO, "livingscenes_amd", "csrc"), os.path.join(HERE, "tools", "carve_plan_dump.cpp"), "-o", exe], check=True)

    def run(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(lines)
        return [[int(t) for t in line.split()] for line in out]
    return run


def _hex(values):
    return " ".join(float(t).hex() for t in np.asarray(values, np.float64).reshape(-1))


def _case_lines(A, depth, K, E, tol, znear, k, eif):
    H, W = depth.shape
    tail = f"{_hex(E)} {_hex(K)}"
    img = _hex(depth)
    return [f"case {W} {H} {k} {eif} {float(tol).hex()} {float(znear).hex()} {tail} {_hex(x)} {img}" for x in A]


def test_carve_plan_header_equals_the_twin(plan):
    assert plan(["constants"])[0] == [co.OUT, co.SEEN, co.FREE, co.OCCLUDED, co.MIXED, 2, 256]
    lines, want = [], []
    for name, A, depth, K, E, kw, _ in hand_cases():
        for k in (0, 1, 2):
            for eif in (0, 1):
                lines += _case_lines(A, depth[0], K[0], E[0], kw["tol"], kw["znear"], k, eif)
                want += co.view_states(A, depth[0], K[0], E[0], kw["tol"], k, bool(eif), kw["znear"]).tolist()
    rng = np.random.Generator(np.random.Philox(key=[23, 7]))
    for H, W in ((3, 3), (5, 7), (16, 16)):
        for k in (0, 1, 2):
            A, depth, K, E = random_problem(rng, 40, 2, H, W)
            for v in range(2):
                for eif in (0, 1):
                    tol = float(rng.choice([0.0, 0.01, 0.1, 0.3]))
                    lines += _case_lines(A, depth[v], K[v], E[v], tol, 0.05, k, eif)
                    want += co.view_states(A, depth[v], K[v], E[v], tol, k, bool(eif), 0.05).tolist()
    got = [g[0] for g in plan(lines)]
    wrong = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not wrong, wrong[:5]
    hist = np.bincount(want, minlength=5)
    print(f"{len(want)} (point, view) cases, states {hist.tolist()}")
    assert (hist >= 20).all(), "a state the cases hardly reach"


def test_carve_plan_rules_and_pieces(plan):
    cases = [(s, f, mf, ms) for s in range(4) for f in range(4) for mf in (1, 2, 3) for ms in (0, 1, 2)]
    assert [g[0] for g in plan([f"drop {s} {f} {mf} {ms}" for s, f, mf, ms in cases])] == [int(f >= mf and s <= ms) for s, f, mf, ms in cases]
    good = (0.01, 0.05, 1, 1, 0, 0)
    bad = {1: [(-1e-9, NAN, INF, -INF)], 2: [(0.0, -1.0, NAN, INF)], 3: [(-1, 3)], 4: [(0, -2)], 5: [(-1,)], 6: [(2, -1)]}
    lines, want = [" ".join(["scalars", float(good[0]).hex(), float(good[1]).hex()] + [str(t) for t in good[2:]])], [0]
    for which, (values,) in bad.items():
        for t in values:
            a = list(good)
            a[which - 1] = t
            lines.append(" ".join(["scalars", float(a[0]).hex(), float(a[1]).hex()] + [str(t) for t in a[2:]]))
            want.append(which)
    for a in ((0.0, 1e-300, 0, 1, 0, 1), (1e300, 1e300, 2, 2 ** 31 - 1, 2 ** 31 - 1, 0)):   # the least and the largest accepted
        lines.append(" ".join(["scalars", float(a[0]).hex(), float(a[1]).hex()] + [str(t) for t in a[2:]]))
        want.append(0)
    assert [g[0] for g in plan(lines)] == want
    assert plan(["pieces 1 0 0 4096", "pieces 1 1 0 4096", "pieces 5 4096 4 4096", "pieces 5 4097 4 4096", "pieces 2 16777216 4 4096"]) == \
        [[0, 0, 0, 0, 1], [0, 1, 1, 1, 1], [24, 4096, 4096, 1, 1], [24, 4097, 4097, 2, 1], [12, 16777216, 16777216, 4096, 1]]


# ------------------------------------------------------------------------------------------------ properties of the twin on a rendered scene
def test_own_rows_are_seen_by_their_own_view():
    s = carve_scene()
    pts, _, off = ro.depth_points(s["depth"], s["K"], s["M"])
    for v in range(3):
        own = pts[off[v]:off[v + 1]]
        st = co.view_states(own, s["depth"][v], s["K"][v], s["E"][v], 1e-5, 0)
        assert len(own) > 1500 and (st == co.SEEN).all(), (v, np.bincount(st, minlength=5).tolist())


def test_no_true_surface_sample_is_dropped():
    s = carve_scene()
    r = co.carve(s["points"], s["depth"], s["K"], s["E"], 0.01, window=1, empty="free")
    narrow = co.carve(s["points"], s["depth"], s["K"], s["E"], 0.01, window=0, empty="free")
    print(f"true surface, tol 0.01, empty free: window 1 counts {r['counts'].tolist()}, window 0 counts {narrow['counts'].tolist()}")
    assert r["counts"][2] == 0 and r["counts"][1] == 0 and len(r["points"]) == len(s["points"])
    assert r["counts"][0] > len(s["points"]) // 2                          # most samples are confirmed by some view
    assert narrow["counts"][2] > 0, "the nearest pixel alone does call surface samples free: the window is what protects them"


def test_a_displaced_copy_is_carved():
    s = carve_scene()
    B = (s["points"] + DISPLACEMENT).astype(F)
    free = co.carve(B, s["depth"], s["K"], s["E"], 0.01, window=1, empty="free")
    unknown = co.carve(B, s["depth"], s["K"], s["E"], 0.01, window=1, empty="unknown")
    print(f"displaced copy: dropped {free['counts'][2]} (empty free) / {unknown['counts'][2]} (empty unknown) of {len(B)}, "
          f"seen {free['counts'][0]}")
    assert 2 * free["counts"][2] >= len(B)
    assert unknown["counts"][2] <= free["counts"][2] and not (unknown["dropped"] & ~free["dropped"]).any()
    assert unknown["counts"][2] > 0
    for r in (free, unknown):                                             # a subsequence of the input, the same bits
        assert (np.diff(r["src"]) > 0).all() and np.array_equal(r["points"].view(np.uint32), B[r["src"]].view(np.uint32))
        assert len(r["src"]) == len(B) - r["counts"][2]
    # rows some view confirms are protected at max_seen 0 and given up at max_seen 1; two views must agree at min_free 2
    loose = co.carve(B, s["depth"], s["K"], s["E"], 0.01, window=1, empty="free", max_seen=1)
    strict = co.carve(B, s["depth"], s["K"], s["E"], 0.01, window=1, empty="free", min_free=2)
    assert loose["counts"][2] > free["counts"][2] > strict["counts"][2] > 0


def test_zero_views_drop_nothing():
    s = carve_scene()
    r = co.carve(s["points"], s["depth"][:0], s["K"][:0], s["E"][:0], 0.01)
    assert r["counts"].tolist() == [0, 0, 0, len(s["points"])] and r["state"].shape == (0, len(s["points"])) and r["view_counts"].shape == (0, 5)
    assert np.array_equal(r["points"].view(np.uint32), s["points"].view(np.uint32))
    empty = co.carve(np.zeros((0, 3), F), s["depth"], s["K"], s["E"], 0.01)
    assert empty["counts"].tolist() == [0, 0, 0, 0] and not empty["view_counts"].any() and empty["points"].shape == (0, 3)


# ------------------------------------------------------------------------------------------------ the library, host side only
def test_symbols_and_bindings():
    from livingscenes_amd import _lib, build, ops, synth
    from livingscenes_amd.lib_more.more_solver import More_Solver, sequence_plan, solve_sequence
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "livingscenes_hip.h")).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and name + "(" in header, name
    assert int(lib.ls_version()) == _lib.ABI_VERSION == 107 and "#define LS_ABI_VERSION 107" in header
    assert "ls_cloud_carve_f32 / ls_cloud_carve_batch_f32" in header.split("#define LS_ABI_VERSION")[0]
    for text in ("ROW i IS DROPPED IFF free_i >= min_free AND seen_i <= max_seen", "qx = floor(u + 0.5)", "both ends inclusive",
                 "NO tol IS RECOMMENDED", "2 memsets", "6 kernels"):
        assert text in header, text
    assert "cloudcarve.hip" in build.SOURCES and build.PACKED_FP32_GUARD["cloudcarve.hip"] == []
    plan_h = open(os.path.join(REPO, "livingscenes_amd", "csrc", "carve_plan.h")).read()
    assert "#include <hip" not in plan_h and '#include "ls_' not in plan_h   # the host compiler builds it above: no HIP in it
    for f in (ops.cloud_carve, ops.cloud_carve_batch):
        sig = inspect.signature(f).parameters
        assert sig["tol"].default is inspect.Parameter.empty and sig["tol"].kind is inspect.Parameter.KEYWORD_ONLY
        assert [sig[k].default for k in ("window", "min_free", "max_seen", "empty", "znear", "return_state")] == [1, 1, 0, "unknown", 0.05, False]
        assert "derived" in f.__doc__.lower() and "recommended" in f.__doc__.lower()
    assert inspect.signature(ops.cloud_carve_batch).parameters["packed"].default is False
    assert ops.CARVE_STATE == ("out", "seen", "free", "occluded", "mixed")
    sig = inspect.signature(More_Solver._carve_batch).parameters
    assert list(sig)[1:5] == ["mem_pcs", "views", "T", "g"] and sig["tol"].default is inspect.Parameter.empty
    sig = inspect.signature(solve_sequence).parameters
    assert [sig[k].default for k in ("carve_tol", "carve_window", "carve_min_free", "carve_max_seen", "carve_empty")] == [None, 1, 1, 0, "unknown"]
    assert "carve_tol HAS NO DEFAULT AND NONE IS RECOMMENDED" in solve_sequence.__doc__ and "unmeasured" in solve_sequence.__doc__
    assert inspect.signature(synth.make_partial_views).parameters["with_depth"].default is False
    # today's values for today's arguments
    assert sequence_plan(3, [1, -1, 0], 3, [4, 0]) == {"pairs": [(0, 1), (2, 0)], "updated": [0, 2], "reencode": [0], "unmatched_new": [2]}


def test_workspace_sizes():
    from livingscenes_amd import _lib
    lib = _lib.load()
    one, batch = lib.ls_cloud_carve_workspace_bytes, lib.ls_cloud_carve_batch_workspace_bytes
    top = 2 ** 24                                                       # SCAN_MAX_N
    assert one(-1, 1) == 0 and one(1, -1) == 0 and one(top + 1, 1) == 0 and one(1, 2 ** 31) == 0
    assert batch(0, 1, 1) == 0 and batch(-1, 1, 1) == 0 and batch(1, -1, 1) == 0 and batch(2, top + 1, 1) == 0 and batch(2, 1, -1) == 0
    assert one(0, 0) > 0 and one(top, 2 ** 31 - 1) > 0 and batch(1, 0, 0) > 0
    grid = (0, 1, 100, 255, 256, 257, 4096, 4097, 60000, 3840000, top)
    sizes = [one(n, 3) for n in grid]
    assert sizes == sorted(sizes) and sizes[-1] > sizes[0] and all(v % 256 == 0 for v in sizes)
    for n in grid:
        assert one(n, 0) == one(n, 1) == one(n, 1000)                     # the views are read where they lie
        assert 8 * n <= one(n, 3) <= 8 * n + 4 * (n // 4096 + 1) + 4 * 256 + 8
        for P in (1, 7, 64):
            assert batch(P, n, 5) % 256 == 0 and one(n, 5) <= batch(P, n, 5) <= one(n, 5) + 32 * (P + 1) + 256
    assert [batch(P, 1000, 8) for P in (1, 2, 64, 4096)] == sorted(batch(P, 1000, 8) for P in (1, 2, 64, 4096))


GOOD = dict(tol=0.01, znear=0.05, window=1, min_free=1, max_seen=0, empty_is_free=0)


def _bufs():
    return (ctypes.c_float * 4096)(), (ctypes.c_float * 4096)()


def _one(lib, a=3, views=2, H=4, W=4, ws=True, ws_bytes=64, null=(), **kw):
    """the single entry with made-up buffers: only for calls the host checks refuse before anything is dereferenced"""
    s = dict(GOOD, **kw)
    A, buf = _bufs()
    b = {k: (None if k in null else buf) for k in ("A", "depth", "K", "E", "out_pts", "out_src", "out_off", "seen", "free", "counts", "view_counts")}
    b["A"] = None if "A" in null else A
    rc = lib.ls_cloud_carve_f32(b["A"], a, b["depth"], views, H, W, b["K"], b["E"], s["tol"], s["znear"], s["window"], s["min_free"], s["max_seen"],
                                s["empty_is_free"], b["out_pts"], b["out_src"], b["out_off"], b["seen"], b["free"], b["counts"], b["view_counts"],
                                None, None, buf if ws else None, ws_bytes, None)
    return rc, lib.ls_last_error().decode()


def _batch(lib, P, a_total, a_off, views_total, view_off, H=4, W=4, ws_bytes=64, **kw):
    s = dict(GOOD, **kw)
    A, buf = _bufs()
    ao, vo = np.asarray(a_off, np.int64), np.asarray(view_off, np.int64)
    rc = lib.ls_cloud_carve_batch_f32(P, A, a_total, ao.ctypes.data, buf, views_total, vo.ctypes.data, H, W, buf, buf, s["tol"], s["znear"],
                                      s["window"], s["min_free"], s["max_seen"], s["empty_is_free"], buf, buf, buf, buf, buf, buf, buf, None, None,
                                      buf, ws_bytes, None)
    return rc, lib.ls_last_error().decode()


def test_every_host_refusal():
    from livingscenes_amd import _lib
    lib = _lib.load()
    INVALID, WORKSPACE = -1, -3
    name = "cloud_carve_batch"
    good = (2, 10, [0, 4, 10], 3, [0, 1, 3])
    rc, msg = _batch(lib, 3, 30, [0, 10, 5, 30], 3, [0, 1, 2, 3])
    assert rc == INVALID and name in msg and "problem 1" in msg and "a_off" in msg and "decreases" in msg, msg
    rc, msg = _batch(lib, 3, 30, [0, 10, 20, 29], 3, [0, 1, 2, 3])
    assert rc == INVALID and "problem 2" in msg and "a_off" in msg and "ends at 29" in msg, msg
    rc, msg = _batch(lib, 3, 30, [1, 10, 20, 30], 3, [0, 1, 2, 3])
    assert rc == INVALID and "a_off[0]" in msg, msg
    rc, msg = _batch(lib, 3, 30, [0, 10, 20, 30], 3, [0, 2, 1, 3])
    assert rc == INVALID and "problem 1" in msg and "view_off" in msg and "decreases" in msg, msg
    rc, msg = _batch(lib, 3, 30, [0, 10, 20, 30], 3, [0, 1, 2, 4])
    assert rc == INVALID and "view_off" in msg and "ends at 4" in msg, msg
    rc, msg = _batch(lib, 0, 0, [0], 0, [0])
    assert rc == INVALID and "P must be" in msg, msg
    for call in (lambda **kw: _batch(lib, *good, **kw), lambda **kw: _one(lib, **kw)):
        for bad in (-1e-9, NAN, INF, -INF):
            rc, msg = call(tol=bad)
            assert rc == INVALID and "cloud_carve" in msg and "tol must be finite and >= 0" in msg, (bad, msg)
        for bad in (0.0, -0.5, NAN, INF):
            rc, msg = call(znear=bad)
            assert rc == INVALID and "znear must be finite and > 0" in msg, (bad, msg)
        for bad in (-1, 3, 100):
            rc, msg = call(window=bad)
            assert rc == INVALID and "window must be 0, 1 or 2" in msg and str(bad) in msg, (bad, msg)
        for bad in (0, -3):
            rc, msg = call(min_free=bad)
            assert rc == INVALID and "min_free must be >= 1" in msg, (bad, msg)
        rc, msg = call(max_seen=-1)
        assert rc == INVALID and "max_seen must be >= 0" in msg, msg
        for bad in (2, -1):
            rc, msg = call(empty_is_free=bad)
            assert rc == INVALID and "empty_is_free must be 0 or 1" in msg, (bad, msg)
        for H, W in ((0, 4), (4, 0), (-1, 4)):
            rc, msg = call(H=H, W=W)
            assert rc == INVALID and "at least one pixel" in msg, msg
        rc, msg = call(tol=0.0, znear=1e-300, window=0, min_free=2 ** 31 - 1, max_seen=2 ** 31 - 1, empty_is_free=1)   # the accepted extremes:
        assert rc == WORKSPACE and "workspace" in msg, msg                                                        # only the workspace is short
        rc, msg = call(window=2)
        assert rc == WORKSPACE, msg
    rc, msg = _one(lib, a=-1)
    assert rc == INVALID and "negative" in msg, msg
    rc, msg = _one(lib, views=-1)
    assert rc == INVALID and "negative" in msg, msg
    rc, msg = _one(lib, a=2 ** 24 + 1)
    assert rc == INVALID and "scan's reach" in msg, msg
    rc, msg = _one(lib, views=2 ** 31)
    assert rc == INVALID and "views exceed" in msg, msg
    for k in ("A", "out_pts", "out_src", "seen", "free"):
        rc, msg = _one(lib, null=(k,))
        assert rc == INVALID and "null A / out_pts / out_src / seen / free" in msg, (k, msg)
    for k in ("out_off", "counts"):
        rc, msg = _one(lib, null=(k,))
        assert rc == INVALID and "null out_off / counts" in msg, (k, msg)
    for k in ("depth", "K", "E", "view_counts"):
        rc, msg = _one(lib, null=(k,))
        assert rc == INVALID and "null depth / intrinsics / world_to_cam / view_counts" in msg, (k, msg)
    rc, msg = _one(lib, views=0, null=("depth", "K", "E", "view_counts"))   # no views: their arrays may be null, only the workspace is short
    assert rc == WORKSPACE, msg
    rc, msg = _batch(lib, *good)
    assert rc == WORKSPACE and "ls_cloud_carve_batch_workspace_bytes(2, 10, 3)" in msg, msg
    rc, msg = _batch(lib, *good, ws_bytes=lib.ls_cloud_carve_batch_workspace_bytes(2, 10, 3) - 1)
    assert rc == WORKSPACE and "workspace" in msg, msg
    rc, msg = _one(lib, ws=False, ws_bytes=0)
    assert rc == WORKSPACE and "ls_cloud_carve_workspace_bytes(3, 2)" in msg, msg
    rc, msg = _one(lib, ws_bytes=lib.ls_cloud_carve_workspace_bytes(3, 2) - 1)
    assert rc == WORKSPACE, msg
