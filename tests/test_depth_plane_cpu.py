"""CPU-only tests (-m "not gpu") of the normals of a depth map and of the weighted point-to-plane depth fusion
(include/livingscenes_hip.h: ls_depth_normals_f32, ls_depth_fuse_weighted_f32 / ls_depth_fuse_weighted_batch_f32): the hand cases of the
definitions; csrc/plane_plan.h -- compiled on its own with the host compiler, plain and under the address and undefined-behaviour
sanitizers, as a program with its own main -- against the NumPy twin (tests/plane_oracle.py) per step and per class; the properties of
the twin (the unweighted fuse, order, splits, a uniform weight, saturation, the analytic sphere); and what the C entry points decide on
the host before any HIP call (the exported symbols, the workspace sizes, every refusal).  The shared generators of
tests/test_hip_depth_plane.py (`normal_cases`, `weighted_cases`) live here.  The kernels are held to the twin by equality there."""
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
import plane_oracle as po         # noqa: E402
import tsdf_ray_oracle as tro     # noqa: E402
from test_depth_fuse_cpu import EYE, GPU_DIMS, _sphere_depth, fuse_problem, gpu_cases   # noqa: E402

NAMES = ("ls_depth_normals_workspace_bytes", "ls_depth_normals_f32", "ls_depth_fuse_weighted_workspace_bytes", "ls_depth_fuse_weighted_f32",
         "ls_depth_fuse_weighted_batch_workspace_bytes", "ls_depth_fuse_weighted_batch_f32")
F = np.float32
NAN, INF = float("nan"), float("inf")

# the size edges of the normals kernel: 63 / 64 / 65 and 255 / 256 / 257 pixels per view, one row, one column, one pixel
NORMAL_IMAGES = ((1, 1), (1, 5), (5, 1), (2, 2), (7, 9), (8, 8), (5, 13), (16, 16), (1, 257), (17, 15))      # (H, W)
NORMAL_VIEWS = ("1", "3", "1 plain")
WEIGHTS = ((64, 1, 64, 1), (3, 2, 5, 7))
FUSE_JUMP = 0.3            # max_jump of the normals the weighted-fuse cases carry: about the spread of fuse_problem's sheet, so both kinds of NEAR occur
WILD_F = 2.0 ** -130       # the focal length of the "wild" view
WILD_DEPTH = 2.0 ** 127    # ... and the depth of its patch


# ------------------------------------------------------------------------------------------------ shared generators
def plain_view(rng, H, W):
    """an ordinary view: a tilted, gently curved sheet about 1 away with pixel noise, a block pushed back by four max_jump (a step no
    difference may cross), holes, negative, NaN and inf pixels, and one depth pixel fenced in by holes -> (depth [H,W] f32, K [4], max_jump)"""
    y, x = np.mgrid[0:H, 0:W]
    d = 1.0 + rng.uniform(-0.02, 0.02) * x + rng.uniform(-0.02, 0.02) * y + 0.001 * (x - W / 2) ** 2 + 0.004 * rng.standard_normal((H, W))
    max_jump = 0.05
    y0, x0 = rng.integers(0, H), rng.integers(0, W)
    d[y0:y0 + max(H // 3, 1), x0:x0 + max(W // 3, 1)] += 4 * max_jump
    d = d.astype(F)
    hole = rng.random((H, W))
    d[hole < 0.10] = 0.0
    d[(hole > 0.10) & (hole < 0.12)] = -1.0
    d[(hole > 0.12) & (hole < 0.14)] = NAN
    d[(hole > 0.14) & (hole < 0.16)] = INF
    if H >= 3 and W >= 3:                                                          # NO_NEIGHBOUR inside the image: a pixel whose row is cut on both sides
        yi, xi = rng.integers(0, H), rng.integers(1, W - 1)
        d[yi, xi - 1], d[yi, xi], d[yi, xi + 1] = 0.0, 1.0, NAN
    K = np.array([1.5 * W, 1.5 * W, (W - 1) / 2.0, (H - 1) / 2.0]) + rng.uniform(-0.3, 0.3, 4)
    return d, K, max_jump


def wild_view(rng, H, W):
    """DEGENERATE cannot be reached with ordinary numbers: the three rays of a pixel, its horizontal and its vertical neighbour are never
    coplanar, so in exact arithmetic a x b is neither zero nor perpendicular to P.  What reaches it is the overflow of m . m.  This view
    has the focal length 2^-130 and depths of 1 and 3 in blocks (max_jump = 0.5: equal neighbours are usable, the others are not, and
    every valid normal is exactly (0, 0, -1)), with a 2 x 2 patch of depth 2^127: there a = (2^257, 0, 0), b = (0, 2^257, 0), m . m =
    2^1028 = inf.  Holes, NaN and inf as in plain_view."""
    bs = 3
    d = np.kron(np.where(rng.random((-(-H // bs), -(-W // bs))) < 0.5, 1.0, 3.0), np.ones((bs, bs)))[:H, :W].astype(F)
    hole = rng.random((H, W))
    d[hole < 0.08] = 0.0
    d[(hole > 0.10) & (hole < 0.12)] = NAN
    d[(hole > 0.12) & (hole < 0.14)] = INF
    if H >= 3 and W >= 3:
        yi, xi = rng.integers(0, H), rng.integers(1, W - 1)
        d[yi, xi - 1], d[yi, xi], d[yi, xi + 1] = 0.0, 1.0, -2.0
    if H >= 2 and W >= 2:
        yp, xp = rng.integers(0, H - 1), rng.integers(0, W - 1)
        d[yp:yp + 2, xp:xp + 2] = WILD_DEPTH
    K = np.array([WILD_F, WILD_F, (W - 1) / 2.0, (H - 1) / 2.0])
    return d, K, 0.5


def normal_problem(rng, H, W, views):
    """views "1": the wild view alone; "3": the wild view between two plain ones; "1 plain": one plain view -> dict(depth [V,H,W], K [V,4],
    max_jump [V])"""
    makers = {"1": (wild_view,), "3": (plain_view, wild_view, plain_view), "1 plain": (plain_view,)}[views]
    d, K, mj = zip(*[m(rng, H, W) for m in makers])
    return dict(depth=np.stack(d), K=np.stack(K), max_jump=np.array(mj, np.float64))


def reaches_every_state(H, W, views, counts):
    """what the cases are chosen for: from 64 pixels up, every state occurs in the case.  Two things are impossible: an image of one row
    or one column has no vertical (horizontal) neighbour, so it is NO_DEPTH or NO_NEIGHBOUR everywhere -- (1, 257) is such a case --, and
    a case of plain views alone cannot be DEGENERATE (wild_view says why): "1 plain" is an extra case beyond the two view counts."""
    if H * W < 64:
        return True
    tot = counts.sum(0)
    if min(H, W) == 1:
        return bool(tot[po.NO_DEPTH] > 0 and tot[po.NO_NEIGHBOUR] > 0 and tot[po.VALID] == 0 and tot[po.DEGENERATE] == 0)
    want = [po.NO_DEPTH, po.VALID, po.NO_NEIGHBOUR] + ([] if views == "1 plain" else [po.DEGENERATE])
    return bool((tot[want] > 0).all())


@functools.lru_cache(maxsize=None)
def normal_cases():
    """(H, W, views, problem, twin's (normals, state, counts)) for every image size and view set, seeded by the sizes alone: the first
    draw of salt = 0, 1, ... that reaches_every_state under the twin"""
    out = []
    for H, W in NORMAL_IMAGES:
        for vi, views in enumerate(NORMAL_VIEWS):
            for salt in range(256):
                rng = np.random.Generator(np.random.Philox(key=[H * 1000 + W, vi * 256 + salt]))
                pr = normal_problem(rng, H, W, views)
                tw = po.normals(pr["depth"], pr["K"], pr["max_jump"])
                if reaches_every_state(H, W, views, tw[2]):
                    break
            else:
                raise AssertionError(f"no draw of {H} x {W}, views {views!r} reaches every state")
            out.append((H, W, views, pr, tw))
    return out


def case_normals(pr, salt=0):
    """the normals a weighted-fuse case carries: the twin's, max_jump = FUSE_JUMP, with about half of them struck out (seeded by `salt`) so
    that NEAR voxel-views of both kinds occur however few there are; a 1 x 1 image has no neighbour and so no normal of its own: it
    carries a made-up unit normal, so that its plane path runs too"""
    V, H, W = pr["depth"].shape
    if (H, W) == (1, 1):
        return np.tile(np.array([0.6, 0.0, -0.8], F), (V, 1, 1, 1))
    if V == 0:
        return np.zeros((0, H, W, 3), F)
    n = po.normals(pr["depth"], pr["K"], FUSE_JUMP)[0]
    n[np.random.Generator(np.random.Philox(key=[H * 1000 + W, salt])).random((V, H, W)) < 0.5] = 0.0
    return n


def run_weighted(dims, pr, weights, normals=None, empty="unknown", state=None):
    state = fo.new_state(dims) if state is None else state
    vc = po.fuse_weighted(state, pr["depth"], pr["K"], pr["E"], pr["origin"], pr["voxel"], pr["trunc"], weights, normals, empty)
    return state, vc


def reaches_every_weighted_class(dims, V, H, W, vc_none, vc_plane):
    """from 255 voxels up and with a view: OUT, OCCLUDED and FREE in both runs, NEAR_PROJ without normals, NEAR_PLANE with them -- and
    NEAR_PROJ with them too unless the image is 1 x 1, whose made-up normal leaves no pixel without one"""
    if V == 0 or np.prod(dims) < 255:
        return True
    a, b = vc_none.sum(0), vc_plane.sum(0)
    ok = all(t[k] > 0 for t in (a, b) for k in (po.OUT, po.OCCLUDED, po.FREE)) and a[po.NEAR_PROJ] > 0 and a[po.NEAR_PLANE] == 0 and b[po.NEAR_PLANE] > 0
    return bool(ok and ((H, W) == (1, 1) or b[po.NEAR_PROJ] > 0) and a[po.SATURATED] == 0 and b[po.SATURATED] == 0)


@functools.lru_cache(maxsize=None)
def weighted_cases(dims):
    """the problems of tests/test_depth_fuse_cpu.gpu_cases with the normals they carry: (V, (H, W), problem, normals); the normals are
    the first case_normals(salt), salt = 0, 1, ..., with which the case reaches_every_weighted_class under the twin"""
    out = []
    for V, (H, W), pr in gpu_cases(dims):
        va = run_weighted(dims, pr, WEIGHTS[0])[1]
        for salt in range(64):
            nrm = case_normals(pr, salt)
            if reaches_every_weighted_class(dims, V, H, W, va, run_weighted(dims, pr, WEIGHTS[0], nrm)[1]):
                break
        else:
            raise AssertionError(f"no normals of {dims}, {V} views, {H} x {W} reach every class")
        out.append((V, (H, W), pr, nrm))
    return out


# ------------------------------------------------------------------------------------------------ the hand cases
K5 = np.array([4.0, 4.0, 2.0, 2.0])


def _n(depth, K=K5, max_jump=0.1):
    n, st, counts = po.normals(np.asarray(depth, F)[None], K, max_jump)
    assert counts.sum() == st.size and np.array_equal(counts[0], np.bincount(st.reshape(-1), minlength=4))
    assert not n[st != po.VALID].any()
    return n[0], st[0]


def test_normals_hand_cases():
    one = np.ones((5, 5), F)
    n, st = _n(one)                                                       # a fronto-parallel plane: (0, 0, -1) at EVERY pixel (one-sided at the rim)
    assert (st == po.VALID).all() and np.array_equal(n, np.tile(np.array([0, 0, -1], F), (5, 5, 1)))
    # a plane tilted about y: z = 1 + 0.25 X, so d (1 - 0.25 (x - 2) / 4) = 1; the normal is (0.25, 0, -1) / |.| wherever differences exist
    x = np.arange(5)
    tilt = np.tile(1.0 / (1.0 - 0.25 * (x - 2) / 4.0), (5, 1))
    n, st = _n(tilt, max_jump=1.0)
    want = np.array([0.25, 0.0, -1.0]) / np.sqrt(1.0625)
    assert (st == po.VALID).all() and np.abs(n - want).max() < 1e-6 and (n[..., 2] < 0).all()      # fp32 rounding of the depths: 6e-8 relative
    # beside a hole the one-sided difference: the same plane, the same normal, and the hole itself has no depth
    hole = tilt.copy()
    hole[2, 2] = 0.0
    n, st = _n(hole, max_jump=1.0)
    assert st[2, 2] == po.NO_DEPTH and (np.delete(st.reshape(-1), 12) == po.VALID).all() and np.abs(n[2, 1] - want).max() < 1e-6
    Pm = np.array(po.points(hole.astype(F).astype(np.float64), K5))
    a, b = Pm[:, 2, 1] - Pm[:, 2, 0], Pm[:, 3, 1] - Pm[:, 1, 1]             # backward: P(x) - P(x-1); central along y
    m = np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])
    m = m / np.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])
    assert np.array_equal(n[2, 1], (-m if m @ Pm[:, 2, 1] > 0 else m).astype(F))
    # one pixel, one row, one column: no neighbour
    assert _n(np.ones((1, 1), F))[1].tolist() == [[po.NO_NEIGHBOUR]]
    assert (_n(np.ones((1, 5), F))[1] == po.NO_NEIGHBOUR).all() and (_n(np.ones((5, 1), F))[1] == po.NO_NEIGHBOUR).all()
    # no depth: 0, negative, NaN, inf (an infinite depth is FREE to the fuse and no surface here)
    for bad in (0.0, -1.0, NAN, INF, -INF):
        d = one.copy()
        d[2, 2] = bad
        n, st = _n(d)
        assert st[2, 2] == po.NO_DEPTH and (np.delete(st.reshape(-1), 12) == po.VALID).all(), bad
    # a jump of exactly max_jump is usable, one ulp more is not (0.5 and 0.25 are exact): the centre loses all four neighbours
    for d0, usable in ((1.25, True), (np.nextafter(F(1.25), F(2)), False)):
        d = one.copy()
        d[2, 2] = d0
        n, st = _n(d, max_jump=0.25)
        assert (st[2, 2] == po.VALID) == usable and st[2, 2] in (po.VALID, po.NO_NEIGHBOUR), d0
        assert (np.delete(st.reshape(-1), 12) == po.VALID).all()          # its neighbours fall back on their other side
        assert usable or np.array_equal(n[2, 1], np.array([0, 0, -1], F))
    # three collinear points: under an infinite focal length every pixel back-projects onto the optical axis, a and b are parallel, m = 0
    n, st = _n(np.array([[1.0, 2.0], [3.0, 4.0]], F), K=np.array([INF, INF, 0.5, 0.5]), max_jump=10.0)
    assert (st == po.DEGENERATE).all() and not n.any()
    # ... and the overflow of m . m (wild_view)
    n, st = _n(np.full((2, 2), WILD_DEPTH, F), K=np.array([WILD_F, WILD_F, 0.5, 0.5]))
    assert (st == po.DEGENERATE).all()
    n, st = _n(np.ones((2, 2), F), K=np.array([WILD_F, WILD_F, 0.5, 0.5]))
    assert (st == po.VALID).all() and np.array_equal(n, np.tile(np.array([0, 0, -1], F), (2, 2, 1)))
    for bad in (0.0, -1.0, NAN, INF):
        with pytest.raises(ValueError, match="max_jump"):
            po.normals(one[None], K5, bad)


def _voxel(x, depth, normal, weights, empty="unknown", trunc=0.04, state=None):
    """one voxel at x under the identity camera and one view -> (class, sum, n)"""
    state = fo.new_state((1, 1, 1)) if state is None else state
    vc = po.fuse_weighted(state, depth[None], K5[None], EYE[None], np.array(x, np.float64), 1.0, trunc, weights, None if normal is None else normal[None], empty)
    assert vc.sum() == 1 and vc.shape == (1, 7)
    return int(np.flatnonzero(vc[0])[0]), int(state[0][0, 0, 0]), int(state[1][0, 0, 0])


def test_weighted_fuse_hand_cases():
    """identity camera, a constant depth image d = 1.0 (5 x 5, f = 4, c = 2: the axis meets pixel (2, 2)), trunc = 0.04, weights (8, 3, 5, 2)"""
    one, w = np.ones((5, 5), F), (8, 3, 5, 2)
    flat = np.tile(np.array([0, 0, -1], F), (5, 5, 1))
    tilt = np.tile(np.array([0.6, 0.0, -0.8], F), (5, 5, 1))
    assert _voxel((0, 0, 0.99), one, None, w) == (po.NEAR_PROJ, 3 * 4096, 3)
    assert _voxel((0, 0, 0.99), one, flat, w) == (po.NEAR_PLANE, 8 * 4096, 8)                     # n = -z: the plane distance IS d - z
    assert _voxel((0, 0, 0.99), one, 0 * flat, w) == (po.NEAR_PROJ, 3 * 4096, 3)                  # a zero normal: the projective value
    bad = flat.copy()
    bad[2, 2, 0] = NAN
    assert _voxel((0, 0, 0.99), one, bad, w) == (po.NEAR_PROJ, 3 * 4096, 3)                       # a normal that is not finite is not used
    # the tilted plane: s_n = 0.6 * 0 - 0.8 * (0.99 - 1) = 0.008 in fp32-widened components; q = floor(0.2 * 16384 + 0.5) up to that rounding
    s_n = (np.float64(F(0.6)) * 0.0 + 0.0) + np.float64(F(-0.8)) * (np.float64(0.99) - 1.0)
    assert _voxel((0, 0, 0.99), one, tilt, w) == (po.NEAR_PLANE, 8 * int(np.floor(s_n / 0.04 * 16384 + 0.5)), 8)
    assert abs(int(np.floor(s_n / 0.04 * 16384 + 0.5)) - 3277) <= 1
    # off the axis the plane through p = P(qx, qy), not through the voxel's own ray: c = (0.01, 0, 0.99) still rounds to pixel (2, 2)
    s_n = (np.float64(F(0.6)) * 0.01 + 0.0) + np.float64(F(-0.8)) * (np.float64(0.99) - 1.0)
    assert _voxel((0.01, 0, 0.99), one, tilt, w) == (po.NEAR_PLANE, 8 * int(np.floor(s_n / 0.04 * 16384 + 0.5)), 8)
    # the band is projective: s = 0.05 > trunc is FREE whatever the plane says, s = -0.05 OCCLUDED; inside it the plane value is clamped
    assert _voxel((0, 0, 0.95), one, tilt, w) == (po.FREE, 5 * 16384, 5)
    assert _voxel((0, 0, 1.05), one, tilt, w) == (po.OCCLUDED, 0, 0)
    steep = np.tile(np.array([1.0, 0.0, 0.0], F), (5, 5, 1))
    far = np.float64(0.97) * 0.24 / 4.0                                                            # u = 2.24: still pixel (2, 2), c.x - p.x = 0.058 > trunc
    assert _voxel((far, 0, 0.97), one, steep, w) == (po.NEAR_PLANE, 8 * 16384, 8)
    assert _voxel((-far, 0, 0.97), one, steep, w) == (po.NEAR_PLANE, -8 * 16384, 8)
    # empty pixels: skipped, or free with w_empty; an infinite depth is FREE with w_free
    hole = one.copy()
    hole[2, 2] = 0.0
    assert _voxel((0, 0, 0.99), hole, flat, w) == (po.EMPTY, 0, 0)
    assert _voxel((0, 0, 0.99), hole, flat, w, "free") == (po.FREE, 2 * 16384, 2)
    hole[2, 2] = INF
    assert _voxel((0, 0, 0.99), hole, flat, w, "free") == (po.FREE, 5 * 16384, 5)
    assert _voxel((0, 0, 0.04), one, flat, w) == (po.OUT, 0, 0)
    # saturation at n + w > 65535: a weight that fits exactly, one over
    for n0, cls, n1 in ((65535 - 8, po.NEAR_PLANE, 65535), (65535 - 7, po.SATURATED, 65535 - 7), (65535, po.SATURATED, 65535)):
        st = (np.full((1, 1, 1), 7, np.int32), np.full((1, 1, 1), n0, np.int32))
        assert _voxel((0, 0, 0.99), one, flat, w, state=st) == (cls, 7 + (8 * 4096 if cls != po.SATURATED else 0), n1)
    for bad in ((0, 1, 1, 1), (1, 256, 1, 1), (1, 1, 1), (1, 1, 1.5, 1), (1, 1, 1, -3)):
        with pytest.raises(ValueError, match="weights"):
            po.fuse_weighted(fo.new_state((1, 1, 1)), one[None], K5[None], EYE[None], np.zeros(3), 1.0, 0.04, bad)


# ------------------------------------------------------------------------------------------------ plane_plan.h against the twin
def _compile(out, flags):
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *flags, "-I",
                    os.path.join(REPO, "livingscenes_amd", "csrc"), os.path.join(HERE, "tools", "plane_plan_dump.cpp"), "-o", out], check=True)
    return out


@pytest.fixture(scope="module")
def runners(tmp_path_factory):
    d = tmp_path_factory.mktemp("plane_plan")
    exes = {"plain": _compile(str(d / "dump"), ["-O1"]),
            "sanitized": _compile(str(d / "dump_san"), ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])}

    def run(which, lines):
        out = subprocess.run([exes[which]], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(lines)
        return [line.split() for line in out]
    return run


def _hex(values):
    return " ".join(float(t).hex() if np.isfinite(t) else str(float(t)) for t in np.asarray(values, np.float64).reshape(-1))


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_plane_plan_normals_equal_the_twin(runners, which):
    """every case of the GPU test, pixel by pixel; the sanitised build is the same program with its own main: nothing is preloaded"""
    assert [int(t) for t in runners(which, ["constants"])[0]] == [po.NO_DEPTH, po.VALID, po.NO_NEIGHBOUR, po.DEGENERATE, po.OUT, po.EMPTY, po.OCCLUDED,
                                                                 po.NEAR_PLANE, po.NEAR_PROJ, po.FREE, po.SATURATED, 256, po.MAX_WEIGHT]
    lines, want = [], []
    for H, W, views, pr, (n, st, _) in normal_cases():
        for v in range(pr["depth"].shape[0]):
            lines.append(f"normals {W} {H} {float(pr['max_jump'][v]).hex()} {_hex(pr['K'][v])} {_hex(pr['depth'][v])}")
            want.append((st[v].reshape(-1), n[v].reshape(-1, 3)))
    hist = np.zeros(4, np.int64)
    for g, (st, n) in zip(runners(which, lines), want):
        g = np.array(g).reshape(-1, 4)
        assert np.array_equal(g[:, 0].astype(np.int64), st)
        got = np.array([[float.fromhex(t) for t in row] for row in g[:, 1:]], np.float64).astype(F)
        assert np.array_equal(got.view(np.uint32), n.view(np.uint32))
        hist += np.bincount(st, minlength=4)
    print(f"{len(lines)} views, states {hist.tolist()}")
    assert (hist >= 20).all()
    rng = np.random.default_rng(1)
    lines, want = [], []
    for _ in range(100):
        d, x, y, K = rng.uniform(0.1, 5), int(rng.integers(0, 300)), int(rng.integers(0, 300)), rng.uniform(0.5, 300, 4)
        lines.append(f"point {float(d).hex()} {x} {y} {_hex(K)}")
        want.append([d * (np.float64(x) - K[2]) / K[0], d * (np.float64(y) - K[3]) / K[1], d])
    assert [[float.fromhex(t) for t in g] for g in runners(which, lines)] == want


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_plane_plan_fuse_equals_the_twin(runners, which):
    rng = np.random.Generator(np.random.Philox(key=[41, 5]))
    lines, want = [], []
    for dims, (H, W) in (((3, 3, 7), (5, 7)), ((4, 4, 4), (1, 1)), ((5, 13, 1), (16, 16)), ((6, 6, 6), (3, 3))):
        pr = fuse_problem(rng, dims, 3, H, W)
        nrm = case_normals(pr)
        x = fo.positions(dims, pr["origin"], pr["voxel"])
        X = np.stack([a.reshape(-1) for a in x], 1)
        for v in range(3):
            for eif in (0, 1):
                for use in (0, 1):
                    w = WEIGHTS[(v + eif) % 2]
                    cls, q, wt = po.view_classes(x, pr["depth"][v], nrm[v] if use else None, pr["K"][v], pr["E"][v], pr["trunc"], w, bool(eif))
                    lines.append(f"fuse {W} {H} {eif} {float(pr['trunc']).hex()} {float(0.05).hex()} {' '.join(map(str, w))} {use} {_hex(pr['E'][v])} "
                                 f"{_hex(pr['K'][v])} {len(X)} {_hex(X)} {_hex(pr['depth'][v])}" + (f" {_hex(nrm[v])}" if use else ""))
                    want.append(np.stack([cls.reshape(-1).astype(np.int64), q.reshape(-1), wt.reshape(-1)], 1))
    hist = np.zeros(7, np.int64)
    for g, w in zip(runners(which, lines), want):
        got = np.array(g, np.int64).reshape(-1, 3)
        assert np.array_equal(got, w), np.flatnonzero((got != w).any(1))[:5]
        hist += np.bincount(w[:, 0], minlength=7)
    print(f"{sum(len(w) for w in want)} (voxel, view) cases, classes {hist.tolist()}")
    assert (hist[:6] >= 20).all() and hist[6] == 0, "a class the cases hardly reach"
    # the update, the weights, the sizes, max_jump and the pieces
    cases = [(c, q, w, s, n) for c in range(6) for q in (-16384, 0, 77) for w in (1, 64, 255) for s in (0, -5) for n in (0, 1, 65535 - 64, 65535 - 63, 65535)]
    want = []
    for c, q, w, s, n in cases:
        if c not in (po.NEAR_PLANE, po.NEAR_PROJ, po.FREE):
            want.append([c, s, n])
        elif n + w > 65535:
            want.append([po.SATURATED, s, n])
        else:
            want.append([c, s + w * q, n + w])
    assert [[int(t) for t in g] for g in runners(which, [f"update {c} {q} {w} {s} {n}" for c, q, w, s, n in cases])] == want
    ws = [((1, 1, 1, 1), -1), ((255, 255, 255, 255), -1), ((0, 1, 1, 1), 0), ((1, 256, 1, 1), 1), ((1, 1, -1, 1), 2), ((1, 1, 1, 1000), 3), ((0, 0, 0, 0), 0)]
    assert [int(g[0]) for g in runners(which, ["weights " + " ".join(map(str, w)) for w, _ in ws])] == [r for _, r in ws]
    sizes = [((1, 1, 1), 1), ((0, 1, 1), 1), ((-1, 4, 4), 0), ((1, 0, 4), 0), ((1, 4, -1), 0), ((8, 16384, 16383), 1), ((8, 16384, 16384), 0),
             ((0, 46341, 46341), 0), ((0, 46340, 46340), 1), ((2 ** 31 - 1, 1, 1), 1), ((2 ** 31, 1, 1), 0), ((2 ** 40, 1, 1), 0), ((3, 2 ** 31 - 1, 2 ** 31 - 1), 0)]
    assert [int(g[0]) for g in runners(which, [f"sizes {a} {b} {c}" for (a, b, c), _ in sizes])] == [r for _, r in sizes]
    jumps = [(0.1, 0), (1e-300, 0), (1e300, 0), (0.0, 1), (-1.0, 1), (NAN, 1), (INF, 1)]
    assert [int(g[0]) for g in runners(which, [f"jump {_hex([j])}" for j, _ in jumps])] == [r for _, r in jumps]
    assert [int(g[0]) for g in runners(which, ["pieces 0", "pieces 1", "pieces 24"])] == [1, 1, 24]


# ------------------------------------------------------------------------------------------------ properties of the twin
def test_cases_reach_every_state_and_class():
    """printed: the totals per image size and per grid size; the exceptions are those of reaches_every_state and reaches_every_weighted_class"""
    for H, W, views, pr, (n, st, counts) in normal_cases():
        assert reaches_every_state(H, W, views, counts) and counts.sum() == st.size
        assert not n[st != po.VALID].any() and np.allclose(np.linalg.norm(n[st == po.VALID].astype(np.float64), axis=-1), 1.0, atol=1e-6)
        P = np.stack([np.stack(po.points(pr["depth"][v].astype(np.float64), pr["K"][v]), -1) for v in range(len(st))])
        with np.errstate(all="ignore"):
            assert ((n.astype(np.float64) * np.where(np.isfinite(P), P, 0.0)).sum(-1)[st == po.VALID] < 0).all()          # towards the camera
    print("normals:", np.sum([c[4][2].sum(0) for c in normal_cases()], 0).tolist())
    for dims in GPU_DIMS:
        total = np.zeros(7, np.int64)
        for V, (H, W), pr, nrm in weighted_cases(dims):
            for w in WEIGHTS:
                _, va = run_weighted(dims, pr, w)
                _, vb = run_weighted(dims, pr, w, nrm)
                assert va.shape == (V, 7) and (va.sum(1) == np.prod(dims)).all() and (vb.sum(1) == np.prod(dims)).all()
                assert reaches_every_weighted_class(dims, V, H, W, va, vb), (dims, V, H, W, va.sum(0), vb.sum(0))
            total += vb.sum(0)
        print(dims, total.tolist())


def test_unit_weights_without_normals_are_the_fuse():
    """weights (any, 1, 1, 1) and no normals: the state of fuse_oracle.fuse bit for bit, on every problem of gpu_cases, both modes"""
    for dims in GPU_DIMS:
        for V, (H, W), pr in gpu_cases(dims):
            for empty in ("unknown", "free"):
                want = fo.new_state(dims)
                wc = fo.fuse(want, pr["depth"], pr["K"], pr["E"], pr["origin"], pr["voxel"], pr["trunc"], empty)
                got, vc = run_weighted(dims, pr, (9, 1, 1, 1), None, empty)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
                assert np.array_equal(vc[:, [po.OUT, po.EMPTY, po.OCCLUDED, po.NEAR_PROJ, po.FREE, po.SATURATED]], wc) and not vc[:, po.NEAR_PLANE].any()


def test_order_splits_and_a_uniform_weight():
    rng = np.random.Generator(np.random.Philox(key=[42, 9]))
    dims = (6, 7, 8)
    pr = fuse_problem(rng, dims, 5, 16, 16)
    nrm = case_normals(pr)
    part = lambda idx: dict(pr, depth=pr["depth"][idx], K=pr["K"][idx], E=pr["E"][idx])    # noqa: E731
    for empty in ("unknown", "free"):
        for w in WEIGHTS:
            (S, N), vc = run_weighted(dims, pr, w, nrm, empty)
            assert N.max() >= 3 and (S != 0).any() and vc[:, po.NEAR_PLANE].all() and vc[:, po.NEAR_PROJ].all()
            assert (np.abs(S.astype(np.int64)) <= N.astype(np.int64) * fo.SCALE).all()
            for perm in ([4, 3, 2, 1, 0], [2, 0, 4, 1, 3]):
                (S2, N2), vc2 = run_weighted(dims, part(perm), w, nrm[perm], empty)
                assert np.array_equal(S, S2) and np.array_equal(N, N2) and np.array_equal(vc2, vc[perm])
            for cut in (0, 1, 2, 5):
                state = fo.new_state(dims)
                parts = [run_weighted(dims, part(slice(a, b)), w, nrm[a:b], empty, state)[1] for a, b in ((0, cut), (cut, 5))]
                assert np.array_equal(S, state[0]) and np.array_equal(N, state[1]) and np.array_equal(np.concatenate(parts), vc)
        # a uniform weight k: exactly k times the state of weight 1, with and without normals
        for use in (None, nrm):
            (S1, N1), v1 = run_weighted(dims, pr, (1, 1, 1, 1), use, empty)
            for k in (2, 64, 255):
                (Sk, Nk), vk = run_weighted(dims, pr, (k,) * 4, use, empty)
                assert np.array_equal(Sk, k * S1) and np.array_equal(Nk, k * N1) and np.array_equal(vk, v1)


def test_saturation_of_the_twin():
    """n + w > 65535 is skipped, n + w == 65535 is taken; three views, so the order of the call decides"""
    one = np.ones((3, 5, 5), F)
    K, E = np.tile(K5, (3, 1)), np.tile(EYE, (3, 1, 1))
    for n0, want_n, want_cls in ((65535 - 128, 65535 - 128 + 128, [po.NEAR_PROJ, po.NEAR_PROJ, po.SATURATED]), (65535 - 127, 65535 - 127 + 64, [po.NEAR_PROJ] + [po.SATURATED] * 2),
                                 (65535, 65535, [po.SATURATED] * 3), (0, 192, [po.NEAR_PROJ] * 3)):
        state = (np.full((1, 1, 1), 7, np.int32), np.full((1, 1, 1), n0, np.int32))
        vc = po.fuse_weighted(state, one, K, E, np.array([0, 0, 0.99]), 1.0, 0.04, (1, 64, 1, 1))
        assert state[1][0, 0, 0] == want_n and state[0][0, 0, 0] == 7 + 4096 * (want_n - n0)
        assert [int(np.flatnonzero(r)[0]) for r in vc] == want_cls


# ------------------------------------------------------------------------------------------------ the analytic sphere
@functools.lru_cache(maxsize=None)
def sphere_fusions():
    """test_tsdf_ray_cpu.analytic_sphere's own grid and views (8 analytic depth maps of 200 x 200, f = 120, empty pixels taken as free),
    fused by the twin three ways -> ({name: state}, origin, h, trunc, E, K): "projective" is analytic_sphere's state itself, "plane" the
    plane value with weights (64, 1, 64, 1), "equal" the plane value with all weights 1; the normals use max_jump = trunc"""
    import test_tsdf_ray_cpu as tr
    state, origin, h, trunc, E, K = tr.analytic_sphere()
    views = len(E) - 1
    Kf = np.array([120.0, 120.0, 100.0, 100.0])
    depth = np.stack([_sphere_depth(e, Kf, 200, 200, 0.4) for e in E[:views]])
    nrm, st, counts = po.normals(depth, Kf, trunc)
    out = {"projective": state}
    for name, w, use in (("check", (7, 1, 1, 1), None), ("plane", (64, 1, 64, 1), nrm), ("equal", (1, 1, 1, 1), nrm)):
        out[name] = fo.new_state(state[0].shape)
        po.fuse_weighted(out[name], depth, Kf, E[:views], origin, h, trunc, w, use, "free")
    assert np.array_equal(out["check"][0], state[0]) and np.array_equal(out["check"][1], state[1])       # the same views, the same fuse
    return out, origin, h, trunc, E, K, counts


def sphere_medians(state, which, r=0.4):
    """test_tsdf_ray_cpu.sphere_errors for a given state: the twin's raycast at camera `which` against the analytic depth and normal ->
    (median |depth error| / h, median angle in degrees, 99th percentile of the depth error, the number of HIT pixels)"""
    _, origin, h, trunc, E, K, _ = sphere_fusions()
    e = E[which]
    M = np.concatenate([e[:, :3].T, (-e[:, :3].T @ e[:, 3])[:, None]], 1)
    got = tro.raycast(state, M[None], K, 100, 100, origin, h, trunc, 1, 0.5, 0.05)
    want = _sphere_depth(e, K, 100, 100, r).astype(np.float64)
    py, px = np.mgrid[0:100, 0:100]
    d = np.stack([(px - K[2]) / K[0], (py - K[3]) / K[1], np.ones((100, 100))], -1) @ M[:, :3].T
    hit = (got["state"][0] == tro.HIT) & (want > 0)
    pts = M[:, 3] + want[..., None] * d
    nrm = pts / np.linalg.norm(pts, axis=-1, keepdims=True)
    ang = np.degrees(np.arccos(np.clip((got["normal"][0].astype(np.float64) * nrm).sum(-1), -1, 1)))[hit]
    err = np.abs(got["depth"][0].astype(np.float64) - want)[hit] / h
    return float(np.median(err)), float(np.median(ang)), float(np.percentile(err, 99)), int(hit.sum())


MEASURED_PLANE_DEPTH = (0.0260, 0.0292)     # voxels, the MEDIAN over the HIT pixels: fused camera, unfused camera
MEASURED_PLANE_ANGLE = (2.701, 2.891)       # degrees, the median


def test_the_plane_fusion_sees_the_analytic_sphere_better():
    """Measured on the twin (the sphere, the grid and the eight views of test_tsdf_ray_cpu.analytic_sphere, empty pixels taken as free,
    normals with max_jump = trunc: 3457 VALID pixels per view, none without a neighbour; raycast at 100 x 100 pixels, f = 100, step 0.5),
    median depth error / 99th percentile / median normal angle over the HIT pixels:
                                                        from a FUSED camera              from an UNFUSED one
      projective, every vote weighs 1 (the reference)   0.2121 h / 1.277 h / 10.863 deg  0.2101 h / 1.382 h / 10.444 deg   (2386 / 2388 HIT pixels)
      plane value in the band, weights (64, 1, 64, 1)   0.0260 h / 0.603 h /  2.701 deg  0.0292 h / 0.512 h /  2.891 deg   (2402 / 2404)
      plane value, all four weights 1                   0.3921 h / 2.502 h / 11.886 deg  0.4177 h / 1.975 h / 12.095 deg   (2340 / 2358)
    The exact field read by the same raycast gives 1.154 deg (test_tsdf_ray_cpu).  Asserted: more than 1500 HIT pixels (a fusion that
    lost the silhouette would flatter its medians), both medians strictly below the projective fusion's at both cameras and at most 1.5 x
    the measured values, and -- why the weights are part of the feature -- with equal weights the plane value is NOT better than the
    projective one: most of the projective error is the t = +1 votes of pixels that hit nothing, cast with the weight of a surface
    observation onto the voxels that hug the silhouette, and a better value inside the band does nothing about them."""
    states, origin, h, trunc, E, K, counts = sphere_fusions()
    assert counts[:, po.VALID].min() > 3000 and not counts[:, po.DEGENERATE].any()      # the disc: pi (120 * 0.4 / sqrt(1.5^2 - 0.4^2))^2 = 3463 pixels
    for j, which in enumerate((0, len(E) - 1)):
        proj, plane, equal = (sphere_medians(states[k], which) for k in ("projective", "plane", "equal"))
        for name, r in (("projective", proj), ("plane 64:1", plane), ("plane, equal weights", equal)):
            print(f"camera {which}, {name}: {r[3]} HIT pixels, depth error median {r[0]:.4f} h (99th pct {r[2]:.3f} h), normal angle median {r[1]:.3f} deg")
        assert plane[3] > 1500, plane[3]
        assert plane[0] < proj[0] and plane[1] < proj[1], (which, plane, proj)
        assert plane[0] <= 1.5 * MEASURED_PLANE_DEPTH[j] and plane[1] <= 1.5 * MEASURED_PLANE_ANGLE[j], (which, plane)
        assert not (equal[0] < proj[0] and equal[1] < proj[1]), (which, equal, proj)       # without the weights the plane value is NOT better


# ------------------------------------------------------------------------------------------------ the library, host side only
def test_symbols_and_bindings():
    from livingscenes_amd import _lib, build, ops
    from livingscenes_amd.lib_more.more_solver import More_Solver, solve_sequence, solve_sequence_view_gated, solve_sequence_weighted_fusion
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "livingscenes_hip.h")).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and name + "(" in header, name
        res, args = _lib.SIGNATURES[name]
        assert getattr(lib, name).restype is res and list(getattr(lib, name).argtypes) == list(args)
    assert [len(_lib.SIGNATURES[n][1]) for n in NAMES] == [3, 12, 4, 22, 5, 24]
    assert len(_lib.SIGNATURES["ls_depth_fuse_weighted_f32"][1]) == len(_lib.SIGNATURES["ls_depth_fuse_f32"][1]) + 2
    assert int(lib.ls_version()) == _lib.ABI_VERSION == 107 and "#define LS_ABI_VERSION 107" in header
    assert "ls_depth_normals_f32, ls_depth_fuse_weighted_f32 / ls_depth_fuse_weighted_batch_f32" in header.split("#define LS_ABI_VERSION")[0]
    for text in ("P(x, y) = (d * ((double)x - cx) / fx, d * ((double)y - cy) / fy, d)", "|d_nb - d| <= max_jump", "NO_NEIGHBOUR if a or b is missing",
                 "DEGENERATE if mm is 0 or not finite", "DEGENERATE if t == 0", "1 memset (counts_out)", "literally steps 1 - 5 of ls_depth_fuse_f32",
                 "s_n = ((n_x (c_x - p_x) + n_y (c_y - p_y)) + n_z (c_z - p_z))", "q = (int) floor(value / trunc * 16384 + 0.5)",
                 "SATURATED, and skipped, if n + w > 65535", "sum += w * q and n += w", "The band is decided projectively", "BIT FOR BIT that of ls_depth_fuse_f32",
                 "NO WEIGHTS ARE RECOMMENDED"):
        assert text in " ".join(header.replace("\n *", " ").split()), text
    assert "depthplane.hip" in build.SOURCES and build.PACKED_FP32_GUARD["depthplane.hip"] == []
    csrc = os.path.join(REPO, "livingscenes_amd", "csrc")
    plan_h = open(os.path.join(csrc, "plane_plan.h")).read()
    assert "#include <hip" not in plan_h and '#include "ls_' not in plan_h and "contract(off)" in plan_h and '#include "fuse_plan.h"' in plan_h
    assert "fp::fuse_camera(" in plan_h and "cp::carve_pixel(" in plan_h and "fp::fuse_distance(" in plan_h          # steps 1 - 5 are called, not copied
    kernels = open(os.path.join(csrc, "depthplane.hip")).read()
    assert "hipMalloc" not in kernels and "Synchronize" not in kernels and kernels.count("hipLaunchKernelGGL(") == 2
    assert kernels.count("atomicAdd(") == 1 and "atomicAdd((unsigned long long*)" in kernels
    for name in ("depthfuse.hip", "fuse_plan.h"):                               # the fuse itself is untouched: the texts its own test quotes
        assert "weight" not in open(os.path.join(csrc, name)).read()
    sig = inspect.signature(ops.depth_normals).parameters
    assert list(sig) == ["depth", "intrinsics", "max_jump"] and sig["max_jump"].kind is inspect.Parameter.KEYWORD_ONLY and sig["max_jump"].default is inspect.Parameter.empty
    for f in (ops.depth_fuse_weighted, ops.depth_fuse_weighted_batch):
        sig = inspect.signature(f).parameters
        assert list(sig)[:4] == ["state", "depth" if f is ops.depth_fuse_weighted else "depths", "intrinsics", "world_to_cam"]
        for k in ("origin", "voxel", "trunc", "weights"):
            assert sig[k].default is inspect.Parameter.empty and sig[k].kind is inspect.Parameter.KEYWORD_ONLY
        assert [sig[k].default for k in ("normals", "empty", "znear")] == [None, "unknown", 0.05] and "NONE" in f.__doc__ and "RECOMMENDED" in f.__doc__
    assert ops.DEPTH_NORMAL_STATE == ("no_depth", "valid", "no_neighbour", "degenerate")
    assert ops.FUSE_WEIGHTED_CLASS == ("out", "empty", "occluded", "near_plane", "near_proj", "free", "saturated")
    assert ops.FUSE_CLASS == ("out", "empty", "occluded", "near", "free", "saturated")
    sig = inspect.signature(More_Solver._fuse_weighted_batch).parameters
    assert list(sig)[1:5] == ["fusion", "views", "T", "g"] and sig["weights"].default is inspect.Parameter.empty and sig["weights"].kind is inspect.Parameter.KEYWORD_ONLY
    assert [sig[k].default for k in ("value", "max_jump", "empty", "znear")] == ["plane", None, "unknown", 0.05]
    assert "UNMEASURED DEFAULT" in More_Solver._fuse_weighted_batch.__doc__
    sig = inspect.signature(solve_sequence_weighted_fusion).parameters
    assert list(sig) == ["solver", "ref", "rescans", "fuse_weights", "fuse_value", "fuse_max_jump", "view_tol", "min_view_agreement", "kw"]
    assert sig["fuse_weights"].kind is inspect.Parameter.KEYWORD_ONLY and sig["fuse_weights"].default is inspect.Parameter.empty
    assert [sig[k].default for k in ("fuse_value", "fuse_max_jump", "view_tol", "min_view_agreement")] == ["plane", None, None, None]
    assert "NONE IS RECOMMENDED" in solve_sequence_weighted_fusion.__doc__
    for f in (solve_sequence, solve_sequence_view_gated):                       # the pinned parameter lists stay as they are
        assert not [k for k in inspect.signature(f).parameters if "weight" in k or k in ("fuse_value", "fuse_max_jump")]
    for bad in ((0, 1, 1, 1), (1, 1, 1, 256), (1, 1, 1), (1.5, 1, 1, 1), None, "6411"):
        with pytest.raises(ValueError, match="weights"):
            ops._fuse_weights("op", bad)
    assert ops._fuse_weights("op", (64, 1, 64, 1)).tolist() == [64, 1, 64, 1] and ops._fuse_weights("op", np.array([1, 2, 3, 255])).dtype == np.int32


def test_solve_sequence_weighted_fusion_refuses_before_any_device_work():
    from livingscenes_amd.lib_more.more_solver import solve_sequence_weighted_fusion
    with pytest.raises(ValueError, match="fuse_res"):
        solve_sequence_weighted_fusion(None, None, [], fuse_weights=(64, 1, 64, 1))
    with pytest.raises(ValueError, match="fuse_res"):
        solve_sequence_weighted_fusion(None, None, [], fuse_weights=(64, 1, 64, 1), fuse_value="projective", view_tol=0.02)
    with pytest.raises(TypeError, match="fuse_weights"):
        solve_sequence_weighted_fusion(None, None, [], fuse_res=32)                              # the weights have no default
    for bad in ((0, 1, 1, 1), (1, 1, 1, 256), (1, 1, 1), None):
        with pytest.raises(ValueError, match="weights"):
            solve_sequence_weighted_fusion(None, None, [], fuse_res=32, fuse_weights=bad)
    with pytest.raises(ValueError, match="fuse_value"):
        solve_sequence_weighted_fusion(None, None, [], fuse_res=32, fuse_weights=(1, 1, 1, 1), fuse_value="cosine")
    with pytest.raises(ValueError, match="view_tol"):
        solve_sequence_weighted_fusion(None, None, [], fuse_res=32, fuse_weights=(1, 1, 1, 1), view_tol=0.0)
    with pytest.raises(ValueError, match="view_tol"):
        solve_sequence_weighted_fusion(None, None, [], fuse_res=32, fuse_weights=(1, 1, 1, 1), min_view_agreement=0.5)
    with pytest.raises(TypeError):
        solve_sequence_weighted_fusion(None, None, [], fuse_res=32, fuse_weights=(1, 1, 1, 1), no_such_argument=1)


def test_workspace_sizes():
    from livingscenes_amd import _lib
    lib = _lib.load()
    nrm, one, batch = lib.ls_depth_normals_workspace_bytes, lib.ls_depth_fuse_weighted_workspace_bytes, lib.ls_depth_fuse_weighted_batch_workspace_bytes
    assert nrm(-1, 4, 4) == 0 and nrm(1, 0, 4) == 0 and nrm(1, 4, -1) == 0 and nrm(8, 16384, 16384) == 0 and nrm(2 ** 31, 1, 1) == 0
    assert nrm(0, 4, 4) == 256 and nrm(1, 4, 4) == 256 and nrm(32, 100, 100) == 256 and nrm(33, 100, 100) == 512 and nrm(8, 16384, 16383) > 0
    assert one(0, 4, 4, 1) == 0 and one(4, 4, -1, 1) == 0 and one(4, 4, 4, -1) == 0 and one(4, 4, 4, 2 ** 31) == 0 and one(1291, 1291, 1291, 1) == 0
    assert batch(0, 4, 4, 4, 1) == 0 and batch(8, 646, 646, 646, 1) == 0 and batch(2, 4, 4, 4, -1) == 0
    for dims in ((1, 1, 1), (4, 8, 8), (64, 64, 64)):
        for views in (0, 1, 8, 1000):
            assert one(*dims, views) == lib.ls_depth_fuse_workspace_bytes(*dims, views) == batch(1, *dims, views) > 0      # the fuse's own pieces
            for P in (1, 5, 64, 4096):
                assert batch(P, *dims, views) == lib.ls_depth_fuse_batch_workspace_bytes(P, *dims, views)


GOOD = dict(nx=4, ny=4, nz=4, origin=(0.0, 0.0, 0.0), voxel=0.01, trunc=0.04, views=2, H=4, W=4, znear=0.05, empty_is_free=0, weights=(64, 1, 64, 1))


def _bufs():
    return (ctypes.c_int * 4096)(), (ctypes.c_float * 4096)()


def _one(lib, ws=True, ws_bytes=0, null=(), **kw):
    """the single entry with made-up buffers: only for calls the host checks refuse before anything is dereferenced"""
    s = dict(GOOD, **kw)
    state, buf = _bufs()
    b = {k: (None if k in null else buf) for k in ("depth", "normals", "K", "E", "view_counts")}
    b.update({k: (None if k in null else state) for k in ("sum", "n")})
    o = None if "origin" in null else np.asarray(s["origin"], np.float64).ctypes.data
    w = np.asarray(s["weights"], np.int32)
    rc = lib.ls_depth_fuse_weighted_f32(b["sum"], b["n"], s["nx"], s["ny"], s["nz"], o, s["voxel"], s["trunc"], b["depth"], b["normals"], s["views"], s["H"],
                                        s["W"], b["K"], b["E"], s["znear"], s["empty_is_free"], None if "weights" in null else w.ctypes.data, b["view_counts"],
                                        buf if ws else None, ws_bytes, None)
    return rc, lib.ls_last_error().decode()


def _batch(lib, P=2, view_off=(0, 1, 2), origin=None, voxel=None, trunc=None, ws_bytes=0, **kw):
    s = dict(GOOD, **kw)
    state, buf = _bufs()
    o = np.ascontiguousarray(np.zeros((max(P, 1), 3)) if origin is None else origin, np.float64)
    h = np.ascontiguousarray(np.full(max(P, 1), 0.01) if voxel is None else voxel, np.float64)
    t = np.ascontiguousarray(np.full(max(P, 1), 0.04) if trunc is None else trunc, np.float64)
    vo, w = np.asarray(view_off, np.int64), np.asarray(s["weights"], np.int32)
    rc = lib.ls_depth_fuse_weighted_batch_f32(P, state, state, s["nx"], s["ny"], s["nz"], o.ctypes.data, h.ctypes.data, t.ctypes.data, buf, buf, s["views"],
                                              vo.ctypes.data, s["H"], s["W"], buf, buf, s["znear"], s["empty_is_free"], w.ctypes.data, buf, buf, ws_bytes, None)
    return rc, lib.ls_last_error().decode()


def _normals(lib, views=2, H=4, W=4, max_jump=(0.1, 0.1), ws=True, ws_bytes=0, null=()):
    _, buf = _bufs()
    b = {k: (None if k in null else buf) for k in ("depth", "K", "normals", "state", "counts")}
    mj = np.asarray(max_jump, np.float64)
    rc = lib.ls_depth_normals_f32(b["depth"], views, H, W, b["K"], None if "max_jump" in null else mj.ctypes.data, b["normals"], b["state"], b["counts"],
                                  buf if ws else None, ws_bytes, None)
    return rc, lib.ls_last_error().decode()


def test_every_host_refusal():
    from livingscenes_amd import _lib
    lib = _lib.load()
    INVALID, WORKSPACE = -1, -3
    for call, name in ((lambda **kw: _batch(lib, **kw), "depth_fuse_weighted_batch"), (lambda **kw: _one(lib, **kw), "depth_fuse_weighted")):
        for k in range(4):
            for bad in (0, -1, 256, 2 ** 20):
                w = [64, 1, 64, 1]
                w[k] = bad
                rc, msg = call(weights=w)
                assert rc == INVALID and name in msg and f"weights[{k}] must be in 1 .. 255" in msg and f"got {bad}" in msg, (k, bad, msg)
        for w in ((1, 1, 1, 1), (255, 255, 255, 255)):                 # the accepted extremes: only the workspace is short
            rc, msg = call(weights=w)
            assert rc == WORKSPACE and f"ls_{name}_workspace_bytes" in msg, msg
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
    rc, msg = _batch(lib, P=3, view_off=[0, 2, 1, 2])
    assert rc == INVALID and "problem 1" in msg and "view_off" in msg and "decreases" in msg, msg
    rc, msg = _batch(lib, P=2, view_off=[0, 1, 3])
    assert rc == INVALID and "view_off" in msg and "ends at 3" in msg, msg
    rc, msg = _batch(lib, P=0, view_off=[0])
    assert rc == INVALID and "P must be" in msg, msg
    rc, msg = _one(lib, views=-1)
    assert rc == INVALID and "negative" in msg, msg
    rc, msg = _one(lib, views=2 ** 31)
    assert rc == INVALID and "views exceed" in msg, msg
    for k in ("sum", "n"):
        rc, msg = _one(lib, null=(k,))
        assert rc == INVALID and "null sum / n" in msg, (k, msg)
    rc, msg = _one(lib, null=("origin",))
    assert rc == INVALID and "null origin / voxel / trunc" in msg, msg
    rc, msg = _one(lib, null=("weights",))
    assert rc == INVALID and "null weights" in msg, msg
    for k in ("depth", "K", "E", "view_counts"):
        rc, msg = _one(lib, null=(k,))
        assert rc == INVALID and "null depth / intrinsics / world_to_cam / view_counts" in msg, (k, msg)
    rc, msg = _one(lib, null=("normals",))                                      # normals may be null: only the workspace is short
    assert rc == WORKSPACE, msg
    rc, msg = _one(lib, views=0, null=("depth", "normals", "K", "E", "view_counts"))
    assert rc == WORKSPACE, msg
    rc, msg = _one(lib, ws=False, ws_bytes=1 << 20)
    assert rc == WORKSPACE, msg
    rc, msg = _batch(lib, ws_bytes=lib.ls_depth_fuse_weighted_batch_workspace_bytes(2, 4, 4, 4, 2) - 1)
    assert rc == WORKSPACE and "workspace" in msg, msg
    # the normals
    for bad in (0.0, -0.1, NAN, INF, -INF):
        rc, msg = _normals(lib, max_jump=(0.1, bad))
        assert rc == INVALID and "depth_normals: view 1: max_jump must be finite and > 0" in msg, (bad, msg)
    for H, W in ((0, 4), (4, 0), (-1, 4)):
        rc, msg = _normals(lib, H=H, W=W)
        assert rc == INVALID and "at least one pixel" in msg, msg
    rc, msg = _normals(lib, views=-1)
    assert rc == INVALID and "negative" in msg, msg
    rc, msg = _normals(lib, views=8, H=16384, W=16384, max_jump=[0.1] * 8)
    assert rc == INVALID and "reaches 2^31" in msg, msg
    for k in ("depth", "K", "max_jump", "normals", "state", "counts"):
        rc, msg = _normals(lib, null=(k,))
        assert rc == INVALID and "null depth / intrinsics / max_jump / normals_out / state_out / counts_out" in msg, (k, msg)
    rc, msg = _normals(lib, max_jump=(1e-300, 1e300))                           # the accepted extremes: only the workspace is short
    assert rc == WORKSPACE and "ls_depth_normals_workspace_bytes" in msg, msg
    rc, msg = _normals(lib, views=0, null=("depth", "K", "max_jump", "normals", "state", "counts"))
    assert rc == WORKSPACE, msg
    rc, msg = _normals(lib, ws=False, ws_bytes=1 << 20)
    assert rc == WORKSPACE, msg
    rc, msg = _normals(lib, ws_bytes=255)
    assert rc == WORKSPACE, msg
