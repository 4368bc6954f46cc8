"""CPU tests of the depth renderer's definition (include/livingscenes_hip.h: ls_mesh_render_depth_f64, ls_depth_points_f32): the NumPy twin
(tests/render_oracle.py) against geometry it cannot have been tuned to, the integer header csrc/render_plan.h -- compiled on its own with
the host compiler -- against the twin, the back-projection against the reference's own pointcloud (a committed fixture), and the host side
of livingscenes_amd.render.  The kernels are held to the twin bit for bit in tests/test_hip_render.py.  No GPU needed."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, ".."))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import render_oracle as ro   # noqa: E402

K100 = np.array([[100.0, 100.0, 50.0, 50.0]])


# ---------------------------------------------------------------------------------------------------- 1. the twin against a sphere
@pytest.fixture(scope="module")
def sphere_errors():
    """icospheres of radius 0.4 seen from 1.5 away at 100 x 100, f = 100, against the analytic ray-sphere depth
    -> {faces: (max error over the kept pixels, kept pixels that were not hit)}, analytic hits, kept pixels"""
    pose = ro.look_at_pose(1.5 * np.array([0.3, 0.5, 1.2]) / np.linalg.norm([0.3, 0.5, 1.2]))
    E = ro.world_to_cam(pose)
    c = E @ np.array([0.0, 0.0, 0.0, 1.0])                       # the sphere's centre in the camera frame
    py, px = np.mgrid[0:100, 0:100]
    dirs = np.stack([(px - 50) / 100.0, (py - 50) / 100.0, np.ones((100, 100))], -1)   # the ray through the INTEGER pixel coordinate, z = 1
    a, b = (dirs ** 2).sum(-1), -2.0 * (dirs @ c)
    disc = b * b - 4.0 * a * (c @ c - 0.4 ** 2)
    t = (-b - np.sqrt(np.maximum(disc, 0.0))) / (2.0 * a)        # dirs.z = 1: the ray parameter is the depth
    keep = disc > 0.02 * b * b                                   # away from the silhouette, where an inscribed polyhedron has no depth at all
    out = {}
    for level, faces in ((3, 1280), (4, 5120)):
        V, F = ro.icosphere(level, 0.4)
        assert F.shape[0] == faces
        depth, _, counts = ro.render(V, F, E[None], K100, 100, 100)
        assert counts[0, 1] == faces and counts[0, 2] == counts[0, 3] == 0
        out[faces] = (float(np.abs(depth[0][keep] - t[keep]).max()), int((depth[0][keep] == 0).sum()))
    return out, int((disc > 0).sum()), int(keep.sum())


def test_twin_converges_to_the_analytic_sphere(sphere_errors):
    """The inscribed polyhedron converges at second order: four times the faces, a quarter of the error.  Measured with this definition:
    2 409 analytic hits, 1 741 kept, max error 3.15e-3 (1 280 faces) -> 7.59e-4 (5 120 faces), ratio 0.24.  No absolute tolerance."""
    err, hits, kept = sphere_errors
    print(f"analytic hits {hits}, kept {kept}, max error {err[1280][0]:.3e} -> {err[5120][0]:.3e}, ratio {err[5120][0] / err[1280][0]:.3f}")
    assert kept >= 0.7 * hits, "the silhouette guard hides more than 30 % of the analytic hits"
    assert err[1280][1] == 0 and err[5120][1] == 0, "a kept pixel was not hit"
    assert err[5120][0] <= 0.3 * err[1280][0]


# ---------------------------------------------------------------------------------------------------- 2. shared edge and ties
QUAD_V = np.array([[-1, -1, 2], [1, -1, 2], [1, 1, 2], [-1, 1, 2]], np.float64)
QUAD_F = np.array([[0, 1, 2], [0, 2, 3]])
QUAD_E, QUAD_K = np.eye(4)[None, :3], np.array([[8.0, 8.0, 8.0, 8.0]])


def test_shared_edge_is_covered_once_and_owned_by_the_lower_face():
    depth, face, counts = ro.render(QUAD_V, QUAD_F, QUAD_E, QUAD_K, 16, 16)
    assert counts.tolist() == [[81, 2, 0, 0]]
    assert (depth[0] > 0).sum() == 81 and set(np.unique(depth[0][depth[0] > 0]).tolist()) == {2.0}
    assert [int(face[0, i, i]) for i in range(4, 13)] == [0] * 9, "the diagonal passes through nine pixel centres: both faces cover them, face 0 wins"
    assert int((face[0] == 0).sum()) == 45 and int((face[0] == 1).sum()) == 36
    hit = np.zeros((16, 16), bool)
    hit[4:13, 4:13] = True                                       # u, v = 8 x / 2 + 8 in [4, 12], edges inclusive
    assert np.array_equal(depth[0] > 0, hit), "a crack or an overshoot"


def test_coincident_faces_go_to_the_lower_index():
    depth, face, _ = ro.render(QUAD_V, np.array([[0, 1, 2], [0, 1, 2], [2, 1, 0]]), QUAD_E, QUAD_K, 16, 16)
    assert set(np.unique(face[0]).tolist()) == {-1, 0} and (face[0] == 0).sum() == 45
    depth2, face2, _ = ro.render(QUAD_V, np.array([[2, 1, 0], [0, 1, 2]]), QUAD_E, QUAD_K, 16, 16)   # no back-face culling
    assert np.array_equal(depth, depth2) and np.array_equal(face, face2)


# ---------------------------------------------------------------------------------------------------- 3. render_plan.h against the twin
@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("render_plan") / "render_plan_dump")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", "-I",
                    os.path.join(REPO, "livingscenes_amd", "csrc"), os.path.join(HERE, "tools", "render_plan_dump.cpp"), "-o", exe], check=True)

    def run(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(lines)
        return [[int(t) for t in line.split()] for line in out]
    return run


def _twin_plan(W, H, uv, small_box):
    sn = [ro.snap(t) for t in uv]
    if not all(ok for ok, _ in sn):
        return [0] * 14
    xs, ys = [sn[0][1], sn[2][1], sn[4][1]], [sn[1][1], sn[3][1], sn[5][1]]
    box = ro.pixel_box(xs, ys, W, H)
    x0, x1, y0, y1 = box if box else (0, -1, 0, -1)
    pixels = (x1 - x0 + 1) * (y1 - y0 + 1) if box else 0
    return [1, xs[0], ys[0], xs[1], ys[1], xs[2], ys[2], ro.area2(xs, ys), x0, x1, y0, y1, pixels, int(pixels <= small_box)]


def test_render_plan_header_equals_the_twin(plan):
    sub, snap_max, small_box = plan(["constants"])[0][:3]
    assert (sub, snap_max) == (ro.SUB, ro.SNAP_MAX) and small_box >= 1
    cases = []
    rng = np.random.Generator(np.random.Philox(key=[11, 3]))
    for _ in range(300):                                         # negative and off-image coordinates, every side
        cases.append((16, 12, tuple(rng.uniform(-40, 60, 6))))
    for _ in range(100):                                         # sub-pixel faces around and below zero: floor / ceil of negative integers
        c = rng.uniform(-3, 3, 2)
        cases.append((16, 12, tuple((np.tile(c, 3) + rng.uniform(-0.6, 0.6, 6)))))
    cases.append((16, 12, (5.0, 7.0, 5.0, 7.0, 9.0, 3.0)))       # a vertex exactly on a pixel centre
    cases.append((16, 12, (5.0, 7.0, 5.0, 7.0, 5.0, 7.0)))       # ... and three of them: zero area, a one-pixel box
    cases.append((16, 12, (-1.0, -1.0, -1.0, -3.0, -2.0, -1.0)))  # on pixel centres left of and above the image
    for t in (1.0 / 512, -1.0 / 512, 3.0 / 512, -3.0 / 512, 0.5 - 1.0 / 512, -0.5 - 1.0 / 512):   # the rounding of the snap at its ties
        cases.append((16, 12, (t, t, 4.0 + t, t, t, 4.0 + t)))
    for n in (small_box - 1, small_box, small_box + 1):          # boxes of n pixels: n x 1, 1 x n, and 2-row boxes where n is even
        cases.append((512, 512, (3.0, 5.0, 3.0 + n - 1, 5.0, 3.0, 5.0)))
        cases.append((512, 512, (3.0, 5.0, 3.0, 5.0 + n - 1, 3.4, 5.0)))
        if n % 2 == 0:
            cases.append((512, 512, (3.0, 5.0, 3.0 + n // 2 - 1, 6.0, 3.0, 6.0)))
    lim = float(ro.SNAP_MAX) / ro.SUB                            # +-2^24 snapped, and one beyond
    for s in (1.0, -1.0):
        cases.append((16, 12, (s * lim, 0.0, 1.0, 1.0, 2.0, 5.0)))
        cases.append((16, 12, (1.0, 1.0, 2.0, s * lim, 3.0, 4.0)))
        cases.append((16, 12, (s * (lim + 1.0 / ro.SUB), 0.0, 1.0, 1.0, 2.0, 5.0)))
        cases.append((16, 12, (1.0, 1.0, 2.0, 5.0, 3.0, s * (lim + 1.0 / ro.SUB))))
    for bad in (float("nan"), float("inf"), -float("inf"), 1e300):
        cases.append((16, 12, (bad, 0.0, 1.0, 1.0, 2.0, 5.0)))
    got = plan([f"{W} {H} " + " ".join(float(t).hex() for t in uv) for W, H, uv in cases])
    want = [_twin_plan(W, H, uv, small_box) for W, H, uv in cases]
    wrong = [(c, g, w) for c, g, w in zip(cases, got, want) if g != w]
    assert not wrong, wrong[:3]
    # the cases reach what they are there for
    assert {w[13] for w in want if w[0] and w[12] in (small_box - 1, small_box, small_box + 1)} == {0, 1}
    assert any(w[0] and w[12] == 0 for w in want) and any(not w[0] for w in want) and any(w[0] and min(w[1:7]) < 0 for w in want)
    assert [w[0] for w in want[-12:-4]] == [1, 1, 0, 0] * 2, "2^24 is within the snap's range, one sub-pixel further is not"


def test_render_plan_strips(plan):
    """render_strips: who walks the large boxes is a choice of speed (every strip pass gives the same images, tests/test_hip_render.py), but
    the strips must tile the image's rows exactly, and a call with many items must keep the walk in the rasteriser"""
    strip_waves, min_rows, max_strips = plan(["constants"])[0][3:]
    cases = [(items, H) for items in (0, 1, 12, 63, 64, 65, 4096, 64 * strip_waves // 2, 64 * strip_waves // 2 + 1, 64 * strip_waves - 1, 64 * strip_waves,
                                      10 ** 7, 2 ** 31 - 1) for H in (1, 3, 4, 5, 7, 100, 480, 4097, 2 ** 20)]
    for (items, H), (count, rows) in zip(cases, plan([f"strips {i} {h}" for i, h in cases])):
        waves = max((items + 63) // 64, 1)
        assert 1 <= count <= max_strips and rows >= 1 and count * rows >= H > (count - 1) * rows, (items, H, count, rows)
        assert count == 1 or rows >= min(min_rows, H), (items, H, count, rows)
        assert count * waves <= max(strip_waves, waves), (items, H, count, rows)
        assert count == 1 if 2 * waves > strip_waves or H < 2 * min_rows else count >= 2, (items, H, count, rows)
    assert plan(["strips 12 480"])[0] == [120, 4] and plan([f"strips {64 * strip_waves} 480"])[0] == [1, 480]


# ---------------------------------------------------------------------------------------------------- 4. pointcloud against the reference's own
def test_pointcloud_equals_the_reference_fixture():
    """tests/golden/render_pointcloud.npz (scripts/dev/make_render_golden.py): a 7 x 5 depth map and the reference's pointcloud of it.  The
    reference multiplies by inv(k) held in fp32 (0.01f, -0.5f) in mixed fp32 / float64 arithmetic; here (px - cx) / fx is formed in float64.
    Measured difference to the fixture: 2.9e-9 for the mirror (float64 out) and 5.0e-8 for the twin's fp32 output, at a largest coordinate
    of 2.47 (one fp32 ulp there: 2.4e-7).  Allowed: 4 ulp of the largest coordinate, 9.5e-7."""
    from livingscenes_amd import render
    g = np.load(os.path.join(HERE, "golden", "render_pointcloud.npz"))
    depth, want = g["depth"], g["xyz"]
    assert depth.shape == (7, 5) and depth.dtype == np.float32 and (depth == 0).any() and want.shape[0] == (depth > 0).sum()
    tol = 4 * float(np.spacing(np.float32(np.abs(want).max())))
    mirror = render.pointcloud(depth)
    pts, pix, off = ro.depth_points(depth[None], [[render.fx, render.fy, render.cx, render.cy]])
    d_mirror, d_twin = float(np.abs(mirror - want).max()), float(np.abs(pts.astype(np.float64) - want).max())
    print(f"largest coordinate {np.abs(want).max():.4f}, tolerance {tol:.3e}, mirror {d_mirror:.3e}, twin {d_twin:.3e}")
    assert mirror.shape == want.shape and d_mirror <= tol
    assert pts.shape == want.shape and d_twin <= tol
    py, px = np.where(depth > 0)
    assert np.array_equal(pix, py * 5 + px) and off.tolist() == [0, want.shape[0]]


# ---------------------------------------------------------------------------------------------------- 5. gen_random_poses
def test_gen_random_poses():
    from livingscenes_amd import render
    poses = render.gen_random_poses(16, seed=3)
    assert len(poses) == 16 and all(p.shape == (4, 4) and p.dtype == np.float64 for p in poses)
    for p in poses:
        R = p[:3, :3]
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(R) - 1.0) < 1e-14
        assert np.array_equal(p[:3, 3], 1.5 * R[:, 2]) and np.array_equal(p[3], [0, 0, 0, 1])
        # the camera is the origin of its own frame and the world origin lies 1.5 in front of it (1e-14: a few dozen float64 roundings at magnitude 1.5)
        assert np.abs(render.world_to_cam(p) @ np.append(p[:3, 3], 1.0)).max() < 1e-14
        assert np.abs(render.world_to_cam(p) @ np.array([0, 0, 0, 1.0]) - [0, 0, 1.5]).max() < 1e-14
        assert np.abs(render.cam_to_world(p) @ np.append(render.world_to_cam(p) @ np.array([0.1, 0.2, 0.3, 1.0]), 1.0) - [0.1, 0.2, 0.3]).max() < 1e-14
    again = render.gen_random_poses(16, seed=3)
    assert all(np.array_equal(a, b) for a, b in zip(poses, again))
    assert not np.array_equal(render.gen_random_poses(1, seed=4)[0], poses[0])
    assert np.array_equal(render.gen_random_poses(3, seed=3)[2], poses[2]), "a prefix of a longer draw"
    assert (render.image_height, render.image_width, render.fx, render.fy, render.cx, render.cy) == (100, 100, 100, 100, 50, 50)
    # the directions are spread over the sphere (a uniform rotation, not a fixed one)
    z = np.stack([p[:3, 2] for p in render.gen_random_poses(400, seed=0)])
    assert np.abs(z.mean(0)).max() < 0.15 and np.abs((z ** 2).mean(0) - 1.0 / 3).max() < 0.08
