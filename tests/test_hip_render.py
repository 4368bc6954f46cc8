"""GPU tests of the depth renderer (csrc/meshrender.hip: ls_mesh_render_depth_f64 / ls_mesh_render_depth_batch_f64 / ls_depth_points_f32;
ops.mesh_render_depth / mesh_render_depth_batch / depth_points) and of the layers on top (livingscenes_amd.render, synth.make_partial_views).

The kernels are held to the NumPy twin of the definition (tests/render_oracle.py) BIT FOR BIT: depth and points compared as uint32, face,
counts, pixel indices and offsets as integers.  The two tolerances of this file are geometric and derived where they stand
(test_points_lie_on_the_mesh, test_render_depth_covers_a_convex_mesh)."""
import os
import re

import numpy as np
import pytest
import torch

import render_oracle as ro

pytestmark = pytest.mark.gpu
REPO = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
SMALL_BOX = int(re.search(r"\bRENDER_SMALL_BOX\s*=\s*(\d+)", open(os.path.join(REPO, "livingscenes_amd", "csrc", "render_plan.h")).read()).group(1))


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _d(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x)).to(device=_dev(), dtype=dtype)


def _bits(x):
    return np.ascontiguousarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x).view(np.uint32)


def _mesh(V, F):
    return _d(np.asarray(V, np.float64).reshape(-1, 3), torch.float64), _d(np.asarray(F, np.int64).reshape(-1, 3), torch.int32)


def _device_render(V, F, E, K, H, W, znear=0.05):
    from livingscenes_amd import ops
    depth, face, counts = ops.mesh_render_depth(*_mesh(V, F), _d(E, torch.float64), _d(K, torch.float64), H, W, znear)
    views = np.asarray(E).reshape(-1, 3, 4).shape[0]
    assert depth.dtype == torch.float32 and face.dtype == torch.int32 and counts.dtype == torch.int64
    assert depth.shape == face.shape == (views, H, W) and counts.shape == (views, 4) and counts.device.type == "cpu"
    return depth, face, counts


def _check(V, F, E, K, H, W, znear=0.05, what="", M=None):
    """the single op and the back-projection of its images against the twin -> the device's (depth, face, counts)"""
    from livingscenes_amd import ops
    E, K = np.asarray(E, np.float64).reshape(-1, 3, 4), np.asarray(K, np.float64).reshape(-1, 4)
    depth, face, counts = _device_render(V, F, E, K, H, W, znear)
    w_depth, w_face, w_counts = ro.render(V, F, E, K, H, W, znear)
    assert np.array_equal(counts.numpy(), w_counts), (what, counts.numpy().tolist(), w_counts.tolist())
    assert np.array_equal(face.cpu().numpy(), w_face), (what, "face", int((face.cpu().numpy() != w_face).sum()))
    assert np.array_equal(_bits(depth), _bits(w_depth)), (what, "depth", int((_bits(depth) != _bits(w_depth)).sum()))
    if E.shape[0]:
        pts, pix, off = ops.depth_points(depth, _d(K, torch.float64), None if M is None else _d(M, torch.float64), packed=True)
        w_pts, w_pix, w_off = ro.depth_points(w_depth, K, M)
        assert pts.dtype == torch.float32 and pix.dtype == torch.int32 and off.dtype == np.int64
        assert np.array_equal(off, w_off) and np.array_equal(pix.cpu().numpy(), w_pix), (what, "pix / off")
        assert np.array_equal(_bits(pts), _bits(w_pts)), (what, "pts")
    return depth, face, counts


def _cams(views, seed, f=None, H=64, W=64):
    """`views` cameras 1.5 from the origin looking at it -> (E [views,3,4], K [views,4], M [views,3,4])"""
    rng = np.random.default_rng(seed)
    poses = []
    for _ in range(views):
        d = rng.standard_normal(3)
        poses.append(ro.look_at_pose(1.5 * d / np.linalg.norm(d)))
    f = float(max(H, W)) if f is None else f
    K = np.tile([f, f * 0.9, W / 2.0 - 0.25, H / 2.0 + 0.5], (views, 1)) + rng.uniform(-0.5, 0.5, (views, 4))
    if views == 0:
        return np.zeros((0, 3, 4)), K, np.zeros((0, 3, 4))
    return np.stack([ro.world_to_cam(p) for p in poses]), K, np.stack([ro.cam_to_world(p) for p in poses])


def _soup(n, seed):
    """n triangles in the ball of radius 0.5: from far below a pixel to most of the image, every one its own three vertices"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-0.35, 0.35, (n, 1, 3))
    size = 10.0 ** rng.uniform(-3.5, -0.3, (n, 1, 1))
    V = (c + size * rng.standard_normal((n, 3, 3))).reshape(-1, 3)
    return V, np.arange(3 * n).reshape(n, 3)


# ------------------------------------------------------------------------------------------------ size edges
@pytest.mark.parametrize("nf", [0, 1, 255, 256, 257, 300])
def test_face_counts_across_a_workgroup(nf):
    """0 and 1 face; 255, 256, 257 across a workgroup of 256; 300 = 4 * 64 + 44: the last wave, which walks its large faces together, is partial"""
    V, F = _soup(nf, 100 + nf)
    if nf == 0:
        V = np.zeros((3, 3))
    for views in (1, 3):
        E, K, M = _cams(views, nf + views)
        _, _, counts = _check(V, F, E, K, 64, 64, what=f"nf {nf} views {views}", M=M)
        assert nf < 255 or (counts[:, 0] > 0).all()


@pytest.mark.parametrize("H,W", [(1, 1), (7, 5), (5, 7), (64, 64), (100, 100)])
def test_image_sizes(H, W):
    """7 x 5 and 5 x 7 are not square: swapped rows and columns cannot pass"""
    V, F = _soup(120, H * 1000 + W)
    for views in (1, 3):
        E, K, M = _cams(views, H + W + views, H=H, W=W)
        _check(V, F, E, K, H, W, what=f"{H} x {W} views {views}", M=M)


@pytest.fixture(scope="module")
def chair16():
    from livingscenes_amd import synth
    m = synth.canonical_mesh(5, res=16, device=_dev())
    return np.asarray(m.vertices, np.float64), np.asarray(m.faces, np.int64)


def test_canonical_mesh_against_the_twin(chair16):
    V, F = chair16
    E, K, M = _cams(3, 16, f=60.0)
    _, _, counts = _check(V, F, E, K, 64, 64, what="canonical_mesh(res=16)", M=M)
    assert (counts[:, 0] > 100).all() and (counts[:, 2:] == 0).all()


# ------------------------------------------------------------------------------------------------ the special faces
EYE, K64 = np.eye(4)[None, :3], np.array([[64.0, 64.0, 32.0, 32.0]])


def _at(u, v, z=2.0, k=K64[0]):
    """the camera-frame point that projects to pixel (u, v) at depth z"""
    return [(u - k[2]) / k[0] * z, (v - k[3]) / k[1] * z, z]


def test_shared_edge_and_coincident_faces():
    depth, face, counts = _check(ro_quad()[0], ro_quad()[1], EYE, [[8.0, 8.0, 8.0, 8.0]], 16, 16, what="quad")
    assert counts.tolist() == [[81, 2, 0, 0]] and int((face == 0).sum()) == 45 and int((face == 1).sum()) == 36
    assert set(torch.unique(depth).tolist()) == {0.0, 2.0}
    _, face, _ = _check(ro_quad()[0], [[0, 1, 2], [0, 1, 2], [2, 1, 0]], EYE, [[8.0, 8.0, 8.0, 8.0]], 16, 16, what="coincident")
    assert set(torch.unique(face).tolist()) == {-1, 0}


def ro_quad():
    return np.array([[-1, -1, 2], [1, -1, 2], [1, 1, 2], [-1, 1, 2]], np.float64), np.array([[0, 1, 2], [0, 2, 3]])


def test_whole_image_triangle_and_the_small_large_boundary():
    """one face over every pixel (the wave's lanes walk it together), and boxes of RENDER_SMALL_BOX - 1, RENDER_SMALL_BOX and
    RENDER_SMALL_BOX + 1 pixels on their own rows: the thread's walk, its last size, and the wave's first"""
    V = [_at(-200, -100), _at(400, -100), _at(-200, 500)]
    depth, _, counts = _check(V, [[0, 1, 2]], EYE, K64, 64, 64, what="whole image")
    assert counts.tolist() == [[64 * 64, 1, 0, 0]] and float(depth.min()) == 2.0
    W = SMALL_BOX + 8
    V, F = [], []
    for row, n in enumerate((SMALL_BOX - 1, SMALL_BOX, SMALL_BOX + 1)):        # n x 1 pixels; the pixel centres lie on the inclusive edge
        V += [_at(3, 1 + 2 * row, 2.0 + row), _at(3 + n - 1, 1 + 2 * row, 2.0 + row), _at(3, 1.4 + 2 * row, 2.0 + row)]
        F.append([3 * row, 3 * row + 1, 3 * row + 2])
    for row, n in enumerate((SMALL_BOX // 2, SMALL_BOX // 2 + 1)):              # two rows: 2 (n) pixels, SMALL_BOX and SMALL_BOX + 2
        V += [_at(3, 8 + 3 * row, 3.0), _at(3 + n - 1, 8 + 3 * row, 3.0), _at(3, 9 + 3 * row, 3.0)]
        F.append([9 + 3 * row, 10 + 3 * row, 11 + 3 * row])
    depth, face, counts = _check(V, F, EYE, K64, 16, W, what="small / large boundary")
    assert [int((face[0, 1 + 2 * r] == r).sum()) for r in range(3)] == [SMALL_BOX - 1, SMALL_BOX, SMALL_BOX + 1]
    for views in (1, 3):                                                         # the same faces seen at an angle, several views
        E, K, M = _cams(views, 7, f=30.0, H=16, W=W)
        _check(np.asarray(V) - [0, 0, 2.5], F, E, K, 16, W, what="boundary, posed", M=M)


def test_dropped_and_clipped_faces():
    """one corner behind znear; wholly off-image; partly off-image on each of the four sides; zero area; a NaN corner; beyond 2^24"""
    nan = float("nan")
    tris = [[_at(10, 10), _at(30, 12), _at(20, 20, 0.01)],                  # one corner nearer than znear: dropped, not clipped
            [_at(10, 10), _at(30, 12), _at(20, 20, -1.0)],                  # ... and one behind the camera
            [_at(-30, -30), _at(-10, -28), _at(-20, -5)],                   # wholly off-image
            [_at(-8.3, 20), _at(6.2, 24.6), _at(3.1, 30.7)],                # left
            [_at(70.5, 40), _at(58.2, 44.6), _at(61.1, 50.7)],              # right
            [_at(40, -6.1), _at(45.5, 4.4), _at(36.6, 5.5)],                # top
            [_at(40, 70.1), _at(45.5, 59.4), _at(36.6, 58.5)],              # bottom
            [_at(5, 50), _at(9, 54), _at(13, 58)],                          # zero area: collinear
            [_at(50, 5), _at(50, 5), _at(55, 9)],                           # zero area: a repeated corner
            [[nan, 0.0, 2.0], _at(30, 30), _at(33, 36)],                    # NaN x: 0 * NaN reaches c.z, fails the near test
            [[0.0, 0.0, nan], _at(30, 30), _at(33, 36)],                    # NaN z: fails the near test
            [[0.0, float("inf"), 2.0], _at(30, 30), _at(33, 36)],           # inf y: 0 * inf = NaN reaches c.z likewise
            [[1e5, 0.0, 0.06], _at(30, 30), _at(33, 36)],                   # projects to ~1e8 pixels: beyond 2^24 / 256
            [_at(65536.0, 20), _at(30, 30), _at(33, 36)],                   # exactly 2^24 snapped: kept
            [_at(65536.0 + 1.0 / 256, 20), _at(30, 30), _at(33, 36)],       # one sub-pixel further: dropped
            [_at(20, 40, 5.0), _at(28, 41, 5.0), _at(23, 47, 5.0)],         # an ordinary face, so that something is drawn behind the others
            [[1e308, 0.0, 2.0], _at(30, 30), _at(33, 36)]]                  # u overflows to inf: a finite c.z, not finite at the snap
    V = np.asarray(tris, np.float64).reshape(-1, 3)
    F = np.arange(V.shape[0]).reshape(-1, 3)
    _, face, counts = _check(V, F, EYE, K64, 64, 64, what="specials")
    assert counts[0, 2] == 5 and counts[0, 3] == 3 and counts[0, 1] == len(tris) - 5 - 3 - 2
    seen = set(torch.unique(face).tolist())
    assert {3, 4, 5, 6, 13, 15} <= seen and not ({0, 1, 2, 7, 8, 9, 10, 11, 12, 14, 16} & seen)
    for i, t in enumerate(tris):                                                 # and each on its own
        _check(np.asarray(t, np.float64), [[0, 1, 2]], EYE, K64, 64, 64, what=f"special {i}")


def test_a_face_outside_its_mesh_is_an_error():
    from livingscenes_amd import _lib, ops
    V, F = _mesh([[0, 0, 2], [1, 0, 2], [0, 1, 2]], [[0, 1, 2], [0, 1, 3]])
    with pytest.raises(_lib.LsError, match="outside its mesh"):
        ops.mesh_render_depth(V, F, _d(EYE, torch.float64), _d(K64, torch.float64), 8, 8)
    with pytest.raises(_lib.LsError, match="outside its mesh"):
        ops.mesh_render_depth_batch([_mesh(*ro_quad()), (V, F)], [_d(EYE, torch.float64)] * 2, _d(K64[0], torch.float64), 8, 8)


# ------------------------------------------------------------------------------------------------ ragged batches
def _batch_case(chair16):
    soup = _soup(257, 9)
    meshes = [chair16, (np.zeros((3, 3)), np.zeros((0, 3), np.int64)), ro_quad(), soup, ([_at(-200, -100), _at(400, -100), _at(-200, 500)], [[0, 1, 2]])]
    nviews = [2, 2, 0, 3, 1]
    cams = [_cams(n, 40 + i, f=70.0) for i, n in enumerate(nviews)]
    cams[4] = (EYE, K64, EYE)
    return meshes, nviews, cams


def _run_batch(meshes, cams):
    from livingscenes_amd import ops
    return ops.mesh_render_depth_batch([_mesh(V, F) for V, F in meshes], [_d(E.reshape(-1, 3, 4), torch.float64) for E, _, _ in cams],
                                       [_d(K.reshape(-1, 4), torch.float64) for _, K, _ in cams], 64, 64)


def test_batch_of_five_equals_the_single_op(chair16):
    """M = 5 with a mesh without faces and a mesh with zero views: every mesh bit-identical to the single op, which the tests above hold to the twin"""
    meshes, nviews, cams = _batch_case(chair16)
    out = _run_batch(meshes, cams)
    assert len(out) == 5
    for m, ((V, F), n, (E, K, _), (depth, face, counts)) in enumerate(zip(meshes, nviews, cams, out)):
        assert depth.shape == face.shape == (n, 64, 64) and counts.shape == (n, 4)
        if n == 0:
            continue
        s_depth, s_face, s_counts = _device_render(V, F, E, K, 64, 64)
        assert np.array_equal(_bits(depth), _bits(s_depth)) and torch.equal(face, s_face) and torch.equal(counts, s_counts), m
    assert out[1][2][:, :2].sum() == 0 and float(out[1][0].max()) == 0.0 and int(out[1][1].max()) == -1, "a mesh without faces: empty views"
    assert out[4][2].tolist() == [[64 * 64, 1, 0, 0]]


def _kernel_launches(fn):
    """the device kernels a call launches, by name, from torch's profiler"""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sorted(e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower()
                  and "memset" not in e.name.lower())


def test_launch_count_does_not_depend_on_the_batch(chair16):
    from livingscenes_amd import ops
    meshes, nviews, cams = _batch_case(chair16)
    dev_meshes = [_mesh(V, F) for V, F in meshes]
    Es = [_d(E.reshape(-1, 3, 4), torch.float64) for E, _, _ in cams]
    Ks = [_d(K.reshape(-1, 4), torch.float64) for _, K, _ in cams]
    ws = torch.empty(64 << 20, dtype=torch.uint8, device=_dev())   # so that no allocation of the bindings shows up as a kernel

    def raw(ms):
        """the C entry alone: what the bindings add around it (torch.cat, torch.empty) is not what is counted"""
        from livingscenes_amd._lib import call, ptr, stream_ptr
        V, vo, F, fo = ops._pack_meshes([dev_meshes[m] for m in ms])
        E, K = torch.cat([Es[m] for m in ms]), torch.cat([Ks[m] for m in ms])
        views, wo = E.shape[0], ops._offsets([nviews[m] for m in ms])
        depth = torch.empty(views, 64, 64, dtype=torch.float32, device=_dev())
        face = torch.empty(views, 64, 64, dtype=torch.int32, device=_dev())
        counts = torch.empty(views * 4 + 1, dtype=torch.int64, device=_dev())
        torch.cuda.synchronize()
        return lambda: call(_dev(), "ls_mesh_render_depth_batch_f64", len(ms), ptr(V), V.shape[0], ops._hptr(vo), ptr(F), F.shape[0], ops._hptr(fo),
                            views, ops._hptr(wo), ptr(E), ptr(K), 64, 64, 0.05, ptr(depth), ptr(face), ptr(counts), ptr(counts[views * 4:]), ptr(ws),
                            ws.numel(), stream_ptr(_dev()))
    one, five = _kernel_launches(raw([0])), _kernel_launches(raw([0, 1, 2, 3, 4]))
    assert len(one) == len(five) == 3, (one, five)
    for names in (one, five):
        assert [sum(k in n for n in names) for k in ("raster_kernel", "strip_kernel", "resolve_kernel")] == [1, 1, 1], names


def test_the_two_walks_of_large_faces_agree():
    """Who walks the large boxes depends on the number of (view, face) items (render_plan.h: render_strips): in a call with fewer than 64 *
    RENDER_STRIP_WAVES / 2 items a strip pass, otherwise the rasteriser's own waves.  The same views rendered four at a time (strips, the
    path every other test of this file takes and holds to the twin) and sixteen at a time (no strips), as one mesh and as a batch."""
    from livingscenes_amd import ops
    strip_waves = int(re.search(r"\bRENDER_STRIP_WAVES\s*=\s*(\d+)", open(os.path.join(REPO, "livingscenes_amd", "csrc", "render_plan.h")).read()).group(1))
    nf = 64 * strip_waves // 16 + 4                          # 16 views: just over 64 * strip_waves items; 4 views: a quarter of it
    V, F = _mesh(*_soup(nf, 77))
    E, K, _ = _cams(16, 5)
    E, K = _d(E, torch.float64), _d(K, torch.float64)
    whole = ops.mesh_render_depth(V, F, E, K, 64, 64)
    assert (whole[2][:, 0] > 1000).all()
    parts = [ops.mesh_render_depth(V, F, E[i:i + 4], K[i:i + 4], 64, 64) for i in range(0, 16, 4)]
    batch = ops.mesh_render_depth_batch([(V, F)] * 4, [E[i:i + 4] for i in range(0, 16, 4)], [K[i:i + 4] for i in range(0, 16, 4)], 64, 64)
    for got in (parts, batch):
        assert torch.equal(torch.cat([d for d, _, _ in got]).view(torch.int32), whole[0].view(torch.int32))
        assert torch.equal(torch.cat([f for _, f, _ in got]), whole[1]) and torch.equal(torch.cat([c for _, _, c in got]), whole[2])


def test_same_bits_twice_and_with_streams_in_flight(chair16):
    from livingscenes_amd import ops
    meshes, _, cams = _batch_case(chair16)

    def run():
        out = _run_batch(meshes, cams)
        depth = torch.cat([d for d, _, _ in out])
        pts, pix, off = ops.depth_points(depth, _d(np.concatenate([K.reshape(-1, 4) for _, K, _ in cams]), torch.float64), packed=True)
        return [t.cpu() for o in out for t in o] + [pts.cpu(), pix.cpu(), torch.from_numpy(off)]

    def same(a, b):
        return all(x.shape == y.shape and np.array_equal(x.numpy().view(np.uint8), y.numpy().view(np.uint8)) for x, y in zip(a, b))
    alone = run()
    assert same(alone, run())
    a = torch.randn(2048, 2048, device=_dev())
    s0, s1, s2 = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    for _ in range(2):
        for s in (s1, s2):
            with torch.cuda.stream(s):
                for _ in range(8):
                    a @ a
        with torch.cuda.stream(s0):
            got = run()
        torch.cuda.synchronize()
        assert same(alone, got)


# ------------------------------------------------------------------------------------------------ geometry
def test_points_lie_on_the_mesh():
    """Every back-projected point of canonical_mesh(res=24) lies on the mesh, up to what the definition moves it.  The snap moves a projected
    corner by at most 1/512 pixel in u and in v, that is the corner itself by at most z / 512 * sqrt(1 / fx^2 + 1 / fy^2) at its own depth
    z <= z_max; a rendered point is a convex combination of the moved corners, so it is no farther from the face than the largest such move.
    The fp32 roundings of the depth and of the output point are 2^-24 relative each, of z_max and of the point's coordinates: 2^-22 * extent
    covers both with a factor 2 to spare, extent = the larger of z_max and the largest coordinate."""
    from livingscenes_amd import ops, render, synth
    m = synth.canonical_mesh(7, res=24, device=_dev())
    V, F = _mesh(np.asarray(m.vertices), np.asarray(m.faces))
    poses = render.gen_random_poses(4, seed=2)
    E = _d(np.stack([render.world_to_cam(p) for p in poses]), torch.float64)
    Mw = _d(np.stack([render.cam_to_world(p) for p in poses]), torch.float64)
    K = _d(np.array([100.0, 100.0, 50.0, 50.0]), torch.float64)
    depth, _, counts = ops.mesh_render_depth(V, F, E, K, 100, 100)
    assert (counts[:, 0] > 200).all() and (counts[:, 2:] == 0).all()
    pts, _, off = ops.depth_points(depth, K, Mw, packed=True)
    assert off[-1] == counts[:, 0].sum()
    z_max = float(depth.max())
    bound = z_max / 512.0 * (2.0 / 100.0 ** 2) ** 0.5 + 2.0 ** -22 * max(z_max, float(pts.abs().max()))
    dist = ops.mesh_distance(V, F, pts.double(), 0.05)
    print(f"{pts.shape[0]} points, z_max {z_max:.4f}, bound {bound:.3e}, largest distance {float(dist.max()):.3e}")
    assert float(dist.max()) <= bound


def test_render_depth_covers_a_convex_mesh():
    """render.render_depth of an icosphere from eight cameras on the corners of a cube around it: the union of the clouds, at the true poses
    (the clouds come back in the mesh's frame), leaves no surface sample farther than two pixel footprints from a cloud point.  A footprint
    is z_max / f, the side of a pixel at the largest depth seen.  Every point of the sphere is within 54.8 degrees of the nearest cube corner,
    so its surface element is seen at an angle of at most 54.8 + 16 degrees (the ray's own tilt) from its normal by that camera: the pixel
    grid on the surface is stretched to at most 1 / cos(71 degrees) = 3.1 footprints one way and 1 the other, and the nearest grid point is at
    most half that diagonal, 1.6 footprints, away."""
    from livingscenes_amd import ops, render
    from livingscenes_amd.mesh_extractor2 import make_mesh
    V, F = ro.icosphere(3, 0.4)
    poses = [ro.look_at_pose(1.5 * np.array(c, np.float64) / 3 ** 0.5) for c in
             ((1, 1, 1), (1, 1, -1), (1, -1, 1), (1, -1, -1), (-1, 1, 1), (-1, 1, -1), (-1, -1, 1), (-1, -1, -1))]
    pcls, T_cw, depth = render.render_depth(make_mesh(V, F), 8, poses=poses, return_depth=True)
    assert len(pcls) == len(T_cw) == 8 and depth.shape == (8, 100, 100) and all(np.array_equal(t, p) for t, p in zip(T_cw, poses))
    assert all(p.dtype == torch.float32 and p.device.type == "cuda" and p.shape[0] > 1000 for p in pcls)
    cloud = torch.cat(pcls).double()
    r = cloud.norm(dim=1)
    assert float(r.max()) <= 0.4 + 1e-4 and float(r.min()) >= 0.4 * 0.985, "the clouds are in the mesh's frame, on the inscribed polyhedron (1e-4: the snap)"
    samples, _ = ops.mesh_sample(*_mesh(V, F), 4000, seed=1)
    nearest = torch.cdist(samples, cloud).min(dim=1).values
    footprint = float(depth.max()) / render.fx
    print(f"{cloud.shape[0]} points, footprint {footprint:.4f}, farthest sample {float(nearest.max()):.4f} = {float(nearest.max()) / footprint:.2f} footprints")
    assert float(nearest.max()) <= 2.0 * footprint
    # the mirror's own names: seeded poses, one cloud per view, pointcloud of a depth map is that view's cloud in the camera frame
    pcls2, T2 = render.render_depth(make_mesh(V, F), 3, seed=5)
    assert len(pcls2) == 3 and all(np.array_equal(a, b) for a, b in zip(T2, render.gen_random_poses(3, seed=5)))
    again, _, d2 = render.render_depth(make_mesh(V, F), 3, seed=5, return_depth=True)
    assert all(torch.equal(a, b) for a, b in zip(pcls2, again))
    cam = render.pointcloud(d2[1])
    back = (_d(render.cam_to_world(T2[1]), torch.float64) @ torch.cat([cam.double(), torch.ones(cam.shape[0], 1, dtype=torch.float64, device=cam.device)], 1).T).T
    assert cam.shape == pcls2[1].shape and float((back - pcls2[1].double()).abs().max()) < 1e-6
    batch = render.render_depth_batch([make_mesh(V, F), make_mesh(V * 0.5, F)], 3, seeds=[5, 6])
    assert all(torch.equal(a, b) for a, b in zip(batch[0][0], pcls2)) and len(batch[1][0]) == 3


def test_make_partial_views():
    from livingscenes_amd import synth
    out = synth.make_partial_views([3, 8], 2, res=16, device=_dev())
    assert len(out) == 2
    for o in out:
        assert set(o) == {"clouds", "poses"} and len(o["clouds"]) == 2 and o["poses"].shape == (2, 4, 4) and o["poses"].dtype == np.float64
        for c in o["clouds"]:
            assert c.dtype == torch.float32 and c.device.type == "cuda" and c.dim() == 2 and c.shape[1] == 3 and c.shape[0] > 100
            assert float(c.abs().max()) < 1.0, "in the shape's canonical frame"
    again = synth.make_partial_views([3, 8], 2, res=16, device=_dev())
    assert all(torch.equal(a, b) for o, p in zip(out, again) for a, b in zip(o["clouds"], p["clouds"]))
    assert all(np.array_equal(o["poses"], p["poses"]) for o, p in zip(out, again))
    other = synth.make_partial_views([3], 2, res=16, view_seed=1, device=_dev())
    assert not np.array_equal(other[0]["poses"], out[0]["poses"])
    alone = synth.make_partial_views([8], 2, res=16, device=_dev())
    assert all(torch.equal(a, b) for a, b in zip(alone[0]["clouds"], out[1]["clouds"])), "a shape's views do not depend on its batch"
    noisy = synth.make_partial_views([3], 2, res=16, noise=0.01, device=_dev())
    noisy2 = synth.make_partial_views([3], 2, res=16, noise=0.01, device=_dev())
    for c, n, n2 in zip(out[0]["clouds"], noisy[0]["clouds"], noisy2[0]["clouds"]):
        assert n.shape == c.shape and torch.equal(n, n2) and 0.005 < float((n - c).std()) < 0.015


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    from livingscenes_amd import _lib, ops
    V, F = _mesh(*ro_quad())
    E, K = _d(EYE, torch.float64), _d(K64, torch.float64)
    for args in ((V.cpu(), F, E, K), (V, F.cpu(), E, K), (V, F, E.cpu(), K), (V, F, E, K.cpu())):
        with pytest.raises(_lib.LsError):
            ops.mesh_render_depth(*args, 8, 8)
    with pytest.raises(_lib.LsError):
        ops.mesh_render_depth_batch([(V.cpu(), F)], [E], K[0], 8, 8)
    with pytest.raises(_lib.LsError):
        ops.depth_points(torch.zeros(1, 4, 4), K)
    with pytest.raises(_lib.LsError):
        ops.depth_points(torch.zeros(1, 4, 4, device=_dev()), K.cpu())
    with pytest.raises(ValueError, match="2\\^31"):
        ops.mesh_render_depth(V, F, E, K, 46341, 46341)          # 46341^2 = 2^31 + 4 633
    with pytest.raises(ValueError, match="2\\^31"):
        ops.mesh_render_depth_batch([(V, F)] * 2, [E.expand(2 ** 15, 3, 4)] * 2, K[0], 256, 128)   # 2^16 views of 2^15 pixels
    for znear in (0.0, -0.05, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="znear"):
            ops.mesh_render_depth(V, F, E, K, 8, 8, znear=znear)
    with pytest.raises(ValueError):
        ops.mesh_render_depth(V, F, E[:, :, :3], K, 8, 8)
    with pytest.raises(ValueError):
        ops.mesh_render_depth(V, F, E, K, 0, 8)
    # the C entries refuse the same on their own
    from livingscenes_amd._lib import load, ptr, stream_ptr
    depth, face = torch.empty(1, 8, 8, device=_dev()), torch.empty(1, 8, 8, dtype=torch.int32, device=_dev())
    meta, ws = torch.empty(5, dtype=torch.int64, device=_dev()), torch.empty(1 << 16, dtype=torch.uint8, device=_dev())
    for H, W, znear in ((8, 8, 0.0), (8, 8, -1.0), (0, 8, 0.05), (46341, 46341, 0.05)):
        rc = load().ls_mesh_render_depth_f64(ptr(V), 4, ptr(F), 2, 1, ptr(E), ptr(K), H, W, znear, ptr(depth), ptr(face), ptr(meta), ptr(meta[4:]), ptr(ws),
                                             ws.numel(), stream_ptr(_dev()))
        assert rc != 0 and load().ls_last_error()
    assert load().ls_mesh_render_depth_workspace_bytes(1, 46341, 46341) == 0 and load().ls_mesh_render_depth_workspace_bytes(1, 8, 8) >= 8 * 64
