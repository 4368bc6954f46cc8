"""Depth views of watertight meshes and their back-projection to partial point clouds: the reference's utils/render.py under its names
(gen_random_poses, pointcloud, render_depth), with the rasteriser on the device (ops.mesh_render_depth, csrc/meshrender.hip) where the
reference uses pyrender / OpenGL.  Parity with pyrender's rasteriser is NOT pinned (it is not available to the tests): the semantics are
those of include/livingscenes_hip.h (ls_mesh_render_depth_f64), which tests/render_oracle.py states as NumPy.  Import it as
`from livingscenes_amd import render`; dropin.install() does not register it (the reference's package name `utils` is too generic to claim).
render_mesh (colour, shading) is out of scope."""
import numpy as np
import torch

from . import ops

scale = 1
image_height = 100 * scale
image_width = 100 * scale
fx = 100 * scale
fy = 100 * scale
cx = 50 * scale
cy = 50 * scale
k = np.array([fx, 0, cx, 0, fy, cy, 0, 0, 1], dtype=np.float32).reshape((3, 3))


def _random_rotation(rng):
    """uniform on SO(3): a unit quaternion from four normals (what scipy's Rotation.random draws)"""
    q = rng.standard_normal(4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def gen_random_poses(n_views, seed=0):
    """utils/render.py:22-32: n_views pyrender-style camera-to-world poses [4,4] float64 with a uniform rotation R and the translation
    1.5 R[:, 2] -- what the reference's `Rot @ inv(k) @ [cx, cy, 1] * 1.5` evaluates to (inv(k) @ [cx, cy, 1] = [0, 0, 1]): the camera sits
    1.5 from the origin and looks at it.  `seed` is the one argument the reference lacks: it draws from the unseeded global generator."""
    rng = np.random.Generator(np.random.Philox(key=[int(seed) & 0xFFFFFFFF, 0x52454E44]))
    poses = []
    for _ in range(int(n_views)):
        R = _random_rotation(rng)
        pose = np.eye(4)
        pose[:3, :3] = R
        pose[:3, 3] = 1.5 * R[:, 2]
        poses.append(pose)
    return poses


def world_to_cam(pose):
    """E [3,4] float64 = diag(1, -1, -1) inverse(pose)[:3]: world -> the renderer's camera frame (x right, y down, z forward)"""
    return np.diag([1.0, -1.0, -1.0]) @ np.linalg.inv(np.asarray(pose, np.float64))[:3]


def cam_to_world(pose):
    """M [3,4] float64 = (pose diag(1, -1, -1, 1))[:3]: the renderer's camera frame -> world"""
    return (np.asarray(pose, np.float64) @ np.diag([1.0, -1.0, -1.0, 1.0]))[:3]


def _intrinsics(dev):
    return torch.tensor([fx, fy, cx, cy], dtype=torch.float64, device=dev)


def pointcloud(depth):
    """utils/render.py:93-108: the pixels with depth > 0 of one depth map [H,W], in np.where's order, back-projected with the module's
    intrinsics into the camera frame (x right, y down, z forward): x = ((px - cx) / fx) d, y = ((py - cy) / fy) d, z = d.
    A HIP tensor goes through ops.depth_points and comes back as an fp32 HIP tensor [n,3]; a NumPy array is the reference's host-side
    data preparation and is evaluated in float64 NumPy -> float64 [n,3], as the reference returns (which multiplies by an fp32 inv(k): the
    two agree to fp32 rounding, tests/test_render_cpu.py)."""
    if torch.is_tensor(depth):
        if depth.dim() != 2:
            raise ValueError(f"pointcloud: depth is [H, W], got {tuple(depth.shape)}")
        return ops.depth_points(depth[None], _intrinsics(depth.device))[0][0]
    depth = np.asarray(depth)
    py, px = np.where(depth > 0)
    d = depth[py, px].astype(np.float64)
    return np.stack([((px - np.float64(cx)) / np.float64(fx)) * d, ((py - np.float64(cy)) / np.float64(fy)) * d, d], 1)


def _render(meshes, pose_lists, dev):
    """every mesh under its poses in one device call and one back-projection -> per mesh (clouds [views], depth [views,H,W])"""
    from .evaluate import _device_meshes
    dm = _device_meshes(meshes, dev, one=len(meshes) == 1)
    E = [torch.from_numpy(np.stack([world_to_cam(p) for p in poses]).reshape(-1, 3, 4)).to(dev) if len(poses) else
         torch.zeros(0, 3, 4, dtype=torch.float64, device=dev) for poses in pose_lists]
    K = _intrinsics(dev)
    out = ops.mesh_render_depth_batch(dm, E, K, image_height, image_width)
    nviews = [len(p) for p in pose_lists]
    if sum(nviews) == 0:
        return [([], d) for d, _, _ in out]
    depth = torch.cat([d for d, _, _ in out], 0)
    Mw = torch.from_numpy(np.stack([cam_to_world(p) for poses in pose_lists for p in poses])).to(dev)
    clouds = [pts for pts, _ in ops.depth_points(depth, K, Mw)]
    res, at = [], 0
    for (d, _, _), n in zip(out, nviews):
        res.append((clouds[at:at + n], d))
        at += n
    return res


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("livingscenes_amd.render renders on the device: no HIP device is available and there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def render_depth(tri_mesh, n_views, seed=0, poses=None, return_depth=False):
    """utils/render.py:50-91: n_views depth views of `tri_mesh` (anything with .vertices / .faces) from gen_random_poses(n_views, seed), or
    from the given pyrender-style `poses`, at the module's camera settings, each back-projected to a point cloud in the MESH's frame.
    -> (pcls, T_cw_list): pcls = n_views fp32 HIP tensors [n_i,3], T_cw_list = the poses [4,4] float64 (T_cw equals the pose: the
    reference's `T[:, 1:3] *= -1` acts on a [3,1] array, whose columns 1:3 are empty, and is a no-op).  return_depth=True appends the depth
    maps [n_views,H,W] fp32 (0 = nothing hit).  `seed` is the argument the reference lacks."""
    poses = gen_random_poses(n_views, seed) if poses is None else [np.asarray(p, np.float64) for p in poses]
    if len(poses) != int(n_views):
        raise ValueError(f"render_depth: {len(poses)} poses for n_views = {n_views}")
    (pcls, depth), = _render([tri_mesh], [poses], _device())
    T_cw_list = [p.copy() for p in poses]
    return (pcls, T_cw_list, depth) if return_depth else (pcls, T_cw_list)


def render_depth_batch(meshes, n_views, seeds):
    """render_depth for many meshes in ONE device call: n_views views of meshes[i] from gen_random_poses(n_views, seeds[i])
    -> list of (pcls, T_cw_list), element i equal to render_depth(meshes[i], n_views, seeds[i])."""
    if len(seeds) != len(meshes):
        raise ValueError(f"render_depth_batch: {len(seeds)} seeds for {len(meshes)} meshes")
    if not meshes:
        return []
    pose_lists = [gen_random_poses(n_views, s) for s in seeds]
    return [(pcls, [p.copy() for p in poses]) for (pcls, _), poses in zip(_render(list(meshes), pose_lists, _device()), pose_lists)]
