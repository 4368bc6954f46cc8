"""Evaluation metrics of the reference's evaluate.py, under the reference's names and signatures.

chamfer_distance_torch (/root/reference/evaluate.py:111-123): both clouds are compared after the PREDICTED transform -- the
source moved by the prediction against the target, and the target against itself moved by prediction o inverse(ground truth) --
as mean nearest-neighbour SQUARED distance in each direction, summed.  The reference materialises the [n, m] squared-distance
matrix; here the nearest neighbours come from the library's raw-cloud k-NN (ls_knn_f32, K = 1: wave-per-query kernel), whose
distance is the same (dx^2 + dy^2 + dz^2) chain.  HIP tensors only, like every operator of this package.

The reconstruction metrics (evaluate.py:12-109: compute_chamfer_distance, compute_volumetric_iou, compute_sdf_recall, and libmesh's
check_mesh_contains) run on the device without trimesh / point_cloud_utils / the Cython triangle hash (csrc/meshmetrics.hip).  A mesh is
anything with ``.vertices`` [nv,3] and ``.faces`` [nf,3] (trimesh, mesh_extractor2.SimpleMesh, numpy arrays or torch tensors); a point
cloud (gt_points) anything with ``.vertices``.  An empty mesh (no faces) contains nothing and is infinitely far away.
"""
import numpy as np
import torch

from . import ops
from .lib_math import torch_se3


def _nn_sq_dist(a, b):
    """a [B,n,3], b [B,m,3] -> [B,n] squared distance of every a-point to its nearest b-point"""
    _, d = ops.knn(a.float().contiguous().unsqueeze(-1), b.float().contiguous().unsqueeze(-1), 1, return_dist=True)
    return d[..., 0]


def chamfer_distance_torch(src, ref, pred_tsfm, gt_tsfm):
    src_transformed = torch_se3.transform(pred_tsfm, src)
    ref_inv_transformed = torch_se3.transform(torch_se3.concatenate(pred_tsfm, torch_se3.inverse(gt_tsfm)), ref)
    dist_src = _nn_sq_dist(src_transformed, ref)
    dist_ref = _nn_sq_dist(ref, ref_inv_transformed)
    return dist_src.mean(dim=1) + dist_ref.mean(dim=1)


def registration_metrics_batch(pcs1, pcs2, pred, gt, chamfer_stride=10, sizes=None):
    """What the relocalisation loops compute per registered pair (eval_3rscan.py:384-401, eval_flyingshape.py:136-148), for P pairs in one
    device call (ops.reg_metrics_batch, csrc/regmetrics.hip): pcs1 / pcs2 = lists of [n_p,3] / [m_p,3] clouds or packed tensors plus
    sizes = [(n_p, m_p), ...], pred / gt [P,3,4] or [P,4,4] mapping pc1 to pc2 -> {'rre': rotation_error in degrees (the symmetry fold is the
    caller's), 'rte': translation_error, 'rmse': compute_transformation_error, 'chamfer': chamfer_distance_torch on every
    chamfer_stride-th point}, float64 [P] device tensors evaluated in float64."""
    out = ops.reg_metrics_batch(pcs1, pcs2, pred, gt, chamfer_stride=chamfer_stride, sizes=sizes)
    return {k: out[:, i] for i, k in enumerate(("rre", "rte", "rmse", "chamfer"))}


# ------------------------------------------------------------------------------------------------ reconstruction metrics
def _device():
    return torch.device("cuda", torch.cuda.current_device())


def _points(x, device):
    """[n,3] float64 HIP tensor of numpy / torch points (or an object with .vertices)"""
    x = getattr(x, "vertices", x)
    t = x.detach() if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float64)))
    return t.to(device=device, dtype=torch.float64).reshape(-1, 3).contiguous()


def _device_meshes(meshes, device, one=False):
    """[(V [nv,3] float64, F [nf,3] int32)] on the device; the int64 faces meshes carry are range-checked per mesh (one host read for all of
    them) and narrowed here.  An error names the mesh by its position unless there is only the one."""
    out = []
    for i, mesh in enumerate(meshes):
        V = _points(mesh.vertices, device)
        f = mesh.faces
        F = f.detach().to(device=device, dtype=torch.int64) if torch.is_tensor(f) else torch.from_numpy(np.asarray(f, dtype=np.int64)).to(device)
        if V.shape[0] >= 2 ** 31:
            raise ValueError(f"mesh{'' if one else f' {i}'} has {V.shape[0]} vertices: the mesh operators index vertices with int32 (nv < 2^31)")
        out.append((V, F.reshape(-1, 3)))
    live = [i for i, (_, F) in enumerate(out) if F.numel()]
    if live:
        lim = torch.stack([torch.stack([out[i][1].min(), out[i][1].max()]) for i in live]).cpu().tolist()
        for i, (lo, hi) in zip(live, lim):
            if lo < 0 or hi >= out[i][0].shape[0]:
                raise ValueError(f"mesh{'' if one else f' {i}:'} faces index vertices outside [0, {out[i][0].shape[0]})")
    return [(V, F.to(torch.int32).contiguous()) for V, F in out]


def _device_mesh(mesh, device):
    return _device_meshes([mesh], device, one=True)[0]


def check_mesh_contains(mesh, points, hash_resolution=512):
    """libmesh.check_mesh_contains (occnet_utils/utils/libmesh/inside_mesh.py:5-8): bool [n] numpy array, bit-identical to the reference
    (same float64 operations, same 2-D hash).  A flat mesh (zero extent on an axis) contains nothing, as in the reference."""
    dev = _device()
    P = _points(points, dev)
    V, F = _device_mesh(mesh, dev)
    if P.shape[0] == 0:
        return np.zeros(0, dtype=bool)
    return ops.mesh_contains(V, F, P, hash_resolution).cpu().numpy()


def _sample(mesh, count, seed, device):
    V, F = _device_mesh(mesh, device)
    return ops.mesh_sample(V, F, count, seed)[0]


def _chamfer_means(gt_points, gen, dev):
    """the two directed mean squared nearest-neighbour distances between gt_points and gen [n,3] float64, as float64 scalars on the device"""
    gt = _points(gt_points, dev)
    c = (gt.min(0).values + gt.max(0).values) / 2 if gt.shape[0] else torch.zeros(3, dtype=torch.float64, device=dev)
    a = (gt - c).float().reshape(1, -1, 3, 1).contiguous()
    b = (gen - c).float().reshape(1, -1, 3, 1).contiguous()
    _, d_ab = ops.knn(a, b, 1, return_dist=True)
    _, d_ba = ops.knn(b, a, 1, return_dist=True)
    return d_ab.double().mean(), d_ba.double().mean()


def compute_chamfer_distance(gt_points, gen_mesh, offset, scale, num_mesh_samples=30000, seed=0):
    """evaluate.py:12-40: (gt_to_gen, gen_to_gt) = mean squared nearest-neighbour distance from the points of ``gt_points.vertices`` to
    ``num_mesh_samples`` area-weighted samples of ``gen_mesh`` (moved by ``/ scale - offset``), and back.

    ``seed`` is the one argument the reference does not have: trimesh draws the samples from numpy's unseeded global generator, so the
    reference's value changes from run to run; here the samples are a fixed function of ``seed`` (ls_mesh_sample_f64).  Both clouds are
    centred on the middle of gt's bounding box in float64 before the fp32 nearest-neighbour search (ls_knn_f32, K = 1; distances do not
    change, and scans sit metres from the origin), and the means are accumulated in float64."""
    dev = _device()
    gt_to_gen, gen_to_gt = _chamfer_means(gt_points, _sample(gen_mesh, int(num_mesh_samples), seed, dev) / scale - offset, dev)
    return float(gt_to_gen), float(gen_to_gt)


def mesh_distance(mesh, points, max_dist):
    """[n] float64 numpy: distance from each point to ``mesh`` where it is < max_dist, +inf elsewhere (ls_mesh_distance_f64)."""
    dev = _device()
    P = _points(points, dev)
    V, F = _device_mesh(mesh, dev)
    if P.shape[0] == 0:
        return np.zeros(0)
    return ops.mesh_distance(V, F, P, max_dist).cpu().numpy()


def compute_sdf_recall(mesh1, mesh2, thres=0.1):
    """evaluate.py:100-106: share of ``mesh2.vertices`` whose distance to ``mesh1`` is < thres (|pcu.signed_distance_to_mesh| < thres:
    the sign is never needed).  The reference also computes a Chamfer distance here (:104) and discards it; this one does not."""
    d = mesh_distance(mesh1, mesh2.vertices, thres)
    return float(np.isfinite(d).mean()) if len(d) else float("nan")


def compute_volumetric_iou(mesh1, mesh2, voxel_size=1. / 16):
    """evaluate.py:42-45: share of ``mesh2.vertices`` inside ``mesh1`` (check_mesh_contains); ``voxel_size`` is unused, as in the reference."""
    inside = check_mesh_contains(mesh1, mesh2.vertices)
    return float(inside.mean()) if len(inside) else float("nan")


# ------------------------------------------------------------------------------------------------ the same metrics on many meshes per call
# Element i of every *_batch function equals the per-mesh function on pair i, bit for bit: one ragged device call per metric (csrc/meshmetrics.hip,
# ls_mesh_*_batch_f64) and one host read per batch instead of one per mesh.
def _host_split(parts):
    """per-mesh device results -> per-mesh numpy arrays, one device-to-host copy"""
    if not parts:
        return []
    flat = torch.cat(parts).cpu().numpy()
    return np.split(flat, np.cumsum([p.shape[0] for p in parts])[:-1])


def check_mesh_contains_batch(meshes, points_list, hash_resolution=512):
    """[check_mesh_contains(m, p, hash_resolution) for m, p in zip(meshes, points_list)] in one device call."""
    dev = _device()
    P = [_points(p, dev) for p in points_list]
    return _host_split(ops.mesh_contains_batch(_device_meshes(meshes, dev), P, hash_resolution))


def mesh_distance_batch(meshes, points_list, max_dist):
    """[mesh_distance(m, p, max_dist) for m, p in zip(meshes, points_list)] in one device call."""
    dev = _device()
    P = [_points(p, dev) for p in points_list]
    return _host_split(ops.mesh_distance_batch(_device_meshes(meshes, dev), P, max_dist))


def compute_chamfer_distance_batch(gt_points_list, gen_meshes, offset, scale, num_mesh_samples=30000, seeds=None):
    """[compute_chamfer_distance(g, m, offset, scale, num_mesh_samples, seed) for g, m, seed in zip(gt_points_list, gen_meshes, seeds)]:
    the surface samples of every mesh in one device call, the nearest-neighbour searches one ls_knn_f32 call per mesh (on fresh tensors,
    as the single function makes them), the means read back in one copy.  seeds=None: seed 0 for every mesh.  An empty mesh raises, as
    the single function does."""
    dev = _device()
    M = len(gen_meshes)
    seeds = [0] * M if seeds is None else list(seeds)
    samples = ops.mesh_sample_batch(_device_meshes(gen_meshes, dev), int(num_mesh_samples), seeds)
    means = [torch.stack(_chamfer_means(gt_points, pts / scale - offset, dev)) for gt_points, (pts, _) in zip(gt_points_list, samples)]
    return [tuple(v) for v in torch.stack(means).cpu().tolist()] if means else []


def compute_sdf_recall_batch(meshes1, meshes2, thres=0.1):
    """[compute_sdf_recall(m1, m2, thres) for m1, m2 in zip(meshes1, meshes2)] in one device call."""
    return [float(np.isfinite(d).mean()) if len(d) else float("nan") for d in mesh_distance_batch(meshes1, [m.vertices for m in meshes2], thres)]


def compute_volumetric_iou_batch(meshes1, meshes2, voxel_size=1. / 16):
    """[compute_volumetric_iou(m1, m2) for m1, m2 in zip(meshes1, meshes2)] in one device call."""
    return [float(i.mean()) if len(i) else float("nan") for i in check_mesh_contains_batch(meshes1, [m.vertices for m in meshes2])]


def get_threshold_percentage(dist, thresholds):
    """evaluate.py:88-98: share of ``dist`` <= t for every t in ``thresholds``."""
    dist = np.asarray(dist)
    return [(dist <= t).mean() for t in thresholds]
