"""Mirror of the reference's ``occnet_utils/mesh_extractor2.py``: MISE-driven value grid + marching cubes.

``MISE`` mirrors ``libmise.MISE`` (query / update / to_dense, mise.pyx) with the octree state resident in HBM
(csrc/mise.hip); ``Generator3D.eval_grid`` is the loop of ``__generate_from_latent__`` (mesh_extractor2.py:94-131): per
round the unknown lattice points go straight from the MISE kernels into ``ls_sdf_decode`` and back -- no host round trip
except the 4-byte point count.  ``marching_cubes`` mirrors ``libmcubes.marching_cubes`` (csrc/mcubes.hip: same vertex and
face order, float64 coordinates); ``extract_mesh`` is mesh_extractor2.py:161-214 without normals / refinement (off in the released
settings).  Decimation: ``simplify_mesh_arrays`` is the reference's sequential edge collapse on the host (the default);
``cluster_mesh_arrays`` / ``cluster_mesh_arrays_batch`` are a second decimator on the device (csrc/meshcluster.hip: vertex clustering
with quadric-optimal representatives), chosen with ``Generator3D(simplify_method="cluster")``.
"""
import ctypes
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from ._lib import LsError, call, check, load, ptr, stream_ptr

SIMPLIFY_METHODS = ("collapse", "cluster")


class MISE:
    """libmise.MISE(resolution_0, depth, threshold) on the device.  Points are lattice coordinates [n,3] int64, as in the
    reference; ``query_device`` / ``update_device`` are the zero-copy forms used by Generator3D."""

    def __init__(self, resolution_0, depth, threshold, device="cuda"):
        self.resolution_0, self.depth, self.threshold = int(resolution_0), int(depth), float(threshold)
        self.resolution = self.resolution_0 << self.depth
        self.device = torch.device(device)
        nbytes = load().ls_mise_state_bytes(self.resolution_0, self.depth)
        if nbytes == 0:
            raise ValueError(f"MISE: resolution_0={resolution_0} depth={depth} unsupported")
        self._state = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self._count = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._cap = int(load().ls_mise_lattice_points(self.resolution_0, self.depth))
        self._idx = torch.empty(self._cap, dtype=torch.int32, device=self.device)
        self._pts = torch.empty(self._cap, 3, dtype=torch.float32, device=self.device)
        self.reset()

    def reset(self, threshold=None):
        """Back to the initial lattice (the buffers are kept: a pool of MISE objects serves many instances)."""
        if threshold is not None:
            self.threshold = float(threshold)
        call(self.device, "ls_mise_init", ptr(self._state), self._state.numel(), self.resolution_0, self.depth, stream_ptr(self.device))

    def query_device(self, box_size=1.0):
        """-> (idx [n] int32 lattice indices, pts [n,3] float32 = box_size * (p / resolution - 0.5)), device tensors (views)."""
        call(self.device, "ls_mise_query", ptr(self._state), self.resolution_0, self.depth, float(box_size), ptr(self._idx), ptr(self._pts),
                                   self._cap, ptr(self._count), stream_ptr(self.device))
        n = int(self._count.item())   # the only host round trip of a round
        return self._idx[:n], self._pts[:n]

    def update_device(self, idx, values):
        values = values.to(torch.float32).contiguous()
        idx = idx.to(torch.int32).contiguous()
        assert idx.shape[0] == values.shape[0]
        call(self.device, "ls_mise_update", ptr(self._state), self.resolution_0, self.depth, ctypes.c_double(self.threshold), ptr(idx),
                                    ptr(values), int(idx.shape[0]), stream_ptr(self.device))

    # ---- the reference's host-side surface (mise.pyx:87-165)
    def query(self):
        idx, _ = self.query_device()
        G = self.resolution + 1
        i = idx.long().cpu().numpy()
        return np.stack([i // (G * G), (i // G) % G, i % G], 1).astype(np.int64)

    def update(self, points, values):
        points = np.asarray(points, np.int64)
        G = self.resolution + 1
        idx = torch.from_numpy(((points[:, 0] * G + points[:, 1]) * G + points[:, 2]).astype(np.int32)).to(self.device)
        self.update_device(idx, torch.as_tensor(np.asarray(values, np.float32)).to(self.device))

    def to_dense_device(self):
        G = self.resolution + 1
        out = torch.empty(G, G, G, dtype=torch.float32, device=self.device)
        call(self.device, "ls_mise_to_dense", ptr(self._state), self.resolution_0, self.depth, ptr(out), stream_ptr(self.device))
        return out

    def to_dense(self):
        return self.to_dense_device().cpu().numpy().astype(np.float64)


class MISEBatch:
    """B octrees of one (resolution_0, depth, threshold) advancing in lock-step (csrc/mise.hip, the *_batch ops): a round is one query, one
    decoder call on (pts, inst) as they come out of the query, one update -- the number of launches does not depend on B.  The state is B
    ``MISE`` states back to back; every octree evolves exactly as a ``MISE`` of its own would."""

    def __init__(self, B, resolution_0, depth, threshold, device="cuda"):
        self.B, self.resolution_0, self.depth, self.threshold = int(B), int(resolution_0), int(depth), float(threshold)
        self.resolution = self.resolution_0 << self.depth
        self.device = torch.device(device)
        nbytes = load().ls_mise_batch_state_bytes(self.B, self.resolution_0, self.depth)
        if nbytes == 0:
            raise ValueError(f"MISEBatch: B={B} resolution_0={resolution_0} depth={depth} unsupported")
        self._state = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self._off = torch.zeros(self.B + 1, dtype=torch.int64, device=self.device)
        self._cap = self.B * int(load().ls_mise_lattice_points(self.resolution_0, self.depth))
        self._idx = torch.empty(self._cap, dtype=torch.int32, device=self.device)
        self._inst = torch.empty(self._cap, dtype=torch.int32, device=self.device)
        self._pts = torch.empty(self._cap, 3, dtype=torch.float32, device=self.device)
        self.reset()

    def reset(self, threshold=None):
        """Back to the initial lattice (the buffers are kept: one MISEBatch serves many batches)."""
        if threshold is not None:
            self.threshold = float(threshold)
        call(self.device, "ls_mise_init_batch", ptr(self._state), self._state.numel(), self.B, self.resolution_0, self.depth,
             stream_ptr(self.device))

    def query_device(self, box_size=1.0):
        """-> (idx [n] int32 lattice index within the octree, inst [n] int32 octree, pts [n,3] float32, offsets): device tensors (views), octree
        after octree; ``offsets`` is a host list of B+1 integers (rows of octree b: offsets[b]:offsets[b+1]) -- the round's only host read."""
        call(self.device, "ls_mise_query_batch", ptr(self._state), self.B, self.resolution_0, self.depth, float(box_size), ptr(self._idx),
             ptr(self._inst), ptr(self._pts), self._cap, ptr(self._off), stream_ptr(self.device))
        offsets = self._off.cpu().tolist()
        n = offsets[-1]
        return self._idx[:n], self._inst[:n], self._pts[:n], offsets

    def update_device(self, idx, inst, values):
        values = values.to(torch.float32).contiguous()
        idx, inst = idx.to(torch.int32).contiguous(), inst.to(torch.int32).contiguous()
        assert idx.shape[0] == values.shape[0] == inst.shape[0]
        call(self.device, "ls_mise_update_batch", ptr(self._state), self.B, self.resolution_0, self.depth, ctypes.c_double(self.threshold),
             ptr(idx), ptr(inst), ptr(values), int(idx.shape[0]), stream_ptr(self.device))

    def to_dense_device(self):
        G = self.resolution + 1
        out = torch.empty(self.B, G, G, G, dtype=torch.float32, device=self.device)
        call(self.device, "ls_mise_to_dense_batch", ptr(self._state), self.B, self.resolution_0, self.depth, ptr(out), stream_ptr(self.device))
        return out


class Generator3D:
    """mesh_extractor2.py:17-58 (constructor arguments kept); ``eval_grid`` = everything of ``__generate_from_latent__`` before
    ``extract_mesh``."""

    def __init__(self, points_batch_size=100000, threshold=0.5, refinement_step=0, resolution0=16, upsampling_steps=3,
                 with_normals=False, padding=0.1, sample=False, simplify_nfaces=None, simplify_method="collapse"):
        """simplify_method (an extension): how a mesh is decimated to simplify_nfaces faces.  "collapse" (the default) is the reference's
        quadric edge collapse on the host, bit-identical to it; "cluster" is the device decimator (cluster_mesh_arrays): vertex clustering
        on the packed marching-cubes output, only the decimated mesh travels to the host.  It is never chosen implicitly: two sheets closer
        than one grid cell cancel, so thin parts can vanish where the edge collapse keeps them."""
        if simplify_method not in SIMPLIFY_METHODS:
            raise ValueError(f"Generator3D: simplify_method must be one of {SIMPLIFY_METHODS}, got {simplify_method!r}")
        self.simplify_method = simplify_method
        self.implicit_F = None
        self.device = "cuda"
        self.points_batch_size = points_batch_size
        self.refinement_step = refinement_step
        self.threshold = threshold
        self.resolution0 = resolution0
        self.upsampling_steps = upsampling_steps
        self.with_normals = with_normals
        self.padding = padding
        self.sample = sample
        self.simplify_nfaces = simplify_nfaces

    def eval_points(self, p, z, c=None, **kwargs):
        """mesh_extractor2.py:136-159: logits at points p [n,3] (device tensor), in chunks of points_batch_size."""
        outs = []
        for pi in torch.split(p, self.points_batch_size):
            with torch.no_grad():
                outs.append(self.implicit_F(pi.unsqueeze(0), z, c, **kwargs).logits.squeeze(0))
        return torch.cat(outs, 0) if outs else p.new_zeros(0)

    def eval_grid(self, c, F, stats_dict=None, on_device=False, **kwargs):
        """-> value grid float64 [(R+1)^3] as numpy (what the reference hands to marching cubes), R = resolution0 << steps.
        on_device=True (used by generate_from_latent): the same values as a float64 DEVICE tensor -- the 129^3 grid (17 MB) does not
        travel to the host and back between the octree and the marching cubes kernels."""
        self.implicit_F = F
        z = torch.zeros(1, 0, device=self.device)
        threshold = np.log(self.threshold) - np.log(1.0 - self.threshold)
        box_size = 1 + self.padding
        if self.upsampling_steps == 0:
            nx = self.resolution0
            lin = torch.linspace(-0.5, 0.5, nx, device=self.device)
            g = torch.stack(torch.meshgrid(lin, lin, lin, indexing="ij"), -1).reshape(-1, 3)   # make_3d_grid, common.py:157
            dense = self.eval_points(box_size * g, z, c, **kwargs).reshape(nx, nx, nx)
            return dense.to(torch.float64) if on_device else dense.cpu().numpy().astype(np.float64)
        mise = MISE(self.resolution0, self.upsampling_steps, threshold, device=self.device)
        rounds = []
        idx, pts = mise.query_device(box_size)
        while idx.shape[0] != 0:
            rounds.append(int(idx.shape[0]))
            mise.update_device(idx, self.eval_points(pts, z, c, **kwargs))
            idx, pts = mise.query_device(box_size)
        if stats_dict is not None:
            stats_dict["mise rounds"] = rounds
        return mise.to_dense_device().to(torch.float64) if on_device else mise.to_dense()

    def eval_grid_batch(self, codes, F, on_device=False):
        """Value grids of SEVERAL instances at once (an extension: the reference extracts one mesh at a time).  codes: dict of
        [B,...] tensors.  All MISE octrees advance in lock-step (MISEBatch); each round the unknown points of every instance go into
        ONE ragged decoder call (ls_sdf_decode_rows), so the small late rounds and the per-round host round trip are shared.
        Returns a list of B float64 grids, each bit-identical to ``eval_grid`` on that instance."""
        dense = self._eval_grid_batch_device(codes, F)
        if on_device:
            return list(dense.to(torch.float64))
        return list(dense.cpu().numpy().astype(np.float64))

    def _eval_grid_batch_device(self, codes, F):
        """eval_grid_batch as ONE float32 device tensor [B,G,G,G] (the float64 grids hold float32 values)."""
        assert self.upsampling_steps > 0, "eval_grid_batch: MISE path only"
        B = codes["z_inv"].shape[0]
        threshold = np.log(self.threshold) - np.log(1.0 - self.threshold)
        box_size = 1 + self.padding
        hip = F._owner().hip_model()
        key = (B, self.resolution0, self.upsampling_steps)
        cache = self.__dict__.setdefault("_mise_batches", {})
        if key not in cache:
            cache[key] = MISEBatch(B, self.resolution0, self.upsampling_steps, threshold, device=self.device)
        mise = cache[key]
        mise.reset(threshold)
        while True:
            idx, inst, pts, offsets = mise.query_device(box_size)
            if offsets[-1] == 0:
                break
            sdf = hip.sdf_decode_rows(pts, inst, codes["z_so3"], codes["z_inv"], codes["s"], codes["t"])
            mise.update_device(idx, inst, F.sdf2occ_factor * sdf)
        return mise.to_dense_device()

    def generate_from_latent_batch(self, codes, F, threads=None):
        """Meshes of B codes: batched MISE rounds, one batched marching cubes, then the decimation of every non-empty mesh on a thread
        pool (simplify_mesh_arrays_batch; ``threads`` as there).  Mesh i equals extract_mesh of instance i's grid.  With
        simplify_method "cluster" the packed marching-cubes output is decimated on the device in one call and ``threads`` is ignored."""
        arrays = self._mc_arrays_batch(self._eval_grid_batch_device(codes, F), cluster=self._clusters())
        if self._clusters():
            return [make_mesh(v, t) for v, t in arrays]
        if self.simplify_nfaces is not None:             # :205-208, an empty mesh is returned as it is (:196-197)
            live = [i for i, (v, _) in enumerate(arrays) if v.shape[0] != 0]
            for i, vf in zip(live, simplify_mesh_arrays_batch([arrays[i] for i in live], self.simplify_nfaces, 5.0, threads=threads)):
                arrays[i] = vf
        return [make_mesh(v, t) for v, t in arrays]

    def generate_from_latent(self, c, F, **kwargs):
        """mesh_extractor2.py:60-74."""
        return self.extract_mesh(self.eval_grid(c, F, on_device=True, **kwargs), None, c)

    def extract_mesh(self, occ_hat, z, c=None, stats_dict=None):
        """mesh_extractor2.py:161-214: pad with -1e6 (watertight), marching cubes at the logit threshold, undo the library's 0.5
        shift and the padding, normalise to the bounding box."""
        vertices, triangles = self._mc_arrays(occ_hat, cluster=self._clusters())
        if vertices.shape[0] == 0:                       # mesh_extractor2.py:196-197: an empty mesh is returned as it is
            return make_mesh(vertices, triangles)
        if self.simplify_nfaces is not None and not self._clusters():   # :205-208 -- the released configs set 5000 / 100000
            vertices, triangles = simplify_mesh_arrays(vertices, triangles, self.simplify_nfaces, 5.0)
        return make_mesh(vertices, triangles)

    def _clusters(self):
        return self.simplify_nfaces is not None and self.simplify_method == "cluster"

    def _mc_arrays(self, occ_hat, cluster=False):
        """extract_mesh up to the decimation: (vertices float64 [nv,3], faces int64 [nf,3]) numpy, in the normalised frame.
        cluster=True: decimated on the device to simplify_nfaces faces, in the marching-cubes frame (the normalisation is a uniform scale
        and a shift, so the cells correspond), before the copy to the host."""
        self._refuse_normals_and_refinement()
        n_x, n_y, n_z = occ_hat.shape
        box_size = 1 + self.padding
        threshold = np.log(self.threshold) - np.log(1.0 - self.threshold)
        if torch.is_tensor(occ_hat) and occ_hat.is_cuda:
            vol = occ_hat.to(torch.float64)              # grid still on the device (generate_from_latent)
        else:
            vol = torch.as_tensor(np.asarray(occ_hat, np.float64), device=self.device)
        vol = torch.nn.functional.pad(vol, (1, 1, 1, 1, 1, 1), value=-1e6)
        vertices, triangles = marching_cubes(vol, threshold)
        if cluster:
            vertices, triangles = cluster_mesh_arrays(vertices, triangles, self.simplify_nfaces)
        return self._normalise_vertices(vertices.cpu().numpy(), (n_x, n_y, n_z)), triangles.cpu().numpy()

    def _mc_arrays_batch(self, grids, cluster=False):
        """[_mc_arrays(g, cluster) for g in grids] for B device grids of one shape ([B,nx,ny,nz] tensor or a list of [nx,ny,nz] tensors): one
        padding call, one batched marching cubes (marching_cubes_batch), with cluster=True one batched decimation of the packed meshes, one
        copy of the packed vertices and faces to the host."""
        self._refuse_normals_and_refinement()
        vol = grids if torch.is_tensor(grids) else torch.stack(list(grids))
        if not vol.is_cuda:
            raise ValueError("_mc_arrays_batch: the grids must live on the GPU (no CPU fallback)")
        assert vol.dim() == 4, "_mc_arrays_batch: [B,nx,ny,nz]"
        threshold = np.log(self.threshold) - np.log(1.0 - self.threshold)
        vol = torch.nn.functional.pad(vol.to(torch.float64), (1, 1, 1, 1, 1, 1), value=-1e6)
        verts, faces, vo, fo = _marching_cubes_packed(vol, threshold)
        if cluster and vo[-1]:
            verts, faces, vo, fo, _ = _cluster_packed(verts, vo, faces, fo, self.simplify_nfaces, 256)
        verts, faces = self._normalise_vertices(verts.cpu().numpy(), grids[0].shape), faces.cpu().numpy()   # element-wise: the same on a slice
        return [(verts[vo[b]:vo[b + 1]], faces[fo[b]:fo[b + 1]]) for b in range(vol.shape[0])]

    def _normalise_vertices(self, vertices, shape):
        """mesh_extractor2.py:178-186: undo the library's 0.5 shift and the padding, normalise to the bounding box (in place)."""
        n_x, n_y, n_z = shape
        box_size = 1 + self.padding
        vertices -= 0.5
        vertices -= 1
        vertices /= np.array([n_x - 1, n_y - 1, n_z - 1])
        vertices = box_size * (vertices - 0.5)
        return vertices

    def _refuse_normals_and_refinement(self):
        if self.with_normals or self.refinement_step > 0:
            # Off in every released configuration (configs/more_3rscan.yaml:19-26, room4cates.yaml:32-39) -- and not runnable in the reference on this call
            # path either: generate_from_latent hands the code DICT on as `c`, estimate_normals does `c.unsqueeze(0)` (mesh_extractor2.py:231: AttributeError
            # on a dict) and refine_mesh starts with `self.model.eval()` (:257), an attribute Generator3D never sets (OccNet leftovers).  There is no reference
            # behaviour to reproduce, so the switch is refused loudly instead of inventing one.
            raise NotImplementedError("with_normals / refinement_step > 0: off in every released configuration and broken in the reference on the "
                                      "generate_from_latent path (mesh_extractor2.py:231 c.unsqueeze on the code dict, :257 self.model) -- nothing to reproduce")


def marching_cubes(volume, isovalue):
    """libmcubes.marching_cubes(volume [nx,ny,nz], isovalue) on the device -> (vertices [nv,3] float64, faces [nf,3] int64),
    device tensors, in the reference's vertex / face order (coordinates carry the library's +0.5 offset)."""
    vol = torch.as_tensor(volume)
    if not vol.is_cuda:
        raise ValueError("marching_cubes: the volume must live on the GPU (no CPU fallback)")
    vol = vol.to(torch.float64).contiguous()
    assert vol.dim() == 3, "Only three-dimensional arrays are supported."
    nx, ny, nz = vol.shape
    iso = float(np.float32(isovalue))   # mcubes.pyx:22 declares `float isovalue`
    dev = vol.device
    ws_bytes = load().ls_mcubes_workspace_bytes(nx, ny, nz)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    args = (ptr(vol), nx, ny, nz, ctypes.c_double(iso))
    call(dev, "ls_marching_cubes_f64", *args, None, 0, None, 0, ptr(counts), ptr(ws), ws_bytes, stream_ptr(dev))
    nv, nf = (int(v) for v in counts.cpu())
    verts = torch.empty(nv, 3, dtype=torch.float64, device=dev)
    faces = torch.empty(nf, 3, dtype=torch.int64, device=dev)
    if nv:
        call(dev, "ls_marching_cubes_f64", *args, ptr(verts), nv, ptr(faces), nf, ptr(counts), ptr(ws), ws_bytes, stream_ptr(dev))
    return verts, faces


def marching_cubes_batch(volumes, isovalue):
    """[marching_cubes(v, isovalue) for v in volumes] for a device tensor [B,nx,ny,nz] in one batched call (csrc/mcubes.hip,
    ls_marching_cubes_batch_f64) -> list of B (vertices [nv,3] float64, faces [nf,3] int64), device tensors (views of the packed outputs),
    each bit-identical to the single op: one sizing call, ONE host read of the offsets, one real call."""
    verts, faces, vo, fo = _marching_cubes_packed(volumes, isovalue)
    return [(verts[vo[b]:vo[b + 1]], faces[fo[b]:fo[b + 1]]) for b in range(len(vo) - 1)]


def _marching_cubes_packed(volumes, isovalue):
    """-> (vertices [sum nv,3], faces [sum nf,3], vertex offsets, face offsets): the meshes one after the other, offsets as host lists of B+1."""
    vol = torch.as_tensor(volumes)
    if not vol.is_cuda:
        raise ValueError("marching_cubes_batch: the volumes must live on the GPU (no CPU fallback)")
    vol = vol.to(torch.float64).contiguous()
    assert vol.dim() == 4, "marching_cubes_batch: [B,nx,ny,nz]"
    B, nx, ny, nz = vol.shape
    iso = float(np.float32(isovalue))   # mcubes.pyx:22 declares `float isovalue`
    dev = vol.device
    ws_bytes = load().ls_mcubes_batch_workspace_bytes(B, nx, ny, nz)
    if ws_bytes == 0:
        raise ValueError(f"marching_cubes_batch: B={B} volumes of {nx} x {ny} x {nz} unsupported (include/livingscenes_hip.h: limits)")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    off = torch.zeros(2, B + 1, dtype=torch.int64, device=dev)
    args = (ptr(vol), B, nx, ny, nz, ctypes.c_double(iso))
    call(dev, "ls_marching_cubes_batch_f64", *args, None, 0, None, 0, ptr(off), ptr(ws), ws_bytes, stream_ptr(dev))
    vo, fo = off.cpu().tolist()
    verts = torch.empty(vo[B], 3, dtype=torch.float64, device=dev)
    faces = torch.empty(fo[B], 3, dtype=torch.int64, device=dev)
    if vo[B]:
        call(dev, "ls_marching_cubes_batch_f64", *args, ptr(verts), vo[B], ptr(faces), fo[B], ptr(off), ptr(ws), ws_bytes, stream_ptr(dev))
    return verts, faces, vo, fo


def _cluster_caps(nv, nf, f_target):
    """Bounds on a mesh's output that need no sizing call: a mesh under the target is copied, else at most f_target faces remain and every
    output vertex is both a corner of one of them and the cell of an input vertex."""
    if nf <= f_target:
        return nv, nf
    return min(nv, 3 * f_target), f_target


def _cluster_inputs(vertices, faces, f_target, r_max, what):
    V, F = torch.as_tensor(vertices), torch.as_tensor(faces)
    if not (V.is_cuda and F.is_cuda):
        raise ValueError(f"{what}: vertices and faces must live on the GPU (no CPU fallback; simplify_mesh_arrays is the host decimator)")
    f_target, r_max = int(f_target), int(r_max)
    if f_target < 1 or not 1 <= r_max <= 256:
        raise ValueError(f"{what}: f_target >= 1 and 1 <= r_max <= 256, got {f_target}, {r_max}")
    return V.to(torch.float64).reshape(-1, 3).contiguous(), F.to(torch.int64).reshape(-1, 3).contiguous(), f_target, r_max


def _cluster_status(what, r):
    for m, rm in enumerate(r):
        if rm < 0:
            raise LsError(f"{what}: mesh {m}: " + {-1: "a face index outside the mesh's vertices, or outputs too small",
                                                   -3: "the face hash overflowed"}.get(rm, f"status {rm}"))


def cluster_mesh_arrays(vertices, faces, f_target, r_max=256, return_r=False):
    """Decimation on the device (csrc/meshcluster.hip, ls_mesh_cluster_f64; include/livingscenes_hip.h holds the definition): vertex
    clustering on the finest uniform grid of at most r_max cells per axis that leaves at most f_target faces, one quadric-optimal vertex
    per cell.  vertices [nv,3], faces [nf,3] device tensors -> (vertices [nv',3] float64, faces [nf',3] int64) device tensors
    (return_r: and the grid resolution r, 0 when nf <= f_target and the mesh is returned unchanged).  Deterministic: the same bits alone,
    in a batch and in any run.  Not the reference's edge collapse: sheets closer than one cell cancel and thin parts can vanish."""
    V, F, f_target, r_max = _cluster_inputs(vertices, faces, f_target, r_max, "cluster_mesh_arrays")
    dev = V.device
    nv, nf = V.shape[0], F.shape[0]
    ws_bytes = load().ls_mesh_cluster_workspace_bytes(nv, nf, r_max)
    if ws_bytes == 0:
        raise ValueError(f"cluster_mesh_arrays: {nv} vertices, {nf} faces unsupported (include/livingscenes_hip.h: limits)")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    cap_v, cap_f = _cluster_caps(nv, nf, f_target)
    verts = torch.empty(max(cap_v, 1), 3, dtype=torch.float64, device=dev)
    tris = torch.empty(max(cap_f, 1), 3, dtype=torch.int64, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    r = torch.zeros(1, dtype=torch.int32, device=dev)
    call(dev, "ls_mesh_cluster_f64", ptr(V), nv, ptr(F), nf, f_target, r_max, ptr(verts), cap_v, ptr(tris), cap_f, ptr(counts), ptr(r), ptr(ws),
         ws_bytes, stream_ptr(dev))
    (nvo, nfo), r = counts.cpu().tolist(), int(r.cpu())   # the call's host read
    _cluster_status("cluster_mesh_arrays", [r])
    return (verts[:nvo], tris[:nfo], r) if return_r else (verts[:nvo], tris[:nfo])


def cluster_mesh_arrays_batch(meshes, f_target, r_max=256, offsets=None, return_r=False):
    """[cluster_mesh_arrays(v, f, f_target, r_max) for v, f in meshes] in ONE call (ls_mesh_cluster_batch_f64: the number of launches does
    not depend on the number of meshes), every mesh bit-identical to the single call.  meshes: a list of (vertices, faces) device tensors
    (or objects with .vertices / .faces), or -- with offsets = (vertex offsets, face offsets), host sequences of M + 1 integers -- the pair
    (vertices [sum nv,3], faces [sum nf,3]) packed mesh after mesh with indices local to each mesh.  -> list of M (vertices, faces) device
    tensors, views of the packed outputs (return_r: and the list of the M resolutions)."""
    if offsets is None:
        pairs = [(m.vertices, m.faces) if hasattr(m, "vertices") else tuple(m) for m in meshes]
        if not pairs:
            return ([], []) if return_r else []
        Vs = [torch.as_tensor(v).reshape(-1, 3) for v, _ in pairs]
        Fs = [torch.as_tensor(f).reshape(-1, 3) for _, f in pairs]
        V, F = torch.cat([v.to(torch.float64) for v in Vs], 0), torch.cat([f.to(torch.int64) for f in Fs], 0)
        vo = np.concatenate([[0], np.cumsum([v.shape[0] for v in Vs])]).tolist()
        fo = np.concatenate([[0], np.cumsum([f.shape[0] for f in Fs])]).tolist()
    else:
        V, F = meshes
        vo, fo = ([int(x) for x in o] for o in offsets)
        if len(vo) != len(fo) or len(vo) < 1:
            raise ValueError(f"cluster_mesh_arrays_batch: {len(vo)} vertex offsets, {len(fo)} face offsets")
        if len(vo) == 1:
            return ([], []) if return_r else []
    verts, tris, ovo, ofo, r = _cluster_packed(V, vo, F, fo, f_target, r_max)
    out = [(verts[ovo[m]:ovo[m + 1]], tris[ofo[m]:ofo[m + 1]]) for m in range(len(vo) - 1)]
    return (out, r) if return_r else out


def _cluster_packed(vertices, vert_off, faces, face_off, f_target, r_max):
    """M >= 1 packed meshes (host offsets) -> (vertices, faces, vertex offsets, face offsets, r): the decimated meshes packed the same way,
    offsets and resolutions as host lists.  One call, sized by _cluster_caps, and one host read."""
    V, F, f_target, r_max = _cluster_inputs(vertices, faces, f_target, r_max, "cluster_mesh_arrays_batch")
    dev = V.device
    M = len(vert_off) - 1
    vo, fo = np.ascontiguousarray(vert_off, np.int64), np.ascontiguousarray(face_off, np.int64)
    ws_bytes = load().ls_mesh_cluster_batch_workspace_bytes(M, V.shape[0], F.shape[0], r_max)
    if ws_bytes == 0:
        raise ValueError(f"cluster_mesh_arrays_batch: {M} meshes, {V.shape[0]} vertices, {F.shape[0]} faces unsupported "
                         "(include/livingscenes_hip.h: limits)")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    caps = [_cluster_caps(int(vo[m + 1] - vo[m]), int(fo[m + 1] - fo[m]), f_target) for m in range(M)]
    cap_v, cap_f = sum(c[0] for c in caps), sum(c[1] for c in caps)
    verts = torch.empty(max(cap_v, 1), 3, dtype=torch.float64, device=dev)
    tris = torch.empty(max(cap_f, 1), 3, dtype=torch.int64, device=dev)
    off = torch.zeros(2, M + 1, dtype=torch.int64, device=dev)
    r = torch.zeros(M, dtype=torch.int32, device=dev)
    P = ctypes.c_void_p
    call(dev, "ls_mesh_cluster_batch_f64", M, ptr(V), V.shape[0], P(vo.ctypes.data), ptr(F), F.shape[0], P(fo.ctypes.data), f_target, r_max,
         ptr(verts), cap_v, ptr(tris), cap_f, ptr(off), ptr(r), ptr(ws), ws_bytes, stream_ptr(dev))
    (ovo, ofo), r = off.cpu().tolist(), r.cpu().tolist()   # the call's host read
    _cluster_status("cluster_mesh_arrays_batch", r)
    return verts[:ovo[M]], tris[:ofo[M]], ovo, ofo, r


def simplify_mesh_arrays(vertices, faces, f_target=10000, agressiveness=7.0, initial_border=1):
    """libsimplify.mesh_simplify (simplify_mesh.pyx:34-88): quadric edge-collapse decimation to f_target faces -> (vertices
    float64 [nv',3], faces int64 [nf',3]), bit-identical to the reference (csrc/simplify.cpp; host code, as in the reference).
    initial_border=1 reproduces the reference as it actually runs (its uninitialised Vertex::border reads non-zero while the
    initial edge costs are computed, see csrc/simplify.cpp); 0 is the algorithm as published."""
    v = np.ascontiguousarray(vertices, np.float64)
    f = np.ascontiguousarray(faces, np.int64)
    vo, fo = np.empty_like(v), np.empty_like(f)
    counts = np.zeros(2, np.int64)
    P = ctypes.c_void_p
    check(load().ls_simplify_mesh_f64_host(P(v.ctypes.data), v.shape[0], P(f.ctypes.data), f.shape[0], int(f_target), float(agressiveness),
                                           int(initial_border), P(vo.ctypes.data), P(fo.ctypes.data), P(counts.ctypes.data)), "ls_simplify_mesh_f64_host")
    return vo[: counts[0]].copy(), fo[: counts[1]].copy()


def default_threads():
    """Host threads of simplify_mesh_arrays_batch: OMP_NUM_THREADS when set, else min(16, the CPUs this process may run on)."""
    env = os.environ.get("OMP_NUM_THREADS", "").strip()
    if env:
        return max(1, int(env))
    return min(16, len(os.sched_getaffinity(0)))


def simplify_mesh_arrays_batch(meshes, f_target, agressiveness=7.0, threads=None):
    """[simplify_mesh_arrays(v, f, f_target, agressiveness) for v, f in meshes] on a pool of ``threads`` host threads (None:
    default_threads()).  The meshes are independent and the decimation keeps no shared state (ctypes releases the GIL during the call),
    so the result does not depend on the thread count.  meshes: (vertices, faces) pairs or objects with .vertices / .faces."""
    pairs = [(m.vertices, m.faces) if hasattr(m, "vertices") else tuple(m) for m in meshes]
    n = default_threads() if threads is None else int(threads)
    if n < 1:
        raise ValueError(f"simplify_mesh_arrays_batch: threads must be >= 1, got {n}")
    load()   # resolve the library once, before the workers use it
    if n == 1 or len(pairs) <= 1:
        return [simplify_mesh_arrays(v, f, f_target, agressiveness) for v, f in pairs]
    with ThreadPoolExecutor(max_workers=min(n, len(pairs))) as ex:
        return list(ex.map(lambda vf: simplify_mesh_arrays(vf[0], vf[1], f_target, agressiveness), pairs))


def simplify_mesh(mesh, f_target=10000, agressiveness=7.0):
    """occnet_utils/utils/libsimplify/__init__.py:7-17 (same name and arguments): mesh in, simplified mesh out."""
    v, f = simplify_mesh_arrays(mesh.vertices, mesh.faces, f_target, agressiveness)
    return make_mesh(v, f)


class SimpleMesh:
    """Stand-in for trimesh.Trimesh(vertices, faces, process=False) when trimesh is not installed."""

    def __init__(self, vertices, faces):
        self.vertices, self.faces = np.asarray(vertices, np.float64), np.asarray(faces, np.int64)

    def export_obj(self, path):
        with open(path, "w") as f:
            for v in self.vertices:
                f.write(f"v {v[0]:.9g} {v[1]:.9g} {v[2]:.9g}\n")
            for t in self.faces:
                f.write(f"f {t[0] + 1} {t[1] + 1} {t[2] + 1}\n")


def make_mesh(vertices, faces):
    try:
        import trimesh
        return trimesh.Trimesh(vertices, faces, process=False)   # mesh_extractor2.py:193
    except ImportError:
        return SimpleMesh(vertices, faces)
