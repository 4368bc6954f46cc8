"""The NumPy twin of the depth renderer and its back-projection: the definition of include/livingscenes_hip.h (ls_mesh_render_depth_f64,
ls_depth_points_f32) as plain loops over the faces, vectorised over a face's pixel box.  float64 and int64 throughout, every product and sum
rounded on its own (NumPy never contracts), so the kernels of csrc/meshrender.hip are held to it bit for bit."""
import numpy as np

SUB = 256
SNAP_MAX = 1 << 24
NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)


def snap(u):
    """step 4 for one value -> (ok, int): floor(u 256 + 0.5) as an integer, refused when not finite or beyond 2^24 in magnitude"""
    with np.errstate(all="ignore"):
        t = np.floor(np.float64(u) * np.float64(SUB) + np.float64(0.5))
    if not (np.abs(t) <= SNAP_MAX):
        return False, 0
    return True, int(t)


def pixel_box(xs, ys, W, H):
    """step 5 -> (x0, x1, y0, y1) clipped to the image, or None when it is empty.  Python's // floors for negative integers."""
    x0, x1 = max(-((-min(xs)) // SUB), 0), min(max(xs) // SUB, W - 1)
    y0, y1 = max(-((-min(ys)) // SUB), 0), min(max(ys) // SUB, H - 1)
    if x0 > x1 or y0 > y1:
        return None
    return x0, x1, y0, y1


def edge(xs, ys, i, j, X, Y):
    return (xs[j] - xs[i]) * (Y - ys[i]) - (ys[j] - ys[i]) * (X - xs[i])


def area2(xs, ys):
    return edge(xs, ys, 1, 2, 0, 0) + edge(xs, ys, 2, 0, 0, 0) + edge(xs, ys, 0, 1, 0, 0)


def face_setup(tri, E, K, W, H, znear):
    """steps 1 - 5 of one (view, face): tri [3,3] -> (state, xs, ys, iz, box), state in 'near', 'snap', 'flat', 'empty', 'raster'"""
    fx, fy, cx, cy = (np.float64(k) for k in K)
    E = np.asarray(E, np.float64)
    c = np.empty((3, 3))
    with np.errstate(all="ignore"):
        for i in range(3):
            x, y, z = (np.float64(t) for t in tri[i])
            c[i] = ((E[:, 0] * x + E[:, 1] * y) + E[:, 2] * z) + E[:, 3]
        if any((not np.isfinite(c[i, 2])) or c[i, 2] < znear for i in range(3)):
            return "near", None, None, None, None
        u = [fx * (c[i, 0] / c[i, 2]) + cx for i in range(3)]
        v = [fy * (c[i, 1] / c[i, 2]) + cy for i in range(3)]
        iz = [np.float64(1.0) / c[i, 2] for i in range(3)]
    sx, sy = [snap(t) for t in u], [snap(t) for t in v]
    if not all(ok for ok, _ in sx + sy):
        return "snap", None, None, None, None
    xs, ys = [t for _, t in sx], [t for _, t in sy]
    if area2(xs, ys) == 0:
        return "flat", xs, ys, iz, None
    box = pixel_box(xs, ys, W, H)
    return ("raster" if box else "empty"), xs, ys, iz, box


def render(V, F, E, K, H, W, znear=0.05):
    """V [nv,3], F [nf,3], E [views,3,4], K [views,4] -> depth [views,H,W] float32, face [views,H,W] int32, counts [views,4] int64"""
    V, F = np.asarray(V, np.float64).reshape(-1, 3), np.asarray(F, np.int64).reshape(-1, 3)
    E, K = np.asarray(E, np.float64).reshape(-1, 3, 4), np.asarray(K, np.float64).reshape(-1, 4)
    views = E.shape[0]
    if F.size and (F.min() < 0 or F.max() >= V.shape[0]):
        raise ValueError("a face names a vertex outside the mesh")
    keys = np.full((views, H, W), NO_KEY, np.uint64)
    counts = np.zeros((views, 4), np.int64)
    for w in range(views):
        for f in range(F.shape[0]):
            state, xs, ys, iz, box = face_setup(V[F[f]], E[w], K[w], W, H, znear)
            if state == "near":
                counts[w, 2] += 1
            elif state == "snap":
                counts[w, 3] += 1
            if state in ("empty", "raster"):
                counts[w, 1] += 1
            if state != "raster":
                continue
            x0, x1, y0, y1 = box
            Y, X = np.meshgrid(np.arange(y0, y1 + 1, dtype=np.int64) * SUB, np.arange(x0, x1 + 1, dtype=np.int64) * SUB, indexing="ij")
            e0, e1, e2 = edge(xs, ys, 1, 2, X, Y), edge(xs, ys, 2, 0, X, Y), edge(xs, ys, 0, 1, X, Y)
            A = e0 + e1 + e2
            cov = (A != 0) & (((e0 >= 0) & (e1 >= 0) & (e2 >= 0)) | ((e0 <= 0) & (e1 <= 0) & (e2 <= 0)))
            with np.errstate(all="ignore"):
                z = A.astype(np.float64) / ((e0.astype(np.float64) * iz[0] + e1.astype(np.float64) * iz[1]) + e2.astype(np.float64) * iz[2])
                d = z.astype(np.float32)
            key = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(f)
            sub = keys[w, y0:y1 + 1, x0:x1 + 1]
            take = cov & (key < sub)
            sub[take] = key[take]
    hit = keys != NO_KEY
    depth = np.where(hit, (keys >> np.uint64(32)).astype(np.uint32).view(np.float32), np.float32(0))
    face = np.where(hit, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    counts[:, 0] = hit.reshape(views, -1).sum(1)
    return depth.astype(np.float32), face, counts


def depth_points(depth, K, M=None):
    """depth [views,H,W] float32, K [views,4], M [views,3,4] or None -> pts [n,3] float32, pix [n] int32, off [views+1] int64"""
    depth = np.asarray(depth, np.float32)
    views, H, W = depth.shape
    K = np.asarray(K, np.float64).reshape(views, 4)
    pts, pix, off = [], [], [0]
    for w in range(views):
        py, px = np.where(depth[w] > 0)
        d = depth[w][py, px].astype(np.float64)
        fx, fy, cx, cy = K[w]
        xc = ((px.astype(np.float64) - cx) / fx) * d
        yc = ((py.astype(np.float64) - cy) / fy) * d
        zc = d
        if M is None:
            p = np.stack([xc, yc, zc], 1)
        else:
            m = np.asarray(M, np.float64).reshape(views, 3, 4)[w]
            p = np.stack([((m[r, 0] * xc + m[r, 1] * yc) + m[r, 2] * zc) + m[r, 3] for r in range(3)], 1)
        pts.append(p.astype(np.float32))
        pix.append((py * W + px).astype(np.int32))
        off.append(off[-1] + len(px))
    return np.concatenate(pts).reshape(-1, 3), np.concatenate(pix), np.asarray(off, np.int64)


# ---------------------------------------------------------------------------------------------------- cameras and test meshes
def world_to_cam(pose):
    """E = diag(1, -1, -1) inverse(pose)[:3] for a pyrender-style camera-to-world pose (x right, y up, looking down -z)"""
    return np.diag([1.0, -1.0, -1.0]) @ np.linalg.inv(np.asarray(pose, np.float64))[:3]


def cam_to_world(pose):
    """M = (pose diag(1, -1, -1, 1))[:3]"""
    return (np.asarray(pose, np.float64) @ np.diag([1.0, -1.0, -1.0, 1.0]))[:3]


def look_at_pose(eye):
    """a pyrender-style pose at `eye` whose -z axis points at the origin"""
    eye = np.asarray(eye, np.float64)
    z = eye / np.linalg.norm(eye)
    up = np.array([0.0, 1.0, 0.0]) if abs(z[1]) < 0.9 else np.array([1.0, 0.0, 0.0])
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    pose = np.eye(4)
    pose[:3, 0], pose[:3, 1], pose[:3, 2], pose[:3, 3] = x, y, z, eye
    return pose


def icosphere(level, radius=1.0):
    """20 4^level faces, vertices on the sphere"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    V = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    V = [np.asarray(v, np.float64) / np.linalg.norm(v) for v in V]
    F = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2),
         (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        mid, F2 = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = V[a] + V[b]
                V.append(p / np.linalg.norm(p))
                mid[k] = len(V) - 1
            return mid[k]
        for a, b, c in F:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            F2 += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        F = F2
    return np.asarray(V) * radius, np.asarray(F, np.int64)
