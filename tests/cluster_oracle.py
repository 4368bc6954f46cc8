"""NumPy twin of the device decimator (csrc/meshcluster.hip): vertex clustering on a uniform grid with quadric-optimal representatives.
The definition (include/livingscenes_hip.h, ls_mesh_cluster_f64) step by step, in float64 and in the stated summation orders; the cell
keys, the resolution search and the face selection are integer-exact, so faces and r must equal the kernels', vertices agree to rounding.
"""
import numpy as np

REG = 1e-3   # the solve is (A + REG tr(A) I) d = g


def grid(vertices):
    """-> (lo [3], ext): per-axis minimum over all vertices, largest axis extent (1 when it is 0)."""
    lo = vertices.min(0)
    ext = float((vertices.max(0) - lo).max())
    return lo, (ext if ext != 0 else 1.0)


def cell_coords(vertices, lo, ext, r):
    """[nv,3] int64: c_a = min(r - 1, floor((v_a - lo_a) / h)), h = ext / r."""
    h = ext / r
    return np.minimum(r - 1, np.floor((vertices - lo) / h).astype(np.int64))


def cell_keys(vertices, lo, ext, r):
    c = cell_coords(vertices, lo, ext, r)
    return (c[:, 0] * r + c[:, 1]) * r + c[:, 2]


def n_keep(vertices, faces, lo, ext, r):
    """Faces whose three corners have three different keys."""
    k = cell_keys(vertices, lo, ext, r)[faces]
    return int(((k[:, 0] != k[:, 1]) & (k[:, 1] != k[:, 2]) & (k[:, 0] != k[:, 2])).sum())


def find_resolution(vertices, faces, lo, ext, f_target, r_max):
    a, b = 1, int(r_max)
    while a < b:
        mid = (a + b + 1) // 2
        if n_keep(vertices, faces, lo, ext, mid) <= f_target:
            a = mid
        else:
            b = mid - 1
    return a


def cluster_mesh(vertices, faces, f_target, r_max=256):
    """-> (vertices_out [nv',3] float64, faces_out [nf',3] int64, r, info); r = 0: the input unchanged (nf <= f_target).
    info: {"n_keep": faces with three different keys at r, "keys": the output vertices' cell keys, "h": cell edge, "lo": grid origin}."""
    V = np.ascontiguousarray(vertices, np.float64).reshape(-1, 3)
    F = np.ascontiguousarray(faces, np.int64).reshape(-1, 3)
    if f_target < 1 or not 1 <= r_max <= 256:
        raise ValueError("cluster_mesh: f_target >= 1 and 1 <= r_max <= 256")
    if F.shape[0] <= f_target:
        return V.copy(), F.copy(), 0, {"n_keep": F.shape[0], "keys": None, "h": None, "lo": None}
    lo, ext = grid(V)
    r = find_resolution(V, F, lo, ext, f_target, r_max)
    h = ext / r
    key = cell_keys(V, lo, ext, r)
    fk = key[F]
    live = np.nonzero((fk[:, 0] != fk[:, 1]) & (fk[:, 1] != fk[:, 2]) & (fk[:, 0] != fk[:, 2]))[0]
    # groups of the unordered key triple: odd groups keep their first member, even groups cancel
    groups = {}
    for f in live:
        groups.setdefault(tuple(sorted(fk[f])), []).append(f)
    kept = np.array(sorted(g[0] for g in groups.values() if len(g) % 2 == 1), np.int64)
    out_keys = np.unique(fk[kept]) if kept.size else np.zeros(0, np.int64)
    faces_out = np.searchsorted(out_keys, fk[kept]).astype(np.int64).reshape(-1, 3)
    # representatives
    members = {int(k): [] for k in out_keys}
    for i, k in enumerate(key):
        if int(k) in members:
            members[int(k)].append(i)
    corners = {int(k): [] for k in out_keys}
    for f in range(F.shape[0]):
        for c in range(3):
            if int(fk[f, c]) in corners:
                corners[int(fk[f, c])].append(f)
    verts_out = np.zeros((out_keys.size, 3), np.float64)
    P0 = V[F[:, 0]]
    N = np.cross(V[F[:, 1]] - P0, V[F[:, 2]] - P0)                # n = (p1 - p0) x (p2 - p0), once per face
    AREA = np.sqrt(N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1] + N[:, 2] * N[:, 2])
    with np.errstate(invalid="ignore", divide="ignore"):
        NH = N / AREA[:, None]
    for j, k in enumerate(out_keys):
        k = int(k)
        s = np.zeros(3)
        for i in members[k]:
            s = s + V[i]
        xbar = s / len(members[k])
        A, g = np.zeros((3, 3)), np.zeros(3)
        for f in corners[k]:                                      # ascending (face, corner)
            a, nh = AREA[f], NH[f]
            if a == 0:
                continue
            d = P0[f] - xbar
            A += a * np.outer(nh, nh)
            g += (a * (nh[0] * d[0] + nh[1] * d[1] + nh[2] * d[2])) * nh
        tr = A[0, 0] + A[1, 1] + A[2, 2]
        delta = np.linalg.solve(A + REG * tr * np.eye(3), g) if tr != 0 else np.zeros(3)
        c = np.array([k // (r * r), (k // r) % r, k % r], np.float64)
        verts_out[j] = np.minimum(np.maximum(xbar + delta, lo + c * h), lo + (c + 1) * h)
    return verts_out, faces_out, r, {"n_keep": int(live.size), "keys": out_keys, "h": h, "lo": lo}
