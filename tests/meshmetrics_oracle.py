"""numpy restatement of the mesh metrics (csrc/meshmetrics.hip) -- test infrastructure, imported by tests/test_meshmetrics_cpu.py and
tests/test_hip_meshmetrics.py.

  contains          libmesh.check_mesh_contains (inside_mesh.py:5-154 + triangle_hash.pyx): same float64 operations, same 2-D hash
                    (a (point, triangle) pair is tested only when the point's cell lies in the triangle's truncated cell box), parity of the
                    strict 2-D hits above / below the point.  Pinned against the reference itself by tests/golden/mesh_contains.npz.
  contains(brute=True)  the same parity count over EVERY triangle (no hash).
  distance          Ericson's closest point on a triangle (Real-Time Collision Detection 5.1.5), zero-area triangles as their edges.
  uniforms / sample the splitmix64 stream of ls_mesh_sample_f64 and trimesh.sample.sample_surface's algorithm (sequential cumsum).
  chamfer           evaluate.py:12-40 on given samples with scipy's cKDTree.
"""
import numpy as np

M64 = np.uint64(0xFFFFFFFFFFFFFFFF)
GOLD = np.uint64(0x9E3779B97F4A7C15)


# ------------------------------------------------------------------------------------------------ point in mesh
def _rescale_params(V, F, R):
    tri = V[F].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        lo, hi = tri.reshape(-1, 3).min(0), tri.reshape(-1, 3).max(0)
        scale = (R - 1) / (hi - lo)
        translate = 0.5 - scale * lo
        tri = scale * tri + translate
    return scale, translate, tri


def _parity_pairs(P, tri, pi, ti):
    """(n0, n1) hit counts of the (point, triangle) pairs pi, ti (check_triangles + compute_intersection_depth)"""
    p, t = P[pi], tri[ti]
    a00, a01 = t[:, 0, 0] - t[:, 2, 0], t[:, 1, 0] - t[:, 2, 0]
    a10, a11 = t[:, 0, 1] - t[:, 2, 1], t[:, 1, 1] - t[:, 2, 1]
    y0, y1 = p[:, 0] - t[:, 2, 0], p[:, 1] - t[:, 2, 1]
    det = a00 * a11 - a01 * a10
    sd, ad = np.sign(det), np.abs(det)
    u = (a11 * y0 - a01 * y1) * sd
    v = (-a10 * y0 + a00 * y1) * sd
    suv = u + v
    hit = (det != 0) & (0 < u) & (u < ad) & (0 < v) & (v < ad) & (0 < suv) & (suv < ad)
    t0, t1, t2 = t[:, 0], t[:, 1], t[:, 2]
    n = np.cross(t2 - t0, t1 - t0)
    alpha = n[:, 0] * (t0[:, 0] - p[:, 0]) + n[:, 1] * (t0[:, 1] - p[:, 1])
    an = np.abs(n[:, 2])
    with np.errstate(invalid="ignore"):
        depth = np.where(an != 0, t0[:, 2] * an + alpha * np.sign(n[:, 2]), np.nan)
        pd = p[:, 2] * an
        c0 = hit & (depth >= pd)
        c1 = hit & (depth < pd)
    n0 = np.bincount(pi[c0], minlength=len(P))
    n1 = np.bincount(pi[c1], minlength=len(P))
    return n0, n1


def contains(V, F, points, R=512, brute=False):
    V, F, points = np.asarray(V, np.float64), np.asarray(F, np.int64), np.asarray(points, np.float64)
    out = np.zeros(len(points), bool)
    if len(F) == 0 or len(points) == 0:
        return out
    scale, translate, tri = _rescale_params(V, F, R)
    if not (np.all(np.isfinite(scale)) and np.all(np.isfinite(translate))):
        return out
    P = scale * points + translate
    keep = np.all((0 <= P) & (P <= R), axis=1)
    cx, cy = np.floor(P[:, 0]).astype(np.int64), np.floor(P[:, 1]).astype(np.int64)
    if not brute:
        keep &= (cx < R) & (cy < R)
    idx = np.nonzero(keep)[0]
    if len(idx) == 0:
        return out
    # candidate pairs: every triangle whose truncated, clamped (x, y) cell box holds the point's cell (brute: every triangle)
    clip = lambda v: np.clip(np.trunc(np.clip(v, -1, R)).astype(np.int64), 0, R - 1)
    bx0, bx1 = clip(tri[:, :, 0].min(1)), clip(tri[:, :, 0].max(1))
    by0, by1 = clip(tri[:, :, 1].min(1)), clip(tri[:, :, 1].max(1))
    n0 = np.zeros(len(P), np.int64)
    n1 = np.zeros(len(P), np.int64)
    if brute:
        chunk = max(1, 4_000_000 // max(len(F), 1))
        for s in range(0, len(idx), chunk):
            q = idx[s:s + chunk]
            a, b = _parity_pairs(P, tri, np.repeat(q, len(F)), np.tile(np.arange(len(F)), len(q)))
            n0 += a
            n1 += b
    else:
        # the hash as lists: (cell, triangle) for every cell of every triangle's box, sorted by cell; each point takes its cell's run
        nx, ny = bx1 - bx0 + 1, by1 - by0 + 1
        per = nx * ny
        t_of = np.repeat(np.arange(len(F)), per)
        k = np.arange(per.sum()) - np.repeat(np.cumsum(per) - per, per)
        cell = (bx0[t_of] + k // ny[t_of]) * R + by0[t_of] + k % ny[t_of]
        order = np.argsort(cell, kind="stable")
        cell, t_of = cell[order], t_of[order]
        pc = cx[idx] * R + cy[idx]
        lo_, hi_ = np.searchsorted(cell, pc, "left"), np.searchsorted(cell, pc, "right")
        cnt = hi_ - lo_
        pi = np.repeat(idx, cnt)
        ti = t_of[np.repeat(lo_, cnt) + np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)]
        for s in range(0, len(pi), 4_000_000):
            a, b = _parity_pairs(P, tri, pi[s:s + 4_000_000], ti[s:s + 4_000_000])
            n0 += a
            n1 += b
    out[idx] = (n0[idx] % 2 == 1) & (n1[idx] % 2 == 1)
    return out


# ------------------------------------------------------------------------------------------------ distance
def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _d2_at(p, a, d, s):
    e = p - (a + s[..., None] * d)
    return _dot(e, e)


def _seg_d2(p, a, b):
    ab, ap = b - a, p - a
    l = _dot(ab, ab)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(l > 0, _dot(ap, ab) / np.where(l > 0, l, 1), 0.0)
    return _d2_at(p, a, ab, np.clip(s, 0, 1))


def point_triangle_d2(p, a, b, c):
    """squared distance, broadcast over leading axes (Ericson 5.1.5; the branch order of ClosestPtPointTriangle)"""
    ab, ac, ap, bp, cp = b - a, c - a, p - a, p - b, p - c
    d1, d2 = _dot(ab, ap), _dot(ac, ap)
    d3, d4 = _dot(ab, bp), _dot(ac, bp)
    vc = d1 * d4 - d3 * d2
    d5, d6 = _dot(ab, cp), _dot(ac, cp)
    vb = d5 * d2 - d1 * d6
    va = d3 * d6 - d5 * d4
    e43, e56 = d4 - d3, d5 - d6
    den = va + vb + vc
    safe = lambda num, dd: np.where(dd > 0, num / np.where(dd > 0, dd, 1), 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        v, w = safe(vb, den), safe(vc, den)
        e = p - (a + ab * v[..., None] + ac * w[..., None])
        face = _dot(e, e)
        degen = np.minimum(np.minimum(_seg_d2(p, a, b), _seg_d2(p, b, c)), _seg_d2(p, c, a))
        conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (e43 >= 0) & (e56 >= 0), ~(den > 0)]
        vals = [_dot(ap, ap), _dot(bp, bp), _d2_at(p, a, ab, safe(d1, d1 - d3)), _dot(cp, cp), _d2_at(p, a, ac, safe(d2, d2 - d6)),
                _d2_at(p, b, c - b, safe(e43, e43 + e56)), degen]
        return np.select(conds, vals, face)


def distance(V, F, points, max_dist, chunk_pairs=4_000_000):
    """[n] distance to the closest triangle where < max_dist, +inf elsewhere (brute force over every triangle)"""
    V, F, points = np.asarray(V, np.float64), np.asarray(F, np.int64), np.asarray(points, np.float64)
    out = np.full(len(points), np.inf)
    if len(F) == 0:
        return out
    T = V[F]
    step = max(1, chunk_pairs // len(F))
    for s in range(0, len(points), step):
        p = points[s:s + step, None, :]
        d2 = point_triangle_d2(p, T[None, :, 0], T[None, :, 1], T[None, :, 2]).min(1)
        d = np.sqrt(d2)
        out[s:s + step] = np.where(d < max_dist, d, np.inf)
    return out


# ------------------------------------------------------------------------------------------------ sampling
def _mix(z):
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def uniforms(seed, j):
    """u_j of stream `seed`: (splitmix64(key + (j + 1) * golden) >> 11) * 2^-53, key = splitmix64(seed + golden)"""
    with np.errstate(over="ignore"):
        key = _mix(np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF) + GOLD)
        z = key + (np.asarray(j, np.uint64) + np.uint64(1)) * GOLD
    return (_mix(z) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def face_areas(V, F):
    T = np.asarray(V, np.float64)[np.asarray(F, np.int64)]
    c = np.cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0])
    return np.sqrt(c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1] + c[:, 2] * c[:, 2]) / 2.0


def sample(V, F, count, seed):
    """-> (points [count,3], face [count], pick [count], cumsum [nf]) with numpy's sequential cumsum"""
    V, F = np.asarray(V, np.float64), np.asarray(F, np.int64)
    cum = np.cumsum(face_areas(V, F))
    j = 3 * np.arange(count, dtype=np.uint64)
    u0, r1, r2 = uniforms(seed, j), uniforms(seed, j + np.uint64(1)), uniforms(seed, j + np.uint64(2))
    pick = u0 * cum[-1]
    face = np.minimum(np.searchsorted(cum, pick), len(F) - 1)
    fold = r1 + r2 > 1.0
    r1 = np.where(fold, np.abs(r1 - 1.0), r1)
    r2 = np.where(fold, np.abs(r2 - 1.0), r2)
    T = V[F[face]]
    pts = (r1[:, None] * (T[:, 1] - T[:, 0]) + r2[:, None] * (T[:, 2] - T[:, 0])) + T[:, 0]
    return pts, face, pick, cum


def chamfer(gt_points, samples):
    """evaluate.py:27-38 on given samples: (gt_to_gen, gen_to_gt) mean squared nearest-neighbour distances"""
    from scipy.spatial import cKDTree
    d1, _ = cKDTree(samples).query(gt_points)
    d2, _ = cKDTree(gt_points).query(samples)
    return float(np.mean(np.square(d1))), float(np.mean(np.square(d2)))


# ------------------------------------------------------------------------------------------------ test meshes
def cube():
    V = np.array([[x, y, z] for x in (0., 1.) for y in (0., 1.) for z in (0., 1.)])
    F = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
                  [1, 5, 7], [1, 7, 3]])
    return V, F


def icosphere(level=2):
    t = (1 + 5 ** 0.5) / 2
    V = [[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t], [t, 0, -1], [t, 0, 1],
         [-t, 0, -1], [-t, 0, 1]]
    F = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
         [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]]
    V = [np.array(v, float) / np.linalg.norm(v) for v in V]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                v = V[a] + V[b]
                V.append(v / np.linalg.norm(v))
                mid[k] = len(V) - 1
            return mid[k]
        for a, b, c in F:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        F = nf
    return np.array(V), np.array(F)


def torus(R=1.0, r=0.35, nu=32, nv=16):
    u, v = np.meshgrid(np.arange(nu) * 2 * np.pi / nu, np.arange(nv) * 2 * np.pi / nv, indexing="ij")
    V = np.stack([(R + r * np.cos(v)) * np.cos(u), (R + r * np.cos(v)) * np.sin(u), r * np.sin(v)], -1).reshape(-1, 3)
    F = []
    for i in range(nu):
        for j in range(nv):
            a, b, c, d = i * nv + j, ((i + 1) % nu) * nv + j, ((i + 1) % nu) * nv + (j + 1) % nv, i * nv + (j + 1) % nv
            F += [[a, b, c], [a, c, d]]
    return V, np.array(F)
