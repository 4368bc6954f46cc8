"""NumPy twin of the normals of csrc/cloudnear.hip (ls_cloud_normals_f32 / ls_cloud_normals_batch_f32) -- not a test module.
The definition of include/livingscenes_hip.h step by step, on the cells of merge_oracle (edge r, inv = float32(1) / float32(r)):
  neighbours  of row i (which has a cell): the rows j, i included, whose cell differs from i's by at most 1 on every axis and with
              d2 <= r2 = float32(r) * float32(r), dx = A[i][0] - A[j][0] ..., d2 = ((dx dx + dy dy) + dz dz) in fp32; m_i of them
  moments     u = dx * inv in fp32, q = rint(u * 32768) as an integer; s1 = sum q [3], s2 = sum q_a q_b [6] in int64: exact, in any order
  covariance  C_ab = float64(s2_ab) - (float64(s1_a) * float64(s1_b)) / float64(m_i), in this order
  eigen       np.linalg.eigh(C): l0 <= l1 <= l2
  valid       m_i >= min_nbrs, l2 > 0 and l1 > 2^-40 l2
  normal      the eigenvector of l0, rounded to fp32, negated if its first component of largest fp32 magnitude is negative
  variation   float32(l0 / ((l0 + l1) + l2))
An invalid row has the normal (0, 0, 0) and variation 0; a row without a cell also m_i = 0.
`normals` is the vectorised form the GPU tests compare against (rows sorted by cell, 27 lookups per row), `normals_brute` the O(a^2) literal
reading with Python ints that tests/test_cloud_plane_cpu.py holds it to.  Both return a dict: normals [a,3] fp32, nbr_cnt [a] int32,
variation [a] fp32, counts int64 [2] = (rows with a cell, valid rows), valid [a] bool, lam [a,3] float64 (ascending; 0 where m_i = 0),
s1 [a,3] and s2 [a,6] int64."""
import itertools

import numpy as np

from merge_oracle import cells

SCALE = np.float32(32768.0)
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def _setup(A, r):
    A = np.ascontiguousarray(A, dtype=np.float32).reshape(-1, 3)
    r = np.float32(r)
    r2, inv = r * r, np.float32(1) / r
    assert np.isfinite(r2) and r2 > 0 and np.isfinite(inv)
    c, valid = cells(A, r)
    return A, r2, inv, c, valid


def _q(d, inv):
    """the integer offsets of the definition from the fp32 differences d [..., 3]"""
    with np.errstate(all="ignore"):
        u = d * inv
        assert u.dtype == np.float32
        return np.rint(u * SCALE).astype(np.int64)


def _d2(d):
    with np.errstate(all="ignore"):
        out = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    assert out.dtype == np.float32
    return out


def _finish(a, has_cell, m, s1, s2, min_nbrs):
    """the float64 part of the definition from the integer moments"""
    lam = np.zeros((a, 3))
    normals = np.zeros((a, 3), dtype=np.float32)
    variation = np.zeros(a, dtype=np.float32)
    valid = np.zeros(a, dtype=bool)
    rows = np.flatnonzero(m > 0)
    if rows.size:
        dm, d1, d2 = m[rows].astype(np.float64), s1[rows].astype(np.float64), s2[rows].astype(np.float64)
        C = np.zeros((rows.size, 3, 3))
        for k, (u, v) in enumerate(PAIRS):
            C[:, u, v] = C[:, v, u] = d2[:, k] - (d1[:, u] * d1[:, v]) / dm
        lm, vec = np.linalg.eigh(C)
        lam[rows] = lm
        ok = (m[rows] >= min_nbrs) & (lm[:, 2] > 0) & (lm[:, 1] > 2.0 ** -40 * lm[:, 2])
        n = vec[:, :, 0].astype(np.float32)
        big = np.argmax(np.abs(n), axis=1)                               # the first of the largest
        n = np.where((n[np.arange(rows.size), big] < 0)[:, None], -n, n)
        n = np.where(n == 0, np.float32(0), n)                           # no negative zeros
        with np.errstate(all="ignore"):
            var = (lm[:, 0] / ((lm[:, 0] + lm[:, 1]) + lm[:, 2])).astype(np.float32)
        normals[rows[ok]], variation[rows[ok]], valid[rows[ok]] = n[ok], var[ok], True
    counts = np.array([int(has_cell.sum()), int(valid.sum())], dtype=np.int64)
    return {"normals": normals, "nbr_cnt": m.astype(np.int32), "variation": variation, "counts": counts, "valid": valid, "lam": lam,
            "s1": s1, "s2": s2}


def normals(A, r, min_nbrs=5):
    A, r2, inv, c, has_cell = _setup(A, r)
    a = A.shape[0]
    m, s1, s2 = np.zeros(a, dtype=np.int64), np.zeros((a, 3), dtype=np.int64), np.zeros((a, 6), dtype=np.int64)
    ta = np.flatnonzero(has_cell)
    if ta.size:
        vals = [np.unique(c[ta, k]).astype(np.int64) for k in range(3)]
        n1, n2 = len(vals[1]), len(vals[2])
        rk = [np.searchsorted(vals[k], c[ta, k]) for k in range(3)]
        tkey = (rk[0] * n1 + rk[1]) * n2 + rk[2]
        order = np.argsort(tkey, kind="stable")
        skey, tidx = tkey[order], ta[order]
        for off in itertools.product((-1, 0, 1), repeat=3):
            nc = c[ta].astype(np.int64) + np.asarray(off, dtype=np.int64)
            ok = np.ones(ta.size, dtype=bool)
            pos = []
            for k in range(3):
                p = np.minimum(np.searchsorted(vals[k], nc[:, k]), len(vals[k]) - 1)
                ok &= vals[k][p] == nc[:, k]
                pos.append(p)
            key = (pos[0] * n1 + pos[1]) * n2 + pos[2]
            lo = np.searchsorted(skey, key, "left")
            cnt = np.where(ok, np.searchsorted(skey, key, "right") - lo, 0)
            sel = np.flatnonzero(cnt > 0)
            if sel.size == 0:
                continue
            cn = cnt[sel]
            starts = np.cumsum(cn) - cn
            rep = np.repeat(np.arange(sel.size), cn)
            i = ta[sel][rep]
            j = tidx[lo[sel][rep] + (np.arange(int(cn.sum())) - starts[rep])]
            with np.errstate(all="ignore"):
                d = A[i] - A[j]
            inside = _d2(d) <= r2
            i, q = i[inside], _q(d[inside], inv)
            np.add.at(m, i, 1)
            np.add.at(s1, i, q)
            np.add.at(s2, i, np.stack([q[:, u] * q[:, v] for u, v in PAIRS], 1))
    return _finish(a, has_cell, m, s1, s2, min_nbrs)


def normals_brute(A, r, min_nbrs=5):
    """the definition read literally: O(a^2), the moments as Python ints"""
    A, r2, inv, c, has_cell = _setup(A, r)
    a = A.shape[0]
    m, s1, s2 = np.zeros(a, dtype=np.int64), np.zeros((a, 3), dtype=np.int64), np.zeros((a, 6), dtype=np.int64)
    for i in range(a):
        if not has_cell[i]:
            continue
        mi, t1, t2 = 0, [0, 0, 0], [0, 0, 0, 0, 0, 0]
        for j in range(a):
            if not has_cell[j] or np.abs(c[j].astype(np.int64) - c[i].astype(np.int64)).max() > 1:
                continue
            with np.errstate(all="ignore"):
                d = A[i] - A[j]
            if not _d2(d) <= r2:
                continue
            q = [int(v) for v in _q(d, inv)]
            mi += 1
            for k in range(3):
                t1[k] += q[k]
            for k, (u, v) in enumerate(PAIRS):
                t2[k] += q[u] * q[v]
        m[i], s1[i], s2[i] = mi, t1, t2
    return _finish(a, has_cell, m, s1, s2, min_nbrs)


def normals_batch(As, rs, min_nbrs=5):
    return [normals(A, rs[p], min_nbrs) for p, A in enumerate(As)]
