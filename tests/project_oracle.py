"""NumPy twin of the projection of csrc/cloudnear.hip (ls_cloud_project_f32 / ls_cloud_project_batch_f32) -- not a test module.
The definition of include/livingscenes_hip.h step by step.  For a row i that has a cell, the neighbours, m_i, the integer moments s1 / s2,
the covariance C, its eigenvalues l0 <= l1 <= l2 and the validity rule are those of normals_oracle, exactly.  Then, all in float64:
  normal      n = v / sqrt((v_0 v_0 + v_1 v_1) + v_2 v_2), v the eigenvector of l0 (np.linalg.eigh), never rounded to fp32; no sign rule
  offset      unit = 1.0 / (float64(inv) * 32768.0); d_k = (float64(s1_k) / float64(m_i)) * unit: the row minus the centroid of its neighbours
  distance    s = (d_0 n_0 + d_1 n_1) + d_2 n_2
  variation   l0 / ((l0 + l1) + l2)
  state       0: no cell; 1: not valid; 2 (held): variation > float64(float32(max_variation)) or |s| > float64(float32(max_shift)); 3: moved
  points      state 3: float32(float64(A[i]_k) - s * n_k); else the input row bit for bit
  shift       float32(|s|) in states 2 and 3, else 0
  counts      the rows per state, int64 [4]
  sum_shift2  the sum of s^2 over the moved rows by the chunk rule of the search: chunks of 256 rows, each added in the fixed tree of
              chunk_sum (t += t + o for o = 128, 64, ..., 1), the partials added in chunk order from 0.0
`project` is the vectorised form the GPU tests compare against, `project_brute` the O(a^2) literal reading with Python-int moments and
Python floats that tests/test_cloud_project_cpu.py holds it to.  Both return a dict: points [a,3] fp32, state [a] int32, shift [a] fp32,
counts int64 [4], sum_shift2 float, nbr_cnt [a] int32, and for the bounds of the GPU tests s [a], n [a,3], variation [a], lam [a,3] float64
(s, n and variation are 0 where the row has no plane)."""
import numpy as np

import normals_oracle as nmo

CHUNK = 256
NO_CELL, NO_PLANE, HELD, MOVED = 0, 1, 2, 3


def chunk_rule(v):
    """the float64 sum of v [a] by the chunk rule of the definition"""
    total = 0.0
    for c0 in range(0, v.shape[0], CHUNK):
        lds = np.zeros(CHUNK)
        lds[: min(CHUNK, v.shape[0] - c0)] = v[c0:c0 + CHUNK]
        o = CHUNK // 2
        while o > 0:
            lds[:o] = lds[:o] + lds[o:2 * o]
            o //= 2
        total = total + float(lds[0])
    return total


def _limits(max_variation, max_shift):
    mv, ms = np.float32(max_variation), np.float32(max_shift)
    assert mv >= 0 and ms >= 0                                           # neither NaN nor negative
    return float(mv), float(ms)


def _unit(r):
    inv = np.float32(1) / np.float32(r)
    return 1.0 / (float(inv) * 32768.0)


def _result(A, has_cell, tw, state, points, shift, s, n, var):
    counts = np.bincount(state, minlength=4).astype(np.int64)
    return {"points": points, "state": state, "shift": shift, "counts": counts, "sum_shift2": chunk_rule(np.where(state == MOVED, s * s, 0.0)),
            "nbr_cnt": tw["nbr_cnt"], "s": s, "n": n, "variation": var, "lam": tw["lam"]}


def project(A, r, min_nbrs=5, max_variation=1 / 3, max_shift=np.inf):
    A = np.ascontiguousarray(A, dtype=np.float32).reshape(-1, 3)
    a = A.shape[0]
    mv, ms = _limits(max_variation, max_shift)
    tw = nmo.normals(A, r, min_nbrs)
    has_cell = tw["nbr_cnt"] > 0                                         # a row with a cell is its own neighbour
    state = np.where(has_cell, NO_PLANE, NO_CELL).astype(np.int32)
    points, shift = A.copy(), np.zeros(a, dtype=np.float32)
    s, n, var = np.zeros(a), np.zeros((a, 3)), np.zeros(a)
    rows = np.flatnonzero(tw["valid"])
    if rows.size:
        dm, d1, d2 = tw["nbr_cnt"][rows].astype(np.float64), tw["s1"][rows].astype(np.float64), tw["s2"][rows].astype(np.float64)
        C = np.zeros((rows.size, 3, 3))
        for k, (u, v) in enumerate(nmo.PAIRS):
            C[:, u, v] = C[:, v, u] = d2[:, k] - (d1[:, u] * d1[:, v]) / dm
        lm, vec = np.linalg.eigh(C)
        v = vec[:, :, 0]
        ln = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
        nn = v / ln[:, None]
        d = (d1 / dm[:, None]) * _unit(r)
        ss = (d[:, 0] * nn[:, 0] + d[:, 1] * nn[:, 1]) + d[:, 2] * nn[:, 2]
        vv = lm[:, 0] / ((lm[:, 0] + lm[:, 1]) + lm[:, 2])
        held = (vv > mv) | (np.abs(ss) > ms)
        s[rows], n[rows], var[rows] = ss, nn, vv
        state[rows] = np.where(held, HELD, MOVED)
        shift[rows] = np.abs(ss).astype(np.float32)
        mvd = rows[~held]
        points[mvd] = (A[mvd].astype(np.float64) - ss[~held, None] * nn[~held]).astype(np.float32)
    return _result(A, has_cell, tw, state, points, shift, s, n, var)


def project_brute(A, r, min_nbrs=5, max_variation=1 / 3, max_shift=np.inf):
    """the definition read literally: O(a^2), the moments as Python ints, the float64 part in Python floats row by row"""
    A = np.ascontiguousarray(A, dtype=np.float32).reshape(-1, 3)
    a = A.shape[0]
    mv, ms = _limits(max_variation, max_shift)
    tw = nmo.normals_brute(A, r, min_nbrs)
    unit = _unit(r)
    state = np.zeros(a, dtype=np.int32)
    points, shift = A.copy(), np.zeros(a, dtype=np.float32)
    s, n, var = np.zeros(a), np.zeros((a, 3)), np.zeros(a)
    for i in range(a):
        m = int(tw["nbr_cnt"][i])
        if m == 0:
            continue                                                     # no cell
        state[i] = NO_PLANE
        if m < min_nbrs:
            continue
        s1, s2 = [int(x) for x in tw["s1"][i]], [int(x) for x in tw["s2"][i]]
        C = np.zeros((3, 3))
        for k, (u, v) in enumerate(nmo.PAIRS):
            C[u, v] = C[v, u] = float(s2[k]) - (float(s1[u]) * float(s1[v])) / float(m)
        lm, vec = np.linalg.eigh(C)
        l0, l1, l2 = (float(x) for x in lm)
        if not (l2 > 0 and l1 > 2.0 ** -40 * l2):
            continue
        v = [float(x) for x in vec[:, 0]]
        ln = float(np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]))
        nn = [x / ln for x in v]
        d = [(float(s1[k]) / float(m)) * unit for k in range(3)]
        ss = (d[0] * nn[0] + d[1] * nn[1]) + d[2] * nn[2]
        vv = l0 / ((l0 + l1) + l2)
        s[i], n[i], var[i] = ss, nn, vv
        shift[i] = np.float32(abs(ss))
        if vv > mv or abs(ss) > ms:
            state[i] = HELD
            continue
        state[i] = MOVED
        points[i] = [np.float32(float(A[i, k]) - ss * nn[k]) for k in range(3)]
    return _result(A, tw["nbr_cnt"] > 0, tw, state, points, shift, s, n, var)


def project_batch(As, rs, min_nbrs=5, max_variation=1 / 3, max_shift=np.inf):
    return [project(A, rs[p], min_nbrs, max_variation, max_shift) for p, A in enumerate(As)]
