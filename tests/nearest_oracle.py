"""NumPy twin of csrc/cloudnear.hip (ls_cloud_nearest_f32 / ls_cloud_nearest_batch_f32) -- not a test module.
The definition of include/livingscenes_hip.h step by step, with every fp32 product and sum rounded on its own (NumPy never contracts):
  queries     the rows of B under g (R | t), merge_oracle.transform: y_a = ((R_a0 x_0 + R_a1 x_1) + R_a2 x_2) + t_a; g None: B as it is
  cells       of edge r for targets and queries alike, merge_oracle.cells: inv = float32(1) / float32(r); c_a = floor(x_a * inv) clamped to
              [-2^30, 2^30], as int32; a row with a non-finite coordinate has no cell: such a target is never a neighbour, such a query has none
  distance    d2(i,j) = ((dx dx + dy dy) + dz dz), dx = y_0 - A[j][0] ..., in fp32; r2 = float32(r) * float32(r)
  neighbour   of query i: among the targets j whose cell differs from the query's by at most 1 on every axis and with d2(i,j) <= r2, the least
              under (d2, j)
-> (nn_idx [b] int32, -1: none; nn_d2 [b] fp32, +inf: none; counts int64 [3] = finite queries, queries with a neighbour, targets that are a
neighbour; sum_d2 = math.fsum of the float64 values of the finite nn_d2: the exactly rounded sum the device's float64 sum is held to).
`nearest` is the vectorised form the GPU tests compare against (targets sorted by cell, 27 lookups per query), `nearest_brute` the O(a b)
literal reading, cell condition included, that tests/test_cloud_nearest_cpu.py holds it to."""
import itertools
import math

import numpy as np

from merge_oracle import cells, transform

PAIRS_PER_PASS = 1 << 22   # (query, member) pairs expanded at a time: bounds the memory of `nearest`, not its result


def _inputs(A, B, g, r):
    A = np.ascontiguousarray(A, dtype=np.float32).reshape(-1, 3)
    Y = transform(B, g)
    r = np.float32(r)
    r2 = r * r
    assert r2.dtype == np.float32 and np.isfinite(r2) and r2 > 0
    ca, va = cells(A, r)
    cb, vb = cells(Y, r)
    return A, Y, r2, ca, va, cb, vb


def _d2(Yq, At):
    with np.errstate(all="ignore"):
        d = Yq - At
        out = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    assert out.dtype == np.float32
    return out


def _result(idx, d2, vb):
    has = idx >= 0
    counts = np.array([int(vb.sum()), int(has.sum()), int(np.unique(idx[has]).size)], dtype=np.int64)
    return idx, d2, counts, math.fsum(d2[has].astype(np.float64).tolist())


def nearest(A, B, g, r):
    A, Y, r2, ca, va, cb, vb = _inputs(A, B, g, r)
    b = Y.shape[0]
    idx = np.full(b, -1, dtype=np.int32)
    d2 = np.full(b, np.inf, dtype=np.float32)
    ta, qi = np.flatnonzero(va), np.flatnonzero(vb)
    if ta.size == 0 or qi.size == 0:
        return _result(idx, d2, vb)
    # a cell triple as one int64: per axis the rank among the targets' cell coordinates (a coordinate no target has matches nothing)
    vals = [np.unique(ca[ta, k]).astype(np.int64) for k in range(3)]
    n1, n2 = len(vals[1]), len(vals[2])
    rk = [np.searchsorted(vals[k], ca[ta, k]) for k in range(3)]
    tkey = (rk[0] * n1 + rk[1]) * n2 + rk[2]
    order = np.argsort(tkey, kind="stable")
    skey, tidx = tkey[order], ta[order]
    BIG = np.int64(2 ** 40)
    for off in itertools.product((-1, 0, 1), repeat=3):
        nc = cb[qi].astype(np.int64) + np.asarray(off, dtype=np.int64)
        ok = np.ones(qi.size, dtype=bool)
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
        group = (np.cumsum(cnt[sel]) - 1) // PAIRS_PER_PASS
        for q in np.split(sel, np.flatnonzero(np.diff(group)) + 1):
            c = cnt[q]
            starts = np.cumsum(c) - c
            rep = np.repeat(np.arange(q.size), c)
            j = tidx[lo[q][rep] + (np.arange(int(c.sum())) - starts[rep])].astype(np.int64)
            dd = _d2(Y[qi[q]][rep], A[j])
            inside = dd <= r2
            dd = np.where(inside, dd, np.float32(np.inf))
            mn = np.minimum.reduceat(dd, starts)
            jm = np.minimum.reduceat(np.where(inside & (dd == mn[rep]), j, BIG), starts)
            gq = qi[q]
            better = (jm < BIG) & ((mn < d2[gq]) | ((mn == d2[gq]) & (jm < idx[gq])))
            d2[gq[better]] = mn[better]
            idx[gq[better]] = jm[better].astype(np.int32)
    return _result(idx, d2, vb)


def nearest_brute(A, B, g, r):
    """the neighbour rule read literally: O(a b)"""
    A, Y, r2, ca, va, cb, vb = _inputs(A, B, g, r)
    idx = np.full(Y.shape[0], -1, dtype=np.int32)
    d2 = np.full(Y.shape[0], np.inf, dtype=np.float32)
    for i in range(Y.shape[0]):
        if not vb[i]:
            continue
        for j in range(A.shape[0]):
            if not va[j] or np.abs(ca[j].astype(np.int64) - cb[i].astype(np.int64)).max() > 1:
                continue
            dd = _d2(Y[i], A[j])
            if dd <= r2 and dd < d2[i]:        # ascending j: an equal d2 later on does not replace the lower index
                d2[i], idx[i] = dd, j
    return _result(idx, d2, vb)


def nearest_batch(As, Bs, gs, rs):
    """problem by problem -> list of (nn_idx, nn_d2, counts, sum_d2)"""
    return [nearest(A, B, None if gs is None else gs[p], rs[p]) for p, (A, B) in enumerate(zip(As, Bs))]
