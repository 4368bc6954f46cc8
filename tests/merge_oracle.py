"""NumPy twin of csrc/cloudmerge.hip (ls_cloud_merge_f32 / ls_cloud_merge_batch_f32) -- not a test module.
The definition of include/livingscenes_hip.h step by step, with every fp32 product and sum rounded on its own (NumPy never contracts):
  candidates  the rows of A as given, then the rows of B under g (R | t): y_a = ((R_a0 x_0 + R_a1 x_1) + R_a2 x_2) + t_a; g None: B as it is
  cell        inv = float32(1) / float32(h); c_a = floor(y_a * inv) clamped to [-2^30, 2^30], as int32
  non-finite  a candidate with a non-finite coordinate has no cell and is never kept
  keep        candidate i is kept iff no candidate j < i has the same cell triple
`merge` is the vectorised form the GPU tests compare against, `merge_brute` the O(n^2) reading of the keep rule that tests/
test_cloud_merge_cpu.py holds it to."""
import numpy as np

CELL_MAX = np.float32(2.0 ** 30)


def transform(B, g):
    """[b,3] fp32 under g [3,4] (or [4,4]) fp32, in the stated order of operations; g None: B itself"""
    B = np.ascontiguousarray(B, dtype=np.float32).reshape(-1, 3)
    if g is None:
        return B
    g = np.asarray(g, dtype=np.float32)[:3]
    x0, x1, x2 = B[:, 0], B[:, 1], B[:, 2]
    with np.errstate(all="ignore"):
        cols = [((g[a, 0] * x0 + g[a, 1] * x1) + g[a, 2] * x2) + g[a, 3] for a in range(3)]
    out = np.stack(cols, 1)
    assert out.dtype == np.float32
    return out


def candidates(A, B, g):
    A = np.ascontiguousarray(A, dtype=np.float32).reshape(-1, 3)
    return np.concatenate([A, transform(B, g)], 0)


def cells(Y, h):
    """-> (cell [n,3] int32, valid [n] bool); the rows of `cell` without `valid` mean nothing"""
    h = np.float32(h)
    assert np.isfinite(h) and h > 0
    inv = np.float32(1) / h
    assert np.isfinite(inv)
    valid = np.isfinite(Y).all(1)
    with np.errstate(all="ignore"):
        c = np.floor(np.where(valid[:, None], Y, np.float32(0)) * inv)
    assert c.dtype == np.float32
    return np.clip(c, -CELL_MAX, CELL_MAX).astype(np.int32), valid


def merge(A, B, g, h):
    """-> (pts [n,3] fp32, src [n] int32): the kept candidates in ascending candidate order"""
    Y = candidates(A, B, g)
    c, valid = cells(Y, h)
    idx = np.flatnonzero(valid)
    if idx.size:
        _, first = np.unique(c[idx], axis=0, return_index=True)     # the first occurrence of every cell triple
        idx = np.sort(idx[first])
    return Y[idx], idx.astype(np.int32)


def merge_brute(A, B, g, h):
    """the keep rule read literally: O(n^2)"""
    Y = candidates(A, B, g)
    c, valid = cells(Y, h)
    kept = []
    for i in range(Y.shape[0]):
        if valid[i] and not any(valid[j] and (c[j] == c[i]).all() for j in range(i)):
            kept.append(i)
    idx = np.asarray(kept, dtype=np.int64)
    return Y[idx], idx.astype(np.int32)


def merge_batch(As, Bs, gs, hs):
    """problem by problem -> (pts, src, off [P+1] int64), packed as the batch op packs them"""
    outs = [merge(A, B, None if gs is None else gs[p], hs[p]) for p, (A, B) in enumerate(zip(As, Bs))]
    off = np.zeros(len(outs) + 1, dtype=np.int64)
    np.cumsum([o[1].shape[0] for o in outs], out=off[1:])
    return np.concatenate([o[0] for o in outs], 0), np.concatenate([o[1] for o in outs], 0), off
