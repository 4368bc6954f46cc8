"""NumPy twin of the completion of a fused state by the shape prior's field (csrc/tsdfprior.hip: ls_tsdf_prior_rows_f32 /
ls_tsdf_prior_vote_f32 and their batches) -- not a test module.  The definition of include/livingscenes_hip.h step by step, the same
text as csrc/tsdfprior_plan.h: integers and float64, every product and sum rounded on its own (NumPy never contracts), so the header and
the kernels are held to it by equality.  The decoder's values f are an INPUT.
  weight     w = max(w0 - n, 0); eligible iff w > 0
  rows       the eligible samples in ascending linear index (k fastest), problems in order: points = fp32(origin_a + voxel * index_a),
             row_inst = p, row_index = i
  vote       d = float64(s) * float64(f); t = clip(d / trunc, -1, 1); q = floor(t * 16384 + 0.5); sum' = sum + w q, n' = n + w; a NaN
             f casts no vote; a sample that is not eligible keeps (sum, n)
  counts     int64 [4] = eligible, voted, skipped (NaN), untouched; the rows leave voted and skipped 0"""
import numpy as np

from fuse_oracle import MAX_OBS, SCALE

ELIGIBLE, VOTED, SKIPPED, UNTOUCHED = range(4)


def weights(state, w0):
    """-> int64 [nx,ny,nz]: the votes the prior has at every sample"""
    if not 1 <= int(w0) <= MAX_OBS:
        raise ValueError(f"w0 in 1 .. {MAX_OBS}, got {w0}")
    return np.maximum(int(w0) - np.asarray(state[1]).astype(np.int64), 0)


def rows(state, origin, voxel, w0, inst=0):
    """one problem -> dict: points fp32 [R,3], row_inst int32 [R], row_index int32 [R], counts int64 [4]"""
    dims = np.asarray(state[1]).shape
    origin, h = np.asarray(origin, np.float64).reshape(3), np.float64(voxel)
    index = np.flatnonzero(weights(state, w0).reshape(-1) > 0)
    ijk = np.stack(np.unravel_index(index, dims), 1).reshape(-1, 3)
    points = (origin[None, :] + h * ijk.astype(np.float64)).astype(np.float32)
    voxels = int(np.prod(dims))
    return {"points": points, "row_inst": np.full(len(index), inst, np.int32), "row_index": index.astype(np.int32),
            "counts": np.array([len(index), 0, 0, voxels - len(index)], np.int64)}


def rows_batch(states, origins, voxels, w0):
    """P problems -> dict of the packed rows, offsets (list of P+1) and counts int64 [P,4]"""
    rs = [rows(st, o, h, w0, p) for p, (st, o, h) in enumerate(zip(states, origins, voxels))]
    out = {k: np.concatenate([r[k] for r in rs]) for k in ("points", "row_inst", "row_index")}
    out["offsets"] = [0] + np.cumsum([len(r["row_index"]) for r in rs]).tolist()
    out["counts"] = np.stack([r["counts"] for r in rs])
    return out


def quantise(s, f, trunc):
    """the vote of the values f (fp32, no NaN) -> int64"""
    d = np.float64(s) * np.asarray(f, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        t = np.clip(d / np.float64(trunc), -1.0, 1.0)
        return np.floor(t * np.float64(SCALE) + 0.5).astype(np.int64)


def vote(state, f, s, trunc, w0):
    """one problem, f fp32 [R] in the order of rows() -> ((sum', n') int32, counts int64 [4])"""
    S, N = (np.asarray(t).astype(np.int64) for t in state)
    w = weights(state, w0).reshape(-1)
    at = np.flatnonzero(w > 0)
    f = np.asarray(f, np.float32).reshape(-1)
    if len(f) != len(at):
        raise ValueError(f"{len(f)} values for {len(at)} eligible samples")
    cast = ~np.isnan(f)
    q = quantise(s, np.where(cast, f, np.float32(0)), trunc)
    So, No = S.reshape(-1).copy(), N.reshape(-1).copy()
    So[at[cast]] += w[at[cast]] * q[cast]
    No[at[cast]] += w[at[cast]]
    counts = np.array([len(at), int(cast.sum()), int((~cast).sum()), w.size - len(at)], np.int64)
    return (So.reshape(S.shape).astype(np.int32), No.reshape(N.shape).astype(np.int32)), counts


def vote_batch(states, f, offsets, s, truncs, w0):
    """P problems, f the packed values -> (list of P (sum', n'), counts int64 [P,4])"""
    out = [vote(st, f[offsets[p]:offsets[p + 1]], s[p], truncs[p], w0) for p, st in enumerate(states)]
    return [o[0] for o in out], np.stack([o[1] for o in out])
