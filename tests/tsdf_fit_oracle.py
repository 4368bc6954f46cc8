"""NumPy twin of the scene memory's fit of the latent codes to a fused state (csrc/tsdffit.hip: ls_tsdf_draw_f32 / ls_tsdf_draw_batch_f32
and ls_tsdf_fit_loss_f64) -- not a test module.  The definition of include/livingscenes_hip.h step by step, the same text as
csrc/tsdffit_plan.h: integers and float64, every product and sum rounded on its own (NumPy never contracts), so the header and the
kernels are held to it by equality.
  kinds      eligible iff n >= min_obs; FREE iff sum == n * 16384 (integers), every other eligible sample BAND
  lists      the eligible samples of a kind in linear index order (k fastest), length L
  quota      T = min(L, m); stratum j = ranks [j L // T, (j + 1) L // T), width w; rank = j L // T + ((r_j * w) >> 32),
             r_j = mix64(key + (j + 1) * golden) >> 32, key = mix64(seed + kind * golden), all modulo 2^64
  columns    band first, then free; points = fp32(origin_a + voxel * index_a), target = trunc * (sum / (n * 16384)); a column beyond T is
             a PAD: the position of sample 0, target 0, index -1
  loss       u = float64(sdf); BAND e = u - target / s; FREE e = min(u - trunc / s, 0); PAD e = 0; loss = chunk_sum(e^2) / m with m the
             non-PAD columns (0.0 where m = 0), grad = fp32(2 e / m); chunk_sum is tsdf_sample_oracle's."""
import numpy as np

from fuse_oracle import SCALE
from tsdf_sample_oracle import chunk_sum

PAD, BAND, FREE = 0, 1, 2
GOLDEN = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1


def mix64(z):
    """the finaliser of splitmix64 on a Python int"""
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def kinds(state, min_obs=1):
    """-> uint8 [nx,ny,nz]: PAD (not eligible), BAND or FREE"""
    S, N = (np.asarray(t).astype(np.int64) for t in state)
    eligible = N >= int(min_obs)
    free = eligible & (S == N * SCALE)
    return np.where(free, FREE, np.where(eligible, BAND, PAD)).astype(np.uint8)


def ranks(L, m, seed, kind):
    """the list ranks a quota m takes out of a list of length L -> list of T = min(L, m) ints, ascending"""
    T = min(int(L), int(m))
    key = mix64(int(seed) + kind * GOLDEN)
    out = []
    for j in range(T):
        lo, hi = (j * L) // T, ((j + 1) * L) // T
        r = mix64(key + (j + 1) * GOLDEN) >> 32
        out.append(lo + ((r * (hi - lo)) >> 32))
    return out


def draw(state, origin, voxel, trunc, n_band, n_free, seed, min_obs=1):
    """one problem -> dict: points fp32 [N,3], target float64 [N], kind uint8 [N], index int32 [N], counts int64 [3] = (eligible, band,
    free), taken = (band, free) columns that are no PAD"""
    S, N = (np.asarray(t) for t in state)
    dims = S.shape
    origin, h, trunc = np.asarray(origin, np.float64).reshape(3), np.float64(voxel), np.float64(trunc)
    kd = kinds(state, min_obs).reshape(-1)
    cols = int(n_band) + int(n_free)
    index = np.full(cols, -1, np.int64)
    kind = np.zeros(cols, np.uint8)
    counts, taken, at = [0, 0, 0], [], 0
    for k, m in ((BAND, int(n_band)), (FREE, int(n_free))):
        where = np.flatnonzero(kd == k)
        counts[k] = len(where)
        take = ranks(len(where), m, seed, k)
        index[at:at + len(take)] = where[np.array(take, np.int64)] if take else []
        kind[at:at + len(take)] = k
        taken.append(len(take))
        at += m
    counts[0] = counts[1] + counts[2]
    safe = np.maximum(index, 0)
    ijk = np.stack(np.unravel_index(safe, dims), 1)
    points = (origin[None, :] + h * ijk.astype(np.float64)).astype(np.float32)
    s, n = S.reshape(-1)[safe].astype(np.float64), N.reshape(-1)[safe].astype(np.float64)
    with np.errstate(all="ignore"):
        target = np.where(index >= 0, trunc * (s / (np.maximum(n, 1.0) * np.float64(SCALE))), 0.0)
    return {"points": points, "target": target, "kind": kind, "index": index.astype(np.int32), "counts": np.array(counts, np.int64),
            "taken": tuple(taken)}


def draw_batch(states, origins, voxels, truncs, n_band, n_free, seeds, min_obs=1):
    """P problems: every one is its own draw -> dict of stacked arrays"""
    ds = [draw(st, o, h, tr, n_band, n_free, sd, min_obs) for st, o, h, tr, sd in zip(states, origins, voxels, truncs, seeds)]
    return {k: np.stack([d[k] for d in ds]) for k in ("points", "target", "kind", "index", "counts")}


def errors(sdf, s, trunc, target, kind):
    """one problem: e float64 [N]"""
    u = np.asarray(sdf, np.float32).astype(np.float64)
    sd, trunc = np.float64(np.float32(s)), np.float64(trunc)
    e_band = u - np.asarray(target, np.float64) / sd
    e_free = np.minimum(u - trunc / sd, 0.0)
    kind = np.asarray(kind)
    return np.where(kind == BAND, e_band, np.where(kind == FREE, e_free, 0.0))


def fit_loss(sdf, s, trunc, target, kind, min_loss=None, improved=None):
    """sdf fp32 [P,N], s fp32 [P], trunc float64 [P], target float64 [P,N], kind uint8 [P,N] -> (loss float64 [P], grad fp32 [P,N]);
    min_loss float64 [P] and improved int32 [P], if given, are updated in place as ls_mse_f32 does"""
    sdf = np.asarray(sdf, np.float32)
    P, N = sdf.shape
    loss, grad = np.zeros(P, np.float64), np.zeros((P, N), np.float32)
    for p in range(P):
        e = errors(sdf[p], s[p], trunc[p], target[p], kind[p])
        m = int((np.asarray(kind[p]) != PAD).sum())
        if m > 0:
            loss[p] = np.float64(chunk_sum(e * e)) / np.float64(m)
            grad[p] = (2.0 * e / np.float64(m)).astype(np.float32)
        if min_loss is not None and loss[p] < min_loss[p]:
            min_loss[p] = loss[p]
            if improved is not None:
                improved[p] = 1
    return loss, grad
