"""TEST INFRASTRUCTURE ONLY -- the two registration kernels restated in numpy on the CPU, in a type of the caller's choice: float64 is the
oracle, the same functions called with dtype=float32 give the float32 side (e32) of the rule of tests/tools/registration_vs_float64.py.

  kabsch(x1, x2, weights, raw_weights)   kabsch_kernel of csrc/match.hip: oracle/more.py::kabsch_transformation_estimation (pose_estimation.py:29-121) for
                                         ONE problem, plus the mean residual the residual matrix stores and the conditioning of the covariance
  kabsch_codes / residual_matrix         the two other entry shapes of the same kernel (pseudo-points z + t with selectors; all pairs of two lists of sets)
  icp(X, Y, R0, T0)                      icp_kernel of csrc/icp.hip: oracle/more.py::iterative_closest_point for ONE problem with an EXACT nearest-neighbour
                                         search, and the trace icp_certificate() needs
  icp_certificate(trace, c, e32_pose)    a yes / no on the INPUTS: when it holds, a correct float32 implementation follows the float64 trajectory step for
                                         step (same assignments, same iteration count), so poses can be compared under a rounding-sized bound

Pure functions, no state, nothing from the device."""
from collections import namedtuple

import numpy as np

U32 = 2.0 ** -24          # unit roundoff of float32


# ------------------------------------------------------------------------------------------------ Kabsch
def _rotation(H, row_convention):
    """SVD of the 3 x 3 covariance with the determinant fix -> (R, gap).  Column convention (pose_estimation.py:79-94): H = U S V^T,
    R = V diag(1, 1, det(V U^T)) U^T.  Row convention (pytorch3d's corresponding_points_alignment): R = U diag(1, 1, det(U V^T)) V^T, its
    transpose.  gap = (s2 + sign(det H) s3) / s1: the distance of the problem from the covariances whose optimal rotation is not unique,
    relative to its size -- the rotation's sensitivity to a perturbation of H is 1 / gap."""
    U, S, Vt = np.linalg.svd(H)
    d = np.linalg.det(Vt.T @ U.T)
    D = np.diag(np.array([1.0, 1.0, d], dtype=H.dtype))
    R = Vt.T @ D @ U.T
    gap = float((S[1] + np.sign(np.linalg.det(H.astype(np.float64))) * S[2]) / S[0]) if S[0] > 0 else 0.0
    return (R.T if row_convention else R), gap


def _outer_sum(a, b):
    """sum_i a_i b_i^T of two [n,3] arrays in their own type.  Products and numpy's pairwise sums, no BLAS: the float32 side is then the same
    numbers on every host"""
    return (a[:, :, None] * b[:, None, :]).sum(0, dtype=a.dtype)


def _rows(X, R, T):
    """X R + T, row convention, in the arrays' type (no BLAS, as above)"""
    return (X[:, :, None] * R[None, :, :]).sum(1, dtype=X.dtype) + T


def kabsch(x1, x2, weights=None, raw_weights=False, eps=1e-7, dtype=np.float64):
    """x1, x2 [n,3], weights [n] or None -> (R [3,3], t [3], res [n], mean(res), gap), everything evaluated in `dtype`.
    weights / (sum + eps) unless raw_weights (the caller has normalised, thresholded and NOT renormalised them: they are used as they are);
    means divided by (sum of the normalised weights + eps); H = sum w (x1 - mu1)(x2 - mu2)^T; R from _rotation; t = mu2 - R mu1;
    res = |R x1 + t - x2|."""
    x1, x2 = np.asarray(x1).astype(dtype), np.asarray(x2).astype(dtype)
    n = x1.shape[0]
    e = dtype(eps)
    w = np.ones(n, dtype=dtype) if weights is None else np.asarray(weights).astype(dtype)
    if weights is None or not raw_weights:
        w = w / (w.sum(dtype=dtype) + e)
    denom = w.sum(dtype=dtype) + e
    mu1 = (w[:, None] * x1).sum(0, dtype=dtype) / denom
    mu2 = (w[:, None] * x2).sum(0, dtype=dtype) / denom
    c1, c2 = x1 - mu1, x2 - mu2
    H = _outer_sum(w[:, None] * c1, c2)
    R, gap = _rotation(H, False)
    t = mu2 - (R * mu1[None, :]).sum(1, dtype=dtype)
    d = (x1[:, None, :] * R[None, :, :]).sum(2, dtype=dtype) + t - x2
    res = np.sqrt((d * d).sum(1, dtype=dtype))
    return R, t, res, res.mean(dtype=dtype), gap


def pseudo_points(z, t):
    """fl32(z + t): z [k,c,3], t [k,1,3] or [k,3] -> [k,c,3] float32, the sum the kernel forms per coordinate before anything else"""
    z, t = np.asarray(z, dtype=np.float32), np.asarray(t, dtype=np.float32).reshape(-1, 1, 3)
    return (z + t).astype(np.float32)


def codes_problems(z1, t1, z2, t2, sel1=None, sel2=None):
    """the point sets ops.kabsch_codes pairs: problem p reads the pseudo-points of set sel1[p] (default p) of side 1 and of set sel2[p] of
    side 2; a negative entry reads set 0 (matches0.clamp(min=0)) -> [(x1 [c,3], x2 [c,3])] float32"""
    p1, p2 = pseudo_points(z1, t1), pseudo_points(z2, t2)
    b = len(sel1) if sel1 is not None else len(sel2) if sel2 is not None else p1.shape[0]
    pick = lambda sel, p: max(int(sel[p]), 0) if sel is not None else p    # noqa: E731
    return [(p1[pick(sel1, p)], p2[pick(sel2, p)]) for p in range(b)]


def kabsch_codes(z1, t1, z2, t2, sel1=None, sel2=None, dtype=np.float64):
    """ops.kabsch_codes -> list of kabsch() results, one per problem"""
    return [kabsch(a, b, dtype=dtype) for a, b in codes_problems(z1, t1, z2, t2, sel1, sel2)]


def residual_matrix(src, tgt, dtype=np.float64):
    """ops.kabsch_residual_matrix: src [n,P,3], tgt [m,P,3] -> (mean residual [n,m], smallest gap of the n m problems)"""
    out = np.zeros((len(src), len(tgt)), dtype=dtype)
    gap = np.inf
    for i in range(len(src)):
        for j in range(len(tgt)):
            _, _, _, out[i, j], g = kabsch(src[i], tgt[j], dtype=dtype)
            gap = min(gap, g)
    return out, gap


# ------------------------------------------------------------------------------------------------ ICP
IcpResult = namedtuple("IcpResult", "R T rmse iterations assignment trace c")


def nearest2(Q, Y, chunk=128):
    """exact: for every row of Q the index of its nearest row of Y (the first of equals) and the two smallest squared distances d1 <= d2.
    Brute force over differences in float64 (exact differences of the inputs' values, no |q|^2 + |y|^2 - 2 q.y cancellation), in chunks."""
    Q, Y = np.asarray(Q, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    nn = np.empty(len(Q), dtype=np.int64)
    d1, d2 = np.empty(len(Q)), np.full(len(Q), np.inf)
    for a in range(0, len(Q), chunk):
        diff = Q[a:a + chunk, None, :] - Y[None, :, :]
        d = (diff * diff).sum(2)
        nn[a:a + chunk] = d.argmin(1)
        if Y.shape[0] > 1:
            two = np.partition(d, 1, axis=1)[:, :2]
            d1[a:a + chunk], d2[a:a + chunk] = two[:, 0], two[:, 1]
        else:
            d1[a:a + chunk] = d[:, 0]
    return nn, d1, d2


def icp(X, Y, R0, T0, max_iter=100, thr=1e-6, dtype=np.float64):
    """One problem of oracle/more.py::iterative_closest_point, row convention Xt = X R + T: X [n,3], Y [m,3], R0 [3,3], T0 [3].  Per iteration:
    the exact nearest neighbour in Y of every row of Xt, the rigid alignment of X onto the matched rows (means, covariance / n, SVD with the
    determinant fix), rmse of the new transform against the same matches, stop when (prev - rmse) / prev <= thr.
    -> IcpResult(R, T, rmse, iterations, assignment of the last iteration, trace, c); trace: per iteration a dict with nn, d1, d2 (the two
    smallest squared distances of every point, float64), rel (None in the first iteration), gap (of the covariance), R, T (after the update);
    c: the largest absolute coordinate of Y and of every Xt a search saw."""
    X, Y = np.asarray(X).astype(dtype), np.asarray(Y).astype(dtype)
    R, T = np.asarray(R0).astype(dtype), np.asarray(T0).astype(dtype)
    n = X.shape[0]
    Xt = _rows(X, R, T)
    mx = X.mean(0, dtype=dtype)
    trace, prev, rmse = [], None, dtype(0)
    c = float(np.abs(Y).max())
    for _ in range(max_iter):
        c = max(c, float(np.abs(Xt).max()))
        nn, d1, d2 = nearest2(Xt, Y)
        Yn = Y[nn]
        my = Yn.mean(0, dtype=dtype)
        cov = _outer_sum(X - mx, Yn - my) / dtype(n)
        R, gap = _rotation(cov, True)
        T = my - (mx[:, None] * R).sum(0, dtype=dtype)
        Xt = _rows(X, R, T)
        d = Xt - Yn
        rmse = np.sqrt((d * d).sum(1, dtype=dtype).mean(dtype=dtype))
        rel = None if prev is None else float((prev - rmse) / prev)
        trace.append(dict(nn=nn, d1=d1, d2=d2, rel=rel, gap=gap, R=R, T=T))
        if rel is not None and rel <= thr:
            break
        prev = rmse
    return IcpResult(R, T, float(rmse), len(trace), trace[-1]["nn"], trace, c)


def icp_margin(trace, c, e32_pose):
    """the smallest (d2 - d1) - 2 (sqrt d1 + sqrt d2) delta over every iteration and point of a trace, delta = c (16 e32_pose + 8 x 2^-24):
    a transformed point moves by at most delta under the largest pose error the rule accepts (16 e32_pose on R's entries and on T / c)
    plus the rounding of the transform itself (three products, three sums of values up to c); two distances |q - y1| <= |q - y2| keep their
    order under such a move when d2 - d1 = (sqrt d2 - sqrt d1)(sqrt d2 + sqrt d1) >= 2 delta (sqrt d1 + sqrt d2)"""
    delta = c * (16.0 * e32_pose + 8.0 * U32)
    return min(float((t["d2"] - t["d1"] - 2.0 * (np.sqrt(t["d1"]) + np.sqrt(t["d2"])) * delta).min()) for t in trace)


def icp_certificate(trace, c, e32_pose, rel_min=1e-4, gap_min=0.01):
    """True when a correct float32 ICP must follow this float64 trace step for step:
      every point's nearest neighbour is ahead of the second by more than a pose error of 16 e32_pose can close (icp_margin >= 0);
      every stop test that says 'go on' says so by rel >= rel_min, a hundred times the threshold 1e-6;
      the last iteration repeats the assignment of the one before it, so its rmse IS the previous one and rel is exactly 0 on both sides;
      every covariance on the way has gap >= gap_min."""
    if len(trace) < 2 or not np.array_equal(trace[-1]["nn"], trace[-2]["nn"]):
        return False
    if any(t["rel"] is None or t["rel"] < rel_min for t in trace[1:-1]):
        return False
    if any(t["gap"] < gap_min for t in trace):
        return False
    return icp_margin(trace, c, e32_pose) >= 0.0
