"""kabsch_kernel (csrc/match.hip, through its four entries) and icp_kernel (csrc/icp.hip) against the float64 oracles of
tests/registration_oracle.py at their size edges: the case ladders, their inputs, the references and the rule.

    python tests/tools/registration_vs_float64.py            (CPU: every precondition, the e32 and the certificate margin of every ICP case)
    python tests/tools/registration_vs_float64.py --gpu      (GPU: both ladders under the rule, the largest err / e32 per entry and path)

The ladders are the one statement of the cases, shared by tests/test_registration_oracle_cpu.py (the preconditions on the inputs) and
tests/test_hip_registration_f64.py (the comparison).
  kabsch_ladder()   ops.kabsch: n on both sides of every multiple of 64 up to the 256 points a lane keeps in registers, then the rolled loop
                    (257, 320, 1000); b = 1, 3, 4, 5 problems (four waves per workgroup: a partly filled last one); four kinds of cloud, three
                    kinds of weights
  codes_ladder()    ops.kabsch_codes: pseudo-points fl32(z + t) of width 70, 256, 257, 300 with no selector, sel2 alone, both selectors, a
                    negative and a repeated entry in each
  resmat_ladder()   ops.kabsch_residual_matrix at (n, m, P) and ops.kabsch_residual_matrix_batch: a ragged batch with an empty problem per width
  icp_ladder()      'dynamic': small problems that take several iterations; 'edge': n on both sides of every 1024 (the ICP_PT = 4 slots of a
                    thread), n != m, m on both sides of the 64 KB of dynamic LDS (5461 | 5462) and the advertised maximum 10240, certified by
                    construction (a jittered lattice: every point's neighbour is far ahead of the second)

The rule (tests/tools/edge_vs_float64.py's margin and caps).  Per PROBLEM and per measure -- max |dR|, max |dt| / s, max |dres| / s,
|dmean(res)| / s for Kabsch; max |dR|, max |dT| / s, |drmse| / s for ICP; s = max(1, largest |coordinate| of the problem's inputs) --
    err <= min(16 x e32, 1e-4),
e32 the same measure of the float32 oracle against the float64 one, on the same inputs, computed on the CPU.  R, t and res are measured where
a kernel writes them (ops.kabsch, ops.kabsch_codes), mean(res) where it is written (the residual matrix: one measure per matrix, the largest
over its entries, each on its own scale).  Preconditions of every input, checked on the CPU: e32_min <= e32 <= 1e-5 (E32_MIN below says why
there is a lower end) and, for Kabsch, gap >= 0.01; for ICP also registration_oracle.icp_certificate, which makes the discrete assignment a
property of the inputs, so that iteration counts and final assignments are compared EXACTLY.  The generators draw an input again until it
meets them with a factor 2 in hand; nothing is seeded by hand."""
import argparse
import binascii
import os
import sys

import numpy as np

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
for p in (REPO, os.path.join(REPO, "tests"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import registration_oracle as ro  # noqa: E402
from edge_vs_float64 import E32_MAX, MARGIN, TOL, bound  # noqa: E402,F401

GAP_MIN = 0.01
# The rule reads e32 as the SIZE of float32's error on an input.  A measure is a maximum over a few numbers -- three for t, one for a 1 x 1
# residual matrix -- and in one input in twenty the float32 oracle's few errors happen to cancel: e32 then says nothing about float32
# arithmetic, and 16 x e32 is no bound for another float32 evaluation of the same input.  Every measure is relative to the scale s of
# coordinates that are float32 numbers, so a quarter of float32's unit roundoff is the least e32 that is kept: e32 >= E32_MIN is a
# precondition of every Kabsch input like e32 <= E32_MAX, and an input that breaks it is replaced, not excused.
# The mean of n residuals averages n such roundings: there the least e32 is E32_MIN / sqrt(n).
E32_MIN = 2.0 ** -26


def e32_min(measure, n):
    return E32_MIN / n ** 0.5 if measure == "mean_res" else E32_MIN
F32, F64 = np.float32, np.float64

def _rng(key):
    return np.random.default_rng(binascii.crc32(key.encode()))


def _rot(rng, proper=True):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if (np.linalg.det(q) > 0) != proper:
        q[:, 2] = -q[:, 2]
    return q


def _small_rot(rng, angle):
    a = rng.standard_normal(3)
    a *= angle / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) / angle * K + (1 - np.cos(angle)) / angle ** 2 * K @ K


def _aniso(rng, n, scales=(0.5, 0.3, 0.15)):
    """[n,3]: axis scales `scales` in a random frame, centred on 0"""
    return (rng.standard_normal((n, 3)) * np.array(scales)) @ _rot(rng).T


def scale_of(*arrays):
    return max(1.0, max(float(np.abs(a).max()) for a in arrays if a.size))


# ------------------------------------------------------------------------------------------------ the Kabsch ladder
KB_N = (3, 4, 63, 64, 65, 255, 256, 257, 320, 1000)
KB_B = (1, 3, 4, 5)
KB_KINDS = ("generic", "planar", "reflected", "far")
KB_WEIGHTS = ("none", "random", "raw_zeros")
KB_MEASURES = ("R", "t", "res")           # what ops.kabsch and ops.kabsch_codes write; the residual matrix writes mean_res alone


def kabsch_ladder():
    """[(key, n, b, kind, weights)]"""
    return [(f"kabsch(n={n}, b={b}, {kind}, weights={wm})", n, b, kind, wm) for n in KB_N for b in KB_B for kind in KB_KINDS for wm in KB_WEIGHTS]


_INPUTS, _REFS = {}, {}


def kabsch_errs(out, ref, s):
    """the measures of one problem: out, ref = (R [3,3], t [3], res [n], ...) -> {measure: error}"""
    d = lambda a, b: float(np.abs(np.asarray(a, dtype=F64) - np.asarray(b, dtype=F64)).max())    # noqa: E731
    return {"R": d(out[0], ref[0]), "t": d(np.reshape(out[1], 3), ref[1]) / s, "res": d(out[2], ref[2]) / s}


def kabsch_ref(x1, x2, w=None, raw=False):
    """one problem -> dict(ref = the float64 (R, t, res, mean(res)), e32 = {measure: error of the float32 oracle} (mean_res among them), gap, s)"""
    r64, r32 = ro.kabsch(x1, x2, w, raw, dtype=F64), ro.kabsch(x1, x2, w, raw, dtype=F32)
    s = scale_of(x1, x2)
    e32 = kabsch_errs(r32, r64, s)
    e32["mean_res"] = abs(float(r32[3]) - float(r64[3])) / s
    return dict(ref=r64[:4], e32=e32, gap=min(r64[4], r32[4]), s=s)


def well_posed(r, n, measures=KB_MEASURES):
    """what a draw of n points has to meet to be kept: the preconditions with a factor 2 in hand (e32 is the host's float32 arithmetic as
    much as the input)"""
    return r["gap"] >= 2 * GAP_MIN and all(2 * e32_min(k, n) <= r["e32"][k] <= E32_MAX / 2 for k in measures)


def kabsch_inputs(case):
    """-> (x1 [b,n,3], x2 [b,n,3], weights [b,n] or None, raw_weights), float32.
    x1: an anisotropic cloud (planar: the third scale is 0, so the covariance has rank 2 up to rounding and the rotation is still unique)
    about a centroid 0.3 randn (far: (10, -7, 3) + that); x2 = R (x1 - c) + c + t + 0.01 noise, R a rotation (reflected: a reflection, so the
    determinant fix is taken).  weights: none | uniform in [0.05, 1) | those normalised in float32, min(n // 3, n - 3) of them zeroed and
    NOT renormalised, passed raw (the w_threshold path of pose_estimation.py:58-66; three points keep a weight so that the rank stays 2).
    A problem is drawn again until it is well_posed().  Three or four points span a triangle whose shape decides the gap: one draw in six of
    those is rejected for its gap (down to 1e-4, with e32(R) 2e-5), one in seven for an e32 of t or res below the lower end.  From 63 points on
    one draw in sixteen is rejected, always for e32(t)."""
    key, n, b, kind, wm = case
    if key not in _INPUTS:
        rng = _rng(key)
        x1, x2 = np.empty((b, n, 3), dtype=F32), np.empty((b, n, 3), dtype=F32)
        w = None
        if wm != "none":
            w = (0.05 + 0.95 * rng.random((b, n))).astype(F32)
            if wm == "raw_zeros":
                w = (w / (w.sum(1, keepdims=True, dtype=F32) + F32(1e-7))).astype(F32)
                for p in range(b):
                    w[p, rng.permutation(n)[:min(n // 3, n - 3)]] = 0.0
        refs = []
        for p in range(b):
            while True:
                c = 0.3 * rng.standard_normal(3) + (np.array([10.0, -7.0, 3.0]) if kind == "far" else 0.0)
                a = _aniso(rng, n, (0.5, 0.3, 0.0) if kind == "planar" else (0.5, 0.3, 0.15))
                x1[p] = a + c
                x2[p] = a @ _rot(rng, kind != "reflected").T + c + 0.5 * rng.standard_normal(3) + 0.01 * rng.standard_normal((n, 3))
                r = kabsch_ref(x1[p], x2[p], None if w is None else w[p], wm == "raw_zeros")
                if well_posed(r, n):
                    break
            refs.append(r)
        _INPUTS[key], _REFS[key] = (x1, x2, w, wm == "raw_zeros"), refs
    return _INPUTS[key]


def kabsch_reference(case):
    kabsch_inputs(case)
    return _REFS[case[0]]


# ------------------------------------------------------------------------------------------------ pseudo-points and the residual matrix
CODE_WIDTHS = (70, 256, 257, 300)
CODE_SETS = 6
CODE_SELECTORS = {"none": (None, None), "sel2": (None, (3, -1, 5, 3, 0)), "both": ((5, 5, 0, 2, -1, 1, 3), (1, -2, 4, 4, 0, 2, 5))}   # (sel1, sel2)


def codes_ladder():
    """[(key, width, selectors)]: 6, 5 and 7 problems -- a partly filled last workgroup in each"""
    return [(f"kabsch_codes(width={c}, selectors={sm})", c, sm) for c in CODE_WIDTHS for sm in CODE_SELECTORS]


def _sets(rng, k, base, offset):
    """k rotated, noisy copies of one cloud: any two of them are related by a rotation, so every pairing is well conditioned"""
    if k == 0:
        return np.zeros((0,) + base.shape)
    return np.stack([base @ _rot(rng).T + 0.01 * rng.standard_normal(base.shape) + offset * rng.standard_normal(3) for _ in range(k)])


def _selectors(sm):
    return tuple(None if s is None else np.array(s, dtype=np.int64) for s in CODE_SELECTORS[sm])


def codes_inputs(case):
    """-> (z1 [6,c,3], t1 [6,1,3], z2, t2, sel1, sel2): float32 arrays, selectors int64 arrays or None.  The three cases of a width share
    their sets, which are drawn again until every problem of the three is well_posed()"""
    key, c, sm = case
    k = f"codes:{c}"
    if k not in _INPUTS:
        rng = _rng(k)
        while True:
            base = _aniso(rng, c)
            sets = tuple(a.astype(F32) for a in (_sets(rng, CODE_SETS, base, 0.0), rng.standard_normal((CODE_SETS, 1, 3)),
                                                 _sets(rng, CODE_SETS, base, 0.0), rng.standard_normal((CODE_SETS, 1, 3))))
            refs = {m: [kabsch_ref(a, b) for a, b in ro.codes_problems(*sets, *_selectors(m))] for m in CODE_SELECTORS}
            if all(well_posed(r, c) for rs in refs.values() for r in rs):
                break
        _INPUTS[k] = sets
        for m, rs in refs.items():
            _REFS[f"kabsch_codes(width={c}, selectors={m})"] = rs
    return _INPUTS[k] + _selectors(sm)


def codes_reference(case):
    codes_inputs(case)
    return _REFS[case[0]]


RESMAT = ((1, 1, 70), (3, 5, 257), (5, 3, 300), (7, 6, 256))
RESMAT_BATCH = ((1, 1), (3, 5), (0, 4), (5, 3), (7, 6))      # at every width of RESMAT, the empty problem between


def resmat_ladder():
    """[(key, [(n, m), ...], P, batched)]"""
    return ([(f"residual_matrix(n={n}, m={m}, P={P})", [(n, m)], P, False) for n, m, P in RESMAT] +
            [(f"residual_matrix_batch(P={P})", list(RESMAT_BATCH), P, True) for _, _, P in RESMAT])


def resmat_err(out, r):
    """a problem's one measure: the largest |out - ref| / s over the entries of its matrix, each entry on its own scale"""
    return {"mean_res": float((np.abs(np.asarray(out, dtype=F64).reshape(r["ref"].shape) - r["ref"]) / r["s"]).max()) if r["ref"].size else 0.0}


def resmat_ref(src, tgt):
    """one problem (a matrix) -> dict(ref [n,m] float64, s [n,m], e32 = {mean_res: resmat_err of the float32 oracle}, gap = the smallest entry's,
    e32_entry = the largest e32 of any entry's R, t, res: the conditioning of the entries)"""
    n, m = len(src), len(tgt)
    rs = [kabsch_ref(a, b) for a in src for b in tgt]
    r = dict(ref=np.array([x["ref"][3] for x in rs], dtype=F64).reshape(n, m), s=np.array([x["s"] for x in rs], dtype=F64).reshape(n, m),
             gap=min([x["gap"] for x in rs], default=np.inf), e32_entry=max([max(x["e32"].values()) for x in rs], default=0.0))
    r["e32"] = resmat_err(np.array([ro.kabsch(a, b, dtype=F32)[3] for a in src for b in tgt], dtype=F64), r)
    return r


def resmat_inputs(case):
    """-> [(src [n,P,3], tgt [m,P,3])] float32 per problem; a problem with entries is drawn again until its matrix is well posed (16 of 36
    draws are rejected, all for the lower end of e32(mean_res), most of them 1 x 1 matrices)"""
    key, sizes, P, _ = case
    if key not in _INPUTS:
        rng = _rng(key)
        ins, refs = [], []
        for n, m in sizes:
            while True:
                base = _aniso(rng, P)
                src, tgt = _sets(rng, n, base, 0.5).astype(F32).reshape(n, P, 3), _sets(rng, m, base, 0.5).astype(F32).reshape(m, P, 3)
                r = resmat_ref(src, tgt)
                if n * m == 0 or (well_posed(r, P, ("mean_res",)) and r["e32_entry"] <= E32_MAX / 2):
                    break
            ins.append((src, tgt))
            refs.append(r)
        _INPUTS[key], _REFS[key] = ins, refs
    return _INPUTS[key]


def resmat_reference(case):
    """-> [resmat_ref per problem]"""
    resmat_inputs(case)
    return _REFS[case[0]]


# ------------------------------------------------------------------------------------------------ the ICP ladder
ICP_DYNAMIC = ((4, 4), (63, 64), (64, 63), (65, 100), (100, 37), (200, 200), (255, 256), (300, 150))
ICP_EDGE = ((1023, 1024), (1024, 1000), (1025, 600), (2048, 600), (2049, 600), (3073, 600), (4096, 600), (700, 5461), (700, 5462), (700, 10240))
ICP_MEASURES = ("R", "T", "rmse")
ICP_N_MAX, ICP_M_MAX = 4096, 10240


def icp_ladder():
    """[(key, family, n, m)]"""
    return [(f"icp({fam}, n={n}, m={m})", fam, n, m) for fam, lad in (("dynamic", ICP_DYNAMIC), ("edge", ICP_EDGE)) for n, m in lad]


def icp_path(case, flags):
    """the code path a case takes: how many of a thread's ICP_PT slots hold a point, which side of 64 KB the dynamic LDS is on, the arithmetic"""
    return f"icp  slots={(case[2] + 1023) // 1024}  lds={'<=64K' if case[3] * 12 <= 65536 else '>64K '}  contract={int(bool(flags))}"


def _icp_draw(rng, fam, n, m):
    if fam == "dynamic":
        Y = rng.random((m, 3))
        disp, turn, move = 0.002 * rng.standard_normal((n, 3)), 0.25, 0.05
    else:
        g = int(np.ceil(m ** (1.0 / 3.0) - 1e-9))
        h = 1.0 / g
        cells = rng.permutation(g ** 3)[:m]
        Y = (np.stack([cells // (g * g), cells // g % g, cells % g], 1) + 0.5 + rng.uniform(-0.2, 0.2, (m, 3))) * h
        d = rng.standard_normal((n, 3))
        disp = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0, 0.1 * h, (n, 1))
        turn, move = 0.1 * h / (0.5 * 3 ** 0.5), 0.1 * h
    pick = rng.permutation(m)[:n] if n <= m else np.concatenate([rng.permutation(m), rng.integers(0, m, n - m)])
    Rg, Tg = _rot(rng), 0.3 * rng.standard_normal(3)
    X = (Y[pick] + disp - Tg) @ Rg.T                     # X Rg + Tg = Y[pick] + disp
    dR = _small_rot(rng, turn)
    v = rng.standard_normal(3)
    dT = move * v / np.linalg.norm(v)
    ctr = np.full(3, 0.5)
    # the initial guess maps X to ((X Rg + Tg) - ctr) dR + ctr + dT
    return tuple(a.astype(F32) for a in (X, Y, Rg @ dR, (Tg - ctr) @ dR + ctr + dT))


def icp_inputs(case):
    """-> (X [n,3], Y [m,3], R0 [3,3], T0 [3]) float32, row convention Xt = X R + T.
    dynamic: Y uniform in the unit cube; X = n rows of Y (drawn with repetition where n > m) + 0.002 noise, pulled back by a random pose;
             the initial pose is that pose turned by 0.25 rad about the cube's centre and moved by 0.05.
    edge:    Y = the first m cells, in a random order, of a g^3 lattice filling the unit cube (cell h = 1 / g), each jittered by +-0.2 h per
             coordinate; X = n rows of Y, each displaced by at most 0.1 h, pulled back by a random pose; the initial pose is off by a turn of
             0.1 h at the cube's corner and a move of 0.1 h.  Two targets are at least 0.6 h apart and a transformed point is within ~0.3 h
             of its own, so the first search already finds the final assignment and the second iteration repeats it.
    A draw is kept when icp_well_posed() holds with a factor 2 in hand: 1 to 10 draws per case, 67 for the 18.  What rejects most of them is
    the lower end of e32(rmse), one number whose typical float32 error is the lower end itself."""
    key, fam, n, m = case
    if key not in _INPUTS:
        rng = _rng(key)
        while True:
            ins = _icp_draw(rng, fam, n, m)
            r = icp_ref(*ins)
            if icp_well_posed(r, n, 2.0):
                break
        _INPUTS[key], _REFS[key] = ins, r
    return _INPUTS[key]


ICP_BATCH = (65, 100)


def icp_batch_inputs():
    """three well-posed dynamic problems of one shape whose iteration counts all differ -> (X [3,n,3], Y [3,m,3], R0 [3,3,3], T0 [3,3], [their
    float64 iteration counts])"""
    key = f"icp-batch{ICP_BATCH}"
    if key not in _INPUTS:
        rng = _rng(key)
        kept = {}
        while len(kept) < 3:
            ins = _icp_draw(rng, "dynamic", *ICP_BATCH)
            r = icp_ref(*ins)
            if icp_well_posed(r, ICP_BATCH[0], 2.0):
                kept.setdefault(r["ref"].iterations, ins)
        _INPUTS[key] = tuple(np.stack([kept[k][j] for k in kept]) for j in range(4)) + (list(kept),)
    return _INPUTS[key]


def icp_ref(X, Y, R0, T0):
    """-> dict(ref = the float64 IcpResult, r32 = the float32 one, e32 = {measure: error}, e32_pose = the largest pose error (R's entries, T / s)
    of the float32 oracle at any iteration, s)"""
    r64, r32 = ro.icp(X, Y, R0, T0, dtype=F64), ro.icp(X, Y, R0, T0, dtype=F32)
    s = scale_of(X, Y)
    e32 = icp_errs((r32.R, r32.T, r32.rmse), (r64.R, r64.T, r64.rmse), s)
    pose = max(max(icp_errs((a["R"], a["T"], 0.0), (b["R"], b["T"], 0.0), s).values()) for a, b in zip(r32.trace, r64.trace))
    return dict(ref=r64, r32=r32, e32=e32, e32_pose=pose, s=s)


def icp_e32_min(measure, n):
    """rmse is a root MEAN square over n points: E32_MIN / sqrt(n), as for the mean residual"""
    return E32_MIN / n ** 0.5 if measure == "rmse" else E32_MIN


def icp_well_posed(r, n, hand=1.0):
    """the preconditions of an ICP input (hand = 1), or what a draw has to meet to be kept (hand = 2: a factor 2 in hand on e32, which is the
    host's float32 arithmetic as much as the input): the certificate holds for the pose error 16 x hand x e32_pose; the float32 oracle
    follows the float64 trajectory (iteration count, final assignment); hand x e32_min <= e32 <= E32_MAX / hand for every measure"""
    r64, r32 = r["ref"], r["r32"]
    return (ro.icp_certificate(r64.trace, r64.c, hand * r["e32_pose"]) and r32.iterations == r64.iterations and
            np.array_equal(r32.assignment, r64.assignment) and all(hand * icp_e32_min(k, n) <= e <= E32_MAX / hand for k, e in r["e32"].items()))


def icp_errs(out, ref, s):
    """out, ref = (R, T, rmse) -> {measure: error}"""
    d = lambda a, b: float(np.abs(np.asarray(a, dtype=F64) - np.asarray(b, dtype=F64)).max())    # noqa: E731
    return {"R": d(out[0], ref[0]), "T": d(out[1], ref[1]) / s, "rmse": d(out[2], ref[2]) / s}


def icp_reference(case):
    icp_inputs(case)
    return _REFS[case[0]]


# ------------------------------------------------------------------------------------------------ the rule
def judge(key, errs, e32, bad, table=None, path=None):
    """one problem: every measure under the rule; failures are appended to bad; table[path, measure] keeps the largest err / e32 with its key"""
    for k, err in errs.items():
        if not e32[k] <= E32_MAX:
            bad.append(f"{key} {k}: precondition e32 = {e32[k]:.3e} <= {E32_MAX:.0e} does not hold (ill-conditioned input)")
        if not err <= bound(e32[k]):
            bad.append(f"{key} {k}: err {err:.3e} > bound {bound(e32[k]):.3e} (e32 {e32[k]:.3e}, err / e32 {err / max(e32[k], 1e-300):.1f})")
        if table is not None:
            r = err / max(e32[k], 1e-300)
            if r > table.get(f"{path}  {k:8s}", (-1.0, ""))[0]:
                table[f"{path}  {k:8s}"] = (r, key)


def kabsch_preconditions(key, refs, n, bad, measures=KB_MEASURES):
    """gap >= GAP_MIN and e32_min <= e32 <= E32_MAX for every problem of a case"""
    for p, r in enumerate(refs):
        if not r["gap"] >= GAP_MIN:
            bad.append(f"{key} problem {p}: precondition gap = {r['gap']:.3e} >= {GAP_MIN} does not hold")
        for k in measures:
            if not e32_min(k, n) <= r["e32"][k] <= E32_MAX:
                bad.append(f"{key} problem {p} {k}: precondition {e32_min(k, n):.1e} <= e32 = {r['e32'][k]:.3e} <= {E32_MAX:.0e} does not hold")
        if not r.get("e32_entry", 0.0) <= E32_MAX:
            bad.append(f"{key} problem {p}: an entry's e32 = {r['e32_entry']:.3e} <= {E32_MAX:.0e} does not hold")


def format_table(table):
    return "\n".join(f"  max err / e32 = {r:7.2f}   {k}   ({where})" for k, (r, where) in sorted(table.items()))


def width_path(entry, n):
    return f"{entry:21s}  {'n<=256' if n <= 256 else 'n>256 '}"


# ------------------------------------------------------------------------------------------------ the device side
def _t(a, dev):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def check_kabsch(cases, dev, table, bad):
    """ops.kabsch on every case: status 0, then the measures of every problem"""
    from livingscenes_amd import ops
    for case in cases:
        x1, x2, w, raw = kabsch_inputs(case)
        R, t, res, fl = (o.cpu().numpy() for o in ops.kabsch(_t(x1, dev), _t(x2, dev), _t(w, dev), return_flags=True, raw_weights=raw))
        refs = kabsch_reference(case)
        kabsch_preconditions(case[0], refs, case[1], bad)
        for p, r in enumerate(refs):
            if fl[p] != 0:
                bad.append(f"{case[0]} problem {p}: status {int(fl[p])}, not 0")
            judge(f"{case[0]} problem {p}", kabsch_errs((R[p], t[p], res[p]), r["ref"], r["s"]), r["e32"], bad, table, width_path("kabsch", case[1]))


def check_codes(cases, dev, table, bad):
    from livingscenes_amd import ops
    for case in cases:
        z1, t1, z2, t2, sel1, sel2 = codes_inputs(case)
        R, t, res = (o.cpu().numpy() for o in ops.kabsch_codes(_t(z1, dev), _t(t1, dev), _t(z2, dev), _t(t2, dev), sel2=_t(sel2, dev),
                                                                sel1=_t(sel1, dev), want_res=True))
        refs = codes_reference(case)
        kabsch_preconditions(case[0], refs, case[1], bad)
        if len(refs) != R.shape[0]:
            bad.append(f"{case[0]}: {R.shape[0]} problems solved, {len(refs)} expected")
            continue
        for p, r in enumerate(refs):
            judge(f"{case[0]} problem {p}", kabsch_errs((R[p], t[p], res[p]), r["ref"], r["s"]), r["e32"], bad, table, width_path("kabsch_codes", case[1]))


def check_resmat(cases, dev, table, bad):
    """the single form on every problem with entries; the batch form where the case is a batch -- which must also give the single form's bits"""
    import torch
    from livingscenes_amd import ops
    for case in cases:
        key, sizes, P, batched = case
        ins, refs = resmat_inputs(case), resmat_reference(case)
        kabsch_preconditions(key, [r for r in refs if r["ref"].size], P, bad, ("mean_res",))
        single = [ops.kabsch_residual_matrix(_t(s, dev), _t(t, dev)) if s.shape[0] and t.shape[0] else torch.empty(s.shape[0], t.shape[0], device=dev)
                  for s, t in ins]
        runs = [("residual_matrix", single)]
        if batched:
            got = ops.kabsch_residual_matrix_batch([_t(s, dev) for s, _ in ins], [_t(t, dev) for _, t in ins])
            runs.append(("residual_matrix_batch", got))
            for q, (a, b) in enumerate(zip(got, single)):
                if a.shape != b.shape or not torch.equal(a, b):
                    bad.append(f"{key} problem {q}: the batch differs from the single call")
        for entry, outs in runs:
            for q, (o, r) in enumerate(zip(outs, refs)):
                if tuple(o.shape) != r["ref"].shape:
                    bad.append(f"{key} problem {q}: {entry} returns {tuple(o.shape)}, not {r['ref'].shape}")
                elif r["ref"].size:
                    judge(f"{key} problem {q}", resmat_err(o.cpu().numpy(), r), r["e32"], bad, table, width_path(entry, P))


def run_icp(case, flags, dev):
    """one ops.icp call on one problem -> (R [3,3], T [3], rmse, iterations) as numpy / Python numbers"""
    from livingscenes_amd import ops
    X, Y, R0, T0 = icp_inputs(case)
    R, T, rmse, it = ops.icp(_t(X[None], dev), _t(Y[None], dev), _t(R0[None], dev), _t(T0[None], dev), flags=flags)
    return R[0].cpu().numpy(), T[0].cpu().numpy(), float(rmse[0]), int(it[0])


def judge_icp(case, flags, out, table, bad):
    """the certificate, the iteration count, the final assignment recomputed in float64 from the kernel's pose, then the three measures"""
    r = icp_reference(case)
    key = f"{case[0]} contract={int(bool(flags))}"
    if not icp_well_posed(r, case[2]):
        bad.append(f"{key}: the preconditions do not hold (icp_well_posed): the inputs do not pin the trajectory, or e32 {r['e32']} is out of range")
    R, T, rmse, it = out
    X, Y, _, _ = icp_inputs(case)
    if it != r["ref"].iterations:
        bad.append(f"{key}: {it} iterations, the oracle takes {r['ref'].iterations}")
    nn = ro.nearest2(X.astype(F64) @ R.astype(F64) + T.astype(F64), Y)[0]
    if not np.array_equal(nn, r["ref"].assignment):
        bad.append(f"{key}: the final assignment differs from the oracle's at {int((nn != r['ref'].assignment).sum())} of {len(nn)} points")
    judge(key, icp_errs((R, T, rmse), (r["ref"].R, r["ref"].T, r["ref"].rmse), r["s"]), r["e32"], bad, table, icp_path(case, flags))


def check_icp(cases, dev, table, bad):
    """every case with contract off and on; a call the library refuses or fails to launch is a failure of that case, not of the run"""
    from livingscenes_amd import _lib
    for case in cases:
        for flags in (0, _lib.FLAG_CONTRACT_FMA):
            try:
                out = run_icp(case, flags, dev)
            except _lib.LsError as e:
                bad.append(f"{case[0]} contract={int(bool(flags))}: {e}")
                continue
            judge_icp(case, flags, out, table, bad)


def cpu_report():
    """every precondition of every ladder -> (lines, [what failed])"""
    bad, lines = [], []
    worst, least = dict.fromkeys(KB_MEASURES + ("mean_res",), 0.0), dict.fromkeys(KB_MEASURES + ("mean_res",), np.inf)
    gap = np.inf

    def seen(r, measures):
        nonlocal gap
        gap = min(gap, r["gap"])
        for k in measures:
            worst[k], least[k] = max(worst[k], r["e32"][k]), min(least[k], r["e32"][k])
    for lad, reference in ((kabsch_ladder(), kabsch_reference), (codes_ladder(), codes_reference)):
        for case in lad:
            refs = reference(case)
            kabsch_preconditions(case[0], refs, case[1], bad)
            for r in refs:
                seen(r, KB_MEASURES)
    for case in resmat_ladder():
        refs = [r for r in resmat_reference(case) if r["ref"].size]
        kabsch_preconditions(case[0], refs, case[2], bad, ("mean_res",))
        for r in refs:
            seen(r, ("mean_res",))
    lines.append("Kabsch ladders: smallest gap %.3e, e32 " % gap + ", ".join(f"{k} {least[k]:.2e} .. {worst[k]:.2e}" for k in worst))
    for case in icp_ladder():
        r = icp_reference(case)
        r64 = r["ref"]
        lines.append(f"{case[0]:34s} iterations {r64.iterations:2d} (float32 {r['r32'].iterations:2d})  e32 " +
                     " ".join(f"{k} {v:.2e}" for k, v in r["e32"].items()) + f"  e32_pose {r['e32_pose']:.2e}"
                     f"  margin {ro.icp_margin(r64.trace, r64.c, r['e32_pose']):.2e}  min d2-d1 {min(float((t['d2'] - t['d1']).min()) for t in r64.trace):.2e}"
                     f"  min gap {min(t['gap'] for t in r64.trace):.2f}")
        if not icp_well_posed(r, case[2]):
            bad.append(f"{case[0]}: the preconditions do not hold (icp_well_posed)")
    return lines, bad


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", action="store_true", help="run the ladders on the device under the rule")
    a = ap.parse_args()
    if not a.gpu:
        lines, bad = cpu_report()
        print("\n".join(lines))
    else:
        import torch
        assert torch.cuda.is_available(), "needs a HIP device"
        dev, table, bad = torch.device("cuda:0"), {}, []
        check_kabsch(kabsch_ladder(), dev, table, bad)
        check_codes(codes_ladder(), dev, table, bad)
        check_resmat(resmat_ladder(), dev, table, bad)
        check_icp(icp_ladder(), dev, table, bad)
        print(f"largest err / e32 per entry and path\n{format_table(table)}")
    print(f"{len(bad)} failures" + "".join("\n  " + b for b in bad[:400]))
    sys.exit(1 if bad else 0)
