"""The kernels of the optimisation-based registration (csrc/optim.hip, csrc/sinkhorn.hip) against float64 at their size edges: the cases, the
figures and the rule of tests/test_hip_optim_f64.py, which imports this file (docs/history.md section 48).

Softmin (ls_sinkhorn_softmin_f32, ls_sinkhorn_softmin_batched_f32 with and without grad_x, ls_sinkhorn_softmin_multi_f32): every (N, M) of
NS x MS, with pot_y given and null, prev / average on and off, on eight kinds of input (KINDS).  Figures PER ROW, so that a wrong row cannot hide
behind a large one, reduced to a maximum per pair:
    out :  |out_i - ref_i| / max(max_i |ref_i| over the pair, eps_p)      (eps_p is the natural unit of a potential)
    grad:  |grad_i - ref_i|_inf / D_i,  D_i = max_j |x_i - y_j|_inf       (the gradient is a convex combination of the row's displacements)
The whole divergence: the loss against |mean f_ba| + |mean f_aa| + |mean g_ab| + |mean g_bb| (the debiased loss is a difference of means, about 0
for identical clouds: it is judged on the scale of what cancels), the gradient per point against (D_i(x, y) + D_i(x, x)) / N.
The SE(3) step and the small kernels: see the functions below.

The rule is the project's (tests/tools/edge_vs_float64.py):  err <= min(16 x max(e32, 2^-23), 1e-4),  e32 the same figure of the float32 oracle
on the same inputs, e32 < 1e-5 a precondition of every case.  A reference that is exactly zero (the gradient of an ended pair, its `out` without
`prev`, a row with D_i = 0) is compared exactly.  A case that misses the precondition is re-seeded through RESEED (the first suffix that meets it),
never dropped."""
import binascii
import math
import os
import sys

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
for p in (REPO, os.path.join(REPO, "tests"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import sinkhorn_oracle as so  # noqa: E402
from edge_vs_float64 import E32_MAX, MARGIN, TOL  # noqa: E402
from oracle import optim as oo  # noqa: E402

FLOOR = 2.0 ** -23
F32, F64 = torch.float32, torch.float64
NS = (1, 3, 4, 5, 8, 9, 15, 16, 17, 31, 32, 33, 65)
MS = (1, 2, 63, 64, 65, 255, 256, 257, 300, 513)
SELF_NS = tuple(sorted(set(NS) | set(MS)))
KINDS = ("unit1", "unit", "scales", "offset", "dup", "self", "peak", "mixed")
BLUR2 = 0.05 ** 2
EXTENTS = (2.0 ** -6, 1.0, 2.0 ** 3)                 # 'scales'
MIXED_EPS = (0.5, 0.0025, 0.0, 2.0, -1.0)            # 'mixed': two ended pairs between live ones
VARIANTS = ((True, "plain"), (True, "prev"), (True, "avg"), (False, "plain"), (False, "prev"), (False, "avg"))   # (pot_y given, prev / average)
# cases whose first seed misses e32 < E32_MAX on one of the two hosts: key -> suffix (the first that meets it on both)
RESEED = {"softmin:scales:1:2": "#2", "softmin:offset:1:2": "#1", "softmin:offset:1:63": "#1", "softmin:dup:1:2": "#1", "softmin:dup:1:64": "#2",
          "softmin:dup:1:256": "#1", "softmin:dup:1:513": "#1", "softmin:mixed:1:2": "#1", "softmin:mixed:8:64": "#1",
          # the SE(3) step at step 399: the geodesic angle of the first seed lies within 1e-2 rad of stop_angle, or a tangent sum cancels
          "se3:1:1:399": "#3", "se3:1:255:399": "#1", "se3:1:256:399": "#2", "se3:1:1025:399": "#1", "se3:3:1:399": "#5", "se3:3:2:399": "#14",
          "se3:3:255:399": "#3", "se3:3:256:0": "#1", "se3:3:256:399": "#1", "se3:3:257:399": "#3", "se3:3:1025:399": "#10"}


def _gen(key):
    key = key + RESEED.get(key, "")
    return torch.Generator().manual_seed(binascii.crc32(key.encode()) & 0x7FFFFFFF)


def bound(e32):
    return min(MARGIN * max(e32, FLOOR), TOL)


class Tally:
    """largest err / e32 per (entry, figure), the failures, the largest e32 per figure"""

    def __init__(self):
        self.table, self.bad, self.e32 = {}, [], {}

    def judge(self, entry, figure, where, err, e32):
        """err, e32: per-pair tensors (float64) or numbers"""
        err, e32 = torch.as_tensor(err, dtype=F64).reshape(-1), torch.as_tensor(e32, dtype=F64).reshape(-1)
        for p in range(err.numel()):
            e, r = float(err[p]), float(e32[p])
            if math.isnan(r) and math.isnan(e):
                continue                                             # a pair that is compared exactly elsewhere
            w = f"{where} pair {p}"
            if not r < E32_MAX:
                self.bad.append(f"PRECONDITION {entry} {figure} {w}: e32 = {r:.3e}")
            if r > self.e32.get(figure, (0.0, ""))[0]:
                self.e32[figure] = (r, w)
            ratio = e / max(r, FLOOR)
            if not ratio <= self.table.get((entry, figure), (-1.0, ""))[0]:
                self.table[(entry, figure)] = (ratio, w)
            if not e <= bound(r):
                self.bad.append(f"{entry} {figure} {w}: err {e:.3e} > bound {bound(r):.3e} (e32 {r:.3e})")

    def exact(self, what, ok):
        if not ok:
            self.bad.append(f"EXACT {what}")

    def report(self, title):
        rows = "\n".join(f"  {e:<26s} {f:<8s} max err / e32 = {r:7.2f}   ({w})" for (e, f), (r, w) in sorted(self.table.items()))
        worst = ", ".join(f"{f} {r:.3e} ({w})" for f, (r, w) in sorted(self.e32.items()))
        return f"{title}\n{rows}\n  largest e32: {worst}"

    def check(self):
        assert not self.bad, f"{len(self.bad)} failures:\n" + "\n".join(self.bad[:30])


# ================================================================================================ softmin: cases and inputs
def peak_positions(M):
    last = (M - 1) // 256 * 256                       # first index of the last (partial or full) 4 x 64 chunk
    return sorted({j for j in (0, 63, 64, M - 1, last) if 0 <= j < M})


def softmin_cases(kind):
    """-> [(key, kind, N, M, extra)]"""
    out = []
    if kind == "self":
        return [(f"softmin:self:{n}", kind, n, n, None) for n in SELF_NS]
    for N in NS:
        for M in MS:
            if kind == "peak":
                out += [(f"softmin:peak:{N}:{M}:{j}", kind, N, M, j) for j in peak_positions(M)]
            else:
                out.append((f"softmin:{kind}:{N}:{M}", kind, N, M, None))
    return out


def _diameter(x, y):
    both = torch.cat([x, y], 1).double()
    return (both.amax(1) - both.amin(1)).norm(dim=1).clamp_min(1e-6)      # the clamp of divergence_batch: a pair that is one point stays live


_inputs = {}


def softmin_inputs(case):
    """x [P,N,3], y [P,M,3], pot [P,M], prev [P,N], eps [P] (float32), logw.  A pair's epsilon is an entry of its own schedule: d^2, d^2 / 4^k, or
    blur^2 -- the last only on clouds of extent <= 1 (at extent 8 and blur^2 the exponents reach 4 x 10^4 and the float32 oracle itself misses
    the precondition: see test_hip_optim_f64.py's docstring)."""
    key, kind, N, M, extra = case
    if key in _inputs:
        return _inputs[key]
    gen = _gen(key)
    c = binascii.crc32(key.encode())
    P = {"unit1": 1, "mixed": 5}.get(kind, 3)
    ext = torch.tensor(EXTENTS if kind == "scales" else (1.0,) * P)[:, None, None]
    x = torch.rand(P, N, 3, generator=gen) * ext
    y = torch.rand(P, M, 3, generator=gen) * ext + 0.1 * ext
    if kind == "offset":
        x, y = x + 100.0, y + 100.0
    if kind == "self":
        y = x.clone()
    if kind == "dup":
        idx = torch.arange(N)
        x[0, ::2] = y[0, idx[::2] % M]                # every other row of pair 0 is a y point
        y[1] = y[1, :1]                               # all y points of pair 1 are one point
        x[2] = y[2, (7 * idx) % M]                    # every row of pair 2 is a y point
    d = _diameter(x, y)
    eps = torch.empty(P, dtype=F64)
    for p in range(P):
        sel = (c + p) % 3
        big = kind == "scales" and EXTENTS[p] > 1.0
        eps[p] = d[p] ** 2 if sel == 0 else (BLUR2 if sel == 2 and not big else d[p] ** 2 / 4.0 ** (1 + (c >> 4) % 4 + (2 if sel == 2 else 0)))
    if kind == "mixed":
        eps = torch.tensor(MIXED_EPS, dtype=F64)
    eps = eps.float()
    logw = -math.log(M)
    # a potential as the loop hands it over: the softmin of y against x at the same epsilon (float64, rounded), moved by up to one epsilon
    live = eps.clamp_min(0) + (eps <= 0) * 1.0
    pot = so.softmin(y, x, None, -math.log(N), live)[0].float()
    pot = pot + live[:, None] * (torch.rand(P, M, generator=gen) * 2 - 1)
    prev = (torch.rand(P, N, generator=gen) * 2 - 1) * (d.float() ** 2)[:, None]
    if kind == "peak":
        pot[:, extra] += 12.0 * live                  # with pot_y: column j* dominates every row by e^12
        y[:, extra] = x[:, N // 2]                    # without: it is row N // 2's own position (cost 0)
    inp = {"x": x.contiguous(), "y": y.contiguous(), "pot": pot.contiguous(), "prev": prev.contiguous(), "eps": eps, "logw": logw, "P": P,
           "d": d}
    _inputs[key] = inp
    return inp


def _figs(out, grad, ref):
    """per-pair maxima of the two figures against ref = (out64, grad64, D, eps); nan where the pair is compared exactly (an ended pair)"""
    o64, g64, D, eps = ref
    live = eps > 0
    den = torch.maximum(o64.abs().amax(1), eps.double().clamp_min(0))
    fo = (out.double() - o64).abs().amax(1) / den
    fo[~live] = float("nan")
    fg = None
    if grad is not None:
        rows = ((grad.double() - g64).abs().amax(2) / D.clamp_min(1e-300))
        rows[D == 0] = 0.0
        fg = rows.amax(1)
        fg[~live] = float("nan")
    return fo, fg


_refs = {}


def softmin_reference(case, pot_on, variant):
    """-> (out64, grad64, D, eps, e32_out [P], e32_grad [P])"""
    k = (case[0], pot_on, variant)
    if k in _refs:
        return _refs[k]
    inp = softmin_inputs(case)
    pot = inp["pot"] if pot_on else None
    prev = None if variant == "plain" else inp["prev"]
    o64, g64, D = so.softmin(inp["x"], inp["y"], pot, inp["logw"], inp["eps"], prev, variant == "avg", F64)
    o32, g32, _ = so.softmin(inp["x"], inp["y"], pot, inp["logw"], inp["eps"], prev, variant == "avg", F32)
    ref = (o64, g64, D, inp["eps"])
    _refs[k] = ref + _figs(o32, g32, ref)
    return _refs[k]


def judge_softmin(tally, entry, where, out, grad, ref):
    """the rule on the live pairs; ended pairs and rows with D_i = 0 exactly"""
    o64, g64, D, eps, e_out, e_grad = ref
    out = out.cpu()
    fo, fg = _figs(out, None if grad is None else grad.cpu(), ref[:4])
    tally.judge(entry, "out", where, fo, e_out)
    dead = ~(eps > 0)
    tally.exact(f"{entry} {where}: out of an ended pair", torch.equal(out[dead], o64[dead].float()))
    if grad is not None:
        grad = grad.cpu()
        tally.judge(entry, "grad", where, fg, e_grad)
        tally.exact(f"{entry} {where}: gradient of an ended pair is not zero", bool((grad[dead] == 0).all()))
        tally.exact(f"{entry} {where}: gradient of a row without spread is not zero", bool((grad[D == 0] == 0).all()))


def single_reference(case, p, pot_on):
    """the single-pair entry takes the whole log-weight vector h = logw + pot / eps (float32, formed by the caller): h is the input here"""
    k = (case[0], "single", p, pot_on)
    if k not in _refs:
        inp = softmin_inputs(case)
        M = inp["y"].shape[1]
        h = torch.full((1, M), inp["logw"], dtype=F64)
        if pot_on:
            h = h + inp["pot"][p:p + 1].double() / inp["eps"][p].double()
        h = h.float()
        x, y, eps = inp["x"][p:p + 1], inp["y"][p:p + 1], inp["eps"][p:p + 1]
        o64, g64, D = so.softmin(x, y, None, h, eps, dtype=F64)
        o32, g32, _ = so.softmin(x, y, None, h, eps, dtype=F32)
        ref = (o64, g64, D, eps)
        _refs[k] = (h[0].contiguous(),) + ref + _figs(o32, g32, ref)
    return _refs[k]


def softmin_preconditions(kinds=KINDS):
    """every softmin reference of the ladder on the CPU: -> Tally whose .bad holds the cases that miss e32 < E32_MAX"""
    t = Tally()
    for kind in kinds:
        for case in softmin_cases(kind):
            for pot_on, variant in VARIANTS:
                ref = softmin_reference(case, pot_on, variant)
                t.judge("oracle", "out", f"{case[0]} {pot_on} {variant}", ref[4] * 0, ref[4])
                t.judge("oracle", "grad", f"{case[0]} {pot_on} {variant}", ref[5] * 0, ref[5])
            p, pot_on = single_pair_of(case)
            if p is not None:
                ref = single_reference(case, p, pot_on)
                t.judge("oracle", "out", f"{case[0]} single", ref[5] * 0, ref[5])
                t.judge("oracle", "grad", f"{case[0]} single", ref[6] * 0, ref[6])
    return t


def single_pair_of(case):
    """which pair of the case the single-pair entry runs, and whether its h carries the potential"""
    inp = softmin_inputs(case)
    c = binascii.crc32(case[0].encode())
    live = [p for p in range(inp["P"]) if float(inp["eps"][p]) > 0]
    return live[(c >> 8) % len(live)], bool((c >> 12) & 1)


def to_dev(inp, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) and k != "d" else v) for k, v in inp.items()}


# ================================================================================================ the whole divergence
DIV_SIZES = ((1, 1), (5, 63), (33, 65), (65, 257), (300, 517))
DIV_EXTENTS = (0.3, 1.0, 3.0)
BLUR = 0.05


def divergence_inputs(N, M):
    key = f"div:{N}:{M}"
    if key in _inputs:
        return _inputs[key]
    gen = _gen(key)
    ext = torch.tensor(DIV_EXTENTS)[:, None, None]
    x = (torch.rand(3, N, 3, generator=gen) * ext).contiguous()
    y = (torch.rand(3, M, 3, generator=gen) * ext + 0.1 * ext).contiguous()
    _inputs[key] = (x, y)
    return x, y


def divergence_reference(N, M):
    """per pair: loss64, grad64 [N,3], the loss scale, the gradient scale per point [N], the schedule length, e32 of both figures"""
    key = ("div", N, M)
    if key in _refs:
        return _refs[key]
    x, y = divergence_inputs(N, M)
    refs = []
    for p in range(3):
        d = float(_diameter(x[p:p + 1], y[p:p + 1])[0])
        frac = math.log2(d / BLUR) % 1.0
        assert min(frac, 1 - frac) >= 1e-3, (key, p, d)                         # else the two precisions may disagree on the schedule length
        l64, g64, means, n64 = so.divergence(x[p], y[p], BLUR, 0.5, F64)
        l32, g32, _, n32 = so.divergence(x[p], y[p], BLUR, 0.5, F32)
        assert n64 == n32, (key, p, n64, n32)
        ls = sum(abs(m) for m in means)
        Dxy = (x[p, :, None].double() - y[p, None].double()).abs().amax((1, 2))
        Dxx = (x[p, :, None].double() - x[p, None].double()).abs().amax((1, 2))
        gs = (Dxy + Dxx) / N
        e_loss = abs(float(l32) - float(l64)) / ls
        e_grad = float(((g32.double() - g64).abs().amax(1) / gs).max())
        refs.append((l64, g64, ls, gs, n64, e_loss, e_grad))
    _refs[key] = refs
    return refs


def judge_divergence(tally, entry, where, p, loss, grad, ref):
    l64, g64, ls, gs, _, e_loss, e_grad = ref
    tally.judge(entry, "loss", f"{where} extent {DIV_EXTENTS[p]}", abs(float(loss) - float(l64)) / ls, e_loss)
    tally.judge(entry, "grad", f"{where} extent {DIV_EXTENTS[p]}", float(((grad.cpu().double() - g64).abs().amax(1) / gs).max()), e_grad)


# ================================================================================================ SE(3) step and the small kernels
STEP_NS = (1, 2, 255, 256, 257, 1025)
STEP_PS = (1, 3)
G_SCALES = (2.0 ** -20, 2.0 ** -10, 1.0)
BETAS, ADAM_EPS = (0.9, 0.999), 1e-8


def rand_pose(gen, P, trans=0.5):
    g = torch.stack([oo.se3_exp(torch.randn(6, generator=gen, dtype=F64)) for _ in range(P)])
    g[:, :, 3] *= trans
    return g.float()


def relmax(a, b):
    """per pair (first axis): max |a - b| / max |b|"""
    a, b = a.double().reshape(a.shape[0], -1), b.double().reshape(b.shape[0], -1)
    return (a - b).abs().amax(1) / b.abs().amax(1).clamp_min(1e-300)


def transform_scale(g, src):
    """per point: max_c (|R| |x| + |t|)_c, the forward error scale of R x + t"""
    g, src = g.double(), src.double()
    return (src.abs() @ g[:, :, :3].abs().transpose(1, 2) + g[:, None, :, 3].abs()).amax(2)


def transform_fig(q, ref, scale):
    return ((q.double() - ref).abs().amax(2) / scale).amax(1)


def small_inputs(P, N):
    key = f"small:{P}:{N}"
    if key not in _inputs:
        gen = _gen(key)
        g = rand_pose(gen, P)
        src = torch.randn(P, N, 3, generator=gen) * 0.4
        sdf = torch.randn(P, N, generator=gen) * 1.5
        special = torch.tensor([1.0, -1.0, 0.0, 0.999999, -1.000001, 1.5, -2.5])       # the kink exactly, both sides of it, both branches
        sdf[0, :min(7, N)] = special[:min(7, N)]
        if N == 1 and P > 1:
            sdf[1, 0], sdf[2, 0] = -1.0, 0.999999
        base = torch.rand(P, generator=gen)
        _inputs[key] = (g, src, sdf, base)
    return _inputs[key]


def smooth_l1_ref(sdf, dtype):
    loss, grad = oo.smooth_l1(sdf.to(dtype))
    return loss, grad


def mse_ref(sdf, dtype):
    x = sdf.to(dtype)
    return (x * x).mean(1), 2 * x / x.shape[1]


def step_cases():
    """(key, P, N, step_no, stop_angle)"""
    out = []
    for P in STEP_PS:
        for N in STEP_NS:
            for step_no, stop in ((0, 0.03), (7, 10.0), (399, 0.03)):
                out.append((f"se3:{P}:{N}:{step_no}", P, N, step_no, stop))
    return out


def step_inputs(case):
    key, P, N, step_no, stop = case
    if key in _inputs:
        return _inputs[key]
    gen = _gen(key)
    sc = torch.tensor(G_SCALES[-P:] if P < 3 else G_SCALES)[:, None, None]
    src = torch.randn(P, N, 3, generator=gen) * 0.4
    g0 = rand_pose(gen, P)
    # point gradients with a common pull beside the noise, as a loss that wants the cloud moved gives them: the tangent sums are then no accidents
    G = (torch.randn(P, N, 3, generator=gen) + 0.3 * torch.randn(P, 1, 3, generator=gen)) * sc
    loss = torch.rand(P, generator=gen)
    m1 = torch.zeros(P, 6)
    m2 = torch.zeros(P, 6)
    if step_no:
        m1 = torch.randn(P, 6, generator=gen) * sc[:, 0] * math.sqrt(N) * 0.5
        m2 = (torch.rand(P, 6, generator=gen) + 0.5) * (sc[:, 0] ** 2) * N * 0.5
    _inputs[key] = {"src": src, "g0": g0, "G": G, "loss": loss, "m1": m1, "m2": m2, "lr": 0.05}
    return _inputs[key]


def _oracle_state(inp, case, dtype):
    _, P, N, step_no, stop = case
    st = oo.Se3AdamState(inp["g0"].to(dtype), inp["src"].to(dtype), stop, BETAS, ADAM_EPS)
    st.step_no = step_no
    st.m1.copy_(inp["m1"].to(dtype)), st.m2.copy_(inp["m2"].to(dtype))
    return st


def step_reference(case):
    """-> dict: the float64 state after the step, the scales, e32 per figure [P]; asserts the case's own preconditions (float64):
    every tangent component |sum| > 1e-3 x sum |terms| (else its sign, and a whole Adam step of size lr, is a rounding accident), the geodesic
    angle at least 1e-2 rad from stop_angle (acosf near 1 resolves about 3e-4), G^2 a normal float32 wherever G is not zero."""
    key = ("se3", case[0])
    if key in _refs:
        return _refs[key]
    inp = step_inputs(case)
    _, P, N, step_no, stop = case
    st64, st32 = _oracle_state(inp, case, F64), _oracle_state(inp, case, F32)
    q, G = st64.query.clone(), inp["G"].double()
    gr = oo.tangent_gradient(q, G)
    lin = G.abs().sum(1)
    rot = torch.stack([(q[..., 1] * G[..., 2]).abs() + (q[..., 2] * G[..., 1]).abs(), (q[..., 2] * G[..., 0]).abs() + (q[..., 0] * G[..., 2]).abs(),
                       (q[..., 0] * G[..., 1]).abs() + (q[..., 1] * G[..., 0]).abs()], -1).sum(1)
    terms = torch.cat([lin, rot], 1)                                                   # [P,6]
    ok = bool((gr.abs() > 1e-3 * terms).all()) and bool(((G * G).float()[G != 0] >= 2.0 ** -126).all())
    oo.se3_adam_step(st64, G, inp["loss"].double(), inp["lr"])
    oo.se3_adam_step(st32, inp["G"], inp["loss"], inp["lr"])
    R, R0 = st64.g[:, :, :3], st64.init_R
    ang = torch.acos((((R * R0).sum((1, 2)) - 1) / 2).clamp(-1, 1))
    ok = ok and bool(((ang - stop).abs() >= 1e-2).all())
    qs = transform_scale(st64.g, inp["src"])
    ref = {"st": st64, "terms": terms, "qscale": qs, "ok": ok, "angle": ang,
           "e32": {"m1": ((st32.m1.double() - st64.m1).abs() / ((1 - BETAS[0]) * terms)).amax(1) if step_no == 0 else relmax(st32.m1, st64.m1),
                   "m2": relmax(st32.m2, st64.m2), "g": relmax(st32.g, st64.g), "best_g": relmax(st32.best_g, st64.best_g),
                   "query": transform_fig(st32.query, st64.query, qs)},
           "active32": st32.active.clone()}
    _refs[key] = ref
    return ref


ADAM_NS = (1, 257, 64, 300)
ADAM_LRS = (1e-5, 1e-4, 5e-4, 1e-3)


def adam_inputs(count, step_no):
    """groups of unequal length; parameters of size 8 lr, so that a float32 ulp of a parameter is 1e-6 of the step it is judged against"""
    key = f"adam:{count}:{step_no}"
    if key not in _inputs:
        gen = _gen(key)
        groups = []
        for i in range(count):
            n, lr = ADAM_NS[i], ADAM_LRS[i]
            p = torch.randn(n, generator=gen) * 8 * lr
            g = torch.randn(n, generator=gen) * (1e-3, 1.0, 2.0 ** -10, 0.1)[i]
            m = torch.zeros(n) if step_no == 0 else torch.randn(n, generator=gen) * g.abs().mean() * 0.5
            v = torch.zeros(n) if step_no == 0 else (torch.rand(n, generator=gen) + 0.5) * (g * g).mean() * 0.5
            groups.append((p, g, m, v, lr))
        _inputs[key] = groups
    return _inputs[key]


def adam_ref(p, g, m, v, lr, step_no, dtype):
    """torch.optim.Adam's order of operations at `dtype`, every scalar formed in double and cast once (csrc/optim.hip: adam_multi_kernel)"""
    p, g, m, v = (t.to(dtype) for t in (p, g, m, v))
    b1, b2 = BETAS
    t = step_no + 1
    m = m + (g - m) * (1 - b1)
    v = b2 * v + (1 - b2) * g * g
    denom = v.sqrt() / math.sqrt(1 - b2 ** t) + ADAM_EPS
    return p - (lr / (1 - b1 ** t)) * (m / denom), m, v


def _forget(key):
    _inputs.pop(key, None)
    for k in [k for k in _refs if key in k]:
        del _refs[k]


def find_reseeds(limit=5e-6):
    """the RESEED entries this host asks for: for every case whose e32 reaches `limit` (half the precondition, so that the other host's float32
    rounding does not tip it) or that misses a precondition of its own, the first suffix that does not"""
    found = {}

    def search(key, worst):
        for i in range(0, 40):
            if i:
                RESEED[key] = f"#{i}"
                _forget(key)
            if worst() < limit:
                break
        else:
            raise RuntimeError(f"no seed for {key}")
        if i:
            found[key] = RESEED[key]

    for kind in KINDS:
        for case in softmin_cases(kind):
            def worst():
                w = 0.0
                for pot_on, variant in VARIANTS:
                    ref = softmin_reference(case, pot_on, variant)
                    w = max(w, float(torch.nan_to_num(ref[4]).max()), float(torch.nan_to_num(ref[5]).max()))
                ref = single_reference(case, *single_pair_of(case))
                return max(w, float(ref[5].max()), float(ref[6].max()))
            search(case[0], worst)
    for case in step_cases():
        def worst():
            r = step_reference(case)
            return max(float(e.max()) for e in r["e32"].values()) if r["ok"] else 1.0
        search(case[0], worst)
    return found


if __name__ == "__main__":
    import time
    t0 = time.time()
    if "--reseed" in sys.argv:
        print("RESEED =", find_reseeds())
    for kind in KINDS:
        t = softmin_preconditions((kind,))
        print(f"{kind}: {len(softmin_cases(kind))} cases, largest e32 " + ", ".join(f"{f} {r:.3e} ({w})" for f, (r, w) in sorted(t.e32.items())),
              f"; {len(t.bad)} miss the precondition", flush=True)
        for b in t.bad[:8]:
            print("   ", b)
    for N, M in DIV_SIZES:
        for p, r in enumerate(divergence_reference(N, M)):
            print(f"div {N} x {M} extent {DIV_EXTENTS[p]}: schedule {r[4]}, e32 loss {r[5]:.3e} grad {r[6]:.3e}")
    worst = {}
    for case in step_cases():
        r = step_reference(case)
        if not r["ok"]:
            print("se3 precondition missed:", case[0])
        for f, e in r["e32"].items():
            worst[f] = max(worst.get(f, 0.0), float(e.max()))
    print("se3 step e32:", worst)
    print(f"{time.time() - t0:.1f} s")
