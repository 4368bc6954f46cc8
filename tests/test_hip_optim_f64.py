"""The kernels of the optimisation-based registration -- the three softmin entries of csrc/optim.hip and csrc/sinkhorn.hip (softmin_rows<false, 8>,
softmin_rows<true, 4>, softmin_multi_kernel, the single-pair softmin_kernel), the two Sinkhorn loops around them, se3_transform / smooth_l1 / mse,
se3_adam_step_kernel and adam_multi_kernel -- against float64 (tests/sinkhorn_oracle.py, oracle/optim.py) at their size edges.  The cases, the
figures and the rule are tests/tools/optim_vs_float64.py:
    err <= min(16 x max(e32, 2^-23), 1e-4),
per row (softmin, transform, query), per point (gradients) or per pair, e32 the same figure of the float32 oracle computed here on the CPU from the
same inputs, e32 < 1e-5 asserted as a precondition of every case.  Softmin: N in {1, 3, 4, 5, 8, 9, 15, 16, 17, 31, 32, 33, 65} x M in {1, 2, 63,
64, 65, 255, 256, 257, 300, 513}, pot_y given and null, prev / average on and off, on unit clouds (P = 1 and 3), clouds of extent 2^-6 / 1 / 2^3
in one batch, clouds offset by 100, duplicated points, y = x, one dominant column at j = 0, 63, 64, M - 1 and the first index of the last
256-chunk, and a P = 5 batch with eps = (0.5, 0.0025, 0, 2.0, -1).  One pairing of the issue's list is not run: extent 8 at blur^2, where the
float32 oracle itself misses the precondition (exponents of 4 x 10^4; the pair takes d^2 / 4^k there).  With the figures go the exact relations:
a pair alone == its rows in the batch; an ended pair returns prev's bits or 0 and a zero gradient whatever `average` says; the first N' rows of a
call == a call of N' rows; multi == batched; lmax above the need == lmax None."""
import binascii
import ctypes
import importlib.util
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
TOOL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools", "optim_vs_float64.py")


def _load():
    spec = importlib.util.spec_from_file_location("optim_vs_float64", TOOL)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


lad = _load()   # one module object: the float64 references it caches serve every test of this file


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _batched(d, pot_on, variant, grad, rows=None, pair=None):
    """ls_sinkhorn_softmin_batched_f32 on the device copy `d` of a case's inputs (optionally its first `rows` rows / one pair alone)"""
    from livingscenes_amd.sinkhorn import _softmin_b
    x, y, pot, prev, eps = d["x"], d["y"], d["pot"] if pot_on else None, None if variant == "plain" else d["prev"], d["eps"]
    if rows is not None:
        x, prev = x[:, :rows].contiguous(), None if prev is None else prev[:, :rows].contiguous()
    if pair is not None:
        x, y, eps = x[pair:pair + 1], y[pair:pair + 1], eps[pair:pair + 1]
        pot, prev = None if pot is None else pot[pair:pair + 1], None if prev is None else prev[pair:pair + 1]
    r = _softmin_b(x, y, pot, d["logw"], eps, prev, variant == "avg", need_grad=grad)
    return r if grad else (r, None)


# ------------------------------------------------------------------------------------------------ softmin
@pytest.mark.parametrize("kind", lad.KINDS)
def test_softmin_batched_vs_float64_per_row(kind):
    """ls_sinkhorn_softmin_batched_f32 without and with grad_x at every (N, M), pot_y given / null x prev off / on / averaged.  Then bit for bit:
    the gradient form's `out` needs no second look (it is judged like the other); a pair alone == its rows in the batch; the first 1, 7, 8, 9 rows
    of a call == a call of that many rows."""
    dev, t = _dev(), lad.Tally()
    for case in lad.softmin_cases(kind):
        inp = lad.softmin_inputs(case)
        d = lad.to_dev(inp, dev)
        N = case[2]
        for pot_on, variant in lad.VARIANTS:
            ref = lad.softmin_reference(case, pot_on, variant)
            where = f"{case[0]} pot={int(pot_on)} {variant}"
            o8, _ = _batched(d, pot_on, variant, False)
            o4, g4 = _batched(d, pot_on, variant, True)
            lad.judge_softmin(t, "batched", where, o8, None, ref)
            lad.judge_softmin(t, "batched+grad", where, o4, g4, ref)
            if (pot_on, variant) not in ((True, "avg"), (False, "plain")):
                continue
            if inp["P"] > 1:
                for p in range(inp["P"]):
                    a8, _ = _batched(d, pot_on, variant, False, pair=p)
                    a4, ag = _batched(d, pot_on, variant, True, pair=p)
                    t.exact(f"{where}: pair {p} alone differs from its rows in the batch",
                            torch.equal(a8[0], o8[p]) and torch.equal(a4[0], o4[p]) and torch.equal(ag[0], g4[p]))
            if N >= 9 and kind in ("unit", "mixed"):
                for n in (1, 7, 8, 9):
                    a8, _ = _batched(d, pot_on, variant, False, rows=n)
                    a4, ag = _batched(d, pot_on, variant, True, rows=n)
                    t.exact(f"{where}: a call of {n} rows differs from the first {n} rows",
                            torch.equal(a8, o8[:, :n]) and torch.equal(a4, o4[:, :n]) and torch.equal(ag, g4[:, :n]))
    print(t.report(f"[softmin, {kind}] largest err / e32"))
    t.check()


@pytest.mark.parametrize("kind", lad.KINDS)
def test_softmin_single_pair_vs_float64_per_row(kind):
    """ls_sinkhorn_softmin_f32 (sinkhorn.hip: base e, 4 rows per workgroup) on one live pair of every case, h with and without the potential;
    `out` of the call without the gradient == `out` of the call with it."""
    from livingscenes_amd.sinkhorn import softmin
    dev, t = _dev(), lad.Tally()
    for case in lad.softmin_cases(kind):
        inp = lad.softmin_inputs(case)
        p, pot_on = lad.single_pair_of(case)
        ref = lad.single_reference(case, p, pot_on)
        x, y, h = inp["x"][p].contiguous().to(dev), inp["y"][p].contiguous().to(dev), ref[0].to(dev)
        out, grad = softmin(float(inp["eps"][p]), x, y, h, need_grad=True)
        lad.judge_softmin(t, "single", f"{case[0]} pair {p} pot={int(pot_on)}", out[None], grad[None], ref[1:])
        t.exact(f"{case[0]}: out without the gradient differs", torch.equal(softmin(float(inp["eps"][p]), x, y, h), out))
    print(t.report(f"[single-pair softmin, {kind}] largest err / e32"))
    t.check()


@pytest.mark.parametrize("kind", lad.KINDS)
def test_softmin_multi_equals_batched_and_float64(kind):
    """ls_sinkhorn_softmin_multi_f32 with 1 .. 4 problems of unequal N in one launch -- (x, y), (y, x), (x, x), (y, y) as a Sinkhorn iteration
    poses them, potentials and previous values of the matching lengths -- at every (N, M): every problem == the batched entry bit for bit, and
    problem 0 under the rule against float64."""
    from livingscenes_amd.sinkhorn import _softmin_b, _softmin_multi
    dev, t = _dev(), lad.Tally()
    for case in lad.softmin_cases(kind):
        inp = lad.softmin_inputs(case)
        d = lad.to_dev(inp, dev)
        c = binascii.crc32(case[0].encode())
        count = 1 + c % 4
        N, M = case[2], case[3]
        la, lb = -math.log(N), -math.log(M)
        for pot_on, variant in ((True, "avg"), (False, "plain"), (True, "prev")):
            x, y = d["x"], d["y"]
            pot, potx = (d["pot"], d["prev"]) if pot_on else (None, None)           # potentials on y (length M) and on x (length N)
            prev, prevy = (None, None) if variant == "plain" else (d["prev"], d["pot"])
            problems = [(x, y, pot, lb, prev), (y, x, potx, la, prevy), (x, x, potx, la, prev), (y, y, pot, lb, prevy)][:count]
            outs = _softmin_multi(problems, d["eps"], variant == "avg")
            where = f"{case[0]} count={count} pot={int(pot_on)} {variant}"
            lad.judge_softmin(t, "multi", where, outs[0], None, lad.softmin_reference(case, pot_on, variant))
            for k, (a, b, po, lw, pv) in enumerate(problems):
                one = _softmin_b(a, b, po, lw, d["eps"], pv, variant == "avg")
                t.exact(f"{where}: problem {k} differs from the batched entry", torch.equal(outs[k], one))
    print(t.report(f"[multi softmin, {kind}] largest err / e32"))
    t.check()


def test_softmin_refusals_name_their_entry():
    """out aliasing prev, average without prev, count 0 and 5, P = 0, N = 0, eps <= 0 in the single-pair entry: the error code, ls_last_error()
    names the entry, and nothing is written."""
    from livingscenes_amd import _lib
    from livingscenes_amd._lib import SoftminProblem, ptr, stream_ptr
    dev = _dev()
    lib = _lib.load()
    P, N, M = 2, 5, 7
    x, y = torch.rand(P, N, 3, device=dev), torch.rand(P, M, 3, device=dev)
    eps, prev, out = torch.full((P,), 0.5, device=dev), torch.rand(P, N, device=dev), torch.full((P, N), 7.0, device=dev)
    s = stream_ptr(dev)

    def batched(prev_, average, P_, N_, out_):
        return lib.ls_sinkhorn_softmin_batched_f32(ptr(x), ptr(y), None, -1.0, ptr(eps), ptr(prev_), average, P_, N_, M, ptr(out_), None, s)

    def multi(count, P_, average=0, prev_=None, out_=out):
        arr = (SoftminProblem * 5)()
        for i in range(5):
            arr[i] = SoftminProblem(ptr(x), ptr(y), None, ptr(prev_), ptr(out_), -1.0, N, M)
        return lib.ls_sinkhorn_softmin_multi_f32(ctypes.addressof(arr), count, ptr(eps), average, P_, s)

    def single(e):
        return lib.ls_sinkhorn_softmin_f32(ptr(x[0]), ptr(y[0]), ptr(torch.zeros(M, device=dev)), N, M, e, ptr(out), None, s)

    keep = prev.clone()
    with torch.cuda.device(dev):
        for what, entry, call in [("out aliases prev", "sinkhorn_softmin_batched", lambda: batched(prev, 0, P, N, prev)),
                                  ("average without prev", "sinkhorn_softmin_batched", lambda: batched(None, 1, P, N, out)),
                                  ("P = 0", "sinkhorn_softmin_batched", lambda: batched(None, 0, 0, N, out)),
                                  ("N = 0", "sinkhorn_softmin_batched", lambda: batched(None, 0, P, 0, out)),
                                  ("count 0", "sinkhorn_softmin_multi", lambda: multi(0, P)),
                                  ("count 5", "sinkhorn_softmin_multi", lambda: multi(5, P)),
                                  ("multi P = 0", "sinkhorn_softmin_multi", lambda: multi(1, 0)),
                                  ("multi: out aliases prev", "sinkhorn_softmin_multi", lambda: multi(2, P, 0, prev, prev)),
                                  ("multi: average without prev", "sinkhorn_softmin_multi", lambda: multi(2, P, 1)),
                                  ("single eps = 0", "sinkhorn_softmin", lambda: single(0.0)),
                                  ("single eps < 0", "sinkhorn_softmin", lambda: single(-1.0))]:
            rc = call()
            msg = lib.ls_last_error().decode()
            assert rc == -1 and msg.startswith(entry + ":"), (what, rc, msg)      # LS_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and torch.equal(prev, keep)


# ------------------------------------------------------------------------------------------------ the whole divergence
@pytest.mark.parametrize("N,M", lad.DIV_SIZES)
def test_divergence_vs_float64(N, M):
    """sinkhorn_divergence (the single-pair loop, autograd backward) and divergence_batch on three pairs of extent 0.3 / 1 / 3 (schedules of
    three lengths in one batch): loss and gradient per point under the rule; return_need == the oracle's schedule length;
    lmax = need + 1 and need + 3 == lmax None bit for bit (ended pairs pass through)."""
    from livingscenes_amd.sinkhorn import divergence_batch, sinkhorn_divergence
    dev, t = _dev(), lad.Tally()
    x, y = lad.divergence_inputs(N, M)
    refs = lad.divergence_reference(N, M)
    xd, yd = x.to(dev), y.to(dev)
    for p in range(3):
        xh = xd[p].clone().requires_grad_(True)
        loss = sinkhorn_divergence(xh[None], yd[p][None], lad.BLUR)
        loss.backward()
        lad.judge_divergence(t, "sinkhorn_divergence", f"{N} x {M}", p, loss.detach(), xh.grad, refs[p])
    loss, grad, need = divergence_batch(xd, yd, lad.BLUR, return_need=True)
    need = int(need)
    assert need == max(r[4] for r in refs) and len({r[4] for r in refs}) == 3, (need, [r[4] for r in refs])
    for p in range(3):
        lad.judge_divergence(t, "divergence_batch", f"{N} x {M}", p, loss[p], grad[p], refs[p])
    for extra in (1, 3):
        l2, g2 = divergence_batch(xd, yd, lad.BLUR, lmax=need + extra)
        t.exact(f"{N} x {M}: lmax = need + {extra} differs from lmax None", torch.equal(l2, loss) and torch.equal(g2, grad))
    print(t.report(f"[divergence {N} x {M}] largest err / e32"))
    t.check()


# ------------------------------------------------------------------------------------------------ SE(3) step and the small kernels
@pytest.mark.parametrize("P", lad.STEP_PS)
def test_transform_smooth_l1_mse_vs_float64(P):
    """ls_se3_transform_f32 per point against |R| |x| + |t|; ls_smooth_l1_f32 (both branches, the kink, accumulate) and ls_mse_f32: the loss per
    pair against itself (a sum of non-negative terms), the gradient per element against 1 / N; min_loss / improved as float64 decides them, and
    a tie l == min_loss (the device's own bits) improves nothing."""
    from livingscenes_amd import ops
    from oracle import optim as oo
    dev, t = _dev(), lad.Tally()
    F32, F64 = torch.float32, torch.float64
    for N in lad.STEP_NS:
        g, src, sdf, base = lad.small_inputs(P, N)
        where = f"P={P} N={N}"
        r64, r32 = oo.se3_transform(g.double(), src.double()), oo.se3_transform(g, src)
        sc = lad.transform_scale(g, src)
        t.judge("se3_transform", "query", where, lad.transform_fig(ops.se3_transform(g.to(dev), src.to(dev)).cpu(), r64, sc), lad.transform_fig(r32, r64, sc))
        # smooth_l1
        (l64, g64), (l32, g32) = lad.smooth_l1_ref(sdf, F64), lad.smooth_l1_ref(sdf, F32)
        loss, grad = ops.smooth_l1(sdf.to(dev))
        t.judge("smooth_l1", "loss", where, (loss.cpu().double() - l64).abs() / l64, (l32.double() - l64).abs() / l64)
        t.judge("smooth_l1", "grad", where, (grad.cpu().double() - g64).abs().amax(1) * N, (g32.double() - g64).abs().amax(1) * N)
        acc, _ = ops.smooth_l1(sdf.to(dev), loss=base.clone().to(dev))
        a64 = base.double() + l64
        t.judge("smooth_l1", "loss+", where, (acc.cpu().double() - a64).abs() / a64, ((base + l32).double() - a64).abs() / a64)
        # mse
        (l64, g64), (l32, g32) = lad.mse_ref(sdf, F64), lad.mse_ref(sdf, F32)
        min0 = torch.tensor([100.0, 0.0, 100.0])[:P]
        min_loss, improved = min0.clone().to(dev), torch.zeros(P, dtype=torch.int32, device=dev)
        loss, grad = ops.mse(sdf.to(dev), min_loss, improved)
        loss0, _ = ops.mse(sdf.to(dev))
        t.exact(f"mse {where}: the loss without min_loss differs", torch.equal(loss0, loss))
        t.judge("mse", "loss", where, (loss.cpu().double() - l64).abs() / l64, (l32.double() - l64).abs() / l64)
        t.judge("mse", "grad", where, (grad.cpu().double() - g64).abs().amax(1) * N, (g32.double() - g64).abs().amax(1) * N)
        want = l64 < min0.double()
        t.exact(f"mse {where}: improved", improved.cpu().bool().tolist() == want.tolist())
        t.exact(f"mse {where}: min_loss", torch.equal(min_loss.cpu(), torch.where(want, loss.cpu(), min0)))
        tie, improved = loss.clone(), torch.zeros(P, dtype=torch.int32, device=dev)
        ops.mse(sdf.to(dev), tie, improved)
        t.exact(f"mse {where}: a tie improved", not bool(improved.any()) and torch.equal(tie, loss))
    print(t.report(f"[transform, smooth_l1, mse; P = {P}] largest err / e32"))
    t.check()


def _device_state(inp, case, dev):
    from livingscenes_amd import ops
    st = ops.Se3Adam(inp["g0"].to(dev), inp["src"].to(dev), case[4], lad.BETAS, lad.ADAM_EPS)
    st.step_no = case[3]
    st.m1.copy_(inp["m1"]), st.m2.copy_(inp["m2"])
    return st


STATE = ("g", "m1", "m2", "min_loss", "best_g", "query", "active")


def _snapshot(st):
    return {k: getattr(st, k).clone() for k in STATE}


@pytest.mark.parametrize("P", lad.STEP_PS)
def test_se3_adam_step_vs_float64(P):
    """ONE ls_se3_adam_step_f32 launch at N = 1, 2, 255, 256, 257, 1025, step numbers 0 / 7 / 399, point gradients of magnitude 2^-20, 2^-10, 1
    in one batch: the tangent gradient (read through m1 at step 0 from zero moments) per component against the sum of |terms|, the moments, the
    new pose, the snapshot and the next query under the rule; the stop flag == the oracle's.  Exactly: G = 0 from zero moments leaves the pose
    bit-identical; a frozen pair is untouched in every buffer; loss == min_loss keeps the old snapshot."""
    from oracle import optim as oo
    dev, t = _dev(), lad.Tally()
    for case in [c for c in lad.step_cases() if c[1] == P]:
        inp, ref = lad.step_inputs(case), lad.step_reference(case)
        where, N, step_no = case[0], case[2], case[3]
        assert ref["ok"], f"{where}: a precondition of the case does not hold (tests/tools/optim_vs_float64.py: step_reference)"
        r, e = ref["st"], ref["e32"]
        st = _device_state(inp, case, dev)
        st.step(inp["G"].to(dev), inp["loss"].to(dev), inp["lr"])
        m1 = st.m1.cpu().double()
        t.judge("se3_adam_step", "m1", where, ((m1 - r.m1).abs() / ((1 - lad.BETAS[0]) * ref["terms"])).amax(1) if step_no == 0 else lad.relmax(m1, r.m1), e["m1"])
        t.judge("se3_adam_step", "m2", where, lad.relmax(st.m2.cpu(), r.m2), e["m2"])
        t.judge("se3_adam_step", "g", where, lad.relmax(st.g.cpu(), r.g), e["g"])
        t.judge("se3_adam_step", "best_g", where, lad.relmax(st.best_g.cpu(), r.best_g), e["best_g"])
        t.judge("se3_adam_step", "query", where, lad.transform_fig(st.query.cpu(), r.query, ref["qscale"]), e["query"])
        t.exact(f"{where}: min_loss", torch.equal(st.min_loss.cpu(), r.min_loss.float()))
        t.exact(f"{where}: stop flags {st.active.cpu().tolist()} against {r.active.tolist()}", st.active.cpu().bool().tolist() == r.active.tolist())
        # exact cases, from the same start
        z = _device_state({**inp, "m1": torch.zeros(P, 6), "m2": torch.zeros(P, 6)}, case, dev)
        q64 = oo.se3_transform(inp["g0"].double(), inp["src"].double())
        z.step(torch.zeros(P, N, 3, device=dev), inp["loss"].to(dev), inp["lr"])
        t.exact(f"{where}: G = 0 moved the pose", torch.equal(z.g.cpu(), inp["g0"]) and torch.equal(z.best_g.cpu(), inp["g0"]))
        sc = lad.transform_scale(inp["g0"], inp["src"])
        t.judge("se3_adam_step", "query0", where, lad.transform_fig(z.query.cpu(), q64, sc),
                lad.transform_fig(oo.se3_transform(inp["g0"], inp["src"]), q64, sc))
        f = _device_state(inp, case, dev)
        f.active[P - 1] = 0
        f.min_loss.copy_(inp["loss"])                       # a tie for every live pair
        before = _snapshot(f)
        f.step(inp["G"].to(dev), inp["loss"].to(dev), inp["lr"])
        t.exact(f"{where}: a frozen pair was touched", all(torch.equal(getattr(f, k)[P - 1], before[k][P - 1]) for k in STATE))
        t.exact(f"{where}: loss == min_loss replaced the snapshot", torch.equal(f.best_g, before["best_g"]) and torch.equal(f.min_loss, before["min_loss"]))
        if P > 1:
            t.exact(f"{where}: a live pair beside a frozen one differs from the full step", torch.equal(f.g[:P - 1], st.g[:P - 1]))
        e = _device_state(inp, case, dev)                   # the tie again with every pair live (at P = 1 the pair above is the frozen one)
        e.min_loss.copy_(inp["loss"])
        before = _snapshot(e)
        e.step(inp["G"].to(dev), inp["loss"].to(dev), inp["lr"])
        t.exact(f"{where}: loss == min_loss replaced the snapshot of a live pair",
                torch.equal(e.best_g, before["best_g"]) and torch.equal(e.min_loss, before["min_loss"]) and torch.equal(e.g, st.g))
    print(t.report(f"[se3_adam_step, P = {P}] largest err / e32"))
    t.check()


@pytest.mark.parametrize("step_no", [0, 399])
def test_adam_step_vs_float64(step_no):
    """ls_adam_step_f32 with 1 .. 4 groups of 1, 257, 64 and 300 elements, each with its own learning rate: one step, the parameter per element
    against its step size lr, the moments against their largest entry."""
    from livingscenes_amd import ops
    dev, t = _dev(), lad.Tally()
    F32, F64 = torch.float32, torch.float64
    for count in (1, 2, 3, 4):
        groups = lad.adam_inputs(count, step_no)
        ps = [p.clone().to(dev) for p, _, _, _, _ in groups]
        opt = ops.Adam([(p, lr) for p, (_, _, _, _, lr) in zip(ps, groups)], lad.BETAS, lad.ADAM_EPS)
        opt.step_no = step_no
        for i, (_, _, m, v, _) in enumerate(groups):
            opt.m[i].copy_(m), opt.v[i].copy_(v)
        opt.step([g.to(dev) for _, g, _, _, _ in groups])
        for i, (p, g, m, v, lr) in enumerate(groups):
            (p64, m64, v64), (p32, m32, v32) = lad.adam_ref(p, g, m, v, lr, step_no, F64), lad.adam_ref(p, g, m, v, lr, step_no, F32)
            where = f"count={count} step={step_no} group {i} (n={p.numel()})"
            t.judge("adam_step", "param", where, float((ps[i].cpu().double() - p64).abs().max()) / lr, float((p32.double() - p64).abs().max()) / lr)
            t.judge("adam_step", "m", where, lad.relmax(opt.m[i].cpu()[None], m64[None]), lad.relmax(m32[None], m64[None]))
            t.judge("adam_step", "v", where, lad.relmax(opt.v[i].cpu()[None], v64[None]), lad.relmax(v32[None], v64[None]))
    print(t.report(f"[adam_step, step {step_no}] largest err / e32"))
    t.check()
