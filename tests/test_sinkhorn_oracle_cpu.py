"""tests/sinkhorn_oracle.py is the float64 reference of tests/test_hip_optim_f64.py.  Here, without a GPU: in float32 it IS the project's own
restatement oracle/sinkhorn.py (loss, autograd gradient and a single softmin, bit for bit), oracle/optim.py carries the dtype of its inputs, and
the epsilon column every pair of livingscenes_amd.sinkhorn.divergence_batch receives is the schedule of the single-pair definition."""
import math

import numpy as np
import pytest
import torch

import sinkhorn_oracle as so
from livingscenes_amd import sinkhorn as ls_sinkhorn
from oracle import optim as oo
from oracle import sinkhorn as osk


def _clouds(N, M, seed, extent=1.0):
    gen = torch.Generator().manual_seed(seed)
    return torch.rand(N, 3, generator=gen) * extent, torch.rand(M, 3, generator=gen) * extent + 0.1 * extent


@pytest.mark.parametrize("N,M", [(33, 65), (300, 517)])
def test_divergence_in_float32_is_the_oracle_bit_for_bit(N, M):
    x, y = _clouds(N, M, 1)
    xr = x.clone().requires_grad_(True)
    ref = osk.sinkhorn_divergence(xr, y)
    ref.backward()
    loss, grad, means, n = so.divergence(x, y, dtype=torch.float32)
    assert loss.dtype == torch.float32 and torch.equal(loss, ref.detach()) and torch.equal(grad, xr.grad)
    assert n == len(ls_sinkhorn.epsilon_schedule(max(float((torch.cat([x, y]).max(0)[0] - torch.cat([x, y]).min(0)[0]).norm()), 1e-6)))
    l64, g64, means64, n64 = so.divergence(x, y, dtype=torch.float64)
    assert l64.dtype == torch.float64 and g64.dtype == torch.float64 and n64 == n
    assert abs(float(l64) - float(loss)) < 1e-5 * sum(abs(m) for m in means64)


@pytest.mark.parametrize("N,M", [(33, 65), (300, 517)])
def test_softmin_in_float32_is_the_oracle_softmin_bit_for_bit(N, M):
    """on the same cost matrix: oracle.sinkhorn._softmin(eps, C, b_log + g / eps); the gradient, which oracle/sinkhorn.py leaves to
    autograd and the oracle states as softmax-weighted displacements, is autograd's of that expression in float64"""
    x, y = _clouds(N, M, 2)
    gen = torch.Generator().manual_seed(3)
    pot = torch.rand(M, generator=gen) - 0.5
    for eps in (0.0025, 0.3, 3.0):
        xr = x.clone().requires_grad_(True)
        C = 0.5 * ((xr[:, None, :] - y[None, :, :]) ** 2).sum(-1)
        ref = osk._softmin(eps, C, torch.full((M,), -math.log(M)) + pot / eps)
        ref.sum().backward()
        out, grad, D = so.softmin(x[None], y[None], pot[None], -math.log(M), torch.tensor([eps]), dtype=torch.float32)
        assert torch.equal(out[0], ref.detach())
        x64 = x.double().requires_grad_(True)
        C64 = 0.5 * ((x64[:, None, :] - y.double()[None, :, :]) ** 2).sum(-1)
        osk._softmin(eps, C64, torch.full((M,), -math.log(M), dtype=torch.float64) + pot.double() / eps).sum().backward()
        _, grad, D = so.softmin(x[None], y[None], pot[None], -math.log(M), torch.tensor([eps], dtype=torch.float64))
        assert float(((grad[0] - x64.grad).abs().amax(1) / D[0]).max()) < 1e-13
        prev = torch.rand(1, N, generator=gen)
        avg, _, _ = so.softmin(x[None], y[None], pot[None], -math.log(M), torch.tensor([eps]), prev, True, torch.float32)
        assert torch.equal(avg[0], 0.5 * (prev[0] + ref.detach()))
        # the single-pair entry's form: the whole log-weight vector in place of logw
        out_h, _, _ = so.softmin(x[None], y[None], None, (torch.full((M,), -math.log(M)) + pot / eps)[None], torch.tensor([eps]), dtype=torch.float32)
        assert torch.equal(out_h, out)


def test_softmin_ended_pairs_and_dtype():
    x, y = _clouds(5, 7, 4)
    x, y = x[None].repeat(3, 1, 1), y[None].repeat(3, 1, 1)
    prev = torch.arange(15.0).reshape(3, 5)
    eps = torch.tensor([0.0, 0.5, -1.0])
    out, grad, D = so.softmin(x, y, None, -math.log(7), eps, prev, True)
    assert out.dtype == grad.dtype == D.dtype == torch.float64
    assert torch.equal(out[0], prev[0].double()) and torch.equal(out[2], prev[2].double()) and not torch.equal(out[1], prev[1].double())
    assert float(grad[0].abs().max()) == 0 and float(grad[2].abs().max()) == 0 and float(grad[1].abs().max()) > 0
    out, _, _ = so.softmin(x, y, None, -math.log(7), eps)
    assert float(out[0].abs().max()) == 0 and float(out[2].abs().max()) == 0
    assert torch.equal(D[1], (x[1, :, None].double() - y[1, None].double()).abs().amax((1, 2)))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_oracle_optim_follows_the_dtype_of_its_inputs(dtype):
    gen = torch.Generator().manual_seed(5)
    P, N = 2, 9
    g0 = torch.stack([oo.se3_exp(torch.randn(6, generator=gen, dtype=torch.float64)) for _ in range(P)]).to(dtype)
    src, G = torch.randn(P, N, 3, generator=gen).to(dtype), torch.randn(P, N, 3, generator=gen).to(dtype)
    assert oo.se3_exp(torch.randn(6, generator=gen).to(dtype)).dtype == dtype
    assert oo.se3_transform(g0, src).dtype == dtype
    loss, grad = oo.smooth_l1(src[:, :, 0])
    assert loss.dtype == dtype and grad.dtype == dtype
    st = oo.Se3AdamState(g0, src, 10.0)
    assert oo.tangent_gradient(st.query, G).dtype == dtype
    oo.se3_adam_step(st, G, torch.rand(P, generator=gen).to(dtype), 0.05)
    for name in ("g", "m1", "m2", "min_loss", "best_g", "init_R", "query", "src"):
        assert getattr(st, name).dtype == dtype, name
    assert float(st.min_loss.max()) < 100 and not torch.equal(st.g, g0) and torch.equal(st.best_g, st.g)


# ------------------------------------------------------------------------------------------------ the epsilon columns of divergence_batch
def _diameters():
    blur = 0.05
    gen = torch.Generator().manual_seed(6)
    special = [0.0, 1e-7, 1e-6, 2e-6, 0.01, 0.049999, 0.05, 0.050001]
    special += [float(np.float32(blur * 2.0 ** k)) for k in range(-2, 12)]
    special += [float(np.nextafter(np.float32(blur * 2.0 ** k), np.float32(s))) for k in range(0, 4) for s in (0.0, 1e9)]
    rand = (10.0 ** (torch.rand(10000, generator=gen, dtype=torch.float64) * 5 - 3)).float().tolist()       # 1e-3 .. 1e2
    rand2 = (10.0 ** (torch.rand(10000, generator=gen, dtype=torch.float64) * 2 - 1.5)).float().tolist()    # the working range, 0.03 .. 3
    return torch.tensor(special + rand + rand2, dtype=torch.float32)


def test_every_pair_of_divergence_batch_receives_its_own_schedule(monkeypatch):
    """_softmin_multi and _softmin_b replaced by recording stubs (no GPU, no kernel): pair p of a batch must be handed epsilon_schedule(d_p)
    entry for entry (as the float32 the kernel reads), then zeros; the opening launch takes entry 0 and the closing softmins blur^2.  Diameters
    below blur, at the 1e-6 clamp, at the float32 blur * 2^k and their neighbours, and 2 x 10^4 random ones: 20 030 schedules, whose lengths
    (ceil of a quotient of logarithms on one side, len(np.arange) on the other) agree without exception."""
    d = _diameters()
    assert d.numel() == 20030
    P = d.numel()
    x = torch.zeros(P, 1, 3)
    y = torch.zeros(P, 1, 3)
    y[:, 0, 0] = d                                    # one point each: the bounding-box diameter of pair p is d[p] exactly
    multi, single = [], []

    def stub_multi(problems, eps, average):
        multi.append((eps.clone(), bool(average), len(problems)))
        return [torch.zeros(P, q[0].shape[1]) for q in problems]

    def stub_b(x_, y_, pot_y, logw, eps, prev=None, average=False, need_grad=False):
        single.append(eps.clone())
        out = torch.zeros(P, x_.shape[1])
        return (out, torch.zeros(P, x_.shape[1], 3)) if need_grad else out

    monkeypatch.setattr(ls_sinkhorn, "_softmin_multi", stub_multi)
    monkeypatch.setattr(ls_sinkhorn, "_softmin_b", stub_b)
    _, _, need = ls_sinkhorn.divergence_batch(x, y, return_need=True)
    cols = torch.stack([e for e, _, _ in multi[1:]], 1)                       # [P, L]
    L = cols.shape[1]
    assert len(multi) == L + 1 and not multi[0][1] and all(a for _, a, _ in multi[1:]) and all(n == 4 for _, _, n in multi)
    assert torch.equal(multi[0][0], cols[:, 0])
    assert len(single) == 4 and all(torch.equal(e, torch.full((P,), 0.05 ** 2)) for e in single)
    dc = d.clamp_min(1e-6).double().tolist()
    longest, bad = 0, []
    for p in range(P):
        want = ls_sinkhorn.epsilon_schedule(dc[p])
        longest = max(longest, len(want))
        want32 = torch.tensor(want + [0.0] * (L - len(want)), dtype=torch.float64).float()
        if len(want) > L or not torch.equal(cols[p], want32):
            bad.append((dc[p], len(want), cols[p].tolist()[:4], want32.tolist()[:4]))
    assert not bad, (len(bad), bad[:5])
    assert int(need) == longest == L
    # a caller's guess above the need: the added columns are zeros for every pair
    multi.clear()
    ls_sinkhorn.divergence_batch(x, y, lmax=L + 3)
    cols3 = torch.stack([e for e, _, _ in multi[1:]], 1)
    assert cols3.shape[1] == L + 3 and torch.equal(cols3[:, :L], cols) and float(cols3[:, L:].abs().max()) == 0
