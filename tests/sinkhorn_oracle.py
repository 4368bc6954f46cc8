"""The batched log-domain softmin of csrc/optim.hip / csrc/sinkhorn.hip and the debiased Sinkhorn divergence around it, in plain dense torch at
a chosen precision -- TEST INFRASTRUCTURE ONLY.  oracle/sinkhorn.py states the same divergence, but its weights `a_log` / `b_log` are float32
whatever its inputs are, so it cannot serve as a float64 reference; here every tensor is cast to `dtype` first and the dtype is carried through.
In float32 both functions reproduce oracle/sinkhorn.py bit for bit (tests/test_sinkhorn_oracle_cpu.py): the float32 twin of the float64 oracle
is the project's own restatement, not a third definition.
"""
import math

import numpy as np
import torch


def _cost(a, b):
    return 0.5 * ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)


def _softmin_c(eps, C, h):
    """oracle.sinkhorn._softmin, operation for operation"""
    return -eps * (h[None, :] - C / eps).logsumexp(1)


def softmin(x, y, pot_y, logw, eps, prev=None, average=False, dtype=torch.float64):
    """x [P,N,3], y [P,M,3], pot_y [P,M] or None, logw a number (or a [P,M] tensor of log-weights, the `h` of the single-pair entry), eps [P],
    prev [P,N] or None -> (out [P,N], grad [P,N,3], D [P,N]):
        v_ij = logw + pot_y_j / eps - |x_i - y_j|^2 / (2 eps);   out_i = -eps logsumexp_j v_ij;   grad_i = sum_j softmax_j(v_i.) (x_i - y_j)
    out is averaged with prev when `average`.  A pair with eps <= 0 has ended: out = prev (0 without prev), grad = 0, whatever `average` says.
    D_i = max_j |x_i - y_j|_inf, the spread of the displacements the gradient is a convex combination of."""
    x, y = x.detach().to(dtype), y.detach().to(dtype)
    P, N, _ = x.shape
    eps = torch.as_tensor(eps).detach().to(dtype).reshape(P)
    pot_y = None if pot_y is None else pot_y.detach().to(dtype)
    prev = None if prev is None else prev.detach().to(dtype)
    lw = logw.detach().to(dtype) if torch.is_tensor(logw) else torch.tensor(float(logw)).to(dtype)
    out, grad = torch.zeros(P, N, dtype=dtype), torch.zeros(P, N, 3, dtype=dtype)
    diff = x[:, :, None, :] - y[:, None, :, :]                                     # [P,N,M,3]
    D = diff.abs().amax(dim=(2, 3))
    for p in range(P):
        e = float(eps[p])
        if not e > 0:
            if prev is not None:
                out[p] = prev[p]
            continue
        h = lw[p] if lw.dim() else lw.expand(y.shape[1])
        if pot_y is not None:
            h = h + pot_y[p] / e
        C = _cost(x[p], y[p])
        o = _softmin_c(e, C, h)
        w = torch.softmax(h[None, :] - C / e, 1)
        grad[p] = (w[:, :, None] * diff[p]).sum(1)
        out[p] = 0.5 * (prev[p] + o) if average else o
    return out, grad, D


def schedule(x, y, blur=0.05, scaling=0.5, p=2, dtype=torch.float64):
    """the epsilon list of one pair (x [N,3], y [M,3]) as oracle/sinkhorn.py forms it, from the diameter taken in `dtype`"""
    both = torch.cat([x.detach().to(dtype), y.detach().to(dtype)], 0)
    diameter = max(float((both.max(0)[0] - both.min(0)[0]).norm()), 1e-6)
    return ([diameter ** p] + [float(np.exp(e)) for e in np.arange(p * math.log(diameter), p * math.log(blur), p * math.log(scaling))]
            + [blur ** p])


def divergence(x, y, blur=0.05, scaling=0.5, dtype=torch.float64):
    """oracle.sinkhorn.sinkhorn_divergence of one pair (x [N,3], y [M,3]) with the dtype carried through ->
    (loss, d loss / d x [N,3] by autograd, (mean f_ba, mean f_aa, mean g_ab, mean g_bb) of the last extrapolation, len(schedule))."""
    x = x.detach().reshape(-1, 3).to(dtype).clone().requires_grad_(True)
    y = y.detach().reshape(-1, 3).to(dtype)
    N, M = x.shape[0], y.shape[0]
    xd, yd = x.detach(), y.detach()
    eps_list = schedule(xd, yd, blur, scaling, 2, dtype)
    a_log = torch.full((N,), -math.log(N), dtype=dtype)
    b_log = torch.full((M,), -math.log(M), dtype=dtype)
    with torch.no_grad():
        Cxy, Cyx, Cxx, Cyy = _cost(xd, yd), _cost(yd, xd), _cost(xd, xd), _cost(yd, yd)
        eps = eps_list[0]
        g_ab, f_ba = _softmin_c(eps, Cyx, a_log), _softmin_c(eps, Cxy, b_log)
        f_aa, g_bb = _softmin_c(eps, Cxx, a_log), _softmin_c(eps, Cyy, b_log)
        for eps in eps_list:
            ft_ba = _softmin_c(eps, Cxy, b_log + g_ab / eps)
            gt_ab = _softmin_c(eps, Cyx, a_log + f_ba / eps)
            ft_aa = _softmin_c(eps, Cxx, a_log + f_aa / eps)
            gt_bb = _softmin_c(eps, Cyy, b_log + g_bb / eps)
            f_ba, g_ab = 0.5 * (f_ba + ft_ba), 0.5 * (g_ab + gt_ab)
            f_aa, g_bb = 0.5 * (f_aa + ft_aa), 0.5 * (g_bb + gt_bb)
    f_ba_l = _softmin_c(eps, _cost(x, yd), b_log + g_ab / eps)
    g_ab_l = _softmin_c(eps, _cost(yd, xd), a_log + f_ba / eps)
    f_aa_l = _softmin_c(eps, _cost(x, xd), a_log + f_aa / eps)
    g_bb_l = _softmin_c(eps, _cost(yd, yd), b_log + g_bb / eps)
    loss = (f_ba_l - f_aa_l).mean() + (g_ab_l - g_bb_l).mean()
    loss.backward()
    means = tuple(float(t.detach().mean()) for t in (f_ba_l, f_aa_l, g_ab_l, g_bb_l))
    return loss.detach(), x.grad, means, len(eps_list)
