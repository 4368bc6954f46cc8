"""The SDF decoder (FieldWrapper.forward + DeepSDF_Decoder.forward) and its gradients, in any floating-point type -- not a test module.
Composed of oracle.net's statements in their order (`mlp` restates net.decoder_forward so that the activation pattern can be stated and the
pre-activations read), every tensor cast to `dtype` first, so that in float32 `field` / `field_grads` reproduce
net.field_query / autograd through net.field_query_with_grad bit for bit (tests/test_sdf_oracle_cpu.py) and in float64 they are the yardstick
of sdf.hip and of the decoder part of model.hip (tests/test_hip_sdf_f64.py).  The hidden width, the number of layers and the skip position
come from `dcfg` alone.
  kind 'inner'   decoder_type "inner_deepsdf": u = [z_inv | <q, z_so3_c>_c | |q|], q = (query - t) / s      (net.field_query)
  kind 'xyz'     decoder_type "deepsdf":       u = [z_inv | query], the raw query; z_so3, s and t are not read
The SDF is judged per row against the instance's largest |ref| (sdf_err), the code / scale / translation gradients per instance
(glob_tail_oracle.per_instance_err's rule on each), the query gradient per row against the row's own upstream gradient (query_grad_err)."""
import torch
import torch.nn.functional as F

from edge_oracle import per_point_err
from oracle import net

__all__ = ["mlp", "field", "field_with_grad", "field_grads", "pattern_violations", "sdf_err", "sdf_err_rows", "query_grad_err", "instance_errs", "GRAD_NAMES"]
KINDS = ("inner", "xyz")
GRAD_NAMES = ("query", "z_so3", "z_inv", "s", "t")


def _decoder_input(query, code, kind):
    B, M, _ = query.shape
    z_inv = code["z_inv"]
    if kind == "xyz":
        return torch.cat([z_inv[:, None, :].expand(-1, M, -1), query], -1)
    assert kind == "inner", kind
    q = (query - code["t"]) / code["s"][:, None, None]
    inner = (q.unsqueeze(1) * code["z_so3"].unsqueeze(2)).sum(dim=-1)
    length = q.norm(dim=-1).unsqueeze(1)
    inv_query = torch.cat([inner, length], 1).transpose(2, 1)
    return torch.cat([z_inv[:, None, :].expand(-1, M, -1), inv_query], -1)


def _cast(dw, query, code, dtype):
    """(weights, query, code) in `dtype`; t as [B,1,3] (both [B,3] and [B,1,3] are taken)"""
    c = {k: v.to(dtype) for k, v in code.items()}
    if "t" in c:
        c["t"] = c["t"].reshape(-1, 1, 3)
    return {k: v.to(dtype) for k, v in dw.items()}, query.to(dtype), c


def mlp(w, cfg, inp, masks=None, trace=None):
    """net.decoder_forward's statements (DeepSDF_Decoder.forward, 'val') under the caller's grad mode.  trace (a list) receives every hidden
    layer's pre-activation z_l [B * M, out_l].  masks (one 0 / 1 tensor [B * M, out_l] per hidden layer): h_l = z_l * mask_l stands in for
    relu(z_l) -- the network on a STATED activation pattern.  The gradient of a ReLU network is defined only given the pattern: a unit whose
    pre-activation is zero to within the arithmetic's round-off may be counted on either side, and each choice moves a row's gradient by about
    1 / width; with the pattern stated, what is left to compare is arithmetic."""
    w = net.as_params(w)
    dims = [cfg["latent_size"] + cfg["pe_dim"]] + list(cfg["dims"]) + [1]
    n_layers = len(dims)
    B, M, Lw = inp.shape
    x0 = inp.reshape(-1, Lw)
    x = x0
    for layer in range(n_layers - 1):
        if layer in cfg["latent_in"]:
            x = torch.cat([x, x0], 1)
        if cfg["weight_norm"] and layer in cfg["norm_layers"]:
            W = net.fold_weight_norm(w[f"lin{layer}.weight_g"], w[f"lin{layer}.weight_v"])
        else:
            W = w[f"lin{layer}.weight"]
        x = F.linear(x, W, w[f"lin{layer}.bias"])
        if layer < n_layers - 2:
            if trace is not None:
                trace.append(x.detach())
            x = F.relu(x) if masks is None else x * masks[layer].to(x.dtype)
    return torch.tanh(x).view(B, M)


def field(dw, dcfg, query, code, dtype, kind, trace=None):
    """query [B,M,3], code {z_so3 [B,c,3], z_inv [B,c], s [B], t [B,1,3]} ('xyz': z_inv alone will do) -> sdf [B,M] in `dtype`"""
    w, q, c = _cast(dw, query, code, dtype)
    with torch.no_grad():
        return mlp(w, dcfg, _decoder_input(q, c, kind), trace=trace)


def field_with_grad(dw, dcfg, query, code, dtype, kind, masks=None, trace=None):
    """`field` with autograd enabled, on the tensors as given (the leaves are the caller's, already in `dtype`)"""
    w = {k: v.to(dtype) for k, v in dw.items()}
    with torch.enable_grad():
        return mlp(w, dcfg, _decoder_input(query, code, kind), masks, trace)


def field_grads(dw, dcfg, query, code, gsdf, dtype, kind, masks=None, trace=None):
    """-> (sdf [B,M], (g_query [B,M,3], g_z_so3 [B,c,3], g_z_inv [B,c], g_s [B], g_t [B,3])) of sum(gsdf * sdf) by autograd in `dtype`.  A query
    at the instance origin has gradient 0 through |q| (torch's norm backward); 'xyz': the gradients of z_so3, s and t are exact zeros.
    masks: on that activation pattern (mlp); None: on the pattern [z_l > 0] of this very evaluation, as autograd's relu has it."""
    _, q, c = _cast({}, query, code, dtype)
    q = q.detach().clone().requires_grad_(True)
    leaves = {k: c[k].detach().clone().requires_grad_(True) for k in ("z_so3", "z_inv", "s", "t")}
    sdf = field_with_grad(dw, dcfg, q, leaves, dtype, kind, masks, trace)
    (sdf * gsdf.to(dtype)).sum().backward()
    g = lambda v: torch.zeros_like(v) if v.grad is None else v.grad
    return sdf.detach(), (g(q), g(leaves["z_so3"]), g(leaves["z_inv"]), g(leaves["s"]), g(leaves["t"]).reshape(-1, 3))


def pattern_violations(masks, trace, tol):
    """masks: an activation pattern (bool / 0-1 [R, >= out_l] per hidden layer; columns past out_l are padding and must be off), trace: the float64
    pre-activations z_l [R, out_l] -> (units counted on the other side than [z_l > 0], those of them with |z_l| > tol * max_u |z_l[r, :]|).
    The first are the units a finite-precision forward may legitimately flip; the second are wrong."""
    flipped = wrong = 0
    assert len(masks) == len(trace)
    for m, z in zip(masks, trace):
        n = z.shape[1]
        m = torch.as_tensor(m).cpu() != 0
        assert m.shape[0] == z.shape[0] and m.shape[1] >= n, (m.shape, z.shape)
        differ = m[:, :n] != (z > 0)
        far = z.abs() > tol * z.abs().amax(1, keepdim=True)
        flipped += int(differ.sum())
        wrong += int((differ & far).sum()) + int(m[:, n:].sum())
    return flipped, wrong


# ------------------------------------------------------------------------------------------------ the error measures
def sdf_err(sdf, ref):
    """[B,M] each -> the largest, over all rows, of |sdf - ref| / max |ref| of the row's instance (an all-zero instance must be met exactly)"""
    B = ref.shape[0]
    return per_point_err(torch.as_tensor(sdf).reshape(B, -1, 1, 1), torch.as_tensor(ref).reshape(B, -1, 1, 1))


def sdf_err_rows(sdf, ref, counts):
    """the same for ragged rows: sdf, ref [R], counts = rows per instance in order (an instance without rows has no error)"""
    worst, r0 = 0.0, 0
    for n in counts:
        if n:
            worst = max(worst, sdf_err(torch.as_tensor(sdf)[r0:r0 + n][None], torch.as_tensor(ref)[r0:r0 + n][None]))
        r0 += n
    assert r0 == len(ref)
    return worst


def query_grad_err(gq, ref, gsdf):
    """gq, ref [B,M,3], gsdf [B,M] (no zero in it) -> max over the rows of ||gq[r] - ref[r]||_inf / (|gsdf[r]| G_b), G_b the instance's largest
    ||ref[r]||_inf / |gsdf[r]|: every row is judged on the scale of its own upstream gradient, so a row with a 2^-12 gradient cannot hide behind
    one with 2^0.  An instance whose reference is all zero must be met exactly."""
    gq, ref, g = torch.as_tensor(gq).double(), torch.as_tensor(ref).double(), torch.as_tensor(gsdf).double().abs()
    assert gq.shape == ref.shape and g.shape == ref.shape[:2] and bool((g > 0).all())
    diff = (gq - ref).abs().amax(-1) / g
    G = (ref.abs().amax(-1) / g).amax(1, keepdim=True)
    err = torch.where(G > 0, diff / G.clamp(min=1e-300), torch.where(diff > 0, torch.full_like(diff, float("inf")), torch.zeros_like(diff)))
    assert not torch.isnan(err).any()
    return float(err.max())


def instance_errs(a, ref):
    """(g_z_so3, g_z_inv, g_s, g_t) each with the instance axis first -> {name: the largest per-instance error}"""
    out = {}
    for name, x, r in zip(GRAD_NAMES[1:], a, ref):
        B = r.shape[0]
        out[name] = per_point_err(torch.as_tensor(x).reshape(B, -1, 1, 1), torch.as_tensor(r).reshape(B, -1, 1, 1))
    return out
