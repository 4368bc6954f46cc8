"""One edge-conv layer of the encoder on given neighbour lists, in any floating-point type -- not a test module.
The message of layer i WITHOUT its residual global conv, composed only of oracle.net's functions and the attention lines of
net.encoder_forward (same statements, same order), so that in float32 it reproduces trace["msg_f_i"] of net.encoder_forward bit for bit
(tests/test_edge_oracle_cpu.py) and in float64 it is the yardstick of the HIP kernels (tests/test_hip_edge_layers_f64.py):
  destination   dst_f = src_f gathered at `rows` along the point axis (a down-sampling layer), else src_f itself
  edges         net.get_graph_feature(src_f, dst_f, K, cross=(i == 0), idx=knn)
  pool layers   mean over the neighbours of vec_lna(y, V)
  attention     k, v = vec_lna(y, K / V), q = vec_lna(dst_f, Q); k, q through channel_equi_vec_normalize; per head of atten_multi_head_c
                channels softmax over the neighbours of sum_c <k, q> / sqrt(3 head_c); the weighted sum of v
`per_point_err` is the comparison rule of the float64 tests: per destination point, max |a - ref| over the point's 3 x Co block relative to
the same block's max |ref|, then the max over the points."""
import numpy as np
import torch

from oracle import net


@torch.no_grad()
def layer(w, cfg, i, src_f, knn, rows, dtype):
    """src_f [B,Cin,3,Ns] (layer 0: the cloud as [B,1,3,N]), knn [B,Nd,16], rows [B,Nd] or None -> the message [B,Co,3,Nd] in `dtype`"""
    w = {k: v.to(dtype) for k, v in net.as_params(w).items() if k.split(".")[1] == str(i)}
    ns, hc, K = cfg.get("leak_neg_slope", 0.2), cfg["atten_multi_head_c"], cfg["num_knn"]
    src_f = src_f.to(dtype)
    C = src_f.shape[1]
    if rows is None:
        dst_f = src_f
    else:
        dst_f = torch.gather(src_f, dim=-1, index=torch.as_tensor(rows).to(torch.int64)[:, None, None, :].expand(-1, C, 3, -1))
    y, _ = net.get_graph_feature(src_f, dst_f, K, cross=(i == 0), idx=knn)
    Wv, Wvd = w[f"V_list.{i}.lin.weight"], w[f"V_list.{i}.act.lin_dir.weight"]
    if i < cfg["atten_start_layer"]:
        return net.vec_lna(y, Wv, Wvd, ns).mean(dim=-1)
    k = net.vec_lna(y, w[f"K_list.{i}.lin.weight"], w[f"K_list.{i}.act.lin_dir.weight"], ns)
    q = net.vec_lna(dst_f, w[f"Q_list.{i}.lin.weight"], w[f"Q_list.{i}.act.lin_dir.weight"], ns)
    v = net.vec_lna(y, Wv, Wvd, ns)
    k = net.channel_equi_vec_normalize(k)
    q = net.channel_equi_vec_normalize(q)
    qk = (k * q[..., None]).sum(2)
    B, C, N, Kn = qk.shape
    n_head = C // hc
    qk_c = qk.reshape(B, n_head, hc, N, Kn)
    atten = qk_c.sum(2, keepdim=True) / np.sqrt(3 * hc)
    atten = torch.softmax(atten, dim=-1)
    atten = atten.expand(-1, -1, hc, -1, -1).reshape(qk.shape).unsqueeze(2)
    return (atten * v).sum(-1)


def per_point_err(a, ref):
    """a, ref [B,Co,3,Nd] -> max over the points of max |a - ref| / max |ref| of the point's block; a point whose reference block is all zero
    must be reproduced exactly (its error counts as 0 if it is, as inf if not)"""
    a, ref = torch.as_tensor(a).double(), torch.as_tensor(ref).double()
    assert a.shape == ref.shape, (a.shape, ref.shape)
    diff = (a - ref).abs().amax(dim=(1, 2))
    top = ref.abs().amax(dim=(1, 2))
    err = torch.where(top > 0, diff / top.clamp(min=1e-300), torch.where(diff > 0, torch.full_like(diff, float("inf")), torch.zeros_like(diff)))
    assert not torch.isnan(err).any()
    return float(err.max())
