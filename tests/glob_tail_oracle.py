"""The residual global conv of one layer and the encoder's tail, in any floating-point type -- not a test module.
Composed only of oracle.net's functions and the statements of net.encoder_forward (the residual branch and everything after the layer loop), in
the same order, so that in float32 they reproduce trace["dst_f_i"] from trace["msg_f_i"] and the four outputs of net.encoder_forward bit for
bit (tests/test_glob_tail_oracle_cpu.py) and in float64 they are the yardstick of the HIP kernels (tests/test_hip_glob_tail_f64.py):
  global_conv   vec_lna(cat(msg, mean_n msg), global_conv_list.j), j = i - res_global_start_layer
  tail          xx = mean_n vec_lna(f, conv_c); z_so3 = cevn(xx); scale = mean_c |xx_c| * scale_factor; z_inv = <cevn(fc_inv xx), z_so3>;
                center = vec_resblock(xx, fc_center) (* scale_factor with center_pred_scale).  Without center_pred the reference's encoder
                returns no center at all (vec_dgcnn_atten.py:246-252: the flag guards the head AND its scaling) and the library's t is
                its centroid argument alone: center = 0 here, whatever center_pred_scale says.
The global conv is judged per point (edge_oracle.per_point_err); the tail per instance (per_instance_err): for each instance and each of
z_so3, z_inv, s, t, max |a - ref| over the instance's values / max |ref| over the same values, an all-zero reference reproduced exactly."""
import torch

from edge_oracle import per_point_err
from oracle import net

__all__ = ["global_conv", "tail", "per_point_err", "per_instance_err"]


@torch.no_grad()
def global_conv(w, cfg, i, msg, dtype):
    """msg [B,Co,3,N], the message of layer i >= res_global_start_layer -> the layer's output [B,Co,3,N] in `dtype`"""
    j = i - cfg["res_global_start_layer"]
    assert cfg.get("use_res_global_conv", True) and j >= 0, i
    w = {k: v.to(dtype) for k, v in net.as_params(w).items() if k.startswith(f"global_conv_list.{j}.")}
    ns = cfg.get("leak_neg_slope", 0.2)
    dst_f = msg.to(dtype)
    g = dst_f.mean(dim=-1)
    dst_f = torch.cat([dst_f, g[..., None].expand_as(dst_f)], 1)
    return net.vec_lna(dst_f, w[f"global_conv_list.{j}.lin.weight"], w[f"global_conv_list.{j}.act.lin_dir.weight"], ns)


@torch.no_grad()
def tail(w, cfg, f, dtype):
    """f [B,Cl,3,NP], the last layer's output -> (z_so3 [B,c,3], z_inv [B,c], scale [B], center [B,1,3]) in `dtype`"""
    w = {k: v.to(dtype) for k, v in net.as_params(w).items() if k.split(".")[0] in ("conv_c", "fc_inv", "fc_center")}
    ns = cfg.get("leak_neg_slope", 0.2)
    dst_f = f.to(dtype)
    xx = net.vec_lna(dst_f, w["conv_c.lin.weight"], w["conv_c.act.lin_dir.weight"], ns)
    xx = xx.mean(dim=-1)
    z_so3 = net.channel_equi_vec_normalize(xx)
    scale = xx.norm(dim=-1).mean(1) * cfg["scale_factor"]
    z_inv_dual = net.vec_linear(xx[..., None], w["fc_inv.weight"]).squeeze(-1)
    z_inv = (net.channel_equi_vec_normalize(z_inv_dual) * z_so3).sum(-1)
    if cfg.get("center_pred", False):
        center = net.vec_resblock(xx[..., None], w, "fc_center.", ns).squeeze(-1)
        if cfg.get("center_pred_scale", False):
            center = center * cfg["scale_factor"]
    else:
        center = torch.zeros(xx.shape[0], 1, 3, dtype=dtype)
    return z_so3, z_inv, scale, center


TAIL_NAMES = ("z_so3", "z_inv", "s", "t")


def per_instance_errs(a, ref):
    """a, ref: (z_so3, z_inv, s, t), each with the instance axis first -> {name: the largest per-instance error}.  per_point_err on a
    [B, n, 1, 1] view takes its two maxima over exactly one instance's values, and keeps its rule for an all-zero reference."""
    assert len(a) == len(ref) == 4
    out = {}
    for name, x, r in zip(TAIL_NAMES, a, ref):
        B = r.shape[0]
        out[name] = per_point_err(torch.as_tensor(x).reshape(B, -1, 1, 1), torch.as_tensor(r).reshape(B, -1, 1, 1))
    return out


def per_instance_err(a, ref):
    return max(per_instance_errs(a, ref).values())
