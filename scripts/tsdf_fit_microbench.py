"""The fit of the latent codes to the fused states (csrc/tsdffit.hip) against its yardsticks.

    python scripts/tsdf_fit_microbench.py [--instances 64] [--views 8] [--res 64] [--mesh-res 48] [--band 512] [--free 512] [--min-obs 1] [--reps 20]

The states of scripts/tsdf_mesh_microbench.py: P synth shapes, `views` rendered depth views each (synth.make_partial_views), fused into P
grids of res^3 samples (trunc = 4 voxels, empty pixels free, so that observed free space exists).  Timed with device events after
warm-up, median of `reps`, the forms alternating, the library calls on outputs already sized:
  draw        one ls_tsdf_draw_batch_f32 call (3 kernels) with quotas band + free per instance
  torch draw  the same samples from torch device ops, per problem: the two masks, nonzero, the ranks of the definition in int64
              arithmetic, index, gather; its samples are asserted IDENTICAL to the kernel's before anything is timed
  loss        one ls_tsdf_fit_loss_f64 call on [P, band + free] against the same loss and gradient from torch device ops (float64
              where / clamp / sum; equal within the rounding of the sum's order, asserted)
  step        one Adam step of More_Solver._optimize_code_on_fusion_batch (decoder forward, fit loss, decoder backward, Adam) against one
              step of _optimize_code_batch (the same with ops.mse) at the same P x N, in the same run; the released decoder's sizes with
              synthetic weights
Bytes: the draw must read sum and n of every sample (8 bytes) and write 25 bytes per column.  Nothing here was profiled with counters: the
figures are wall times of whole calls."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from livingscenes_amd import _lib, ops, synth  # noqa: E402
from livingscenes_amd.lib_more.more_solver import More_Solver  # noqa: E402
from livingscenes_amd.model_utils import Shape_Prior  # noqa: E402
from cloud_nearest_microbench import median_ms  # noqa: E402

PEAK = 8.0e12
GOLDEN = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1


def mix64(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def _i64(z):
    """the int64 with the bits of the uint64 z"""
    return z - (1 << 64) if z >= 1 << 63 else z


def _lsr(z, k):
    return (z >> k) & ((1 << (64 - k)) - 1)


def mix64_t(z):
    """mix64 on an int64 tensor holding uint64 bits (the products wrap, the shifts are made logical)"""
    z = (z ^ _lsr(z, 30)) * _i64(0xBF58476D1CE4E5B9)
    z = (z ^ _lsr(z, 27)) * _i64(0x94D049BB133111EB)
    return z ^ _lsr(z, 31)


def torch_draw(S, N, origin, h, trunc, n_band, n_free, seed, min_obs):
    """one problem in torch device ops -> (points, target, kind, index)"""
    dev = S.device
    s, n = S.reshape(-1), N.reshape(-1)
    eligible = n >= min_obs
    free = eligible & (s.long() == n.long() * 16384)
    cols = n_band + n_free
    index = torch.full((cols,), -1, dtype=torch.int64, device=dev)
    kind = torch.zeros(cols, dtype=torch.uint8, device=dev)
    at = 0
    for k, mask, m in ((1, eligible & ~free, n_band), (2, free, n_free)):
        where = torch.nonzero(mask).reshape(-1)
        L = where.shape[0]
        T = min(L, m)
        if T:
            j = torch.arange(T, dtype=torch.int64, device=dev)
            lo, hi = (j * L) // T, ((j + 1) * L) // T
            key = mix64(seed + k * GOLDEN)
            r = _lsr(mix64_t((j + 1) * _i64(GOLDEN) + _i64(key)), 32)
            index[at:at + T] = where[lo + ((r * (hi - lo)) >> 32)]
            kind[at:at + T] = k
        at += m
    safe = index.clamp(min=0)
    nz, ny = S.shape[2], S.shape[1]
    ijk = torch.stack([(safe // nz) // ny, (safe // nz) % ny, safe % nz], 1).double()
    points = (origin[None, :] + h * ijk).float()
    target = torch.where(index >= 0, trunc * (s[safe].double() / (n[safe].clamp(min=1).double() * 16384.0)), torch.zeros((), dtype=torch.float64, device=dev))
    return points, target, kind, index.int()


def torch_loss(sdf, s, trunc, target, kind):
    u, sd = sdf.double(), s.double()[:, None]
    e = torch.where(kind == 1, u - target / sd, torch.where(kind == 2, (u - trunc[:, None] / sd).clamp(max=0.0), torch.zeros_like(u)))
    m = (kind != 0).sum(1).clamp(min=1).double()
    return (e * e).sum(1) / m, (2.0 * e / m[:, None]).float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=64)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--res", type=int, default=64)
    ap.add_argument("--mesh-res", type=int, default=48)
    ap.add_argument("--band", type=int, default=512)
    ap.add_argument("--free", type=int, default=512)
    ap.add_argument("--min-obs", type=int, default=1)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    P, V, res, nb, nf = a.instances, a.views, a.res, a.band, a.free
    cols = nb + nf
    parts = synth.make_partial_views(range(P), V, res=a.mesh_res, with_depth=True, device=dev)
    clouds = [torch.cat(p["clouds"]) for p in parts]
    grids = More_Solver._fusion_grids(clouds, res, 4)
    S, N = ops.tsdf_state(P, (res,) * 3, dev)
    ops.depth_fuse_batch((S, N), [p["depth"] for p in parts], [p["intrinsics"] for p in parts], [p["world_to_cam"] for p in parts],
                         origin=grids["origin"], voxel=grids["voxel"], trunc=grids["trunc"], empty="free")
    o, h, tr = (np.ascontiguousarray(grids[k].numpy(), np.float64) for k in ("origin", "voxel", "trunc"))
    seeds = np.arange(P, dtype=np.uint64) + np.uint64(1)
    points = torch.empty(P, cols, 3, device=dev)
    target = torch.empty(P, cols, dtype=torch.float64, device=dev)
    kind = torch.empty(P, cols, dtype=torch.uint8, device=dev)
    index = torch.empty(P, cols, dtype=torch.int32, device=dev)
    counts = torch.empty(P, 3, dtype=torch.int64, device=dev)
    lib = _lib.load()
    ws = torch.empty(lib.ls_tsdf_draw_batch_workspace_bytes(P, res, res, res), dtype=torch.uint8, device=dev)
    st = _lib.stream_ptr(dev)

    def draw():
        _lib.call(dev, "ls_tsdf_draw_batch_f32", P, _lib.ptr(S), _lib.ptr(N), res, res, res, a.min_obs, ops._hptr(o), ops._hptr(h), ops._hptr(tr), nb, nf,
                  ops._hptr(seeds), _lib.ptr(points), _lib.ptr(target), _lib.ptr(kind), _lib.ptr(index), _lib.ptr(counts), _lib.ptr(ws), ws.numel(), st)

    od, hd, td = (torch.from_numpy(x).to(dev) for x in (o, h, tr))

    def torch_form():
        return [torch_draw(S[p], N[p], od[p], hd[p], td[p], nb, nf, int(seeds[p]), a.min_obs) for p in range(P)]
    # identical samples before anything is timed
    draw()
    torch.cuda.synchronize()
    ref = torch_form()
    assert torch.equal(torch.stack([r[3] for r in ref]), index), "the two forms disagree on the samples"
    assert torch.equal(torch.stack([r[2] for r in ref]), kind), "the two forms disagree on the kinds"
    assert torch.equal(torch.stack([r[0] for r in ref]).view(torch.int32), points.view(torch.int32)), "the two forms disagree on the points"
    assert torch.equal(torch.stack([r[1] for r in ref]).view(torch.int64), target.view(torch.int64)), "the two forms disagree on the targets"
    c = counts.cpu().numpy().copy()
    del ref
    # the loss on the decoder's values of these columns
    ecfg, dcfg = synth.default_encoder_cfg(), synth.default_decoder_cfg()
    sp = Shape_Prior.from_state(ecfg, dcfg, synth.make_encoder_weights(ecfg, 4), synth.make_decoder_weights(dcfg, 4), device=dev, n_pcl=cols)
    solver = More_Solver({"shape_priors": {"n_input_point": cols, "prior_name": "chair", "ckpt_dir": ""}, "fps": {"n_init": 1}}, model=sp)
    pc = solver._sample(clouds, cols)
    with torch.no_grad():
        code = sp.encode(pc.transpose(1, 2).contiguous())
    z_inv, z_so3 = code["z_inv"].detach().float().contiguous().clone(), code["z_so3"].detach().float().contiguous().clone()
    t, s_ = code["t"].detach().float().reshape(P, 3).contiguous().clone(), code["s"].detach().float().contiguous()
    s_row = s_.reshape(P).contiguous()
    hip = sp.hip_model()
    prev = hip.set_option(_lib.OPT_SDF_TRAIN_SPLITK, 0)
    sdf, _ = hip.sdf_decode_train(points, z_so3, z_inv, s_, t)
    loss, grad = ops.tsdf_fit_loss(sdf, s_row, td, target, kind)
    l_ref, g_ref = torch_loss(sdf, s_row, td, target, kind)
    assert float(((loss - l_ref).abs() / l_ref.clamp(min=1e-300)).max()) < cols * 2.0 ** -52, "the two forms disagree on the loss"
    assert float((grad - g_ref).abs().max()) <= 2.0 ** -23 * float(g_ref.abs().max()), "the two forms disagree on the gradient"
    inv_only = hip.desc.dec_input == _lib.DEC_XYZ
    groups = [(z_inv, 1e-5)] if inv_only else [(z_inv, 1e-5), (t, 1e-4), (z_so3, 5e-4)]
    opt_fit, opt_pts = ops.Adam(groups), ops.Adam(groups)
    min_fit, min_pts = torch.full((P,), 100.0, dtype=torch.float64, device=dev), torch.full((P,), 100.0, device=dev)
    imp = torch.zeros(P, dtype=torch.int32, device=dev)

    def step_fit():
        v, saved = hip.sdf_decode_train(points, z_so3, z_inv, s_, t)
        _, gs = ops.tsdf_fit_loss(v, s_row, td, target, kind, min_fit, imp)
        _, gso3, ginv, _, gt = hip.sdf_backward(saved, gs, need_query_grad=False)
        opt_fit.step([ginv] if inv_only else [ginv, gt, gso3])

    def step_points():
        v, saved = hip.sdf_decode_train(pc, z_so3, z_inv, s_, t)
        _, gs = ops.mse(v, min_pts, imp)
        _, gso3, ginv, _, gt = hip.sdf_backward(saved, gs, need_query_grad=False)
        opt_pts.step([ginv] if inv_only else [ginv, gt, gso3])

    fns = [draw, torch_form, lambda: ops.tsdf_fit_loss(sdf, s_row, td, target, kind), lambda: torch_loss(sdf, s_row, td, target, kind), step_fit,
           step_points]
    (t_d, t_td, t_l, t_tl, t_sf, t_sp), spread = median_ms(fns, a.reps)
    hip.set_option(_lib.OPT_SDF_TRAIN_SPLITK, prev)
    taken = (kind != 0).sum().item()
    print(f"instances {P} x {res}^3 samples fused from {V} views each, quotas {nb} + {nf}, min_obs {a.min_obs}; eligible {c[:, 0].sum()}, band "
          f"{c[:, 1].sum()}, free {c[:, 2].sum()} of {P * res ** 3}; columns taken {taken} of {P * cols}")
    names = ("draw", "torch draw", "loss", "torch loss", "step fit", "step pts")
    for name, tm, (lo, hi) in zip(names, (t_d, t_td, t_l, t_tl, t_sf, t_sp), spread):
        print(f"{name:10s} {tm:9.3f} ms (min {lo:.3f}, max {hi:.3f})")
    must = 8 * P * res ** 3 + 25 * P * cols
    print(f"draw: must-move {must / 2 ** 20:.0f} MiB (8 per sample in + 25 per column out) = {must / (t_d * 1e-3) / 1e9:.0f} GB/s, "
          f"{100 * must / (t_d * 1e-3) / PEAK:.1f} % of 8.0 TB/s; workspace {ws.numel() / 2 ** 20:.1f} MiB; torch / draw = {t_td / t_d:.1f}")
    print(f"loss: torch / loss = {t_tl / t_l:.1f}; one Adam step at P x N = {P} x {cols}: fit / points = {t_sf / t_sp:.3f}")


if __name__ == "__main__":
    main()
