"""The completion of the fused states by the shape prior's field (csrc/tsdfprior.hip) against its yardstick.

    python scripts/tsdf_prior_microbench.py [--instances 64] [--views 8] [--res 64] [--mesh-res 48] [--reps 20]

The states of scripts/depth_fuse_microbench.py: P synth shapes, `views` rendered depth views of 100 x 100 each
(synth.make_partial_views), fused into P grids of res^3 samples (trunc = 4 voxels, empty pixels unknown).  For the prior weights 1 and 8,
timed with device events after warm-up, median of `reps`, the forms alternating, the library calls on outputs already sized:
  rows        one ls_tsdf_prior_rows_batch_f32 call (classify, scan, emit)
  vote        one ls_tsdf_prior_vote_batch_f32 call (classify, scan, vote) on the decoder's values of those rows
  torch rows  the same rows from torch device ops, the whole batch at once: nonzero of weight - n > 0, the lattice index, the float64
              position rounded once
  torch vote  the same state from torch device ops: gather of n and s by the rows' instance, where / clamp / floor in float64, the
              integer products scattered into copies of the state
Rows, row order and the completed state of the two forms are asserted IDENTICAL before anything is timed.  Reported apart: the sizing
protocol of ops.tsdf_prior_rows_batch (sizing call, one host read, real call) and the share of the decoder
(HipModel.sdf_decode_rows, the released sizes with synthetic weights) in More_Solver._complete_fusion_batch -- expected to dominate.
Must-move bytes: the vote reads 8 and writes 8 per sample and reads 4 per row; the rows write 20 per row (and must read n: 4 per
sample).  Nothing here was profiled with counters and no bound is claimed: the figures are wall times of whole calls."""
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


def torch_rows(N, od, hd, w0):
    """the whole batch in torch device ops -> (points, row_inst, row_index)"""
    P, nx, ny, nz = N.shape
    at = torch.nonzero((w0 - N.reshape(P, -1)) > 0)                              # lexicographic: problems in order, ascending index
    p, i = at[:, 0], at[:, 1]
    ijk = torch.stack([(i // nz) // ny, (i // nz) % ny, i % nz], 1).double()
    return (od[p] + hd[p][:, None] * ijk).float(), p.int(), i.int()


def torch_vote(S, N, f, p, i, sd, td, w0):
    """-> (sum', n'), copies of the state with the votes scattered in"""
    P = S.shape[0]
    V = S[0].numel()
    lin = p.long() * V + i.long()
    w = w0 - N.reshape(-1)[lin].long()
    cast = ~torch.isnan(f)
    t = ((sd[p.long()] * f.double()) / td[p.long()]).clamp(-1.0, 1.0)
    q = torch.floor(torch.where(cast, t, torch.zeros_like(t)) * 16384.0 + 0.5).long()
    zero = torch.zeros_like(w)
    So, No = S.reshape(-1).clone(), N.reshape(-1).clone()
    So[lin] += torch.where(cast, w * q, zero).int()
    No[lin] += torch.where(cast, w, zero).int()
    return So.reshape(S.shape), No.reshape(N.shape)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=64)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--res", type=int, default=64)
    ap.add_argument("--mesh-res", type=int, default=48)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    P, V, res = a.instances, a.views, a.res
    parts = synth.make_partial_views(range(P), V, res=a.mesh_res, with_depth=True, device=dev)
    clouds = [torch.cat(p["clouds"]) for p in parts]
    grids = More_Solver._fusion_grids(clouds, res, 4)
    S, N = ops.tsdf_state(P, (res,) * 3, dev)
    ops.depth_fuse_batch((S, N), [p["depth"] for p in parts], [p["intrinsics"] for p in parts], [p["world_to_cam"] for p in parts],
                         origin=grids["origin"], voxel=grids["voxel"], trunc=grids["trunc"])
    o, h, tr = (np.ascontiguousarray(grids[k].numpy(), np.float64) for k in ("origin", "voxel", "trunc"))
    od, hd, td = (torch.from_numpy(x).to(dev) for x in (o, h, tr))
    fusion = {"sum": S, "n": N, "origin": o, "voxel": h, "trunc": tr}
    n_in = 512
    ecfg, dcfg = synth.default_encoder_cfg(), synth.default_decoder_cfg()
    sp = Shape_Prior.from_state(ecfg, dcfg, synth.make_encoder_weights(ecfg, 4), synth.make_decoder_weights(dcfg, 4), device=dev, n_pcl=n_in)
    solver = More_Solver({"shape_priors": {"n_input_point": n_in, "prior_name": "chair", "ckpt_dir": ""}, "fps": {"n_init": 1}}, model=sp)
    with torch.no_grad():
        code = sp.encode(solver._sample(clouds, n_in).transpose(1, 2).contiguous())
    code = {k: v.detach() for k, v in code.items()}
    s_host = code["s"].float().reshape(P).double().cpu().numpy()
    sd = torch.from_numpy(s_host).to(dev)
    hip = sp.hip_model()
    lib = _lib.load()
    ws = torch.empty(lib.ls_tsdf_prior_rows_batch_workspace_bytes(P, res, res, res), dtype=torch.uint8, device=dev)
    st = _lib.stream_ptr(dev)
    voxels = P * res ** 3
    print(f"instances {P} x {res}^3 samples fused from {V} views each; observed {int((N > 0).sum())} of {voxels}; workspace {ws.numel() / 2 ** 20:.1f} MiB")
    for w0 in (1, 8):
        rows = ops.tsdf_prior_rows_batch((S, N), origin=o, voxel=h, weight=w0, packed=True)
        points, inst, index, off, counts = rows
        R = off[P]
        f = hip.sdf_decode_rows(points, inst, code["z_so3"], code["z_inv"], code["s"].float().contiguous(), code["t"])
        (S2, N2), vcounts = ops.tsdf_complete_batch((S, N), f, rows, s=s_host, trunc=tr, weight=w0)
        # identical results before anything is timed
        tp, ti, tx = torch_rows(N, od, hd, w0)
        assert torch.equal(tx, index) and torch.equal(ti, inst) and torch.equal(tp.view(torch.int32), points.view(torch.int32)), "the two forms disagree on the rows"
        tS, tN = torch_vote(S, N, f, inst, index, sd, td, w0)
        assert torch.equal(tS, S2) and torch.equal(tN, N2), "the two forms disagree on the completed state"
        del tp, ti, tx, tS, tN
        row_off = torch.empty(P + 1, dtype=torch.int64, device=dev)
        cnt = torch.empty(P, 4, dtype=torch.int64, device=dev)

        def k_rows():
            _lib.call(dev, "ls_tsdf_prior_rows_batch_f32", P, _lib.ptr(N), res, res, res, w0, ops._hptr(o), ops._hptr(h), _lib.ptr(points), _lib.ptr(inst),
                      _lib.ptr(index), R, _lib.ptr(row_off), _lib.ptr(cnt), _lib.ptr(ws), ws.numel(), st)

        def k_vote():
            _lib.call(dev, "ls_tsdf_prior_vote_batch_f32", P, _lib.ptr(S), _lib.ptr(N), res, res, res, w0, ops._hptr(s_host), ops._hptr(tr), _lib.ptr(f), R,
                      _lib.ptr(S2), _lib.ptr(N2), _lib.ptr(cnt), _lib.ptr(ws), ws.numel(), st)

        fns = [k_rows, lambda: torch_rows(N, od, hd, w0), k_vote, lambda: torch_vote(S, N, f, inst, index, sd, td, w0),
               lambda: ops.tsdf_prior_rows_batch((S, N), origin=o, voxel=h, weight=w0, packed=True),
               lambda: hip.sdf_decode_rows(points, inst, code["z_so3"], code["z_inv"], code["s"].float().contiguous(), code["t"]),
               lambda: solver._complete_fusion_batch(fusion, code, weight=w0)]
        (t_r, t_tr, t_v, t_tv, t_ops, t_dec, t_all), spread = median_ms(fns, a.reps)
        c = vcounts.cpu().numpy().sum(0)
        print(f"weight {w0}: rows {R} of {voxels} samples; eligible {c[0]}, voted {c[1]}, skipped {c[2]}, untouched {c[3]}")
        names = ("rows", "torch rows", "vote", "torch vote", "rows (ops)", "decoder", "complete")
        for name, tm, (lo, hi) in zip(names, (t_r, t_tr, t_v, t_tv, t_ops, t_dec, t_all), spread):
            print(f"  {name:10s} {tm:9.3f} ms (min {lo:.3f}, max {hi:.3f})")
        m_rows, m_vote = 4 * voxels + 20 * R, 16 * voxels + 4 * R
        print(f"  rows: must-move {m_rows / 2 ** 20:.0f} MiB = {m_rows / (t_r * 1e-3) / 1e9:.0f} GB/s ({100 * m_rows / (t_r * 1e-3) / PEAK:.1f} % of 8.0 TB/s); "
              f"torch / rows = {t_tr / t_r:.2f}")
        print(f"  vote: must-move {m_vote / 2 ** 20:.0f} MiB = {m_vote / (t_v * 1e-3) / 1e9:.0f} GB/s ({100 * m_vote / (t_v * 1e-3) / PEAK:.1f} % of 8.0 TB/s); "
              f"torch / vote = {t_tv / t_v:.2f}; rows + vote: torch / kernels = {(t_tr + t_tv) / (t_r + t_v):.2f}")
        print(f"  decoder: {R / (t_dec * 1e-3) / 1e6:.1f} M queries/s, {100 * t_dec / t_all:.1f} % of _complete_fusion_batch")


if __name__ == "__main__":
    main()
