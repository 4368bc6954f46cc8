"""GPU tests of decoder_type "deepsdf" (the invariant-decoder ablation, model_utils.py:247-250): the raw query after z_inv, a
512-wide DeepSDF MLP.  Against tests/golden/inv_deepsdf.npz (the reference's own Shape_Prior, make_golden_inv_deepsdf.py) at the
project's 1e-4-of-max-norm bar, and against CPU fp64 restatements where a trajectory is compared."""
import os

import numpy as np
import pytest
import torch
import yaml

import sdf_oracle
from livingscenes_amd import _lib, synth

pytestmark = pytest.mark.gpu
TOL = 1e-4
HERE = os.path.dirname(os.path.abspath(__file__))
CONFIGS = {"full": (synth.default_encoder_cfg, synth.inv_decoder_cfg), "small": (synth.small_encoder_cfg, synth.small_inv_decoder_cfg)}


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def relerr(a, b):
    a, b = ((v.detach().cpu() if torch.is_tensor(v) else torch.as_tensor(v)).double() for v in (a, b))
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(HERE, "golden", "inv_deepsdf.npz"))
    return {k: g[k] for k in g.files}


def _fixture(g, tag):
    return {k[len(tag) + 1:]: v for k, v in g.items() if k.startswith(tag + "_")}


def _prior(tag, seed=0, n_pcl=1024):
    from livingscenes_amd.model_utils import Shape_Prior
    ecfg, dcfg = CONFIGS[tag][0](), CONFIGS[tag][1]()
    ew, dw = synth.make_encoder_weights(ecfg, seed), synth.make_decoder_weights(dcfg, seed)
    sp = Shape_Prior.from_state(ecfg, dcfg, ew, dw, device=_dev(), n_pcl=n_pcl, decoder_type="deepsdf")
    return sp, (ecfg, dcfg, ew, dw)


@pytest.fixture(scope="module")
def small_inv():
    return _prior("small", seed=4, n_pcl=128)


def _codes(f, requires_grad=False):
    return {k: torch.from_numpy(f[k]).to(_dev()).requires_grad_(requires_grad) for k in ("z_so3", "z_inv", "s", "t")}


def _mlp64(dw, dcfg, query, z_inv):
    """deepsdf_decoder.py:78-123 with model_utils.py:247-250's input in fp64 on the CPU (weight norm folded in fp64), autograd enabled: the
    'xyz' kind of tests/sdf_oracle.py"""
    return sdf_oracle.field_with_grad(dw, dcfg, query, {"z_inv": z_inv}, torch.float64, "xyz")


# ------------------------------------------------------------------------------------------------ loader + forward vs the reference
@pytest.mark.parametrize("tag", ["full", "small"])
def test_load_ckpt_from_log_vs_reference_fixture(golden, tag, tmp_path, monkeypatch):
    """load_ckpt_from_log on a log dir whose yaml says decoder_type "deepsdf" -> encode -> FieldWrapper (sdf and Bernoulli logits)."""
    from livingscenes_amd.model_utils import load_ckpt_from_log
    f = _fixture(golden, tag)
    ecfg, dcfg = CONFIGS[tag][0](), CONFIGS[tag][1]()
    ew, dw = synth.make_encoder_weights(ecfg, 0), synth.make_decoder_weights(dcfg, 0)
    log = tmp_path / "log" / "inv_deepsdf"
    (log / "checkpoint").mkdir(parents=True)
    (log / "files_backup").mkdir()
    torch.save(synth.to_checkpoint(ew, dw, epoch=2), log / "checkpoint" / "inv_latest.pt")
    field = {"model": {"model_name": "sim3sdf_vanilla", "encoder_type": "vecdgcnn_atten", "decoder_type": "deepsdf", "encoder": ecfg,
                       "decoder": dcfg, "sdf2occ_factor": -1.0}, "dataset": {"n_pcl": 1024}}
    (log / "files_backup" / "dgcnn_attn_inv_deepsdf.yaml").write_text(yaml.safe_dump(field))
    (tmp_path / "configs").mkdir()
    (tmp_path / "configs" / "room4cates.yaml").write_text(yaml.safe_dump(
        {"shape_priors": {"chair": {"field_pt": "./x.pt", "field_cfg": "./x.yaml"}}, "solver_global": {"use_double": False}}))
    monkeypatch.chdir(tmp_path)
    sp = load_ckpt_from_log(str(log))["chair"]
    assert sp.decoder_type == "deepsdf" and sp.decoder.decoder_type == "deepsdf"
    assert sp.hip_model().desc.dec_input == _lib.DEC_XYZ
    q = torch.from_numpy(f["query"]).to(_dev())
    with torch.no_grad():
        emb = sp.encode(synth.make_instances(2, 1024, seed=0).to(_dev()))
        for k in ("z_so3", "z_inv", "s", "t"):
            assert relerr(emb[k], f[k]) < TOL, k
        sdf = sp.decoder(q, None, _codes(f), return_sdf=True)          # the reference's own codes
        assert relerr(sdf, f["sdf"]) < TOL
        assert relerr(sp.decoder(q, None, emb, return_sdf=True), f["sdf"]) < TOL   # end to end on this model's codes
        assert relerr(sp.decoder(q, None, _codes(f)).logits, -f["sdf"]) < TOL
    assert float(np.abs(f["sdf"]).max()) > 0


def test_field_wrapper_gradients_vs_reference_fixture(golden):
    """Autograd through FieldWrapper: d sum(w sdf) / d query and / d z_inv as the reference's autograd; z_so3, s, t get None."""
    f = _fixture(golden, "full")
    sp, _ = _prior("full")
    code = _codes(f, requires_grad=True)
    q = torch.from_numpy(f["query"]).to(_dev()).requires_grad_(True)
    w = torch.from_numpy(f["w"]).to(_dev())
    (w * sp.decoder(q, None, code, return_sdf=True)).sum().backward()
    assert relerr(q.grad, f["g_query"]) < TOL
    assert relerr(code["z_inv"].grad, f["g_z_inv"]) < TOL
    assert f["none_grads"].all()
    for k in ("z_so3", "s", "t"):
        assert code[k].grad is None, k


def test_sdf_backward_writes_zeros_for_the_unused_inputs(small_inv):
    """ls_sdf_backward called directly: grad_z_so3 / grad_s / grad_t, pre-filled with NaN, come back exact zeros; the query and
    code gradients agree with the fp64 restatement."""
    from livingscenes_amd._lib import call, ptr, stream_ptr
    sp, (_, dcfg, _, dw) = small_inv
    hip = sp.hip_model()
    dev = _dev()
    B, M = 2, 96
    code = sp.encode(synth.make_instances(B, 128, seed=5).to(dev))
    q = (synth.make_queries(B, M, seed=5).to(dev) * code["s"][:, None, None] + code["t"]).contiguous()
    z_so3, z_inv, s, t = (code[k].float().contiguous() for k in ("z_so3", "z_inv", "s", "t"))
    t = t.reshape(B, 3).contiguous()
    sdf, saved = hip.sdf_decode_train(q, z_so3, z_inv, s, t)
    ws = saved[-1]
    g = torch.linspace(-1.0, 1.0, B * M, device=dev).reshape(B, M).contiguous()
    gq = torch.full((B, M, 3), float("nan"), device=dev)
    gso3, ginv = torch.full_like(z_so3, float("nan")), torch.full_like(z_inv, float("nan"))
    gs, gt = torch.full_like(s, float("nan")), torch.full_like(t, float("nan"))
    call(dev, "ls_sdf_backward", hip._h, ptr(q), ptr(z_so3), ptr(z_inv), ptr(s), ptr(t), B, M, ptr(sdf), ptr(g), ptr(ws), ws.numel(),
         ptr(gq), ptr(gso3), ptr(ginv), ptr(gs), ptr(gt), stream_ptr(dev))
    torch.cuda.synchronize()
    for name, v in (("z_so3", gso3), ("s", gs), ("t", gt)):
        assert torch.equal(v, torch.zeros_like(v)), name
    # the inputs the invariant decoder ignores may be NULL
    gq2, ginv2 = torch.empty_like(gq), torch.empty_like(ginv)
    call(dev, "ls_sdf_backward", hip._h, ptr(q), None, ptr(z_inv), None, None, B, M, ptr(sdf), ptr(g), ptr(ws), ws.numel(),
         ptr(gq2), None, ptr(ginv2), None, None, stream_ptr(dev))
    assert torch.equal(gq2, gq) and torch.equal(ginv2, ginv)
    qd = q.detach().cpu().double().requires_grad_(True)
    zd = z_inv.detach().cpu().double().requires_grad_(True)
    (g.cpu().double() * _mlp64(dw, dcfg, qd, zd)).sum().backward()
    assert relerr(sdf, _mlp64(dw, dcfg, qd.detach(), zd.detach())) < TOL
    assert relerr(gq, qd.grad) < TOL and relerr(ginv, zd.grad) < TOL


# ------------------------------------------------------------------------------------------------ call-size invariance
@pytest.mark.parametrize("tag", ["full", "small"])
def test_decode_is_bit_identical_across_call_shapes(tag):
    """One instance alone == its rows in a batched call == the ragged rows path, bit for bit; z_so3 / s / t do not enter."""
    sp, _ = _prior(tag, seed=1)
    hip = sp.hip_model()
    dev = _dev()
    B, M = 3, 700
    code = sp.encode(synth.make_instances(B, 1024, seed=6).to(dev))
    q = (synth.make_queries(B, M, seed=6).to(dev) * code["s"][:, None, None] + code["t"]).contiguous()
    with torch.no_grad():
        full = hip.sdf_decode(q, code["z_so3"], code["z_inv"], code["s"], code["t"])
        for b in range(B):
            one = hip.sdf_decode(q[b:b + 1].contiguous(), code["z_so3"][b:b + 1], code["z_inv"][b:b + 1], code["s"][b:b + 1], code["t"][b:b + 1])
            assert torch.equal(one[0], full[b]), b
            part = hip.sdf_decode(q[b:b + 1, :37].contiguous(), code["z_so3"][b:b + 1], code["z_inv"][b:b + 1], code["s"][b:b + 1],
                                  code["t"][b:b + 1])
            assert torch.equal(part[0], full[b, :37]), b
        ri = torch.arange(B, device=dev, dtype=torch.int32).repeat_interleave(M)
        rows = hip.sdf_decode_rows(q.reshape(-1, 3), ri, code["z_so3"], code["z_inv"], code["s"], code["t"])
        assert torch.equal(rows.reshape(B, M), full)
        other = hip.sdf_decode(q, torch.randn_like(code["z_so3"]), code["z_inv"], code["s"] * 3.0, code["t"] + 1.0)
        assert torch.equal(other, full)


def test_deepsdf_decoder_forward_matches_field_wrapper(golden):
    """DeepSDF_Decoder.forward on the assembled [z_inv | query] input (259 wide) == FieldWrapper's fused path, within the bar."""
    f = _fixture(golden, "full")
    sp, _ = _prior("full")
    q = torch.from_numpy(f["query"]).to(_dev())
    z_inv = torch.from_numpy(f["z_inv"]).to(_dev())
    inp = torch.cat([z_inv[:, None, :].expand(-1, q.shape[1], -1), q], -1)
    assert inp.shape[-1] == 259
    with torch.no_grad():
        direct = sp.decoder.F(inp, "val")
        fused = sp.decoder(q, None, _codes(f), return_sdf=True)
    assert relerr(direct, fused) < TOL and relerr(direct, f["sdf"]) < TOL


# ------------------------------------------------------------------------------------------------ meshing and code optimisation
def test_generator3d_on_a_deepsdf_prior_vs_oracle_chain(small_inv):
    """Generator3D.generate_from_latent (device MISE, ragged decode, device marching cubes) == the oracle MISE + marching cubes
    driven by the same device decoder: identical value grid, vertices and faces."""
    from livingscenes_amd.mesh_extractor2 import Generator3D
    from oracle import mcubes as omc
    from oracle import mise as om
    sp, _ = small_inv
    code = sp.encode(synth.make_instances(1, 128, seed=22).to(_dev()))
    code["t"], code["s"] = torch.zeros_like(code["t"]), torch.ones_like(code["s"])   # canonical frame (model_utils.py:293-305)
    res0, steps = 16, 2
    gen = Generator3D(threshold=0.5, resolution0=res0, upsampling_steps=steps, padding=0.1)
    level = float(np.median(gen.eval_grid(code, sp.decoder)))   # the synthetic field has no zero level set: cut it at its median
    gen.threshold = 1.0 / (1.0 + np.exp(-level))
    thr = np.log(gen.threshold) - np.log(1.0 - gen.threshold)

    def field(pf):
        with torch.no_grad():
            return sp.decoder(torch.from_numpy(pf).to(_dev())[None], None, code).logits[0].cpu().numpy()
    ref = om.run(field, res0, steps, threshold=thr, box_size=1.1)
    assert np.array_equal(gen.eval_grid(code, sp.decoder), ref)
    mesh = gen.generate_from_latent(code, sp.decoder)
    v, fc = omc.marching_cubes(np.pad(ref, 1, "constant", constant_values=-1e6), thr)
    n = np.array(ref.shape) - 1
    v = 1.1 * ((v - 0.5 - 1) / n - 0.5)
    assert len(fc) > 100
    assert np.array_equal(np.asarray(mesh.vertices), v) and np.array_equal(np.asarray(mesh.faces), fc)


def test_optimize_code_vs_fp64_adam_and_pose_untouched(small_inv):
    """More_Solver._optimize_code, 20 steps: z_inv follows torch.optim.Adam / MultiStepLR on the fp64 restatement of the MLP; t and
    z_so3 come back bit-identical (the reference's Adam never moves a parameter whose .grad is None)."""
    from livingscenes_amd.lib_more.more_solver import More_Solver
    from livingscenes_amd.model_utils import fps
    sp, (_, dcfg, _, dw) = small_inv
    dev = _dev()
    x = synth.make_instances(1, 128, seed=31)
    code = sp.encode(x.to(dev))
    pc = x[0].to(dev)
    mask = torch.ones(1, 128, dtype=torch.bool, device=dev)
    solver = More_Solver({"shape_priors": {"n_input_point": 128}}, model=sp)
    start = {k: v.detach().clone() for k, v in code.items()}
    steps = 20
    best = solver._optimize_code({k: v.detach().clone() for k, v in code.items()}, pc, mask, n_steps=steps)
    assert best is not None
    for k in ("t", "z_so3", "s"):
        assert torch.equal(best[k], start[k]), k
    pts, _ = fps(pc.T[None], K=128)
    z = start["z_inv"].cpu().double().clone().requires_grad_(True)
    opt = torch.optim.Adam([{"params": z, "lr": 1e-5}])
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[160], gamma=0.1)
    for _ in range(steps):
        opt.zero_grad()
        sdf = _mlp64(dw, dcfg, pts.cpu().double(), z)
        torch.nn.functional.mse_loss(sdf, torch.zeros_like(sdf)).backward()
        opt.step()
        sched.step()
    moved = float((z.detach() - start["z_inv"].cpu().double()).abs().max())
    assert moved > 0
    assert float((best["z_inv"].cpu().double() - z.detach()).abs().max()) < 2e-3 * moved + 1e-7
