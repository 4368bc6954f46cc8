"""tests/glob_tail_oracle.py, the float64 yardstick of the residual global conv and of the encoder tail, pinned to oracle.net: in float32, on
the tensors of net.encoder_forward's own trace, `global_conv` must give trace["dst_f_i"] from trace["msg_f_i"] and `tail` the four outputs of
net.encoder_forward BIT FOR BIT, on the small and the released configuration.  Then the ladder of tests/tools/glob_tail_vs_float64.py where no
GPU is needed to see it: every input is well conditioned, a zero instance gives exactly zero, and the plan (csrc/gemm_plan.h, compiled on its
own) launches for the cases what the ladder was built to reach.  No GPU needed."""
import importlib.util
import os

import pytest
import torch

import glob_tail_oracle as gto
from livingscenes_amd import synth
from oracle import net


def _ladder():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools", "glob_tail_vs_float64.py")
    spec = importlib.util.spec_from_file_location("glob_tail_vs_float64", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


lad = _ladder()


@pytest.mark.parametrize("which,N", [("small", 128), ("released", 1024)])
def test_oracles_reproduce_encoder_forward_bit_for_bit(which, N):
    cfg = synth.small_encoder_cfg() if which == "small" else synth.default_encoder_cfg()
    w = synth.make_encoder_weights(cfg, 0)
    x = synth.make_instances(2, N, seed=11, rigid=False)
    x = (x - x.mean(-1, keepdim=True)) / 1.2
    tr = {}
    center, scale, z_so3, z_inv = net.encoder_forward(w, cfg, x, trace=tr)
    L = cfg["num_layers"]
    for i in range(cfg["res_global_start_layer"], L):
        out = gto.global_conv(w, cfg, i, tr[f"msg_f_{i}"], torch.float32)
        assert out.dtype == torch.float32 and torch.equal(out, tr[f"dst_f_{i}"]), f"layer {i}"
        # ... and the float64 form is the same function: it differs from the float32 one by fp32 round-off, per point
        ref = gto.global_conv(w, cfg, i, tr[f"msg_f_{i}"], torch.float64)
        assert ref.dtype == torch.float64 and gto.per_point_err(out, ref) < 1e-5, f"layer {i}"
    got = gto.tail(w, cfg, tr[f"dst_f_{L - 1}"], torch.float32)
    for name, a, b in zip(gto.TAIL_NAMES, got, (z_so3, z_inv, scale, center)):
        assert a.dtype == torch.float32 and torch.equal(a, b), name
    ref = gto.tail(w, cfg, tr[f"dst_f_{L - 1}"], torch.float64)
    assert all(r.dtype == torch.float64 for r in ref) and gto.per_instance_err(got, ref) < 1e-5


def test_tail_follows_the_center_flags():
    """center_pred_scale multiplies the center by scale_factor; without center_pred the reference returns no center (the library: t = its
    centroid argument), whatever center_pred_scale says -- and the other three outputs do not notice either flag"""
    cfg = synth.small_encoder_cfg()
    w = synth.make_encoder_weights(cfg, 0)
    f = torch.randn(2, cfg["feat_dim"][-1], 3, 5, generator=torch.Generator().manual_seed(3))
    full = gto.tail(w, cfg, f, torch.float64)
    plain = gto.tail(w, dict(cfg, center_pred_scale=False), f, torch.float64)
    none = gto.tail({k: v for k, v in w.items() if not k.startswith("fc_center.")}, dict(cfg, center_pred=False), f, torch.float64)
    assert torch.equal(full[3], plain[3] * cfg["scale_factor"]) and (plain[3] != 0).all()
    assert none[3].shape == full[3].shape and (none[3] == 0).all()
    for k in range(3):
        assert torch.equal(full[k], plain[k]) and torch.equal(full[k], none[k])


def test_per_instance_err_does_not_let_an_instance_or_an_output_hide():
    ref = (torch.ones(3, 4, 3, dtype=torch.float64), torch.ones(3, 4, dtype=torch.float64), torch.ones(3, dtype=torch.float64),
           torch.ones(3, 3, dtype=torch.float64))
    ref[0][2] *= 1e6                              # a large last instance
    ref[1][1] = 0                                 # an all-zero z_inv of instance 1
    a = tuple(r.clone() for r in ref)
    assert gto.per_instance_err(a, ref) == 0.0
    a[0][0, 3, 2] += 1e-3                         # 1e-9 of the tensor's max-norm, 1e-3 of the instance's
    assert abs(gto.per_instance_err(a, ref) - 1e-3) < 1e-12
    a[3][1, 0] += 1e-2                            # ... and t of another instance is judged on its own
    errs = gto.per_instance_errs(a, ref)
    assert abs(errs["t"] - 1e-2) < 1e-12 and abs(errs["z_so3"] - 1e-3) < 1e-12 and errs["z_inv"] == 0.0 and errs["s"] == 0.0
    a[1][1, 2] = 1e-30                            # a zero instance has to stay zero
    assert gto.per_instance_err(a, ref) == float("inf")


def test_every_ladder_input_is_well_conditioned():
    """The precondition of tests/test_hip_glob_tail_f64.py: on every case and kind of both ladders the float32 oracle is within E32_MAX = 1e-5
    of the float64 one (per point / per instance), so that min(MARGIN x e32, TOL) is a bound an fp32 implementation can meet and that means
    something; an all-zero instance gives finite references that are exactly zero while the other two instances do not vanish."""
    for family, cases, reference in (("global conv", lad.gc_ladder(), lad.gc_reference), ("tail", lad.tail_ladder(), lad.tail_reference)):
        worst, where = 0.0, None
        for case in cases:
            for kind in lad.kinds_of(case[-2][0]):
                ref, e32 = reference(case, kind)
                refs = ref if isinstance(ref, tuple) else (ref,)
                assert all(torch.isfinite(r).all() for r in refs), (case[0], kind)
                assert 0 < e32 < lad.E32_MAX, (case[0], kind, e32)
                if kind == "zero":
                    # (t: all zero without center_pred; with the epilogue the zero instance's t is its centroid)
                    for name, r in zip(gto.TAIL_NAMES if family == "tail" else ("out",), refs):
                        assert name == "t" or ((r[0] != 0).any() and (r[2] != 0).any()), (case[0], name)
                        assert (r[1] == 0).all() or (name == "t" and case[3]), (case[0], name)
                if e32 > worst:
                    worst, where = e32, f"{case[0]} {kind}"
        print(f"largest e32 of the {family} ladder: {worst:.3e} ({where})")


# ------------------------------------------------------------------------------------------------ what the plan launches for the ladder
@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    return lad.compile_plan_dump(tmp_path_factory.mktemp("gemm_plan"))


VN_KERNELS = {"ls::gemm_vn_direct_kernel<64, true>", "ls::gemm_vn_smallk_kernel<64>", "ls::gemm_vn_kernel<true>"}
REDUCE, LATENCY = "ls::gemm_splitk_reduce_kernel", "ls::gemm_f32_kernel<false, 3>"


def _gemms(chain):
    return [n for n in chain if n.startswith("ls::gemm_")]


def test_the_ladder_reaches_the_kernels_it_was_built_for(dump):
    """Default mode.  The enumerators of gemm_vn_plan these exports cannot reach, and why:
      VN_ANYK       (gemm_vn_kernel<false>) needs K % 32 != 0, but global_conv sets K = C and the plan wants C % 64 == 0;
      VN_SMALLK32   needs K = 32 with C % 64 == 0 -- the same contradiction (Co = 32 gives NONE: the unfused path);
      VN_DIRECT     (several parts) needs a_parts > 1: row maxima in parts come only from a producer kernel inside ls_encode; the export computes
                    exact maxima in one part (LS_OPT_GLOB_FUSE = 2)."""
    mode = lad.MODES[0]
    gc = lad.gc_ladder()
    chains = dict(zip((c[0] for c in gc), lad.gc_planned(gc, mode, dump)))
    fused = {k: v for k, v in chains.items() if v[0] == "ls::glob_mean_gemv_kernel"}
    assert {v[1] for v in fused.values()} == VN_KERNELS
    # the thresholds, case by case: tm = 15 | 16, M = 1536, N % 8, glob_fuse 1 | 2
    want = {("released", 2, 1, 600, 1): "ls::gemm_vn_kernel<true>", ("released", 2, 1, 600, 2): "ls::gemm_vn_direct_kernel<64, true>",
            ("released", 2, 1, 601, 1): "ls::gemm_vn_smallk_kernel<64>", ("released", 2, 1, 601, 2): "ls::gemm_vn_smallk_kernel<64>",
            ("released", 2, 1, 608, 1): "ls::gemm_vn_smallk_kernel<64>", ("released", 2, 1, 608, 2): "ls::gemm_vn_direct_kernel<64, true>",
            ("released", 3, 2, 256, 1): "ls::gemm_vn_kernel<true>", ("released", 3, 2, 256, 2): "ls::gemm_vn_direct_kernel<64, true>",
            ("released", 3, 1, 504, 1): "ls::gemm_vn_kernel<true>", ("released", 3, 1, 504, 2): "ls::gemm_vn_kernel<true>",
            ("released", 6, 3, 41, 2): "ls::gemm_vn_kernel<true>", ("released", 4, 1, 1, 1): "ls::gemm_vn_kernel<true>"}
    for (model, i, B, N, gf), kernel in want.items():
        assert chains[f"global_conv({model}, layer={i}, B={B}, N={N}, glob_fuse={gf})"] == ["ls::glob_mean_gemv_kernel", kernel], (model, i, B, N, gf)
    # NONE: Co = 32 / 96 run the unfused path under every option; the other widths with LS_OPT_GLOB_FUSE = 0 only
    unfused = {k: v for k, v in chains.items() if k not in fused}
    for key, model, i, (B, N), gf in gc:
        assert (key in unfused) == (gf == 0 or model != "released"), key
    assert all(v[0] == "ls::mean_points_kernel" and v[-1] == "ls::vn_act_rows_kernel" for v in unfused.values())
    # the latency kernel on the 3B mean rows, M = 3 and M = 9, alone (K = 32, 64, 96) and as a split launch with its reduce (K >= 128)
    for model, i, split in (("small", 2, False), ("attn96", 2, False), ("released", 2, False), ("released", 4, True), ("released", 6, True)):
        for B, N in ((1, 1), (3, 7)):
            g = _gemms(chains[f"global_conv({model}, layer={i}, B={B}, N={N}, glob_fuse=0)"])
            assert g[-2:] == [LATENCY, REDUCE] if split else (g[-1] == LATENCY and REDUCE not in g), (model, i, B, N, g)
    # the per-point GEMM: the tiled kernels at K = 32, 64 and 96; split along K from 128 channels on, with W planes at 512
    first = lambda model, i, B, N: _gemms(chains[f"global_conv({model}, layer={i}, B={B}, N={N}, glob_fuse=0)"])[:-1 - int(model == "released" and i >= 4)]
    assert first("small", 2, 3, 41) == ["ls::gemm_f32_kernel<true, 22>"] and first("released", 3, 1, 608) == ["ls::gemm_f32_kernel<true, 22>"]
    assert first("attn96", 2, 3, 41) == ["ls::gemm_h2_kernel<true, false>"] and first("attn96", 2, 1, 1) == ["ls::gemm_h2_kernel<true, false>"]
    assert first("released", 4, 3, 40) == ["ls::gemm_h2_kernel<true, false>", REDUCE]
    assert first("released", 6, 3, 39) == ["ls::gemm_h2_kernel<true, true>", REDUCE]
    # the tail: conv_c splits K at the released width (with W planes); at 64 channels it is the tiled kernel, the persistent one from 16 M-tiles on
    tl = lad.tail_ladder()
    tchains = dict(zip((c[0] for c in tl), lad.tail_planned(tl, mode, dump)))
    for key, name, (B, NP), epi in tl:
        Cl = lad.tail_cfg(name)["feat_dim"][-1]
        k64 = "ls::gemm_h2_smallk_kernel<64, false>" if 3 * B * NP > 15 * 128 else "ls::gemm_f32_kernel<true, 22>"
        assert tchains[key] == (["ls::gemm_h2_kernel<true, true>", REDUCE] if Cl == 512 else [k64]) + ["ls::tail_kernel"], key
    assert {"ls::gemm_h2_smallk_kernel<64, false>", "ls::gemm_f32_kernel<true, 22>", REDUCE} <= {n for v in tchains.values() for n in v}


@pytest.mark.parametrize("mode,kernel", [("bf16x3", "ls::gemm_f32_kernel<true, 3>"), ("fp32", "ls::gemm_f32_kernel<false, 3>")])
def test_the_other_modes_run_the_unfused_path(dump, mode, kernel):
    """the fused kernels exist for the default mode only: every case is mean + GEMM (+ reduce) + latency GEMM (+ reduce) + activation on the
    mode's own tiled kernel, the latency kernel being the exact one in every mode"""
    gc = lad.gc_ladder()
    for case, chain in zip(gc, lad.gc_planned(gc, mode, dump)):
        assert chain[0] == "ls::mean_points_kernel" and chain[-1] == "ls::vn_act_rows_kernel", case[0]
        assert set(_gemms(chain)) <= {kernel, LATENCY, REDUCE} and _gemms(chain)[0] == kernel, (case[0], chain)
    tl = lad.tail_ladder()
    for case, chain in zip(tl, lad.tail_planned(tl, mode, dump)):
        assert chain[0] == kernel and chain[-1] == "ls::tail_kernel" and set(chain[1:-1]) <= {REDUCE}, (case[0], chain)
