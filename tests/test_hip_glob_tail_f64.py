"""The residual global conv (HipModel.vn_lna_global: glob_mean_gemv_kernel + one of the three VN GEMMs, or mean_points_kernel + GEMM + latency GEMM
+ vn_act_rows_kernel) and the encoder tail (HipModel.encoder_tail: conv_c, which may split K, + tail_kernel with its tail_gemv3) against the
float64 oracles tests/glob_tail_oracle.py at their size edges: N = 1 and N on both sides of the mean kernels' 16 row slices and of the 40-point
tile, the plan thresholds at 64 channels, Co = 32 / 96 where no fused kernel exists; c_dim % 4 != 0, c_dim > 256, dynamic LDS above 64 KB,
NP = 1 / 2 / 257, every center flag, B = 1.  The cases, their inputs and the rule are tests/tools/glob_tail_vs_float64.py: PER POINT for the global
conv, PER INSTANCE and per output for the tail (a wrong small point, or a wrong last instance, cannot hide behind a large one),
    err <= min(16 x e32, 1e-4),
e32 the same error of the float32 oracle, computed here on the CPU from the same inputs; e32 < 1e-5 is asserted as a precondition.
tests/test_glob_tail_oracle_cpu.py shows which kernels the ladder reaches.  With the comparison go the exact relations the code promises:
LS_OPT_GLOB_FUSE = 2 equals 1 bit for bit, and the encode epilogue changes nothing but s = scale0 * s and t = t + centroid."""
import importlib.util
import os
import subprocess
import sys

import pytest
import torch

from livingscenes_amd import synth

pytestmark = pytest.mark.gpu
TOOL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools", "glob_tail_vs_float64.py")


def _load():
    spec = importlib.util.spec_from_file_location("glob_tail_vs_float64", TOOL)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


lad = _load()   # one module object: the float64 references it caches serve every test of this file


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    return lad.compile_plan_dump(tmp_path_factory.mktemp("gemm_plan"))


# ------------------------------------------------------------------------------------------------ the ladders, in this process's mode
@pytest.mark.parametrize("model,layer", lad.GC_MODELS, ids=[f"{m}-{i}" for m, i in lad.GC_MODELS])
def test_global_conv_vs_float64_per_point(model, layer, plan_exe):
    """Every shape x LS_OPT_GLOB_FUSE x kind of one (model, layer): a few dozen tiny launches.  Prints the largest err / e32 per kernel chain.
    Then, on the same outputs: LS_OPT_GLOB_FUSE = 2 (exact row maxima handed over; the streaming kernel where it applies) gives the bits of 1,
    as the header states at the option."""
    cases = [c for c in lad.gc_ladder() if (c[1], c[2]) == (model, layer)]
    outs = {}
    table, bad = lad.check_cases("gc", cases, lad.own_mode(), _dev(), plan_exe, outs=outs)
    print(f"[{model} layer {layer}, mode {lad.own_mode()}] largest err / e32 per kernel chain\n{lad.format_table(table)}")
    for key, _, _, (B, _), gf in cases:
        if gf == 1:
            for kind in lad.kinds_of(B):
                if not torch.equal(outs[(key, kind)], outs[(key.replace("glob_fuse=1", "glob_fuse=2"), kind)]):
                    bad.append(f"{key} {kind}: glob_fuse = 2 differs from glob_fuse = 1 in "
                               f"{int((outs[(key, kind)] != outs[(key.replace('glob_fuse=1', 'glob_fuse=2'), kind)]).sum())} floats")
    assert not bad, f"{len(bad)} failures:\n" + "\n".join(bad[:20])


TAIL_CFGS = [t[0] for t in lad.tail_cfgs()]


@pytest.mark.parametrize("name", TAIL_CFGS)
def test_tail_vs_float64_per_instance(name, plan_exe):
    """Every (B, NP) x epilogue x kind of one configuration.  Then, on the same outputs: encoder_tail(f, centroid, scale0) returns the z_so3 and
    z_inv bits of encoder_tail(f), s = scale0 * s_plain and t = t_plain + centroid evaluated in float32 (the kernel forms exactly these)."""
    cases = [c for c in lad.tail_ladder() if c[1] == name]
    outs = {}
    table, bad = lad.check_cases("tail", cases, lad.own_mode(), _dev(), plan_exe, outs=outs)
    print(f"[{name}, mode {lad.own_mode()}] largest err / e32 per kernel chain\n{lad.format_table(table)}")
    for case in cases:
        if not case[3]:
            continue
        for kind in lad.kinds_of(case[2][0]):
            z_so3, z_inv, s, t = outs[(case[0], kind)]
            p_so3, p_inv, p_s, p_t = outs[(case[0].replace("epilogue=1", "epilogue=0"), kind)]
            _, centroid, scale0 = lad.tail_inputs(case, kind)
            for what, ok in (("z_so3", torch.equal(z_so3, p_so3)), ("z_inv", torch.equal(z_inv, p_inv)), ("s == scale0 * s_plain", torch.equal(s, scale0 * p_s)),
                             ("t == t_plain + centroid", torch.equal(t, p_t + centroid))):
                if not ok:
                    bad.append(f"{case[0]} {kind}: {what} does not hold bit for bit against the call without the epilogue")
    assert not bad, f"{len(bad)} failures:\n" + "\n".join(bad[:20])


# ------------------------------------------------------------------------------------------------ the other arithmetic modes
def test_glob_tail_vs_float64_in_the_other_arithmetic_modes(tmp_path):
    """LS_GEMM_MODE is read once per process: the two tests above hold the ladders in this process's mode; here bf16x3 / fp32 (or the default)
    once each in a fresh child under a time limit (tests/tools/glob_tail_vs_float64.py --check MODE; the float64 references, computed here on
    the CPU where the tests above have not left them, are handed over in a file).  A child that dies of a signal or runs out of time fails the
    test, and no further child is started."""
    mine = lad.own_mode()
    worst = lad.all_references()
    print(f"largest e32 of the ladders: global conv {worst[0]:.3e}, tail {worst[1]:.3e}")
    refs = str(tmp_path / "refs.pt")
    lad.save_references(refs)
    for mode in lad.MODES:
        if mode == mine:
            continue
        env = dict(os.environ)
        env.pop("LS_GEMM_MODE", None)
        if mode != lad.MODES[0]:
            env["LS_GEMM_MODE"] = mode
        try:
            p = subprocess.run([sys.executable, TOOL, "--check", mode, "--refs", refs], env=env, capture_output=True, text=True, timeout=240)
        except subprocess.TimeoutExpired as e:
            pytest.fail(f"mode {mode}: the child ran out of time; no further child started\n{(e.stdout or b'')[-2000:]}")
        print(p.stdout[-12000:])
        assert p.returncode >= 0, f"mode {mode}: the child died of signal {-p.returncode}; no further child started\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}"
        assert p.returncode == 0, (mode, p.stdout[-4000:], p.stderr[-2000:])


# ------------------------------------------------------------------------------------------------ the refusal
@pytest.mark.parametrize("c_dim", [1026, 33])
def test_an_unsupported_c_dim_is_refused_before_anything_is_enqueued(c_dim):
    """tail_kernel serves an even c_dim <= 1024.  The export returns tail_launch's error for anything else -- and has enqueued nothing by then:
    not conv_c either, whose output would land in the workspace.  Outputs and workspace, filled with a pattern, are untouched after the call."""
    from livingscenes_amd import _lib, ops, packing
    dev = _dev()
    cfg = synth.small_encoder_cfg()
    cfg["c_dim"] = c_dim
    desc, blob = packing.pack_model(synth.make_encoder_weights(cfg, 0), cfg, None, None)
    m = ops.HipModel(desc, blob, dev)
    try:
        B, NP = 2, 5
        f = torch.randn(B, NP, 3, cfg["feat_dim"][-1], generator=torch.Generator().manual_seed(c_dim)).to(dev)
        outs = [torch.full(s, 7.0, dtype=torch.float32, device=dev) for s in ((B, c_dim, 3), (B, c_dim), (B,), (B, 3))]
        lib = _lib.load()
        need = lib.ls_encoder_tail_workspace_bytes(m._h, B, NP)
        assert need > 0
        ws = torch.full((need,), 0x5A, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            rc = lib.ls_encoder_tail_f32(m._h, ops.ptr(f), None, None, B, NP, *[ops.ptr(o) for o in outs], ops.ptr(ws), ws.numel(), ops.stream_ptr(dev))
        msg = lib.ls_last_error().decode()
        torch.cuda.synchronize()
        assert rc == -1 and msg == f"tail: c_dim={c_dim} unsupported (even, <= 1024)", (rc, msg)      # LS_ERR_INVALID
        assert bool((ws == 0x5A).all()), f"{int((ws != 0x5A).sum())} workspace bytes were written by a refused call"
        assert all(bool((o == 7.0).all()) for o in outs)
        with pytest.raises(_lib.LsError, match="unsupported"):
            m.encoder_tail(f)
    finally:
        m.close()
