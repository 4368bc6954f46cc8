"""Every edge-conv kernel form (csrc/edge_plan.h: the thirteen EdgeKernel enumerators, and edge_l0_kernel of layer 0) against the float64 layer
oracle tests/edge_oracle.py at its size edges: partial waves and workgroups, Nd = 1, Ns = 16, `rows` on layers the released schedule never
down-samples, repeated neighbours and the point itself, instances of very different magnitude in one batch, an all-zero instance.  The cases,
their inputs and the rule are tests/tools/edge_vs_float64.py: per DESTINATION POINT (a wrong small point cannot hide behind a large one)
    err = max over points of max |out - ref| over the point's 3 x Co block / max |ref| over the block  <=  min(16 x e32, 1e-4),
e32 the same error of the float32 oracle, computed here on the CPU from the same inputs; e32 < 1e-5 is asserted as a precondition.
tests/test_edge_plan_cpu.py shows that the ladder reaches every enumerator.  The side products of the kernels (row maxima, partial column sums
for the residual global conv) are held through whole encodes of three reduced schedules in which every layer >= 2 is such a kernel."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from livingscenes_amd import synth

pytestmark = pytest.mark.gpu
TOL = 1e-4  # of the reference tensor's max-norm (the encodes)
TOOL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools", "edge_vs_float64.py")


def _load():
    spec = importlib.util.spec_from_file_location("edge_vs_float64", TOOL)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


lad = _load()   # one module object: the float64 references it caches serve every test of this file


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    return lad.compile_plan_dump(tmp_path_factory.mktemp("edge_plan"))


# ------------------------------------------------------------------------------------------------ 3a: the ladder, in this process's mode
@pytest.mark.parametrize("model,layer", lad.groups(), ids=[f"{m}-{i}" for m, i in lad.groups()])
def test_edgeconv_vs_float64_per_destination_point(model, layer, plan_exe):
    """Every case x kind x option setting of one (model, layer): a few dozen tiny launches.  Prints the largest err / e32 per kernel."""
    cases = [c for c in lad.ladder() if (c[1], c[2]) == (model, layer)]
    table, bad = lad.check_cases(cases, lad.own_mode(), _dev(), plan_exe)
    print(f"[{model} layer {layer}, mode {lad.own_mode()}] largest err / e32 per kernel\n{lad.format_table(table)}")
    assert not bad, f"{len(bad)} failures:\n" + "\n".join(bad[:20])


# ------------------------------------------------------------------------------------------------ 3b: the other arithmetic modes
def test_edgeconv_vs_float64_in_every_arithmetic_mode(plan_exe, tmp_path):
    """LS_GEMM_MODE is read once per process: the whole ladder under the same rule in this process for its own mode, then bf16x3 / fp32 (or the
    default) once each in a fresh child under a time limit (tests/tools/edge_vs_float64.py --check MODE; the float64 references computed here
    are handed over in a file).  A child that dies of a signal or runs out of time fails the test, and no further child is started."""
    mine = lad.own_mode()
    table, bad = lad.check_cases(lad.ladder(), mine, _dev(), plan_exe)
    print(f"[mode {mine}] largest err / e32 per kernel\n{lad.format_table(table)}")
    assert not bad, f"{len(bad)} failures:\n" + "\n".join(bad[:20])
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
        print(p.stdout[-4000:])
        assert p.returncode >= 0, f"mode {mode}: the child died of signal {-p.returncode}; no further child started\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}"
        assert p.returncode == 0, (mode, p.stdout[-4000:], p.stderr[-2000:])


# ------------------------------------------------------------------------------------------------ 3c: the side products, through encode
def relerr(a, b):
    a = np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, dtype=np.float64)
    b = np.asarray(b.detach().cpu() if torch.is_tensor(b) else b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def _codes_vs_oracle(cfg, w, x, tr, ref, dev_out, what):
    """One encode against net.encoder_forward on the same cloud, as tests/test_hip_parity.py::test_encoder_forward_vs_oracle judges it: FPS and
    layer-0 lists bit-exact; a deeper list may differ from the oracle's by feature-space near-ties, and the oracle re-run on the DEVICE's lists
    is then the reference of the codes; codes per instance within TOL."""
    from oracle import net
    hz, hi, hs, ht, knn_l, fps_l = dev_out
    B, L = x.shape[0], cfg["num_layers"]
    assert np.array_equal(knn_l[0].cpu().numpy(), tr["knn_idx_0"].numpy().astype(np.int32)), what
    for j, i in enumerate(cfg["down_sample_layers"]):
        assert np.array_equal(fps_l[j].cpu().numpy(), tr[f"fps_idx_{i}"].numpy().astype(np.int32)), f"{what}: fps level {j}"
    center, scale, z_so3, z_inv = ref
    flipped = False
    for i in range(1, L):
        rate = (knn_l[i].cpu().numpy() == tr[f"knn_idx_{i}"].numpy()).mean()
        assert rate > 0.995, f"{what}: layer {i}: k-NN index agreement {rate:.5f}"
        flipped |= rate < 1.0
    if flipped:
        tr2 = {}
        center, scale, z_so3, z_inv = net.encoder_forward(w, cfg, x, trace=tr2, graph={i: knn_l[i].cpu() for i in range(1, L)})
        for i in range(1, L):
            a, ref_idx = knn_l[i].cpu().numpy().astype(np.int64), tr[f"knn_idx_{i}"].numpy()
            if np.array_equal(a, ref_idx) or not torch.equal(tr[f"src_f_{i}"], tr2[f"src_f_{i}"]):
                continue   # (below the first flipped layer the two runs see different features: only the first one can be judged)
            src = tr[f"src_f_{i}"].reshape(B, -1, tr[f"src_f_{i}"].shape[-1]).transpose(1, 2).double().numpy()
            dst = tr[f"dst_f_in_{i}"].reshape(B, -1, tr[f"dst_f_in_{i}"].shape[-1]).transpose(1, 2).double().numpy()
            bb, nn, kk = np.nonzero(a != ref_idx)
            d_dev = ((dst[bb, nn] - src[bb, a[bb, nn, kk]]) ** 2).sum(-1)
            d_ref = ((dst[bb, nn] - src[bb, ref_idx[bb, nn, kk]]) ** 2).sum(-1)
            assert (np.abs(d_dev - d_ref) <= 1e-5 * np.maximum(d_ref, 1e-30)).all(), f"{what}: layer {i}: a flipped neighbour is not a near-tie"
    for b in range(B):
        errs = (relerr(hz[b], z_so3[b]), relerr(hi[b], z_inv[b]), relerr(hs[b], scale[b]), relerr(ht[b], center.reshape(B, 3)[b]))
        assert max(errs) < TOL, f"{what}: instance {b}: z_so3 / z_inv / s / t differ by {errs}"


@pytest.mark.parametrize("name,N", lad.REDUCED, ids=[f"{n}-{N}" for n, N in lad.REDUCED])
def test_encode_on_reduced_schedules_holds_the_side_products(name, N):
    """Row maxima and partial column sums of the edge kernels feed the residual global conv (its operand scaling, its mean); only whole encodes
    see them.  edge_vs_float64.reduced_cfg: schedules in which every layer >= 2 is a kernel that emits them (FT_256 / FT_128 / the three ATTN_FQ
    forms, and ATTN_V4_16 / 32 with LS_OPT_EDGE_FUSE_Q = 0; tests/test_edge_plan_cpu.py states what is planned and written), B = 3,
    LS_OPT_GLOB_FUSE 0 / 1 / 2, per instance against the oracle.  Once more with the three clouds scaled by 2^-6, 1, 2^5, which moves the
    instances' row maxima 11 binades apart (the encoder is positively homogeneous up to its tail; the oracle on the scaled clouds is the
    reference)."""
    from livingscenes_amd import _lib, ops, packing
    from oracle import net
    cfg = lad.reduced_cfg(name)
    w = synth.make_encoder_weights(cfg, 0)
    desc, blob = packing.pack_model(w, cfg, None, None)
    m = ops.HipModel(desc, blob, _dev())
    x0 = synth.make_instances(3, N, seed=5, rigid=False)
    x0 = (x0 - x0.mean(-1, keepdim=True)) / 1.1
    try:
        for scales in ((1.0, 1.0, 1.0), (2.0 ** -6, 1.0, 2.0 ** 5)):
            x = x0 * torch.tensor(scales)[:, None, None]
            tr = {}
            ref = net.encoder_forward(w, cfg, x, trace=tr)
            for fq in ((1, 0) if name == "fq" else (1,)):
                for gf in (0, 1, 2):
                    prev = [(o, m.set_option(o, v)) for o, v in ((_lib.OPT_EDGE_FUSE_Q, fq), (_lib.OPT_GLOB_FUSE, gf))]
                    try:
                        out = m.encode(x.to(_dev()), pre_normalised=True, trace=True)
                        torch.cuda.synchronize()
                    finally:
                        for o, v in prev:
                            m.set_option(o, v)
                    _codes_vs_oracle(cfg, w, x, tr, ref, out, f"{name} N={N} scales={scales} fuse_q={fq} glob_fuse={gf}")
    finally:
        m.close()
