"""tests/edge_oracle.py, the one-layer float64 yardstick of the edge-conv kernels, pinned to oracle.net: in float32, on the tensors of
net.encoder_forward's own trace, `layer` must give trace["msg_f_i"] BIT FOR BIT, for every layer (layer 0 with its cross products, the pool
layer, the down-sampling layers through `rows`) of the small and the released configuration.  oracle.net itself is pinned to the reference's
modules by tests/test_oracle_golden.py.  No GPU needed."""
import pytest
import torch

import edge_oracle
from livingscenes_amd import synth
from oracle import net


@pytest.mark.parametrize("which,N", [("small", 128), ("released", 1024)])
def test_layer_reproduces_the_trace_of_encoder_forward_bit_for_bit(which, N):
    cfg = synth.small_encoder_cfg() if which == "small" else synth.default_encoder_cfg()
    w = synth.make_encoder_weights(cfg, 0)
    x = synth.make_instances(2, N, seed=11, rigid=False)
    x = (x - x.mean(-1, keepdim=True)) / 1.2
    tr = {}
    net.encoder_forward(w, cfg, x, trace=tr)
    for i in range(cfg["num_layers"]):
        rows = tr[f"fps_idx_{i}"] if i in cfg["down_sample_layers"] else None
        msg = edge_oracle.layer(w, cfg, i, tr[f"src_f_{i}"], tr[f"knn_idx_{i}"], rows, torch.float32)
        assert msg.dtype == torch.float32 and torch.equal(msg, tr[f"msg_f_{i}"]), f"layer {i}"
        # ... and the float64 form is the same function: it differs from the float32 one by fp32 round-off, per destination point
        ref = edge_oracle.layer(w, cfg, i, tr[f"src_f_{i}"], tr[f"knn_idx_{i}"], rows, torch.float64)
        assert ref.dtype == torch.float64 and edge_oracle.per_point_err(msg, ref) < 1e-5, f"layer {i}"


def test_per_point_err_does_not_let_a_small_point_hide():
    ref = torch.ones(1, 2, 3, 4, dtype=torch.float64)
    ref[..., 0] *= 1e6
    ref[..., 3] = 0
    a = ref.clone()
    assert edge_oracle.per_point_err(a, ref) == 0.0
    a[0, 1, 2, 1] += 1e-3                      # 1e-9 of the tensor's max-norm, 1e-3 of the point's
    assert abs(edge_oracle.per_point_err(a, ref) - 1e-3) < 1e-12
    a[0, 0, 0, 3] = 1e-30                      # a zero point has to stay zero
    assert edge_oracle.per_point_err(a, ref) == float("inf")


def _ladder():
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools", "edge_vs_float64.py")
    spec = importlib.util.spec_from_file_location("edge_vs_float64", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_ladder_input_is_well_conditioned():
    """The precondition of tests/test_hip_edge_layers_f64.py, where no GPU is needed to see it: on every case and kind of
    tests/tools/edge_vs_float64.py the float32 oracle is within 1e-5 of the float64 one per destination point (so 16 x e32 is a bound below TOL
    that an fp32 implementation can meet), and an all-zero instance gives an exactly zero message in both."""
    lad = _ladder()
    worst, seen = 0.0, set()
    for case in lad.ladder():
        if lad.shape_key(case) in seen:
            continue
        seen.add(lad.shape_key(case))
        for kind in lad.kinds_of(case[3][0]):
            if kind == "zero":
                cfg, w = lad.weights(case[1])
                src, knn, rows = lad.inputs(case, kind)
                for dt in (torch.float32, torch.float64):
                    out = edge_oracle.layer(w, cfg, case[2], src, knn, rows, dt)
                    assert (out[1] == 0).all() and (out[0] != 0).any() and (out[2] != 0).any(), (case[0], dt)
                continue
            ref, e32 = lad.reference(case, kind)
            assert torch.isfinite(ref).all() and 0 < e32 < lad.E32_MAX, (case[0], kind, e32)
            worst = max(worst, e32)
    print(f"largest e32 of the ladder: {worst:.3e}")
    assert lad.bound(worst) < lad.TOL
