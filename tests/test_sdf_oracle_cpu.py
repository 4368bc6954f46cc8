"""tests/sdf_oracle.py, the float64 yardstick of the SDF decoder and its backward, pinned to oracle.net: in float32 `field` must give
net.field_query and `field_grads` the autograd gradients of net.field_query_with_grad BIT FOR BIT, on the small and the released decoder.  Then
the ladder of tests/tools/sdf_vs_float64.py where no GPU is needed to see it: every decoder packs, every input meets both preconditions
(e32 < 1e-5 on each figure, max |sdf| < 0.5), and the plan (csrc/gemm_plan.h, compiled on its own) launches for the cases the GEMM kernels the
ladder was built to reach.  No GPU needed.

What the ladder does not reach: the 256 x 256 wide kernels (W2*) need cdiv(M, 256) x cdiv(N, 256) >= 256 tiles, about 20 000 rows at the
released width; they stay with test_hip_parity.py::test_sdf_dense_grid_mise_resolution."""
import importlib.util
import os

import pytest
import torch

import sdf_oracle as so
from livingscenes_amd import packing, synth
from oracle import net


def _ladder():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools", "sdf_vs_float64.py")
    spec = importlib.util.spec_from_file_location("sdf_vs_float64", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


lad = _ladder()


@pytest.mark.parametrize("which", ["small", "released"])
def test_oracle_reproduces_field_query_and_its_autograd_bit_for_bit(which):
    dcfg = synth.small_decoder_cfg() if which == "small" else synth.default_decoder_cfg()
    dw = synth.make_decoder_weights(dcfg, 0)
    B, M, L = 3, 129, dcfg["latent_size"]
    g = torch.Generator().manual_seed(5)
    code = {"z_so3": 0.05 * torch.randn(B, L, 3, generator=g), "z_inv": 0.05 * torch.randn(B, L, generator=g), "s": 0.75 + 0.5 * torch.rand(B, generator=g),
            "t": 0.1 * torch.randn(B, 1, 3, generator=g)}
    q = synth.make_queries(B, M, seed=11) * code["s"][:, None, None] + code["t"]
    q[0, 0] = code["t"][0, 0]                    # a query at the instance origin: |q| = 0, gradient 0 through the norm
    gsdf = torch.randn(B, M, generator=g)
    want = net.field_query(dw, dcfg, q, code)
    got = so.field(dw, dcfg, q, code, torch.float32, "inner")
    assert got.dtype == torch.float32 and torch.equal(got, want)
    leaves = {k: v.clone().requires_grad_(True) for k, v in code.items()}
    ql = q.clone().requires_grad_(True)
    sdf_ref = net.field_query_with_grad(dw, dcfg, ql, leaves)
    (sdf_ref * gsdf).sum().backward()
    sdf, grads = so.field_grads(dw, dcfg, q, code, gsdf, torch.float32, "inner")
    assert torch.equal(sdf, sdf_ref.detach())
    for name, a, b in zip(so.GRAD_NAMES, grads, (ql.grad, leaves["z_so3"].grad, leaves["z_inv"].grad, leaves["s"].grad, leaves["t"].grad.reshape(B, 3))):
        assert a.dtype == torch.float32 and torch.equal(a, b), name
    assert torch.isfinite(grads[0]).all() and (grads[0][0, 0] != 0).any()
    # ... and the float64 form is the same function: it differs from the float32 one by fp32 round-off
    ref, grads64 = so.field_grads(dw, dcfg, q, code, gsdf, torch.float64, "inner")
    assert ref.dtype == torch.float64 and all(v.dtype == torch.float64 for v in grads64)
    assert so.sdf_err(sdf, ref) < 1e-5 and max(so.instance_errs(grads[1:], grads64[1:]).values()) < 1e-5 and so.query_grad_err(grads[0], grads64[0], gsdf) < 1e-5


def test_a_stated_activation_pattern_replaces_relu_and_nothing_else():
    """mlp on the pattern [z_l > 0] of its own evaluation gives the SDF and the gradients of the plain evaluation bit for bit (float64 and
    float32); one unit moved to the other side changes the gradient of its row alone, and pattern_violations counts it: as a flip where its
    pre-activation is within the tolerance of zero, as wrong where it is not, and so a live padding column."""
    dcfg = synth.small_decoder_cfg()
    dw = synth.make_decoder_weights(dcfg, 0)
    B, M, L = 2, 9, dcfg["latent_size"]
    g = torch.Generator().manual_seed(8)
    code = {"z_so3": 0.05 * torch.randn(B, L, 3, generator=g), "z_inv": 0.05 * torch.randn(B, L, generator=g), "s": 0.75 + 0.5 * torch.rand(B, generator=g),
            "t": 0.1 * torch.randn(B, 1, 3, generator=g)}
    q, gsdf = synth.make_queries(B, M, seed=3), torch.randn(B, M, generator=g)
    for dtype in (torch.float64, torch.float32):
        tr = []
        sdf, grads = so.field_grads(dw, dcfg, q, code, gsdf, dtype, "inner", trace=tr)
        assert [tuple(z.shape) for z in tr] == [(B * M, 128), (B * M, 63), (B * M, 128), (B * M, 128)]
        pattern = [z > 0 for z in tr]
        sdf_p, grads_p = so.field_grads(dw, dcfg, q, code, gsdf, dtype, "inner", masks=pattern)
        assert torch.equal(sdf_p, sdf) and all(torch.equal(a, b) for a, b in zip(grads_p, grads))
    assert so.pattern_violations(pattern, tr, 1e-4) == (0, 0)
    row = 4
    unit = int(tr[2][row].abs().argmax())                      # the unit of layer 2 farthest from zero in that row
    moved = [p.clone() for p in pattern]
    moved[2][row, unit] = ~moved[2][row, unit]
    assert so.pattern_violations(moved, tr, 1e-4) == (1, 1) and so.pattern_violations(moved, tr, 2.0) == (1, 0)
    _, grads_m = so.field_grads(dw, dcfg, q, code, gsdf, torch.float64, "inner", masks=moved)
    _, grads = so.field_grads(dw, dcfg, q, code, gsdf, torch.float64, "inner")
    changed = (grads_m[0] != grads[0]).reshape(B * M, 3).any(-1)
    assert changed[row] and int(changed.sum()) == 1
    padded = [torch.cat([p, torch.zeros(B * M, 1, dtype=torch.bool)], 1) for p in pattern]
    assert so.pattern_violations(padded, tr, 1e-4) == (0, 0)
    padded[1][0, -1] = True
    assert so.pattern_violations(padded, tr, 1e-4) == (0, 1)


def test_xyz_kind_feeds_the_raw_query_after_the_code():
    """decoder_type "deepsdf": u = [z_inv | query]; z_so3, s and t do not enter and their gradients are exact zeros"""
    dcfg = synth.small_inv_decoder_cfg()
    dw = synth.make_decoder_weights(dcfg, 0)
    g = torch.Generator().manual_seed(6)
    B, M, L = 2, 7, dcfg["latent_size"]
    z_inv, q = 0.05 * torch.randn(B, L, generator=g), torch.randn(B, M, 3, generator=g)
    code = {"z_so3": torch.randn(B, L, 3, generator=g), "z_inv": z_inv, "s": torch.rand(B, generator=g) + 0.5, "t": torch.randn(B, 1, 3, generator=g)}
    want = net.decoder_forward(dw, dcfg, torch.cat([z_inv[:, None, :].expand(B, M, L), q], -1))
    assert torch.equal(so.field(dw, dcfg, q, code, torch.float32, "xyz"), want)
    assert torch.equal(so.field(dw, dcfg, q, {"z_inv": z_inv}, torch.float32, "xyz"), want)
    _, grads = so.field_grads(dw, dcfg, q, code, torch.ones(B, M), torch.float64, "xyz")
    assert (grads[0] != 0).any() and (grads[2] != 0).any()
    for k in (1, 3, 4):
        assert (grads[k] == 0).all(), so.GRAD_NAMES[k]


def test_error_measures_do_not_let_a_row_or_an_instance_hide():
    ref = torch.ones(3, 5, dtype=torch.float64)
    ref[2] *= 1e6                                 # a large last instance
    a = ref.clone()
    a[0, 3] += 1e-3                               # 1e-9 of the tensor's max-norm, 1e-3 of the instance's
    assert abs(so.sdf_err(a, ref) - 1e-3) < 1e-12
    assert abs(so.sdf_err_rows(a.reshape(-1), ref.reshape(-1), (5, 5, 0, 5)) - 1e-3) < 1e-12
    ref[1] = 0
    a[1] = 0
    a[1, 0] = 1e-30                               # an all-zero instance has to stay zero
    assert so.sdf_err(a, ref) == float("inf")
    # the query gradient: a row with a 2^-12 upstream gradient is judged on its own scale
    gsdf = torch.tensor([[1.0, 2.0 ** -12]])
    gref = torch.tensor([[[1.0, 0.0, 0.0], [2.0 ** -12, 0.0, 0.0]]], dtype=torch.float64)
    gq = gref.clone()
    gq[0, 1, 1] = 2.0 ** -12 * 1e-3               # 2.4e-7 of the tensor's max-norm
    assert abs(so.query_grad_err(gq, gref, gsdf) - 1e-3) < 1e-12
    assert so.query_grad_err(torch.zeros(1, 2, 3), torch.zeros(1, 2, 3), gsdf) == 0.0
    gq = torch.zeros(1, 2, 3)
    gq[0, 0, 0] = 1e-30
    assert so.query_grad_err(gq, torch.zeros(1, 2, 3), gsdf) == float("inf")


@pytest.mark.parametrize("dec", list(lad.DECODERS))
def test_every_ladder_decoder_packs(dec):
    w, nh, li, L, kind = lad.DECODERS[dec]
    for dead0 in (False, True):
        ecfg, dcfg = lad.cfgs(dec)
        desc, blob = packing.pack_model(synth.make_encoder_weights(ecfg, 0), ecfg, lad.weights(dec, dead0), dcfg)
        assert (desc.dec_num_linear, desc.dec_width, desc.dec_latent_in, desc.c_dim) == (nh + 1, w, li[0] if li else -1, L)
        assert desc.dec_input == (1 if kind == "xyz" else 0) and blob.size == desc.blob_floats


@pytest.mark.parametrize("dec", list(lad.DECODERS))
def test_every_ladder_input_meets_both_preconditions(dec):
    """The preconditions of tests/test_hip_sdf_f64.py: on every case and kind the float32 oracle is within E32_MAX = 1e-5 of the float64 one on
    each figure and max |sdf| < 0.5, so that the GPU tests can fail only on the kernel; 'xyz' gives exact zeros for z_so3, s and t, and dead0
    leaves the no-skip decoder a constant."""
    worst, where = {f: 0.0 for f in lad.FIGURES}, {}
    for case in lad.ladder(dec):
        for kind in lad.KINDS:
            ref, e32 = lad.reference(case, kind)
            assert torch.isfinite(ref[0]).all() and float(ref[0].abs().max()) < lad.SDF_MAX, (case[0], kind, float(ref[0].abs().max()))
            assert set(e32) == ({"sdf"} if case[2] == "rows" else set(lad.FIGURES))
            for f, e in e32.items():
                assert 0 <= e < lad.E32_MAX, (case[0], kind, f, e)
                if e > worst[f]:
                    worst[f], where[f] = e, f"{case[0]} {kind}"
            if ref[1] is not None:
                assert all(torch.isfinite(v).all() for v in ref[1])
                if lad.kind_of(dec) == "xyz":
                    assert all((ref[1][k] == 0).all() for k in (1, 3, 4)), case[0]
                if kind == "dead0" and dec.startswith("noskip"):
                    assert (ref[1][0] == 0).all() and (ref[0] == ref[0][0]).all(), case[0]
            if kind == "rows" and lad.kind_of(dec) == "inner" and lad.counts_of(case)[0]:
                inp = lad.inputs(case, kind)
                assert torch.equal(inp["query"][0], inp["t"][0, 0]), case[0]
    print(f"largest e32 of the {dec} ladder: " + ", ".join(f"{f} {worst[f]:.3e} ({where.get(f, '-')})" for f in lad.FIGURES))


# ------------------------------------------------------------------------------------------------ what the plan launches for the ladder
@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    return lad.compile_plan_dump(tmp_path_factory.mktemp("gemm_plan"))


REDUCE = "ls::gemm_splitk_reduce_kernel"
F16X2, H2, H2_PLANES, H2_ANYK = ("ls::gemm_f32_kernel<true, 22>", "ls::gemm_h2_kernel<true, false>", "ls::gemm_h2_kernel<true, true>",
                                 "ls::gemm_h2_kernel<false, false>")


def test_the_ladder_reaches_the_kernels_it_was_built_for(dump):
    """Default mode, on the decoder's GemmTraits as record_gemm_launches.sdf_traits_of forms them."""
    mode = lad.MODES[0]
    chains = {}
    for dec in lad.DECODERS:
        cases = lad.ladder(dec)
        chains.update(zip((c[0] for c in cases), lad.planned(cases, mode, dump)))
    kernels = lambda key: [g[0] for g in chains[key]]
    # no inference case splits K, whatever its size
    for dec in lad.DECODERS:
        for case in lad.ladder(dec):
            if case[2] != "train":
                assert all(g == g[:1] for g in chains[case[0]]), case[0]
    # forward GEMMs per decoder: layers 1 .. nl - 2, K = the width except after the narrow layer
    assert kernels("decode(small, B=3, M=129)") == [H2, F16X2, H2]                    # the narrow layer (K = 128, N = 64), the skip layer's GEMM (K = 64), K = 128
    assert kernels("decode(noskip, B=3, M=129)") == [H2, H2] and kernels("decode(noskip_inv, B=1, M=1)") == [H2, H2]
    assert kernels("decode(skip_last, B=3, M=129)") == [H2, H2, F16X2]                # the narrow layer is the last GEMM with a bias, the skip GEMM has K = 64
    assert kernels("decode(w132, B=3, M=129)") == [H2_ANYK, H2_ANYK, H2_ANYK]         # K = 132, 68, 132
    assert kernels("decode(w132_inv, B=3, M=129)") == [H2_ANYK, H2_ANYK, H2_ANYK]     # K = 132, 100, 132 (the narrow layer is 132 - 35 = 97 -> 100 wide)
    assert kernels("decode(w260, B=1, M=257)") == [H2_ANYK, H2_ANYK, H2_ANYK]         # K = 260, 196, 260
    assert kernels("decode(w64, B=2, M=65)") == [F16X2, F16X2, F16X2]                 # K = 64, 52, 64
    assert set(kernels("decode(released, B=3, M=129)")) == {H2_PLANES, H2}            # W planes at K = 768; the K = 256 layer after the narrow one has none
    assert kernels("decode(released, B=3, M=129)").count(H2) == 1
    assert set(kernels("decode(inv, B=3, M=129)")) == {H2_PLANES, H2}
    assert kernels("decode_rows(w132, rows=[64, 1, 0, 129, 1])") == [H2_ANYK] * 3
    # training at small M with the split-K scratch: the launches with K >= 128 split and write no out_rowmax (RowMaxChain::emit_none), the narrow
    # K <= 64 ones do not; without the scratch (splitk = 0) the backward runs masked and nothing splits
    tr = chains["train(small, B=3, M=2, splitk=1)"]
    assert [g[0] for g in tr] == [H2, F16X2, H2, H2, H2, F16X2] and [len(g) for g in tr] == [2, 1, 2, 2, 2, 1], tr
    case = next(c for c in lad.ladder("small") if c[0] == "train(small, B=3, M=2, splitk=1)")
    # (the skip layer's GEMM hands its maxima to the accumulate launch and never asks; of the others only the one that stays whole does)
    assert [t["wants_out_rowmax"] for t in lad.gemm_traits(case)] == [0, 0, 0, 0, 0, 1]
    assert all(len(g) == 2 and g[1] == REDUCE for g in chains["train(noskip, B=1, M=1, splitk=1)"])
    tr = chains["train(w132, B=3, M=129, splitk=1)"]
    assert [g[0] for g in tr] == [H2_ANYK] * 6 and [len(g) for g in tr] == [2, 1, 2, 2, 2, 1], tr      # K = 68 (forward of the skip layer, backward of the narrow one) stays whole
    for dec in lad.DECODERS:
        for B, M in lad.dense_shapes(dec):
            assert all(len(g) == 1 for g in chains[f"train({dec}, B={B}, M={M}, splitk=0)"]), (dec, B, M)
    assert [g[0] for g in chains["train(released, B=3, M=129, splitk=1)"]].count(H2_PLANES) >= 10
    assert any(len(g) == 2 for g in chains["train(released, B=3, M=129, splitk=1)"])


@pytest.mark.parametrize("mode,kernel", [("bf16x3", "ls::gemm_f32_kernel<true, 3>"), ("fp32", "ls::gemm_f32_kernel<false, 3>")])
def test_the_other_modes_run_their_own_tiled_kernel(dump, mode, kernel):
    for dec in lad.DECODERS:
        cases = lad.ladder(dec)
        for case, gemms in zip(cases, lad.planned(cases, mode, dump)):
            assert all(g[0] == kernel and set(g[1:]) <= {REDUCE} for g in gemms), (case[0], gemms)
