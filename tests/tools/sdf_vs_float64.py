"""The SDF decoder and its backward against the float64 oracle tests/sdf_oracle.py at their size edges: the decoders, the row ladders, the
inputs and the rule.

    python tests/tools/sdf_vs_float64.py --check MODE [--refs FILE]    (GPU; the process must be in arithmetic mode MODE: LS_GEMM_MODE unset /
                                                                        bf16x3 / fp32; FILE: references another process saved, else computed)
It runs every decoder's ladder under the rule below, prints the largest err / e32 per kernel chain and exits non-zero with the failing keys.

DECODERS and ladder() are the one statement of the cases, shared by tests/test_sdf_oracle_cpu.py (the preconditions on the inputs, which GEMM
kernels the plan launches for them) and tests/test_hip_sdf_f64.py (the comparison, the exact relations).
  a decoder   (width x hidden layers, skip, c_dim, kind): the four the project serves (small, small_inv, released, inv) and
              noskip / noskip_inv   128 x 3, no skip: dec_latent_in = -1 -- one prep launch, no accumulate launch, sdf_code_grad_kernel with a null
                                    second table, the li < 0 branches of ls_sdf_backward
              skip_last             128 x 4, skip at the last hidden layer (li = nl - 2): the accumulate feeds sdf_out_kernel, the narrow layer is the
                                    last GEMM with a bias
              w132 / w132_inv       width 132: one live lane in a 16-lane row-max group, a partly live last 64-column block, short last trips,
                                    K % 32 != 0 in every GEMM (H2_ANYK), narrow layer 67 -> 68
              w260                  width 260: a second column block with one live lane, 8 row-max parts of which three are always 0, a second
                                    trip of sdf_out_kernel with one live lane, narrow layer 195 -> 196
              w64                   width 64, c_dim 6: the K <= 64 kernel, narrow layer 51 -> 52, c_dim % 8 != 0 in sdf_prep_kernel's unrolled loop
  a case      one entry point at one shape: ('decode', (B, M)) = HipModel.sdf_decode; ('rows', counts) = sdf_decode_rows on counts[b] rows of
              instance b; ('train', (B, M), splitk) = sdf_decode_train + sdf_backward under LS_OPT_SDF_TRAIN_SPLITK = splitk
Every case runs on four kinds of input (KINDS), seeded from the case's shape key:
  randn   codes 0.05 randn, t 0.1 randn, s in [0.75, 1.25), normalised queries in the MISE box (|q| <= 0.55 sqrt 3)
  rows    s = 2^-6, 1, 2^5 cycled over the instances; normalised queries of magnitude 2^U(-10, 4) in random directions, row 0 of instance 0
          exactly at t ('xyz' decoders read the raw query: they are given the normalised one)
  zero    randn with z_so3 = z_inv = 0 in instance 1 (instance 0 when B = 1)
  dead0   the inputs of 'rows' on the decoder with lin0.bias - 64: every layer-0 activation is 0, so are the row maxima the first GEMM is given
The backward's upstream gradient is randn 2^k, k drawn per row from -12 .. 0.

The rule.  Three figures per case, each against sdf_oracle.field / field_grads in float64:
  sdf     per row |sdf - ref| / the instance's max |ref|                                                   (sdf_oracle.sdf_err)
  code    z_so3, z_inv, s and t gradients, per instance and per output                                       (sdf_oracle.instance_errs)
  query   per row ||gq[r] - ref[r]||_inf / (|gsdf[r]| G_b), G_b the instance's largest ||ref[r]||_inf / |gsdf[r]|   (sdf_oracle.query_grad_err)
The gradient of a ReLU network is defined only given its activation pattern, and a unit whose pre-activation is zero to within round-off is
counted on either side by any finite-precision forward, which moves a row's gradient by about 1 / width -- far more than 16 x e32, and on other
units on every host.  So both gradient figures are taken on a STATED pattern: the device's gradients against float64 on the pattern of the
activations the device kept (read from the training workspace; it may differ from float64's own only in units within TOL of zero relative to
their row, which is asserted), the float32 oracle's e32 on float64's own pattern.
err <= min(MARGIN x max(e32, 2^-23), TOL), e32 the same figure of the float32 oracle on the same inputs, computed on the CPU; e32 < E32_MAX and
max |ref sdf| < 0.5 (tanh far from saturation: it would hide an error before it) are preconditions of every input.  The floor 2^-23 is one float32
ulp of the denominator: below it e32 measures the luck of a constant output (noskip on dead0: every row the same value), not accuracy.  An all-zero
reference ('xyz': z_so3, s, t gradients; noskip on dead0: the query gradient) must be met exactly.  The margin and both caps are
tests/tools/edge_vs_float64.py's.  With LS_OPT_SDF_BF16X2 (two-piece products, 2^-16 each) the sdf figure of every forward entry point is held
to the flat TOL instead, the gradients are measured and printed."""
import argparse
import binascii
import os
import sys

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
for p in (REPO, os.path.join(REPO, "tests"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

from edge_vs_float64 import E32_MAX, MARGIN, MODES, TOL, own_mode  # noqa: E402
from glob_tail_vs_float64 import PLAN_FIELDS, _plan, compile_plan_dump, format_table  # noqa: E402,F401

KINDS = ("randn", "rows", "zero", "dead0")
SCALES = (2.0 ** -6, 1.0, 2.0 ** 5)        # 'rows' / 'dead0': s of instance b = SCALES[b % 3]
E32_FLOOR = 2.0 ** -23
SDF_MAX = 0.5
FIGURES = ("sdf", "code", "query")
# Shape keys whose inputs were replaced (the suffix goes into the seed).  The figure that decides is the s gradient, one sum over an instance's
# rows that can nearly cancel, and its e32 is a property of the host's float32 BLAS as much as of the input: the first inputs of three shapes
# broke the precondition (e32 = 5.9e-5 at small 2 x 65, 8.8e-5 at released 2 x 63, 3.8e-5 at skip_last 3 x 2), four came within a factor of two
# of it (5.2e-6 .. 7.7e-6), and small 2 x 63 measured 1.4e-6 on one host and 7.7e-6 on another.  The seeds below are the first with e32 < 5e-6
# on every kind and figure, so that the precondition does not hang on the host.
RESEED = {"sdf:small:3:2": "#1", "sdf:small:2:63": "#1", "sdf:small:2:65": "#1", "sdf:small:3:129": "#1", "sdf:released:2:63": "#1",
          "sdf:released:2:64": "#1", "sdf:skip_last:3:2": "#1", "sdf:w260:2:64": "#1"}

# name: (width, hidden layers, skip, c_dim, kind)
DECODERS = {"small": (128, 4, [2], 32, "inner"), "small_inv": (128, 4, [2], 32, "xyz"), "released": (768, 8, [4], 256, "inner"),
            "inv": (512, 8, [4], 256, "xyz"), "noskip": (128, 3, [], 32, "inner"), "noskip_inv": (128, 3, [], 32, "xyz"),
            "skip_last": (128, 4, [3], 32, "inner"), "w132": (132, 4, [2], 32, "inner"), "w132_inv": (132, 4, [2], 32, "xyz"),
            "w260": (260, 4, [2], 32, "inner"), "w64": (64, 4, [2], 6, "inner")}
DENSE = ((1, 1), (3, 2), (2, 63), (2, 64), (2, 65), (3, 129), (1, 257))
RAGGED = ((64, 1, 0, 129, 1), (0, 5, 0), (1,))


def kind_of(dec):
    return DECODERS[dec][4]


def cfgs(dec):
    """(encoder cfg, decoder cfg): the encoder half is the small encoder at the decoder's c_dim (it is packed, never run)"""
    from livingscenes_amd import synth
    w, nh, li, L, kind = DECODERS[dec]
    ecfg = synth.small_encoder_cfg()
    ecfg["c_dim"] = L
    known = {"small": synth.small_decoder_cfg, "small_inv": synth.small_inv_decoder_cfg, "released": synth.default_decoder_cfg, "inv": synth.inv_decoder_cfg}
    if dec in known:
        dcfg = known[dec]()
        assert (dcfg["dims"], list(dcfg["latent_in"]), dcfg["latent_size"], dcfg["pe_dim"]) == ([w] * nh, li, L, 3 if kind == "xyz" else L + 1), dec
    else:
        dcfg = dict(dims=[w] * nh, dropout=None, dropout_prob=0.0, latent_dropout=False, latent_in=list(li), latent_size=L, norm_layers=list(range(nh)),
                    pe_dim=3 if kind == "xyz" else L + 1, use_tanh=False, weight_norm=True)
    return ecfg, dcfg


def dense_shapes(dec):
    return tuple(s for s in DENSE if not (dec in ("released", "inv") and s == (1, 257)))


def ladder(dec):
    """[(key, decoder, entry, shape, splitk)]: entry 'decode' / 'train' with shape (B, M), 'rows' with shape = rows per instance"""
    c = [(f"decode({dec}, B={B}, M={M})", dec, "decode", (B, M), None) for B, M in dense_shapes(dec)]
    c += [(f"decode_rows({dec}, rows={list(r)})", dec, "rows", r, None) for r in RAGGED]
    c += [(f"train({dec}, B={B}, M={M}, splitk={v})", dec, "train", (B, M), v) for B, M in dense_shapes(dec) for v in (1, 0)]
    return c


def counts_of(case):
    """rows per instance"""
    return tuple(case[3]) if case[2] == "rows" else (case[3][1],) * case[3][0]


# ------------------------------------------------------------------------------------------------ what the plan launches (CPU)
def gemm_traits(case, x2=False):
    """the GemmTraits of the case's decoder GEMMs, forward then (entry 'train') backward, as record_gemm_launches.sdf_traits forms them"""
    import record_gemm_launches as rec
    return rec.sdf_traits_of(cfgs(case[1])[1], sum(counts_of(case)), x2, case[4] if case[2] == "train" else None)


def planned(cases, mode, exe, x2=False):
    """-> [[[kernel name(, reduce)] per GEMM] per case]"""
    traits = [gemm_traits(c, x2) for c in cases]
    flat = _plan(exe, mode, [t for ts in traits for t in ts])
    out, n = [], 0
    for ts in traits:
        out.append(flat[n:n + len(ts)])
        n += len(ts)
    return out


def chain_label(case, gemms):
    """the entry point and the distinct GEMM kernels of its chain, in launch order"""
    names = list(dict.fromkeys(n for g in gemms for n in g))
    short = lambda n: n[4:] if n.startswith("ls::") else n
    return f"{case[2]}: " + ", ".join(short(n) for n in names)


# ------------------------------------------------------------------------------------------------ inputs and references (CPU)
_WEIGHTS, _INPUTS, _REFS = {}, {}, {}


def weights(dec, dead0=False):
    """the decoder's weights, seed 0; dead0: lin0.bias - 64"""
    from livingscenes_amd import synth
    if dec not in _WEIGHTS:
        _WEIGHTS[dec] = synth.make_decoder_weights(cfgs(dec)[1], 0)
    dw = _WEIGHTS[dec]
    return dict(dw, **{"lin0.bias": dw["lin0.bias"] - 64.0}) if dead0 else dw


def shape_key(case):
    """train and decode cases of one (decoder, B, M) see the same inputs"""
    return f"sdf:{case[1]}:" + (f"rows{list(case[3])}" if case[2] == "rows" else f"{case[3][0]}:{case[3][1]}")


def inputs(case, kind):
    """-> {query [R,3] (the instances' rows back to back), z_so3 [B,c,3], z_inv [B,c], s [B], t [B,1,3], gsdf [R]} float32"""
    import torch
    sk = shape_key(case)
    if (sk, kind) in _INPUTS:
        return _INPUTS[(sk, kind)]
    counts = counts_of(case)
    B, R, L = len(counts), sum(counts), DECODERS[case[1]][3]
    g = torch.Generator().manual_seed(binascii.crc32((sk + RESEED.get(sk, "")).encode()))
    z_so3, z_inv, t = 0.05 * torch.randn(B, L, 3, generator=g), 0.05 * torch.randn(B, L, generator=g), 0.1 * torch.randn(B, 1, 3, generator=g)
    s = 0.75 + 0.5 * torch.rand(B, generator=g)
    box = (torch.rand(R, 3, generator=g) - 0.5) * 1.1
    dirs = torch.randn(R, 3, generator=g)
    dirs = dirs / dirs.norm(dim=-1, keepdim=True)
    mag = 2.0 ** (torch.rand(R, 1, generator=g) * 14.0 - 10.0)
    gsdf = torch.randn(R, generator=g) * 2.0 ** -torch.randint(0, 13, (R,), generator=g).float()
    inst = torch.repeat_interleave(torch.arange(B), torch.tensor(counts))
    if kind in ("rows", "dead0"):
        s = torch.tensor([SCALES[b % 3] for b in range(B)])
        qn = dirs * mag
        if counts[0]:
            qn[0] = 0.0
    else:
        assert kind in ("randn", "zero"), kind
        qn = box
        if kind == "zero":
            z = 1 if B > 1 else 0
            z_so3[z], z_inv[z] = 0.0, 0.0
    query = qn if kind_of(case[1]) == "xyz" else qn * s[inst][:, None] + t[inst, 0]
    _INPUTS[(sk, kind)] = dict(query=query.contiguous(), z_so3=z_so3, z_inv=z_inv, s=s, t=t, gsdf=gsdf)
    return _INPUTS[(sk, kind)]


def instances(inp, counts):
    """the non-empty instances as ([1,n,3] query, the instance's code, [1,n] gsdf, row range)"""
    r0 = 0
    for b, n in enumerate(counts):
        if n:
            code = {k: inp[k][b:b + 1] for k in ("z_so3", "z_inv", "s", "t")}
            yield inp["query"][r0:r0 + n][None], code, inp["gsdf"][r0:r0 + n][None], (r0, r0 + n)
        r0 += n


def _figures(got, ref, gsdf, counts):
    """{figure: err} of (sdf [R], grads or None) against the float64 (sdf, grads): the grads are those of a dense case"""
    import sdf_oracle as so
    out = {"sdf": so.sdf_err_rows(got[0].reshape(-1), ref[0].reshape(-1), counts)}
    if ref[1] is not None and got[1] is not None:
        B, M = len(counts), counts[0]
        out["code"] = max(so.instance_errs(got[1][1:], ref[1][1:]).values())
        out["query"] = so.query_grad_err(got[1][0].reshape(B, M, 3), ref[1][0], gsdf.reshape(B, M))
    return out


def _dense_args(case, kind):
    """(decoder cfg, weights, query [B,M,3], code, gsdf [B,M], decoder kind) of a dense case"""
    dec, (B, M) = case[1], case[3]
    inp = inputs(case, kind)
    return (cfgs(dec)[1], weights(dec, kind == "dead0"), inp["query"].reshape(B, M, 3), {n: inp[n] for n in ("z_so3", "z_inv", "s", "t")},
            inp["gsdf"].reshape(B, M), kind_of(dec))


def reference(case, kind):
    """-> ((sdf64 [R], grads64 or None), {figure: e32}): the gradients with the dense shapes only (the ragged entry has no backward).  The
    gradients' e32: the float32 oracle on the float64 evaluation's activation pattern [z_l > 0] (sdf_oracle.mlp) -- its round-off, not the
    units it happens to count on the other side, which differ from host to host."""
    import torch
    import sdf_oracle as so
    k = (shape_key(case), kind)
    if k not in _REFS:
        dec, counts = case[1], counts_of(case)
        inp = inputs(case, kind)
        if case[2] == "rows":
            dcfg, dw = cfgs(dec)[1], weights(dec, kind == "dead0")
            ref, r32 = ((torch.cat([so.field(dw, dcfg, q, code, dtype, kind_of(dec))[0] for q, code, _, _ in instances(inp, counts)]), None)
                        for dtype in (torch.float64, torch.float32))
        else:
            dcfg, dw, q, code, gsdf, dk = _dense_args(case, kind)
            tr = []
            sdf, grads = so.field_grads(dw, dcfg, q, code, gsdf, torch.float64, dk, trace=tr)
            ref = (sdf.reshape(-1), grads)
            r32 = (so.field(dw, dcfg, q, code, torch.float32, dk).reshape(-1), so.field_grads(dw, dcfg, q, code, gsdf, torch.float32, dk, masks=[z > 0 for z in tr])[1])
        _REFS[k] = (ref, _figures(r32, ref, inp["gsdf"], counts))
    return _REFS[k]


def reference_on_pattern(case, kind, masks):
    """the float64 gradients of a dense case on the activation pattern `masks` (the device's own: device_pattern), after checking the pattern:
    it may differ from float64's [z_l > 0] only in units with |z_l| <= TOL x the row's largest |z_l| -- the project's tolerance on an
    activation row, under which such a unit has no defined sign -> (grads64, units flipped, units wrongly flipped)"""
    import torch
    import sdf_oracle as so
    dcfg, dw, q, code, gsdf, dk = _dense_args(case, kind)
    tr = []
    so.field(dw, dcfg, q, code, torch.float64, dk, trace=tr)
    flipped, wrong = so.pattern_violations(masks, tr, TOL)
    live = [m.cpu()[:, :z.shape[1]] for m, z in zip(masks, tr)]      # without the padding columns
    return so.field_grads(dw, dcfg, q, code, gsdf, torch.float64, dk, masks=live)[1], flipped, wrong


def all_references():
    """every reference of every ladder -> {figure: (largest e32, where)}, the largest |ref sdf|"""
    worst, top = {f: (0.0, "") for f in FIGURES}, 0.0
    for dec in DECODERS:
        for case in ladder(dec):
            for kind in KINDS:
                ref, e32 = reference(case, kind)
                top = max(top, float(ref[0].abs().max()))
                for f, e in e32.items():
                    if e > worst[f][0]:
                        worst[f] = (e, f"{case[0]} {kind}")
    return worst, top


def save_references(path):
    import torch
    torch.save({f"{a}|{kind}": v for (a, kind), v in _REFS.items()}, path)


def load_references(path):
    import torch
    for k, v in torch.load(path).items():
        _REFS[tuple(k.split("|"))] = v


def bound(e32):
    return min(MARGIN * max(e32, E32_FLOOR), TOL)


# ------------------------------------------------------------------------------------------------ the device side
def make_model(dec, dev, dead0=False):
    from livingscenes_amd import ops, packing, synth
    ecfg, dcfg = cfgs(dec)
    desc, blob = packing.pack_model(synth.make_encoder_weights(ecfg, 0), ecfg, weights(dec, dead0), dcfg)
    return ops.HipModel(desc, blob, dev)


def device_args(case, kind, dev):
    """(query [B,M,3] or [R,3], z_so3, z_inv, s, t) on the device"""
    inp = inputs(case, kind)
    q = inp["query"] if case[2] == "rows" else inp["query"].reshape(case[3][0], case[3][1], 3)
    return tuple(v.to(dev) for v in (q, inp["z_so3"], inp["z_inv"], inp["s"], inp["t"]))


def device_pattern(saved, dec):
    """[h_l > 0] of the activations sdf_decode_train kept, one bool [R, padded out_l] per hidden layer.  Mirrors sdf_buffers (model.hip):
    pieces on 256-byte boundaries (ls_workspace.h) -- A0, A4 [B,w,4], b0, b4 [B,w], then h_l [R,w] for l = 0 .. nl - 2, of which the layer
    before the skip fills pad4(w - u) columns."""
    import torch
    query, ws = saved[0], saved[-1]
    B, R = query.shape[0], query.shape[0] * query.shape[1]
    w, nh, li, L, kind = DECODERS[dec]
    u = L + 3 if kind == "xyz" else 2 * L + 1
    end, out = 0, []
    for l, floats in enumerate([B * w * 4, B * w * 4, B * w, B * w] + [R * w] * nh):
        o = (end + 255) // 256 * 256
        end = o + 4 * floats
        if l >= 4:
            cols = (w - u + 3) // 4 * 4 if li and l - 4 + 1 == li[0] else w
            out.append(ws[o:end].view(torch.float32).reshape(R, w)[:, :cols] > 0)
    assert end <= ws.numel()
    return out


def run_case(m, case, kind, dev):
    """-> (sdf [R], (gq, gso3, ginv, gs, gt) or None, the device's activation pattern or None) on the CPU"""
    import torch
    from livingscenes_amd import _lib
    args = device_args(case, kind, dev)
    if case[2] == "decode":
        return m.sdf_decode(*args).cpu().reshape(-1), None, None
    if case[2] == "rows":
        ri = torch.repeat_interleave(torch.arange(len(case[3]), dtype=torch.int32), torch.tensor(case[3])).to(dev)
        return m.sdf_decode_rows(args[0], ri, *args[1:]).cpu(), None, None
    prev = m.set_option(_lib.OPT_SDF_TRAIN_SPLITK, case[4])
    try:
        sdf, saved = m.sdf_decode_train(*args)
        grads = m.sdf_backward(saved, inputs(case, kind)["gsdf"].reshape(case[3]).to(dev))
        pattern = [p.cpu() for p in device_pattern(saved, case[1])]
    finally:
        m.set_option(_lib.OPT_SDF_TRAIN_SPLITK, prev)
    return sdf.cpu().reshape(-1), tuple(v.cpu() for v in grads), pattern


def check_cases(cases, mode, dev, exe, models=None, outs=None, x2=False):
    """run `cases` (of any decoders) in this process, which must be in arithmetic mode `mode`; x2: under LS_OPT_SDF_BF16X2 = 1
    -> ({kernel chain [figure]: (max err / e32, its case and kind)}, [what failed]); outs (a dict) receives {(case key, kind): run_case's output};
    models (a dict) keeps the handles {(decoder, dead0): HipModel} open for the caller"""
    from livingscenes_amd import _lib
    own = models is None
    models = {} if own else models
    table, bad, flips = {}, [], [0]
    try:
        for case, gemms in zip(cases, planned(cases, mode, exe, x2)):
            for kind in KINDS:
                mk = (case[1], kind == "dead0")
                if mk not in models:
                    models[mk] = make_model(case[1], dev, kind == "dead0")
                prev = models[mk].set_option(_lib.OPT_SDF_BF16X2, int(x2))
                try:
                    out = run_case(models[mk], case, kind, dev)
                finally:
                    models[mk].set_option(_lib.OPT_SDF_BF16X2, prev)
                if outs is not None:
                    outs[(case[0], kind)] = out
                ref, e32 = reference(case, kind)
                if out[1] is not None:
                    on_pattern, flipped, wrong = reference_on_pattern(case, kind, out[2])
                    ref = (ref[0], on_pattern)
                    flips[0] += flipped
                    if wrong:
                        bad.append(f"{case[0]} {kind}: {wrong} units of the kept activations are on the wrong side of zero by more than {TOL:.0e} of their row")
                if not float(ref[0].abs().max()) < SDF_MAX:
                    bad.append(f"{case[0]} {kind}: precondition max |ref sdf| = {float(ref[0].abs().max()):.3f} < {SDF_MAX} does not hold")
                for fig, err in _figures(out, ref, inputs(case, kind)["gsdf"], counts_of(case)).items():
                    e = e32[fig]
                    if not e < E32_MAX:
                        bad.append(f"{case[0]} {kind} [{fig}]: precondition e32 = {e:.3e} < {E32_MAX:.0e} does not hold (ill-conditioned input)")
                    limit = bound(e) if not x2 else (TOL if fig == "sdf" else float("inf"))
                    if not err <= limit:
                        bad.append(f"{case[0]} {kind} [{fig}]: err {err:.3e} > bound {limit:.3e} (e32 {e:.3e}, err / e32 {err / max(e, E32_FLOOR):.1f})")
                    label, r = f"{chain_label(case, gemms)} [{fig}]", err / max(e, E32_FLOOR)
                    if r > table.get(label, (-1.0, ""))[0]:
                        table[label] = (r, f"{case[0]} {kind}")
    finally:
        if own:
            for m in models.values():
                m.close()
    if flips[0]:
        table["units the device counts on the other side of zero than float64, all within the tolerance"] = (float(flips[0]), "a count, all cases")
    return table, bad


if __name__ == "__main__":
    import tempfile
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", choices=MODES, required=True, help="run every ladder under the rule; the process must be in that arithmetic mode")
    ap.add_argument("--refs", help="references saved by save_references() in another process")
    a = ap.parse_args()
    assert a.check == own_mode(), f"LS_GEMM_MODE says {own_mode()}, --check {a.check}"
    import torch
    if a.refs:
        load_references(a.refs)
    assert torch.cuda.is_available(), "needs a HIP device"
    bad = []
    with tempfile.TemporaryDirectory(prefix="ls_gemm_plan_") as tmp:
        exe = compile_plan_dump(tmp)
        for dec in DECODERS:                                    # one decoder's handles at a time
            table, b = check_cases(ladder(dec), a.check, torch.device("cuda:0"), exe)
            bad += b
            print(f"mode {a.check}, {dec}: largest err / e32 per kernel chain\n{format_table(table)}")
    print(f"{len(bad)} failures" + "".join("\n  " + b for b in bad[:40]))
    sys.exit(1 if bad else 0)
