"""Every edge-conv kernel against a float64 layer oracle at its size edges: the case ladder, its inputs and the comparison rule.

    python tests/tools/edge_vs_float64.py --check MODE [--refs FILE]    (GPU; the process must be in arithmetic mode MODE: LS_GEMM_MODE unset /
                                                                         bf16x3 / fp32; FILE: references another process saved, else computed)
It runs the whole ladder under the rule below, prints the largest err / e32 per kernel and exits non-zero with the failing keys.

ladder() is the one statement of the cases, shared by tests/test_edge_plan_cpu.py (what the plan launches for them: every EdgeKernel enumerator
in the default mode, a table kernel in the other two), tests/test_edge_oracle_cpu.py (the precondition on the inputs) and
tests/test_hip_edge_layers_f64.py (the comparison).  A case is one HipModel.edgeconv call: a model, a layer, (B, Ns, Nd, rows) and the options
LS_OPT_EDGE_FUSE_Q / _T; it runs on four kinds of input (KINDS).  `rows` goes to any layer >= 1, also where the model's own schedule never
down-samples.

The rule.  err = max over the destination points of max |out - ref| over the point's 3 x Co block / max |ref| over the same block
(edge_oracle.per_point_err), ref = edge_oracle.layer(..., float64).  The bound of a case is MARGIN x e32, e32 the same error of
edge_oracle.layer(..., float32) on the same inputs, computed on the CPU: the reference measures itself, never the code under test.
MARGIN = 16 is what tests/test_hip_range.py gives the split GEMM over an fp32 unit (22-bit products, another summation order); the bound
is never looser than the project's TOL = 1e-4, and e32 < E32_MAX = 1e-5 is a precondition of every input (an input that breaks it is
ill-conditioned and has to be replaced, not excused)."""
import argparse
import binascii
import os
import subprocess
import sys

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
for p in (REPO, os.path.join(REPO, "tests"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

MODES = ("f16", "bf16x3", "fp32")
KINDS = ("randn", "scaled", "dups", "zero")
MARGIN, TOL, E32_MAX = 16.0, 1e-4, 1e-5
FIELDS = ("mode", "attn", "Cin", "Co", "head_c", "B", "Ns", "Nd", "has_rows", "fuse_q", "fuse_t", "want_rowmax", "want_colsum")


def model_cfg(which):
    """the encoder configuration of a ladder model: 'released', 'small', 'pool64' / 'pool96' (small with feat_dim[1] = 64 / 96, as
    record_gemm_launches.model_cfgs), 'attn96' (small with feat_dim = [32, 32, 96, 64]: the generic attention kernel with six heads and a
    half-filled second 64-channel chunk)"""
    from livingscenes_amd import synth
    if which == "released":
        return synth.default_encoder_cfg()
    cfg = synth.small_encoder_cfg()
    if which.startswith("pool"):
        cfg["feat_dim"] = [32, int(which[4:]), 32, 64]
    elif which == "attn96":
        cfg["feat_dim"] = [32, 32, 96, 64]
    else:
        assert which == "small", which
    return cfg


REDUCED = (("ft256", 32), ("ft128", 128), ("fq", 64), ("fq", 72))   # (schedule, N) of the encodes that hold the kernels' side products


def reduced_cfg(name):
    """Small-config schedules (c_dim = 32) in which every layer >= 2 is a kernel that hands row maxima and partial column sums to the residual
    global conv: 'ft256' (no down-sampling, N = 32: layer 2 = FT_256 after a generic POOL at Co = 256), 'ft128' (layer 2 selects 32 of 128
    points: FT_128 after POOL at Co = 128), 'fq' (layers 2 - 4 = ATTN_FQ_16_32 / 16_64 / 32_64, or ATTN_V4_16 / 16 / 32 with LS_OPT_EDGE_FUSE_Q = 0;
    N = 64: Nd = 32 / 32 / 16, column sums written; N = 72: Nd = 36 / 36 / 18, none)"""
    from livingscenes_amd import synth
    cfg = synth.small_encoder_cfg()
    if name == "ft256":
        cfg.update(num_layers=3, feat_dim=[32, 256, 512], down_sample_layers=[], down_sample_factor=[])
    elif name == "ft128":
        cfg.update(num_layers=3, feat_dim=[32, 128, 256], down_sample_layers=[2], down_sample_factor=[4])
    else:
        assert name == "fq", name
        cfg.update(num_layers=5, feat_dim=[32, 32, 64, 64, 128], down_sample_layers=[2, 4], down_sample_factor=[2, 2])
    return cfg


def ladder():
    """[(key, model, layer, (B, Ns, Nd, rows), {option: value})].  B = 3 unless a shape says otherwise."""
    R, N = 1, 0
    l0 = [(3, 16, 16, N), (3, 37, 37, N)]
    pool = [(3, 16, 16, N), (3, 37, 37, N), (3, 70, 35, R), (1, 16, 1, R)]
    generic = [(3, 70, 35, R), (3, 35, 35, N), (1, 16, 1, R)]
    attn = [(3, 70, 35, R), (3, 35, 35, N), (3, 66, 17, R), (3, 16, 16, N), (1, 16, 1, R)]
    l5 = [(1, 128, 32, R), (3, 128, 32, R), (3, 124, 31, R), (3, 32, 32, N)]
    l6 = [(1, 32, 32, N), (3, 32, 32, N), (3, 31, 31, N), (3, 17, 17, N), (3, 128, 32, R)]
    plan = [("released", 0, l0, None), ("small", 0, l0, None),
            ("released", 1, pool, None), ("pool64", 1, pool, None), ("pool96", 1, pool, None),
            ("small", 2, generic, None), ("attn96", 2, generic, None),
            ("released", 2, attn, "OPT_EDGE_FUSE_Q"), ("released", 3, attn, "OPT_EDGE_FUSE_Q"), ("released", 4, attn, "OPT_EDGE_FUSE_Q"),
            ("small", 3, attn, "OPT_EDGE_FUSE_Q"),
            ("released", 5, l5, "OPT_EDGE_FUSE_T"), ("released", 6, l6, "OPT_EDGE_FUSE_T")]
    c = []
    for model, i, shapes, opt in plan:
        for B, Ns, Nd, rows in shapes:
            for v in ((None,) if opt is None else (0, 1)):
                o = {} if opt is None else {opt: v}
                tag = "".join(f", {k[4:].lower()}={x}" for k, x in o.items())
                c.append((f"edgeconv({model}, layer={i}, B={B}, Ns={Ns}, Nd={Nd}, rows={rows}{tag})", model, i, (B, Ns, Nd, rows), o))
    return c


def groups():
    """[(model, layer)] in ladder order: the parametrisation of the GPU test"""
    out = []
    for _, model, i, _, _ in ladder():
        if (model, i) not in out:
            out.append((model, i))
    return out


def kinds_of(B):
    """'zero' and the instance-wise scalings need the three instances"""
    return KINDS if B == 3 else ("randn", "scaled", "dups")


def traits(case, mode):
    """EdgeTraits (csrc/edge_plan.h) of a ladder case of layer >= 1, as record_gemm_launches.edge_traits states them for an export call"""
    import record_gemm_launches as rec
    _, model, i, (B, Ns, Nd, rows), o = case
    return rec.edge_traits(model_cfg(model), mode, i, B, Ns, Nd, rows, o.get("OPT_EDGE_FUSE_Q", 1), o.get("OPT_EDGE_FUSE_T", 1))


def planned_kernels(cases, mode, exe):
    """the gather kernel the plan names for each case (layer 0: edge_l0_kernel, which no plan chooses), through the compiled edge_plan_dump"""
    rest = [c for c in cases if c[2] >= 1]
    lines = [" ".join(str(int(traits(c, mode)[f])) for f in FIELDS) for c in rest]
    out = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(lines)
    names = {c[0]: l.split(" # ")[0].split(";")[-1].split("|")[0] for c, l in zip(rest, out)}
    return [names.get(c[0], "ls::edge_l0_kernel") for c in cases]


def compile_plan_dump(outdir):
    exe = os.path.join(str(outdir), "edge_plan_dump")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-I", os.path.join(REPO, "livingscenes_amd", "csrc"),
                    os.path.join(REPO, "tests", "tools", "edge_plan_dump.cpp"), "-o", exe], check=True)
    return exe


# ------------------------------------------------------------------------------------------------ inputs and references (CPU)
_WEIGHTS, _INPUTS, _REFS = {}, {}, {}


def weights(model):
    from livingscenes_amd import synth
    if model not in _WEIGHTS:
        cfg = model_cfg(model)
        _WEIGHTS[model] = (cfg, synth.make_encoder_weights(cfg, 0))
    return _WEIGHTS[model]


def shape_key(case):
    _, model, i, (B, Ns, Nd, rows), _ = case
    return f"{model}:{i}:{B}:{Ns}:{Nd}:{rows}"


def inputs(case, kind):
    """-> (src_f [B,Cin,3,Ns] float32 in the oracle's layout, knn [B,Nd,16] int64, rows [B,Nd] int64 or None).  The generator is seeded from the
    case's shape key (not its options, not the kind: 'zero' is 'randn' with instance 1 zeroed, so that the other instances can be compared bit
    for bit); neighbour lists are random 16-subsets of the Ns source rows, rows a random Nd-subset."""
    import torch
    sk = shape_key(case)
    if (sk, kind) in _INPUTS:
        return _INPUTS[(sk, kind)]
    _, model, i, (B, Ns, Nd, has_rows), _ = case
    cfg, _ = weights(model)
    Cin = 1 if i == 0 else cfg["feat_dim"][i - 1]
    g = torch.Generator().manual_seed(binascii.crc32(sk.encode()))
    src = torch.randn(B, Cin, 3, Ns, generator=g)
    knn = torch.stack([torch.stack([torch.randperm(Ns, generator=g)[:16] for _ in range(Nd)]) for _ in range(B)])
    rows = torch.stack([torch.randperm(Ns, generator=g)[:Nd] for _ in range(B)]) if has_rows else None
    if kind == "scaled":
        src[0] *= 2.0 ** -17
        if B == 3:
            src[2] *= 2.0 ** 14
            src[1, :4] *= 1e3
    elif kind == "dups":
        knn[..., 0] = rows if has_rows else torch.arange(Nd).expand(B, Nd)
        knn[..., 8:] = knn[..., :8].clone()
        if i == 0:
            src[:, :, :, 3] = 0.0                       # one point exactly at the origin
            src[:, :, :, 7] = src[:, :, :, 5]           # two points coincide
    elif kind == "zero":
        assert B == 3
        src[1] = 0.0
    else:
        assert kind == "randn", kind
    _INPUTS[(sk, kind)] = (src, knn, rows)
    return _INPUTS[(sk, kind)]


def reference(case, kind):
    """-> (ref float64 [B,Co,3,Nd], e32): the float64 oracle and the per-point error of the float32 oracle against it"""
    import torch
    import edge_oracle
    sk = shape_key(case)
    if (sk, kind) not in _REFS:
        cfg, w = weights(case[1])
        src, knn, rows = inputs(case, kind)
        ref = edge_oracle.layer(w, cfg, case[2], src, knn, rows, torch.float64)
        e32 = edge_oracle.per_point_err(edge_oracle.layer(w, cfg, case[2], src, knn, rows, torch.float32), ref)
        _REFS[(sk, kind)] = (ref, e32)
    return _REFS[(sk, kind)]


def save_references(path):
    """what reference() has computed so far in this process -> a file for a child process in another arithmetic mode (the inputs, hence the
    references, do not depend on the mode; a missing entry is computed where it is needed)"""
    import torch
    torch.save({f"{sk}|{kind}": v for (sk, kind), v in _REFS.items()}, path)


def load_references(path):
    import torch
    for k, v in torch.load(path).items():
        _REFS[tuple(k.split("|"))] = v


def bound(e32):
    return min(MARGIN * e32, TOL)


# ------------------------------------------------------------------------------------------------ the device side
def rows_layout(f):
    """the oracle's [B,C,3,N] -> the library's [B,N,3,C]"""
    return f.permute(0, 3, 2, 1).contiguous()


def make_model(model, dev):
    from livingscenes_amd import ops, packing
    cfg, w = weights(model)
    desc, blob = packing.pack_model(w, cfg, None, None)
    return ops.HipModel(desc, blob, dev)


def run_case(m, case, kind, dev):
    """one HipModel.edgeconv call under the case's options -> the output in the oracle's layout [B,Co,3,Nd], on the CPU"""
    import torch
    from livingscenes_amd import _lib
    _, _, i, (B, Ns, Nd, _), o = case
    src, knn, rows = inputs(case, kind)
    s = rows_layout(src).to(dev)
    if i == 0:
        s = s.reshape(B, Ns, 3)
    prev = {k: m.set_option(getattr(_lib, k), v) for k, v in o.items()}
    try:
        out = m.edgeconv(i, s, knn.to(torch.int32).to(dev), None if rows is None else rows.to(torch.int32).to(dev))
    finally:
        for k, v in prev.items():
            m.set_option(getattr(_lib, k), v)
    return out.permute(0, 3, 2, 1).cpu()


def check_case(m, case, dev):
    """-> ({kind: (err, e32)} of the three compared kinds, [what failed]) of one case"""
    import torch
    import edge_oracle
    B = case[3][0]
    figs, bad, outs = {}, [], {}
    for kind in kinds_of(B):
        out = outs[kind] = run_case(m, case, kind, dev)
        if kind == "zero":
            # as both oracles give: the zero instance's message is exactly 0; the other two do not notice it
            if not (out[1] == 0).all():
                bad.append(f"{case[0]} zero: {int((out[1] != 0).sum())} floats of the zero instance's output are not 0")
            if not (torch.equal(out[0], outs["randn"][0]) and torch.equal(out[2], outs["randn"][2])):
                bad.append(f"{case[0]} zero: the other instances differ from the call without the zeroing")
            continue
        ref, e32 = reference(case, kind)
        err = edge_oracle.per_point_err(out, ref)
        figs[kind] = (err, e32)
        if not e32 < E32_MAX:
            bad.append(f"{case[0]} {kind}: precondition e32 = {e32:.3e} < {E32_MAX:.0e} does not hold (ill-conditioned input)")
        if not err <= bound(e32):
            bad.append(f"{case[0]} {kind}: err {err:.3e} > bound {bound(e32):.3e} (e32 {e32:.3e}, err / e32 {err / max(e32, 1e-300):.1f})")
    return figs, bad


def check_cases(cases, mode, dev, exe, models=None):
    """run `cases` in this process (which must be in arithmetic mode `mode`) -> ({kernel: (max err / e32, its case and kind)}, [what failed])"""
    own = models is None
    models = {} if own else models
    table, bad = {}, []
    try:
        for case, kernel in zip(cases, planned_kernels(cases, mode, exe)):
            if case[1] not in models:
                models[case[1]] = make_model(case[1], dev)
            figs, b = check_case(models[case[1]], case, dev)
            bad += b
            for kind, (err, e32) in figs.items():
                r = err / max(e32, 1e-300)
                if r > table.get(kernel, (-1.0, ""))[0]:
                    table[kernel] = (r, f"{case[0]} {kind}")
    finally:
        if own:
            for m in models.values():
                m.close()
    return table, bad


def format_table(table):
    return "\n".join(f"  {k:<36s} max err / e32 = {r:7.2f}   ({where})" for k, (r, where) in sorted(table.items()))


def own_mode():
    return os.environ.get("LS_GEMM_MODE") if os.environ.get("LS_GEMM_MODE") in MODES[1:] else MODES[0]


if __name__ == "__main__":
    import tempfile
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", choices=MODES, required=True, help="run the whole ladder under the rule; the process must be in that arithmetic mode")
    ap.add_argument("--refs", help="references saved by save_references() in another process")
    a = ap.parse_args()
    assert a.check == own_mode(), f"LS_GEMM_MODE says {own_mode()}, --check {a.check}"
    import torch
    if a.refs:
        load_references(a.refs)
    assert torch.cuda.is_available(), "needs a HIP device"
    with tempfile.TemporaryDirectory(prefix="ls_edge_plan_") as tmp:
        table, bad = check_cases(ladder(), a.check, torch.device("cuda:0"), compile_plan_dump(tmp))
    print(f"mode {a.check}: largest err / e32 per kernel\n{format_table(table)}")
    print(f"{len(bad)} failures" + "".join("\n  " + b for b in bad[:40]))
    sys.exit(1 if bad else 0)
