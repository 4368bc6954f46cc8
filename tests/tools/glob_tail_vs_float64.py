"""The residual global conv and the encoder tail against float64 oracles at their size edges: the case ladders, their inputs and the rule.

    python tests/tools/glob_tail_vs_float64.py --check MODE [--refs FILE]    (GPU; the process must be in arithmetic mode MODE: LS_GEMM_MODE unset /
                                                                              bf16x3 / fp32; FILE: references another process saved, else computed)
It runs both ladders under the rule below, prints the largest err / e32 per planned kernel chain and exits non-zero with the failing keys.

gc_ladder() / tail_ladder() are the one statement of the cases, shared by tests/test_glob_tail_oracle_cpu.py (the precondition on the inputs,
which kernels the plan launches for them) and tests/test_hip_glob_tail_f64.py (the comparison, the exact relations).
  a global-conv case   one HipModel.vn_lna_global call: (model, layer, B, N, LS_OPT_GLOB_FUSE 0 / 1 / 2).  Models: 'released' (Co = 64, 64, 128, 256,
                       512 at layers 2 .. 6), 'small' (layer 2: Co = 32) and 'attn96' (layer 2: Co = 96) -- gemm_vn_plan names no kernel for the
                       last two, so the unfused path runs whatever the option says, at K = 32 and K = 96.  Shapes: N = 1, N on both sides of the
                       16 row slices of the two mean kernels and of the 40-point tile of the VN kernels; at 64 channels 3 B N / 120 = 15 | 16
                       (tiled | persistent), M = 3 B N = 1536 and N % 8 (streaming with LS_OPT_GLOB_FUSE = 2)
  a tail case          one HipModel.encoder_tail call: (configuration, B, NP, with the encode epilogue or without).  The configuration is the small
                       one with feat_dim[-1] = Cl, c_dim, center_pred, center_pred_scale: c_dim % 4 != 0 (tail_gemv3's scalar path), c_dim > 256
                       (second trips of tail_kernel's loops), c_dim > ~840 (dynamic LDS above 64 KB), pad4(c_dim + 1) on both sides of a multiple
                       of 4, Cl = 512 (conv_c splits K)
Every case runs on four kinds of input (KINDS), seeded from the case's shape key.

The rule.  Global conv: err = edge_oracle.per_point_err against glob_tail_oracle.global_conv(..., float64).  Tail: err =
glob_tail_oracle.per_instance_err over z_so3, z_inv, s, t against glob_tail_oracle.tail(..., float64) (with the epilogue: s = scale0 * scale,
t = center + centroid, formed in the oracle's type).  err <= min(MARGIN x e32, TOL), e32 the same error of the float32 oracle on the same inputs,
computed on the CPU; e32 < E32_MAX is a precondition of every input.  The margin and both caps are tests/tools/edge_vs_float64.py's."""
import argparse
import binascii
import os
import subprocess
import sys

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
for p in (REPO, os.path.join(REPO, "tests"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

from edge_vs_float64 import E32_MAX, MARGIN, MODES, TOL, bound, model_cfg, own_mode, rows_layout  # noqa: E402

KINDS = ("randn", "scaled", "zero", "chan")
SCALES = (2.0 ** -6, 1.0, 2.0 ** 5)        # 'scaled': instance b times SCALES[b]
# the input line of tests/tools/gemm_plan_dump.cpp after `mode form` (tests/test_gemm_plan_cpu.py: FIELDS)
PLAN_FIELDS = ("M", "N", "K", "lda", "ldw", "pieces", "gather", "masked", "may_split", "latency", "has_planes", "wants_out_rowmax", "C", "npts", "has_G_or_cs",
               "a_parts", "has_a_rowmax", "has_w_rowmax")
# Shapes whose inputs were replaced (the suffix goes into the seed).  e32 is a property of the host's float32 BLAS as much as of the input: at the
# wide layers one point whose 3 x Co block nearly cancels decides it, and two hosts differed by 10 - 20 %.  The first inputs of three of these
# shapes broke the precondition (e32 = 1.3e-5, 4.6e-5, 1.3e-5) and one came within 20 % of it; the seeds below are the first with e32 < 5.5e-6
# on every kind, so that the precondition does not hang on the host.
RESEED = {"gc:released:5:3:15": "#1", "gc:released:6:3:17": "#1", "gc:released:6:3:40": "#4", "gc:released:6:3:41": "#2"}


def kinds_of(B):
    """'zero' needs an instance beside the zeroed one"""
    return KINDS if B == 3 else tuple(k for k in KINDS if k != "zero")


# ------------------------------------------------------------------------------------------------ the ladders
GC_MODELS = (("released", 2), ("released", 3), ("released", 4), ("released", 5), ("released", 6), ("small", 2), ("attn96", 2))


def gc_ladder():
    """[(key, model, layer, (B, N), glob_fuse)]"""
    every = [(1, 1), (3, 7), (3, 15), (3, 17), (3, 39), (3, 40), (3, 41)]
    # 64 channels: tm = 15 tiled | tm = 16 persistent, a partial tile, N % 8 != 0 | streaming with glob_fuse = 2 | M = 1536 exactly | M = 1512, N % 8 == 0
    wide = [(1, 600), (1, 601), (1, 608), (2, 256), (1, 504)]
    c = []
    for model, i in GC_MODELS:
        Co = model_cfg(model)["feat_dim"][i]
        for B, N in every + (wide if Co == 64 else []):
            assert Co < 256 or N <= 41
            for gf in (0, 1, 2):
                c.append((f"global_conv({model}, layer={i}, B={B}, N={N}, glob_fuse={gf})", model, i, (B, N), gf))
    return c


TAIL_DIMS = ((2, 64), (6, 64), (30, 64), (32, 64), (254, 64), (256, 512), (258, 64), (1022, 64), (1024, 512))     # (c_dim, Cl)
TAIL_NP = (1, 2, 33, 257)


def tail_cfgs():
    """[(name, c_dim, Cl, center_pred, center_pred_scale)]"""
    out = []
    for cd, Cl in TAIL_DIMS:
        for cp, cps in ((True, True), (True, False), (False, False)):
            if (cp, cps) == (True, True) or cd in (6, 256, 1024):
                out.append((f"c{cd}-l{Cl}-center{int(cp)}{int(cps)}", cd, Cl, cp, cps))
    return out


def tail_cfg(name):
    from livingscenes_amd import synth
    _, cd, Cl, cp, cps = next(t for t in tail_cfgs() if t[0] == name)
    cfg = synth.small_encoder_cfg()
    cfg["feat_dim"] = cfg["feat_dim"][:-1] + [Cl]
    cfg.update(c_dim=cd, center_pred=cp, center_pred_scale=cps)
    return cfg


def tail_ladder():
    """[(key, cfg name, (B, NP), with_epilogue)]: B = 3 at every NP, B = 1 once per configuration (NP = 1: conv_c on M = 3 rows)"""
    c = []
    for name, *_ in tail_cfgs():
        for B, NP in [(3, n) for n in TAIL_NP] + [(1, 1)]:
            for epi in (0, 1):
                c.append((f"tail({name}, B={B}, NP={NP}, epilogue={epi})", name, (B, NP), epi))
    return c


# ------------------------------------------------------------------------------------------------ what the plan launches (CPU)
def compile_plan_dump(outdir):
    exe = os.path.join(str(outdir), "gemm_plan_dump")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(REPO, "livingscenes_amd", "csrc"),
                    os.path.join(REPO, "tests", "tools", "gemm_plan_dump.cpp"), "-o", exe], check=True)
    return exe


def _plan(exe, mode, traits):
    """[GemmTraits as record_gemm_launches.mm / vn state them] -> [[kernel name, ...] per problem] (a split launch: the kernel and its reduce)"""
    if not traits:
        return []
    lines = [" ".join(str(int(v)) for v in [MODES.index(mode), t["form"] == "vn"] + [t.get(f, 0) for f in PLAN_FIELDS]) for t in traits]
    out = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(lines)
    return [[launch.split("|")[0] for launch in l.split(";")] for l in out]


def gc_traits(case, fused):
    """the GemmTraits model.hip: global_conv builds for a case: fused -> the one VN problem (the export hands over exact row maxima, one part,
    with LS_OPT_GLOB_FUSE = 2 only; G is always given); else the per-point GEMM and the 3B-row latency GEMM, both with the split-K scratch"""
    import record_gemm_launches as rec
    _, model, i, (B, N), gf = case
    Co = model_cfg(model)["feat_dim"][i]
    if fused:
        return [rec.vn(3 * B * N, Co, Co, N, a_parts=int(gf == 2), has_a_rowmax=int(gf == 2))]
    return [rec.mm(3 * B * N, 2 * Co, Co, may_split=1, has_planes=int(Co >= 512 and Co % 32 == 0)), rec.mm(3 * B, 4 * Co, Co, may_split=1, latency=1)]


def gc_planned(cases, mode, exe):
    """-> [[kernel name, ...]] per case, in launch order: glob_mean_gemv_kernel + a VN kernel where LS_OPT_GLOB_FUSE != 0, the mode is the default
    and gemm_vn_plan names a kernel; else mean_points_kernel, the two GEMMs (with their reduces) and vn_act_rows_kernel"""
    try_fused = [c for c in cases if c[4] != 0 and mode == MODES[0]]
    vn = dict(zip((c[0] for c in try_fused), _plan(exe, mode, [gc_traits(c, True)[0] for c in try_fused])))
    unfused = [c for c in cases if vn.get(c[0], ["none"]) == ["none"]]
    mm = _plan(exe, mode, [t for c in unfused for t in gc_traits(c, False)])
    chains = {c[0]: ["ls::mean_points_kernel"] + mm[2 * n] + mm[2 * n + 1] + ["ls::vn_act_rows_kernel"] for n, c in enumerate(unfused)}
    return [chains[c[0]] if c[0] in chains else ["ls::glob_mean_gemv_kernel"] + vn[c[0]] for c in cases]


def tail_traits(case):
    import record_gemm_launches as rec
    _, name, (B, NP), _ = case
    cfg = tail_cfg(name)
    Cl, Cdp = cfg["feat_dim"][-1], (cfg["c_dim"] + 1 + 3) // 4 * 4
    return [rec.mm(3 * B * NP, Cdp, Cl, may_split=1, has_planes=int(Cl >= 512 and Cl % 32 == 0))]


def tail_planned(cases, mode, exe):
    return [p + ["ls::tail_kernel"] for p in _plan(exe, mode, [tail_traits(c)[0] for c in cases])]


def chain_label(names):
    return " + ".join(n[4:] if n.startswith("ls::") else n for n in names)


# ------------------------------------------------------------------------------------------------ inputs and references (CPU)
_WEIGHTS, _INPUTS, _REFS = {}, {}, {}


def weights(model):
    """(cfg, weights) of a global-conv model or of a tail configuration, seed 0"""
    from livingscenes_amd import synth
    if model not in _WEIGHTS:
        cfg = tail_cfg(model) if any(model == t[0] for t in tail_cfgs()) else model_cfg(model)
        _WEIGHTS[model] = (cfg, synth.make_encoder_weights(cfg, 0))
    return _WEIGHTS[model]


def gc_shape_key(case):
    _, model, i, (B, N), _ = case
    return f"gc:{model}:{i}:{B}:{N}"


def tail_shape_key(case):
    """the features depend on the last layer's width only: configurations of one Cl see the same clouds"""
    _, name, (B, NP), _ = case
    return f"tail:{tail_cfg(name)['feat_dim'][-1]}:{B}:{NP}"


def _features(sk, kind, B, C, N):
    """[B,C,3,N] float32 in the oracle's layout.  The generator is seeded from the shape key; every kind is 'randn' transformed: 'scaled' = the
    instances times 2^-6, 1, 2^5; 'zero' = instance 1 all zero; 'chan' = the first C / 8 channels times 1e4 and the first N / 4 points times 1e-6"""
    import torch
    g = torch.Generator().manual_seed(binascii.crc32((sk + RESEED.get(sk, "")).encode()))
    f = torch.randn(B, C, 3, N, generator=g)
    if kind == "scaled":
        f *= torch.tensor(SCALES[:B])[:, None, None, None]
    elif kind == "zero":
        assert B == 3
        f[1] = 0.0
    elif kind == "chan":
        f[:, :C // 8] *= 1e4
        f[..., :N // 4] *= 1e-6
    else:
        assert kind == "randn", kind
    return f, g


def gc_inputs(case, kind):
    sk = gc_shape_key(case)
    if (sk, kind) not in _INPUTS:
        _, model, i, (B, N), _ = case
        _INPUTS[(sk, kind)] = _features(sk, kind, B, weights(model)[0]["feat_dim"][i], N)[0]
    return _INPUTS[(sk, kind)]


def tail_inputs(case, kind):
    """-> (f [B,Cl,3,NP], centroid [B,3], scale0 [B] in [0.5, 1.5)); the last two are used by the cases with the epilogue"""
    import torch
    sk = tail_shape_key(case)
    if (sk, kind) not in _INPUTS:
        _, name, (B, NP), _ = case
        f, g = _features(sk, kind, B, weights(name)[0]["feat_dim"][-1], NP)
        _INPUTS[(sk, kind)] = (f, torch.randn(B, 3, generator=g), 0.5 + torch.rand(B, generator=g))
    return _INPUTS[(sk, kind)]


def gc_reference(case, kind):
    """-> (ref float64 [B,Co,3,N], e32)"""
    import torch
    import glob_tail_oracle as gto
    k = (gc_shape_key(case), kind)
    if k not in _REFS:
        cfg, w = weights(case[1])
        msg = gc_inputs(case, kind)
        ref = gto.global_conv(w, cfg, case[2], msg, torch.float64)
        _REFS[k] = (ref, gto.per_point_err(gto.global_conv(w, cfg, case[2], msg, torch.float32), ref))
    return _REFS[k]


def _with_epilogue(o, centroid, scale0):
    """model_utils.py:182-195 on the oracle's (z_so3, z_inv, scale, center), in the oracle's type -> (z_so3, z_inv, s, t [B,3])"""
    z_so3, z_inv, scale, center = o
    return z_so3, z_inv, scale0.to(scale.dtype) * scale, center.reshape(-1, 3) + centroid.to(center.dtype)


def tail_reference(case, kind):
    """-> ((z_so3, z_inv, s, t) float64, e32)"""
    import torch
    import glob_tail_oracle as gto
    _, name, _, epi = case
    sk = tail_shape_key(case)
    k0 = (f"{sk}:{name}", kind)                      # the oracle's outputs, shared by the case with and the case without the epilogue
    if k0 not in _REFS:
        cfg, w = weights(name)
        f = tail_inputs(case, kind)[0]
        _REFS[k0] = (gto.tail(w, cfg, f, torch.float64), gto.tail(w, cfg, f, torch.float32))
    k = (f"{sk}:{name}:{epi}", kind)
    if k not in _REFS:
        _, centroid, scale0 = tail_inputs(case, kind)
        if not epi:
            centroid, scale0 = torch.zeros_like(centroid), torch.ones_like(scale0)
        ref, r32 = (_with_epilogue(o, centroid, scale0) for o in _REFS[k0])
        _REFS[k] = (ref, gto.per_instance_err(r32, ref))
    return _REFS[k]


def all_references():
    """every reference of both ladders (those already there are kept) -> the largest e32 of the global conv, of the tail"""
    worst = [0.0, 0.0]
    for n, (lad, fn) in enumerate(((gc_ladder(), gc_reference), (tail_ladder(), tail_reference))):
        for case in lad:
            for kind in kinds_of(case[-2][0]):
                worst[n] = max(worst[n], fn(case, kind)[1])
    return tuple(worst)


def save_references(path):
    """what the two reference functions have computed so far in this process -> a file for a child process in another arithmetic mode (the
    inputs, hence the references, do not depend on the mode; a missing entry is computed where it is needed)"""
    import torch
    torch.save({f"{a}|{kind}": v for (a, kind), v in _REFS.items()}, path)


def load_references(path):
    import torch
    for k, v in torch.load(path).items():
        _REFS[tuple(k.split("|"))] = v


# ------------------------------------------------------------------------------------------------ the device side
def make_model(model, dev):
    from livingscenes_amd import ops, packing
    cfg, w = weights(model)
    desc, blob = packing.pack_model(w, cfg, None, None)
    return ops.HipModel(desc, blob, dev)


def gc_run(m, case, kind, dev):
    """one HipModel.vn_lna_global call under the case's LS_OPT_GLOB_FUSE -> the output in the oracle's layout [B,Co,3,N], on the CPU"""
    from livingscenes_amd import _lib
    prev = m.set_option(_lib.OPT_GLOB_FUSE, case[4])
    try:
        out = m.vn_lna_global(case[2], rows_layout(gc_inputs(case, kind)).to(dev))
    finally:
        m.set_option(_lib.OPT_GLOB_FUSE, prev)
    return out.permute(0, 3, 2, 1).cpu()


def tail_run(m, case, kind, dev):
    """one HipModel.encoder_tail call -> (z_so3 [B,c,3], z_inv [B,c], s [B], t [B,3]) on the CPU"""
    f, centroid, scale0 = tail_inputs(case, kind)
    args = (centroid.to(dev), scale0.to(dev)) if case[3] else ()
    return tuple(o.cpu() for o in m.encoder_tail(rows_layout(f).to(dev), *args))


def _judge(key, kind, err, e32, bad):
    if not e32 < E32_MAX:
        bad.append(f"{key} {kind}: precondition e32 = {e32:.3e} < {E32_MAX:.0e} does not hold (ill-conditioned input)")
    if not err <= bound(e32):
        bad.append(f"{key} {kind}: err {err:.3e} > bound {bound(e32):.3e} (e32 {e32:.3e}, err / e32 {err / max(e32, 1e-300):.1f})")


def check_cases(family, cases, mode, dev, exe, models=None, outs=None):
    """run `cases` of one ladder (family 'gc' / 'tail') in this process, which must be in arithmetic mode `mode`
    -> ({kernel chain: (max err / e32, its case and kind)}, [what failed]); outs (a dict) receives {(case key, kind): the output}"""
    import glob_tail_oracle as gto
    planned, run, reference, err_of = ((gc_planned, gc_run, gc_reference, gto.per_point_err) if family == "gc" else
                                       (tail_planned, tail_run, tail_reference, gto.per_instance_err))
    own = models is None
    models = {} if own else models
    table, bad = {}, []
    try:
        for case, chain in zip(cases, planned(cases, mode, exe)):
            if case[1] not in models:
                models[case[1]] = make_model(case[1], dev)
            for kind in kinds_of(case[-2][0]):
                out = run(models[case[1]], case, kind, dev)
                if outs is not None:
                    outs[(case[0], kind)] = out
                ref, e32 = reference(case, kind)
                err = err_of(out, ref)
                _judge(case[0], kind, err, e32, bad)
                r = err / max(e32, 1e-300)
                if r > table.get(chain_label(chain), (-1.0, ""))[0]:
                    table[chain_label(chain)] = (r, f"{case[0]} {kind}")
    finally:
        if own:
            for m in models.values():
                m.close()
    return table, bad


def format_table(table):
    return "\n".join(f"  max err / e32 = {r:7.2f}   {k}   ({where})" for k, (r, where) in sorted(table.items()))


if __name__ == "__main__":
    import tempfile
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", choices=MODES, required=True, help="run both ladders under the rule; the process must be in that arithmetic mode")
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
        for family, lad in (("gc", gc_ladder()), ("tail", tail_ladder())):
            for group in dict.fromkeys(c[1] for c in lad):      # one handle at a time
                table, b = check_cases(family, [c for c in lad if c[1] == group], a.check, torch.device("cuda:0"), exe)
                bad += b
                print(f"mode {a.check}, {family} {group}: largest err / e32 per kernel chain\n{format_table(table)}")
    print(f"{len(bad)} failures" + "".join("\n  " + b for b in bad[:40]))
    sys.exit(1 if bad else 0)
