"""The SDF decoder (HipModel.sdf_decode / sdf_decode_rows / sdf_decode_train: sdf_prep_kernel, sdf_affine_kernel, the decoder GEMMs with their
row-max chain, sdf_out_kernel) and its backward (HipModel.sdf_backward: sdf_out_bwd_kernel, the transposed GEMMs, relu_mask_kernel, the two
sdf_affine_bwd kernels, sdf_code_grad_kernel, sdf_query_grad_kernel) against the float64 oracle tests/sdf_oracle.py at their size edges: a decoder
without a skip, a skip at the last hidden layer, widths 132 / 260 / 64 beside the four decoders the project serves; M = 1, 2, 63 | 64 | 65, 129, 257;
ragged rows with empty instances; rows whose |q| spans fourteen binades, a zeroed instance, an all-zero first operand.  The decoders, their
inputs and the rule are tests/tools/sdf_vs_float64.py: the SDF PER ROW against its instance's largest value, the code / scale / translation
gradients PER INSTANCE and per output, the query gradient per row on the scale of the row's own upstream gradient,
    err <= min(16 x max(e32, 2^-23), 1e-4),
e32 the same figure of the float32 oracle, computed here on the CPU from the same inputs; e32 < 1e-5 and max |sdf| < 0.5 are asserted as
preconditions.  tests/test_sdf_oracle_cpu.py shows which GEMM kernels the ladder reaches.  With the comparison go the exact relations the code
promises: the ragged entry, a shorter call, a single instance and a chunked call return the bits of the dense call; the training forward
without split-K returns the bits of sdf_decode; sdf_backward without the query or without the code gradient returns the bits of the rest."""
import importlib.util
import os
import subprocess
import sys

import pytest
import torch

import sdf_oracle
from livingscenes_amd import _lib

pytestmark = pytest.mark.gpu
TOOL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools", "sdf_vs_float64.py")


def _load():
    spec = importlib.util.spec_from_file_location("sdf_vs_float64", TOOL)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


lad = _load()   # one module object: the float64 references it caches serve every test of this file
DECS = list(lad.DECODERS)


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    return lad.compile_plan_dump(tmp_path_factory.mktemp("gemm_plan"))


@pytest.fixture(scope="module")
def models():
    """{(decoder, dead0): HipModel}, filled by check_cases, shared by the tests of this file"""
    held = {}
    yield held
    for m in held.values():
        m.close()


def _cases(dec, *entries):
    return [c for c in lad.ladder(dec) if c[2] in entries]


def _model(models, dec, kind):
    return models[(dec, kind == "dead0")]


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("dec", DECS)
def test_decode_vs_float64_per_row(dec, plan_exe, models):
    """sdf_decode at every dense shape and sdf_decode_rows at every ragged one, on every kind of input.  Prints the largest err / e32 per kernel
    chain.  Then, on the same outputs and inputs, bit for bit: the ragged rows == each instance decoded alone; the first M rows of the 3 x 129
    call == a call of M rows; an instance inside B = 3 == the instance alone (the arithmetic must not depend on M); a call cut into 64-row
    chunks (max_ws_bytes) == the call in one piece."""
    dev = _dev()
    cases = _cases(dec, "decode", "rows")
    outs = {}
    table, bad = lad.check_cases(cases, lad.own_mode(), dev, plan_exe, models=models, outs=outs)
    print(f"[{dec}, mode {lad.own_mode()}] largest err / e32 per kernel chain\n{lad.format_table(table)}")
    by_shape = {c[3]: c for c in cases}
    for kind in lad.KINDS:
        m = _model(models, dec, kind)
        for case in _cases(dec, "rows"):
            inp, got = lad.inputs(case, kind), outs[(case[0], kind)][0]
            for q, code, _, (r0, r1) in lad.instances(inp, lad.counts_of(case)):
                one = m.sdf_decode(q.to(dev), *[code[k].to(dev) for k in ("z_so3", "z_inv", "s", "t")]).cpu().reshape(-1)
                if not torch.equal(one, got[r0:r1]):
                    bad.append(f"{case[0]} {kind}: rows {r0}:{r1} differ from the instance decoded alone")
        case = by_shape[(3, 129)]
        q, z_so3, z_inv, s, t = lad.device_args(case, kind, dev)
        full = outs[(case[0], kind)][0].reshape(3, 129)
        for M in (1, 2, 63, 64, 65):
            if not torch.equal(m.sdf_decode(q[:, :M].contiguous(), z_so3, z_inv, s, t).cpu(), full[:, :M]):
                bad.append(f"{case[0]} {kind}: the call of M = {M} rows differs from the first {M} rows")
        for b in range(3):
            if not torch.equal(m.sdf_decode(q[b:b + 1].contiguous(), z_so3[b:b + 1], z_inv[b:b + 1], s[b:b + 1], t[b:b + 1]).cpu()[0], full[b]):
                bad.append(f"{case[0]} {kind}: instance {b} alone differs from its rows in the batch")
        case = by_shape.get((1, 257), case)
        chunked = m.sdf_decode(*lad.device_args(case, kind, dev), max_ws_bytes=1).cpu().reshape(-1)
        if not torch.equal(chunked, outs[(case[0], kind)][0]):
            bad.append(f"{case[0]} {kind}: the call in 64-row chunks differs from the call in one piece")
    assert not bad, f"{len(bad)} failures:\n" + "\n".join(bad[:20])


# ------------------------------------------------------------------------------------------------ training forward and backward
@pytest.mark.parametrize("dec", DECS)
def test_train_and_backward_vs_float64(dec, plan_exe, models):
    """sdf_decode_train + sdf_backward at every dense shape, LS_OPT_SDF_TRAIN_SPLITK 1 and 0, on every kind of input: the SDF and all five
    gradients under the rule.  Then bit for bit: the training forward without split-K == sdf_decode; sdf_backward(need_query_grad=False) and
    sdf_backward(need_code_grad=False) return what the full call returned for the outputs they keep, and None for the others."""
    dev = _dev()
    cases = _cases(dec, "train")
    outs = {}
    table, bad = lad.check_cases(cases, lad.own_mode(), dev, plan_exe, models=models, outs=outs)
    print(f"[{dec}, mode {lad.own_mode()}] largest err / e32 per kernel chain\n{lad.format_table(table)}")
    for case in cases:
        for kind in lad.KINDS:
            m = _model(models, dec, kind)
            args = lad.device_args(case, kind, dev)
            sdf, grads, _ = outs[(case[0], kind)]
            if case[4] == 0 and not torch.equal(m.sdf_decode(*args).cpu().reshape(-1), sdf):
                bad.append(f"{case[0]} {kind}: the training forward differs from sdf_decode")
            if kind not in ("rows", "randn"):
                continue
            prev = m.set_option(_lib.OPT_SDF_TRAIN_SPLITK, case[4])
            try:
                sdf2, saved = m.sdf_decode_train(*args)
                gsdf = lad.inputs(case, kind)["gsdf"].reshape(case[3]).to(dev)
                no_q = m.sdf_backward(saved, gsdf, need_query_grad=False)
                no_c = m.sdf_backward(saved, gsdf, need_code_grad=False)
            finally:
                m.set_option(_lib.OPT_SDF_TRAIN_SPLITK, prev)
            if not torch.equal(sdf2.cpu().reshape(-1), sdf):
                bad.append(f"{case[0]} {kind}: a second training forward differs from the first")
            if no_q[0] is not None or no_c[1] is not None or no_c[2] is not None:
                bad.append(f"{case[0]} {kind}: a gradient that was not asked for came back")
            for name, k, got in [(n, k, no_q[k]) for k, n in enumerate(sdf_oracle.GRAD_NAMES) if k > 0] + [(n, k, no_c[k]) for k, n in enumerate(sdf_oracle.GRAD_NAMES) if k in (0, 3, 4)]:
                if got is None or not torch.equal(got.cpu(), grads[k]):
                    bad.append(f"{case[0]} {kind}: grad {name} of the reduced call differs from the full call's")
    assert not bad, f"{len(bad)} failures:\n" + "\n".join(bad[:20])


# ------------------------------------------------------------------------------------------------ the other arithmetic
@pytest.mark.parametrize("dec", DECS)
def test_two_piece_mode_per_row(dec, plan_exe, models):
    """LS_OPT_SDF_BF16X2 = 1 through set_option (two bf16 pieces per operand, 2^-16 per product, no row-max chain): the SDF of every forward
    entry point within the flat 1e-4 that test_sdf_decode_two_piece_mode_stays_inside_the_tolerance asserts on the whole tensor, here per row
    against the instance's largest value.  The gradients are measured and printed with the rest of the err / e32 table."""
    table, bad = lad.check_cases(lad.ladder(dec), lad.own_mode(), _dev(), plan_exe, models=models, x2=True)
    print(f"[{dec}, mode {lad.own_mode()}, two-piece products] largest err / e32 per kernel chain\n{lad.format_table(table)}")
    assert not bad, f"{len(bad)} failures:\n" + "\n".join(bad[:20])


def test_sdf_vs_float64_in_the_other_arithmetic_modes(tmp_path):
    """LS_GEMM_MODE is read once per process: the tests above hold the ladders in this process's mode; here bf16x3 / fp32 (or the default) once
    each in a fresh child under a time limit (tests/tools/sdf_vs_float64.py --check MODE; the float64 references, computed here on the CPU where
    the tests above have not left them, are handed over in a file).  The children run one after the other; a child that dies of a signal or runs
    out of time fails the test, and no further child is started."""
    mine = lad.own_mode()
    worst, top = lad.all_references()
    print("largest e32 of the ladders: " + ", ".join(f"{f} {e:.3e} ({w})" for f, (e, w) in worst.items()) + f"; largest |sdf| {top:.3f}")
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
        print(p.stdout[-16000:])
        assert p.returncode >= 0, f"mode {mode}: the child died of signal {-p.returncode}; no further child started\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}"
        assert p.returncode == 0, (mode, p.stdout[-4000:], p.stderr[-2000:])


# ------------------------------------------------------------------------------------------------ the refusal
@pytest.mark.parametrize("entry", ["ls_sdf_decode", "ls_sdf_decode_train"])
def test_a_dense_call_of_2_31_rows_is_refused_before_anything_is_sized(entry, models):
    """The decoder's GEMMs take the row count as an int.  B x M >= 2^31 is refused by name -- not by whatever the truncated count would size --
    and nothing is enqueued: the workspace and the output, filled with a pattern, are untouched."""
    from livingscenes_amd import ops
    dev = _dev()
    if ("small", False) not in models:
        models[("small", False)] = lad.make_model("small", dev)
    m = models[("small", False)]
    lib = _lib.load()
    B, M = 65536, 32768
    q, z_so3, z_inv, s, t = (torch.zeros(n, device=dev) for n in (3, 96, 32, 1, 3))
    out = torch.full((16,), 7.0, device=dev)
    ws = torch.full((4096,), 0x5A, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = getattr(lib, entry)(m._h, ops.ptr(q), ops.ptr(z_so3), ops.ptr(z_inv), ops.ptr(s), ops.ptr(t), B, M, ops.ptr(out), ops.ptr(ws), ws.numel(),
                                 ops.stream_ptr(dev))
    msg = lib.ls_last_error().decode()
    torch.cuda.synchronize()
    assert rc == -1 and msg == f"{entry[3:]}: B={B} x M={M} rows too many for one call (< 2^31): split the queries", (rc, msg)      # LS_ERR_INVALID
    assert bool((ws == 0x5A).all()) and bool((out == 7.0).all())
