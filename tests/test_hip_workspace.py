"""The workspace contract on the device (csrc/ls_workspace.h: one layout function per operator gives both the size the query reports and
the pieces the operator uses).

1. The queries that need a model handle answer what tests/golden/workspace_bytes_model.json holds (recorded on an MI355X from the library as
   it was before ls::Arena; ladder: tests/tools/record_workspace_bytes.py).  The model-free queries: tests/test_workspace_bytes_cpu.py.
2. Exact fit, for the operators whose size used to be a formula of its own beside the pointer arithmetic: with workspace_bytes = exactly the
   queried size the operator leaves the 4096 bytes after it untouched and computes, bit for bit, what it computes in a workspace 1 MiB larger;
   one byte less is refused with LS_ERR_WORKSPACE before anything is written.  (The guard bytes lie inside the allocation.)"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from livingscenes_amd import synth
from test_workspace_bytes_cpu import recorder

pytestmark = pytest.mark.gpu
LS_ERR_WORKSPACE = -3
GUARD, FILL = 4096, 0xA5


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def test_model_bound_workspace_sizes_are_the_recorded_ones():
    from livingscenes_amd import _lib
    rec = recorder()
    lib = _lib.load()
    with open(os.path.join(rec.GOLDEN, "workspace_bytes_model.json")) as f:
        want = json.load(f)
    got = {}
    for which in rec.MODELS:
        ecfg, m = rec.make_model(which)
        for n, a in rec.model_ladder(ecfg):
            got[which + ":" + rec.key(n, a)] = int(getattr(lib, n)(m._h, *a))
        assert lib.ls_encoder_workspace_bytes(m._h, 0, 1024) == 0   # (divided by zero on the host before: not in the record)
        m.close()
    assert set(got) == set(want), "the ladder and the record list different cases: re-record (see the recorder's docstring)"
    wrong = {k: (want[k], got[k]) for k in want if got[k] != want[k]}
    assert not wrong, f"{len(wrong)} sizes differ from the record (recorded, now): {dict(list(wrong.items())[:8])}"
    for name in {k.split(":")[1].split("(")[0] for k in want}:   # every query both sizes and refuses something on the ladder
        vals = [v for k, v in want.items() if k.split(":")[1].startswith(name + "(")]
        assert any(v > 0 for v in vals) and (any(v == 0 for v in vals) or name.startswith("ls_sdf_")), name


# ------------------------------------------------------------------------------------------------ exact fit
def _exact_fit(need, op, outputs):
    """op(ws tensor, workspace_bytes) -> status.  `outputs()` -> fresh output tensors (pre-filled: a refused call must leave them alone); they
    are passed to op through the closure's `out` list."""
    from livingscenes_amd import _lib
    assert need > 0
    d = _dev()

    def run(alloc, passed):
        ws = torch.full((alloc,), FILL, dtype=torch.uint8, device=d)
        out = outputs()
        rc = op(ws, passed, out)
        torch.cuda.synchronize()
        return rc, ws, [o.clone() for o in out]

    rc, ws, fit = run(need + GUARD, need)
    assert rc == 0, _lib.load().ls_last_error()
    assert bool((ws[need:] == FILL).all()), "the operator wrote past the size its query reports"
    rc, _, roomy = run(need + (1 << 20), need + (1 << 20))
    assert rc == 0, _lib.load().ls_last_error()
    for a, b in zip(fit, roomy):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "the result depends on the workspace beyond the queried size"
    rc, ws, short = run(need + GUARD, need - 1)
    assert rc == LS_ERR_WORKSPACE, (rc, _lib.load().ls_last_error())
    assert bool((ws == FILL).all()), "a refused call wrote to the workspace"
    for o, fresh in zip(short, outputs()):
        assert torch.equal(o.view(torch.uint8), fresh.view(torch.uint8)), "a refused call wrote an output"
    return fit


@pytest.fixture(scope="module")
def released():
    from livingscenes_amd import ops, packing
    cfg = synth.default_encoder_cfg()
    desc, blob = packing.pack_model(synth.make_encoder_weights(cfg, 0), cfg, None, None)
    m = ops.HipModel(desc, blob, _dev())
    yield cfg, m
    m.close()


@pytest.mark.parametrize("layer", [5, 6])
def test_edgeconv_attention_layers_5_and_6_fit_their_workspace_exactly(released, layer):
    """The 32-point attention layers of the released widths at B = 1 (the only shapes the table-free path takes): layer 5 reads 128 source points
    and selects 32 destination rows, layer 6 works on the 32 points."""
    from livingscenes_amd import _lib
    from livingscenes_amd._lib import ptr, stream_ptr
    cfg, m = released
    lib, d = _lib.load(), _dev()
    Ns, Nd, Cin, Co = (128, 32, cfg["feat_dim"][4], cfg["feat_dim"][5]) if layer == 5 else (32, 32, cfg["feat_dim"][5], cfg["feat_dim"][6])
    g = torch.Generator().manual_seed(layer)
    src = torch.randn(1, Ns, 3, Cin, generator=g).to(d)
    knn = torch.stack([torch.randperm(Ns, generator=g)[:16] for _ in range(Nd)])[None].to(torch.int32).to(d)
    rows = torch.randperm(Ns, generator=g)[:Nd][None].to(torch.int32).contiguous().to(d) if layer == 5 else None
    need = lib.ls_vn_edgeconv_workspace_bytes(m._h, layer, 1, Ns, Nd, int(rows is not None))

    def op(ws, nbytes, out):
        with torch.cuda.device(d):
            return lib.ls_vn_edgeconv_attn_f32(m._h, layer, ptr(src), ptr(knn), ptr(rows), 1, Ns, Nd, ptr(out[0]), ptr(ws), nbytes, stream_ptr(d))
    out, = _exact_fit(need, op, lambda: [torch.full((1, Nd, 3, Co), -7.0, device=d)])
    assert bool(torch.isfinite(out).all()) and float(out.abs().max()) > 0


def test_encoder_tail_fits_its_workspace_exactly(released):
    from livingscenes_amd import _lib
    from livingscenes_amd._lib import ptr, stream_ptr
    cfg, m = released
    lib, d = _lib.load(), _dev()
    NP, C = 32, cfg["c_dim"]
    f = torch.randn(1, NP, 3, cfg["feat_dim"][-1], generator=torch.Generator().manual_seed(1)).to(d)
    need = lib.ls_encoder_tail_workspace_bytes(m._h, 1, NP)

    def op(ws, nbytes, out):
        with torch.cuda.device(d):
            return lib.ls_encoder_tail_f32(m._h, ptr(f), None, None, 1, NP, ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(out[3]), ptr(ws), nbytes,
                                           stream_ptr(d))
    outs = _exact_fit(need, op, lambda: [torch.full(s, -7.0, device=d) for s in ((1, C, 3), (1, C), (1,), (1, 3))])
    assert all(bool(torch.isfinite(o).all()) for o in outs) and float(outs[0].abs().max()) > 0


def test_cosine_scores_batch_fits_its_workspace_exactly():
    """Three problems of 1 x 1, 5 x 0 and 33 x 17 rows: 57 inverse norms after the offsets, so the size does not end on a multiple of 256."""
    from livingscenes_amd import _lib
    from livingscenes_amd._lib import ptr, stream_ptr
    lib, d = _lib.load(), _dev()
    sizes, D = [(1, 1), (5, 0), (33, 17)], 8
    src_off = np.cumsum([0] + [n for n, _ in sizes]).astype(np.int64)
    tgt_off = np.cumsum([0] + [m for _, m in sizes]).astype(np.int64)
    nt, mt, entries = int(src_off[-1]), int(tgt_off[-1]), sum(n * m for n, m in sizes)
    g = torch.Generator().manual_seed(2)
    M0, M1 = torch.randn(nt, D, generator=g).to(d), torch.randn(mt, D, generator=g).to(d)
    need = lib.ls_cosine_scores_batch_workspace_bytes(len(sizes), nt, mt)
    assert need % 256 != 0
    hp = lambda a: ctypes.c_void_p(a.ctypes.data)

    def op(ws, nbytes, out):
        with torch.cuda.device(d):
            return lib.ls_cosine_scores_batch_f32(len(sizes), ptr(M0), nt, hp(src_off), ptr(M1), mt, hp(tgt_off), D, ptr(out[0]), ptr(ws), nbytes,
                                                  stream_ptr(d))
    S, = _exact_fit(need, op, lambda: [torch.full((entries,), -7.0, device=d)])
    want = torch.nn.functional.normalize(M0[6:].double(), dim=1) @ torch.nn.functional.normalize(M1[1:].double(), dim=1).T
    assert float((S[1:].double().view(33, 17) - want).abs().max()) < 1e-5   # fp32 dot products of unit rows, D = 8


def test_mise_batch_state_fits_exactly():
    """B = 3 octrees of res0 = 2, depth = 1: ls_mise_init_batch clears the state, ls_mise_query_batch takes its block sums from the end of it."""
    from livingscenes_amd import _lib
    from livingscenes_amd._lib import ptr, stream_ptr
    lib, d = _lib.load(), _dev()
    B, res0, depth = 3, 2, 1
    npts = lib.ls_mise_lattice_points(res0, depth)
    cap = B * npts
    need = lib.ls_mise_batch_state_bytes(B, res0, depth)

    def op(state, nbytes, out):
        with torch.cuda.device(d):
            rc = lib.ls_mise_init_batch(ptr(state), nbytes, B, res0, depth, stream_ptr(d))
            if rc != 0:
                return rc
            return lib.ls_mise_query_batch(ptr(state), B, res0, depth, 1.0, ptr(out[0]), ptr(out[1]), ptr(out[2]), cap, ptr(out[3]), stream_ptr(d))
    fresh = lambda: [torch.full((cap,), -7, dtype=torch.int32, device=d), torch.full((cap,), -7, dtype=torch.int32, device=d),
                     torch.full((cap, 3), -7.0, device=d), torch.full((B + 1,), -7, dtype=torch.int64, device=d)]
    idx, inst, pts, off = _exact_fit(need, op, fresh)
    off = off.cpu().tolist()
    n0 = (res0 + 1) ** 3   # a fresh octree asks for the corners of its level-0 voxels
    assert off == [0, n0, 2 * n0, 3 * n0] and inst[:off[-1]].cpu().tolist() == [b for b in range(B) for _ in range(n0)]
