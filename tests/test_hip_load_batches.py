"""The kernels whose global loads were batched (row maxima of the GEMM family, the G terms and point -> instance map of gemm_vn_kernel, the weight
walk of glob_mean_gemv_kernel) at the smallest shapes where such an edit can go wrong, and their outputs pinned to the parent commit's bits.

1. row maxima through ls_gemm_f32_ex: a_rowmax [M][parts] for parts 1 .. 16 (vector path, dword path, clamped last trip), placed as the TAIL of its
   allocation; M = 130 (the last tile clamps at M - 1), K = 128 / 512, and the conv_c shape that splits K.  All equal bit for bit.
2. the residual global conv in its one-launch form (gemm_vn_kernel<true>, C = K = 128 / 256): a ten-point M-tile spanning four, three, one instance and a
   ragged last tile; a_parts 1 / 16, out_rowmax on / off; float64 oracle under the rule of tests/tools/glob_tail_vs_float64.py.
3. glob_mean_gemv_kernel alone at C with and without a remainder trip, from partial column sums and from a five-point message: float64 under the same
   rule, and bit for bit against a host restatement of the fp32 chains (the fused multiply-add is restated exactly: the product of two float32 is exact
   in float64, the sum is rounded to odd there and then once to float32).
4. the sha256 of every output above equals tests/golden/load_batches_parent_hashes.json, recorded from the parent commit's kernels.

    python tests/test_hip_load_batches.py --record FILE     (GPU; writes the hashes of the library LS_LIB_PATH names; see the fixture's header)
"""
import hashlib
import importlib.util
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(HERE, "golden", "load_batches_parent_hashes.json")


def _load_tool():
    spec = importlib.util.spec_from_file_location("glob_tail_vs_float64", os.path.join(HERE, "tools", "glob_tail_vs_float64.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


lad = _load_tool()
_OUT = {}     # {hash key: numpy array}: what the cases below produced in this process (each case runs once)
_DONE = set()  # the case groups (a GEMM shape, a conv layer, a mean (C, source)) that ran to their end in this process


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _keep(key, t):
    a = t.detach().cpu().numpy()
    assert key not in _OUT or np.array_equal(_OUT[key].view(np.uint32), a.view(np.uint32)), key
    _OUT[key] = a
    return a


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _gen(*key):
    import binascii
    return torch.Generator().manual_seed(binascii.crc32(":".join(str(k) for k in key).encode()))


# ------------------------------------------------------------------------------------------------ 1. row maxima through ls_gemm_f32_ex
GEMM_SHAPES = ((130, 128, 128, False), (130, 128, 512, False), (192, 260, 512, True))     # M, N, K, with the split-K workspace
PARTS = (1, 2, 3, 4, 5, 7, 8, 16)
SLACK = 64            # floats in front of a_rowmax (NaN); the array ends where its allocation ends


def block_maxima(A, parts):
    """[M, K] -> [M, parts]: max |A[row, q-th block of ceil(K / parts) columns]|, 0 where the block is empty"""
    M, K = A.shape
    w = -(-K // parts)
    out = torch.zeros(M, parts, dtype=torch.float32)
    for q in range(parts):
        if q * w < K:
            out[:, q] = A[:, q * w:(q + 1) * w].abs().amax(dim=1)
    return out


def gemm_inputs(M, N, K):
    g = _gen("gemm_ex", M, N, K)
    A, W = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5
    A[[0, 5]] *= 2.0 ** 20
    A[[64, M - 1]] *= 2.0 ** -20
    return A, W


def run_gemm_ex(A, W, a_rowmax, split, dev, offset=SLACK):
    """ls_gemm_f32_ex with the row maxima of W handed over; a_rowmax [M, parts] (CPU) or None"""
    from livingscenes_amd import _lib, ops
    M, K = A.shape
    N = W.shape[0]
    lib = _lib.load()
    Ad, Wd = A.to(dev), W.to(dev)
    wmax = ops.rowmax(Wd)
    out = torch.empty(M, N, dtype=torch.float32, device=dev)
    rm, parts, buf = None, 0, None
    if a_rowmax is not None:
        parts = a_rowmax.shape[1]
        buf = torch.full((offset + M * parts,), float("nan"), dtype=torch.float32, device=dev)
        rm = buf[offset:]
        rm.copy_(a_rowmax.reshape(-1))
    nb = int(lib.ls_gemm_workspace_bytes(M, N, K)) if split else 0
    ws = torch.empty(nb, dtype=torch.uint8, device=dev) if nb else None
    _lib.call(dev, "ls_gemm_f32_ex", ops.ptr(Ad), K, ops.ptr(Wd), K, None, ops.ptr(out), N, M, N, K, 0, ops.ptr(rm), parts, ops.ptr(wmax), None,
              ops.ptr(ws), nb, ops.stream_ptr(dev))
    torch.cuda.synchronize()
    if buf is not None:
        assert bool(torch.isnan(buf[:offset]).all()) and torch.equal(rm.cpu(), a_rowmax.reshape(-1)), "the row maxima or the slack in front were written"
    return out


def gemm_case(shape, dev):
    """every output of one shape -> {hash key: array}; asserts the bit identities"""
    M, N, K, split = shape
    A, W = gemm_inputs(M, N, K)
    name = f"gemm_ex:M{M}:N{N}:K{K}"
    if split:
        from livingscenes_amd import _lib
        assert int(_lib.load().ls_gemm_workspace_bytes(M, N, K)) > 0, "this shape is meant to split K"
    folded = block_maxima(A, 1)
    assert torch.equal(folded[:, 0], A.abs().amax(dim=1))
    base = _keep(f"{name}:parts1", run_gemm_ex(A, W, folded, split, dev))
    null = _keep(f"{name}:null", run_gemm_ex(A, W, None, split, dev))
    bad = []
    if not np.array_equal(base.view(np.uint32), null.view(np.uint32)):
        bad.append(f"{name}: a_rowmax = NULL differs from parts = 1 in {int((base != null).sum())} floats")
    for parts in PARTS[1:]:
        rmx = block_maxima(A, parts)
        assert torch.equal(rmx.amax(dim=1), folded[:, 0])
        for off in (SLACK,) + ((SLACK - 3,) if parts in (4, 16) else ()):      # 16-byte aligned parts, and the same parts on the dword path
            o = _keep(f"{name}:parts{parts}" + ("" if off == SLACK else ":unaligned"), run_gemm_ex(A, W, rmx, split, dev, off))
            if not np.array_equal(o.view(np.uint32), base.view(np.uint32)):
                bad.append(f"{name}: parts = {parts} (offset {off}) differs from parts = 1 in {int((o != base).sum())} floats")
    _DONE.add(("gemm", shape))
    return bad


@pytest.mark.parametrize("shape", GEMM_SHAPES, ids=[f"M{m}-N{n}-K{k}" + ("-split" if s else "") for m, n, k, s in GEMM_SHAPES])
def test_row_maxima_in_parts_give_the_bits_of_one_part_and_of_none(shape):
    bad = gemm_case(shape, _dev())
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------ 2. the global conv, one-launch form
VN_LAYERS = (4, 5)                                              # released model: C = K = 128, 256
VN_SHAPES = ((3, 3), (3, 7), (2, 10), (2, 32), (1, 41))         # (B, npts): a ten-point M-tile over 4 | 3 | 1 instances, whole tiles, a ragged last tile
# (this module's own copy of the tool: the first input of this shape has e32 = 7.2e-6 on the 'chan' kind, within a host's 20 % of the precondition --
# the tool's RESEED says why that matters; "#1" is the first suffix with e32 < 5.5e-6 on every kind)
lad.RESEED.setdefault("gc:released:5:1:41", "#1")


def vn_case_tuple(layer, B, N):
    return (f"global_conv(released, layer={layer}, B={B}, N={N}, glob_fuse=1)", "released", layer, (B, N), 1)


def run_vn(m, layer, f, a_rowmax, want_out_rowmax, dev):
    """ls_vn_lna_ex_f32 -> (out [B,N,3,C], out_rowmax [B*N*3, C/32] or None), on the device"""
    import ctypes
    from livingscenes_amd import _lib, ops
    B, N, _, C = f.shape
    lib = _lib.load()
    out = torch.empty_like(f)
    orm = torch.full((B * N * 3, C // 32), -1.0, dtype=torch.float32, device=dev) if want_out_rowmax else None
    nb = int(lib.ls_vn_lna_workspace_bytes(m._h, layer, B, N))
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    written = ctypes.c_int(-1)
    parts = 0 if a_rowmax is None else a_rowmax.shape[1]
    _lib.call(dev, "ls_vn_lna_ex_f32", m._h, layer, ops.ptr(f), B, N, ops.ptr(a_rowmax), parts, ops.ptr(orm), ctypes.addressof(written), ops.ptr(out),
              ops.ptr(ws), nb, ops.stream_ptr(dev))
    torch.cuda.synchronize()
    assert written.value == int(want_out_rowmax), "the one-launch form of the conv (gemm_vn_kernel) did not run"
    return out, orm


def vn_cases(layer, dev, model):
    from livingscenes_amd import _lib
    import glob_tail_oracle as gto
    bad = []
    prev = model.set_option(_lib.OPT_GLOB_FUSE, 1)
    try:
        for B, N in VN_SHAPES:
            case = vn_case_tuple(layer, B, N)
            for kind in lad.kinds_of(B):
                msg = lad.gc_inputs(case, kind)
                ref, e32 = lad.gc_reference(case, kind)
                f = lad.rows_layout(msg).to(dev)
                rows = f.reshape(B * N * 3, -1).cpu()
                outs = {}
                for parts in (1, 16):
                    rm = block_maxima(rows, parts).to(dev)
                    for orm_on in (0, 1):
                        out, orm = run_vn(model, layer, f, rm, bool(orm_on), dev)
                        key = f"vn:layer{layer}:B{B}:N{N}:{kind}:parts{parts}:rowmax{orm_on}"
                        outs[(parts, orm_on)] = _keep(key, out)
                        if orm_on:
                            C = out.shape[-1]
                            want = out.reshape(B * N * 3, C // 32, 32).abs().amax(dim=2)
                            _keep(key + ":out_rowmax", orm)
                            if not torch.equal(orm, want):
                                bad.append(f"{key}: out_rowmax is not max |out| over each 32-channel block in {int((orm != want).sum())} entries")
                        err = gto.per_point_err(out.permute(0, 3, 2, 1).cpu(), ref)
                        print(f"{key}: err {err:.3e} e32 {e32:.3e} bound {lad.bound(e32):.3e}")
                        lad._judge(key, kind, err, e32, bad)
                first = outs[(1, 0)]
                for k, o in outs.items():
                    if not np.array_equal(o.view(np.uint32), first.view(np.uint32)):
                        bad.append(f"vn layer {layer} B={B} N={N} {kind}: (a_parts, out_rowmax) = {k} differs from (1, 0) in {int((o != first).sum())} floats")
    finally:
        model.set_option(_lib.OPT_GLOB_FUSE, prev)
    _DONE.add(("vn", layer))
    return bad


@pytest.fixture(scope="module")
def released_model():
    m = lad.make_model("released", _dev())
    yield m
    m.close()


@pytest.mark.parametrize("layer", VN_LAYERS)
def test_global_conv_tiles_that_span_instances_vs_float64(layer, released_model):
    bad = vn_cases(layer, _dev(), released_model)
    assert not bad, f"{len(bad)} failures:\n" + "\n".join(bad[:20])


# ------------------------------------------------------------------------------------------------ 3. mean + contraction
MEAN_C = (36, 64, 68, 100, 128, 512)
MEAN_SOURCES = (("cs1", 1, 7), ("cs16", 16, 40), ("msg5", 5, 0))       # (name, rows N, npoints: > 0 = the rows are partial column sums over npoints points)
MEAN_B = 3


def mean_inputs(C, src):
    _, N, _ = next(s for s in MEAN_SOURCES if s[0] == src)
    g = _gen("mean", C, src)
    return torch.randn(MEAN_B, N, 3, C, generator=g), torch.randn(4 * C, C, generator=g) / C ** 0.5


def _fma32(a, b, c):
    """round(a * b + c) to float32, once: a * b is exact in float64, the float64 sum is rounded to ODD (TwoSum gives its error), so that the rounding
    to float32 sees what an infinitely precise sum would show it"""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    away = np.where(e > 0, np.inf, -np.inf)
    other = np.nextafter(s, away)
    odd = (s.view(np.int64) & 1) == 1
    s = np.where((e != 0) & ~odd, other, s)
    return s.astype(np.float32)


def mean_host_fp32(f, W, npoints):
    """glob_mean_gemv_kernel's fp32 chains with numpy.float32: the mean (sixteen row slices summed each, the slices ascending, where 3 C < 512; the rows
    ascending otherwise; times 1 / points), then per column sixteen lanes with k = 4 l, 4 l + 64, ... (x, y, z, w of a float4 in turn, one fma chain
    per output) combined in the order of group_sum<16>: lane ^ 1, lane ^ 2, 7 - lane within eight, 15 - lane within sixteen"""
    f, W = f.numpy(), W.numpy()
    B, N, _, C = f.shape
    ncols, col0 = 2 * C, 2 * C
    inv = np.float32(1.0) / np.float32(npoints if npoints > 0 else N)
    rows = f.reshape(B, N, 3 * C)
    if 3 * C >= 512:
        s = np.zeros((B, 3 * C), np.float32)
        for n in range(N):
            s = s + rows[:, n]
    else:
        part = np.zeros((16, B, 3 * C), np.float32)
        for n in range(N):
            part[n % 16] = part[n % 16] + rows[:, n]
        s = part[0]
        for r in range(1, 16):
            s = s + part[r]
    mean = (s * inv).reshape(B, 3, C)
    Wc = W[col0:col0 + ncols]                                    # [ncols, C]
    acc = np.zeros((16, B, 3, ncols), np.float32)                # lane, instance, axis, column
    for lane in range(16):
        for k in range(4 * lane, C, 64):
            for e in range(4):
                acc[lane] = _fma32(np.broadcast_to(mean[:, :, None, k + e], acc[lane].shape), np.broadcast_to(Wc[None, None, :, k + e], acc[lane].shape), acc[lane])
    lanes = np.arange(16)
    for partner in (lanes ^ 1, lanes ^ 2, (lanes & 8) | (7 - (lanes & 7)), 15 - lanes):
        acc = acc + acc[partner]
    return acc[0]                                                # [B, 3, ncols]


def run_mean(f, W, npoints, dev):
    from livingscenes_amd import _lib, ops
    B, N, _, C = f.shape
    fd, Wd = f.to(dev), W.to(dev)
    G = torch.full((B * 3, 4 * C), 7.0, dtype=torch.float32, device=dev)
    _lib.call(dev, "ls_glob_mean_gemv_f32", ops.ptr(fd), B, N, C, ops.ptr(Wd), 2 * C, 2 * C, ops.ptr(G), 4 * C, npoints, ops.stream_ptr(dev))
    torch.cuda.synchronize()
    assert bool((G[:, :2 * C] == 7.0).all()), "columns below col0 were written"
    return G[:, 2 * C:].reshape(B, 3, 2 * C)


def mean_case(C, src, dev):
    import glob_tail_oracle as gto
    _, N, npoints = next(s for s in MEAN_SOURCES if s[0] == src)
    f, W = mean_inputs(C, src)
    key = f"mean:C{C}:{src}"
    out = torch.from_numpy(_keep(key, run_mean(f, W, npoints, dev)))
    den = npoints if npoints > 0 else N

    def oracle(dtype):
        return torch.einsum("bxk,jk->bxj", f.to(dtype).sum(dim=1) / den, W[2 * C:].to(dtype))
    ref = oracle(torch.float64)
    as_points = lambda t: t.reshape(MEAN_B, -1, 1, 1)            # per instance (glob_tail_oracle.per_instance_errs)
    e32 = gto.per_point_err(as_points(oracle(torch.float32)), as_points(ref))
    err = gto.per_point_err(as_points(out), as_points(ref))
    print(f"{key}: err {err:.3e} e32 {e32:.3e} bound {lad.bound(e32):.3e}")
    bad = []
    lad._judge(key, "randn", err, e32, bad)
    host = mean_host_fp32(f, W, npoints)
    if not np.array_equal(host.view(np.uint32), out.numpy().view(np.uint32)):
        bad.append(f"{key}: differs from the host restatement of the fp32 chains in {int((host != out.numpy()).sum())} of {host.size} floats")
    _DONE.add(("mean", C, src))
    return bad


@pytest.mark.parametrize("C", MEAN_C)
def test_mean_and_contraction_vs_float64_and_the_fp32_chain(C):
    bad = [b for src, _, _ in MEAN_SOURCES for b in mean_case(C, src, _dev())]
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------ 4. the parent commit's bits
def all_outputs(dev):
    """run whatever has not run in this process -> {hash key: sha256}"""
    for shape in GEMM_SHAPES:
        if ("gemm", shape) not in _DONE:
            gemm_case(shape, dev)
    todo = [layer for layer in VN_LAYERS if ("vn", layer) not in _DONE]
    if todo:
        m = lad.make_model("released", dev)
        try:
            for layer in todo:
                vn_cases(layer, dev, m)
        finally:
            m.close()
    for C in MEAN_C:
        for src, _, _ in MEAN_SOURCES:
            if ("mean", C, src) not in _DONE:
                mean_case(C, src, dev)
    return {k: _sha(v) for k, v in sorted(_OUT.items())}


def test_outputs_carry_the_parent_commits_bits():
    with open(GOLDEN) as fh:
        golden = json.load(fh)["sha256"]
    got = all_outputs(_dev())
    assert sorted(got) == sorted(golden), sorted(set(got) ^ set(golden))
    nulls = [k for k, v in golden.items() if v is None]
    assert 10 * len(nulls) <= len(golden), f"{len(nulls)} of {len(golden)} cases are not reproducible on the parent: the inputs are wrong"
    bad = [k for k, v in golden.items() if v is not None and got[k] != v]
    assert not bad, f"{len(bad)} of {len(golden)} outputs differ from the parent commit's:\n" + "\n".join(bad[:30])


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "--record", __doc__
    first = all_outputs(_dev())
    _OUT.clear()
    _DONE.clear()
    second = all_outputs(_dev())
    head = {}
    if os.path.exists(sys.argv[2]):      # the fixture's header (what, recorded_with) stays
        with open(sys.argv[2]) as fh:
            head = {k: v for k, v in json.load(fh).items() if k in ("what", "recorded_with")}
    with open(sys.argv[2], "w") as fh:
        json.dump({**head, "cases": len(first), "sha256": {k: (v if second[k] == v else None) for k, v in first.items()}}, fh, indent=1)
    print(f"{len(first)} hashes, {sum(first[k] != second[k] for k in first)} not reproducible -> {sys.argv[2]}")
