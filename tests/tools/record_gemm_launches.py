"""Record which GEMM kernels the library launches, and with what grid, on a fixed ladder of problems.

    python tests/tools/record_gemm_launches.py [--out PATH]                 -> tests/golden/gemm_launches.json   (GPU, rocprofv3 on the PATH)
    python tests/tools/record_gemm_launches.py --family edge [--out PATH]   -> tests/golden/edge_launches.json   (the edge-conv layers, below)
    python tests/tools/record_gemm_launches.py --family knn [--out PATH]    -> tests/golden/knn_launches.json    (the k-NN builds, below)

The wide, the tiled and the persistent kernels agree to the bit by design, so no numerical test sees a change of the kernel CHOICE; it only
shows as a slower benchmark line.  The choice is therefore recorded from the library BEFORE a change to the dispatch code (csrc/gemm_plan.h)
and compared afterwards: tests/test_gemm_plan_cpu.py replays the plan on the host against the record, tests/test_hip_range.py compares the
outputs' hashes, and running this tool again must reproduce the file byte for byte.  Re-record only when a choice is meant to change.

How: one child process per arithmetic mode (LS_GEMM_MODE is read once per process) runs `--worker` as the program of a
`rocprofv3 --kernel-trace` run (CSV, no counters, under a time limit).  The worker walks ladder() / model_ladder() in order and brackets every
case with a marker launch (ls_rowmax_f32 on MARKER_ROWS rows: a grid no case produces; the count of markers is checked).  The launches between
a case's two markers whose kernel name starts with ls::gemm_ are the record, operand preparation (gemm_rowmax_kernel, gemm_presplit_w_kernel)
left out.  ladder() / model_ladder() are the one statement of the cases, shared with the tests.

--family edge records the encoder's edge-conv layers the same way (csrc/edge_plan.h; tests/test_edge_plan_cpu.py, tests/test_hip_range.py):
edge_ladder() runs HipModel.edgeconv per layer and whole ls_encode calls; the record keeps the kernels of edge.hip / edge_fused.hip and the two
mean kernels of the global conv (their grid is the only visible trace of the column sums), counts the table GEMMs, and hashes every output.

--family knn records ops.knn (ls_knn_f32) on knn_ladder(): both sides of every boundary of csrc/knn_plan.h at the smallest size that reaches it
(tests/test_knn_plan_cpu.py replays the plan, tests/test_hip_parity.py holds every case to the oracle and to the recorded hash).  The k-NN
kernels do not read LS_GEMM_MODE: one process, filed under the default mode."""
import argparse
import binascii
import csv
import glob
import hashlib
import json
import os
import subprocess
import sys
import tempfile

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
GOLDEN = os.path.join(REPO, "tests", "golden", "gemm_launches.json")
GOLDENS = {"gemm": GOLDEN, "edge": os.path.join(REPO, "tests", "golden", "edge_launches.json"), "knn": os.path.join(REPO, "tests", "golden", "knn_launches.json")}
MODES = ("f16", "bf16x3", "fp32")          # GemmTraits::mode 0 / 1 / 2; the first is the default (no LS_GEMM_MODE)
MARKER_ROWS = 52                            # 13 workgroups of gemm_rowmax_kernel
TEST_MAX_OUT = 1 << 22                      # outputs up to 4 M floats are hashed (tests/test_hip_range.py runs these cases), plus TEST_WIDE
TEST_WIDE = "f32(4096x4096x128)"            # the first shape the wide kernel accepts
UNITS = {"kernels": "[demangled name up to the parameter list, workgroup (x, y, z) in work-items, LDS bytes per workgroup], as the kernel trace reports "
                    "them (LDS: the static part; the dynamic LDS of gemm_w2_kernel does not show)",
         "launch": "[index into kernels, grid x, grid y] in work-items as the kernel trace reports them (workgroups x workgroup size); grid z is 1",
         "cases": "by key, which names the entry point and its arguments; the GemmTraits behind a key are stated by ladder() / model_ladder() of "
                  "tests/tools/record_gemm_launches.py; per arithmetic mode the launches in order",
         "sha256": "of the output's bytes, row-major [M][N] float32; operands from numpy.random.default_rng(crc32(case key))",
         "status": "the entry point's return value where it is not 0 (a refusal: no launch)"}


EDGE_UNITS = {"kernels": UNITS["kernels"].replace("gemm_w2_kernel", "edge_attn_kernel"),
              "launch": UNITS["launch"],
              "cases": "by key; edge_ladder() of tests/tools/record_gemm_launches.py states the handle, the layer and the sizes behind a key, edge_traits() the "
                       "EdgeTraits; per arithmetic mode the launches of the kernels of edge.hip / edge_fused.hip and of glob_mean_gemv_kernel / mean_points_kernel: "
                       "in order for edgeconv(...), sorted for encode(...) (two side streams make the trace's order vary)",
              "tables": "edgeconv(...) only: how many GEMM launches formed the case's tables",
              "sha256": "of the output's bytes (encode: z_so3, z_inv, s, t one after the other); inputs from numpy.random.default_rng(crc32(case key))"}


KNN_UNITS = {"kernels": UNITS["kernels"].replace(" (LDS: the static part; the dynamic LDS of gemm_w2_kernel does not show)", ""),
             "launch": UNITS["launch"],
             "cases": "by key; knn_ladder() of tests/tools/record_gemm_launches.py states the sizes and the data behind a key, knn_traits() the KnnTraits; the "
                      "launches of the kernels of knn.hip / knn_mfma.hip / knn_xyz.hip in order (one process: the k-NN kernels have no arithmetic modes)",
             "sha256": "of the bytes of idx [B][Nd][16] int32, then dist [B][Nd][16] float32; inputs from knn_inputs()"}


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ the public entry points
def mm(M, N, K, lda=None, ldw=None, pieces=3, gather=0, masked=0, may_split=0, latency=0, has_planes=0, wants_out_rowmax=0):
    """GemmTraits of one A[M,K] W[N,K]^T problem (mode comes from the process)."""
    return dict(form="mm", M=M, N=N, K=K, lda=lda or K, ldw=ldw or K, pieces=pieces, gather=gather, masked=masked, may_split=may_split, latency=latency,
                has_planes=has_planes, wants_out_rowmax=wants_out_rowmax)


def vn(M, C, K, npts, a_parts, has_a_rowmax, has_w_rowmax=1, has_G_or_cs=1):
    return dict(form="vn", M=M, C=C, K=K, lda=K, ldw=K, npts=npts, has_G_or_cs=has_G_or_cs, a_parts=a_parts, has_a_rowmax=has_a_rowmax,
                has_w_rowmax=has_w_rowmax)


def ladder():
    """[(key, entry, traits)]: entry 'f32' = ls_gemm_f32 with the workspace its query asks for; 'ex' = ls_gemm_f32_ex (traits say whether
    with a workspace and an out_rowmax); 'planes' = ls_gemm_f32_planes.  A case on each side of every threshold of the plan."""
    shapes = []
    # wide 256 x 256 tiles: cdiv(M,256) * cdiv(N,256) = 255 | 256 | 257, 435 | 436, 1024 at K = 128; K = 96 is never wide
    shapes += [(3833, 4352, 128), (4096, 4096, 128), (250, 65792, 128), (3840, 7424, 128), (1024, 27904, 128), (8192, 8192, 128), (4096, 4096, 96)]
    # split-K: cdiv(M,128) * cdiv(N,128) = 191 | 192; K = 124 | 128; N % 4 != 0; the two shapes of the global conv's mean rows / conv_c
    shapes += [(128, 24448, 128), (128, 24576, 128), (192, 1024, 124), (192, 1024, 128), (96, 258, 512), (192, 1024, 512), (96, 260, 512)]
    # persistent small-K kernels: K = 32 | 64 with cdiv(M,128) = 15 | 16
    shapes += [(1920, 96, 32), (1925, 96, 32), (1920, 96, 64), (1925, 96, 64)]
    # K classes: tiled at K <= 64, K % 32 != 0, and long K with / without W planes
    shapes += [(300, 200, 16), (300, 200, 4), (700, 200, 132), (700, 200, 96), (700, 200, 512), (700, 200, 520)]
    c = []
    for M, N, K in shapes:
        s = f"{M}x{N}x{K}"
        c.append((f"f32({s})", "f32", mm(M, N, K, may_split=1)))
        c.append((f"ex({s})", "ex", mm(M, N, K)))
        c.append((f"ex({s}, out_rowmax)", "ex", mm(M, N, K, wants_out_rowmax=1)))
        c.append((f"ex({s}, workspace)", "ex", mm(M, N, K, may_split=1)))
        if K in (64, 96, 128, 512, 520) and M * N <= 1 << 24:      # (refused below K = 512 and at K % 32 != 0: recorded as a status)
            c.append((f"planes({s})", "planes", mm(M, N, K, has_planes=1)))
            c.append((f"planes({s}, out_rowmax)", "planes", mm(M, N, K, has_planes=1, wants_out_rowmax=1)))
    # the wide kernel addresses its operands by 32-bit byte offsets: M * lda and N * max(ldw, K) on each side of 2^30 elements
    c.append(("ex(4096x4096x128, lda=262140)", "ex", mm(4096, 4096, 128, lda=262140)))
    c.append(("ex(4096x4096x128, lda=262144)", "ex", mm(4096, 4096, 128, lda=262144)))
    c.append(("ex(4096x4096x128, ldw=262144)", "ex", mm(4096, 4096, 128, ldw=262144)))
    return c


def tested(key, t):
    """The cases small enough for a test: their outputs are hashed."""
    return key == TEST_WIDE or (t["M"] * t["N"] <= TEST_MAX_OUT and t["lda"] == t["K"] and t["ldw"] == t["K"])


def _seed(key):
    return binascii.crc32(key.encode())


def run_public(key, entry, t):
    """Run one ladder() case on the current device -> (status, sha256 of the output or None)."""
    import numpy as np
    import torch
    from livingscenes_amd import _lib, ops
    lib, dev = _lib.load(), torch.device("cuda:0")
    M, N, K, lda, ldw = t["M"], t["N"], t["K"], t["lda"], t["ldw"]
    rng = np.random.default_rng(_seed(key))
    a = torch.from_numpy(rng.standard_normal((M, K), dtype=np.float32))
    w = torch.from_numpy(rng.standard_normal((N, K), dtype=np.float32))
    bias = torch.from_numpy(rng.standard_normal(N, dtype=np.float32)).to(dev)

    def place(x, ld):     # rows at a leading dimension of ld floats (only the first K of a row are ever read)
        if ld == K:
            return x.to(dev)
        buf = torch.empty(x.shape[0], ld, dtype=torch.float32, device=dev)
        buf[:, :K] = x.to(dev)
        return buf
    A, W = place(a, lda), place(w, ldw)
    out = torch.zeros(M, N, dtype=torch.float32, device=dev)
    st = ops.stream_ptr(dev)
    p = ops.ptr
    if entry == "f32":
        nb = lib.ls_gemm_workspace_bytes(M, N, K)
        ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=dev)
        args = ("ls_gemm_f32", p(A), lda, p(W), ldw, p(bias), p(out), N, M, N, K, 1, p(ws) if nb else None, nb, st)
    else:
        wmax = ops.rowmax(w.to(dev))
        amax = ops.rowmax(a.to(dev))
        orm = torch.empty(M, lib.ls_gemm_rowmax_parts(N), dtype=torch.float32, device=dev) if t["wants_out_rowmax"] else None
        if entry == "ex":
            nb = lib.ls_gemm_workspace_bytes(M, N, K) if t["may_split"] else 0
            ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=dev)
            args = ("ls_gemm_f32_ex", p(A), lda, p(W), ldw, p(bias), p(out), N, M, N, K, 1, p(amax), 1, p(wmax), p(orm), p(ws) if nb else None, nb, st)
        else:
            nb = lib.ls_gemm_w_planes_bytes(N, K)
            planes = torch.empty(max(nb, 16), dtype=torch.uint8, device=dev)
            if nb:
                ops.call(dev, "ls_gemm_presplit_w_f32", p(W), ldw, N, K, p(wmax), p(planes), nb, st)
            args = ("ls_gemm_f32_planes", p(A), lda, p(W), ldw, p(planes), p(bias), p(out), N, M, N, K, 1, p(amax), 1, p(wmax), p(orm), st)
    marker()
    with torch.cuda.device(dev):
        status = int(getattr(lib, args[0])(*args[1:]))
    marker()
    sha = None
    if status == 0 and tested(key, t):
        sha = hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()
    return status, sha


def check_hashes(mode):
    """Run the small public cases of ladder() in this process (which must be in arithmetic mode `mode`) -> {key: (recorded, now)} of the
    cases whose status or output hash differs from the record.  The trace does not show the arguments the plan hands the kernels (kchunk,
    slab stride, per_n, tn); the outputs do, and every path is free of atomics, so equality is exact."""
    want = load()
    wrong, n = {}, 0
    for key, entry, t in ladder():
        w = want[f"{mode}:{key}"]
        if not tested(key, t):
            continue
        got = run_public(key, entry, t)
        n += 1
        if got != (w["status"], w["sha256"]):
            wrong[key] = ((w["status"], w["sha256"]), got)
    assert n > 60, n
    return wrong


_marker = None


def marker():
    import torch
    from livingscenes_amd import ops
    global _marker
    if _marker is None:
        _marker = torch.ones(MARKER_ROWS, 4, dtype=torch.float32, device="cuda:0")
    ops.rowmax(_marker)


# ------------------------------------------------------------------------------------------------ the internal traits, through a model handle
def model_ladder(mode=MODES[0]):
    """[(key, model, op, args, options, traits or None)]: gather, masked, two-piece, latency and the three VN kernels are reachable only
    through a model handle (built as record_workspace_bytes.py --model builds its handles).  options: {_lib.OPT_* name: value} set around the call.
    traits: the GemmTraits of the case's GEMMs in launch order, where this file can state them.  The other two arithmetic modes run the
    encoder's cases (the fused kernels exist for the default mode only: the table path and GEMM + activation are taken whatever the options say)."""
    from livingscenes_amd import synth
    c = []
    e = synth.default_encoder_cfg()
    fd, a0 = e["feat_dim"], e["atten_start_layer"]

    def tables(i, B, Ns, Nd, rows, planes_q=False):      # the table path of edge-conv layer i (model.hip: edge_tables)
        cin, nc, pc = fd[i - 1], (10 if i >= a0 else 4) * fd[i], (4 if i >= a0 else 2) * fd[i]
        pl = int(cin >= 512 and cin % 32 == 0)
        if rows:
            return [mm(B * Ns * 3, pc, cin, has_planes=pl), mm(B * Nd * 3, nc - pc, cin, gather=1, has_planes=pl)]
        return [mm(B * Ns * 3, nc, cin, has_planes=pl)]
    # gather: the destination-side table of a down-sampling layer on the FPS-selected rows; K = 32 / 64 / 128 / 256, cdiv(M,128) on both sides of 16
    for i, B, Ns, Nd in ((2, 1, 512, 256), (2, 4, 512, 256), (2, 8, 512, 256), (4, 4, 256, 64), (4, 32, 256, 64), (5, 8, 128, 32), (3, 4, 256, 256),
                         (6, 8, 32, 32), (1, 4, 512, 512)):
        rows = int(Ns != Nd)
        c.append((f"edgeconv(layer={i}, B={B}, Ns={Ns}, Nd={Nd}, fuse_q=0, fuse_t=0)", "released", "edgeconv", (i, B, Ns, Nd, rows),
                  {"OPT_EDGE_FUSE_Q": 0, "OPT_EDGE_FUSE_T": 0}, tables(i, B, Ns, Nd, rows)))
        if i >= a0:
            c.append((f"edgeconv(layer={i}, B={B}, Ns={Ns}, Nd={Nd})", "released", "edgeconv", (i, B, Ns, Nd, rows), {},
                      None if mode == MODES[0] else tables(i, B, Ns, Nd, rows)))
    # residual global conv: OPT_GLOB_FUSE 0 (GEMM + latency GEMM + activation) / 1 (tiled VN kernels) / 2 (streaming VN kernel where it applies);
    # 64 channels at M = 3 B Nd on both sides of 1536 (streaming) and of 16 tiles of 120 rows (persistent), 128 and 512 channels
    for i, B, Nd in ((2, 1, 504), (2, 1, 512), (2, 1, 600), (2, 1, 608), (3, 8, 256), (2, 1, 508), (4, 8, 64), (4, 1, 64), (6, 64, 32), (6, 1, 32)):
        Co, M = fd[i], B * Nd * 3
        for gf in (0, 1, 2):
            tr = [vn(M, Co, Co, Nd, a_parts=int(gf == 2), has_a_rowmax=int(gf == 2))] if gf and mode == MODES[0] else \
                 [mm(M, 2 * Co, Co, may_split=1, has_planes=int(Co >= 512)), mm(B * 3, 4 * Co, Co, may_split=1, latency=1)]
            c.append((f"lna(layer={i}, B={B}, N={Nd}, glob_fuse={gf})", "released", "lna", (i, B, Nd), {"OPT_GLOB_FUSE": gf}, tr))
    # conv_c of the encoder tail: M = 96 B rows against K = 512, split along K while the grid is under-filled
    for B in (1, 3, 64, 256):
        c.append((f"tail(B={B}, NP=32)", "released", "tail", (B, 32), {}, [mm(B * 96, 260, 512, may_split=1, has_planes=1)]))
    if mode != MODES[0]:
        return c
    # the decoder: inference (never splits K; two-piece products opt-in), training forward + backward (masked; split-K opt-out)
    for model, B, M in (("released", 1, 1024), ("released", 1, 37376), ("small", 2, 256)):
        for x2 in (0, 1):
            c.append((f"sdf_decode(B={B}, M={M}, bf16x2={x2})", model, "sdf_decode", (B, M), {"OPT_SDF_BF16X2": x2}, sdf_traits(model, B * M, x2, None)))
            for sk in (0, 1):
                c.append((f"sdf_train_backward(B={B}, M={M}, bf16x2={x2}, train_splitk={sk})", model, "sdf_backward", (B, M),
                          {"OPT_SDF_BF16X2": x2, "OPT_SDF_TRAIN_SPLITK": sk}, sdf_traits(model, B * M, x2, sk)))
    return c


def _scratch_floats(M, N, K):   # only to say whether the decoder's training workspace has split-K slabs at all (model.hip: sdf_gemm_scratch)
    tiles = cdiv(M, 128) * cdiv(N, 128)
    if tiles >= 192 or K < 128 or N % 4:
        return 0
    s2 = min(512 // tiles, K // 32)
    return s2 * M * N if s2 >= 2 else 0


def sdf_traits(model, rows, x2, train_splitk):
    """The decoder's GEMMs (model.hip: sdf_forward, ls_sdf_backward); train_splitk None = inference."""
    from livingscenes_amd import synth
    dcfg = synth.default_decoder_cfg() if model == "released" else synth.small_decoder_cfg()
    return sdf_traits_of(dcfg, rows, x2, train_splitk)


def sdf_traits_of(dcfg, rows, x2, train_splitk):
    """sdf_traits for any decoder configuration packing.pack_model takes: the width, the depth and the skip (none: latent_in = []) come from
    dcfg, the width of the decoder input u from latent_size + pe_dim"""
    w, nl, li = dcfg["dims"][0], len(dcfg["dims"]) + 1, (list(dcfg["latent_in"]) + [-1])[0]
    pad4 = lambda v: (v + 3) // 4 * 4
    outw = [w] + [pad4(w - (dcfg["latent_size"] + dcfg["pe_dim"])) if l + 1 == li else w for l in range(1, nl - 1)]
    pl = lambda K: int(K >= 512 and K % 32 == 0)
    layers = [(l, outw[l - 1], outw[l]) for l in range(1, nl - 1)]
    gws = bool(train_splitk) and any(_scratch_floats(rows, o, k) or _scratch_floats(rows, k, o) for _, k, o in layers)
    fwd = []
    for l, kin, o in layers:
        if x2 and not gws:
            fwd.append(mm(rows, o, kin, lda=w, pieces=2))                 # (the two-piece launch takes no operand ranges or planes)
        else:
            fwd.append(mm(rows, o, kin, lda=w, may_split=int(gws), has_planes=pl(kin), wants_out_rowmax=int(l != li and not x2 and not (gws and _scratch_floats(rows, o, kin)))))
    if train_splitk is None:
        return fwd
    bwd = []
    for l, kin, o in reversed(layers):
        if not gws and kin % 4 == 0:
            bwd.append(mm(rows, kin, o, lda=w, ldw=o, pieces=2 if x2 else 3, masked=1, has_planes=pl(o), wants_out_rowmax=int(not x2)))
        else:
            bwd.append(mm(rows, kin, o, lda=w, ldw=o, may_split=int(gws), has_planes=pl(o), wants_out_rowmax=int(not x2 and not (gws and _scratch_floats(rows, kin, o)))))
    return fwd + bwd


def model_cfgs(which):
    """'released' / 'small' as record_workspace_bytes.py builds them; 'pool64' / 'pool96': the small model with feat_dim[1] = 64 / 96."""
    import record_workspace_bytes as rwb
    if which in rwb.MODELS:
        return rwb.model_cfgs(which)
    ecfg, dcfg = rwb.model_cfgs("small")
    return dict(ecfg, feat_dim=[32, int(which[4:]), 32, 64]), dcfg


def make_model(which):
    import torch
    from livingscenes_amd import ops, packing, synth
    ecfg, dcfg = model_cfgs(which)
    desc, blob = packing.pack_model(synth.make_encoder_weights(ecfg, 0), ecfg, synth.make_decoder_weights(dcfg, 0), dcfg)
    return ecfg, ops.HipModel(desc, blob, torch.device("cuda:0"))


def run_model(models, key, model, op, args, options, want_hash=False):
    import numpy as np
    import torch
    from livingscenes_amd import _lib
    if model not in models:
        models[model] = make_model(model)
    ecfg, m = models[model]
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(_seed(key))
    rnd = lambda *s: torch.from_numpy(rng.standard_normal(s, dtype=np.float32)).to(dev)
    prev = {k: m.set_option(getattr(_lib, k), v) for k, v in options.items()}
    out = None
    try:
        if op == "edgeconv":
            i, B, Ns, Nd, rows = args
            src = rnd(B, Ns, 3, ecfg["feat_dim"][i - 1])
            knn = torch.from_numpy(rng.integers(0, Ns, (B, Nd, 16), dtype=np.int32)).to(dev)
            dst = torch.from_numpy(np.stack([rng.permutation(Ns)[:Nd] for _ in range(B)]).astype(np.int32)).to(dev) if rows else None
            marker(); out = m.edgeconv(i, src, knn, dst); marker()
        elif op == "encode":
            B, N = args
            x = rnd(B, 3, N)
            marker(); out = torch.cat([o.reshape(-1) for o in m.encode(x)]); marker()
        elif op == "lna":
            i, B, N = args
            f = rnd(B, N, 3, ecfg["feat_dim"][i])
            marker(); m.vn_lna_global(i, f); marker()
        elif op == "tail":
            B, NP = args
            f = rnd(B, NP, 3, ecfg["feat_dim"][-1])
            marker(); m.encoder_tail(f); marker()
        else:
            B, M = args
            c = ecfg["c_dim"]
            q, zs, zi, s, t = rnd(B, M, 3), rnd(B, c, 3), rnd(B, c), torch.ones(B, device=dev), torch.zeros(B, 3, device=dev)
            if op == "sdf_decode":
                marker(); m.sdf_decode(q, zs, zi, s, t, max_ws_bytes=1 << 40); marker()
            else:
                g = rnd(B, M)
                marker()
                sdf, saved = m.sdf_decode_train(q, zs, zi, s, t)
                m.sdf_backward(saved, g)
                marker()
    finally:
        for k, v in prev.items():
            m.set_option(getattr(_lib, k), v)
    torch.cuda.synchronize()
    return 0, hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest() if want_hash else None


# ------------------------------------------------------------------------------------------------ the edge-conv layers (--family edge)
ENCODE_B, ENCODE_N = 2, (1024, 1008, 512)   # 1024: table-free layers, column sums everywhere; 1008: Nd = 504 / 126 / 31; 512: layer 6 has 16 source points


def edge_ladder():
    """[(key, model, op, args, options)], the same in every mode.  (a) HipModel.edgeconv with LS_OPT_EDGE_FUSE_Q / _T each 0 and 1: the released
    layers 1 - 6 at B = 2 and one more B across the 16-tile edge of the table GEMM (K = 32 / 64: 3 B Ns / 128 = 12 | 24, 12 | 18); layers 5 / 6 with
    32 destination points of 128 sources + rows, of 32 sources without rows, and with 31; the small model's layers 2 (Co = 32: the generic
    attention kernel) and 3; layer 1 at 64 / 96 channels (edge_pool_v4_kernel<16>, the generic pool kernel).  (b) whole ls_encode calls."""
    shapes = [("released", 1, B, 512, 512) for B in (1, 2)] + [("released", 1, 2, 100, 100)]
    shapes += [("released", 2, B, 512, 256) for B in (1, 2)] + [("released", 2, 2, 500, 250)]
    shapes += [("released", 3, B, 512, 512) for B in (1, 2)]
    shapes += [("released", 4, B, 256, 64) for B in (2, 3)]
    for i in (5, 6):
        shapes += [("released", i, 2, 128, 32), ("released", i, 2, 32, 32), ("released", i, 2, 124, 31), ("released", i, 2, 31, 31)]
    shapes += [("small", 2, 2, 256, 128), ("small", 3, 2, 128, 128), ("pool64", 1, 2, 256, 256), ("pool96", 1, 2, 256, 256)]
    c = []
    for model, i, B, Ns, Nd in shapes:
        for fq in (0, 1):
            for ft in (0, 1):
                c.append((f"edgeconv({model}, layer={i}, B={B}, Ns={Ns}, Nd={Nd}, fuse_q={fq}, fuse_t={ft})", model, "edgeconv", (i, B, Ns, Nd, int(Ns != Nd)),
                          {"OPT_EDGE_FUSE_Q": fq, "OPT_EDGE_FUSE_T": ft}))
    c += [(f"encode(released, B={ENCODE_B}, N={N})", "released", "encode", (ENCODE_B, N), {}) for N in ENCODE_N]
    return c


def edge_traits(ecfg, mode, i, B, Ns, Nd, rows, fuse_q=1, fuse_t=1, encode=False, glob_fuse=1):
    """EdgeTraits (csrc/edge_plan.h) of layer i >= 1 of a handle built from ecfg.  The handle holds the destination-side / table-free planes
    where the header's two shape predicates say so (tests/tools/edge_plan_dump.cpp fills them in); the export wants no side products, an
    encode wants row maxima and (LS_OPT_GLOB_FUSE != 0) column sums from the layers with a residual global conv."""
    glob = bool(encode and i >= ecfg["res_global_start_layer"])
    return dict(mode=MODES.index(mode), attn=int(i >= ecfg["atten_start_layer"]), Cin=ecfg["feat_dim"][i - 1], Co=ecfg["feat_dim"][i],
                head_c=ecfg["atten_multi_head_c"], B=B, Ns=Ns, Nd=Nd, has_rows=int(rows), fuse_q=fuse_q, fuse_t=fuse_t, want_rowmax=int(glob),
                want_colsum=int(glob and glob_fuse))


# ------------------------------------------------------------------------------------------------ the k-NN builds (--family knn)
def knn_ladder():
    """[(key, case)]: case = the sizes of one ops.knn call with K = 16.  self: the queries are rows of the candidate set (dst is src; through
    dst_rows where Nd != Ns); otherwise dst is a set of its own of dst_n rows (rows: Nd of them through dst_rows).  Every shape with contract 0
    and 1 (LS_FLAG_CONTRACT_FMA)."""
    def case(B, Nd, Ns, C, self=0, dst_n=None, seeded=0, valu_only=0):
        dst_n = Ns if self else (dst_n or Nd)
        return dict(B=B, Nd=Nd, dst_n=dst_n, Ns=Ns, C=C, self=self, rows=int(dst_n != Nd), seeded=seeded, valu_only=valu_only)
    shapes = []
    # raw clouds (C = 1): one chunk of 1024 candidates | two; queries per wave 1 (7 queries), 16 (B cdiv(Nd, 64) = 1024), 8 (512)
    shapes += [case(2, 40, 1024, 1), case(2, 40, 1025, 1), case(1, 7, 100, 1), case(16, 4096, 100, 1), case(16, 2048, 100, 1)]
    # 32 | 33 queries: the small kernel against the fused one (C = 32 / 64) or the tile kernel (C = 128 / 256); seeded, 32 queries take the fused one
    shapes += [case(2, Nd, Ns, C) for C, Ns in ((32, 128), (64, 128), (128, 128), (256, 32)) for Nd in (32, 33)]
    shapes += [case(2, 32, 128, 32, seeded=1)]
    # the fused kernel's candidate tiles per wave: 8 | 9, 16 | 17, 24 | 25 tiles of 32; 1024 candidates still fused, 1025 tiled (17 tiles of 64: 16 splits asked,
    # 9 of two tiles run); 1000 pads to 1024; LS_FLAG_KNN_VALU_ONLY; one call with a destination set of its own (77 rows, 40 of them queried)
    for C in (32, 64):
        shapes += [case(2, 40, Ns, C, self=1) for Ns in (256, 257, 512, 513, 768, 769, 1024, 1025, 1000)]
        shapes += [case(2, 40, 300, C, self=1, valu_only=1)]
    shapes += [case(2, 40, 300, 32, dst_n=77)]
    # the tile kernel (C = 96): one candidate tile | two (two splits); 18 tiles on 2 workgroups: 16 splits asked, 9 of two tiles run; 512 workgroups: never
    # split; 510 and 256: cdiv(256, workgroups) = 1, not split either; 254: two splits; seeded with LS_FLAG_KNN_VALU_ONLY: hints, and the merge drops what
    # it meets twice
    shapes += [case(2, 33, 64, 96), case(2, 33, 65, 96), case(1, 70, 1100, 96), case(256, 128, 130, 96), case(255, 128, 130, 96), case(128, 128, 130, 96),
               case(127, 128, 130, 96), case(2, 70, 130, 64, seeded=1, valu_only=1)]
    c = []
    for s in shapes:
        for contract in (0, 1):
            d = dict(s, contract=contract)
            c.append(("knn(" + ", ".join(f"{k}={v}" for k, v in d.items() if v or k in ("B", "Nd", "Ns", "C", "contract")) + ")", d))
    assert len({k for k, _ in c}) == len(c)
    return c


def knn_traits(case, has_scratch=1):
    """KnnTraits (csrc/knn_plan.h) of a knn_ladder() case.  ops.knn hands over the workspace the sizing call asks for; where that is nothing,
    no choice depends on it."""
    return dict(B=case["B"], Nd=case["Nd"], dst_n=case["dst_n"], Ns=case["Ns"], C=case["C"], K=16, fma=case["contract"], valu_only=case["valu_only"],
                seeded=case["seeded"], self=case["self"], has_scratch=has_scratch)


def knn_inputs(key, case):
    """numpy (dst or None for self, src, dst_rows or None, seeds or None, the query rows [B][Nd][3][C] for the oracle): the conventions of
    test_knn_bit_exact -- candidate 7 of instance 0 repeats candidate 2 (a tie: the lower index wins), its query 0 is that row (distance 0)."""
    import numpy as np
    B, Nd, dst_n, Ns, C = (case[k] for k in ("B", "Nd", "dst_n", "Ns", "C"))
    rng = np.random.default_rng(_seed(key))
    src = rng.standard_normal((B, Ns, 3, C)).astype(np.float32)
    src[0, 7] = src[0, 2]
    dst = None if case["self"] else rng.standard_normal((B, dst_n, 3, C)).astype(np.float32)
    rows = np.stack([rng.permutation(dst_n)[:Nd] for _ in range(B)]).astype(np.int32) if case["rows"] else None
    if case["self"]:
        if rows is not None:
            rows[0, 0] = 2
    else:
        dst[0, rows[0, 0] if rows is not None else 0] = src[0, 2]
    seeds = None
    if case["seeded"]:     # hints: in and out of range, one repeated; a result never depends on them
        seeds = rng.integers(-3, Ns + 5, (B, Nd, 16)).astype(np.int32)
        seeds[:, :, 1] = seeds[:, :, 0]
    from_set = src if case["self"] else dst
    q = from_set if rows is None else np.stack([from_set[b][rows[b]] for b in range(B)])
    return dst, src, rows, seeds, q


def knn_call(case, dst, src, rows, seeds):
    """ops.knn on the current device -> (idx, dist) as numpy."""
    import torch
    from livingscenes_amd import _lib, ops
    dev = torch.device("cuda:0")
    up = lambda a: None if a is None else torch.from_numpy(a).to(dev)
    s = up(src)
    d = s if dst is None else up(dst)
    flags = (_lib.FLAG_CONTRACT_FMA if case["contract"] else 0) | (_lib.FLAG_KNN_VALU_ONLY if case["valu_only"] else 0)
    idx, dist = ops.knn(d, s, 16, dst_rows=up(rows), flags=flags, return_dist=True, seeds=up(seeds))
    return idx.cpu().numpy(), dist.cpu().numpy()


def knn_sha(idx, dist):
    return hashlib.sha256(idx.tobytes() + dist.tobytes()).hexdigest()


def run_knn(key, case):
    dst, src, rows, seeds, _ = knn_inputs(key, case)
    marker()
    idx, dist = knn_call(case, dst, src, rows, seeds)      # (the copies back to the host synchronise: the closing marker comes after the case's launches)
    marker()
    return 0, knn_sha(idx, dist)


# ------------------------------------------------------------------------------------------------ worker (under the trace) and collector
def cases_of(mode, family="gemm"):
    """[(key, traits, runner)] of one mode's process, in launch order: the public ladder, then the model ladder (edge: edge_ladder())."""
    if family == "edge":
        return [(k, None, ("model", k, mdl, op, a, o, True)) for k, mdl, op, a, o in edge_ladder()]
    if family == "knn":
        return [(k, None, ("knn", k, c)) for k, c in knn_ladder()]
    out = [(k, [t], ("public", k, e, t)) for k, e, t in ladder()]
    out += [(k, tr, ("model", k, mdl, op, a, o)) for k, mdl, op, a, o, tr in model_ladder(mode)]
    return out


def check_edge_hashes(mode):
    """Run edge_ladder() in this process (which must be in arithmetic mode `mode`) -> {key: (recorded, now)} of the outputs that differ."""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    want, models, wrong = load("edge"), {}, {}
    try:
        for key, _, run in cases_of(mode, "edge"):
            sha = run_model(models, *run[1:])[1]
            if want[f"{mode}:{key}"]["sha256"] not in (None, sha):      # (None: the case was not reproducible when it was recorded)
                wrong[key] = (want[f"{mode}:{key}"]["sha256"], sha)
    finally:
        for _, m in models.values():
            m.close()
    return wrong


def worker(mode, sidecar, family):
    import torch
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    models, rec = {}, []
    for key, traits, run in cases_of(mode, family):
        if run[0] == "public":
            status, sha = run_public(*run[1:])
        elif run[0] == "knn":
            status, sha = run_knn(*run[1:])
        else:
            status, sha = run_model(models, *run[1:])
        rec.append({"key": key, "status": status, "sha256": sha})
        torch.cuda.synchronize()
    for _, m in models.values():
        m.close()
    with open(sidecar, "w") as f:
        json.dump(rec, f)


def kernel_name(full):
    """Demangled name up to the parameter list, without the return type: 'ls::gemm_f32_kernel<true, 22>'."""
    s = full.strip()
    if s.endswith(" [clone .kd]"):
        s = s[:-len(" [clone .kd]")]
    if s.endswith(".kd"):
        s = s[:-3]
    if s.endswith(")"):
        depth = 0
        for i in range(len(s) - 1, -1, -1):
            depth += (s[i] == ")") - (s[i] == "(")
            if depth == 0:
                s = s[:i]
                break
    return s[5:] if s.startswith("void ") else s


def read_trace(outdir):
    files = glob.glob(os.path.join(outdir, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, f"expected one kernel trace under {outdir}: {files}"
    with open(files[0], newline="") as f:
        rows = list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    return [[kernel_name(r["Kernel_Name"]), [int(r["Grid_Size_X"]), int(r["Grid_Size_Y"]), int(r["Grid_Size_Z"])],
             [int(r["Workgroup_Size_X"]), int(r["Workgroup_Size_Y"]), int(r["Workgroup_Size_Z"])], int(r["LDS_Block_Size"])] for r in rows]


def is_marker(l):
    return l[0] == "ls::gemm_rowmax_kernel" and l[1][0] == cdiv(MARKER_ROWS, 4) * 256


def is_gemm(l):
    return l[0].startswith("ls::gemm_") and not l[0].startswith(("ls::gemm_rowmax_kernel", "ls::gemm_presplit_w_kernel"))


def is_edge(l):
    return l[0].startswith(("ls::edge_", "ls::glob_mean_gemv_kernel", "ls::mean_points_kernel"))


def is_knn(l):
    return l[0].startswith("ls::knn_")


def segment(launches, ncases):
    """The launches between the 2 k-th and the 2 k + 1-st marker belong to case k."""
    marks = [i for i, l in enumerate(launches) if is_marker(l)]
    assert len(marks) == 2 * ncases, f"{len(marks)} marker launches in the trace, {2 * ncases} expected"
    return [launches[marks[2 * k] + 1:marks[2 * k + 1]] for k in range(ncases)]


def record(family="gemm", timeout=600):
    cases = {}
    for mode in (MODES[:1] if family == "knn" else MODES):
        with tempfile.TemporaryDirectory(prefix="ls_gemm_trace_") as tmp:
            sidecar = os.path.join(tmp, "cases.json")
            env = dict(os.environ)
            env.pop("LS_GEMM_MODE", None)
            if mode != MODES[0]:
                env["LS_GEMM_MODE"] = mode
            cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", os.path.join(tmp, "trace"), "--",
                   sys.executable, os.path.abspath(__file__), "--worker", mode, "--sidecar", sidecar, "--family", family]
            subprocess.run(cmd, check=True, env=env, cwd=REPO, timeout=timeout)
            with open(sidecar) as f:
                rec = json.load(f)
            for r, launches in zip(rec, segment(read_trace(os.path.join(tmp, "trace")), len(rec))):
                c = cases[f"{mode}:{r['key']}"] = {"status": r["status"], "launches": [l for l in launches if is_gemm(l)], "sha256": r["sha256"]}
                if family == "knn":
                    c["launches"] = [l for l in launches if is_knn(l)]
                if family == "edge":
                    c["launches"] = [l for l in launches if is_edge(l)]
                    if r["key"].startswith("encode("):
                        c["launches"].sort()
                    else:
                        c["tables"] = sum(1 for l in launches if is_gemm(l))
        print(f"mode {mode}: {len(rec)} cases", flush=True)
    return cases


def dump(cases, path, units=UNITS):
    """{"mode:key": {status, launches, sha256[, tables]}} -> the file: one line per case key, the modes side by side, kernels by index."""
    kernels = sorted({(l[0], tuple(l[2]), l[3]) for v in cases.values() for l in v["launches"]})
    out = {}
    for mk, v in cases.items():
        mode, key = mk.split(":", 1)
        c = out.setdefault(key, {})
        assert all(l[1][2] == 1 for l in v["launches"]), mk
        c[mode] = [[kernels.index((l[0], tuple(l[2]), l[3])), l[1][0], l[1][1]] for l in v["launches"]]
        if v["sha256"]:
            c.setdefault("sha256", {})[mode] = v["sha256"]
        if v["status"]:
            c.setdefault("status", {})[mode] = v["status"]
        if "tables" in v:
            c.setdefault("tables", {})[mode] = v["tables"]
    js = lambda v: json.dumps(v, sort_keys=True, separators=(",", ":"))
    with open(path, "w") as f:
        f.write('{"units": ' + json.dumps(units, sort_keys=True, indent=1) + ',\n"kernels": [\n')
        f.write(",\n".join(js([k[0], list(k[1]), k[2]]) for k in kernels) + '],\n"cases": {\n')
        f.write(",\n".join(json.dumps(k) + ":" + js(v) for k, v in sorted(out.items())))
        f.write("\n}}\n")


def load(family="gemm", path=None):
    """The file -> {"mode:key": {status, launches, sha256[, tables]}} as record() returns it."""
    with open(path or GOLDENS[family]) as f:
        rec = json.load(f)
    cases = {}
    for key, c in rec["cases"].items():
        for mode in MODES:
            if mode in c:
                launches = [[rec["kernels"][k][0], [gx, gy, 1], rec["kernels"][k][1], rec["kernels"][k][2]] for k, gx, gy in c[mode]]
                cases[f"{mode}:{key}"] = {"status": c.get("status", {}).get(mode, 0), "launches": launches, "sha256": c.get("sha256", {}).get(mode)}
                if "tables" in c:
                    cases[f"{mode}:{key}"]["tables"] = c["tables"][mode]
    return cases


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--worker", choices=MODES)
    ap.add_argument("--sidecar")
    ap.add_argument("--family", choices=sorted(GOLDENS), default="gemm")
    ap.add_argument("--check-hashes", choices=MODES, help="compare the small public cases' outputs with the record (the process is in that mode)")
    a = ap.parse_args()
    if a.check_hashes:
        bad = check_edge_hashes(a.check_hashes) if a.family == "edge" else check_hashes(a.check_hashes)
        print(f"{len(bad)} cases differ from the record (recorded, now): {dict(list(bad.items())[:6])}")
        sys.exit(1 if bad else 0)
    elif a.worker:
        worker(a.worker, a.sidecar, a.family)
    else:
        rec = record(a.family)
        dump(rec, a.out or GOLDENS[a.family], {"edge": EDGE_UNITS, "knn": KNN_UNITS}.get(a.family, UNITS))
        print(f"{len(rec)} cases -> {a.out or GOLDENS[a.family]}")
