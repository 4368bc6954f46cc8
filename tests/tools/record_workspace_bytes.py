"""Record what every ls_*_workspace_bytes / ls_*_state_bytes query returns on a fixed ladder of arguments.

    python tests/tools/record_workspace_bytes.py            -> tests/golden/workspace_bytes.json        (host arithmetic: no GPU needed)
    python tests/tools/record_workspace_bytes.py --model    -> tests/golden/workspace_bytes_model.json  (queries on a live model handle: GPU)
    (--out PATH writes elsewhere)

The sizes are part of the library's contract with its callers ("the library never allocates behind an operator call": the caller allocates
what the query says, the operator cuts exactly that up).  A change to how an operator lays its workspace out must not move them, so they are
recorded from the library BEFORE such a change and tests/test_workspace_bytes_cpu.py / tests/test_hip_workspace.py compare the library with
the record afterwards.  Re-record only when a size is meant to change.

A record is {"query(arg, arg, ...)": bytes}; ladder() / model_ladder() are the one statement of the cases, shared with the tests."""
import argparse
import itertools
import json
import os
import sys

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
GOLDEN = os.path.join(REPO, "tests", "golden")

LS_FLAG_KNN_VALU_ONLY = 4
INT_MAX = 2 ** 31 - 1
MATCH_BATCH = ("ls_cosine_scores_batch_workspace_bytes", "ls_greedy_match_batch_workspace_bytes", "ls_nn_match_batch_workspace_bytes",
               "ls_sinkhorn_match_batch_workspace_bytes", "ls_kabsch_residual_matrix_batch_workspace_bytes")


def ladder():
    """[(query name, argument tuple)]: the model-free queries, their refusal cases (arguments they answer with 0) included."""
    c = []
    # ---- k-NN (B, Nd, dst_n, Ns, C, seeded, flags): both kernels' layouts (sweep: C = 32 / 64 and Ns <= 1024), self and cross sets
    for C, Ns, Nd, B, seeded, flags in itertools.product((1, 32, 64, 128), (32, 128, 512, 1024, 2048, 4096), (32, 512), (1, 64), (0, 1),
                                                         (0, LS_FLAG_KNN_VALU_ONLY)):
        c.append(("ls_knn_workspace_bytes", (B, Nd, Ns, Ns, C, seeded, flags)))
    for C, Ns, dst_n in itertools.product((32, 64), (33, 1000, 1024, 1025), (1, 31, 777)):
        c.append(("ls_knn_workspace_bytes", (3, min(dst_n, 40), dst_n, Ns, C, 0, 0)))
    for bad in ((0, 32, 32, 32, 32, 0, 0), (1, 0, 32, 32, 32, 0, 0), (1, 32, 0, 32, 32, 0, 0), (1, 32, 32, 0, 32, 0, 0), (-1, 32, 32, 32, 32, 0, 0)):
        c.append(("ls_knn_workspace_bytes", bad))
    # ---- FPS (B, N, K): the bucket scratch starts above 8192 points
    for N, B in itertools.product((128, 8192, 8193, 60000), (1, 3, 64)):
        c.append(("ls_fps_workspace_bytes", (B, N, 512)))
    c += [("ls_fps_workspace_bytes", a) for a in ((0, 128, 8), (1, 0, 8), (-1, 9000, 8), (1, -5, 8))]
    # ---- GEMM (M, N, K): split-K slabs only for under-filled, long-K problems
    for a in ((192, 1024, 512), (4, 4, 8), (1024, 1024, 512), (96, 260, 512), (3, 2048, 512), (192, 1024, 96), (96, 258, 512), (192, 1024, 510),
              (0, 4, 8), (4, 0, 8), (4, 4, 0), (-1, 4, 8)):
        c.append(("ls_gemm_workspace_bytes", a))
    for a in ((768, 768), (768, 256), (64, 520), (0, 768), (768, 0)):
        c.append(("ls_gemm_w_planes_bytes", a))
    # ---- matchers: the single cosine op, and the five ragged batches (P, n_total, m_total)
    for a in ((32, 32), (1, 1), (200, 3), (0, 5), (5, 0), (-1, 5)):
        c.append(("ls_cosine_scores_workspace_bytes", a))
    for name in MATCH_BATCH:
        for P, (nt, mt) in itertools.product((1, 3, 200), ((0, 0), (39, 18), (64, 64), (1000, 777), (0, 5), (5, 0))):
            c.append((name, (P, nt, mt)))
        c += [(name, a) for a in ((0, 4, 4), (-2, 4, 4), (1, -1, 4), (1, 4, -1))]
    c += [("ls_icp_workspace_bytes", a) for a in ((1, 1), (4, 1000), (0, 0))]
    # ---- MISE octrees (res0, depth) and batches of them (B, res0, depth)
    mise = ((1, 0), (2, 1), (16, 3), (32, 2), (32, 3), (3, 2), (1, 7))
    mise_bad = ((0, 0), (1, 8), (1, -1), (2048, 0), (16, 7), (-4, 2))
    c += [("ls_mise_state_bytes", a) for a in mise + mise_bad]
    for B, rd in itertools.product((1, 3, 16), mise + mise_bad):
        c.append(("ls_mise_batch_state_bytes", (B,) + rd))
    c += [("ls_mise_batch_state_bytes", a) for a in ((0, 2, 1), (-1, 2, 1), (65535, 1, 0), (65536, 1, 0), (16, 32, 5), (2, 32, 5), (1, 32, 5))]
    # ---- marching cubes (nx, ny, nz) and (B, nx, ny, nz): a volume without a cube keeps its 256 bytes
    vols = ((2, 2, 2), (1, 5, 5), (5, 1, 5), (5, 5, 1), (33, 33, 33), (17, 9, 65), (129, 129, 129), (0, 4, 4))
    c += [("ls_mcubes_workspace_bytes", v) for v in vols]
    for B, v in itertools.product((1, 3, 16), vols):
        c.append(("ls_mcubes_batch_workspace_bytes", (B,) + v))
    c += [("ls_mcubes_batch_workspace_bytes", a) for a in ((0, 9, 9, 9), (65535, 2, 2, 2), (65536, 2, 2, 2), (1, 2048, 2048, 2048), (100, 129, 129, 129),
                                                            (1, 9, 9, -1), (66, 129, 129, 129), (67, 129, 129, 129))]
    # ---- mesh metrics: one mesh (nf[, hash_resolution]) and ragged batches (M, nf_total[, hash_resolution])
    for nf, R in itertools.product((0, 1, 1000, 100000), (2, 64, 512, 4096)):
        c.append(("ls_mesh_contains_workspace_bytes", (nf, R)))
    c += [("ls_mesh_contains_workspace_bytes", a) for a in ((-1, 64), (10, 1), (10, 4097), (10, 0))]
    for nf in (0, 1, 1000, 100000, 4097, -1):
        c.append(("ls_mesh_distance_workspace_bytes", (nf,)))
        c.append(("ls_mesh_sample_workspace_bytes", (nf,)))
    for M, nf in itertools.product((0, 1, 3, 64), (0, 1000, 123457)):
        for R in (2, 512):
            c.append(("ls_mesh_contains_batch_workspace_bytes", (M, nf, R)))
        c.append(("ls_mesh_distance_batch_workspace_bytes", (M, nf)))
        c.append(("ls_mesh_sample_batch_workspace_bytes", (M, nf)))
    c += [("ls_mesh_contains_batch_workspace_bytes", a) for a in ((-1, 10, 64), (2, -1, 64), (2, INT_MAX + 1, 64), (2, 10, 1), (2, 10, 4097))]
    for name in ("ls_mesh_distance_batch_workspace_bytes", "ls_mesh_sample_batch_workspace_bytes"):
        c += [(name, a) for a in ((-1, 10), (2, -1), (2, INT_MAX + 1))]
    # ---- mesh clustering (nv, nf, r_max) and (M, nv_total, nf_total, r_max)
    meshes = ((0, 0, 1), (1, 1, 256), (100, 200, 16), (5000, 10000, 256), (123457, 246913, 64), (4097, 0, 3))
    meshes_bad = ((-1, 10, 16), (10, -1, 16), (INT_MAX, 1, 16), (10, 10, 0), (10, 10, 257))
    c += [("ls_mesh_cluster_workspace_bytes", a) for a in meshes + meshes_bad]
    for M, a in itertools.product((1, 3, 64), meshes + meshes_bad):
        c.append(("ls_mesh_cluster_batch_workspace_bytes", (M,) + a))
    c += [("ls_mesh_cluster_batch_workspace_bytes", a) for a in ((0, 10, 10, 16), (-1, 10, 10, 16))]
    # ---- registration metrics (P, n_total, m_total, chamfer_stride)
    for P, (nt, mt), s in itertools.product((1, 3, 200), ((0, 0), (200, 200), (5000, 1024), (123457, 99999)), (1, 10)):
        c.append(("ls_reg_metrics_batch_workspace_bytes", (P, nt, mt, s)))
    c += [("ls_reg_metrics_batch_workspace_bytes", a) for a in ((0, 10, 10, 1), (1, -1, 10, 1), (1, 10, -1, 1), (1, 10, 10, 0))]
    return c


def key(name, args):
    return f"{name}({', '.join(str(int(a)) for a in args)})"


def record():
    from livingscenes_amd import _lib, build
    build.build()
    lib = _lib.load()
    return {key(n, a): int(getattr(lib, n)(*a)) for n, a in ladder()}


# ------------------------------------------------------------------------------------------------ queries on a model handle
MODELS = ("released", "small")          # synth.default_* (the released widths) and synth.small_* (the tests' small model), encoder + decoder
MODEL_B, MODEL_N = (1, 3, 64), (256, 1024)


def model_cfgs(which):
    from livingscenes_amd import synth
    return (synth.default_encoder_cfg(), synth.default_decoder_cfg()) if which == "released" else (synth.small_encoder_cfg(), synth.small_decoder_cfg())


def layer_sizes(ecfg, N):
    """[(Ns, Nd, has_rows)] of every encoder layer at N input points (a down-sampling layer selects its destination points by FPS rows)."""
    out, cur = [], N
    for i in range(ecfg["num_layers"]):
        ns = cur
        if i in ecfg["down_sample_layers"]:
            cur //= ecfg["down_sample_factor"][ecfg["down_sample_layers"].index(i)]
        out.append((ns, cur, int(cur != ns)))
    return out


def model_ladder(ecfg):
    """[(query name, argument tuple after the handle)] for one model."""
    c = []
    L, g0 = ecfg["num_layers"], ecfg["res_global_start_layer"]
    for B, N in itertools.product(MODEL_B, MODEL_N):
        sizes = layer_sizes(ecfg, N)
        c.append(("ls_encoder_workspace_bytes", (B, N)))
        for i, (ns, nd, rows) in enumerate(sizes):
            c.append(("ls_vn_edgeconv_workspace_bytes", (i, B, ns, nd, rows)))
            if i >= g0:
                c.append(("ls_vn_lna_workspace_bytes", (i, B, nd)))
        c.append(("ls_encoder_tail_workspace_bytes", (B, sizes[-1][1])))
        c.append(("ls_sdf_workspace_bytes", (B, N)))
        c.append(("ls_sdf_rows_workspace_bytes", (B, B * N - 7)))
        c.append(("ls_sdf_train_workspace_bytes", (B, N)))
    # refusals (not ls_encoder_workspace_bytes at B = 0: before the arena that query divided by zero on the host, so no size was recorded)
    c += [("ls_encoder_workspace_bytes", (1, 8)), ("ls_vn_edgeconv_workspace_bytes", (L, 1, 32, 32, 0)),
          ("ls_vn_edgeconv_workspace_bytes", (-1, 1, 32, 32, 0)), ("ls_vn_edgeconv_workspace_bytes", (1, 0, 32, 32, 0)),
          ("ls_vn_lna_workspace_bytes", (g0 - 1, 1, 32)), ("ls_vn_lna_workspace_bytes", (L, 1, 32)), ("ls_vn_lna_workspace_bytes", (g0, 0, 32)),
          ("ls_vn_lna_workspace_bytes", (g0, 1, 0)), ("ls_encoder_tail_workspace_bytes", (0, 32)), ("ls_encoder_tail_workspace_bytes", (1, 0))]
    return c


def make_model(which):
    import torch
    from livingscenes_amd import ops, packing, synth
    ecfg, dcfg = model_cfgs(which)
    desc, blob = packing.pack_model(synth.make_encoder_weights(ecfg, 0), ecfg, synth.make_decoder_weights(dcfg, 0), dcfg)
    return ecfg, ops.HipModel(desc, blob, torch.device("cuda:0"))


def record_model():
    from livingscenes_amd import _lib
    lib, out = _lib.load(), {}
    for which in MODELS:
        ecfg, m = make_model(which)
        for n, a in model_ladder(ecfg):
            out[which + ":" + key(n, a)] = int(getattr(lib, n)(m._h, *a))
        m.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    path = a.out or os.path.join(GOLDEN, "workspace_bytes_model.json" if a.model else "workspace_bytes.json")
    rec = record_model() if a.model else record()
    with open(path, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(rec)} sizes -> {path} ({sum(1 for v in rec.values() if v == 0)} refusals)")
