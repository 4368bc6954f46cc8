"""CPU-only tests (-m "not gpu"): the C-ABI library loads and exports every symbol include/livingscenes_hip.h
declares (no compute without a GPU), the host-side mirrors keep the reference's names / state_dict keys, weight
packing is consistent, the product path refuses to run without a HIP device, and the world_size-2 sharding path
works over gloo."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from livingscenes_amd import synth

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN_DIR = os.path.join(REPO, "tests", "golden")


@pytest.fixture(scope="module")
def lib():
    from livingscenes_amd import _lib, build
    build.build()  # hipcc cross-compiles for gfx950 without a GPU
    return _lib.load()


def test_abi_exports_every_declared_symbol(lib):
    hdr = open(os.path.join(REPO, "include", "livingscenes_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(ls_[a-z0-9_]+)\s*\(", hdr))
    from livingscenes_amd import _lib
    assert declared == set(_lib.SIGNATURES), (declared ^ set(_lib.SIGNATURES))
    for name in declared:
        assert hasattr(lib, name), f"{name} not exported"
    assert lib.ls_version() >= 100


def test_abi_table_types_match_the_header_prototypes():
    """_lib.SIGNATURES is transcribed by hand from include/livingscenes_hip.h; the test above compares names only.  A `long long` or a `size_t`
    typed as `int` in the table would load, pass every call that stays below 2^31 and corrupt the arguments after it silently -- so every
    prototype's return and argument types are parsed from the header and compared with the table: pointers (arrays, handles, strings as
    arguments) are c_void_p or a typed ctypes pointer, scalars the ctypes type of the same C type."""
    from livingscenes_amd import _lib
    hdr = open(os.path.join(REPO, "include", "livingscenes_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    hdr = re.sub(r"//[^\n]*", "", hdr)
    protos = re.findall(r"([A-Za-z_][\w \*]*?)\b(ls_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", hdr)
    scalars = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "unsigned int": ctypes.c_uint, "float": ctypes.c_float, "double": ctypes.c_double,
               "long long": ctypes.c_longlong, "size_t": ctypes.c_size_t, "unsigned long long": ctypes.c_ulonglong}

    def of_header(decl, is_return=False):
        """the C declaration of one parameter (its name included) or of the return type -> a ctypes type code, 'P' for every pointer"""
        t = " ".join(re.sub(r"\bconst\b", " ", decl).replace("*", " * ").split())
        if t.endswith("]"):
            return "P"
        if not is_return:
            t = re.sub(r"\s*\b[A-Za-z_]\w*$", "", t)   # every parameter of the header is named: drop the name
        if "*" in t:
            return "z" if is_return and t == "char *" else "P"
        return None if t == "void" else scalars[t]._type_

    def of_table(c):
        if c is None:
            return None
        if isinstance(c, type) and issubclass(c, ctypes._Pointer):
            return "P"
        return c._type_

    assert len(protos) == len(_lib.SIGNATURES) and {p[1] for p in protos} == set(_lib.SIGNATURES)
    wrong = []
    for ret, name, args in protos:
        args = args.strip()
        want_args = [] if args in ("", "void") else [of_header(a) for a in args.split(",")]
        res, argtypes = _lib.SIGNATURES[name]
        if (of_header(ret, True), want_args) != (of_table(res), [of_table(a) for a in argtypes]):
            wrong.append((name, of_header(ret, True), want_args, of_table(res), [of_table(a) for a in argtypes]))
    assert not wrong, wrong
    # the parser tells the widths apart (the test would be empty otherwise)
    assert of_header("long long n") != of_header("int n") and of_header("size_t workspace_bytes") != of_header("int n")
    assert of_header("const long long* off") == "P" and of_header("ls_model_t** out") == "P" and of_header("unsigned flags") == "I"


def test_abi_fails_loudly_without_device(lib):
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    assert lib.ls_device_count() < 0
    assert b"device" in lib.ls_last_error().lower()
    from livingscenes_amd import _lib, ops
    with pytest.raises(_lib.LsError, match="no CPU fallback"):
        ops.knn(torch.zeros(1, 16, 3, 1), torch.zeros(1, 16, 3, 1))
    with pytest.raises(_lib.LsError):
        ops.HipModel(None, None, "cpu")


def test_argument_validation_without_device(lib):
    # shape checks happen on the host before any launch
    P = ctypes.c_void_p
    assert lib.ls_knn_f32(P(16), P(16), None, None, 1, 8, 8, 8, 5, 16, 0, P(16), None, None, 0, None) == -1
    assert b"multiple of 32" in lib.ls_last_error()
    assert lib.ls_knn_f32(P(16), P(16), None, None, 1, 8, 8, 8, 32, 17, 0, P(16), None, None, 0, None) == -1
    assert lib.ls_gemm_f32(P(16), 6, P(16), 8, None, P(16), 8, 4, 4, 6, 0, None, 0, None) == -1
    # the library never allocates scratch behind an operator call: a missing / short caller workspace is an error, not a hipMalloc
    need = lib.ls_knn_workspace_bytes(4, 512, 512, 512, 64, 0, 0)
    assert need > 0 and lib.ls_knn_f32(P(16), P(16), None, None, 4, 512, 512, 512, 64, 16, 0, P(16), None, P(16), need - 1, None) == -3
    assert b"workspace" in lib.ls_last_error()
    gneed = lib.ls_gemm_workspace_bytes(192, 1024, 512)
    assert gneed > 0 and lib.ls_gemm_f32(P(16), 512, P(16), 512, None, P(16), 1024, 192, 1024, 512, 0, None, 0, None) == -3
    assert lib.ls_cosine_scores_workspace_bytes(32, 32) == 64 * 4
    assert lib.ls_cosine_scores_f32(P(16), P(16), 32, 32, 256, P(16), None, 0, None) == -3
    assert lib.ls_fps_f32(P(16), None, 1, 100000, 8, 0, P(16), None, None, 0, None) == -1
    assert b"too large" in lib.ls_last_error()
    # pre-split weight planes: only where a kernel reads them (K >= 512, K % 32 == 0), the caller's buffer is checked, planes need their maxima
    assert lib.ls_gemm_w_planes_bytes(768, 768) == 4 * 768 * 768 and lib.ls_gemm_w_planes_bytes(768, 256) == 0 and lib.ls_gemm_w_planes_bytes(64, 520) == 0
    assert lib.ls_gemm_presplit_w_f32(P(16), 768, 768, 768, P(16), P(16), 4 * 768 * 768 - 1, None) == -3
    assert lib.ls_gemm_presplit_w_f32(P(16), 256, 64, 256, P(16), P(16), 1 << 20, None) == -1
    assert lib.ls_gemm_f32_planes(P(16), 768, P(16), 768, P(16), None, P(16), 768, 4, 768, 768, 0, None, 0, None, None, None) == -1
    assert b"w_rowmax" in lib.ls_last_error()


def test_module_mirrors_keep_reference_state_dict_keys():
    from livingscenes_amd.deepsdf_decoder import DeepSDF_Decoder
    from livingscenes_amd.vec_dgcnn_atten import VecDGCNN_att
    ecfg, dcfg = synth.default_encoder_cfg(), synth.default_decoder_cfg()
    enc, dec = VecDGCNN_att(**ecfg), DeepSDF_Decoder(**dcfg)
    assert set(enc.state_dict().keys()) == set(synth.encoder_param_shapes(ecfg).keys())
    assert sum(p.numel() for p in enc.parameters()) == 3255009      # SURVEY.md section 8 [probe]
    assert sum(p.numel() for p in dec.parameters()) == 4140799
    enc.load_state_dict(synth.make_encoder_weights(ecfg, 0), strict=True)
    dec.load_state_dict(synth.make_decoder_weights(dcfg, 0), strict=True)
    ck = synth.to_checkpoint(enc.state_dict(), dec.state_dict())
    assert all(k.startswith(("network_dict.encoder.", "network_dict.decoder.")) for k in ck["model_state_dict"])
    with pytest.raises(Exception):
        enc(torch.zeros(1, 3, 64))  # CPU tensor -> loud failure, never a silent fallback


def test_shape_prior_checkpoint_roundtrip(tmp_path):
    """Shape_Prior.__init__ reads the reference's checkpoint / yaml layout (model_utils.py:85-128)."""
    import yaml
    from livingscenes_amd.model_utils import Shape_Prior, load_ckpt_from_log
    ecfg, dcfg = synth.small_encoder_cfg(), synth.small_decoder_cfg()
    ew, dw = synth.make_encoder_weights(ecfg, 3), synth.make_decoder_weights(dcfg, 3)
    (tmp_path / "checkpoint").mkdir()
    (tmp_path / "files_backup").mkdir()
    torch.save(synth.to_checkpoint(ew, dw, epoch=7), tmp_path / "checkpoint" / "x_latest.pt")
    field = {"model": {"encoder": ecfg, "decoder": dcfg, "encoder_type": "vecdgcnn_atten", "decoder_type": "inner_deepsdf",
                       "sdf2occ_factor": -1.0}, "dataset": {"n_pcl": 256}}
    (tmp_path / "files_backup" / "model_config.yaml").write_text(yaml.safe_dump(field))
    sp = Shape_Prior({"working_dir": "/", "field_cfg": str(tmp_path / "files_backup" / "model_config.yaml"),
                      "field_pt": str(tmp_path / "checkpoint" / "x_latest.pt")}, "chair", use_double=False)
    assert sp.field_input_n == 256 and sp.decoder.sdf2occ_factor == -1.0
    for k, v in ew.items():
        assert torch.equal(sp.encoder.state_dict()[k], v)
    for k, v in dw.items():
        assert torch.equal(sp.decoder.F.state_dict()[k], v)
    # use_double (model_utils.py:148-152): accepted -- the fp32 kernels run and the codes come back as float64 (tests/test_hip_surface.py)
    spd = Shape_Prior({"working_dir": "/", "field_cfg": str(tmp_path / "files_backup" / "model_config.yaml"),
                       "field_pt": str(tmp_path / "checkpoint" / "x_latest.pt")}, "chair", use_double=True)
    assert spd.use_double is True and sp.use_double is False
    room = tmp_path / "room.yaml"
    room.write_text(yaml.safe_dump({"shape_priors": {"chair": {}}, "solver_global": {"use_double": False}}))
    if not torch.cuda.is_available():
        with pytest.raises(Exception):  # load_ckpt_from_log moves the model to "cuda" like the reference (:280)
            load_ckpt_from_log(str(tmp_path), room_cfg=str(room))


def test_packing_folds_match_the_oracle_math():
    """The folded tables reproduce lin / lin_dir of the oracle's VecLNA on the edge feature (fp64 check)."""
    from livingscenes_amd import packing
    from oracle import net
    ecfg = synth.small_encoder_cfg()
    ew = synth.make_encoder_weights(ecfg, 5)
    desc, blob = packing.pack_model(ew, ecfg)
    i, cin, co = 2, ecfg["feat_dim"][1], ecfg["feat_dim"][2]
    Wt = torch.from_numpy(blob[desc.off_edge[i]: desc.off_edge[i] + 10 * co * cin].reshape(10 * co, cin)).double()
    g = torch.Generator().manual_seed(0)
    nbr, ctr = torch.randn(1, cin, 3, 1, 1, generator=g).double(), torch.randn(1, cin, 3, 1, 1, generator=g).double()
    E = torch.cat([nbr - ctr, ctr], 1)
    for br, name in ((0, "V_list"), (2, "K_list")):
        W, Wd = ew[f"{name}.{i}.lin.weight"].double(), ew[f"{name}.{i}.act.lin_dir.weight"].double()
        y = net.vec_linear(E, W)
        k = net.vec_linear(y, Wd)
        P, Q = Wt[br * co:(br + 2) * co], Wt[(4 + br) * co:(6 + br) * co]
        yy = net.vec_linear(nbr, P[:co]) + net.vec_linear(ctr, Q[:co])
        kk = net.vec_linear(nbr, P[co:]) + net.vec_linear(ctr, Q[co:])
        assert (yy - y).abs().max() < 1e-6 and (kk - k).abs().max() < 1e-6
    # decoder: weight-norm fold + code split of layer 0
    dcfg = synth.small_decoder_cfg()
    dw = synth.make_decoder_weights(dcfg, 5)
    desc, blob = packing.pack_model(ew, ecfg, dw, dcfg)
    W0 = net.fold_weight_norm(dw["lin0.weight_g"], dw["lin0.weight_v"]).double()
    lat, width = dcfg["latent_size"], dcfg["dims"][0]
    inv_t = blob[desc.off_dec_inv_t[0]: desc.off_dec_inv_t[0] + lat * width].reshape(lat, width)
    assert np.abs(inv_t.T - W0[:, :lat].numpy()).max() < 1e-6
    assert desc.dec_num_linear == len(dcfg["dims"]) + 1 and desc.dec_latent_in == dcfg["latent_in"][0]


def test_se3_and_metrics_match_golden(golden):
    from livingscenes_amd.lib_math import torch_se3
    from livingscenes_amd.lib_more import pose_estimation as pe
    g = golden("registration")
    T1, T2, x1 = torch.from_numpy(g["se3_T1"]), torch.from_numpy(g["se3_T2"]), torch.from_numpy(g["kab_x1"])
    assert torch.allclose(torch_se3.inverse(T1), torch.from_numpy(g["se3_inv"]), atol=1e-6)
    assert torch.allclose(torch_se3.concatenate(T1, T2), torch.from_numpy(g["se3_cat"]), atol=1e-6)
    assert torch.allclose(torch_se3.transform(T1, x1), torch.from_numpy(g["se3_tf"]), atol=1e-5)
    assert torch.allclose(torch_se3.Rt_to_SE3(torch.from_numpy(g["kab_R"]), torch.from_numpy(g["kab_t"])), T1, atol=1e-7)
    assert torch.allclose(pe.rotation_error(torch.from_numpy(g["kab_R"]), torch.from_numpy(g["kab_Rg"])), torch.from_numpy(g["rot_err"]), atol=1e-3)
    assert torch.allclose(pe.translation_error(torch.from_numpy(g["kab_t"]), torch.from_numpy(g["kab_tg"])), torch.from_numpy(g["trans_err"]), atol=1e-6)
    assert torch.allclose(pe.inverse_3d_transform(T1), torch.from_numpy(g["inv3d"]), atol=1e-6)
    x2 = torch.from_numpy(g["kab_x2"])
    assert torch.allclose(pe.compute_transformation_error(x1[:1], x2[:1], T1[:1], T2[:1]), torch.from_numpy(g["rmse"]), atol=1e-6)


def test_dropin_registers_reference_import_names():
    code = ("import sys; sys.path.insert(0, %r); from livingscenes_amd import dropin; dropin.install();"
            "from lib_more.more_solver import More_Solver; from lib_more.pose_estimation import *;"
            "from lib_more.matcher_new import sequential_matcher, eq_seq_matcher, sim3_seq_matcher, nn_matcher, sinkhorn_matcher;"
            "from lib_math import torch_se3; from model_utils import load_ckpt_from_log, Shape_Prior, slice_code_dict;"
            "assert callable(kabsch_transformation_estimation) and callable(rotation_error) and callable(transform) and callable(inverse);"
            "print('ok')") % REPO
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr[-2000:]


def test_balanced_assignment_evens_out_skewed_costs():
    """sharding.balanced_assignment (SURVEY 8e, configs[3]: 3RScan clouds of 1 k - 60 k raw points, FPS cost ~ P): a partition (every item once),
    identical on every rank, equal costs -> the block partition, skewed costs -> per-rank totals within 10 %% of the mean once a rank holds several
    items; the restore index undoes the rank-order concatenation."""
    import numpy as np
    import torch
    from livingscenes_amd import sharding
    for n, ws in ((0, 3), (5, 8), (64, 8), (7, 2)):
        a = sharding.balanced_assignment([1024] * n, ws)
        assert a == [list(range(*sharding.shard_range(n, r, ws))) for r in range(ws)]
    rng = np.random.default_rng(0)
    for ws in (2, 3, 8):
        costs = np.exp(rng.uniform(np.log(1e3), np.log(6e4), 40 * ws)).astype(int).tolist()       # log-uniform 1 k .. 60 k
        a = sharding.balanced_assignment(costs, ws)
        assert sorted(i for part in a for i in part) == list(range(len(costs))) and all(part == sorted(part) for part in a)
        assert a == sharding.balanced_assignment(list(costs), ws)
        loads = [sum(costs[i] for i in part) for part in a]
        assert max(loads) <= 1.1 * (sum(costs) / ws) and min(loads) >= 0.9 * (sum(costs) / ws), loads
        block = [sum(costs[i] for i in range(*sharding.shard_range(len(costs), r, ws))) for r in range(ws)]
        assert max(loads) <= max(block)
        inv = sharding.assignment_restore(a)
        flat = torch.tensor([i for part in a for i in part])
        assert torch.equal(flat[inv], torch.arange(len(costs)))
    # one dominant item: nothing can balance it, but nothing else rides with it
    a = sharding.balanced_assignment([60000, 1000, 1000, 1000, 1000], 2)
    assert a == [[0], [1, 2, 3, 4]]


def test_launcher_world_and_rank_cpu_sets(monkeypatch):
    """launch.py: WORLD_SIZE=1 alone is not a launcher; no --gpus adopts the launcher's world; an explicit mismatch is refused; the per-rank CPU
    sets are disjoint, follow the GPU's NUMA node, keep SMT siblings together and fall back to an even split where the node is unknown."""
    from livingscenes_amd import launch
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR"):
        monkeypatch.delenv(k, raising=False)
    assert launch.launcher_world() is None and launch.ensure_ranks(None, "x.py", []) == (1, 0, 0)
    monkeypatch.setenv("WORLD_SIZE", "1")
    assert launch.launcher_world() is None and launch.ensure_ranks(1, "x.py", []) == (1, 0, 0)
    monkeypatch.setenv("WORLD_SIZE", "8"); monkeypatch.setenv("RANK", "3"); monkeypatch.setenv("LOCAL_RANK", "3")
    assert launch.ensure_ranks(None, "x.py", []) == (8, 3, 3) and launch.ensure_ranks(8, "x.py", []) == (8, 3, 3)
    with pytest.raises(SystemExit):
        launch.ensure_ranks(4, "x.py", [])
    assert launch.parse_cpulist("0-3,8,10-11\n") == [0, 1, 2, 3, 8, 10, 11] and launch.format_cpulist([0, 1, 2, 3, 8, 10, 11]) == "0-3,8,10-11"
    nodes = [0, 0, 0, 0, 1, 1, 1, 1]
    node_cpus = {0: list(range(0, 64)) + list(range(128, 192)), 1: list(range(64, 128)) + list(range(192, 256))}
    core_of = {c: c % 128 for c in range(256)}
    sets = [launch.rank_cpus(r, 8, nodes, range(256), node_cpus, core_of) for r in range(8)]
    assert all(len(s) == 32 for s in sets) and len(set().union(*map(set, sets))) == 256
    assert all(set(sets[r]) <= set(node_cpus[nodes[r]]) for r in range(8))
    assert all({core_of[c] for c in s} == {c for c in s if c < 128} for s in sets)              # both hardware threads of a core with one rank
    loose = [launch.rank_cpus(r, 3, [None, None, None], range(12), {}) for r in range(3)]
    assert loose == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10, 11]]
    mixed = [launch.rank_cpus(r, 3, [0, None, 0], range(8), {0: [0, 1, 2, 3]}) for r in range(3)]
    assert mixed == [[0, 1], [4, 5, 6, 7], [2, 3]]
    assert launch.bind_rank(0, 1) == sorted(__import__("os").sched_getaffinity(0))


def test_shard_range_partitions():
    from livingscenes_amd import sharding
    for n in (0, 1, 7, 64, 65):
        for ws in (1, 2, 3, 8):
            spans = [sharding.shard_range(n, r, ws) for r in range(ws)]
            assert spans[0][0] == 0 and spans[-1][1] == n
            assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
            sizes = [hi - lo for lo, hi in spans]
            assert max(sizes) - min(sizes) <= 1


_GLOO_WORKER = r'''
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, %r)
from livingscenes_amd import sharding
from livingscenes_amd.vec_dgcnn_atten import VecDGCNN_att
from livingscenes_amd import synth
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%%d" %% int(sys.argv[1]), rank=int(sys.argv[2]), world_size=2)
rank = dist.get_rank()
cfg = synth.small_encoder_cfg()
enc = VecDGCNN_att(**cfg)
if rank == 0:
    enc.load_state_dict(synth.make_encoder_weights(cfg, 9))
else:
    for p in enc.parameters():
        p.data.zero_()
sharding.broadcast_weights(enc, src=0)
ref = synth.make_encoder_weights(cfg, 9)
assert all(torch.equal(enc.state_dict()[k], v) for k, v in ref.items()), "broadcast mismatch"
# codes: rank r owns a ragged block of 5 instances (3 + 2); every rank ends up with all 5 in order
n, C = 5, 8
g = torch.Generator().manual_seed(1)
full = {"z_so3": torch.randn(n, C, 3, generator=g), "z_inv": torch.randn(n, C, generator=g),
        "s": torch.rand(n, generator=g), "t": torch.randn(n, 1, 3, generator=g)}
lo, hi = sharding.shard_range(n)
mine = {k: v[lo:hi].clone() for k, v in full.items()}
counts = [sharding.shard_range(n, r, 2)[1] - sharding.shard_range(n, r, 2)[0] for r in range(2)]
allc = sharding.all_gather_codes(mine, counts)
assert all(torch.equal(allc[k], full[k]) for k in full), "all_gather mismatch"
got = sharding.gather_codes(mine, dst=0, counts=counts)
assert (got is None) == (rank != 0)
if rank == 0:
    assert all(torch.equal(got[k], full[k]) for k in full)
# fewer instances than ranks (ADVICE r1): rank 1's shard is EMPTY -- it must neither call encode (ls_encode rejects B = 0) nor
# skip the collective (the other rank would block forever)
class _Stub:
    class encoder: c_dim = C
    calls = 0
    def encode(self, x):
        _Stub.calls += 1
        assert x.shape[0] > 0
        return {k: v[: x.shape[0]].clone() for k, v in full.items()}
one = sharding.sharded_encode(_Stub(), torch.zeros(1, 3, 16))
assert _Stub.calls == (1 if rank == 0 else 0)
assert all(torch.equal(one[k], full[k][:1]) for k in full), "n < world_size mismatch"
assert sharding.gather_codes(sharding.empty_codes(C, "cpu"), dst=0, counts=[0, 0]) is None or rank == 0
dist.barrier()
dist.destroy_process_group()
print("rank", rank, "ok")
'''


def test_world_size_2_sharding_over_gloo(tmp_path):
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    script = tmp_path / "worker.py"
    script.write_text(_GLOO_WORKER % REPO)
    procs = [subprocess.Popen([sys.executable, str(script), str(port), str(r)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for r in range(2)]
    for r, p in enumerate(procs):
        out, err = p.communicate(timeout=180)
        assert p.returncode == 0 and f"rank {r} ok" in out, err[-3000:]


_GLOO_E2E_WORKER = r'''
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, %r)
from livingscenes_amd import sharding
from livingscenes_amd.lib_more import more_solver
ws = int(sys.argv[3])
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%%d" %% int(sys.argv[1]), rank=int(sys.argv[2]), world_size=ws)
rank = dist.get_rank()
C = 8
# a deterministic CPU stand-in for the solver (the partition / gather logic is what this test is about; the real kernels run in the
# GPU twin of this test, tests/test_hip_surface.py)
class _Model:
    class encoder: c_dim = C
    calls = 0
    def encode_fps(self, pc, mask):
        _Model.calls += pc.shape[0]
        assert pc.shape[0] > 0
        m = mask.float()
        mean = torch.stack([pc[i][:, mask[i, 0]].mean(-1) for i in range(pc.shape[0])])   # valid points only: independent of the padding width
        f = torch.stack([(k + 1.0) * mean for k in range(C)], 1)              # [B,C,3]
        return {"z_so3": f, "z_inv": f.norm(dim=-1) + m.sum(-1), "s": m.sum(-1)[:, 0] * 1e-3, "t": mean[:, None, :]}
class _Solver:
    model = _Model()
    mesh_extractor = None
    regs = 0
    def _solve_object_matching(self, cr, cs, method):
        n, m = cr["s"].shape[0], cs["s"].shape[0]
        d = (cr["s"][:, None] - cs["s"][None, :]).abs()
        m0 = torch.full((n,), -1, dtype=torch.long)
        used = set()
        for i in range(n):
            for j in d[i].argsort().tolist():
                if j not in used:
                    m0[i] = j; used.add(j); break
        return {"matches0": m0}
    def _solve_pairwise_registration_batch(self, a, b):
        _Solver.regs += len(a)
        assert len(a) > 0
        R = torch.stack([torch.eye(3) * (1 + x.shape[0] * 1e-4) for x in a])
        t = torch.stack([(y.mean(0) - x.mean(0))[:, None] for x, y in zip(a, b)])
        return R, t
    def _transform_latent(self, code, tsfm):
        return {k: v.clone() for k, v in code.items()}
g = torch.Generator().manual_seed(5)
def scene(sizes):
    mx = max(sizes)
    pc, mask = torch.zeros(len(sizes), 3, mx), torch.zeros(len(sizes), 1, mx, dtype=torch.bool)
    for i, n in enumerate(sizes):
        pc[i, :, :n] = torch.randn(3, n, generator=g)
        mask[i, :, :n] = True
    return {"pc": pc, "pc_mask": mask}
pairs = [(scene([30, 41, 52]), scene([41, 30, 52, 17])), (scene([25]), scene([25, 26])), (scene([60, 61]), scene([61, 60]))]
solver = _Solver()
want = more_solver.solve_end2end_batch(solver, pairs)
calls0, regs0 = _Model.calls, _Solver.regs
got = more_solver.solve_end2end_batch(solver, pairs, sharded=True)
sizes = [int(sc["pc_mask"][i].sum()) for p in pairs for sc in p for i in range(sc["pc"].shape[0])]      # the flat (scene, instance) list
assign = sharding.balanced_assignment([n + sharding.ENCODE_COST_POINTS for n in sizes], ws)
assert sorted(i for a in assign for i in a) == list(range(len(sizes)))
assert _Model.calls - calls0 == len(assign[rank]), "each rank encodes only its (cost-balanced) share of the flat instance list"
n_pairs = sum(int((w["matches"] >= 0).sum()) for w in want)
plo, phi = sharding.shard_range(n_pairs)
assert _Solver.regs - regs0 == phi - plo, "each rank registers only its block of the matched pairs"
for w, o in zip(want, got):
    assert torch.equal(w["matches"], o["matches"])
    for a, b in zip(w["registration"], o["registration"]):
        assert (a is None) == (b is None) and (a is None or torch.equal(a, b)), "poses: sharded != unsharded"
    for a, b in zip(w["codes"], o["codes"]):
        assert (a is None) == (b is None) and (a is None or all(torch.equal(a[k], b[k]) for k in a))
# generic rows: ragged + empty shards
rows = torch.arange(12.0).reshape(4, 3) + 100 * rank
cnt = [4 if r == 0 else 0 for r in range(ws)]
allr = sharding.all_gather_rows(rows[: cnt[rank]], cnt)
assert allr.shape == (4, 3) and torch.equal(allr, torch.arange(12.0).reshape(4, 3))
# dense SDF blocks (configs[4]): every instance decoded exactly once, by the rank that owns it
class _Dec:
    class encoder: c_dim = C
    def decoder(self, q, z, code, return_sdf=False):
        return q.sum(-1) + code["s"][:, None]
codes = {"z_inv": torch.zeros(5, C), "s": torch.arange(5.0)}
q = torch.randn(1, 7, 3, generator=g)
lo, hi, part = sharding.sharded_sdf_grid(_Dec(), codes, q)
assert part.shape == (hi - lo, 7) and (lo, hi) == sharding.shard_range(5)
_, _, full = sharding.sharded_sdf_grid(_Dec(), codes, q, gather=True)
assert torch.equal(full, q.sum(-1).expand(5, -1) + torch.arange(5.0)[:, None])
dist.barrier()
dist.destroy_process_group()
print("rank", rank, "ok")
'''


@pytest.mark.parametrize("ws", [2, 3])
def test_sharded_end2end_driver_over_gloo(tmp_path, ws):
    """SURVEY 8(e) steps 2-5 for configs[3] / configs[4] (eval_3rscan.py:337-463,466-502 sharded over the node): the flat
    (scene, instance) list is block-partitioned for FPS + encode, codes all-gathered, matchers replicated, the matched pairs
    block-partitioned again, (R | t) rows all-gathered; dense SDF grids by instance block.  world_size 2 and 3 (ragged and empty
    blocks) over gloo on the CPU with a deterministic stand-in solver: sharded == unsharded, bit for bit, and every rank does only
    its share of the work."""
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    script = tmp_path / "worker.py"
    script.write_text(_GLOO_E2E_WORKER % REPO)
    procs = [subprocess.Popen([sys.executable, str(script), str(port), str(r), str(ws)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for r in range(ws)]
    for r, p in enumerate(procs):
        out, err = p.communicate(timeout=180)
        assert p.returncode == 0 and f"rank {r} ok" in out, err[-3000:]


def test_flyingshape_disk_format_round_trip(tmp_path):
    """livingscenes_amd.datasets.FlyingShape walks <root>/<.._n>/<scene>/*.npz like eval_flyingshape.py:33-60: sorted
    directories, reference scan first, 'pc' / 'transform' arrays intact."""
    import numpy as np
    from livingscenes_amd import datasets, synth
    root = str(tmp_path)
    scenes = []
    for n_obj, name in ((3, "scene_b"), (3, "scene_a"), (5, "scene_c")):
        sc = synth.make_scene_pair(n_obj, 64, seed=n_obj * 7 + len(name))
        scenes.append((n_obj, name, sc))
        datasets.write_scene(root, f"n_shape_{n_obj}", name,
                             [{"pc": sc["ref"].numpy(), "transform": sc["ref_T"].numpy()},
                              {"pc": sc["rescan"].numpy(), "transform": sc["rescan_T"].numpy()}])
    ds = datasets.FlyingShape(root)
    assert len(ds) == 3 and [p.split("/")[-1] for p in ds.scene_lst] == ["scene_a", "scene_b", "scene_c"]
    got = datasets.scene_from_scans(ds[0])
    want = [s for s in scenes if s[1] == "scene_a"][0][2]
    for k in ("ref", "rescan", "ref_T", "rescan_T"):
        assert np.array_equal(got[k].numpy(), want[k].numpy().astype(np.float32)), k
    assert len(list(ds)) == 3


def test_se3_exp_matches_matrix_exponential():
    """The retraction of the optimisation-based registration (More_Solver): exp of a twist (v, omega)."""
    import torch
    from livingscenes_amd.lib_more.more_solver import _se3_exp
    g = torch.Generator().manual_seed(0)
    for scale in (1e-8, 1e-3, 0.3, 2.5):
        xi = torch.randn(6, generator=g, dtype=torch.float64) * scale
        A = torch.zeros(4, 4, dtype=torch.float64)
        w = xi[3:]
        A[:3, :3] = torch.tensor([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], dtype=torch.float64)
        A[:3, 3] = xi[:3]
        assert torch.allclose(_se3_exp(xi), torch.matrix_exp(A), atol=1e-12)


# ------------------------------------------------------------------------------------------------ 3RScan on-disk formats
def _rot_z(deg):
    a = np.deg2rad(deg)
    T = np.eye(4)
    T[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    return T


@pytest.mark.parametrize("binary", [True, False])
def test_3rscan_reader_on_a_synthetic_tree(tmp_path, binary):
    """Dataset_3RScan reads the scan directories / index the way eval_3rscan.py does: category filter, < 1024-point instances
    dropped (but listed in full_objectId), zero padding + mask, background decimation, column-major transforms, moving / static
    split at 1 degree / 0.05."""
    from livingscenes_amd import rscan
    rng = np.random.default_rng(3)
    root = tmp_path / "3RScan" / "data"
    data = root / "val_set"
    sizes = {1: ("chair", 1500), 2: ("sofa", 1100), 3: ("bed", 900), 4: ("wall", 2000), 5: ("floor", 1000), 6: ("desk", 0)}

    def make_scan(scan_id, shift):
        pts, ids, groups = [], [], []
        for oid, (label, n) in sizes.items():
            groups.append({"objectId": oid, "label": label, "id": oid})
            if n:
                p = rng.standard_normal((n, 3)).astype(np.float32) * 0.3 + np.array([oid, 0, 0.5 * oid], np.float32) + shift
                pts.append(p); ids.append(np.full(n, oid))
        pts, ids = np.concatenate(pts), np.concatenate(ids)
        perm = rng.permutation(len(pts))
        rscan.write_scan(str(data), scan_id, pts[perm], ids[perm], groups, binary=binary, extra_uchar=binary)
        return pts[perm], ids[perm]

    ref_pts, ref_ids = make_scan("ref0", 0.0)
    make_scan("rescan0", 0.1)
    rscan.write_scan(str(data), "empty", rng.standard_normal((50, 3)), np.full(50, 4), [{"objectId": 4, "label": "wall"}], binary=binary)
    T_scene = _rot_z(30.0); T_scene[:3, 3] = [0.5, -0.2, 0.1]
    T_static = np.linalg.inv(T_scene)                       # object transform ref -> rescan whose inverse equals the scene transform
    Tt = T_scene.copy(); Tt[:3, 3] += [0.1, 0, 0]           # same rotation, 0.1 translation difference
    cm = lambda M: [float(v) for v in np.asarray(M).T.reshape(-1)]   # column-major
    scenes = [{"reference": "ref0", "scans": [
        {"reference": "rescan0", "transform": cm(T_scene), "rigid": [
            {"instance_reference": 1, "transform": cm(T_static)}, {"instance_reference": 2, "transform": cm(np.linalg.inv(_rot_z(33.0)))},
            {"instance_reference": 3, "transform": cm(np.linalg.inv(Tt))}]},
        {"reference": "empty", "transform": cm(np.eye(4)), "rigid": []}]},
        {"reference": "not_in_split", "scans": []}]
    rscan.write_index(str(root), "val", scenes[:1])
    import json
    with open(root / "3RScan.json", "w") as f:
        json.dump(scenes, f)
    cats = tmp_path / "cate.txt"
    cats.write_text("chair\nsofa\nbed\ndesk\n")
    ds = rscan.Dataset_3RScan({"root_path": str(root), "split": "val", "category_list": str(cats), "n_point_per_instance": 1024,
                               "use_gt_mask": True}, device="cpu")
    assert len(ds) == 1 and sorted(ds.scan_list) == ["empty", "ref0", "rescan0"]
    ref, rescans = ds[0]
    assert ref["pc"].shape == (2, 3, 1500) and ref["pc_mask"].shape == (2, 1, 1500)
    assert ref["objectId"].tolist() == [1, 2] and ref["full_objectId"].tolist() == [1, 2, 3, 6]
    assert ref["pc_mask"].sum(-1).flatten().tolist() == [1500, 1100]
    assert ref["id_label"] == [(1, "chair", "chair"), (2, "sofa", "sofa"), (3, "bed", "bed"), (6, "desk", "table")]
    assert torch.equal(ref["pc"][1, :, 1100:], torch.zeros(3, 400))
    assert np.allclose(ref["pc"][0, :, :1500].T.numpy(), ref_pts[ref_ids == 1])      # file order of the instance's vertices
    z_max = max(ref_pts[ref_ids == i][:, 2].max() for i in (1, 2, 3))
    bg = np.concatenate([ref_pts[ref_ids == i][ref_pts[ref_ids == i][:, 2] < z_max] for i in (4, 5)])[::5]
    assert np.allclose(ref["bg_pc"], bg)
    assert len(rescans) == 1                                                           # the scan without a kept instance is ruled out
    r = rescans[0]
    assert np.allclose(r["rescan2ref_tsfm"][0].numpy(), T_scene, atol=1e-6)
    assert r["static_ids"].tolist() == [1.0] and r["moving_ids"].tolist() == [2.0, 3.0]
    assert rscan.get_shapenet_category("trash can") == "trash_bin" and rscan.get_shapenet_category("wall") == "others"


def test_3rscan_matching_metrics_and_disambiguation(tmp_path):
    """harness.eval_3rscan_matching on a synthetic 3RScan tree with a stub model / solver (CPU): recalls, the static / dynamic
    split, scene-level thresholds, and the symmetry-link walk of ``disambiguate``."""
    from livingscenes_amd import harness, rscan
    rng = np.random.default_rng(5)
    root = tmp_path / "data"
    labels = {1: "chair", 2: "chair", 3: "sofa", 4: "bed"}

    def make_scan(scan_id, ids):
        pts = np.concatenate([rng.standard_normal((1030, 3)).astype(np.float32) * 0.2 + i for i in ids])
        oid = np.concatenate([np.full(1030, i) for i in ids])
        rscan.write_scan(str(root / "val_set"), scan_id, pts, oid, [{"objectId": i, "label": labels[i]} for i in ids])

    make_scan("ref", [1, 2, 3, 4])
    make_scan("res", [4, 3, 2, 1])             # same objects, listed in reverse order
    cm = lambda M: [float(v) for v in np.asarray(M).T.reshape(-1)]
    moved = np.eye(4); moved[:3, 3] = [1.0, 0, 0]
    scenes = [{"reference": "ref", "ambiguity": [[{"instance_source": 1, "instance_target": 2, "transform": cm(np.eye(4))},
                                                   {"instance_source": 2, "instance_target": 1, "transform": cm(np.eye(4))}]],
               "scans": [{"reference": "res", "transform": cm(np.eye(4)),
                          "rigid": [{"instance_reference": 3, "transform": cm(moved)}, {"instance_reference": 4, "transform": cm(np.eye(4))}]}]}]
    rscan.write_index(str(root), "val", scenes)
    import json
    with open(root / "3RScan.json", "w") as f:
        json.dump(scenes, f)
    ds = rscan.Dataset_3RScan({"root_path": str(root), "split": "val", "category_list": ["chair", "sofa", "bed"],
                               "n_point_per_instance": 1024, "use_gt_mask": True}, device="cpu")

    class Model:
        def encode_fps(self, pc, mask):
            return {"n": pc.shape[0]}

    class Solver:
        model = Model()
        def __init__(self, matches): self.matches = matches
        def _solve_object_matching(self, a, b, method): return {"matches0": torch.tensor(self.matches)}

    # ref ids [1,2,3,4], rescan ids [4,3,2,1]: the correct matches0 is [3,2,1,0].
    perfect = harness.eval_3rscan_matching(ds, Solver([3, 2, 1, 0]))
    assert perfect["object_recall[sequential]"] == 100.0 and perfect["scene_recall@75"] == 100.0
    assert perfect["dynamic_recall"] == 100.0 and perfect["static_recall"] == 100.0
    # chairs 1 and 2 swapped: forgiven by the ambiguity links; sofa (the moving object) unmatched, bed wrong
    m = harness.eval_3rscan_matching(ds, Solver([2, 3, -1, 1]))
    assert m["object_recall[sequential]"] == 50.0 and m["dynamic_recall"] == 0.0
    assert abs(m["static_recall"] - 100.0 * 2 / 3) < 1e-9
    assert (m["scene_recall@75"], m["scene_recall@50"], m["scene_recall@25"]) == (0.0, 100.0, 100.0)
    ids = torch.tensor([2, 1, 9])
    assert harness.disambiguate(ids, torch.tensor([1, 2, 3]), scenes[0]["ambiguity"]).tolist() == [1, 2, 9]


def test_3rscan_reader_matches_the_reference_loader(golden):
    """livingscenes_amd.rscan.Dataset_3RScan on the committed synthetic tree (tests/golden/rscan_tree: binary and ascii PLY, colour
    columns, interleaved instances, an instance below 1024 points, one without points, a rescan without valid instances, a scene
    outside the split) against tests/golden/rscan.npz, the output of the REFERENCE's unmodified eval_3rscan.Dataset_3RScan on the
    same files (tests/golden/make_golden_rscan.py): every field of every scan, bit for bit."""
    import numpy as np
    import torch
    from livingscenes_amd import rscan
    g = golden("rscan")
    tree = os.path.join(GOLDEN_DIR, "rscan_tree")
    ds = rscan.Dataset_3RScan({"root_path": os.path.join(tree, "data"), "split": "val", "category_list": os.path.join(tree, "categories.txt"),
                               "n_point_per_instance": 1024, "use_gt_mask": True}, device="cpu")
    assert len(ds) == int(g["n_scenes"]) and [s["reference"] for s in ds.scene_list] == list(g["scene_refs"])

    def same(prefix, inst):
        assert torch.equal(inst["pc"], torch.from_numpy(g[prefix + "pc"])), prefix
        assert torch.equal(inst["pc_mask"], torch.from_numpy(g[prefix + "pc_mask"])), prefix
        assert np.array_equal(inst["objectId"].numpy(), g[prefix + "objectId"]) and np.array_equal(inst["full_objectId"].numpy(), g[prefix + "full_objectId"])
        assert np.array_equal(np.asarray(inst["bg_pc"], np.float64).reshape(-1, 3), g[prefix + "bg_pc"]), prefix
        assert [[str(a), b, c] for a, b, c in inst["id_label"]] == g[prefix + "id_label"].tolist(), prefix
    for i in range(len(ds)):
        reference, rescans = ds[i]
        same(f"s{i}_ref_", reference)
        assert len(rescans) == int(g[f"s{i}_n_rescans"])
        for k, r in enumerate(rescans):
            same(f"s{i}_r{k}_", r)
            assert np.array_equal(r["moving_ids"].numpy(), g[f"s{i}_r{k}_moving_ids"]) and np.array_equal(r["static_ids"].numpy(), g[f"s{i}_r{k}_static_ids"])
            assert np.array_equal(r["rescan2ref_tsfm"].numpy(), g[f"s{i}_r{k}_rescan2ref_tsfm"])


def test_packed_fp32_build_guard_fires_without_the_flag(tmp_path):
    """build.py's determinism pin: edge.hip compiled WITHOUT -fno-slp-vectorize carries compiler-formed v_pk_*_f32 in the
    gather kernels and the guard must refuse it; the objects of the real build pass."""
    import subprocess
    from livingscenes_amd import build as B
    B.build()
    B.check_packed_fp32(os.path.join(B.LIBDIR, "obj"))
    flags = [f for f in B.FLAGS if f != "-fno-slp-vectorize"]
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + flags + ["-x", "hip", "-c", os.path.join(B.CSRC, "edge.hip"), "-o", str(tmp_path / "edge.o")])
    import shutil
    for src in B.PACKED_FP32_GUARD:                                     # every other guarded object: the real build's (they pass)
        if src != "edge.hip":
            shutil.copy(os.path.join(B.LIBDIR, "obj", src.replace(".hip", ".o")), tmp_path / src.replace(".hip", ".o"))
    with pytest.raises(RuntimeError, match="packed fp32"):
        B.check_packed_fp32(str(tmp_path))


_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "livingscenes_amd", "csrc")


@pytest.mark.parametrize("header", sorted(f for f in os.listdir(_CSRC) if f.endswith(".h")))
def test_every_csrc_header_compiles_on_its_own(header):
    """A header under csrc/ includes what it uses: a translation unit of that one #include passes hipcc's syntax check, host and device pass."""
    import shutil
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (shutil.which(hipcc) or os.path.exists(hipcc)):
        pytest.skip("no hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++17", "-fsyntax-only", "-x", "hip", "-"],
                       input=f'#include "{os.path.join(_CSRC, header)}"\n', capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_launcher_refuses_a_world_size_other_than_gpus(monkeypatch):
    """`--gpus N` is the number of ranks (livingscenes_amd/launch.py): under a launcher the world size must BE N, started
    plainly with N = 1 nothing is launched, and a nonsensical N is refused."""
    from livingscenes_amd import launch
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    assert launch.ensure_ranks(1, "x.py", []) == (1, 0, 0)
    with pytest.raises(SystemExit):
        launch.ensure_ranks(0, "x.py", [])
    monkeypatch.setenv("WORLD_SIZE", "4")
    monkeypatch.setenv("RANK", "3")
    monkeypatch.setenv("LOCAL_RANK", "3")
    assert launch.ensure_ranks(4, "x.py", []) == (4, 3, 3)
    with pytest.raises(SystemExit) as e:
        launch.ensure_ranks(8, "x.py", [])
    assert "WORLD_SIZE=4" in str(e.value)
    with pytest.raises(SystemExit):
        launch.ensure_ranks(1, "x.py", [])


def test_bench_gpus_n_starts_n_ranks():
    """`python bench.py --gpus 2` started plainly re-executes under torch.distributed.run with two ranks (there is no HIP device here:
    both ranks announce themselves on stderr before the device check stops them), and a launcher world of another size is
    refused before anything is timed."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    if torch.cuda.is_available():
        pytest.skip("device present: tests/test_hip_fullbatch.py::test_bench_gpus_2_runs_two_ranks covers the real run")
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2"], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode != 0
    log = p.stdout + p.stderr
    assert "rank 0 of 2 started" in log and "rank 1 of 2 started" in log, log[-2000:]
    assert "bench.py needs a HIP device" in log      # (the launcher stops the other rank as soon as one has failed: at least one says it)
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "8"], capture_output=True, text=True,
                       env=dict(env, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0"), timeout=300)
    assert p.returncode != 0 and "WORLD_SIZE=2" in p.stderr
