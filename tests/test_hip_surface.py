"""GPU tests of the reference-facing Python surface (model_utils / lib_more mirrors) against the CPU oracle."""
import numpy as np
import pytest
import torch

from livingscenes_amd import synth

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def relerr(a, b):
    a, b = ((v.detach().cpu() if torch.is_tensor(v) else torch.as_tensor(v)).double() for v in (a, b))
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


@pytest.fixture(scope="module")
def small_prior():
    from livingscenes_amd.model_utils import Shape_Prior
    ecfg, dcfg = synth.small_encoder_cfg(), synth.small_decoder_cfg()
    ew, dw = synth.make_encoder_weights(ecfg, 4), synth.make_decoder_weights(dcfg, 4)
    return Shape_Prior.from_state(ecfg, dcfg, ew, dw, device=_dev(), n_pcl=128), (ecfg, dcfg, ew, dw)


def test_shape_prior_encode_and_decoder(small_prior):
    from oracle import net
    sp, (ecfg, dcfg, ew, dw) = small_prior
    x = synth.make_instances(5, 128, seed=8)
    emb = sp.encode(x.to(_dev()))
    ref = net.shape_prior_encode(ew, ecfg, x)
    assert emb["t"].shape == (5, 1, 3) and emb["z_so3"].shape == (5, ecfg["c_dim"], 3)
    for k in ("z_so3", "z_inv", "s", "t"):
        assert relerr(emb[k], ref[k]) < TOL, k
    q = synth.make_queries(5, 200, seed=1).to(_dev()) * emb["s"][:, None, None] + emb["t"]
    sdf = sp.decoder(q, None, emb, return_sdf=True)
    ref_sdf = net.field_query(dw, dcfg, q.cpu(), {k: v.cpu() for k, v in emb.items()})
    assert relerr(sdf, ref_sdf) < TOL
    occ = sp.decoder(q, None, emb)  # Bernoulli(logits = sdf2occ_factor * sdf), model_utils.py:263
    assert torch.allclose(occ.logits, -sdf)


def test_sdf_decode_two_piece_mode_stays_inside_the_tolerance():
    """LS_SDF_BF16X2=1 (opt-in decoder throughput mode: two bf16 pieces per operand, three MFMAs per 16 k, ~1.7x): still within the
    1e-4 tolerance of the oracle (measured 3e-6 against fp64 on the full-width decoder)."""
    import os, subprocess, sys
    code = (
        "import torch, numpy as np\n"
        "from livingscenes_amd import synth\n"
        "from livingscenes_amd.model_utils import Shape_Prior\n"
        "from oracle import net\n"
        "ecfg, dcfg = synth.default_encoder_cfg(), synth.default_decoder_cfg()\n"
        "ew, dw = synth.make_encoder_weights(ecfg, 0), synth.make_decoder_weights(dcfg, 0)\n"
        "sp = Shape_Prior.from_state(ecfg, dcfg, ew, dw, device=torch.device('cuda:0'))\n"
        "emb = sp.encode(synth.make_instances(3, 1024, seed=2).cuda())\n"
        "q = synth.make_queries(3, 700, seed=4).cuda() * emb['s'][:, None, None] + emb['t']\n"
        "sdf = sp.decoder(q, None, emb, return_sdf=True).cpu()\n"
        "ref = net.field_query(net.as_params(dw), dcfg, q.cpu(), {k: v.cpu() for k, v in emb.items()})\n"
        "err = (sdf - ref).abs().max() / ref.abs().max()\n"
        "assert err < 1e-4, err\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run([sys.executable, "-c", code], check=True, env=dict(os.environ, LS_SDF_BF16X2="1"), cwd=root)


def test_model_options_are_read_back_from_the_library():
    """ls_model_get_option returns what the HANDLE holds: the environment's value as the C side parsed it (atoi: "false" and "" are 0 --
    a Python-side mirror with `!= "0"` called both 1), then whatever ls_model_set_option stored; set_option's "previous value" is that
    read-back, so a temporary change restores exactly the state it found.  Unknown options (incl. the retired 4) are errors, not zeros,
    for get and set alike."""
    import os, subprocess, sys
    code = (
        "import torch\n"
        "from livingscenes_amd import _lib, synth\n"
        "from livingscenes_amd.model_utils import Shape_Prior\n"
        "ecfg, dcfg = synth.small_encoder_cfg(), synth.small_decoder_cfg()\n"
        "sp = Shape_Prior.from_state(ecfg, dcfg, synth.make_encoder_weights(ecfg, 0), synth.make_decoder_weights(dcfg, 0), device=torch.device('cuda:0'))\n"
        "hip = sp.hip_model()\n"
        "import os\n"
        "want = [int(v) for v in os.environ['LS_EXPECT'].split(',')]\n"
        "got = [hip.get_option(o) for o in (_lib.OPT_SDF_TRAIN_SPLITK, _lib.OPT_SDF_BF16X2, _lib.OPT_ENCODE_GRAPH)]\n"
        "assert got == want, (got, want)\n"
        "prev = hip.set_option(_lib.OPT_SDF_BF16X2, 1 - want[1])\n"
        "assert prev == want[1] and hip.get_option(_lib.OPT_SDF_BF16X2) == 1 - want[1]\n"
        "assert hip.set_option(_lib.OPT_SDF_BF16X2, prev) == 1 - want[1] and hip.get_option(_lib.OPT_SDF_BF16X2) == want[1]\n"
        "set_raw = lambda o: _lib.check(_lib.load().ls_model_set_option(hip._h, o, 0), 'ls_model_set_option')\n"
        "for o in (4, 99):\n"   # 4: the retired staged-attention option
        "    for f in (hip.get_option, set_raw):\n"
        "        try:\n"
        "            f(o)\n"
        "            raise SystemExit(f'unknown option {o} accepted by {f}')\n"
        "        except _lib.LsError:\n"
        "            pass\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    base = {k: v for k, v in os.environ.items() if k not in ("LS_SDF_BF16X2", "LS_ENCODE_GRAPH")}
    for env, want in (({}, "1,0,0"), ({"LS_SDF_BF16X2": "1", "LS_ENCODE_GRAPH": "1"}, "1,1,1"), ({"LS_SDF_BF16X2": "false", "LS_ENCODE_GRAPH": ""}, "1,0,0")):
        subprocess.run([sys.executable, "-c", code], check=True, env=dict(base, LS_EXPECT=want, **env), cwd=root)


def test_encoder_refuses_a_cloud_too_small_for_its_schedule():
    """The released schedule down-samples by 32: with N = 256 the last layer would have 8 source points for 16 neighbours
    (-1 padded lists into the gather kernels).  The library refuses instead of reading out of bounds."""
    from livingscenes_amd._lib import LsError
    from livingscenes_amd.model_utils import Shape_Prior
    ecfg, dcfg = synth.default_encoder_cfg(), synth.default_decoder_cfg()
    sp = Shape_Prior.from_state(ecfg, dcfg, synth.make_encoder_weights(ecfg, 0), synth.make_decoder_weights(dcfg, 0), device=_dev())
    with pytest.raises(LsError, match="too small"):
        sp.encode(synth.make_instances(2, 256, seed=1).to(_dev()))
    assert torch.isfinite(sp.encode(synth.make_instances(2, 512, seed=1).to(_dev()))["z_inv"]).all()


def test_use_double_returns_float64_codes_of_the_fp32_path(small_prior):
    """Shape_Prior(use_double=True) (model_utils.py:148-152,166: fp64 encoder in the reference): the fp32 HIP encoder runs and the codes
    are float64 -- equal to the fp32 codes, and within 1e-4 of the oracle evaluated in fp64."""
    from oracle import net
    sp, (ecfg, dcfg, ew, dw) = small_prior
    x = synth.make_instances(3, 128, seed=12)
    emb32 = sp.encode(x.to(_dev()))
    sp.use_double = True
    try:
        emb64 = sp.encode(x.to(_dev()))
    finally:
        sp.use_double = False
    ref = net.shape_prior_encode({k: v.double() for k, v in ew.items()}, ecfg, x.double())
    for k in ("z_so3", "z_inv", "s", "t"):
        assert emb64[k].dtype == torch.float64 and torch.equal(emb64[k], emb32[k].double())
        assert relerr(emb64[k], ref[k]) < TOL, k


def test_encode_fps_ragged_matches_reference_loop(small_prior):
    """encode_fps (model_utils.py:199-215): mask-select, FPS to n_pcl, encode -- vs the oracle run instance by instance."""
    from oracle import net
    sp, (ecfg, dcfg, ew, dw) = small_prior
    g = torch.Generator().manual_seed(3)
    B, Nmax = 3, 700
    pc = torch.randn(B, 3, Nmax, generator=g)
    mask = torch.zeros(B, 1, Nmax, dtype=torch.bool)
    lens = [700, 333, 150]
    for b, L in enumerate(lens):
        perm = torch.randperm(Nmax, generator=g)[:L]
        mask[b, 0, perm] = True
    emb = sp.encode_fps(pc.to(_dev()), mask.to(_dev()))
    for b in range(B):
        valid = pc[b].T[mask[b, 0]].unsqueeze(0)
        pts, _ = net.sample_farthest_points(valid, 128)
        ref = net.shape_prior_encode(ew, ecfg, pts.transpose(1, 2).contiguous())
        for k in ("z_so3", "z_inv", "s", "t"):
            assert relerr(emb[k][b:b + 1], ref[k]) < TOL, (b, k)
    emb2 = sp.encode_fps(pc.to(_dev()), mask.to(_dev()), n_fps=2)  # random-start draws, averaged
    assert emb2["z_inv"].shape == emb["z_inv"].shape and torch.isfinite(emb2["z_so3"]).all()


def test_3rscan_tree_to_codes(small_prior, tmp_path):
    """Disk -> Dataset_3RScan (PLY + labels + semseg json, device tensors) -> Shape_Prior.encode_fps, as eval_3rscan.py:260-261
    drives it; each instance's code equals the oracle's on that instance's vertices in file order."""
    from livingscenes_amd import rscan
    from oracle import net
    sp, (ecfg, dcfg, ew, dw) = small_prior
    rng = np.random.default_rng(8)
    root = tmp_path / "data"
    sizes = {7: ("chair", 1300), 9: ("table", 1024), 11: ("lamp", 600)}
    pts = np.concatenate([rng.standard_normal((n, 3)).astype(np.float32) * 0.4 + oid for oid, (_, n) in sizes.items()])
    ids = np.concatenate([np.full(n, oid) for oid, (_, n) in sizes.items()])
    perm = rng.permutation(len(pts))
    pts, ids = pts[perm], ids[perm]
    rscan.write_scan(str(root / "val_set"), "s0", pts, ids, [{"objectId": o, "label": l} for o, (l, _) in sizes.items()])
    rscan.write_index(str(root), "val", [{"reference": "s0", "scans": []}])
    ds = rscan.Dataset_3RScan({"root_path": str(root), "split": "val", "category_list": ["chair", "table"], "n_point_per_instance": 1024,
                               "use_gt_mask": True}, device=_dev())
    ref, rescans = ds[0]
    assert rescans == [] and ref["pc"].is_cuda and ref["objectId"].tolist() == [7, 9]
    emb = sp.encode_fps(ref["pc"], ref["pc_mask"])
    for b, oid in enumerate((7, 9)):
        valid = torch.from_numpy(pts[ids == oid]).unsqueeze(0)
        sub, _ = net.sample_farthest_points(valid, 128)
        want = net.shape_prior_encode(ew, ecfg, sub.transpose(1, 2).contiguous())
        for k in ("z_so3", "z_inv", "s", "t"):
            assert relerr(emb[k][b:b + 1], want[k]) < TOL, (oid, k)


def test_chamfer_metric_and_3rscan_relocalization_eval(small_prior, tmp_path):
    """evaluate.chamfer_distance_torch (nearest neighbours from the library's raw-cloud k-NN) against the dense formula of
    evaluate.py:111-123, and harness.eval_3rscan_relocalization end to end from a synthetic 3RScan tree: with untrained weights
    the Kabsch init is meaningless, but ICP on a noise-free rigid copy of a small motion still has to recover the pose."""
    from livingscenes_amd import evaluate, harness, rscan
    from livingscenes_amd.lib_math import torch_se3
    from livingscenes_amd.lib_more.more_solver import More_Solver
    sp, _ = small_prior
    d = _dev()
    g = torch.Generator().manual_seed(0)
    src, ref = torch.randn(2, 300, 3, generator=g), torch.randn(2, 257, 3, generator=g)
    def rnd_se3():
        q, _ = torch.linalg.qr(torch.randn(2, 3, 3, generator=g))
        q = q * torch.sign(torch.det(q))[:, None, None]
        return torch.cat([q, torch.randn(2, 3, 1, generator=g)], 2)
    pred, gt = rnd_se3(), rnd_se3()
    sq = lambda a, b: ((a[:, :, None, :] - b[:, None, :, :]) ** 2).sum(-1)
    a = torch_se3.transform(pred, src)
    b = torch_se3.transform(torch_se3.concatenate(pred, torch_se3.inverse(gt)), ref)
    want = sq(a, ref).min(-1)[0].mean(1) + sq(ref, b).min(-1)[0].mean(1)
    got = evaluate.chamfer_distance_torch(src.to(d), ref.to(d), pred.to(d), gt.to(d))
    assert relerr(got, want) < 1e-5

    rng = np.random.default_rng(2)
    root = tmp_path / "data"
    shape = {5: ("chair", np.abs(rng.standard_normal((1400, 3))).astype(np.float32) * [0.3, 0.5, 0.2]),
             6: ("sofa", np.abs(rng.standard_normal((1200, 3))).astype(np.float32) * [0.6, 0.2, 0.3] + 2.0)}
    ang = np.deg2rad(4.0)
    T = np.eye(4); T[:2, :2] = [[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]]; T[:3, 3] = [0.03, -0.02, 0.01]
    def write(scan_id, move):
        pts = np.concatenate([(v @ T[:3, :3].T + T[:3, 3]).astype(np.float32) if move else v for _, v in shape.values()])
        ids = np.concatenate([np.full(len(v), k) for k, (_, v) in shape.items()])
        rscan.write_scan(str(root / "val_set"), scan_id, pts, ids, [{"objectId": k, "label": l} for k, (l, _) in shape.items()])
    write("ref", False); write("res", True)
    cm = lambda M: [float(v) for v in np.asarray(M).T.reshape(-1)]
    scenes = [{"reference": "ref", "ambiguity": [], "scans": [{"reference": "res", "transform": cm(np.eye(4)), "rigid": [
        {"instance_reference": 5, "instance_rescan": 5, "transform": cm(T), "symmetry": 0},
        {"instance_reference": 6, "instance_rescan": 6, "transform": cm(T), "symmetry": 2},
        {"instance_reference": 99, "instance_rescan": 99, "transform": cm(T), "symmetry": 0}]}]}]
    rscan.write_index(str(root), "val", scenes)
    ds = rscan.Dataset_3RScan({"root_path": str(root), "split": "val", "category_list": ["chair", "sofa"], "n_point_per_instance": 1024,
                               "use_gt_mask": True}, device=d)
    solver = More_Solver({"shape_priors": {"n_input_point": 128, "prior_name": "chair", "ckpt_dir": ""}, "fps": {"n_init": 1, "random_start": False}}, model=sp)
    out = harness.eval_3rscan_relocalization(ds, solver, optim=False)
    assert out["n_pairs"] == 2 and out["shape"] == ["chair", "sofa"]
    assert out["recall[T<0.1m]"] == 100.0 and out["recall[RRE<10deg]"] == 100.0, out
    assert out["rre_median[RRE<10deg]"] < 1.0 and out["rte_median[RRE<10deg]"] < 0.02 and out["chamfer_median"] < 1e-3, out


def test_all_matchers_vs_golden(golden):
    from livingscenes_amd.lib_more import matcher_new as mn
    g = golden("matchers")
    d = _dev()
    for name in ("n1", "n2", "n3", "n5", "n32"):
        r = mn.sequential_matcher(torch.from_numpy(g[f"seq_{name}_a"]).to(d), torch.from_numpy(g[f"seq_{name}_b"]).to(d))
        assert r["matches0"].dtype == torch.int64
        assert np.array_equal(r["matches0"].cpu().numpy(), g[f"seq_{name}_m0"]) and np.array_equal(r["matches1"].cpu().numpy(), g[f"seq_{name}_m1"])
    a, b = torch.from_numpy(g["nn_a"]).to(d), torch.from_numpy(g["nn_b"]).to(d)
    r = mn.nn_matcher(a.T[None], b.T[None])
    assert np.array_equal(r["matches0"].cpu().numpy(), g["nn_m0"]) and np.array_equal(r["matches1"].cpu().numpy(), g["nn_m1"])
    r = mn.sinkhorn_matcher(a.T[None], b.T[None])
    assert np.array_equal(r["matches0"].cpu().numpy(), g["sk_m0"]) and np.array_equal(r["matches1"].cpu().numpy(), g["sk_m1"])
    src = {"z_inv": torch.from_numpy(g["eqsrc_z_inv"]).to(d), "z_so3": torch.from_numpy(g["eqsrc_z_so3"]).to(d)}
    tgt = {"z_inv": torch.from_numpy(g["eqtgt_z_inv"]).to(d), "z_so3": torch.from_numpy(g["eqtgt_z_so3"]).to(d)}
    for nm, fn in (("eq", mn.eq_seq_matcher), ("sim3", mn.sim3_seq_matcher)):
        r = fn(src, tgt)
        assert np.array_equal(r["matches0"].cpu().numpy(), g[f"{nm}_m0"]) and np.array_equal(r["matches1"].cpu().numpy(), g[f"{nm}_m1"])


def test_assignment_matchers_vs_reference_fixture_and_oracle(golden):
    """SURVEY 8 a-10b on the device: nn_matcher / sinkhorn_matcher = cosine scores + ONE launch each (ls_nn_match_f32 / ls_sinkhorn_match_f32: the coupling
    matrix in LDS, 100 log-space iterations, mutual arg-maxes, threshold test) -- match assignments bit-exact against the reference's own outputs
    (tests/golden/make_golden_assign.py: realistic 32 x 32, rectangular, 1 x 1, 1 x 3 (squeezed to 0-dim), exact ties, 64 x 50, D = 64) and against the
    oracle on random shapes up to 150 x 120 (the dynamic-LDS path)."""
    from livingscenes_amd import ops
    from livingscenes_amd.lib_more import matcher_new as mn
    from oracle import more
    g = golden("matchers_assign")
    d = _dev()
    for name in g["names"]:
        a, b = torch.from_numpy(g[f"{name}_a"]).to(d), torch.from_numpy(g[f"{name}_b"]).to(d)
        r = mn.nn_matcher(a.T[None], b.T[None])
        assert r["matches0"].dtype == torch.int64 and r["matches0"].shape == g[f"{name}_nn_m0"].shape and r["matches1"].shape == g[f"{name}_nn_m1"].shape
        assert np.array_equal(r["matches0"].cpu().numpy(), g[f"{name}_nn_m0"]) and np.array_equal(r["matches1"].cpu().numpy(), g[f"{name}_nn_m1"]), name
        r = mn.sinkhorn_matcher(a.T[None], b.T[None], desc_dim=a.shape[1])
        assert r["matches0"].shape == g[f"{name}_sk_m0"].shape
        assert np.array_equal(r["matches0"].cpu().numpy(), g[f"{name}_sk_m0"]) and np.array_equal(r["matches1"].cpu().numpy(), g[f"{name}_sk_m1"]), name
        r = mn.sinkhorn_matcher(a.T[None], b.T[None], desc_dim=a.shape[1], match_threshold=float(g[f"{name}_sk_thr"]))
        assert np.array_equal(r["matches0"].cpu().numpy(), g[f"{name}_skt_m0"]) and np.array_equal(r["matches1"].cpu().numpy(), g[f"{name}_skt_m1"]), name
    gen = torch.Generator().manual_seed(5)
    for n, m in ((2, 2), (7, 3), (33, 65), (64, 64), (100, 90), (150, 120)):
        a = torch.randn(n, 256, generator=gen)
        b = torch.cat([a[torch.randperm(n, generator=gen)[:min(n, m)]] + 0.4 * torch.randn(min(n, m), 256, generator=gen),
                       torch.randn(max(m - n, 0), 256, generator=gen)], 0)[torch.randperm(m, generator=gen)]
        for fn_ref, fn in ((more.nn_matcher, mn.nn_matcher), (more.sinkhorn_matcher, mn.sinkhorn_matcher)):
            ref, r = fn_ref(a.T[None], b.T[None]), fn(a.T[None].to(d), b.T[None].to(d))
            assert np.array_equal(r["matches0"].cpu().numpy(), ref["matches0"].numpy()) and np.array_equal(r["matches1"].cpu().numpy(), ref["matches1"].numpy()), (n, m)
    # beyond the LDS of one workgroup: a clear error, nothing enqueued
    with pytest.raises(Exception, match="LDS"):
        ops.sinkhorn_match(torch.zeros(300, 300, device=d), 16.0)


def test_more_solver_matching_registration_end2end(small_prior):
    """More_Solver mirror: _solve_object_matching (5 methods), _solve_pairwise_registration(optim=False) incl. ICP,
    _transform_latent and _solve_end2end vs the oracle pipeline (FPS -> encode -> Kabsch -> ICP) pair by pair."""
    from livingscenes_amd.lib_more.more_solver import More_Solver
    from oracle import more, net
    sp, (ecfg, dcfg, ew, dw) = small_prior
    d = _dev()
    cfg = {"shape_priors": {"n_input_point": 128, "prior_name": "chair", "ckpt_dir": ""}, "fps": {"n_init": 1, "random_start": False}}
    solver = More_Solver(cfg, model=sp)
    sc = synth.make_scene_pair(4, 300, seed=11, noise=0.002)
    ref_x, res_x = sc["ref"], sc["rescan"]
    # --- pairwise registration (raw clouds of 300 points -> FPS 128 -> encode -> Kabsch -> ICP)
    R, t = solver._solve_pairwise_registration(ref_x[:1].to(d), res_x[:1].to(d))
    p1, _ = net.sample_farthest_points(ref_x[:1], 128)
    p2, _ = net.sample_farthest_points(res_x[:1], 128)
    c1 = net.shape_prior_encode(ew, ecfg, p1.transpose(1, 2).contiguous())
    c2 = net.shape_prior_encode(ew, ecfg, p2.transpose(1, 2).contiguous())
    Rk, tk, _, _ = more.kabsch_transformation_estimation(c1["z_so3"] + c1["t"], c2["z_so3"] + c2["t"])
    Ri, Ti, _, _, _ = more.iterative_closest_point(p1, p2, Rk.transpose(1, 2).contiguous(), tk.squeeze(2))
    assert R.shape == (1, 3, 3) and t.shape == (1, 3, 1)
    # same nearest-neighbour assignment at the fixed point => same least-squares pose, to 1e-4 (see test_icp_vs_oracle)
    nn_h = more._nn1(p1 @ R.cpu().transpose(1, 2) + t.cpu().transpose(1, 2), p2)
    nn_o = more._nn1(p1 @ Ri + Ti[:, None], p2)
    tol = 1e-4 if torch.equal(nn_h, nn_o) else 1e-3
    assert relerr(R, Ri.transpose(1, 2)) < tol and relerr(t, Ti.unsqueeze(2)) < tol
    with pytest.raises(KeyError):   # optim=True needs cfg['registration'] (test_optim_registration_refines_the_pose covers it)
        solver._solve_pairwise_registration(ref_x[:1].to(d), res_x[:1].to(d), optim=True)
    # --- matching on encoded scenes, every method returns int64 maps consistent with the oracle
    emb_r = sp.encode(ref_x.transpose(1, 2).contiguous().to(d))
    emb_s = sp.encode(res_x.transpose(1, 2).contiguous().to(d))
    cr = {k: v.cpu() for k, v in emb_r.items()}
    cs = {k: v.cpu() for k, v in emb_s.items()}
    m = solver._solve_object_matching(emb_r, emb_s, "sequential")
    assert np.array_equal(m["matches0"].cpu().numpy(), more.sequential_matcher(cr["z_inv"], cs["z_inv"])["matches0"].numpy())
    for method in ("nn", "sinkhorn", "sim3_seq", "eq_seq"):
        r = solver._solve_object_matching(emb_r, emb_s, method)
        assert r["matches0"].shape == (4,) and r["matches1"].shape == (4,)
    assert np.array_equal(solver._solve_object_matching(emb_r, emb_s, "eq_seq")["matches0"].cpu().numpy(),
                          more.eq_seq_matcher(cr, cs)["matches0"].numpy())
    # --- _transform_latent (more_solver.py:230-244)
    T = torch.eye(4)[None, :3].clone().to(d)
    T[0, :, 3] = torch.tensor([1.0, 2.0, 3.0])
    one = {k: v[:1] for k, v in emb_r.items()}
    tl = solver._transform_latent(one, T)
    assert torch.allclose(tl["t"], one["t"] + T[:, :, 3][:, None]) and torch.equal(tl["z_so3"], one["z_so3"])
    # --- end2end on masked, padded scenes
    def scene(x):
        n, N, _ = x.shape
        pc = torch.zeros(n, 3, N + 50)
        pc[:, :, :N] = x.transpose(1, 2)
        mask = torch.zeros(n, 1, N + 50, dtype=torch.bool)
        mask[:, :, :N] = True
        return {"pc": pc.to(d), "pc_mask": mask.to(d)}
    out = solver._solve_end2end(scene(ref_x), scene(res_x))
    assert len(out["registration"]) == 4 and out["matches"].shape == (4,)
    for i, j in enumerate(out["matches"].tolist()):
        if j >= 0:
            assert out["registration"][i].shape == (1, 4, 4) and abs(float(torch.det(out["registration"][i][0, :3, :3])) - 1) < 1e-3
    assert out["mesh_lst"] == [None] * 4          # no mesh_extractor configured
    # with a mesh extractor every matched instance also gets the mesh of its transformed code (more_solver.py:284-296)
    solver_m = More_Solver(dict(solver.cfg, mesh_extractor=dict(threshold=0.5, resolution0=8, upsampling_steps=1, padding=0.1)), model=sp)
    out_m = solver_m._solve_end2end(scene(ref_x), scene(res_x))
    assert torch.equal(out_m["matches"], out["matches"])
    for i, j in enumerate(out_m["matches"].tolist()):
        if j >= 0:
            assert hasattr(out_m["mesh_lst"][i], "vertices") and hasattr(out_m["mesh_lst"][i], "faces")


def test_flyingshape_style_harness_vs_oracle(small_prior):
    """eval_matching / eval_relocalization counterparts: metrics from the HIP path == metrics from the oracle pipeline."""
    from livingscenes_amd import harness
    from livingscenes_amd.lib_more.more_solver import More_Solver
    from oracle import more, net
    sp, (ecfg, dcfg, ew, dw) = small_prior
    cfg = {"shape_priors": {"n_input_point": 128, "prior_name": "chair", "ckpt_dir": ""}, "fps": {"n_init": 1}}
    solver = More_Solver(cfg, model=sp)
    scenes = [synth.make_scene_pair(6, 128, seed=40 + i, noise=0.002) for i in range(2)]
    m = harness.eval_matching(scenes, solver)
    r = harness.eval_relocalization(scenes, solver, icp=False)
    ok = tot = 0
    rre, poses = [], []
    for sc in scenes:
        cr = net.shape_prior_encode(ew, ecfg, sc["ref"].transpose(1, 2).contiguous())
        cs = net.shape_prior_encode(ew, ecfg, sc["rescan"].transpose(1, 2).contiguous())
        mm = more.sequential_matcher(cr["z_inv"], cs["z_inv"])["matches0"]
        ok += int((mm == torch.arange(6)).sum()); tot += 6
        R, t, _, _ = more.kabsch_transformation_estimation(cr["z_so3"] + cr["t"], cs["z_so3"] + cs["t"])
        gt = more.se3_concatenate(sc["rescan_T"][:, :3], more.se3_inverse(sc["ref_T"][:, :3]))
        e = more.rotation_error(R, gt[:, :, :3]).reshape(-1)
        rre.append(torch.minimum(torch.minimum(e, (180 - e).abs()), (90 - e).abs()))
        poses.append(torch.cat([R, t], 2))
    assert abs(m["object_recall"] - 100.0 * ok / tot) < 1e-9
    # parity at the level of the rotation matrices / translations (north_star: pose within 1e-4 rel) ...
    want = torch.cat(poses).numpy()
    assert relerr(r["poses"][:, :, :3], want[:, :, :3]) < 1e-4 and relerr(r["poses"][:, :, 3], want[:, :, 3]) < 1e-4
    # ... the angle in degrees is an ill-conditioned function of the matrix near 0 (acos'(1) is infinite): an R error of 1e-6
    # moves a 0.02-degree angle by ~0.01 degree, so the DERIVED metric is compared at 2e-2 degrees
    assert np.allclose(r["rre"], torch.cat(rre).numpy(), atol=2e-2)


# ------------------------------------------------------------------------------------------------ MISE (first half)
def _golden_mise():
    import os
    return np.load(os.path.join(os.path.dirname(__file__), "golden", "mise.npz"))


@pytest.mark.gpu
def test_mise_device_matches_reference_golden():
    """csrc/mise.hip through the reference's MISE surface (query / update / to_dense) on the golden cases recorded from the
    reference's Cython MISE: the same lattice points are queried in every round and the dense grid is bit-identical."""
    from livingscenes_amd.mesh_extractor2 import MISE
    from mise_fields import FIELDS
    g = _golden_mise()
    for key in sorted(k[:-4] for k in g.files if k.endswith("_cfg")):
        res0, depth, thr = g[key + "_cfg"]
        name = key.rsplit("_", 2)[0]
        m = MISE(int(res0), int(depth), float(thr), device="cuda:0")
        G = m.resolution + 1
        pts, rounds = m.query(), 0
        while pts.shape[0] != 0:
            assert np.array_equal((pts[:, 0] * G + pts[:, 1]) * G + pts[:, 2], g[key + f"_round{rounds}"]), (key, rounds)
            pf = np.float32(1.1) * (pts.astype(np.float32) / np.float32(m.resolution) - np.float32(0.5))
            m.update(pts, FIELDS[name](pf))
            pts = m.query()
            rounds += 1
        assert rounds == int(g[key + "_nrounds"]), key
        assert np.array_equal(m.to_dense().astype(np.float32), g[key + "_dense"]), key


@pytest.mark.gpu
@pytest.mark.parametrize("res0,steps", [(16, 2), (32, 2), (24, 1)])
def test_generator3d_eval_grid_vs_oracle(small_prior, res0, steps):
    """Generator3D.eval_grid (device MISE + ls_sdf_decode, zero-copy) vs the oracle's MISE driven by the SAME device decoder:
    the query coordinates computed on the device equal the reference's float32 formula bit for bit, so the value grids must be
    identical; plus the grid equals the dense evaluation wherever MISE evaluated a point."""
    from livingscenes_amd.mesh_extractor2 import Generator3D
    from oracle import mise as om
    sp, _ = small_prior
    code = sp.encode(synth.make_instances(1, 128, seed=21).to(_dev()))
    gen = Generator3D(threshold=0.5, resolution0=res0, upsampling_steps=steps, padding=0.1)
    stats = {}
    grid = gen.eval_grid(code, sp.decoder, stats_dict=stats)

    def field(pf):
        with torch.no_grad():
            return sp.decoder(torch.from_numpy(pf).to(_dev())[None], None, code).logits[0].cpu().numpy()
    tr = []
    ref = om.run(field, res0, steps, threshold=0.0, box_size=1.1, trace=tr)
    assert [len(r) for r in tr] == stats["mise rounds"]
    assert grid.shape == ((res0 << steps) + 1,) * 3 and np.array_equal(grid, ref)


# ------------------------------------------------------------------------------------------------ marching cubes (second half)
@pytest.mark.gpu
def test_marching_cubes_device_matches_reference_golden():
    """csrc/mcubes.hip vs the meshes recorded from the reference's libmcubes: same vertices (float64, bit for bit), same faces,
    same ORDER of both."""
    import os
    from livingscenes_amd.mesh_extractor2 import marching_cubes
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "mcubes.npz"))
    for name in sorted(k[:-4] for k in g.files if k.endswith("_vol")):
        v, f = marching_cubes(torch.from_numpy(g[name + "_vol"]).to(_dev()), float(g[name + "_iso"]))
        assert np.array_equal(v.cpu().numpy(), g[name + "_v"]), name
        assert np.array_equal(f.cpu().numpy(), g[name + "_f"]), name


@pytest.mark.gpu
def test_generator3d_mesh_vs_oracle(small_prior):
    """Generator3D.generate_from_latent end to end (device MISE + decoder + device marching cubes) vs the oracle chain on the
    same value grid: identical vertices and faces; the mesh is closed (every edge shared by exactly two faces)."""
    from livingscenes_amd.mesh_extractor2 import Generator3D
    from oracle import mcubes as om
    sp, _ = small_prior
    code = sp.encode(synth.make_instances(1, 128, seed=22).to(_dev()))
    gen = Generator3D(threshold=0.5, resolution0=16, upsampling_steps=2, padding=0.1)
    grid = gen.eval_grid(code, sp.decoder)
    level = float(np.median(grid))                       # the synthetic field has no zero level set: cut it at its median
    gen.threshold = 1.0 / (1.0 + np.exp(-level))
    grid = gen.eval_grid(code, sp.decoder)
    mesh = gen.extract_mesh(grid, None, code)
    thr = np.log(gen.threshold) - np.log(1.0 - gen.threshold)
    v, f = om.marching_cubes(np.pad(grid, 1, "constant", constant_values=-1e6), thr)
    n = np.array(grid.shape) - 1
    v = 1.1 * ((v - 0.5 - 1) / n - 0.5)
    assert len(f) > 100
    assert np.array_equal(np.asarray(mesh.vertices), v) and np.array_equal(np.asarray(mesh.faces), f)
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    _, cnt = np.unique(e, axis=0, return_counts=True)
    assert (cnt == 2).all()


@pytest.mark.gpu
def test_more_solver_mesh_from_latent(small_prior):
    """More_Solver._mesh_from_latent (more_solver.py:37-58): canonical mesh scaled by s and moved to t; the code dict is
    left as it was."""
    from livingscenes_amd.lib_more.more_solver import More_Solver
    sp, _ = small_prior
    code = sp.encode(synth.make_instances(1, 128, seed=23).to(_dev()))
    solver = More_Solver({"mesh_extractor": dict(threshold=0.5, resolution0=16, upsampling_steps=1, padding=0.1)}, model=sp)
    canon = {k: v.clone() for k, v in code.items()}
    canon["t"], canon["s"] = torch.zeros_like(code["t"]), torch.ones_like(code["s"])
    grid = solver.mesh_extractor.eval_grid(canon, sp.decoder)
    level = float(np.median(grid))
    solver.mesh_extractor.threshold = 1.0 / (1.0 + np.exp(-level))
    t0, s0 = code["t"].clone(), code["s"].clone()
    mesh = solver._mesh_from_latent(code)
    assert torch.equal(code["t"], t0) and torch.equal(code["s"], s0)
    ref = solver.mesh_extractor.extract_mesh(solver.mesh_extractor.eval_grid(canon, sp.decoder), None, canon)
    want = np.asarray(ref.vertices) * float(s0) + t0.view(-1).cpu().numpy()
    assert len(mesh.faces) > 50 and np.allclose(np.asarray(mesh.vertices), want, rtol=0, atol=1e-12)


@pytest.mark.gpu
def test_more_solver_from_released_mesh_extractor_section(small_prior):
    """More_Solver built from the VERBATIM mesh_extractor section of the released configs/more_3rscan.yaml:19-26 (it sets
    simplify_nfaces: 5000, which round 1 refused): _mesh_from_latent extracts (MISE 32 -> 128, marching cubes) and decimates like
    Generator3D.extract_mesh (mesh_extractor2.py:205-208 -> libsimplify.simplify_mesh(mesh, 5000, 5.0))."""
    import yaml
    from livingscenes_amd.lib_more.more_solver import More_Solver
    from livingscenes_amd import mesh_extractor2
    released = yaml.safe_load("""
mesh_extractor:
  threshold: 0.5
  resolution0: 32
  upsampling_steps: 2
  sample: False
  simplify_nfaces: 5000
  points_batch_size: 10000
  refinement_step: 0
""")
    sp, _ = small_prior
    code = sp.encode(synth.make_instances(1, 128, seed=23).to(_dev()))
    solver = More_Solver(released, model=sp)
    canon = {k: v.clone() for k, v in code.items()}
    canon["t"], canon["s"] = torch.zeros_like(code["t"]), torch.ones_like(code["s"])
    grid = solver.mesh_extractor.eval_grid(canon, sp.decoder)
    solver.mesh_extractor.threshold = 1.0 / (1.0 + np.exp(-float(np.median(grid))))   # untrained weights: put the level set inside the box
    mesh = solver._mesh_from_latent(code)
    nf = len(mesh.faces)
    assert 50 < nf <= 5001
    # the same grid without decimation has (many) more faces, and decimating it by hand gives the same mesh
    solver.mesh_extractor.simplify_nfaces = None
    full = solver.mesh_extractor.extract_mesh(solver.mesh_extractor.eval_grid(canon, sp.decoder), None, canon)
    assert len(full.faces) > nf
    v, f = mesh_extractor2.simplify_mesh_arrays(np.asarray(full.vertices), np.asarray(full.faces), 5000, 5.0)
    want = v * float(code["s"]) + code["t"].view(-1).cpu().numpy()
    assert np.array_equal(f, np.asarray(mesh.faces)) and np.allclose(np.asarray(mesh.vertices), want, rtol=0, atol=1e-12)


# ------------------------------------------------------------------------------------------------ code optimisation
@pytest.mark.gpu
def test_more_solver_optimize_code_vs_oracle_loop(small_prior):
    """More_Solver._optimize_code (more_solver.py:191-228: Adam on z_inv / t / z_so3 against the SDF at the observed points) with
    the decoder forward + backward in the HIP library vs the same loop on the CPU oracle with torch autograd."""
    from livingscenes_amd.lib_more.more_solver import More_Solver
    from oracle import net
    sp, (ecfg, dcfg, ew, dw) = small_prior
    dev = _dev()
    x = synth.make_instances(1, 128, seed=31)
    code = sp.encode(x.to(dev))
    pc = x[0].to(dev)                                           # [3, N]
    mask = torch.ones(1, 128, dtype=torch.bool, device=dev)
    solver = More_Solver({"shape_priors": {"n_input_point": 128}}, model=sp)
    start = {k: v.detach().clone() for k, v in code.items()}
    steps = 25
    best = solver._optimize_code({k: v.detach().clone() for k, v in code.items()}, pc, mask, n_steps=steps)
    # oracle loop (same FPS subset: n_input_point == N keeps every point, order by FPS)
    from livingscenes_amd.model_utils import fps
    pts, _ = fps(pc.T[None], K=128)
    c = {k: v.cpu().clone() for k, v in start.items()}
    params = [{"params": c["z_inv"], "lr": 1e-5}, {"params": c["t"], "lr": 1e-4}, {"params": c["z_so3"], "lr": 5e-4}]
    for p in params:
        p["params"].requires_grad_(True)
    opt = torch.optim.Adam(params)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[160], gamma=0.1)
    for _ in range(steps):
        opt.zero_grad()
        sdf = net.field_query_with_grad(dw, dcfg, pts.cpu(), c)
        loss = torch.nn.functional.mse_loss(sdf, torch.zeros_like(sdf))
        loss.backward()
        opt.step()
        sched.step()
    for k in ("z_inv", "z_so3", "t"):
        moved = float((c[k].detach() - start[k].cpu()).abs().max())
        assert moved > 0
        assert float((best[k].cpu() - c[k].detach()).abs().max()) < 2e-3 * moved + 1e-7, k
    assert torch.equal(best["s"].cpu(), start["s"].cpu())


@pytest.mark.gpu
def test_optim_registration_refines_the_pose(small_prior):
    """More_Solver._solve_pairwise_registration(optim=True) (more_solver.py:118-189; manifold Adam + Sinkhorn are this build's
    definitions, PARITY UNPINNED): on a rigidly moved, re-sampled, noisy copy the refined pose is a proper rotation, stays close to
    the ground truth and is no worse than the Kabsch + ICP answer by more than a degree."""
    from livingscenes_amd.lib_more.more_solver import More_Solver
    from livingscenes_amd.lib_more.pose_estimation import rotation_error, translation_error
    sp, _ = small_prior
    sc = synth.make_scene_pair(1, 128, seed=77, noise=0.002)
    dev = _dev()
    cfg = {"shape_priors": {"n_input_point": 128}, "fps": {"n_init": 1},
           "registration": {"step_size": {"so3": 0.01}, "n_steps": 40, "early_stop_threshold": 10}}
    solver = More_Solver(cfg, model=sp)
    pc1, pc2 = sc["ref"].to(dev), sc["rescan"].to(dev)
    from livingscenes_amd.lib_math.torch_se3 import concatenate, inverse
    gt = concatenate(sc["rescan_T"][:, :3], inverse(sc["ref_T"][:, :3])).to(dev)
    R0, t0 = solver._solve_pairwise_registration(pc1, pc2, optim=False)
    R1, t1 = solver._solve_pairwise_registration(pc1, pc2, optim=True)
    assert abs(float(torch.det(R1[0])) - 1) < 1e-4 and torch.allclose(R1[0] @ R1[0].T, torch.eye(3, device=dev), atol=1e-4)
    e0, e1 = float(rotation_error(R0, gt[:, :, :3])), float(rotation_error(R1, gt[:, :, :3]))
    assert e1 < e0 + 1.0 and e1 < 5.0, (e0, e1)
    assert float(translation_error(t1, gt[:, :, 3:4])) < 0.05


@pytest.mark.gpu
def test_optim_registration_batch_equals_per_pair(small_prior):
    """_solve_pairwise_registration_optim_batch (P pairs in lock-step, one launch sequence per Adam step) == the same function pair
    by pair, to 1e-5: clouds of different sizes and extents (different epsilon schedules of the Sinkhorn loop), both directions of
    the shared-code choice, and the info the kernel keeps per pair (min loss, stop flags)."""
    from livingscenes_amd.lib_more.more_solver import More_Solver
    sp, _ = small_prior
    dev = _dev()
    cfg = {"shape_priors": {"n_input_point": 128}, "fps": {"n_init": 1},
           "registration": {"step_size": {"so3": 0.01}, "n_steps": 24, "early_stop_threshold": 10}}
    solver = More_Solver(cfg, model=sp)
    p1, p2 = [], []
    for i, (n, scale) in enumerate(((300, 1.0), (128, 0.4), (500, 2.5), (222, 1.3), (150, 0.7))):
        sc = synth.make_scene_pair(1, n, seed=90 + i, noise=0.002)
        p1.append((sc["ref"][0] * scale).to(dev))
        p2.append((sc["rescan"][0] * scale).to(dev))
    R, t, info = solver._solve_pairwise_registration_optim_batch(p1, p2, return_info=True)
    assert R.shape == (5, 3, 3) and t.shape == (5, 3, 1) and info["steps"] == 24
    for i in range(5):
        Ri, ti, inf_i = solver._solve_pairwise_registration_optim_batch([p1[i]], [p2[i]], return_info=True)
        assert bool(inf_i["reverse"][0]) == bool(info["reverse"][i])
        assert relerr(info["pre_icp"][i:i + 1], inf_i["pre_icp"]) < 1e-5, i          # the refined pose before ICP
        assert abs(float(info["min_loss"][i]) - float(inf_i["min_loss"][0])) < 1e-5 * max(abs(float(inf_i["min_loss"][0])), 1e-3)
        assert relerr(R[i:i + 1], Ri) < 1e-4 and relerr(t[i:i + 1], ti) < 1e-4, i
    # the single-pair entry point of the reference's signature is the same path
    Rs, ts = solver._solve_pairwise_registration(p1[2][None], p2[2][None], optim=True)
    assert relerr(Rs, R[2:3]) < 1e-4
    # geodesic early stop: a threshold of 0 rad freezes every pair after its first step
    solver.cfg["registration"]["early_stop_threshold"] = 0.0
    _, _, info0 = solver._solve_pairwise_registration_optim_batch(p1[:2], p2[:2], return_info=True)
    assert info0["steps"] == 16 and not bool(info0["active"].any())


@pytest.mark.gpu
def test_softmin_multi_equals_single_launches():
    """ls_sinkhorn_softmin_multi_f32 (four independent softmins behind one launch) == four ls_sinkhorn_softmin_batched_f32 calls, bit
    for bit, with ragged sizes, a finished pair (eps <= 0 -> prev) and without potentials / prev."""
    from livingscenes_amd.sinkhorn import _softmin_b, _softmin_multi
    g = torch.Generator().manual_seed(3)
    P = 5
    x, y = (torch.randn(P, 300, 3, generator=g) * 0.4).to(_dev()), (torch.randn(P, 173, 3, generator=g) * 0.4).to(_dev())
    f, h = (torch.randn(P, 300, generator=g) * 0.1).to(_dev()), (torch.randn(P, 173, generator=g) * 0.1).to(_dev())
    eps = torch.tensor([0.5, 0.01, 0.0, 0.0025, 2.0]).to(_dev())
    probs = [(x, y, h, -5.1, f), (y, x, f, -5.7, h), (x, x, f, -5.7, f), (y, y, h, -5.1, h)]
    multi = _softmin_multi(probs, eps, True)
    for (a, b, pot, lw, prev), out in zip(probs, multi):
        assert torch.equal(out, _softmin_b(a, b, pot, lw, eps, prev=prev, average=True))
    e1 = torch.full((P,), 0.3).to(_dev())
    multi = _softmin_multi([(x, y, None, -5.1, None), (y, x, None, -5.7, None)], e1, False)
    assert torch.equal(multi[0], _softmin_b(x, y, None, -5.1, e1)) and torch.equal(multi[1], _softmin_b(y, x, None, -5.7, e1))


@pytest.mark.gpu
@pytest.mark.parametrize("P,N,M", [(3, 256, 300), (2, 1024, 1024)])
def test_sinkhorn_divergence_batch_vs_oracle(P, N, M):
    """sinkhorn.divergence_batch (per-pair epsilon schedules inside one launch sequence) against the torch-CPU restatement pair by
    pair (UNPINNED w.r.t. geomloss): loss and gradient; clouds of different extent so that the schedules differ in length."""
    from livingscenes_amd.sinkhorn import divergence_batch
    from oracle import sinkhorn as osk
    g = torch.Generator().manual_seed(P * 1000 + N)
    xs, ys = [], []
    for p in range(P):
        scale = (0.3, 1.0, 3.0)[p % 3]
        y = (torch.rand(M, 3, generator=g) - 0.5) * scale
        x = y[torch.randint(0, M, (N,), generator=g)] + 0.05 * scale * torch.randn(N, 3, generator=g)
        xs.append(x), ys.append(y)
    loss, grad = divergence_batch(torch.stack(xs).to(_dev()), torch.stack(ys).to(_dev()))
    for p in range(P):
        xr = xs[p].clone().requires_grad_(True)
        ref = osk.sinkhorn_divergence(xr, ys[p])
        ref.backward()
        assert abs(float(loss[p]) - float(ref)) < 2e-4 * max(abs(float(ref)), 1e-6) + 2e-7, p
        assert relerr(grad[p], xr.grad) < 5e-4, p


@pytest.mark.gpu
def test_optimize_code_batch_equals_per_instance(small_prior):
    """_optimize_code_batch (P instances per Adam step) == _optimize_code instance by instance."""
    from livingscenes_amd.lib_more.more_solver import More_Solver
    sp, _ = small_prior
    dev = _dev()
    solver = More_Solver({"shape_priors": {"n_input_point": 128}}, model=sp)
    clouds = [synth.make_instances(1, n, seed=50 + i)[0].T.contiguous().to(dev) for i, n in enumerate((200, 128, 321))]
    x = torch.stack([solver._sample([c], 128)[0] for c in clouds]).transpose(1, 2).contiguous()
    with torch.no_grad():
        code = sp.encode(x)
    start = {k: v.detach().clone() for k, v in code.items()}
    best, improved = solver._optimize_code_batch({k: v.detach().clone() for k, v in start.items()}, clouds, n_steps=30)
    assert bool(improved.all())
    for i, c in enumerate(clouds):
        one = {k: v[i:i + 1].detach().clone() for k, v in start.items()}
        pc = c.T.contiguous()
        mask = torch.ones(1, c.shape[0], dtype=torch.bool, device=dev)
        bi = solver._optimize_code(one, pc, mask, n_steps=30)
        for k in ("z_inv", "z_so3", "t"):
            moved = float((bi[k] - start[k][i:i + 1]).abs().max())
            assert moved > 0 and float((best[k][i:i + 1] - bi[k]).abs().max()) < 1e-5 * max(moved, 1e-6) + 1e-9, (i, k)


@pytest.mark.gpu
def test_solve_end2end_batch_equals_per_pair(small_prior):
    """lib_more.more_solver.solve_end2end_batch (all scans / pairs of several scenes in single launches) returns what
    _solve_end2end returns pair by pair: same matches, same registrations, same transformed codes."""
    from livingscenes_amd.lib_more.more_solver import More_Solver, solve_end2end_batch
    sp, _ = small_prior
    d = _dev()
    cfg = {"shape_priors": {"n_input_point": 128, "prior_name": "chair", "ckpt_dir": ""}, "fps": {"n_init": 1}}
    solver = More_Solver(cfg, model=sp)

    def scene(x, pad):
        n, N, _ = x.shape
        pc = torch.zeros(n, 3, N + pad)
        pc[:, :, :N] = x.transpose(1, 2)
        mask = torch.zeros(n, 1, N + pad, dtype=torch.bool)
        mask[:, :, :N] = True
        return {"pc": pc.to(d), "pc_mask": mask.to(d)}
    pairs = []
    for s, (n, N) in enumerate(((3, 200), (5, 150), (2, 333))):
        sc = synth.make_scene_pair(n, N, seed=60 + s, noise=0.002)
        pairs.append((scene(sc["ref"], 7 * s), scene(sc["rescan"], 11)))
    got = solve_end2end_batch(solver, pairs)
    for (ref, res), g in zip(pairs, got):
        w = solver._solve_end2end(ref, res)
        assert torch.equal(g["matches"], w["matches"])
        for i in range(len(w["registration"])):
            if w["registration"][i] is None:
                assert g["registration"][i] is None
                continue
            assert relerr(g["registration"][i], w["registration"][i]) < 1e-5
            for k in ("z_so3", "z_inv", "s", "t"):
                assert relerr(g["codes"][i][k], w["codes"][i][k]) < 1e-5


@pytest.mark.gpu
def test_ragged_decode_and_batched_mise_equal_per_instance(small_prior):
    """ls_sdf_decode_rows on rows of several instances == ls_sdf_decode per instance (bit for bit: every query is independent),
    and Generator3D.eval_grid_batch == eval_grid instance by instance."""
    from livingscenes_amd.mesh_extractor2 import Generator3D
    sp, _ = small_prior
    d = _dev()
    codes = sp.encode(synth.make_instances(3, 128, seed=41).to(d))
    hip = sp.hip_model()
    g = torch.Generator().manual_seed(3)
    counts = [700, 1, 333]
    qs = [(torch.rand(n, 3, generator=g) - 0.5).to(d) for n in counts]
    inst = torch.cat([torch.full((n,), b, dtype=torch.int32) for b, n in enumerate(counts)]).to(d)
    got = hip.sdf_decode_rows(torch.cat(qs, 0), inst, codes["z_so3"], codes["z_inv"], codes["s"], codes["t"])
    o = 0
    for b, n in enumerate(counts):
        one = hip.sdf_decode(qs[b][None], codes["z_so3"][b:b + 1], codes["z_inv"][b:b + 1], codes["s"][b:b + 1], codes["t"][b:b + 1])
        assert torch.equal(got[o:o + n], one[0]), b
        o += n
    gen = Generator3D(threshold=0.5, resolution0=8, upsampling_steps=2, padding=0.1)
    canon = {k: v.clone() for k, v in codes.items()}
    level = float(np.median(gen.eval_grid({k: v[:1] for k, v in canon.items()}, sp.decoder)))
    gen.threshold = 1.0 / (1.0 + np.exp(-level))
    grids = gen.eval_grid_batch(canon, sp.decoder)
    for b in range(3):
        assert np.array_equal(grids[b], gen.eval_grid({k: v[b:b + 1] for k, v in canon.items()}, sp.decoder)), b


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["inner_deepsdf", "deepsdf"])
def test_ragged_decode_at_slab_and_instance_edges(kind, small_prior):
    """ls_sdf_decode_rows == ls_sdf_decode of each instance alone, bit for bit, where the affine kernel's 64-row slabs and the instance
    boundaries meet: a boundary exactly on a slab edge, a one-row instance opening a slab, an instance without rows (its id is skipped,
    as eval_grid_batch does when an octree finishes early), last slabs of 3 rows and of one row, several instance changes inside one
    wave's stride, and a single row.  Width 128 leaves half the lanes of the 256-column block outside the layer."""
    from livingscenes_amd.model_utils import Shape_Prior
    d = _dev()
    if kind == "inner_deepsdf":
        sp = small_prior[0]
    else:
        ecfg, dcfg = synth.small_encoder_cfg(), synth.small_inv_decoder_cfg()
        sp = Shape_Prior.from_state(ecfg, dcfg, synth.make_encoder_weights(ecfg, 4), synth.make_decoder_weights(dcfg, 4), device=d, n_pcl=128,
                                    decoder_type="deepsdf")
    codes = sp.encode(synth.make_instances(5, 128, seed=43).to(d))
    hip = sp.hip_model()
    g = torch.Generator().manual_seed(7)
    for counts in ([64, 1, 0, 129, 1], [1, 1, 1, 61, 1], [0, 0, 1, 0, 0]):
        qs = [(torch.rand(n, 3, generator=g) - 0.5).to(d) for n in counts]
        inst = torch.cat([torch.full((n,), b, dtype=torch.int32) for b, n in enumerate(counts)]).to(d)
        got = hip.sdf_decode_rows(torch.cat(qs, 0), inst, codes["z_so3"], codes["z_inv"], codes["s"], codes["t"])
        assert got.shape == (sum(counts),)
        o = 0
        for b, n in enumerate(counts):
            if n:
                one = hip.sdf_decode(qs[b][None], codes["z_so3"][b:b + 1], codes["z_inv"][b:b + 1], codes["s"][b:b + 1], codes["t"][b:b + 1])
                assert torch.equal(got[o:o + n], one[0]), (counts, b)
            o += n


# ------------------------------------------------------------------------------------------------ multi-GPU path on one device
_SHARD_WORKER = r"""
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, %r)
from livingscenes_amd import sharding, synth
from livingscenes_amd.model_utils import Shape_Prior
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%%d" %% int(sys.argv[1]), rank=int(sys.argv[2]), world_size=int(sys.argv[3]))
rank = dist.get_rank()
dev = torch.device("cuda:0")                       # both ranks share the one device of the test box: a logic check, not a measurement
ecfg, dcfg = synth.small_encoder_cfg(), synth.small_decoder_cfg()
if rank == 0:
    ew, dw = synth.make_encoder_weights(ecfg, 4), synth.make_decoder_weights(dcfg, 4)
else:                                              # other ranks start from zeros and receive rank 0's weights
    ew = {k: torch.zeros(s) for k, s in synth.encoder_param_shapes(ecfg).items()}
    dw = {k: torch.zeros_like(v) for k, v in synth.make_decoder_weights(dcfg, 4).items()}
sp = Shape_Prior.from_state(ecfg, dcfg, ew, dw, device=dev)
sharding.broadcast_weights(sp, src=0)
for n in (7, 2, 1):                                # ragged shards (4 + 3), one instance per rank, and an EMPTY shard on rank 1
    x = synth.make_instances(n, 128, seed=30 + n).to(dev)
    with torch.no_grad():
        allc = sharding.sharded_encode(sp, x)
        whole = sp.encode(x)
    for k in ("z_so3", "z_inv", "s", "t"):
        assert allc[k].shape == whole[k].shape, (n, k, allc[k].shape, whole[k].shape)
        assert torch.equal(allc[k], whole[k]), (n, k)   # sharded == unsharded, bit for bit (a row's code does not depend on its batch)
dist.barrier()
dist.destroy_process_group()
print("rank", rank, "ok")
"""


@pytest.mark.gpu
def test_sharded_encode_world_size_2_on_one_device(tmp_path):
    """The N > 1 path of SURVEY 8(e) on the single-GPU test box: two processes (gloo rendezvous, both on cuda:0) broadcast the
    weights, encode their block of the instance list and all-gather the codes; every rank must end up with exactly the codes of
    the unsharded encode -- including ragged shards and an empty one (fewer instances than ranks)."""
    import os
    import socket
    import subprocess
    import sys
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    script = tmp_path / "shard_worker.py"
    script.write_text(_SHARD_WORKER % os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, str(script), str(port), str(r), "2"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)
             for r in range(2)]
    for r, p in enumerate(procs):
        out, err = p.communicate(timeout=600)
        assert p.returncode == 0 and f"rank {r} ok" in out, err[-3000:]


_SHARD_SKEW_WORKER = r"""
import os, sys, numpy as np, torch, torch.distributed as dist
sys.path.insert(0, %r)
from livingscenes_amd import sharding, synth
from livingscenes_amd.model_utils import Shape_Prior
ws = int(sys.argv[3])
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%%d" %% int(sys.argv[1]), rank=int(sys.argv[2]), world_size=ws)
rank = dist.get_rank()
dev = torch.device("cuda:0")
ecfg, dcfg = synth.small_encoder_cfg(), synth.small_decoder_cfg()
sp = Shape_Prior.from_state(ecfg, dcfg, synth.make_encoder_weights(ecfg, 4), synth.make_decoder_weights(dcfg, 4), device=dev, n_pcl=128)
# deliberately skewed raw clouds (configs[3]: 1 k - 60 k points per 3RScan instance), the big ones FIRST: the block partition would hand
# rank 0 almost everything
rng = np.random.default_rng(7)
sizes = sorted(np.exp(rng.uniform(np.log(300.0), np.log(20000.0), 36)).astype(int).tolist(), reverse=True)
g = torch.Generator().manual_seed(3)
clouds = [torch.randn(n, 3, generator=g).to(dev) for n in sizes]
seen = []
enc = sp.encode_fps
def spy(pc, mask):
    seen.append(int(mask.sum()))
    return enc(pc, mask)
sp.encode_fps = spy
codes = sharding.sharded_encode_fps(sp, clouds)
sp.encode_fps = enc
mine = torch.tensor([float(sum(seen))])
tot = [torch.zeros(1) for _ in range(ws)]
dist.all_gather(tot, mine)
tot = [float(t) for t in tot]
assert abs(sum(tot) - sum(sizes)) < 0.5, (tot, sum(sizes))
mean = sum(tot) / ws
assert max(tot) <= 1.1 * mean and min(tot) >= 0.9 * mean, ("per-rank point totals", tot)
block = [sum(sizes[i] for i in range(*sharding.shard_range(len(sizes), r, ws))) for r in range(ws)]
assert max(block) > 1.5 * mean                     # the partition this replaces was that bad on this list
# list order restored, every code equal to the unsharded encode of the same cloud (a row's code does not depend on the batch it rides in)
mx = max(sizes)
buf = torch.zeros(len(sizes), 3, mx, device=dev)
mask = torch.zeros(len(sizes), 1, mx, dtype=torch.bool, device=dev)
for i, c in enumerate(clouds):
    buf[i, :, : c.shape[0]] = c.T
    mask[i, :, : c.shape[0]] = True
whole = sp.encode_fps(buf, mask)
for k in ("z_so3", "z_inv", "s", "t"):
    assert torch.equal(codes[k], whole[k]), k
dist.barrier()
dist.destroy_process_group()
print("rank", rank, "ok")
"""


@pytest.mark.gpu
def test_sharded_encode_fps_balances_skewed_clouds_world_size_3_on_one_device(tmp_path):
    """SURVEY 8(e), configs[3]: three processes (gloo, all on cuda:0) share a list of 36 raw clouds of 300 - 20 000 points, largest first.
    sharded_encode_fps hands them out by cost (sharding.balanced_assignment): every rank's point total within 10 % of the mean (the block
    partition would give rank 0 more than 1.5x), the codes come back in list order and equal the unsharded encode bit for bit."""
    import os
    import socket
    import subprocess
    import sys
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    script = tmp_path / "skew_worker.py"
    script.write_text(_SHARD_SKEW_WORKER % os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, str(script), str(port), str(r), "3"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)
             for r in range(3)]
    for r, p in enumerate(procs):
        out, err = p.communicate(timeout=600)
        assert p.returncode == 0 and f"rank {r} ok" in out, err[-3000:]


_SHARD_E2E_WORKER = r"""
import os, sys, numpy as np, torch, torch.distributed as dist
sys.path.insert(0, %r)
from livingscenes_amd import sharding, synth
from livingscenes_amd.lib_more.more_solver import More_Solver, solve_end2end_batch
from livingscenes_amd.model_utils import Shape_Prior
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%%d" %% int(sys.argv[1]), rank=int(sys.argv[2]), world_size=int(sys.argv[3]))
rank = dist.get_rank()
dev = torch.device("cuda:0")
ecfg, dcfg = synth.small_encoder_cfg(), synth.small_decoder_cfg()
sp = Shape_Prior.from_state(ecfg, dcfg, synth.make_encoder_weights(ecfg, 4), synth.make_decoder_weights(dcfg, 4), device=dev, n_pcl=128)
cfg = {"shape_priors": {"n_input_point": 128}, "fps": {"n_init": 1},
       "registration": {"step_size": {"so3": 0.01}, "n_steps": 8, "early_stop_threshold": 10},
       "mesh_extractor": dict(threshold=0.5, resolution0=16, upsampling_steps=1, padding=0.1, points_batch_size=100000)}
solver = More_Solver(cfg, model=sp)
rng = np.random.default_rng(2)
pairs = []
for s, n in enumerate((3, 1, 4)):                  # 3 scene pairs, 16 instances in all: ragged blocks; 7 matched pairs: 4 + 3
    shapes = rng.integers(0, 10 ** 6, n)
    pairs.append((synth.make_raw_scan(shapes, 10 * s, 200, 900, device=dev)[0], synth.make_raw_scan(shapes, 10 * s + 1, 200, 900, device=dev)[0]))
code0 = sp.encode_fps(pairs[0][0]["pc"][:1], pairs[0][0]["pc_mask"][:1])
canon = {k: v.clone() for k, v in code0.items()}
canon["t"], canon["s"] = torch.zeros_like(canon["t"]), torch.ones_like(canon["s"])
solver.mesh_extractor.threshold = 1.0 / (1.0 + np.exp(-float(np.median(solver.mesh_extractor.eval_grid(canon, sp.decoder)))))
whole = solve_end2end_batch(solver, pairs, mesh=True)
part = solve_end2end_batch(solver, pairs, mesh=True, sharded=True)
n_slots = sum(int((w["matches"] >= 0).sum()) for w in whole)
lo, hi = sharding.shard_range(n_slots)
k = 0
for w, o in zip(whole, part):
    assert torch.equal(w["matches"], o["matches"])
    for i, (a, b) in enumerate(zip(w["registration"], o["registration"])):
        assert (a is None) == (b is None)
        if a is None:
            continue
        assert torch.equal(a, b), "pose: sharded != unsharded"
        assert all(torch.equal(w["codes"][i][key], o["codes"][i][key]) for key in ("z_so3", "z_inv", "s", "t"))
        mine = lo <= k < hi                          # meshes live on the rank that owns the pair
        assert (o["mesh_lst"][i] is not None) == mine, (k, lo, hi)
        if mine:
            assert np.array_equal(np.asarray(w["mesh_lst"][i].vertices), np.asarray(o["mesh_lst"][i].vertices))
            assert np.array_equal(np.asarray(w["mesh_lst"][i].faces), np.asarray(o["mesh_lst"][i].faces))
        k += 1
# the optim=True branch (eval_3rscan.py:381): 8 steps, every pair advances exactly as if alone
wo = solve_end2end_batch(solver, pairs, optim=True)
po = solve_end2end_batch(solver, pairs, optim=True, sharded=True)
for w, o in zip(wo, po):
    for a, b in zip(w["registration"], o["registration"]):
        assert (a is None) == (b is None) and (a is None or float((a - b).abs().max()) < 1e-5)
# configs[4]: dense grids by instance block
x = synth.make_instances(5, 128, seed=3).to(dev)
codes = sp.encode(x)
q = synth.make_queries(1, 4096, seed=1).to(dev)
full = sp.decoder(q.expand(5, -1, -1).contiguous(), None, codes, return_sdf=True)
b0, b1, loc = sharding.sharded_sdf_grid(sp, codes, q)
assert torch.equal(loc, full[b0:b1])
_, _, allg = sharding.sharded_sdf_grid(sp, codes, q, gather=True)
assert torch.equal(allg, full)
dist.barrier()
dist.destroy_process_group()
print("rank", rank, "ok")
"""


@pytest.mark.gpu
def test_sharded_end2end_and_dense_world_size_2_on_one_device(tmp_path):
    """configs[3] / configs[4] sharded (eval_3rscan.py:337-463,466-502) with the real kernels: two processes (gloo, both on
    cuda:0) run solve_end2end_batch(sharded=True) -- block-partitioned FPS + encode, all-gathered codes, replicated matchers,
    block-partitioned Kabsch + ICP (and the optim refinement), all-gathered (R | t), meshes on the owning rank -- and the dense SDF
    grids by instance block: every pose, code, mesh and grid equals the unsharded run BIT FOR BIT (optim=True: 1e-5)."""
    import os
    import socket
    import subprocess
    import sys
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    script = tmp_path / "shard_e2e_worker.py"
    script.write_text(_SHARD_E2E_WORKER % os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, str(script), str(port), str(r), "2"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)
             for r in range(2)]
    for r, p in enumerate(procs):
        out, err = p.communicate(timeout=900)
        assert p.returncode == 0 and f"rank {r} ok" in out, err[-3000:]
