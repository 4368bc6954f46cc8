"""GPU tests of the ragged matcher batches (ls_*_batch_f32, ops.*_batch, matcher_new.*_matcher_batch, the batched modes of More_Solver,
solve_end2end_batch and the harness).  The contract: for every problem of a batch every output is BIT-IDENTICAL to the single op on that
problem alone (torch.equal throughout; no tolerance anywhere in this file)."""
import numpy as np
import pytest
import torch

from livingscenes_amd import synth

pytestmark = pytest.mark.gpu

# n x m on every edge a kernel choice hangs on -- n m in {1, 64, 65, 1024, 1025, 4096, 4097}: one wave | four waves | 1024 threads for the
# greedy loop, one launch | two launches for the scores -- then 1 x k, k x 1 and rectangular both ways
EDGE = [(1, 1), (8, 8), (5, 13), (32, 32), (25, 41), (64, 64), (17, 241), (1, 40), (40, 1), (1, 70), (3, 50), (50, 3), (100, 20), (20, 100),
        (2, 32), (7, 9), (4, 16), (16, 4), (33, 31), (12, 12)]
BIG = (150, 150)          # nn / sinkhorn: more than 64 KB of LDS
EMPTY = [(0, 5), (4, 0)]


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _sizes(P):
    if P == 1:
        return [(32, 32)]
    if P == 9:
        return [(1, 1), (5, 13), (32, 32), EMPTY[0], BIG, EMPTY[1], (25, 41), (17, 241), (1, 40)]
    s = (EDGE * 4)[:P - 3]
    return s[:30] + [EMPTY[0], BIG, EMPTY[1]] + s[30:]


_cache = {}


def _descs(P, D):
    """P ragged problems of width D: lists of source / target descriptors on the device, the targets noisy permuted copies of the sources (made once)"""
    if (P, D) not in _cache:
        gen = torch.Generator().manual_seed(100 * P + D)
        a, b = [], []
        for n, m in _sizes(P):
            x = torch.randn(n, D, generator=gen)
            k = min(n, m)
            y = torch.cat([x[torch.randperm(n, generator=gen)[:k]] + 0.4 * torch.randn(k, D, generator=gen), torch.randn(m - k, D, generator=gen)], 0)
            a.append(x.to(_dev()))
            b.append(y[torch.randperm(m, generator=gen)].to(_dev()))
        _cache[(P, D)] = (a, b)
    return _cache[(P, D)]


def _empty_matches(n, m, squeeze=False):
    a, b = torch.full((n,), -1, dtype=torch.int64, device=_dev()), torch.full((m,), -1, dtype=torch.int64, device=_dev())
    return (a.squeeze(), b.squeeze()) if squeeze else (a, b)


def _assert_pairs_equal(got, want, what):
    assert len(got) == len(want), what
    for p, (g, w) in enumerate(zip(got, want)):
        for x, y in zip(g, w):
            assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y), (what, p, tuple(x.shape), tuple(y.shape))


# ------------------------------------------------------------------------------------------------ 1. batch == single, bit for bit
@pytest.mark.parametrize("D", [256, 64, 70])
@pytest.mark.parametrize("P", [1, 9, 70])
def test_raw_batch_ops_equal_the_single_ops(P, D):
    from livingscenes_amd import ops
    a, b = _descs(P, D)
    sizes = _sizes(P)
    # scores: list form and packed form
    S1 = [ops.cosine_scores(x, y) if x.shape[0] and y.shape[0] else torch.empty(x.shape[0], y.shape[0], device=_dev()) for x, y in zip(a, b)]
    SB = ops.cosine_scores_batch(a, b)
    _assert_pairs_equal([(s,) for s in SB], [(s,) for s in S1], "cosine_scores")
    packed, got_sizes = ops.cosine_scores_batch(torch.cat(a, 0), torch.cat(b, 0), sizes=sizes, packed=True)
    assert got_sizes == sizes and torch.equal(packed, torch.cat([s.reshape(-1) for s in S1]))
    # the three assignments on those scores
    single = lambda fn, squeeze=False: [fn(s) if s.numel() else _empty_matches(*s.shape) for s in S1]
    keep = packed.clone()
    _assert_pairs_equal(ops.greedy_match_batch(S1), single(ops.greedy_match), "greedy_match")
    _assert_pairs_equal(ops.greedy_match_batch(packed, sizes), single(ops.greedy_match), "greedy_match (packed)")
    assert torch.equal(packed, keep), "greedy_match_batch works on its own copy"
    _assert_pairs_equal(ops.nn_match_batch(S1), single(ops.nn_match), "nn_match")
    for thr in (0.0, 0.2):
        _assert_pairs_equal(ops.sinkhorn_match_batch(packed, D ** 0.5, match_threshold=thr, sizes=sizes),
                            single(lambda s: ops.sinkhorn_match(s, D ** 0.5, match_threshold=thr)), f"sinkhorn_match thr {thr}")


@pytest.mark.parametrize("P,C", [(1, 256), (9, 256), (70, 256), (9, 300)])
def test_residual_matrix_batch_equals_single(P, C):
    """256 pseudo-points (the register-resident path) and more than 256 (the rolled loops)"""
    from livingscenes_amd import ops
    gen = torch.Generator().manual_seed(7 * P + C)
    sizes = [(n, m) for n, m in _sizes(P) if n * m <= 1100] + EMPTY + ([BIG] if P == 9 and C == 256 else [])
    src = [torch.randn(n, C, 3, generator=gen).to(_dev()) for n, _ in sizes]
    tgt = [torch.randn(m, C, 3, generator=gen).to(_dev()) for _, m in sizes]
    want = [ops.kabsch_residual_matrix(s, t) if s.shape[0] and t.shape[0] else torch.empty(s.shape[0], t.shape[0], device=_dev())
            for s, t in zip(src, tgt)]
    _assert_pairs_equal([(r,) for r in ops.kabsch_residual_matrix_batch(src, tgt)], [(w,) for w in want], "kabsch_residual_matrix")
    packed, _ = ops.kabsch_residual_matrix_batch(torch.cat(src, 0), torch.cat(tgt, 0), sizes=sizes, packed=True)
    assert torch.equal(packed, torch.cat([w.reshape(-1) for w in want]))


def _dicts_equal(got, want, what):
    assert len(got) == len(want)
    for p, (g, w) in enumerate(zip(got, want)):
        assert sorted(g) == sorted(w) == ["matches0", "matches1"]
        for k in g:
            assert g[k].dtype == torch.int64 and g[k].shape == w[k].shape and torch.equal(g[k], w[k]), (what, p, k, tuple(g[k].shape), tuple(w[k].shape))


@pytest.mark.parametrize("D", [256, 70])
@pytest.mark.parametrize("P", [1, 9, 70])
def test_matcher_batch_functions_equal_the_single_matchers(P, D):
    from livingscenes_amd.lib_more import matcher_new as mn
    a, b = _descs(P, D)

    def each(fn, squeeze, *lists):
        out = []
        for args in zip(*lists):
            n, m = _n(args[0]), _n(args[1])
            out.append(fn(*args) if n and m else dict(zip(("matches0", "matches1"), _empty_matches(n, m, squeeze))))
        return out
    _n = lambda x: x["z_inv"].shape[0] if isinstance(x, dict) else (x.shape[2] if x.dim() == 3 else x.shape[0])
    _dicts_equal(mn.sequential_matcher_batch(a, b), each(mn.sequential_matcher, False, a, b), "sequential")
    da, db = [x.T[None] for x in a], [y.T[None] for y in b]
    _dicts_equal(mn.nn_matcher_batch(da, db), each(mn.nn_matcher, True, da, db), "nn")
    _dicts_equal(mn.sinkhorn_matcher_batch(da, db, desc_dim=D), each(lambda x, y: mn.sinkhorn_matcher(x, y, desc_dim=D), True, da, db), "sinkhorn")
    _dicts_equal(mn.sinkhorn_matcher_batch(da, db, desc_dim=D, match_threshold=0.2),
                 each(lambda x, y: mn.sinkhorn_matcher(x, y, desc_dim=D, match_threshold=0.2), True, da, db), "sinkhorn thr")
    # the two matchers on equivariant codes: problems of at most 1100 pairs (every greedy class) plus the empty ones
    gen = torch.Generator().manual_seed(P + D)
    keep = [i for i, (n, m) in enumerate(_sizes(P)) if n * m <= 1100]
    src = [{"z_inv": a[i], "z_so3": torch.randn(a[i].shape[0], 256, 3, generator=gen).to(_dev())} for i in keep]
    tgt = [{"z_inv": b[i], "z_so3": torch.randn(b[i].shape[0], 256, 3, generator=gen).to(_dev())} for i in keep]
    _dicts_equal(mn.sim3_seq_matcher_batch(src, tgt), each(mn.sim3_seq_matcher, False, src, tgt), "sim3_seq")
    _dicts_equal(mn.eq_seq_matcher_batch(src, tgt), each(mn.eq_seq_matcher, False, src, tgt), "eq_seq")


# ------------------------------------------------------------------------------------------------ 2. against the reference's fixtures
def _np_equal(r, g, m0, m1, what):
    assert r["matches0"].shape == g[m0].shape and r["matches1"].shape == g[m1].shape, what
    assert np.array_equal(r["matches0"].cpu().numpy(), g[m0]) and np.array_equal(r["matches1"].cpu().numpy(), g[m1]), what


def test_sequential_family_batches_vs_golden(golden):
    from livingscenes_amd.lib_more import matcher_new as mn
    g = golden("matchers")
    d = _dev()
    names = ("n1", "n2", "n3", "n5", "n32", "neg", "tie")
    res = mn.sequential_matcher_batch([torch.from_numpy(g[f"seq_{n}_a"]).to(d) for n in names], [torch.from_numpy(g[f"seq_{n}_b"]).to(d) for n in names])
    for n, r in zip(names, res):
        _np_equal(r, g, f"seq_{n}_m0", f"seq_{n}_m1", n)
    src = {"z_inv": torch.from_numpy(g["eqsrc_z_inv"]).to(d), "z_so3": torch.from_numpy(g["eqsrc_z_so3"]).to(d)}
    tgt = {"z_inv": torch.from_numpy(g["eqtgt_z_inv"]).to(d), "z_so3": torch.from_numpy(g["eqtgt_z_so3"]).to(d)}
    for nm, fn in (("eq", mn.eq_seq_matcher_batch), ("sim3", mn.sim3_seq_matcher_batch)):
        for r in fn([src] * 5, [tgt] * 5):
            _np_equal(r, g, f"{nm}_m0", f"{nm}_m1", nm)


def test_assignment_batches_vs_golden(golden):
    from livingscenes_amd.lib_more import matcher_new as mn
    g = golden("matchers_assign")
    d = _dev()
    for group in ([n for n in g["names"] if n != "dim64"], ["dim64"]):
        da = [torch.from_numpy(g[f"{n}_a"]).to(d).T[None] for n in group]
        db = [torch.from_numpy(g[f"{n}_b"]).to(d).T[None] for n in group]
        D = da[0].shape[1]
        for n, r in zip(group, mn.nn_matcher_batch(da, db)):
            _np_equal(r, g, f"{n}_nn_m0", f"{n}_nn_m1", n)
        for n, r in zip(group, mn.sinkhorn_matcher_batch(da, db, desc_dim=D)):
            _np_equal(r, g, f"{n}_sk_m0", f"{n}_sk_m1", n)
        # the threshold holds for the whole batch: one call per stored threshold, the case it belongs to is compared
        for n in group:
            r = mn.sinkhorn_matcher_batch(da, db, desc_dim=D, match_threshold=float(g[f"{n}_sk_thr"]))[group.index(n)]
            _np_equal(r, g, f"{n}_skt_m0", f"{n}_skt_m1", n)


# ------------------------------------------------------------------------------------------------ 3. isolation
@pytest.mark.parametrize("n,m", [(6, 7), (20, 30), (40, 40)])     # the three greedy kernels
def test_a_nan_problem_and_an_all_negative_problem_do_not_touch_their_neighbours(n, m):
    from livingscenes_amd import ops
    gen = torch.Generator().manual_seed(n)
    ordinary = [torch.rand(n, m, generator=gen).to(_dev()) for _ in range(2)]
    nan = torch.rand(n, m, generator=gen)
    nan[n // 2, m // 3] = float("nan")
    neg = -torch.rand(n, m, generator=gen) - 1e-3          # every score <= -1e-5: the greedy denominators are not positive
    S = [ordinary[0], nan.to(_dev()), neg.to(_dev()), ordinary[1]]
    for what, batch, single in (("greedy", ops.greedy_match_batch, ops.greedy_match), ("nn", ops.nn_match_batch, ops.nn_match),
                                ("sinkhorn", lambda s: ops.sinkhorn_match_batch(s, 16.0), lambda s: ops.sinkhorn_match(s, 16.0))):
        got, want = batch(S), [single(s) for s in S]
        _assert_pairs_equal(got, want, what)
        alone = batch([ordinary[0], ordinary[1]])
        _assert_pairs_equal([got[0], got[3]], alone, what + ": neighbours")


# ------------------------------------------------------------------------------------------------ 4. streams
def test_match_batch_ops_beside_encode_stream():
    """the batch ops on one stream while another runs Shape_Prior.encode: the same results as alone"""
    from livingscenes_amd import ops
    from livingscenes_amd.model_utils import Shape_Prior
    ecfg, dcfg = synth.small_encoder_cfg(), synth.small_decoder_cfg()
    sp = Shape_Prior.from_state(ecfg, dcfg, synth.make_encoder_weights(ecfg, 2), synth.make_decoder_weights(dcfg, 2), device=_dev(), n_pcl=256)
    x = synth.make_instances(64, 256, seed=5).to(_dev())
    a, b = _descs(9, 64)
    gen = torch.Generator().manual_seed(3)
    src = [torch.randn(n, 256, 3, generator=gen).to(_dev()) for n in (3, 0, 9)]
    tgt = [torch.randn(m, 256, 3, generator=gen).to(_dev()) for m in (4, 5, 9)]

    def run():
        S = ops.cosine_scores_batch(a, b)
        out = [tuple(S), tuple(ops.kabsch_residual_matrix_batch(src, tgt))]
        for pairs in (ops.greedy_match_batch(S), ops.nn_match_batch(S), ops.sinkhorn_match_batch(S, 8.0)):
            out.append(tuple(t for pair in pairs for t in pair))
        return out
    alone = [[t.cpu() for t in r] for r in run()]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    for _ in range(2):
        with torch.no_grad(), torch.cuda.stream(s2):
            for _ in range(3):
                sp.encode(x)
        with torch.cuda.stream(s1):
            res = run()
        torch.cuda.synchronize()
        for w, r in zip(alone, res):
            assert len(w) == len(r) and all(torch.equal(u, v.cpu()) for u, v in zip(w, r))


# ------------------------------------------------------------------------------------------------ 5. surface
@pytest.fixture(scope="module")
def small_solver():
    from livingscenes_amd.lib_more.more_solver import More_Solver
    from livingscenes_amd.model_utils import Shape_Prior
    ecfg, dcfg = synth.small_encoder_cfg(), synth.small_decoder_cfg()
    sp = Shape_Prior.from_state(ecfg, dcfg, synth.make_encoder_weights(ecfg, 4), synth.make_decoder_weights(dcfg, 4), device=_dev(), n_pcl=128)
    return More_Solver({"shape_priors": {"n_input_point": 128, "prior_name": "chair", "ckpt_dir": ""}, "fps": {"n_init": 1}}, model=sp)


def test_solver_matching_batch_equals_per_pair_for_all_five_methods(small_solver):
    sp = small_solver.model
    src, tgt = [], []
    for s, (n, m) in enumerate(((3, 3), (12, 9), (5, 7), (8, 8), (4, 11), (10, 10))):
        sc = synth.make_scene_pair(max(n, m), 128, seed=70 + s, noise=0.002)
        with torch.no_grad():
            src.append(sp.encode(sc["ref"][:n].transpose(1, 2).contiguous().to(_dev())))
            tgt.append(sp.encode(sc["rescan"][:m].transpose(1, 2).contiguous().to(_dev())))
    for method in ("sequential", "nn", "sinkhorn", "sim3_seq", "eq_seq"):
        got = small_solver._solve_object_matching_batch(src, tgt, method)
        _dicts_equal(got, [small_solver._solve_object_matching(a, b, method) for a, b in zip(src, tgt)], method)
    assert small_solver._solve_object_matching_batch([], [], "sequential") == []


def test_end2end_batch_and_harness_batched_modes_equal_the_defaults(small_solver):
    from livingscenes_amd import harness
    from livingscenes_amd.lib_more.more_solver import solve_end2end_batch
    d = _dev()

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
    want = solve_end2end_batch(small_solver, pairs)
    got = solve_end2end_batch(small_solver, pairs, match_batched=True)
    for w, g in zip(want, got):
        assert torch.equal(w["matches"], g["matches"])
        for a, b in zip(w["registration"], g["registration"]):
            assert (a is None) == (b is None) and (a is None or torch.equal(a, b))
        for a, b in zip(w["codes"], g["codes"]):
            assert (a is None) == (b is None) and (a is None or all(torch.equal(a[k], b[k]) for k in a))
    scenes = [synth.make_scene_pair(n, 128, seed=40 + i, noise=0.002) for i, n in enumerate((6, 4, 1))]
    for method in ("sequential", "nn"):
        assert harness.eval_matching(scenes, small_solver, method, batched=True) == harness.eval_matching(scenes, small_solver, method)


# ------------------------------------------------------------------------------------------------ 6. argument errors on the device path
def test_argument_errors():
    from livingscenes_amd import _lib, ops
    d = _dev()
    ok = torch.rand(5, 6, device=d)
    m0_before = ops.nn_match_batch([ok])
    with pytest.raises(_lib.LsError, match=r"problem 1: a 300 x 300 problem needs \d+ bytes of LDS"):
        ops.sinkhorn_match_batch([ok, torch.zeros(300, 300, device=d), ok], 16.0)
    with pytest.raises(_lib.LsError, match="problem 2"):
        ops.nn_match_batch([ok, ok, torch.zeros(250, 250, device=d)])
    _assert_pairs_equal(ops.nn_match_batch([ok]), m0_before, "after a refusal")
    with pytest.raises(ValueError, match="width"):
        ops.cosine_scores_batch([torch.rand(3, 64, device=d), torch.rand(3, 32, device=d)], [torch.rand(2, 64, device=d), torch.rand(2, 32, device=d)])
    with pytest.raises(ValueError):
        ops.cosine_scores_batch([torch.rand(3, 64, device=d)], [torch.rand(2, 32, device=d)])
    with pytest.raises(ValueError):
        ops.greedy_match_batch(torch.rand(30, device=d), sizes=[(5, 5)])
    with pytest.raises(ValueError):
        ops.greedy_match_batch(torch.rand(30, device=d))
