"""GPU tests of the scene-memory merge (csrc/cloudmerge.hip: ls_cloud_merge_f32 / ls_cloud_merge_batch_f32; ops.cloud_merge /
cloud_merge_batch) and of the layers on top of it (More_Solver._accumulate_batch, solve_sequence).

The operator is held INTEGER-EXACT to tests/merge_oracle.py: out_src and out_off equal, out_pts equal bit for bit (compared as uint32).  The
only tolerance in this file is the coverage bound of the _accumulate_batch test, sqrt(3) h + 1e-5: a dropped point shares a voxel of edge h
with a kept one (the diagonal is sqrt(3) h), and 1e-5 covers the fp32 transform there and back of coordinates below 4 (a few ulp of 2.4e-7
each).  The solve_sequence test runs untrained weights and makes no accuracy claim."""
import math

import numpy as np
import pytest
import torch

import merge_oracle as mo
from cloud_testlib import CODE_KEYS, STEP_KEYS, TILE, _bits, _dev, _pose, _scene, _solver, _t, small_prior  # noqa: F401 (small_prior is a fixture)
from livingscenes_amd import synth

pytestmark = pytest.mark.gpu


def _single(A, B, g, h):
    from livingscenes_amd import ops
    pts, src = ops.cloud_merge(_t(A), _t(B), g=None if g is None else torch.from_numpy(np.asarray(g, np.float32)).to(_dev()), voxel=h)
    assert pts.dtype == torch.float32 and src.dtype == torch.int32 and pts.shape == (src.shape[0], 3)
    return pts.cpu().numpy(), src.cpu().numpy()


def _check(A, B, g, h, what=""):
    """the single op on (A, B, g, h) against the oracle -> (pts, src) of the device"""
    A, B = np.asarray(A, np.float32).reshape(-1, 3), np.asarray(B, np.float32).reshape(-1, 3)
    got, want = _single(A, B, g, h), mo.merge(A, B, g, h)
    assert got[1].shape == want[1].shape, (what, got[1].shape, want[1].shape)
    assert np.array_equal(got[1], want[1]), (what, "src")
    assert np.array_equal(_bits(got[0]), _bits(want[0])), (what, "pts")
    return got


# ------------------------------------------------------------------------------------------------ size edges, P = 1
K = 13          # the table-size edge: n = 2^K and 2^K + 1 candidates (tables of 2^(K+1) and 2^(K+1) + 2 slots)
SIZES = [(0, 0), (0, 1), (1, 0), (1, 1), (255, 1), (256, 1), (200, 57)] + \
        [(TILE - 1 - 100, 100), (TILE - 100, 100), (TILE + 1 - 100, 100), (TILE, TILE - 1), (TILE, TILE), (TILE + 1, TILE)] + \
        [(2 ** K - 1000, 1000), (2 ** K - 1000, 1001), (0, 2 ** K + 1), (2 ** K + 1, 0)]


@pytest.mark.parametrize("a,b", SIZES)
def test_size_edges(a, b):
    assert TILE == 4096
    rng = np.random.default_rng(1000 * a + b)
    A, B = rng.uniform(-1, 1, (a, 3)).astype(np.float32), rng.uniform(-1, 1, (b, 3)).astype(np.float32)
    for h in (0.11, 1e-4):                      # many candidates per voxel; nearly every candidate alone
        pts, src = _check(A, B, None, h, f"{a}+{b} h={h}")
        assert pts.shape[0] <= a + b and (a + b == 0 or pts.shape[0] >= 1)
    _check(A, B, _pose(rng), 0.11, f"{a}+{b} posed")


def test_one_cell_own_cells_and_exact_copy():
    rng = np.random.default_rng(3)
    A, B = rng.uniform(0.01, 0.99, (3000, 3)).astype(np.float32), rng.uniform(0.01, 0.99, (2000, 3)).astype(np.float32)
    pts, src = _check(A, B, None, 1.0, "one cell")                       # all candidates in one cell: the first one stays
    assert src.tolist() == [0] and np.array_equal(_bits(pts[0]), _bits(A[0]))
    pts, src = _check(A[:0], B, None, 1.0, "one cell, empty memory")
    assert src.tolist() == [0] and np.array_equal(_bits(pts[0]), _bits(B[0]))
    grid = (np.stack(np.meshgrid(*[np.arange(-8, 9)] * 3, indexing="ij"), -1).reshape(-1, 3) + 0.5).astype(np.float32)   # 17^3 own cells
    grid = grid[rng.permutation(grid.shape[0])]
    pts, src = _check(grid[:3000], grid[3000:], None, 1.0, "own cells")
    assert np.array_equal(src, np.arange(grid.shape[0])) and np.array_equal(_bits(pts), _bits(grid))
    eye = np.eye(3, 4, dtype=np.float32)
    for g in (None, eye):                                                # B an exact copy of A: nothing of B is kept
        pts, src = _check(A, A.copy(), g, 0.05, "copy")
        assert (src < A.shape[0]).all() and 0 < src.shape[0] <= A.shape[0]


@pytest.mark.parametrize("name", ("line", "plane", "lattice", "lattice_2^8", "lattice_2^16"))
def test_regular_cells_long_probe_chains(name):
    """cell patterns a weak hash would chain: every cell twice (once per cloud, shuffled), so exactly the first cloud stays"""
    if name == "line":
        c = np.stack([np.arange(4096) - 2048, np.zeros(4096), np.zeros(4096)], 1)
    elif name == "plane":
        c = np.stack(np.meshgrid(np.arange(64) - 32, np.arange(64) - 32, [7], indexing="ij"), -1).reshape(-1, 3)
    else:
        stride = {"lattice": 1, "lattice_2^8": 2 ** 8, "lattice_2^16": 2 ** 16}[name]
        c = (np.stack(np.meshgrid(*[np.arange(16) - 8] * 3, indexing="ij"), -1).reshape(-1, 3)) * stride
    rng = np.random.default_rng(5)
    A = (c[rng.permutation(len(c))] + 0.25).astype(np.float32)           # exact in fp32: |c| <= 2^19
    B = (c[rng.permutation(len(c))] + 0.75).astype(np.float32)
    pts, src = _check(A, B, None, 1.0, name)
    assert np.array_equal(src, np.arange(len(c)))
    pts, src = _check(B[:1000], A, None, 1.0, name + " partly known")
    assert src.shape[0] == len(c)


def test_signs_faces_clamp_and_non_finite():
    rng = np.random.default_rng(7)
    # negative and mixed-sign coordinates, +-0.0, and +-(k h) exactly: h = 0.25 (1 / h exact) and h = 0.1 (not exact)
    for h in (0.25, 0.1):
        k = np.arange(-9, 10, dtype=np.float32)
        on = (k * np.float32(h)).astype(np.float32)
        faces = np.stack(np.meshgrid(on, on[::3], [-on[2], np.float32(-0.0), np.float32(0.0)], indexing="ij"), -1).reshape(-1, 3)
        near = np.nextafter(faces[:100], np.float32(-np.inf)).astype(np.float32)     # one ulp below a face: the cell before
        mixed = (rng.uniform(-2, 2, (800, 3)) * rng.choice([-1, 1], (800, 3))).astype(np.float32)
        A = np.concatenate([faces, mixed[:400]])[rng.permutation(len(faces) + 400)]
        B = np.concatenate([near, -faces, mixed[400:]])
        _check(A, B, None, h, f"faces h={h}")
        _check(A, B, _pose(rng), h, f"faces h={h} posed")
    # |y inv| beyond 2^30: the clamp collects them per sign and axis
    big = np.float32([[3e9, 0, 0], [5e9, 0.1, 0.2], [-3e9, 0, 0], [-1e30, 0.3, 0.1], [1e38, 1e38, -1e38], [2.0 ** 29, 0, 0], [2.0 ** 29 + 64, 0, 0],
                      [0.1, 6e8, -7e8], [0.2, 9e8, -9e8], [2.0 ** 30, 0, 0], [-2.0 ** 30, 0, 0]])
    pts, src = _check(big[:6], big[6:], None, 0.5, "clamp")
    assert 1 not in src.tolist() and 0 in src.tolist() and 2 in src.tolist() and 3 not in src.tolist()
    _check(big, big[::-1].copy(), None, 1e-3, "clamp small h")
    # non-finite rows in A and in B occupy no cell and never come out
    A = rng.uniform(-1, 1, (500, 3)).astype(np.float32)
    B = rng.uniform(-1, 1, (500, 3)).astype(np.float32)
    A[0], A[17], A[499] = [np.nan, 0, 0], [0, np.inf, 0], [-np.inf, np.nan, 1]
    B[0], B[250], B[499] = [0, 0, np.nan], [np.inf, np.inf, np.inf], [1, -np.inf, 1]
    for g in (None, _pose(rng)):
        pts, src = _check(A, B, g, 0.2, "non-finite")
        assert np.isfinite(pts).all() and not set(src.tolist()) & {0, 17, 499, 500, 750, 999}
    pts, src = _check(np.full((300, 3), np.nan, np.float32), np.full((5, 3), np.inf, np.float32), None, 0.2, "nothing finite")
    assert src.shape[0] == 0


def test_pose_transform_bits_and_kept_set():
    rng = np.random.default_rng(11)
    A = rng.uniform(-1.5, 1.5, (3000, 3)).astype(np.float32)
    B = rng.uniform(-1.5, 1.5, (5000, 3)).astype(np.float32)
    g = _pose(rng, 2.0)
    pts, src = _check(A, B, g, 0.07, "posed")
    fromB = src >= A.shape[0]
    assert fromB.any() and (~fromB).any()
    Y = mo.transform(B, g)                                               # the stated expression, evaluated in NumPy fp32
    assert np.array_equal(_bits(pts[fromB]), _bits(Y[src[fromB] - A.shape[0]]))
    assert np.array_equal(_bits(pts[~fromB]), _bits(A[src[~fromB]]))
    want = mo.merge_brute(A[:300], B[:300], g, 0.07)                     # and the kept set is the literal rule's
    got = _single(A[:300], B[:300], g, 0.07)
    assert np.array_equal(got[1], want[1]) and np.array_equal(_bits(got[0]), _bits(want[0]))
    g4 = np.concatenate([g, [[0, 0, 0, 1]]], 0).astype(np.float32)       # [4,4] is read as its first three rows
    got4 = _single(A, B, g4, 0.07)
    assert np.array_equal(got4[1], src) and np.array_equal(_bits(got4[0]), _bits(pts))


# ------------------------------------------------------------------------------------------------ the ragged batch
BATCH_SIZES = [(0, 0), (0, 300), (300, 0), (1, 1), (1025, 4097), (5000, 5000)]
BATCH_VOXELS = [0.05, 0.2, 0.01, 0.5, 0.03, 0.11]


@pytest.fixture(scope="module")
def batch():
    rng = np.random.default_rng(13)
    As = [rng.uniform(-1, 1, (a, 3)).astype(np.float32) for a, _ in BATCH_SIZES]
    Bs = [rng.uniform(-1, 1, (b, 3)).astype(np.float32) for _, b in BATCH_SIZES]
    gs = np.stack([_pose(rng) for _ in BATCH_SIZES])
    return As, Bs, gs


def _run_batch(As, Bs, gs, hs, packed=True):
    from livingscenes_amd import ops
    g = None if gs is None else torch.from_numpy(np.ascontiguousarray(gs)).to(_dev())
    return ops.cloud_merge_batch([_t(A) for A in As], [_t(B) for B in Bs], g=g, voxel=hs, packed=packed)


@pytest.mark.parametrize("posed", (False, True))
def test_batch_against_oracle_single_reversed_and_again(batch, posed):
    As, Bs, gs = batch
    gs = gs if posed else None
    pts, src, off = _run_batch(As, Bs, gs, BATCH_VOXELS)
    wp, wsrc, woff = mo.merge_batch(As, Bs, gs, BATCH_VOXELS)
    assert off.dtype == np.int64 and np.array_equal(off, woff) and off[1] == 0
    assert np.array_equal(src.cpu().numpy(), wsrc) and np.array_equal(_bits(pts), _bits(wp))
    for p in range(len(As)):                                             # every problem: the bits of the single op on it alone
        sp, ss = _single(As[p], Bs[p], None if gs is None else gs[p], BATCH_VOXELS[p])
        assert np.array_equal(ss, wsrc[off[p]:off[p + 1]]) and np.array_equal(_bits(sp), _bits(wp[off[p]:off[p + 1]])), p
    rp, rs, roff = _run_batch(As[::-1], Bs[::-1], None if gs is None else gs[::-1], BATCH_VOXELS[::-1])
    P = len(As)
    for p in range(P):
        q = P - 1 - p
        assert np.array_equal(rs[roff[q]:roff[q + 1]].cpu().numpy(), wsrc[off[p]:off[p + 1]])
        assert np.array_equal(_bits(rp[roff[q]:roff[q + 1]]), _bits(wp[off[p]:off[p + 1]]))
    p2, s2, off2 = _run_batch(As, Bs, gs, BATCH_VOXELS)                  # a second run
    assert np.array_equal(off2, off) and torch.equal(s2, src) and np.array_equal(_bits(p2), _bits(pts))
    lst = _run_batch(As, Bs, gs, BATCH_VOXELS, packed=False)             # the list form: views of the same result
    assert [x[0].shape[0] for x in lst] == np.diff(off).tolist()
    assert all(torch.equal(x[1], src[off[p]:off[p + 1]]) for p, x in enumerate(lst))
    one = _run_batch(As, Bs, gs, 0.05)                                   # a scalar voxel holds for every problem
    assert np.array_equal(one[2], mo.merge_batch(As, Bs, gs, [0.05] * P)[2])


def test_batch_errors_name_the_problem(batch):
    from livingscenes_amd import _lib, ops
    As, Bs, _ = batch
    d = _dev()
    tA, tB = [_t(A) for A in As], [_t(B) for B in Bs]
    P = len(As)
    for bad in (0.0, -1.0, float("nan")):
        hs = list(BATCH_VOXELS)
        hs[4] = bad
        with pytest.raises(_lib.LsError, match="problem 4.*voxel"):
            ops.cloud_merge_batch(tA, tB, voxel=hs)
    lib = _lib.load()
    A, B = torch.cat(tA), torch.cat(tB)
    ao, bo = ops._offsets([a for a, _ in BATCH_SIZES]), ops._offsets([b for _, b in BATCH_SIZES])
    n = A.shape[0] + B.shape[0]
    pts, src = torch.empty(n, 3, device=d), torch.empty(n, dtype=torch.int32, device=d)
    off = torch.empty(P + 1, dtype=torch.int64, device=d)
    ws = torch.empty(lib.ls_cloud_merge_batch_workspace_bytes(P, A.shape[0], B.shape[0]), dtype=torch.uint8, device=d)
    vx = np.asarray(BATCH_VOXELS, np.float32)

    def raw(ao_, bo_):
        return lib.ls_cloud_merge_batch_f32(P, _lib.ptr(A), A.shape[0], ops._hptr(ao_), _lib.ptr(B), B.shape[0], ops._hptr(bo_), None, ops._hptr(vx),
                                            _lib.ptr(pts), _lib.ptr(src), _lib.ptr(off), None, _lib.ptr(ws), ws.numel(), _lib.stream_ptr(d)), \
            lib.ls_last_error().decode()
    bad = ao.copy()
    bad[3] = bad[2] - 1                                                  # non-monotone at problem 2
    rc, msg = raw(bad, bo)
    assert rc == -1 and "problem 2" in msg and "a_off" in msg and "decreases" in msg, msg
    bad = bo.copy()
    bad[P] += 1                                                          # the wrong end
    rc, msg = raw(ao, bad)
    assert rc == -1 and f"problem {P - 1}" in msg and "b_off" in msg and "ends at" in msg, msg
    rc, msg = raw(ao, bo)                                                # and the untouched arrays go through
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert np.array_equal(off.cpu().numpy(), mo.merge_batch(As, Bs, None, BATCH_VOXELS)[2])
    # the Python surface: fp32 HIP tensors only, and it says that there is no CPU fallback
    with pytest.raises(_lib.LsError, match="no CPU fallback"):
        ops.cloud_merge(torch.zeros(3, 3), torch.zeros(3, 3), voxel=0.1)
    with pytest.raises(_lib.LsError, match="fp32"):
        ops.cloud_merge(torch.zeros(3, 3, device=d, dtype=torch.float64), torch.zeros(3, 3, device=d), voxel=0.1)
    with pytest.raises(ValueError):
        ops.cloud_merge_batch(tA, tB[:-1], voxel=0.1)
    with pytest.raises(ValueError):
        ops.cloud_merge_batch(tA, tB, voxel=[0.1, 0.2])


def test_large_and_idempotent():
    rng = np.random.default_rng(17)
    A = (rng.uniform(-1, 1, (120000, 3)) * [1.0, 0.6, 0.3]).astype(np.float32)      # 2 x 60 000 kept + 60 000 new
    B = (rng.uniform(-1, 1, (60000, 3)) * [1.0, 0.6, 0.3]).astype(np.float32)
    h = 0.01
    pts, src = _check(A, B, None, h, "large")
    assert 0 < (src >= 120000).sum() < 60000
    # merge(merge(A, B), {}) == merge(A, B); an output is kept whole by the next merge at the same h, whatever comes
    again, s2 = _check(pts, B[:0], None, h, "idempotent")
    assert np.array_equal(s2, np.arange(pts.shape[0])) and np.array_equal(_bits(again), _bits(pts))
    more, s3 = _check(pts, B, None, h, "the same observation again")
    assert np.array_equal(_bits(more), _bits(pts))
    # g == identity and g == NULL: the same result (finite rows without -0.0: 1 x + 0 y + 0 z + 0 is x bit for bit)
    assert not (np.signbit(B) & (B == 0)).any()
    pi, si = _single(A, B, np.eye(3, 4, dtype=np.float32), h)
    assert np.array_equal(si, src) and np.array_equal(_bits(pi), _bits(pts))


# ------------------------------------------------------------------------------------------------ the layers above


def test_accumulate_batch_known_pose_covers_the_shape():
    d = _dev()
    h = 0.02
    solver = _solver(object(), {"accumulate": {"voxel_size": h}})
    rng = np.random.default_rng(19)
    mems, news, Ts, fulls = [], [], [], []
    for seed in (3, 4):
        full = synth.canonical_shape(4096, seed).astype(np.float32)
        x = (full[:, 0] - 0.5 * (full[:, 0].max() + full[:, 0].min())) / (full[:, 0].max() - full[:, 0].min())
        one, two = full[x < 0.15], full[x > -0.15]
        g = _pose(rng, 1.5).astype(np.float64)                            # memory -> rescan
        moved = (two.astype(np.float64) @ g[:, :3].T + g[:, 3]).astype(np.float32)
        T = np.eye(4, dtype=np.float32)
        T[:3] = g
        mems.append(torch.from_numpy(one).to(d)), news.append(torch.from_numpy(moved).to(d)), Ts.append(T), fulls.append(torch.from_numpy(full).to(d))
    T = torch.from_numpy(np.stack(Ts)).to(d)
    for Tin in (T, T[:, :3].contiguous()):                               # [P,4,4] as Rt_to_SE3 gives it, or [P,3,4]
        merged = solver._accumulate_batch(mems, news, Tin)               # voxel from cfg['accumulate']['voxel_size']
        for full, one, moved, m in zip(fulls, mems, news, merged):
            assert m.shape[0] < one.shape[0] + moved.shape[0] and m.shape[0] > max(one.shape[0], moved.shape[0])
            assert torch.equal(m[:1], one[:1])                           # the memory's first point always stays
            reach = torch.cdist(full.double(), m.double()).min(1)[0].max()
            print(f"merged {m.shape[0]} of {one.shape[0]} + {moved.shape[0]}; farthest point of the shape {float(reach):.5f} (bound {math.sqrt(3) * h + 1e-5:.5f})")
            assert float(reach) <= math.sqrt(3) * h + 1e-5
    assert solver._accumulate_batch(mems, news, T, voxel=0.05)[0].shape[0] < merged[0].shape[0]          # an explicit voxel goes before the cfg's
    assert _solver(object())._accumulate_batch(mems, news, T)[0].shape[0] > merged[0].shape[0]      # the default voxel, 0.01


def test_solve_sequence_memory(small_prior):
    from livingscenes_amd.lib_more import more_solver
    solver = _solver(small_prior)
    n, h = 4, 0.02
    s1, s2 = synth.make_scene_pair(n, 700, seed=71, noise=0.002), synth.make_scene_pair(n, 500, seed=71, noise=0.004)
    ref, rescans = _scene(s1["ref"]), [_scene(s1["rescan"]), _scene(s2["rescan"])]
    steps, memory = more_solver.solve_sequence(solver, ref, rescans, mesh=False, voxel=h)
    assert len(steps) == 2 and memory["meshes"] is None and len(memory["clouds"]) == n
    assert all(memory["codes"][k].shape[0] == n for k in CODE_KEYS)
    matched = 0
    for k, st in enumerate(steps):
        assert set(st) == STEP_KEYS
        assert len(st["ref_pc_lst"]) == len(st["registration"]) == len(st["codes"]) == len(st["merged_sizes"]) == len(st["n_new_points"]) == n
        m0 = st["matches"].tolist()
        after = steps[k + 1]["ref_pc_lst"] if k + 1 < len(steps) else memory["clouds"]
        for i in range(n):
            before = st["ref_pc_lst"][i]
            a = before.shape[0]
            assert st["merged_sizes"][i] == after[i].shape[0] == a + st["n_new_points"][i]
            assert torch.equal(after[i][:a], before)                     # what the memory holds stays, row for row
            if m0[i] < 0:
                assert st["registration"][i] is None and st["codes"][i] is None and st["n_new_points"][i] == 0
            else:
                matched += 1
                assert st["registration"][i].shape == (1, 4, 4) and set(st["codes"][i]) == set(CODE_KEYS)
        assert sorted(st["unmatched_rescan"]) == sorted(set(range(n)) - {j for j in m0 if j >= 0})
    assert matched > 0, "the synthetic scene matched nothing: the test would show nothing"
    # the memory starts as the reference's clouds at one point per voxel
    raw = more_solver._scene_clouds(ref)
    for i in range(n):
        want, _ = mo.merge(raw[i].cpu().numpy(), np.zeros((0, 3), np.float32), None, h)
        assert np.array_equal(_bits(steps[0]["ref_pc_lst"][i]), _bits(want))
    # every code is encode_fps of its cloud as it was when the code was made: the merged cloud for slots that grew, the reference otherwise
    last = {}
    for k, st in enumerate(steps):
        for i in range(n):
            if st["n_new_points"][i] > 0:
                last[i] = (steps[k + 1]["ref_pc_lst"] if k + 1 < len(steps) else memory["clouds"])[i]
    assert last, "no slot grew"
    ref_codes = small_prior.encode_fps(ref["pc"], ref["pc_mask"])
    for i in range(n):
        if i in last:
            c = last[i]
            direct = small_prior.encode_fps(c.T[None].contiguous(), torch.ones(1, 1, c.shape[0], dtype=torch.bool, device=c.device))
            for key in CODE_KEYS:
                assert torch.equal(memory["codes"][key][i], direct[key][0]), (i, key)
        else:
            for key in CODE_KEYS:
                assert torch.equal(memory["codes"][key][i], ref_codes[key][i]), (i, key)


def test_solve_sequence_exact_copy_under_identity(small_prior, monkeypatch):
    """the rescan is the reference bit for bit and the registration is the identity (the untrained weights are taken out of the question by
    replacing the registration): nothing is new, no cloud and no code changes"""
    from livingscenes_amd.lib_more import more_solver
    solver = _solver(small_prior)
    n = 4
    ref = _scene(synth.make_scene_pair(n, 700, seed=72)["ref"])
    copy = {k: v.clone() for k, v in ref.items()}
    calls = []

    def identity(pcs1, pcs2, icp=True):
        calls.append(len(pcs1))
        d = pcs1[0].device
        return torch.eye(3, device=d).repeat(len(pcs1), 1, 1), torch.zeros(len(pcs1), 3, 1, device=d)
    monkeypatch.setattr(solver, "_solve_pairwise_registration_batch", identity)
    steps, memory = more_solver.solve_sequence(solver, ref, [copy, copy], voxel=0.02)
    ref_codes = small_prior.encode_fps(ref["pc"], ref["pc_mask"])
    for st in steps:
        m0 = st["matches"].tolist()
        assert sum(j >= 0 for j in m0) > 0 and calls and st["n_new_points"] == [0] * n
        for i in range(n):
            a = st["ref_pc_lst"][i].shape[0]
            assert st["merged_sizes"][i] == a and torch.equal(memory["clouds"][i][:a], st["ref_pc_lst"][i]) and memory["clouds"][i].shape[0] == a
    assert len(calls) == 2                                                # one registration call per rescan
    for key in CODE_KEYS:
        assert torch.equal(memory["codes"][key], ref_codes[key]), key


def test_solve_sequence_optimize_codes(small_prior, monkeypatch):
    """optimize_codes: ONE _optimize_code_batch call per step on the slots that grew, and a slot keeps the optimised code where its loss improved"""
    from livingscenes_amd.lib_more import more_solver
    solver = _solver(small_prior)
    n, h = 4, 0.02
    s1 = synth.make_scene_pair(n, 700, seed=71, noise=0.002)
    calls = []
    real = type(solver)._optimize_code_batch

    def recorded(code, pcs, n_steps=200):
        enc = {k: code[k].clone() for k in CODE_KEYS}
        opt, improved = real(solver, code, pcs, n_steps=8)               # eight of the 200 steps: the rule is under test, not the optimum
        calls.append((enc, {k: opt[k].clone() for k in CODE_KEYS}, improved.clone(), [p.shape[0] for p in pcs]))
        return opt, improved
    monkeypatch.setattr(solver, "_optimize_code_batch", recorded)
    steps, memory = more_solver.solve_sequence(solver, _scene(s1["ref"]), [_scene(s1["rescan"])], voxel=h, optimize_codes=True)
    grown = [i for i, k in enumerate(steps[0]["n_new_points"]) if k > 0]
    assert grown and len(calls) == 1 and calls[0][3] == [memory["clouds"][i].shape[0] for i in grown]
    enc, opt, improved, _ = calls[0]
    assert improved.dtype == torch.bool and improved.shape == (len(grown),)
    for r, i in enumerate(grown):
        for key in CODE_KEYS:
            want = opt[key][r] if bool(improved[r]) else enc[key][r]
            assert torch.equal(memory["codes"][key][i], want.to(memory["codes"][key].dtype)), (i, key)
