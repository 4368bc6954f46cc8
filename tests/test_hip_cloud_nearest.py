"""GPU tests of the scene memory's radius search (csrc/cloudnear.hip: ls_cloud_nearest_f32 / ls_cloud_nearest_batch_f32; ops.cloud_nearest /
cloud_nearest_batch) and of the layers on top of it (More_Solver._overlap_batch, the overlap gate of solve_sequence).

The operator is held to tests/nearest_oracle.py: nn_idx and counts equal as integers, nn_d2 equal bit for bit (compared as uint32).  The only
tolerance in this file is that of sum_d2, n_matched 2^-52 relative to the twin's math.fsum of the fp32 nn_d2 values: a float64 sum of n
non-negative terms in any order errs by at most (n - 1) 2^-53 relative, and fsum is the correctly rounded sum (another 2^-53).  Between the
single op and the batch sum_d2 is compared bit for bit.  _overlap_batch's rmse = sqrt(sum_d2 / matched) is held to the same bound: the root
halves the sum's error and adds, with the division, one rounding of 2^-53 each.  The solve_sequence tests run untrained weights with the
registration replaced, as the merge's identity test does, and make no accuracy claim."""
import math

import numpy as np
import pytest
import torch

import merge_oracle as mo
import nearest_oracle as no
from cloud_testlib import (CODE_KEYS, GATE_KEYS, STEP_KEYS, TILE, F, _bits, _dev, _g, _pose, _scene, _solver, _t,
                           small_prior)  # noqa: F401 (small_prior is a fixture)
from livingscenes_amd import synth

pytestmark = pytest.mark.gpu


def _host(res):
    idx, d2, counts, s = res
    assert idx.dtype == torch.int32 and d2.dtype == torch.float32 and idx.shape == d2.shape and idx.dim() == 1
    assert isinstance(counts, np.ndarray) and counts.dtype == np.int64 and counts.shape == (3,) and isinstance(s, float)
    return idx.cpu().numpy(), d2.cpu().numpy(), counts, s


def _single(A, B, g, r):
    from livingscenes_amd import ops
    return _host(ops.cloud_nearest(_t(A), _t(B), g=_g(g), radius=r))


def _against(got, want, what=""):
    assert got[0].shape == want[0].shape, (what, got[0].shape, want[0].shape)
    assert np.array_equal(got[0], want[0]), (what, "nn_idx", int((got[0] != want[0]).sum()))
    assert np.array_equal(_bits(got[1]), _bits(want[1])), (what, "nn_d2")
    assert np.array_equal(got[2], want[2]), (what, "counts", got[2], want[2])
    assert abs(got[3] - want[3]) <= int(want[2][1]) * 2.0 ** -52 * want[3], (what, "sum_d2", got[3], want[3])


def _identical(x, y, what=""):
    """two device results of one problem: every output the same bits"""
    assert np.array_equal(x[0], y[0]) and np.array_equal(_bits(x[1]), _bits(y[1])) and np.array_equal(x[2], y[2]), what
    assert np.float64(x[3]).view(np.uint64) == np.float64(y[3]).view(np.uint64), (what, x[3], y[3])


def _check(A, B, g, r, what=""):
    """the single op on (A, B, g, r) against the twin -> the device's (idx, d2, counts, sum)"""
    A, B = np.asarray(A, np.float32).reshape(-1, 3), np.asarray(B, np.float32).reshape(-1, 3)
    got = _single(A, B, g, r)
    _against(got, no.nearest(A, B, g, r), what)
    return got


# ------------------------------------------------------------------------------------------------ size edges, P = 1
# the scanned array is the per-slot count of the 2 a table: its tile edges are at a = TILE / 2 and a = TILE; 256 and 257: the chunk of queries
SIZES = [(0, 0), (0, 1), (1, 0), (1, 1), (255, 1), (256, 1), (1, 257), (200, 57)] + \
        [(TILE // 2 - 1, 300), (TILE // 2, 300), (TILE // 2 + 1, 300), (TILE - 1, 256), (TILE, 255), (TILE + 1, 513)] + \
        [(2 ** 13 - 1, 1000), (2 ** 13, 1001), (2 ** 13 + 1, 2 ** 13 + 1)]


@pytest.mark.parametrize("a,b", SIZES)
def test_size_edges(a, b):
    assert TILE == 4096
    rng = np.random.default_rng(1000 * a + b)
    A, B = rng.uniform(-0.4, 0.4, (a, 3)).astype(np.float32), rng.uniform(-0.4, 0.4, (b, 3)).astype(np.float32)
    k = min(a, b) // 2
    if k:
        B[:2 * k:2] = A[rng.integers(0, a, k)]      # exact duplicates of targets: all that r = 1e-4 can match
    got = _check(A, B, None, 0.11, f"{a}x{b} r=0.11")                      # some 400 cells: many members per cell
    assert k == 0 or got[2][1] >= k
    got = _check(A, B, None, 1e-4, f"{a}x{b} r=1e-4")
    assert got[2][1] >= k and (k == 0 or got[3] == 0.0)
    _check(A, B, _pose(rng, 0.2), 0.11, f"{a}x{b} posed")


# ------------------------------------------------------------------------------------------------ extreme cell shapes
def test_one_cell():
    rng = np.random.default_rng(3)
    A, B = rng.uniform(0.01, 0.99, (3000, 3)).astype(np.float32), rng.uniform(0.01, 0.99, (2000, 3)).astype(np.float32)
    for r in (1.0, 4.0):                                                 # every target is a candidate of every query
        idx, d2, counts, _ = _check(A, B, None, r, f"one cell r={r}")
        assert counts[0] == counts[1] == 2000
        assert np.array_equal(idx[:50], no._d2(B[:50, None, :], A[None]).argmin(1))       # every target compared: the first least one
    _check(A[:0], B, None, 1.0, "one cell, empty memory")
    _check(A, B[:0], None, 1.0, "one cell, no query")


@pytest.mark.parametrize("name", ("line", "plane", "lattice", "lattice_2^8", "lattice_2^16"))
def test_regular_cells_long_probe_chains(name):
    """cell patterns a weak hash would chain; every cell holds one target and one query 0.25 apart on every axis"""
    if name == "line":
        c = np.stack([np.arange(4096) - 2048, np.zeros(4096), np.zeros(4096)], 1)
    elif name == "plane":
        c = np.stack(np.meshgrid(np.arange(64) - 32, np.arange(64) - 32, [7], indexing="ij"), -1).reshape(-1, 3)
    else:
        stride = {"lattice": 1, "lattice_2^8": 2 ** 8, "lattice_2^16": 2 ** 16}[name]
        c = (np.stack(np.meshgrid(*[np.arange(16) - 8] * 3, indexing="ij"), -1).reshape(-1, 3)) * stride
    rng = np.random.default_rng(5)
    pa, pb = rng.permutation(len(c)), rng.permutation(len(c))
    A = (c[pa] + 0.25).astype(np.float32)                                # exact in fp32: |c| <= 2^19
    B = (c[pb] + 0.5).astype(np.float32)
    idx, d2, counts, s = _check(A, B, None, 1.0, name)                   # d2 = 3 / 16 in the own cell; the targets of the next cells are farther
    assert np.array_equal(pa[idx], pb) and (d2 == 0.1875).all() and counts.tolist() == [len(c)] * 3 and s == 0.1875 * len(c)
    _check(A[:1000], B, None, 1.0, name + " partly known")
    _check(A, B, None, 0.5, name + " r=0.5")


# ------------------------------------------------------------------------------------------------ the hand-written cases of the definition
def test_hand_written_cases():
    # d2 == r2 == 0.0625 but the cells are -1 and 1: no neighbour
    got = _check(F([[-1e-30, 0, 0]]), F([[0.25, 0, 0]]), None, 0.25, "two cells apart")
    assert got[0].tolist() == [-1] and np.isinf(got[1][0]) and got[2].tolist() == [1, 0, 0] and got[3] == 0.0
    # d2 == r2 within adjacent cells is a neighbour, the next fp32 above is not
    up = np.nextafter(F(0.25), F(1))
    got = _check(F([[0, 0, 0]]), F([[0.25, 0, 0], [up, 0, 0], [-0.25, 0, 0]]), None, 0.25, "inclusive radius")
    assert got[0].tolist() == [0, -1, 0] and got[1][0] == F(0.0625) and got[2].tolist() == [3, 2, 1] and got[3] == 0.125
    # two targets at equal d2: the lower index wins, whichever way round
    A = F([[9, 9, 9], [0.1, 0, 0], [-0.1, 0, 0], [0, 0.1, 0], [0.1, 0, 0]])
    assert _check(A, F([[0, 0, 0]]), None, 0.25, "tie")[0].tolist() == [1]
    assert _check(A[::-1].copy(), F([[0, 0, 0]]), None, 0.25, "tie reversed")[0].tolist() == [0]
    many = np.repeat(F([[0.3, 0.3, 0.3]]), 700, 0)                       # 700 copies in one cell: index 0, whatever order the members took
    got = _check(many, F([[0.3, 0.3, 0.3], [0.31, 0.3, 0.3]]), None, 0.05, "duplicates")
    assert got[0].tolist() == [0, 0] and got[2].tolist() == [2, 2, 1]
    # the clamp: rows at 1e12 with r = 0.5 share a cell
    got = _check(F([[1e12, 1e12, 1e12]]), F([[1e12, 1e12, 1e12], [-1e12, 0, 0]]), None, 0.5, "clamp")
    assert got[0].tolist() == [0, -1] and got[1][0] == 0.0
    big = F([[3e9, 0, 0], [5e9, 0.1, 0.2], [-3e9, 0, 0], [-1e30, 0.3, 0.1], [1e38, 1e38, -1e38], [2.0 ** 29, 0, 0], [2.0 ** 29 + 64, 0, 0],
             [0.1, 6e8, -7e8], [0.2, 9e8, -9e8], [2.0 ** 30, 0, 0], [-2.0 ** 30, 0, 0]])
    for r in (0.5, 1e-3, 100.0):
        _check(big, big[::-1].copy(), None, r, f"clamp r={r}")


def test_signs_faces_and_non_finite():
    rng = np.random.default_rng(7)
    for r in (0.25, 0.1):                                                # 1 / r exact, and not
        k = np.arange(-9, 10, dtype=np.float32)
        on = (k * F(r)).astype(np.float32)
        faces = np.stack(np.meshgrid(on, on[::3], [-on[2], F(-0.0), F(0.0)], indexing="ij"), -1).reshape(-1, 3)
        near = np.nextafter(faces[:100], F(-np.inf)).astype(np.float32)  # one ulp below a face: the cell before
        mixed = (rng.uniform(-2, 2, (800, 3)) * rng.choice([-1, 1], (800, 3))).astype(np.float32)
        A = np.concatenate([faces, mixed[:400]])[rng.permutation(len(faces) + 400)]
        B = np.concatenate([near, -faces, faces + F(r), mixed[400:]])    # faces + r: d2 at or around r2, one or two cells on
        _check(A, B, None, r, f"faces r={r}")
        _check(A, B, _pose(rng, 0.3), r, f"faces r={r} posed")
    A = rng.uniform(-1, 1, (500, 3)).astype(np.float32)
    B = rng.uniform(-1, 1, (500, 3)).astype(np.float32)
    A[0], A[17], A[499] = [np.nan, 0, 0], [0, np.inf, 0], [-np.inf, np.nan, 1]
    B[0], B[250], B[499] = [0, 0, np.nan], [np.inf, np.inf, np.inf], [1, -np.inf, 1]
    B[1], B[2] = [0, 0, 0], [0, 1, 0]                                    # next to the finite coordinates of A[0] and A[17]
    for g in (None, _pose(rng, 0.3)):
        idx, d2, counts, _ = _check(A, B, g, 0.3, "non-finite")
        assert counts[0] == 497 and not set(idx.tolist()) & {0, 17, 499} and idx[0] == idx[250] == idx[499] == -1
        assert np.isinf(d2[[0, 250, 499]]).all()
    got = _check(np.full((300, 3), np.nan, np.float32), np.full((5, 3), np.inf, np.float32), None, 0.2, "nothing finite")
    assert got[2].tolist() == [0, 0, 0] and got[3] == 0.0
    got = _check(np.full((300, 3), np.nan, np.float32), A, None, 0.2, "no finite target")
    assert got[2].tolist() == [497, 0, 0]


def test_pose_bits():
    rng = np.random.default_rng(11)
    A = rng.uniform(-1.5, 1.5, (3000, 3)).astype(np.float32)
    B = rng.uniform(-1.5, 1.5, (5000, 3)).astype(np.float32)
    B[::5] = A[rng.integers(0, 3000, 1000)]                              # planted exactly on targets
    idx, d2, counts, _ = _check(A, B, None, 0.07, "planted")
    assert not _bits(d2[::5]).any()                                      # g = None: B bit for bit, so the distance is +0.0
    assert np.array_equal(_bits(A[idx[::5]]), _bits(B[::5]))
    g = _pose(rng, 0.5)
    got = _check(A, B, g, 0.07, "posed")
    assert 0 < got[2][1] < 5000
    Y = mo.transform(B, g)                                               # the stated expression, evaluated in NumPy fp32
    has = got[0] >= 0
    assert np.array_equal(_bits(got[1][has]), _bits(no._d2(Y[has], A[got[0][has]])))
    _against(_single(A[:300], B[:300], g, 0.3), no.nearest_brute(A[:300], B[:300], g, 0.3), "the literal rule")
    g4 = np.concatenate([g, [[0, 0, 0, 1]]], 0).astype(np.float32)       # [4,4] is read as its first three rows
    _identical(_single(A, B, g4, 0.07), got, "[4,4]")


# ------------------------------------------------------------------------------------------------ the ragged batch
BATCH_SIZES = [(0, 300), (300, 0), (1, 1), (1025, 4097), (5000, 5000), (700, 257)]
BATCH_RADII = [0.05, 0.2, 0.01, 0.5, 0.03, 0.11]


@pytest.fixture(scope="module")
def batch():
    rng = np.random.default_rng(13)
    As = [rng.uniform(-0.5, 0.5, (a, 3)).astype(np.float32) for a, _ in BATCH_SIZES]
    Bs = [rng.uniform(-0.5, 0.5, (b, 3)).astype(np.float32) for _, b in BATCH_SIZES]
    Bs[2][0] = As[2][0] + F(0.001)
    gs = np.stack([_pose(rng, 0.1) for _ in BATCH_SIZES])
    twins = {posed: no.nearest_batch(As, Bs, gs if posed else None, BATCH_RADII) for posed in (False, True)}
    return As, Bs, gs, twins


def _run_batch(As, Bs, gs, rs, packed=False):
    from livingscenes_amd import ops
    return ops.cloud_nearest_batch([_t(A) for A in As], [_t(B) for B in Bs], g=_g(gs), radius=rs, packed=packed)


@pytest.mark.parametrize("posed", (False, True))
def test_batch_against_twin_single_reversed_and_again(batch, posed):
    As, Bs, gs, twins = batch
    gs = gs if posed else None
    P = len(As)
    res = [_host(x) for x in _run_batch(As, Bs, gs, BATCH_RADII)]
    assert sum(int(x[2][1]) for x in res) > 1000
    for p in range(P):
        _against(res[p], twins[posed][p], f"problem {p}")
        _identical(res[p], _single(As[p], Bs[p], None if gs is None else gs[p], BATCH_RADII[p]), f"problem {p} alone")
    rev = [_host(x) for x in _run_batch(As[::-1], Bs[::-1], None if gs is None else gs[::-1], BATCH_RADII[::-1])]
    again = [_host(x) for x in _run_batch(As, Bs, gs, BATCH_RADII)]
    for p in range(P):
        _identical(rev[P - 1 - p], res[p], f"problem {p} reversed")
        _identical(again[p], res[p], f"problem {p} again")
    idx, d2, counts, sums, off = _run_batch(As, Bs, gs, BATCH_RADII, packed=True)      # the packed form: the same result
    assert off.dtype == np.int64 and off.tolist() == np.cumsum([0] + [b for _, b in BATCH_SIZES]).tolist()
    assert counts.shape == (P, 3) and sums.dtype == np.float64 and sums.shape == (P,)
    assert np.array_equal(idx.cpu().numpy(), np.concatenate([x[0] for x in res])) and np.array_equal(counts, np.stack([x[2] for x in res]))
    assert np.array_equal(_bits(d2), _bits(np.concatenate([x[1] for x in res]))) and sums.tolist() == [x[3] for x in res]
    one = [_host(x) for x in _run_batch(As, Bs, gs, 0.05)]               # a scalar radius holds for every problem
    for p, want in enumerate(no.nearest_batch(As, Bs, gs, [0.05] * P)):
        _against(one[p], want, f"problem {p} r=0.05")


def test_batch_errors_name_the_problem(batch):
    from livingscenes_amd import _lib, ops
    As, Bs, _, _ = batch
    d = _dev()
    tA, tB = [_t(A) for A in As], [_t(B) for B in Bs]
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-45):
        rs = list(BATCH_RADII)
        rs[4] = bad
        with pytest.raises(_lib.LsError, match="problem 4.*radius"):
            ops.cloud_nearest_batch(tA, tB, radius=rs)
    with pytest.raises(_lib.LsError, match="no CPU fallback"):
        ops.cloud_nearest(torch.zeros(3, 3), torch.zeros(3, 3), radius=0.1)
    with pytest.raises(_lib.LsError, match="fp32"):
        ops.cloud_nearest(torch.zeros(3, 3, device=d, dtype=torch.float64), torch.zeros(3, 3, device=d), radius=0.1)
    with pytest.raises(ValueError):
        ops.cloud_nearest(torch.zeros(3, 2, device=d), torch.zeros(3, 3, device=d), radius=0.1)
    with pytest.raises(ValueError):
        ops.cloud_nearest(tA[0], tB[0], g=torch.eye(3, device=d), radius=0.1)
    with pytest.raises(ValueError):
        ops.cloud_nearest_batch(tA, tB[:-1], radius=0.1)
    with pytest.raises(ValueError):
        ops.cloud_nearest_batch(tA, tB, radius=[0.1, 0.2])
    with pytest.raises(ValueError):
        ops.cloud_nearest_batch([], [], radius=0.1)
    with pytest.raises(ValueError):
        ops.cloud_nearest_batch(tA, tB, g=torch.eye(4, device=d).repeat(2, 1, 1), radius=0.1)


def test_memory_sized_case():
    """20 000 memory rows, one per voxel at h = 0.01 (made by the merge), against 20 000 posed rows of the same surface, r = 2 h"""
    from livingscenes_amd import ops
    rng = np.random.default_rng(17)
    h = 0.01
    raw = (rng.uniform(-1, 1, (60000, 3)) * [1.0, 0.6, 0.02]).astype(np.float32)
    mem, _ = ops.cloud_merge(_t(raw[:40000]), _t(raw[:0]), voxel=h)
    A = mem[:20000].cpu().numpy()
    assert A.shape[0] == 20000
    g = _pose(rng, 1.0)
    gi = np.concatenate([g[:, :3].T, -g[:, :3].T @ g[:, 3:]], 1)
    B = (raw[40000:].astype(np.float64) @ gi[:, :3].T + gi[:, 3]).astype(np.float32)      # g takes B back onto the slab
    idx, d2, counts, s = _check(A, B, g, 2 * h, "memory sized")
    assert counts[0] == 20000 and 2000 < counts[1] < 20000 and 0 < counts[2] <= counts[1]
    print(f"matched {counts[1]} of 20000, {counts[2]} memory rows seen, rmse {math.sqrt(s / counts[1]):.5f}")


# ------------------------------------------------------------------------------------------------ the layers above


def _overlap_against(ov, k, twin, a):
    finite, matched, seen = (int(c) for c in twin[2])
    assert np.array_equal(ov["counts"][k], twin[2]) and np.array_equal(ov["nn_idx"][k].cpu().numpy(), twin[0])
    assert ov["overlap"][k] == (matched / finite if finite else 0.0) and ov["memory_seen"][k] == (seen / a if a else 0.0)
    if matched:
        want = math.sqrt(twin[3] / matched)
        assert abs(ov["rmse"][k] - want) <= matched * 2.0 ** -52 * want, (ov["rmse"][k], want)
    else:
        assert math.isnan(ov["rmse"][k])


def test_overlap_batch_known_pose():
    from livingscenes_amd.lib_math.torch_se3 import inverse
    d = _dev()
    h = 0.02
    solver = _solver(object(), {"accumulate": {"voxel_size": h}})
    rng = np.random.default_rng(19)
    mems, news, Ts = [], [], []
    for seed in (3, 4):                                                  # the halves of a shape, as the merge's _accumulate_batch test
        full = synth.canonical_shape(4096, seed).astype(np.float32)
        x = (full[:, 0] - 0.5 * (full[:, 0].max() + full[:, 0].min())) / (full[:, 0].max() - full[:, 0].min())
        one, two = full[x < 0.15], full[x > -0.15]
        g = _pose(rng, 1.5).astype(np.float64)                            # memory -> rescan
        moved = (two.astype(np.float64) @ g[:, :3].T + g[:, 3]).astype(np.float32)
        T = np.eye(4, dtype=np.float32)
        T[:3] = g
        mems.append(torch.from_numpy(one).to(d)), news.append(torch.from_numpy(moved).to(d)), Ts.append(T)
    T = torch.from_numpy(np.stack(Ts)).to(d)
    gi = inverse(T).cpu().numpy()                                        # what the operator receives, bit for bit
    for Tin in (T, T[:, :3].contiguous()):                               # [P,4,4] as Rt_to_SE3 gives it, or [P,3,4]
        ov = solver._overlap_batch(mems, news, Tin)                      # radius: 2 * cfg['accumulate']['voxel_size']
        assert set(ov) == {"overlap", "rmse", "memory_seen", "counts", "nn_idx"} and all(len(v) == 2 for v in ov.values())
        for k in range(2):
            twin = no.nearest(mems[k].cpu().numpy(), news[k].cpu().numpy(), gi[k], 2 * h)
            _overlap_against(ov, k, twin, mems[k].shape[0])
            assert 0.1 < ov["overlap"][k] < 0.9 and 0.1 < ov["memory_seen"][k] < 0.9 and 0 < ov["rmse"][k] <= 2 * h
            print(f"pair {k}: overlap {ov['overlap'][k]:.4f} rmse {ov['rmse'][k]:.5f} memory seen {ov['memory_seen'][k]:.4f}")
    wide = solver._overlap_batch(mems, news, T, radius=0.1)              # an explicit radius goes before the cfg's
    assert wide["overlap"][0] > ov["overlap"][0]
    _overlap_against(_solver(object(), {"accumulate": {"voxel_size": h, "overlap_radius": 0.1}})._overlap_batch(mems, news, T), 0,
                     no.nearest(mems[0].cpu().numpy(), news[0].cpu().numpy(), gi[0], 0.1), mems[0].shape[0])
    assert _solver(object())._overlap_batch(mems, news, T)["overlap"][0] < ov["overlap"][0]            # the default voxel, 0.01: r = 0.02
    # an exact copy under the identity; a translation of 10 r
    eye = torch.eye(4, device=d).repeat(2, 1, 1)
    for Tin in (None, eye):
        same = solver._overlap_batch(mems, [m.clone() for m in mems], Tin)
        assert same["overlap"] == [1.0, 1.0] and same["rmse"] == [0.0, 0.0] and same["memory_seen"] == [1.0, 1.0]
        assert all(np.array_equal(i.cpu().numpy(), np.arange(m.shape[0])) for i, m in zip(same["nn_idx"], mems))
    r = 2 * h
    span = max(float(m.max() - m.min()) for m in mems)
    assert span < 10                                                     # the clouds fit in a box the far shift below clears
    for shift in (10 * r, 10.0):
        far = eye.clone()
        far[:, 0, 3] = shift
        gone = solver._overlap_batch(mems, [m.clone() for m in mems], far)
        twin = no.nearest(mems[0].cpu().numpy(), mems[0].cpu().numpy(), inverse(far)[0].cpu().numpy(), r)
        _overlap_against(gone, 0, twin, mems[0].shape[0])
        if shift == 10.0:
            assert gone["overlap"] == [0.0, 0.0] and all(math.isnan(v) for v in gone["rmse"]) and gone["memory_seen"] == [0.0, 0.0]
            assert all((i == -1).all() for i in gone["nn_idx"])
    with pytest.raises(ValueError):
        solver._overlap_batch(mems, news[:1], T)
    with pytest.raises(ValueError):
        solver._overlap_batch(mems, news, T[:1])


def _counted(monkeypatch, solver, shift=(0.0, 0.0, 0.0)):
    """the registration replaced by the translation `shift` (zero: the identity), and the calls of the steps counted"""
    from livingscenes_amd.lib_more import more_solver
    calls = {"registration": 0, "overlap": 0, "accumulate": 0, "encode": 0}

    def registration(pcs1, pcs2, icp=True):
        calls["registration"] += 1
        d = pcs1[0].device
        t = torch.tensor(shift, dtype=torch.float32, device=d).view(1, 3, 1).repeat(len(pcs1), 1, 1)
        return torch.eye(3, device=d).repeat(len(pcs1), 1, 1), t
    monkeypatch.setattr(solver, "_solve_pairwise_registration_batch", registration)
    for name, key in (("_overlap_batch", "overlap"), ("_accumulate_batch", "accumulate")):
        def counted(*a, _real=getattr(solver, name), _key=key, **kw):
            calls[_key] += 1
            return _real(*a, **kw)
        monkeypatch.setattr(solver, name, counted)

    def encode(*a, _real=more_solver._encode_clouds, **kw):
        calls["encode"] += 1
        return _real(*a, **kw)
    monkeypatch.setattr(more_solver, "_encode_clouds", encode)
    return calls


def _same_memory(m1, m2):
    assert len(m1["clouds"]) == len(m2["clouds"])
    for c1, c2 in zip(m1["clouds"], m2["clouds"]):
        assert c1.shape == c2.shape and np.array_equal(_bits(c1), _bits(c2))
    for key in CODE_KEYS:
        assert torch.equal(m1["codes"][key], m2["codes"][key]), key


def test_solve_sequence_gate_off_and_exact_copy(small_prior, monkeypatch):
    from livingscenes_amd.lib_more import more_solver
    solver = _solver(small_prior)
    n, h = 4, 0.02
    ref = _scene(synth.make_scene_pair(n, 700, seed=72)["ref"])
    copy = {k: v.clone() for k, v in ref.items()}
    calls = _counted(monkeypatch, solver)
    steps0, memory0 = more_solver.solve_sequence(solver, ref, [copy, copy], voxel=h)        # 1. both switches None
    assert all(set(st) == STEP_KEYS for st in steps0) and calls["overlap"] == 0 and calls["registration"] == 2
    steps, memory = more_solver.solve_sequence(solver, ref, [copy, copy], voxel=h, overlap_radius=0.04, min_overlap=0.5)     # 2.
    assert calls["overlap"] == 2 and calls["registration"] == 4         # ONE overlap call per step
    matched = 0
    for st, st0 in zip(steps, steps0):
        assert set(st) == STEP_KEYS | GATE_KEYS and st["rejected"] == [] and st["n_new_points"] == st0["n_new_points"] == [0] * n
        m0 = st["matches"].tolist()
        assert m0 == st0["matches"].tolist()
        for i in range(n):
            if m0[i] < 0:
                assert st["overlap"][i] is None and st["overlap_rmse"][i] is None and st["memory_seen"][i] is None
            else:
                matched += 1
                # the memory is one point per voxel of the reference: every one of them is seen again at distance 0, and a point the merge
                # dropped shares a voxel with a kept one, at most sqrt(3) h = 0.0346 < r away
                assert st["overlap"][i] == 1.0 and st["memory_seen"][i] == 1.0 and 0.0 <= st["overlap_rmse"][i] < 0.04
    assert matched > 0
    _same_memory(memory, memory0)


def test_solve_sequence_gate_rejects_a_wrong_registration(small_prior, monkeypatch):
    from livingscenes_amd.lib_more import more_solver
    solver = _solver(small_prior)
    n, h = 4, 0.02
    ref = _scene(synth.make_scene_pair(n, 700, seed=72)["ref"])
    copy = {k: v.clone() for k, v in ref.items()}
    shift = (0.6, 0.8, 0.0)                                              # 3. every registration is wrong by 1 m; the instances are up to
    calls = _counted(monkeypatch, solver, shift=shift)                   # 1.4 m long, and along this direction none reaches itself
    steps, memory = more_solver.solve_sequence(solver, ref, [copy], voxel=h, overlap_radius=0.04, min_overlap=0.5)
    st = steps[0]
    m0 = st["matches"].tolist()
    slots = [i for i in range(n) if m0[i] >= 0]
    assert slots and st["rejected"] == slots and st["n_new_points"] == [0] * n
    # the premise, from the twin: moved by that metre, no point of a matched instance lies within 0.04 of its own memory
    for i in slots:
        mem_i = st["ref_pc_lst"][i].cpu().numpy()
        twin = no.nearest(mem_i, st["rescan_pc_lst"][m0[i]].cpu().numpy() - F(shift), None, 0.04)
        assert twin[2][1] == 0, (i, twin[2])
        assert st["overlap"][i] == 0.0 and math.isnan(st["overlap_rmse"][i]) and st["memory_seen"][i] == 0.0
        assert st["registration"][i].shape == (1, 4, 4) and st["registration"][i][0, :3, 3].tolist() == F(shift).tolist() and set(st["codes"][i]) == set(CODE_KEYS)
    assert calls == {"registration": 1, "overlap": 1, "accumulate": 1, "encode": 0}      # the one merge is that of the reference
    ref_codes = small_prior.encode_fps(ref["pc"], ref["pc_mask"])
    for i in range(n):                                                   # clouds and codes as before the step
        assert np.array_equal(_bits(memory["clouds"][i]), _bits(st["ref_pc_lst"][i])) and st["merged_sizes"][i] == st["ref_pc_lst"][i].shape[0]
    for key in CODE_KEYS:
        assert torch.equal(memory["codes"][key], ref_codes[key]), key
    # without a threshold the same step reports the same figures and merges: the misplaced copy goes into the memory
    steps2, memory2 = more_solver.solve_sequence(solver, ref, [copy], voxel=h, overlap_radius=0.04)
    assert steps2[0]["rejected"] == [] and steps2[0]["overlap"] == st["overlap"] and all(steps2[0]["n_new_points"][i] > 0 for i in slots)


def test_solve_sequence_gate_reports_without_changing_the_memory(small_prior, monkeypatch):
    from livingscenes_amd.lib_more import more_solver
    solver = _solver(small_prior)
    n, h = 4, 0.02
    s1, s2 = synth.make_scene_pair(n, 700, seed=71, noise=0.002), synth.make_scene_pair(n, 500, seed=71, noise=0.004)
    ref, rescans = _scene(s1["ref"]), [_scene(s1["rescan"]), _scene(s2["rescan"])]
    steps0, memory0 = more_solver.solve_sequence(solver, ref, rescans, voxel=h)
    steps, memory = more_solver.solve_sequence(solver, ref, rescans, voxel=h, min_overlap=0.0)        # 4. the radius: 2 * voxel
    _same_memory(memory, memory0)
    matched = 0
    for st, st0 in zip(steps, steps0):
        assert set(st) == STEP_KEYS | GATE_KEYS and set(st0) == STEP_KEYS and st["rejected"] == []
        assert st["n_new_points"] == st0["n_new_points"] and st["merged_sizes"] == st0["merged_sizes"]
        m0 = st["matches"].tolist()
        slots = [i for i in range(n) if m0[i] >= 0]
        matched += len(slots)
        if not slots:
            continue
        ov = solver._overlap_batch([st["ref_pc_lst"][i] for i in slots], [st["rescan_pc_lst"][m0[i]] for i in slots],
                                   torch.cat([st["registration"][i] for i in slots]), radius=2 * h)
        for k, i in enumerate(slots):
            assert st["overlap"][i] == ov["overlap"][k] and st["memory_seen"][i] == ov["memory_seen"][k]
            assert st["overlap_rmse"][i] == ov["rmse"][k] or (math.isnan(st["overlap_rmse"][i]) and math.isnan(ov["rmse"][k]))
        assert all(st["overlap"][i] is None for i in range(n) if i not in slots)
    assert matched > 0, "the synthetic scene matched nothing: the test would show nothing"
