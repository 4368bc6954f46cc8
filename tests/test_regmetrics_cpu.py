"""Host side of the batched registration metrics, without a GPU: the C ABI of ls_reg_metrics_batch (symbols, workspace query, every refusal,
all of which come before the first HIP call) and the batched modes of the two relocalisation legs of the harness with a stand-in solver and
a float64 torch restatement of the four metrics in place of the device operator."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from livingscenes_amd import _lib

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ("ls_reg_metrics_batch", "ls_reg_metrics_batch_workspace_bytes")


def test_abi_exports_the_registration_metrics():
    lib = _lib.load()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    header = open(os.path.join(os.path.dirname(GOLDEN_DIR), "..", "include", "livingscenes_hip.h")).read()
    assert "int ls_reg_metrics_batch(" in header and "size_t ls_reg_metrics_batch_workspace_bytes(" in header
    assert lib.ls_version() == 107 and "#define LS_ABI_VERSION 107" in header


def test_workspace_query():
    q = _lib.load().ls_reg_metrics_batch_workspace_bytes
    for P, nt, mt, s in ((0, 4, 4, 10), (-1, 4, 4, 10), (2, -1, 4, 10), (2, 4, -1, 10), (2, 4, 4, 0), (2, 4, 4, -3)):
        assert q(P, nt, mt, s) == 0, (P, nt, mt, s)
    assert 0 < q(1, 4, 4, 10) < q(64, 4, 4, 10)                       # grows with P
    assert q(2, 4, 4, 1) < q(2, 4_000_000, 4, 1) < q(2, 4_000_000, 4_000_000, 1)   # and with either total


def _hp(a):
    return ctypes.c_void_p(a.ctypes.data)


def _call(xo, yo, nt=None, mt=None, stride=10, ws_bytes=None, null=None):
    """the entry with host scratch in place of device memory: every case here is refused before anything touches it"""
    lib = _lib.load()
    xo, yo = np.asarray(xo, np.int64), np.asarray(yo, np.int64)
    P = len(xo) - 1
    nt = int(xo[-1]) if nt is None else nt
    mt = int(yo[-1]) if mt is None else mt
    buf = np.zeros(1 << 16, np.uint8)
    need = lib.ls_reg_metrics_batch_workspace_bytes(P, max(nt, 0), max(mt, 0), max(stride, 1))
    a = {k: _hp(buf) for k in ("X", "Y", "pred", "gt", "out", "ws")}
    a["x_off"], a["y_off"] = _hp(xo), _hp(yo)
    if null:
        a[null] = None
    rc = lib.ls_reg_metrics_batch(P, a["X"], nt, a["x_off"], a["Y"], mt, a["y_off"], a["pred"], a["gt"], stride, a["out"], a["ws"],
                                  need if ws_bytes is None else ws_bytes, None)
    return rc, lib.ls_last_error().decode()


def test_refusals_name_the_problem_and_need_no_device():
    rc, msg = _call([0, 3, 2, 5], [0, 2, 4, 6])
    assert rc == -1 and "problem 1: x_off decreases" in msg, msg
    rc, msg = _call([0, 3, 4, 5], [0, 2, 4, 3])
    assert rc == -1 and "problem 2: y_off decreases" in msg, msg
    rc, msg = _call([0, 3, 4, 5], [0, 2, 4, 6], mt=7)
    assert rc == -1 and "problem 2: y_off ends at 6" in msg and "disagrees with the total 7" in msg, msg
    rc, msg = _call([0, 3, 4, 5], [0, 2, 4, 6], nt=4)
    assert rc == -1 and "x_off ends at 5" in msg, msg
    rc, msg = _call([1, 3, 4, 5], [0, 2, 4, 6])
    assert rc == -1 and "x_off[0]" in msg, msg
    rc, msg = _call([0, 3, 4, 5], [2, 2, 4, 6])
    assert rc == -1 and "y_off[0]" in msg, msg
    rc, msg = _call([0, 3, 3, 5], [0, 2, 4, 6])
    assert rc == -1 and "problem 1: empty cloud" in msg, msg
    rc, msg = _call([0, 3, 4, 5], [0, 2, 2, 6])
    assert rc == -1 and "problem 1: empty cloud" in msg, msg
    rc, msg = _call([0, 3, 4, 5], [0, 2, 4, 6], stride=0)
    assert rc == -1 and "chamfer_stride" in msg, msg
    rc, msg = _call([0], [0])                                          # P = 0
    assert rc == -1 and "P" in msg, msg
    for k in ("X", "Y", "pred", "gt", "out", "x_off", "y_off"):
        rc, msg = _call([0, 3, 4, 5], [0, 2, 4, 6], null=k)
        assert rc == -1 and "null" in msg, (k, msg)
    rc, msg = _call([0, 3, 4, 5], [0, 2, 4, 6], ws_bytes=8)
    assert rc == -3 and "workspace" in msg, msg
    rc, msg = _call([0, 3, 4, 5], [0, 2, 4, 6], null="ws")
    assert rc == -3 and "workspace" in msg, msg
    rc, msg = _call([0, 2 ** 31], [0, 5])                              # more than 2^31 - 1 rows in one cloud
    assert rc == -1 and "problem 0" in msg and "at most 2147483647" in msg, msg


# ------------------------------------------------------------------------------------------------ the four definitions, float64 torch
def _inv(g):
    Rt = g[:3, :3].T
    return torch.cat([Rt, -(Rt @ g[:3, 3:4])], 1)


def _app(g, x):
    return x @ g[:3, :3].T + g[:3, 3]


def _sq(a, b):
    return ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)


def restated_metrics(pcs1, pcs2, pred, gt, chamfer_stride=10, sizes=None):
    """evaluate.registration_metrics_batch restated: pose_estimation.py:157-233 and evaluate.py:111-123 in float64, pair by pair"""
    if torch.is_tensor(pcs1):
        pcs1, pcs2 = torch.split(pcs1, [n for n, _ in sizes]), torch.split(pcs2, [m for _, m in sizes])
    rows = []
    for x, y, p, g in zip(pcs1, pcs2, pred, gt):
        x, y, p, g = x.double(), y.double(), p[:3].double(), g[:3].double()
        tr = (p[:, :3] * g[:, :3]).sum()
        rre = torch.rad2deg(torch.acos(((tr - 1) / 2).clamp(-1, 1)))
        rte = (p[:, 3] - g[:, 3]).norm()
        e12, e21 = _app(p, x) - _app(g, x), _app(_inv(p), y) - _app(_inv(g), y)
        rmse = (((e12 ** 2).sum() + (e21 ** 2).sum()) / (3 * (x.shape[0] + y.shape[0]))).sqrt()
        xs, ys = x[::chamfer_stride], y[::chamfer_stride]
        gi = _inv(g)
        pg = torch.cat([p[:, :3] @ gi[:, :3], p[:, :3] @ gi[:, 3:4] + p[:, 3:4]], 1)
        cd = _sq(_app(p, xs), ys).min(1)[0].mean() + _sq(ys, _app(pg, ys)).min(1)[0].mean()
        rows.append(torch.stack([rre, rte, rmse, cd]))
    out = torch.stack(rows)
    return {k: out[:, i] for i, k in enumerate(("rre", "rte", "rmse", "chamfer"))}


def _dense_chamfer(src, ref, pred_tsfm, gt_tsfm):
    """evaluate.py:111-123 as written there (the package's version finds the neighbours on the device)"""
    from livingscenes_amd.lib_math import torch_se3
    a = torch_se3.transform(pred_tsfm, src)
    b = torch_se3.transform(torch_se3.concatenate(pred_tsfm, torch_se3.inverse(gt_tsfm)), ref)
    sq = lambda u, v: ((u[:, :, None, :] - v[:, None, :, :]) ** 2).sum(-1)
    return sq(a, ref).min(-1)[0].mean(1) + sq(ref, b).min(-1)[0].mean(1)


def _rot(axis, deg):
    a = torch.tensor(axis, dtype=torch.float64)
    a = a / a.norm()
    K = torch.tensor([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=torch.float64)
    t = math.radians(deg)
    return (torch.eye(3, dtype=torch.float64) + math.sin(t) * K + (1 - math.cos(t)) * (K @ K)).float()


class _Model:
    def parameters(self):
        return iter([torch.zeros(1)])


class _Solver:
    """counts its calls; `pose_of(a, b)` -> (R [3,3], t [3,1]) is deterministic per pair, so the single and the batched entry points agree"""

    def __init__(self, pose_of):
        self.model = _Model()
        self.pose_of = pose_of
        self.single_calls = self.batch_calls = self.optim_batch_calls = 0
        self.batch_sizes = []

    def _poses(self, pcs1, pcs2):
        self.batch_sizes.append(len(pcs1))
        Rt = [self.pose_of(a, b) for a, b in zip(pcs1, pcs2)]
        return torch.stack([R for R, _ in Rt]), torch.stack([t for _, t in Rt])

    def _solve_pairwise_registration(self, pc1, pc2, optim=False):
        self.single_calls += 1
        R, t = self.pose_of(pc1[0], pc2[0])
        return R[None], t[None]

    def _solve_pairwise_registration_batch(self, pcs1, pcs2, icp=True):
        self.batch_calls += 1
        return self._poses(pcs1, pcs2)

    def _solve_pairwise_registration_optim_batch(self, pcs1, pcs2):
        self.optim_batch_calls += 1
        return self._poses(pcs1, pcs2)


def _tree_pose(a, b):
    """a pose that depends on the pair alone: centroids aligned up to 4 cm under a rotation of 11 .. 27 degrees (what that gives against the
    tree's ground truth is asserted in test_stand_in_poses_are_well_conditioned_on_the_tree)"""
    R = _rot((0.3, -0.5, 1.0), 11.0 + 4.0 * (a.shape[0] % 5))
    return R, (b.mean(0) - R @ a.mean(0) + torch.tensor([0.03, -0.02, 0.015]))[:, None]


def _patch(monkeypatch):
    from livingscenes_amd import evaluate
    calls = []

    def metrics(*a, **k):
        calls.append(len(a[0]))
        return restated_metrics(*a, **k)
    monkeypatch.setattr(evaluate, "registration_metrics_batch", metrics)
    monkeypatch.setattr(evaluate, "chamfer_distance_torch", _dense_chamfer)
    return calls


def _assert_summaries_agree(want, got, exact, skip=()):
    assert sorted(want) == sorted(got)
    for k in want:
        if k in skip:
            continue
        if k in exact:
            assert want[k] == got[k], (k, want[k], got[k])
        else:
            w, g = np.asarray(want[k], np.float64), np.asarray(got[k], np.float64)
            assert w.shape == g.shape and np.array_equal(np.isnan(w), np.isnan(g)), (k, w, g)
            assert np.all(np.abs(w - g)[~np.isnan(w)] <= 1e-4 * np.abs(w)[~np.isnan(w)]), (k, w, g)


@pytest.mark.parametrize("optim", (False, True))
def test_eval_3rscan_relocalization_batched_equals_default(monkeypatch, optim):
    from livingscenes_amd import harness, rscan
    tree = os.path.join(GOLDEN_DIR, "rscan_tree")
    ds = rscan.Dataset_3RScan({"root_path": os.path.join(tree, "data"), "split": "val", "category_list": os.path.join(tree, "categories.txt"),
                               "n_point_per_instance": 1024, "use_gt_mask": True}, device="cpu")
    calls = _patch(monkeypatch)
    seen = []

    def pose_of(a, b):
        R, t = _tree_pose(a, b)
        seen.append((a, b, torch.cat([R, t], 1)))
        return R, t
    solver = _Solver(pose_of)
    want = harness.eval_3rscan_relocalization(ds, solver, optim=optim)
    n = want["n_pairs"]
    assert n >= 2 and solver.single_calls == n and solver.batch_calls == solver.optim_batch_calls == 0 and calls == []
    for chunk, n_calls in ((128, 1), (2, -(-n // 2)), (1, n)):                # one batched solver call per chunk
        solver.__init__(pose_of)
        del calls[:]
        got = harness.eval_3rscan_relocalization(ds, solver, optim=optim, batched=True, **({} if chunk == 128 else {"chunk": chunk}))
        assert solver.single_calls == 0 and calls == [n]                   # ONE metrics call for all the pairs
        assert (solver.optim_batch_calls, solver.batch_calls) == ((n_calls, 0) if optim else (0, n_calls))
        assert sum(solver.batch_sizes) == n and max(solver.batch_sizes) <= chunk
        _assert_summaries_agree(want, got, exact=("n_pairs", "shape", "recall[T<0.1m]", "recall[RRE<10deg]"))
    # the same pairs in the same order, every time
    assert len(seen) == 4 * n
    for k in range(n):
        for rep in (1, 2, 3):
            assert all(torch.equal(u, v) for u, v in zip(seen[k], seen[rep * n + k]))


def test_stand_in_poses_are_well_conditioned_on_the_tree():
    """the premise of the 1e-4 comparison above: unfolded rre in [5, 175] degrees and rte >= 1 cm for every pair of the tree"""
    from livingscenes_amd import evaluate, harness, rscan
    tree = os.path.join(GOLDEN_DIR, "rscan_tree")
    ds = rscan.Dataset_3RScan({"root_path": os.path.join(tree, "data"), "split": "val", "category_list": os.path.join(tree, "categories.txt"),
                               "n_point_per_instance": 1024, "use_gt_mask": True}, device="cpu")
    kept = {}

    def metrics(*a, **k):
        kept.update(restated_metrics(*a, **k))
        return kept
    mp = pytest.MonkeyPatch()
    try:
        mp.setattr(evaluate, "registration_metrics_batch", metrics)
        harness.eval_3rscan_relocalization(ds, _Solver(_tree_pose), optim=False, batched=True)
    finally:
        mp.undo()
    assert bool((kept["rre"] >= 5).all()) and bool((kept["rre"] <= 175).all()) and bool((kept["rte"] >= 0.01).all()), kept


def test_eval_relocalization_batched_equals_default(monkeypatch):
    from livingscenes_amd import harness, synth
    from livingscenes_amd.lib_math.torch_se3 import concatenate, inverse
    scenes = [synth.make_scene_pair(n, 96, seed=40 + n, noise=0.002) for n in (1, 3, 2)]
    # the stand-in knows each pair's ground truth (keyed by the first coordinate of the reference cloud) and moves it by a fixed rotation of
    # 6 .. 172 degrees and 2 cm: 5 degrees and 1 cm or more away before the fold, on both sides of the 5 / 10 degree recalls after it
    table, k = {}, 0
    for sc in scenes:
        gt = concatenate(sc["rescan_T"][:, :3], inverse(sc["ref_T"][:, :3]))
        for i in range(sc["ref"].shape[0]):
            d = torch.cat([_rot((1.0, 0.4 * k, -0.7), (6.0, 13.0, 93.0, 8.0, 172.0, 45.0)[k]), torch.tensor([[0.02], [-0.01], [0.005]])], 1)
            table[float(sc["ref"][i, 0, 0])] = concatenate(d[None], gt[i][None])[0]
            k += 1
    assert len(table) == 6

    def pose_of(a, b):
        g = table[float(a[0, 0])]
        return g[:, :3].contiguous(), g[:, 3:4].contiguous()
    calls = _patch(monkeypatch)
    solver = _Solver(pose_of)
    want = harness.eval_relocalization(scenes, solver)
    assert solver.batch_calls == len(scenes) and calls == []
    assert 0 < want["recall_rre5"] < want["recall_rre10"] < 100 and want["rte"].min() >= 0.01
    for chunk, n_calls in ((128, 1), (4, 2)):
        solver.__init__(pose_of)
        del calls[:]
        got = harness.eval_relocalization(scenes, solver, batched=True, **({} if chunk == 128 else {"chunk": chunk}))
        assert solver.batch_calls == n_calls and solver.single_calls == 0 and calls == [6]
        _assert_summaries_agree(want, got, exact=("recall_rre5", "recall_rre10"))
        assert np.array_equal(want["poses"], got["poses"])
