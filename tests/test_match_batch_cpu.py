"""Host side of the ragged matcher batches, without a GPU: the C ABI of ls_*_batch_f32 (symbols, workspace queries, the offset checks, which
run before the first HIP call) and the batched modes of the harness / the end-to-end driver with a stand-in solver on the CPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

from livingscenes_amd import _lib

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OPS = ("cosine_scores", "greedy_match", "nn_match", "sinkhorn_match", "kabsch_residual_matrix")


def test_abi_exports_the_batch_matchers():
    lib = _lib.load()
    for op in OPS:
        for name in (f"ls_{op}_batch_f32", f"ls_{op}_batch_workspace_bytes"):
            assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    header = open(os.path.join(os.path.dirname(GOLDEN_DIR), "..", "include", "livingscenes_hip.h")).read()
    for op in OPS:
        assert f"int ls_{op}_batch_f32(" in header and f"size_t ls_{op}_batch_workspace_bytes(" in header


def test_workspace_queries():
    lib = _lib.load()
    for op in OPS:
        q = getattr(lib, f"ls_{op}_batch_workspace_bytes")
        for P, nt, mt in ((0, 4, 4), (-1, 4, 4), (2, -1, 4), (2, 4, -1)):
            assert q(P, nt, mt) == 0, (op, P, nt, mt)
        assert 0 < q(1, 4, 4) < q(64, 4, 4)
        assert q(3, 0, 0) > 0            # three empty problems still carry their offsets
    # only the scores keep per-row scratch (the inverse norms)
    assert lib.ls_cosine_scores_batch_workspace_bytes(2, 1000, 1000) >= lib.ls_cosine_scores_batch_workspace_bytes(2, 0, 0) + 2000 * 4
    assert lib.ls_greedy_match_batch_workspace_bytes(2, 1000, 1000) == lib.ls_greedy_match_batch_workspace_bytes(2, 0, 0)


def _hp(a):
    return ctypes.c_void_p(a.ctypes.data)


def _call(op, so, to, nt=None, mt=None, ws_bytes=None):
    """the batch entry of `op` with host scratch in place of device memory: every case here is refused before anything touches it"""
    lib = _lib.load()
    so, to = np.asarray(so, np.int64), np.asarray(to, np.int64)
    P = len(so) - 1
    nt = int(so[-1]) if nt is None else nt
    mt = int(to[-1]) if mt is None else mt
    buf = np.zeros(1 << 16, np.uint8)
    need = getattr(lib, f"ls_{op}_batch_workspace_bytes")(P, max(nt, 0), max(mt, 0))
    ws = _hp(buf), (need if ws_bytes is None else ws_bytes)
    fn = getattr(lib, f"ls_{op}_batch_f32")
    if op == "cosine_scores":
        rc = fn(P, _hp(buf), nt, _hp(so), _hp(buf), mt, _hp(to), 16, _hp(buf), *ws, None)
    elif op == "kabsch_residual_matrix":
        rc = fn(P, _hp(buf), nt, _hp(so), _hp(buf), mt, _hp(to), 8, _hp(buf), *ws, None)
    elif op == "sinkhorn_match":
        rc = fn(P, _hp(buf), nt, _hp(so), mt, _hp(to), 16.0, 1.0, 100, 0.0, _hp(buf), _hp(buf), *ws, None)
    else:
        rc = fn(P, _hp(buf), nt, _hp(so), mt, _hp(to), _hp(buf), _hp(buf), *ws, None)
    return rc, lib.ls_last_error().decode()


@pytest.mark.parametrize("op", OPS)
def test_offset_checks_name_the_problem_and_need_no_device(op):
    rc, msg = _call(op, [0, 3, 2, 5], [0, 2, 4, 6])
    assert rc == -1 and "problem 1: src_off decreases" in msg, msg
    rc, msg = _call(op, [0, 3, 4, 5], [0, 2, 4, 3])
    assert rc == -1 and "problem 2: tgt_off decreases" in msg, msg
    rc, msg = _call(op, [0, 3, 4, 5], [0, 2, 4, 6], mt=7)
    assert rc == -1 and "problem 2: tgt_off ends at 6" in msg and "disagrees with the total 7" in msg, msg
    rc, msg = _call(op, [0, 3, 4, 5], [0, 2, 4, 6], nt=4)
    assert rc == -1 and "src_off ends at 5" in msg, msg
    rc, msg = _call(op, [1, 3, 4, 5], [0, 2, 4, 6])
    assert rc == -1 and "src_off[0]" in msg, msg
    rc, msg = _call(op, [0], [0])                       # P = 0
    assert rc == -1, msg
    rc, msg = _call(op, [0, 3, 4, 5], [0, 2, 4, 6], ws_bytes=8)
    assert rc == -3 and "workspace" in msg, msg
    lib = _lib.load()
    so, to = np.asarray([0, 2], np.int64), np.asarray([0, 2], np.int64)
    fn = getattr(lib, f"ls_{op}_batch_f32")
    args = {"cosine_scores": (1, None, 2, _hp(so), None, 2, _hp(to), 16, None),
            "kabsch_residual_matrix": (1, None, 2, _hp(so), None, 2, _hp(to), 8, None),
            "sinkhorn_match": (1, None, 2, _hp(so), 2, _hp(to), 16.0, 1.0, 100, 0.0, None, None)}.get(op, (1, None, 2, _hp(so), 2, _hp(to), None, None))
    assert fn(*args, None, 0, None) == -3               # a missing workspace


def test_sinkhorn_batch_refuses_an_oversized_problem_by_name():
    rc, msg = _call("sinkhorn_match", [0, 3, 303, 305], [0, 2, 302, 306])
    assert rc == -1 and "problem 1" in msg and "300 x 300" in msg and "LDS" in msg, msg


# ------------------------------------------------------------------------------------------------ harness and driver with a stand-in solver
C = 8


class _Model:
    class encoder:
        c_dim = C

    def encode_fps(self, pc, mask):
        m = mask.float()
        mean = torch.stack([pc[i][:, mask[i, 0]].mean(-1) for i in range(pc.shape[0])])
        f = torch.stack([(k + 1.0) * mean for k in range(C)], 1)
        return {"z_so3": f, "z_inv": f.norm(dim=-1) + m.sum(-1), "s": m.sum(-1)[:, 0] * 1e-3, "t": mean[:, None, :]}


class _Solver:
    """deterministic CPU stand-in: greedy matching on the point counts; the batched form loops the single one"""
    mesh_extractor = None

    def __init__(self):
        self.model = _Model()
        self.single_calls = self.batch_calls = 0

    def _solve_object_matching(self, cr, cs, method):
        self.single_calls += 1
        n = cr["s"].shape[0]
        d = (cr["s"][:, None] - cs["s"][None, :]).abs() * (2.0 if method == "nn" else 1.0)
        m0 = torch.full((n,), -1, dtype=torch.long)
        used = set()
        for i in (range(n) if method != "nn" else reversed(range(n))):
            for j in d[i].argsort().tolist():
                if j not in used and (method != "nn" or float(d[i, j]) < 0.05):
                    m0[i] = j
                    used.add(j)
                    break
        return {"matches0": m0}

    def _solve_object_matching_batch(self, crs, css, method):
        self.batch_calls += 1
        before = self.single_calls
        out = [self._solve_object_matching(a, b, method) for a, b in zip(crs, css)]
        self.single_calls = before
        return out

    def _solve_pairwise_registration_batch(self, a, b):
        R = torch.stack([torch.eye(3) * (1 + x.shape[0] * 1e-4) for x in a])
        t = torch.stack([(y.mean(0) - x.mean(0))[:, None] for x, y in zip(a, b)])
        return R, t

    def _transform_latent(self, code, tsfm):
        return {k: v.clone() + float(tsfm.sum()) for k, v in code.items()}


def _scene(gen, sizes):
    mx = max(sizes)
    pc, mask = torch.zeros(len(sizes), 3, mx), torch.zeros(len(sizes), 1, mx, dtype=torch.bool)
    for i, n in enumerate(sizes):
        pc[i, :, :n] = torch.randn(3, n, generator=gen)
        mask[i, :, :n] = True
    return {"pc": pc, "pc_mask": mask}


def test_solve_end2end_batch_match_batched_equals_default():
    from livingscenes_amd.lib_more import more_solver
    gen = torch.Generator().manual_seed(5)
    pairs = [(_scene(gen, [30, 41, 52]), _scene(gen, [41, 30, 52, 17])), (_scene(gen, [25]), _scene(gen, [25, 26])),
             (_scene(gen, [60, 61, 33, 35]), _scene(gen, [61, 60]))]
    solver = _Solver()
    want = more_solver.solve_end2end_batch(solver, pairs)
    assert solver.single_calls == len(pairs) and solver.batch_calls == 0
    got = more_solver.solve_end2end_batch(solver, pairs, match_batched=True)
    assert solver.single_calls == len(pairs) and solver.batch_calls == 1      # ONE matcher call for all scene pairs
    assert any(int((w["matches"] < 0).sum()) for w in want) and any(int((w["matches"] >= 0).sum()) for w in want)
    for w, o in zip(want, got):
        assert torch.equal(w["matches"], o["matches"])
        assert sorted(w) == sorted(o)
        for a, b in zip(w["registration"], o["registration"]):
            assert (a is None) == (b is None) and (a is None or torch.equal(a, b))
        for a, b in zip(w["codes"], o["codes"]):
            assert (a is None) == (b is None) and (a is None or all(torch.equal(a[k], b[k]) for k in a))


def test_eval_3rscan_matching_batched_equals_default():
    from livingscenes_amd import harness, rscan
    tree = os.path.join(GOLDEN_DIR, "rscan_tree")
    ds = rscan.Dataset_3RScan({"root_path": os.path.join(tree, "data"), "split": "val", "category_list": os.path.join(tree, "categories.txt"),
                               "n_point_per_instance": 1024, "use_gt_mask": True}, device="cpu")
    solver = _Solver()
    methods = ("sequential", "nn")
    want = harness.eval_3rscan_matching(ds, solver, methods)
    n_pairs = solver.single_calls // len(methods)
    assert n_pairs >= 2 and solver.batch_calls == 0
    got = harness.eval_3rscan_matching(ds, solver, methods, batched=True)
    assert solver.batch_calls == len(methods) and solver.single_calls == n_pairs * len(methods)      # one batched call per method
    assert sorted(want) == sorted(got)
    for k in want:
        assert want[k] == got[k] or (np.isnan(want[k]) and np.isnan(got[k])), (k, want[k], got[k])
