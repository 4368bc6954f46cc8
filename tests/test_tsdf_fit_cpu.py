"""CPU-only tests (-m "not gpu") of the fit of the latent codes to a fused state (include/livingscenes_hip.h: ls_tsdf_draw_f32,
ls_tsdf_fit_loss_f64): csrc/tsdffit_plan.h -- compiled on its own with the host compiler and run by tests/tools/tsdffit_plan_run.cpp,
plain and under AddressSanitizer / UBSan -- against tests/tsdf_fit_oracle.py by equality; the properties of the twin's draw; the twin's
loss against math.fsum and its gradient against a central difference; what the C entry points decide on the host before any HIP call; the
bindings; solve_sequence's two new refusals; and the loop of the fit on the twin with the oracle decoder.  The states, the loss cases and
the oracle loop of tests/test_hip_tsdf_fit.py live here.

States: the twelve of tests/test_tsdf_sample_cpu.py (sphere, box, holes on four dims) at min_obs 1 and 2 -- every one holds BAND and FREE
samples except (2,2,2) "sphere" at min_obs 2, which has 2 band samples and no free one: the empty-list case -- plus HAND, a hand-built
state with samples at sum == -n * 16384 (D = -1 exactly: BAND, target == -trunc), at sum == +n * 16384 (FREE) and never observed."""
import ctypes
import functools
import inspect
import math
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, ".."))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import tsdf_fit_oracle as tfo          # noqa: E402
from test_tsdf_sample_cpu import DIMS, KINDS, BOX_HALF, grid_of, state_of   # noqa: E402

NAMES = ("ls_tsdf_draw_workspace_bytes", "ls_tsdf_draw_f32", "ls_tsdf_draw_batch_workspace_bytes", "ls_tsdf_draw_batch_f32",
         "ls_tsdf_fit_loss_f64")
F = np.float32
NAN, INF = float("nan"), float("inf")
QUOTAS = ((1, 1), (255, 257), (256, 256), (0, 7), (7, 0), (10000, 10000))
LOSS_N = (1, 255, 256, 257, 513)
LOSS_S = (0.37, 1.0, 2.95)


@functools.lru_cache(maxsize=None)
def hand_state():
    """-> ((sum, n), origin, voxel, trunc): dims (3,4,5) on a grid that is not dyadic; a quarter of the observed samples at D = -1 exactly"""
    dims = (3, 4, 5)
    rng = np.random.default_rng(5)
    N = rng.choice([0, 1, 2, 3], size=dims, p=[.15, .25, .3, .3])
    S = rng.integers(-16384, 16385, size=dims) * N
    what = rng.integers(0, 4, size=dims)
    S = np.where(what == 0, -16384 * N, np.where(what == 1, 16384 * N, S))
    N[0, 0, 0], S[0, 0, 0] = 2, -2 * 16384                                 # at least one of each, whatever the rng gave
    N[1, 1, 1], S[1, 1, 1] = 3, 3 * 16384
    N[2, 3, 4], S[2, 3, 4] = 0, 0
    state = (S.astype(np.int32), N.astype(np.int32))
    for t in state:
        t.setflags(write=False)
    return state, np.array([0.21, -0.4, 0.903]), 0.0173, 2.5 * 0.0173


def edge_state(dims, seed):
    """a random hand-built state with holes-like probabilities -> ((sum, n), origin, voxel, trunc)"""
    rng = np.random.default_rng(seed)
    N = rng.choice([0, 1, 2, 3], size=dims, p=[.04, .06, .45, .45])
    S = rng.integers(-16384, 16385, size=dims) * N
    S = np.where(rng.uniform(size=dims) < 0.4, 16384 * N, S)
    return (S.astype(np.int32), N.astype(np.int32)), np.array([-0.31, 0.17, 1.003]), 0.0137, 3 * 0.0137


def all_states():
    """(name, ((sum, n), origin, voxel, trunc)) of the twelve states and HAND"""
    return [((kind, dims), state_of(kind, dims)) for kind in KINDS for dims in DIMS] + [(("hand", (3, 4, 5)), hand_state())]


@functools.lru_cache(maxsize=None)
def expected_draw(name, min_obs, quota, seed):
    """the twin's draw, computed once and shared"""
    state, origin, h, trunc = dict(all_states())[name]
    return tfo.draw(state, origin, h, trunc, quota[0], quota[1], seed, min_obs)


@functools.lru_cache(maxsize=None)
def loss_case(N, which=0):
    """P = 3 problems of N columns: s a rotation of LOSS_S, sdf on both sides of every BAND target / s and of trunc / s, at them (the fp32
    nearest; with s = 1 and trunc = 0.25 exactly), PAD columns in the middle of every chunk, problem 1 all PAD (m_p = 0), min_loss below
    the new loss for problem 0 and above it for the others -> dict of arrays"""
    rng = np.random.default_rng(100 * N + which)
    P = 3
    s = np.array([LOSS_S[(p + which + N) % 3] for p in range(P)], F)
    trunc = np.array([0.25 if sv == 1.0 else tv for sv, tv in zip(s, (0.05, 0.0411, 0.25))], np.float64)
    kind = rng.choice([tfo.PAD, tfo.BAND, tfo.FREE], size=(P, N), p=[.2, .45, .35]).astype(np.uint8)
    kind[1] = tfo.PAD
    kind[0, 0] = tfo.BAND                                                  # problem 0 has a column with an error: its loss is above 1e-30
    if N > 2:
        kind[0, N // 2] = tfo.PAD
    target = np.where(kind == tfo.BAND, rng.uniform(-1, 1, (P, N)) * trunc[:, None], 0.0)
    target[kind == tfo.FREE] = (np.ones((P, N)) * trunc[:, None])[kind == tfo.FREE]
    centre = np.where(kind == tfo.BAND, target, trunc[:, None]) / s.astype(np.float64)[:, None]
    delta = rng.choice([0.0, 1e-7, -1e-7, 0.03, -0.03, 0.4, -0.4], size=(P, N))
    delta[0, 0] = 0.4
    sdf = (centre + delta).astype(F)
    sdf[kind == tfo.PAD] = rng.uniform(-1, 1, (P, N)).astype(F)[kind == tfo.PAD]   # a PAD column's value must not matter
    out = {"sdf": sdf, "s": s, "trunc": trunc, "target": target, "kind": kind, "min_loss": np.array([1e-30, 100.0, 100.0]),
           "improved": np.zeros(P, np.int32)}
    for v in out.values():
        v.setflags(write=False)
    return out


def test_every_state_holds_what_the_docstring_says():
    for name, (state, origin, h, trunc) in all_states():
        for min_obs in (1, 2):
            kd = tfo.kinds(state, min_obs)
            band, free = int((kd == tfo.BAND).sum()), int((kd == tfo.FREE).sum())
            if name == ("sphere", (2, 2, 2)) and min_obs == 2:
                assert (band, free) == (2, 0)
            else:
                assert band > 0 and free > 0, (name, min_obs, band, free)
    (S, N), _, _, trunc = hand_state()
    exact = (N >= 1) & (S.astype(np.int64) == -16384 * N.astype(np.int64))
    assert exact.sum() >= 1 and (N == 0).any()
    d = tfo.draw((S, N), *hand_state()[1:], 10000, 10000, 3)
    at = np.flatnonzero(exact.reshape(-1))
    cols = np.flatnonzero(np.isin(d["index"], at))
    assert len(cols) == len(at) and (d["kind"][cols] == tfo.BAND).all() and (d["target"][cols] == -trunc).all()


# ------------------------------------------------------------------------------------------------ tsdffit_plan.h on the host
def _compile(out, flags):
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *flags, "-I",
                    os.path.join(REPO, "livingscenes_amd", "csrc"), os.path.join(HERE, "tools", "tsdffit_plan_run.cpp"), "-o", out], check=True)
    return out


@pytest.fixture(scope="module")
def runners(tmp_path_factory):
    d = tmp_path_factory.mktemp("tsdffit_plan")
    return {"plain": _compile(str(d / "run"), ["-O1"]),
            "sanitized": _compile(str(d / "run_san"), ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])}


def _hex(values):
    return " ".join(float(v).hex() for v in np.asarray(values).reshape(-1))


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def run_draw(exe, state, origin, voxel, trunc, n_band, n_free, seed, min_obs):
    S, N = state
    text = "draw " + " ".join(map(str, [*S.shape, min_obs, n_band, n_free, seed])) + "\n" + _hex([*origin, voxel, trunc]) + "\n"
    text += " ".join(map(str, S.reshape(-1).tolist())) + "\n" + " ".join(map(str, N.reshape(-1).tolist())) + "\n"
    out = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    lines = out.stdout.splitlines()
    assert len(lines) == n_band + n_free + 1
    rows = [line.split() for line in lines[:-1]]
    return {"kind": np.array([int(r[0]) for r in rows], np.uint8), "index": np.array([int(r[1]) for r in rows], np.int32),
            "target": np.array([float.fromhex(r[2]) for r in rows], np.float64),
            "points": np.array([[float.fromhex(t) for t in r[3:]] for r in rows], np.float64).reshape(-1, 3).astype(F),
            "counts": np.array(lines[-1].split(), np.int64)}


def same_draw(got, want):
    return (np.array_equal(got["kind"], want["kind"]) and np.array_equal(got["index"], want["index"]) and np.array_equal(got["counts"], want["counts"])
            and np.array_equal(_bits(got["target"]), _bits(want["target"]))
            and np.array_equal(np.ascontiguousarray(got["points"], F).view(np.uint32), np.ascontiguousarray(want["points"], F).view(np.uint32)))


def test_header_constants(runners):
    out = subprocess.run([runners["plain"]], input="constants\n", capture_output=True, text=True, check=True).stdout.split()
    assert [int(t) for t in out] == [tfo.PAD, tfo.BAND, tfo.FREE, 3, 64, 64, 4096, 4096, 5, tfo.GOLDEN]


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_host_draw_equals_the_twin(runners, which):
    """every state, both min_obs; the sanitised build is the same program with its own main: nothing is preloaded"""
    for name, (state, origin, h, trunc) in all_states():
        for min_obs in (1, 2):
            for quota in ((255, 257), (0, 7), (7, 0), (10000, 10000)):
                seed = 1 + sum(name[1]) + min_obs
                want = expected_draw(name, min_obs, quota, seed)
                got = run_draw(runners[which], state, origin, h, trunc, *quota, seed, min_obs)
                assert same_draw(got, want), (name, min_obs, quota)
    state, origin, h, trunc = state_of("holes", (9, 8, 7))
    zero = (np.zeros_like(state[0]), np.zeros_like(state[1]))
    got = run_draw(runners[which], zero, origin, h, trunc, 3, 2, 2 ** 64 - 1, 1)
    assert same_draw(got, tfo.draw(zero, origin, h, trunc, 3, 2, 2 ** 64 - 1, 1)) and not got["kind"].any() and (got["index"] == -1).all()
    assert not got["counts"].any() and (got["points"] == origin.astype(F)).all() and not got["target"].any()


def run_loss(exe, case, with_min=True):
    P, N = case["sdf"].shape
    text = f"loss {P} {N} {int(with_min)}\n"
    for p in range(P):
        text += _hex([case["s"][p]]) + " " + _hex([case["trunc"][p]]) + (" " + _hex([case["min_loss"][p]]) if with_min else "") + "\n"
        text += " ".join(f"{int(k)} {float(v).hex()} {float(t).hex()}" for k, v, t in zip(case["kind"][p], case["sdf"][p], case["target"][p])) + "\n"
    out = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    lines = out.stdout.splitlines()
    assert len(lines) == 2 * P
    head = [line.split() for line in lines[0::2]]
    return {"loss": np.array([float.fromhex(r[0]) for r in head]), "min_loss": np.array([float.fromhex(r[1]) for r in head]),
            "improved": np.array([int(r[2]) for r in head], np.int32),
            "grad": np.array([[float.fromhex(t) for t in line.split()] for line in lines[1::2]], np.float64).astype(F)}


def expected_loss(case):
    min_loss, improved = case["min_loss"].copy(), case["improved"].copy()
    loss, grad = tfo.fit_loss(case["sdf"], case["s"], case["trunc"], case["target"], case["kind"], min_loss, improved)
    return {"loss": loss, "grad": grad, "min_loss": min_loss, "improved": improved}


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_host_loss_equals_the_twin(runners, which):
    for N, turn in [(N, turn) for N in LOSS_N for turn in (0, 1, 2)]:
        case, want = loss_case(N, turn), expected_loss(loss_case(N, turn))
        got = run_loss(runners[which], case)
        assert np.array_equal(_bits(got["loss"]), _bits(want["loss"])) and np.array_equal(got["grad"].view(np.uint32), want["grad"].view(np.uint32)), N
        assert np.array_equal(_bits(got["min_loss"]), _bits(want["min_loss"])) and np.array_equal(got["improved"], want["improved"]), N
        assert want["improved"].tolist() == [0, 1, 1] and want["loss"][1] == 0.0 and not want["grad"][1].any() and want["loss"][0] > 1e-30
        if N > 2:
            assert want["grad"][0].any() and want["grad"][2].any()


# ------------------------------------------------------------------------------------------------ properties of the twin
def test_ranks_are_distinct_ascending_and_inside_their_strata():
    for L, m in ((1, 1), (5, 3), (100, 7), (1000, 999), (8976, 256), (2 ** 31 - 1, 5)):
        for seed in (0, 1, 2 ** 64 - 1):
            r = tfo.ranks(L, m, seed, tfo.BAND)
            T = min(L, m)
            assert len(r) == T and all(a < b for a, b in zip(r, r[1:]))
            assert all((j * L) // T <= x < ((j + 1) * L) // T for j, x in enumerate(r))
    assert tfo.ranks(7, 7, 3, tfo.FREE) == list(range(7)) and tfo.ranks(7, 100, 3, tfo.FREE) == list(range(7)) and tfo.ranks(0, 5, 3, 1) == []
    assert tfo.ranks(1000, 10, 3, tfo.BAND) != tfo.ranks(1000, 10, 3, tfo.FREE)


def test_a_quota_above_the_list_takes_all_of_it_and_zero_takes_none():
    for name, (state, origin, h, trunc) in all_states():
        kd = tfo.kinds(state, 1).reshape(-1)
        d = expected_draw(name, 1, (10000, 10000), 1 + sum(name[1]) + 1)
        for k, cols in ((tfo.BAND, slice(0, 10000)), (tfo.FREE, slice(10000, 20000))):
            where = np.flatnonzero(kd == k)
            assert np.array_equal(d["index"][cols][:len(where)], where) and (d["index"][cols][len(where):] == -1).all()
            assert (d["kind"][cols][:len(where)] == k).all() and not d["kind"][cols][len(where):].any()
        assert d["counts"].tolist() == [int((kd != 0).sum()), int((kd == 1).sum()), int((kd == 2).sum())]
    state, origin, h, trunc = state_of("box", (9, 8, 7))
    d = tfo.draw(state, origin, h, trunc, 0, 7, 4)
    assert (d["kind"] == tfo.FREE).all() and d["taken"] == (0, 7)
    d = tfo.draw(state, origin, h, trunc, 7, 0, 4)
    assert (d["kind"] == tfo.BAND).all() and d["taken"] == (7, 0)


def test_a_problem_alone_equals_itself_anywhere_in_a_batch_and_seeds_differ():
    names = [("sphere", (9, 8, 7)), ("box", (9, 8, 7)), ("holes", (9, 8, 7))]
    sts = [state_of(*n) for n in names]
    big = tfo.draw(embedded(sts[0][0], (17, 16, 33)), *sts[0][1:], 20, 30, 11)
    small = tfo.draw(sts[0][0], *sts[0][1:], 20, 30, 11)
    assert all(np.array_equal(big[k], small[k]) for k in ("points", "target", "kind", "counts")) and not np.array_equal(big["index"], small["index"])
    alone = [tfo.draw(st[0], *st[1:], 20, 30, 11 + i) for i, st in enumerate(sts)]
    for order in ((0, 1, 2), (2, 0, 1), (1, 2, 0)):
        b = tfo.draw_batch([sts[i][0] for i in order], [sts[i][1] for i in order], [sts[i][2] for i in order], [sts[i][3] for i in order], 20, 30,
                           [11 + i for i in order])
        for row, i in enumerate(order):
            assert all(np.array_equal(b[k][row], alone[i][k]) for k in ("points", "target", "kind", "index", "counts"))
    st = sts[0]
    a, b = tfo.draw(st[0], *st[1:], 20, 30, 1), tfo.draw(st[0], *st[1:], 20, 30, 2)
    assert not np.array_equal(a["index"][:20], b["index"][:20]) and not np.array_equal(a["index"][20:], b["index"][20:])
    assert np.array_equal(a["kind"], b["kind"])


def test_points_and_targets_are_the_lattice_and_the_volume():
    from tsdf_sample_oracle import corner_values
    for name in (("sphere", (17, 16, 33)), ("holes", (9, 8, 7))):
        state, origin, h, trunc = state_of(*name)
        for min_obs in (1, 2):
            d = tfo.draw(state, origin, h, trunc, 300, 300, 9, min_obs)
            D, valid = corner_values(state, min_obs)
            live = d["index"] >= 0
            ijk = np.stack(np.unravel_index(d["index"][live], state[0].shape), 1)
            assert valid.reshape(-1)[d["index"][live]].all()
            assert np.array_equal(d["target"][live], trunc * D.reshape(-1)[d["index"][live]])
            assert np.array_equal(d["points"][live], (origin + h * ijk).astype(F))
            free = d["kind"] == tfo.FREE
            assert (d["target"][free] == trunc).all() and (np.abs(d["target"][d["kind"] == tfo.BAND]) <= trunc).all()
            assert (d["target"][d["kind"] == tfo.BAND] < trunc).all()


# ------------------------------------------------------------------------------------------------ the loss twin
def _plain_loss(case, p, sdf=None):
    """the straightforward float64 statement with math.fsum"""
    sdf = case["sdf"][p].astype(np.float64) if sdf is None else sdf
    s, trunc = float(case["s"][p]), float(case["trunc"][p])
    e2 = []
    for u, t, k in zip(sdf, case["target"][p], case["kind"][p]):
        if k == tfo.BAND:
            e2.append((u - t / s) ** 2)
        elif k == tfo.FREE:
            e2.append(min(u - trunc / s, 0.0) ** 2)
    return math.fsum(e2) / len(e2) if e2 else 0.0


def test_loss_twin_equals_the_plain_statement():
    """the chunk tree changes rounding only: every one of the m squares is added with a relative error of at most 2^-53 per addition it
    passes through, at most m of them, and the terms are non-negative: within m * 2^-52 * loss of the exactly rounded sum"""
    for N in LOSS_N:
        case = loss_case(N)
        loss, grad = tfo.fit_loss(case["sdf"], case["s"], case["trunc"], case["target"], case["kind"])
        for p in range(3):
            m = int((case["kind"][p] != tfo.PAD).sum())
            want = _plain_loss(case, p)
            assert abs(loss[p] - want) <= m * 2.0 ** -52 * want, (N, p, loss[p], want)
            assert (m == 0) == (p == 1)


def test_loss_gradient_is_the_central_difference():
    """The loss is a sum of quadratics (BAND) and half-quadratics (FREE) of single columns: the central difference with step d of a
    quadratic is exact, of the hinge too unless the kink lies within d of the value -- those columns are left out, and counted.  What is
    left is rounding: |loss| * 2^-52 * m / d from the two evaluations, and the fp32 rounding of the gradient, 2^-24 |g|."""
    d = 2.0 ** -10
    checked = 0
    for N in (255, 513):
        case = loss_case(N)
        _, grad = tfo.fit_loss(case["sdf"], case["s"], case["trunc"], case["target"], case["kind"])
        for p in (0, 2):
            base = case["sdf"][p].astype(np.float64)
            m = int((case["kind"][p] != tfo.PAD).sum())
            L = _plain_loss(case, p)
            kink = float(case["trunc"][p]) / float(case["s"][p])
            for i in range(0, N, 7):
                if case["kind"][p][i] == tfo.FREE and abs(base[i] - kink) <= d:
                    continue
                up, dn = base.copy(), base.copy()
                up[i] += d
                dn[i] -= d
                cd = (_plain_loss(case, p, up) - _plain_loss(case, p, dn)) / (2 * d)
                assert abs(cd - float(grad[p][i])) <= 4 * L * 2.0 ** -52 * m / d + 2.0 ** -23 * abs(cd) + 1e-300, (N, p, i, cd, grad[p][i])
                checked += 1
                if case["kind"][p][i] == tfo.PAD:
                    assert grad[p][i] == 0.0
    assert checked > 100


# ------------------------------------------------------------------------------------------------ the library, host side only
def test_symbols_and_bindings():
    from livingscenes_amd import _lib, build, ops
    from livingscenes_amd.lib_more.more_solver import More_Solver, solve_sequence
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "livingscenes_hip.h")).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and name + "(" in header, name
        res, args = _lib.SIGNATURES[name]
        assert getattr(lib, name).restype is res and list(getattr(lib, name).argtypes) == list(args)
    assert [len(_lib.SIGNATURES[n][1]) for n in NAMES] == [3, 20, 4, 21, 12]
    assert int(lib.ls_version()) == _lib.ABI_VERSION == 107 and "#define LS_ABI_VERSION 107" in header
    assert "ls_tsdf_draw_f32 / ls_tsdf_draw_batch_f32, ls_tsdf_fit_loss_f64" in header.split("#define LS_ABI_VERSION")[0]
    assert "times the\n * instance's scale s is a metric distance" in header or "scale s is a metric distance" in header
    assert "tsdffit.hip" in build.SOURCES and build.PACKED_FP32_GUARD["tsdffit.hip"] == []
    csrc = os.path.join(REPO, "livingscenes_amd", "csrc")
    plan_h = open(os.path.join(csrc, "tsdffit_plan.h")).read()
    assert "#include <hip" not in plan_h and '#include "ls_' not in plan_h and "contract(off)" in plan_h and '#include "tsdfsample_plan.h"' in plan_h
    assert "metric distance" in plan_h
    kernels = open(os.path.join(csrc, "tsdffit.hip")).read()
    assert "hipMalloc" not in kernels and "Synchronize" not in kernels and "atomicAdd" not in kernels and "atomicCAS" not in kernels
    assert kernels.count("LS_FIT_PASS(\"") == 4 and "scan_top_block" in kernels and "wave_tree_f64" in kernels and "Arena" in kernels
    for f in (ops.tsdf_draw, ops.tsdf_draw_batch):
        sig = inspect.signature(f).parameters
        assert list(sig) == ["state", "origin", "voxel", "trunc", "n_band", "n_free", "seeds", "min_obs"] and sig["min_obs"].default == 1
        for k in list(sig)[1:]:
            assert sig[k].kind is inspect.Parameter.KEYWORD_ONLY and (k == "min_obs" or sig[k].default is inspect.Parameter.empty)
    sig = inspect.signature(ops.tsdf_fit_loss).parameters
    assert list(sig) == ["sdf", "s", "trunc", "target", "kind", "min_loss", "improved"] and sig["min_loss"].default is None and sig["improved"].default is None
    sig = inspect.signature(More_Solver._optimize_code_on_fusion_batch).parameters
    assert list(sig) == ["self", "code", "fusion", "slots", "n_band", "n_free", "n_steps", "min_obs", "seed"]
    assert [sig[k].default for k in list(sig)[3:]] == [None, None, None, 200, 1, 0]
    doc = solve_sequence.__doc__
    assert "_optimize_code_on_fusion_batch" in doc and "NO QUOTA IS RECOMMENDED" in doc and "nothing here can measure the effect on matching" in doc


SEQUENCE_DEFAULTS = dict(optim=False, mesh=False, voxel=None, optimize_codes=False, overlap_radius=None, min_overlap=None, refine_radius=None,
                         refine_metric="point", normal_radius=None, consolidate=False, consolidate_radius=None, consolidate_max_variation=1 / 3,
                         consolidate_max_shift=float("inf"), carve_tol=None, carve_window=1, carve_min_free=1, carve_max_seen=0, carve_empty="unknown",
                         fuse_res=None, fuse_trunc_voxels=4, fuse_empty="unknown", fuse_mesh=False, fuse_min_obs=1)


def test_solve_sequence_keeps_its_signature_and_refuses_before_device_work():
    from livingscenes_amd.lib_more.more_solver import solve_sequence
    sig = inspect.signature(solve_sequence).parameters
    names = list(sig)
    assert names[:3] == ["solver", "ref", "rescans"] and names[3:3 + len(SEQUENCE_DEFAULTS)] == list(SEQUENCE_DEFAULTS)
    assert {k: sig[k].default for k in SEQUENCE_DEFAULTS} == SEQUENCE_DEFAULTS
    assert names[3 + len(SEQUENCE_DEFAULTS):] == ["code_fit_band", "code_fit_free", "code_fit_seed"]
    assert [sig[k].default for k in names[-3:]] == [None, None, 0]
    with pytest.raises(ValueError, match="fuse_res"):
        solve_sequence(None, None, [], optimize_codes="tsdf")
    for bad in ("points", "TSDF", 2, None):
        with pytest.raises(ValueError, match="optimize_codes"):
            solve_sequence(None, None, [], optimize_codes=bad, fuse_res=16)


def test_workspace_sizes():
    from livingscenes_amd import _lib
    lib = _lib.load()
    a256 = lambda x: -(-x // 256) * 256                                        # noqa: E731
    one, batch = lib.ls_tsdf_draw_workspace_bytes, lib.ls_tsdf_draw_batch_workspace_bytes
    assert one(0, 4, 4) == 0 and one(4, -1, 4) == 0 and one(2048, 1024, 1024) == 0 and batch(0, 4, 4, 4) == 0 and batch(65536, 1, 1, 1) == 0
    assert one(256, 256, 256) > 0 and one(256, 256, 257) == 0                  # 4096 blocks of 4096 samples, and one sample more
    assert batch(64, 64, 64, 64) > 0 and batch(127, 256, 256, 256) > 0 and batch(128, 256, 256, 256) == 0
    for P, dims in ((1, (1, 1, 1)), (1, (16, 16, 16)), (1, (1, 1, 4097)), (5, (9, 8, 7)), (64, (64, 64, 64))):
        nblk = -(-dims[0] * dims[1] * dims[2] // 4096)
        want = a256(8 * 6 * P) + a256(8 * P * nblk) + a256(8 * P) + a256(8 * P * nblk * 128)
        assert batch(P, *dims) == want and (P != 1 or one(*dims) == want), (P, dims)
    assert batch(64, 64, 64, 64) * 16 < 64 * 64 ** 3 * 8                        # the workspace is a small fraction of the state


GOOD = dict(P=2, nx=4, ny=4, nz=4, min_obs=1, n_band=3, n_free=2)


def _call(lib, single=False, origin=None, voxel=None, trunc=None, ws=True, ws_bytes=0, null=(), **kw):
    """the draw entries with made-up buffers: only for calls the host checks refuse before anything is dereferenced"""
    s = dict(GOOD, **kw)
    P = 1 if single else s["P"]
    ints, buf = (ctypes.c_int * 4096)(), (ctypes.c_double * 4096)()
    o = np.ascontiguousarray(np.zeros((max(P, 1), 3)) if origin is None else origin, np.float64)
    h = np.ascontiguousarray(np.full(max(P, 1), 0.01) if voxel is None else voxel, np.float64)
    tr = np.ascontiguousarray(np.full(max(P, 1), 0.04) if trunc is None else trunc, np.float64)
    sd = np.arange(max(P, 1), dtype=np.uint64)
    p = {k: (None if k in null else (ints if k in ("sum", "n", "index") else buf)) for k in ("sum", "n", "points", "target", "kind", "index", "counts")}
    optr = None if "origin" in null else o.ctypes.data
    outs = (p["points"], p["target"], p["kind"], p["index"], p["counts"], buf if ws else None, ws_bytes, None)
    if single:
        rc = lib.ls_tsdf_draw_f32(p["sum"], p["n"], s["nx"], s["ny"], s["nz"], s["min_obs"], optr, float(h[0]), float(tr[0]), s["n_band"], s["n_free"], 7,
                                  *outs)
    else:
        rc = lib.ls_tsdf_draw_batch_f32(P, p["sum"], p["n"], s["nx"], s["ny"], s["nz"], s["min_obs"], optr, None if "voxel" in null else h.ctypes.data,
                                        tr.ctypes.data, s["n_band"], s["n_free"], None if "seeds" in null else sd.ctypes.data, *outs)
    return rc, lib.ls_last_error().decode()


def test_every_host_refusal_of_the_draw():
    from livingscenes_amd import _lib
    lib = _lib.load()
    INVALID, WORKSPACE = -1, -3
    for single in (False, True):
        name = "tsdf_draw" + ("" if single else "_batch")
        call = functools.partial(_call, lib, single)
        last = 0 if single else 1
        for dims in (dict(nx=0), dict(ny=-1), dict(nz=0)):
            rc, msg = call(**dims)
            assert rc == INVALID and msg.startswith(name + ":") and "dims must be at least 1" in msg, msg
        rc, msg = call(nx=2048, ny=1024, nz=1024)
        assert rc == INVALID and "reaches 2^31" in msg, msg
        rc, msg = call(nx=256, ny=256, nz=257, P=1)
        assert rc == INVALID and "exceeds 4096 blocks of 4096 samples" in msg, msg
        for bad in (0, -3):
            rc, msg = call(min_obs=bad)
            assert rc == INVALID and "min_obs must be >= 1" in msg, msg
        for kw in (dict(n_band=-1), dict(n_free=-5)):
            rc, msg = call(**kw)
            assert rc == INVALID and "negative quota" in msg, msg
        rc, msg = call(n_band=0, n_free=0)
        assert rc == INVALID and "n_band + n_free must be at least 1" in msg, msg
        rc, msg = call(n_band=2 ** 30, n_free=2 ** 30)
        assert rc == INVALID and "reaches 2^31 (int column indices)" in msg, msg
        for bad in (0.0, -0.01, NAN, INF):
            rc, msg = call(voxel=[0.01, bad][-1:] if single else [0.01, bad])
            assert rc == INVALID and f"problem {last}" in msg and "voxel must be finite and > 0" in msg, (bad, msg)
            rc, msg = call(trunc=[0.04, bad][-1:] if single else [0.04, bad])
            assert rc == INVALID and f"problem {last}" in msg and "trunc must be finite and > 0" in msg, (bad, msg)
        for bad in (NAN, INF, -INF):
            o = np.zeros((last + 1, 3))
            o[-1, 1] = bad
            rc, msg = call(origin=o)
            assert rc == INVALID and f"problem {last}" in msg and "origin must be finite" in msg, (bad, msg)
        for k in ("sum", "n"):
            rc, msg = call(null=(k,))
            assert rc == INVALID and "null sum / n" in msg, (k, msg)
        rc, msg = call(null=("origin",))
        assert rc == INVALID and "null origin / voxel / trunc" in msg, msg
        for k in ("points", "target", "kind", "index"):
            rc, msg = call(null=(k,))
            assert rc == INVALID and "null points / target / kind / index" in msg, (k, msg)
        rc, msg = call(null=("counts",))
        assert rc == INVALID and "null counts" in msg, msg
        # the accepted extremes: only the workspace is short, and the error names the query
        rc, msg = call(voxel=[1e-300] * (last + 1), trunc=[1e300] * (last + 1), min_obs=2 ** 31 - 1)
        assert rc == WORKSPACE and f"ls_{name}_workspace_bytes" in msg, msg
        rc, msg = call(ws=False, ws_bytes=1 << 30)
        assert rc == WORKSPACE, msg
        need = getattr(lib, f"ls_{name}_workspace_bytes")(*(() if single else (2,)), 4, 4, 4)
        rc, msg = call(ws_bytes=need - 1)
        assert rc == WORKSPACE and f"{need - 1} < required {need}" in msg, msg
    for P in (0, -1):
        rc, msg = _call(lib, P=P)
        assert rc == INVALID and "P must be at least 1" in msg, msg
    rc, msg = _call(lib, P=65536, nx=1, ny=1, nz=1)
    assert rc == INVALID and "outside 1..65535" in msg, msg
    rc, msg = _call(lib, null=("seeds",))
    assert rc == INVALID and "null seeds" in msg, msg
    rc, msg = _call(lib, null=("voxel",))
    assert rc == INVALID and "null origin / voxel / trunc" in msg, msg


def test_every_host_refusal_of_the_loss():
    from livingscenes_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    args = dict(sdf=buf, s=buf, trunc=buf, target=buf, kind=buf, P=2, N=5, loss=buf, grad=buf)

    def call(**kw):
        a = dict(args, **kw)
        rc = lib.ls_tsdf_fit_loss_f64(a["sdf"], a["s"], a["trunc"], a["target"], a["kind"], a["P"], a["N"], a["loss"], a["grad"], None, None, None)
        return rc, lib.ls_last_error().decode()

    for kw in (dict(P=0), dict(N=0), dict(P=-1)):
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith("tsdf_fit_loss:") and "must be at least 1" in msg, msg
    rc, msg = call(P=65535, N=65536)
    assert rc == -1 and "reaches 2^31" in msg, msg
    rc, msg = call(P=65536, N=1)
    assert rc == -1 and "outside 1..65535" in msg, msg
    for k in ("sdf", "s", "trunc", "target", "kind"):
        rc, msg = call(**{k: None})
        assert rc == -1 and "null sdf / s / trunc / target / kind" in msg, (k, msg)
    for k in ("loss", "grad"):
        rc, msg = call(**{k: None})
        assert rc == -1 and "null loss / grad" in msg, (k, msg)


# ------------------------------------------------------------------------------------------------ the loop on the twin
LOOP_STATES = (("sphere", (9, 8, 7)), ("box", (9, 8, 7)), ("sphere", (17, 16, 33)), ("box", (17, 16, 33)))


def object_points(kind, dims, count=128, seed=0):
    """`count` points on the object the state of (kind, dims) was fused from, in the grid's frame -> float32 [count,3]"""
    origin, h, _ = grid_of(kind, dims)
    centre = origin + h * (np.array(dims) - 1) / 2
    rng = np.random.default_rng(seed + sum(dims))
    d = rng.normal(size=(count, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    if kind == "sphere":
        return (centre + 0.4 * d).astype(F)
    return (centre + d / np.abs(d / BOX_HALF).max(1)[:, None]).astype(F)      # the ray through d cut at the box


@functools.lru_cache(maxsize=None)
def loop_start(names=LOOP_STATES):
    """the codes the oracle encoder gives 128 points on each object (the small prior's weights) -> (code dict of CPU tensors, dcfg, dw)"""
    import torch
    from livingscenes_amd import synth
    from oracle import net
    ecfg, dcfg = synth.small_encoder_cfg(), synth.small_decoder_cfg()
    ew, dw = synth.make_encoder_weights(ecfg, 4), synth.make_decoder_weights(dcfg, 4)
    x = torch.from_numpy(np.stack([object_points(*n).T for n in names]))
    with torch.no_grad():
        code = net.shape_prior_encode(ew, ecfg, x)
    return {k: v.detach().clone() for k, v in code.items()}, dcfg, dw


def embedded(state, dims):
    """the state in the low corner of a larger volume whose other samples were never observed: the lexicographic order of its samples,
    hence every list rank and every drawn point and target, is the same -- so states of different dims can share one batch"""
    out = tuple(np.zeros(dims, np.int32) for _ in range(2))
    for big, small in zip(out, state):
        big[tuple(slice(0, d) for d in small.shape)] = small
    return out


def oracle_loop(names, n_band, n_free, steps, seeds, min_obs=1, states=None):
    """The loop of More_Solver._optimize_code_on_fusion_batch on the CPU: the twin's draw, the oracle decoder with torch autograd, the
    loss of the definition written in torch (float64), torch.optim.Adam at the reference's rates.
    -> (start code dict, final code dict, losses [steps, P] float64, the draws)"""
    import torch
    from oracle import net
    start, dcfg, dw = loop_start(tuple(names))
    P = len(names)
    sts = [state_of(*n) for n in names] if states is None else states
    draws = [tfo.draw(st[0], st[1], st[2], st[3], n_band, n_free, sd, min_obs) for st, sd in zip(sts, seeds)]
    pts = torch.from_numpy(np.stack([d["points"] for d in draws]))
    target = torch.from_numpy(np.stack([d["target"] for d in draws]))
    kind = torch.from_numpy(np.stack([d["kind"] for d in draws]))
    trunc = torch.tensor([float(st[3]) for st in sts], dtype=torch.float64)
    c = {k: v.clone() for k, v in start.items()}
    params = [{"params": c["z_inv"], "lr": 1e-5}, {"params": c["t"], "lr": 1e-4}, {"params": c["z_so3"], "lr": 5e-4}]
    for p in params:
        p["params"].requires_grad_(True)
    opt = torch.optim.Adam(params)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[160], gamma=0.1)
    s64 = c["s"].reshape(P, 1).double()
    m = (kind != tfo.PAD).sum(1).clamp(min=1).double()
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        u = net.field_query_with_grad(dw, dcfg, pts, c).reshape(P, -1).double()
        e = torch.where(kind == tfo.BAND, u - target / s64, torch.where(kind == tfo.FREE, (u - trunc[:, None] / s64).clamp(max=0.0), torch.zeros_like(u)))
        per = (e * e).sum(1) / m
        per.sum().backward()
        losses.append(per.detach().numpy().copy())
        opt.step()
        sched.step()
    return start, {k: v.detach() for k, v in c.items()}, np.stack(losses), draws


def test_the_twin_level_loop_lowers_the_loss():
    """25 Adam steps at the reference's rates with the twin's REAL draw (quotas 256 + 256, seed 1) on sphere and box at (9,8,7) and
    (17,16,33), the small prior's weights: the loss at the last step lies below the loss at the first on all four states.  At (9,8,7)
    trunc / s lies above the untrained decoder's values, so the hinges are active; at (17,16,33) it lies below them."""
    start, final, losses, draws = oracle_loop(LOOP_STATES, 256, 256, 25, [1, 1, 1, 1])
    assert losses.shape == (25, 4)
    for p, name in enumerate(LOOP_STATES):
        assert losses[-1, p] < losses[0, p], (name, losses[0, p], losses[-1, p])
        assert draws[p]["taken"][0] > 0 and draws[p]["taken"][1] > 0, name
    s = start["s"].reshape(-1).numpy()
    assert abs(state_of(*LOOP_STATES[0])[3] / s[0] - 0.085) < 0.02 and abs(state_of(*LOOP_STATES[2])[3] / s[2] - 0.023) < 0.01
