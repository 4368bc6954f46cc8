"""CPU-only tests (-m "not gpu") of the completion of a fused state by the shape prior's field (include/livingscenes_hip.h:
ls_tsdf_prior_rows_f32, ls_tsdf_prior_vote_f32): hand cases of the NumPy twin (tests/tsdf_prior_oracle.py) against exact rational
arithmetic; csrc/tsdfprior_plan.h -- compiled on its own with the host compiler and run by tests/tools/tsdfprior_plan_run.cpp, plain and
under AddressSanitizer / UBSan -- against the twin by equality; what the C entry points decide on the host before any HIP call; the
bindings; solve_sequence_completed's refusals; and the capability on the twins alone: the sphere of tests/test_hip_tsdf_prior.py, whose
observed mesh is open and whose completed mesh is closed.  The states, the planted values and the sphere of the GPU tests live here."""
import ctypes
import functools
import inspect
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, ".."))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import fuse_oracle as fo               # noqa: E402
import tsdf_prior_oracle as tpo        # noqa: E402
from test_depth_fuse_cpu import _look_at, _rot, _sphere_depth   # noqa: E402

NAMES = ("ls_tsdf_prior_rows_workspace_bytes", "ls_tsdf_prior_rows_f32", "ls_tsdf_prior_vote_f32", "ls_tsdf_prior_rows_batch_workspace_bytes",
         "ls_tsdf_prior_rows_batch_f32", "ls_tsdf_prior_vote_batch_f32")
F = np.float32
NAN, INF = float("nan"), float("inf")
EDGE_DIMS = ((1, 1, 65), (3, 5, 7), (1, 64, 64), (16, 16, 17))   # one past a ballot word, under two words, one 4096 block, a block + 4 words
WEIGHTS = (1, 3, 65535)


def exact_vote(sum_, n, w0, s, f, trunc):
    """steps 1, 3 and 4 in exact rational arithmetic (s, f, trunc dyadic: the float64 operations of the definition are exact too)"""
    w = max(w0 - n, 0)
    if w == 0 or f != f:
        return sum_, n
    t = Fraction(1) if f == INF else Fraction(-1) if f == -INF else max(Fraction(-1), min(Fraction(1), Fraction(s) * Fraction(float(F(f))) / Fraction(trunc)))
    q = (t * 16384 + Fraction(1, 2)).__floor__()
    return sum_ + w * q, n + w


def edge_grid(dims):
    """a grid that is not dyadic around a sphere of r = 0.3 h max(dims): origin, voxel, trunc"""
    h = 0.0137
    return np.array([-0.31, 0.17, 1.003]), h, 3 * h


def planted_values(R, s, trunc, seed):
    """R fp32 values for the rows of one problem: the special values of the definition first (as many as fit), then uniform over
    +-2 trunc / s.  Specials: +-trunc/s (the fp32 nearest), one ulp inside and beyond each, +-inf, NaN, -0.0, 0.0, and t * 16384 at
    k + 0.5 for both signs (exact where s and trunc are dyadic, the nearest fp32 otherwise)."""
    rng = np.random.default_rng(seed)
    e = F(trunc / s)
    tie = [F((k + 0.5) / 16384 * trunc / s) for k in (5, -6, 16383, -16384, 0, -1)]
    special = [e, -e, np.nextafter(e, F(0)), np.nextafter(-e, F(0)), np.nextafter(e, F(1e9)), np.nextafter(-e, F(-1e9)), F(INF), F(-INF), F(NAN), F(-0.0),
               F(0.0), F(3) * e, F(-3) * e] + tie
    f = rng.uniform(-2 * trunc / s, 2 * trunc / s, size=R).astype(F)
    k = min(R, len(special))
    at = rng.permutation(R)[:k]
    f[at] = np.array(special[:k], F)
    return f


def hand_set(state, w0, kind, seed):
    """state (writable int32 arrays) with hand-set samples.  kind "mixed": a block of never-observed samples, samples at n = w0 - 1, w0
    and 65535 with sum at +-n * 16384 or in between; "empty": all zero; "saturated": n >= w0 everywhere."""
    S, N = state
    rng = np.random.default_rng(seed)
    if kind == "empty":
        S[...] = 0
        N[...] = 0
    elif kind == "saturated":
        add = np.maximum(w0 - N, 0)
        S += (add * rng.integers(-16384, 16385, size=N.shape)).astype(np.int32)
        N += add.astype(np.int32)
    else:
        flat_s, flat_n = S.reshape(-1), N.reshape(-1)
        V = flat_n.size
        at = rng.permutation(V)
        pick = [at[i::6][:max(1, V // 12)] for i in range(6)]
        for idx, n in zip(pick, (0, max(w0 - 1, 0), w0, 65535, min(w0 + 1, 65535), 1)):
            flat_n[idx] = n
            flat_s[idx] = n * rng.choice([-16384, 16384, 0, 777], size=len(idx))
    return state


@functools.lru_cache(maxsize=None)
def sphere_case(res=24, r=0.3, views=2, trunc_voxels=3):
    """the capability case: a sphere of radius r centred in a res^3 grid of side 1, fused from `views` cameras on one side (the twin's
    fusion), trunc = 3 h -> (state, origin, h, trunc, centre, depth [V,H,W], K [V,4], E [V,3,4]); read-only"""
    h = 1.0 / (res - 1)
    origin = np.array([-0.5, -0.5, -0.5])
    centre = origin + h * (res - 1) / 2
    K = np.array([100.0, 100.0, 50.0, 50.0])
    base = _rot(np.random.default_rng(3))
    rots = []
    for v in range(views):                                                 # cameras 25 degrees apart: most of what one sees the next sees too
        a = np.deg2rad(25.0 * v)
        rots.append(base @ np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]]))
    E = np.stack([_look_at(R) for R in rots])
    depth = np.stack([_sphere_depth(e, K, 100, 100, r) for e in E])
    Eg = E.copy()
    Eg[:, :, 3] -= E[:, :, :3] @ centre
    Kv = np.tile(K, (views, 1))
    state = fo.new_state((res,) * 3)
    fo.fuse(state, depth, Kv, Eg, origin, h, trunc_voxels * h)
    for t in state:
        t.setflags(write=False)
    return state, origin, h, trunc_voxels * h, centre, depth, Kv, Eg


def sphere_field(points, centre, r, s):
    """the analytic distance to the sphere at fp32 rows, in the decoder's units (metric distance / s), fp32: float64 from the fp32 rows"""
    p = np.asarray(points, F).astype(np.float64)
    return ((np.sqrt(((p - centre[None, :]) ** 2).sum(1)) - r) / np.float64(s)).astype(F)


def least_seen_around(N, vertices, origin, h):
    """per mesh vertex the least n over every sample that a cube naming the vertex reads: the vertex lies on a lattice edge (one
    coordinate between two lattice planes, the others on one), and the up to four cubes around that edge read the two planes of the
    edge's axis and the three planes around it on the other axes; a vertex ON a lattice point takes three planes on every axis"""
    u = (np.asarray(vertices, np.float64) - origin) / h
    near = np.rint(u)
    on = np.abs(u - near) < 1e-6
    out = np.zeros(len(u), np.int64)
    for k, (row, lat, flags) in enumerate(zip(u, near.astype(np.int64), on)):
        sl = tuple(slice(max(c - 1, 0), c + 2) if f else slice(int(np.floor(x)), int(np.floor(x)) + 2) for x, c, f in zip(row, lat, flags))
        out[k] = N[sl].min()
    return out


def boundary_edges(faces):
    """-> (edges that belong to exactly one face, edges that belong to more than two)"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    _, c = np.unique(e, axis=0, return_counts=True)
    return int((c == 1).sum()), int((c > 2).sum())


# ------------------------------------------------------------------------------------------------ hand cases of the twin
def test_weights_and_the_invariants_of_the_state():
    n = np.array([0, 2, 3, 4, 65535], np.int32)
    assert tpo.weights((n, n), 3).tolist() == [3, 1, 0, 0, 0]                    # n = 0, w0 - 1, w0, above, saturated
    assert tpo.weights((n, n), 1).tolist() == [1, 0, 0, 0, 0] and tpo.weights((n, n), 65535).tolist() == [65535, 65533, 65532, 65531, 0]
    for bad in (0, -1, 65536):
        with pytest.raises(ValueError):
            tpo.weights((n, n), bad)
    rng = np.random.default_rng(0)
    for w0 in WEIGHTS:
        N = rng.choice([0, 1, 2, 3, 65534, 65535], size=(4, 5, 6)).astype(np.int32)
        S = (N.astype(np.int64) * rng.integers(-16384, 16385, size=N.shape)).astype(np.int32)
        S.reshape(-1)[:7] = (N.reshape(-1)[:7].astype(np.int64) * 16384).astype(np.int32)
        R = int((N < w0).sum())
        f = planted_values(R, 2.0, 0.25, w0)
        (S2, N2), counts = tpo.vote((S, N), f, 2.0, 0.25, w0)
        voted = np.zeros(N.size, bool)
        voted[np.flatnonzero(N.reshape(-1) < w0)[~np.isnan(f)]] = True
        voted = voted.reshape(N.shape)
        assert np.array_equal(N2[voted], np.maximum(N, w0)[voted]) and np.array_equal(N2[~voted], N[~voted]) and np.array_equal(S2[~voted], S[~voted])
        assert N2.max() <= 65535 and (np.abs(S2.astype(np.int64)) <= N2.astype(np.int64) * 16384).all()
        assert counts.tolist() == [R, int(voted.sum()), R - int(voted.sum()), N.size - R] and counts[2] == (1 if R > 8 else counts[2])


def test_hand_votes_equal_exact_arithmetic():
    """s = 2, trunc = 0.25 (dyadic: t = s f / trunc is exact): f exactly +-trunc / s, one ulp inside, one beyond, far beyond, +-inf, NaN,
    -0.0, and t * 16384 exactly at k + 0.5 for both signs; against n = 0, w0 - 1, w0, 65535 and the weights 1, 3, 65535"""
    s, trunc = 2.0, 0.25
    e = F(trunc / s)
    assert float(e) == 0.125
    ties = {k: F((k + 0.5) / 16384 * trunc / s) for k in (5, -6, 0, -1, 16383, -16384)}
    for k, v in ties.items():
        assert Fraction(s) * Fraction(float(v)) / Fraction(trunc) * 16384 == Fraction(2 * k + 1, 2)        # exactly k + 0.5
    fs = [e, -e, np.nextafter(e, F(0)), np.nextafter(-e, F(0)), np.nextafter(e, F(1)), np.nextafter(-e, F(-1)), F(7.5), F(-7.5), F(INF), F(-INF), F(NAN),
          F(-0.0), F(0.0)] + list(ties.values())
    assert tpo.quantise(s, np.array([e, -e, np.nextafter(e, F(1)), F(INF), F(-INF), F(-0.0)], F), trunc).tolist() == [16384, -16384, 16384, 16384, -16384, 0]
    assert tpo.quantise(s, np.array([ties[5], ties[-6], ties[0], ties[-1]], F), trunc).tolist() == [6, -5, 1, 0]   # floor(x + 0.5): ties go up
    for w0 in WEIGHTS:
        for n in sorted({0, 1, w0 - 1, w0, 65535} - {-1}):
            for sum_ in sorted({0, n * 16384, -n * 16384, n * 5}):
                S = np.full((1, 1, len(fs)), sum_, np.int32)
                N = np.full((1, 1, len(fs)), n, np.int32)
                r = tpo.rows((S, N), np.zeros(3), 1.0, w0)
                assert len(r["row_index"]) == (len(fs) if n < w0 else 0)
                (S2, N2), counts = tpo.vote((S, N), np.array(fs, F)[:len(r["row_index"])], s, trunc, w0)
                want = [exact_vote(sum_, n, w0, s, float(f), trunc) for f in fs]
                assert S2.reshape(-1).tolist() == [a for a, _ in want] and N2.reshape(-1).tolist() == [b for _, b in want], (w0, n, sum_)
                assert counts.tolist() == ([len(fs), len(fs) - 1, 1, 0] if n < w0 else [0, 0, 0, len(fs)])
    # sum' at its bound: an empty sample filled with 65535 votes of +-1, and a saturated +1 state topped up by one vote
    for f, sign in ((F(INF), 1), (F(-INF), -1), (e, 1), (-e, -1)):
        (S2, N2), _ = tpo.vote((np.zeros((1, 1, 1), np.int32), np.zeros((1, 1, 1), np.int32)), np.array([f], F), s, trunc, 65535)
        assert (int(S2[0, 0, 0]), int(N2[0, 0, 0])) == (sign * 65535 * 16384, 65535)
    (S2, N2), _ = tpo.vote((np.full((1, 1, 1), 65534 * 16384, np.int32), np.full((1, 1, 1), 65534, np.int32)), np.array([e], F), s, trunc, 65535)
    assert (int(S2[0, 0, 0]), int(N2[0, 0, 0])) == (65535 * 16384, 65535)


def test_rows_are_the_lattice_in_index_order_and_batches_are_their_parts():
    origin, h, _ = edge_grid((3, 5, 7))
    rng = np.random.default_rng(1)
    sts = []
    for kind in ("mixed", "empty", "saturated"):
        N = rng.choice([0, 1, 2, 5], size=(3, 5, 7)).astype(np.int32)
        sts.append(hand_set((N * 100, N.copy()), 3, kind, 4))
    alone = [tpo.rows(st, origin, h, 3) for st in sts]
    assert len(alone[1]["row_index"]) == 105 and len(alone[2]["row_index"]) == 0 and 0 < len(alone[0]["row_index"]) < 105
    for r, st in zip(alone, sts):
        idx = r["row_index"]
        assert (np.diff(idx) > 0).all() and (st[1].reshape(-1)[idx] < 3).all() and r["counts"][0] == len(idx) == (st[1] < 3).sum()
        ijk = np.stack(np.unravel_index(idx, (3, 5, 7)), 1).reshape(-1, 3)
        assert np.array_equal(r["points"], (origin + h * ijk).astype(F))
    for order in ((0, 1, 2), (2, 1, 0), (1, 2, 0)):
        b = tpo.rows_batch([sts[i] for i in order], [origin] * 3, [h] * 3, 3)
        for slot, i in enumerate(order):
            lo, hi = b["offsets"][slot], b["offsets"][slot + 1]
            assert np.array_equal(b["points"][lo:hi], alone[i]["points"]) and np.array_equal(b["row_index"][lo:hi], alone[i]["row_index"])
            assert (b["row_inst"][lo:hi] == slot).all() and np.array_equal(b["counts"][slot], alone[i]["counts"])


# ------------------------------------------------------------------------------------------------ tsdfprior_plan.h on the host
def _compile(out, flags):
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *flags, "-I",
                    os.path.join(REPO, "livingscenes_amd", "csrc"), os.path.join(HERE, "tools", "tsdfprior_plan_run.cpp"), "-o", out], check=True)
    return out


@pytest.fixture(scope="module")
def runners(tmp_path_factory):
    d = tmp_path_factory.mktemp("tsdfprior_plan")
    return {"plain": _compile(str(d / "run"), ["-O1"]),
            "sanitized": _compile(str(d / "run_san"), ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])}


def _hex(values):
    return " ".join(float(v).hex() for v in np.asarray(values).reshape(-1))


def run_complete(exe, state, origin, voxel, trunc, s, w0, f):
    S, N = state
    text = "complete " + " ".join(map(str, [*S.shape, w0, len(f)])) + "\n" + _hex([*origin, voxel, trunc, s]) + "\n"
    text += " ".join(map(str, S.reshape(-1).tolist())) + "\n" + " ".join(map(str, N.reshape(-1).tolist())) + "\n" + _hex(f) + "\n"
    out = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    lines = out.stdout.splitlines()
    assert len(lines) == len(f) + 3
    rows = [line.split() for line in lines[:len(f)]]
    return {"row_index": np.array([int(r[0]) for r in rows], np.int32),
            "points": np.array([[float.fromhex(t) for t in r[1:]] for r in rows], np.float64).reshape(-1, 3).astype(F),
            "sum": np.array(lines[-3].split(), np.int64).astype(np.int32).reshape(S.shape),
            "n": np.array(lines[-2].split(), np.int64).astype(np.int32).reshape(S.shape), "counts": np.array(lines[-1].split(), np.int64)}


def test_header_constants_and_checks(runners):
    out = subprocess.run([runners["plain"]], input="constants\n", capture_output=True, text=True, check=True).stdout.split()
    assert [int(t) for t in out] == [tpo.ELIGIBLE, tpo.VOTED, tpo.SKIPPED, tpo.UNTOUCHED, 4, 64, 64, 4096, 4096, 65535, 6]

    def checks(w0, s, P, dims):
        text = f"checks {w0} {s if isinstance(s, str) else float(s).hex()} {P} {dims[0]} {dims[1]} {dims[2]}\n"
        return [int(t) for t in subprocess.run([runners["plain"]], input=text, capture_output=True, text=True, check=True).stdout.split()]

    assert checks(1, 1.0, 1, (4, 4, 4)) == [0, 0, 0, 1] and checks(65535, 1e-300, 65535, (1, 1, 1)) == [0, 0, 0, 1]
    assert [checks(w, 1.0, 1, (4, 4, 4))[0] for w in (0, -1, 65536, 2 ** 31 - 1)] == [1] * 4
    assert [checks(1, s, 1, (4, 4, 4))[1] for s in (0.0, -1.0, "nan", "inf", "-inf")] == [1] * 5
    assert checks(1, 1.0, 1, (256, 256, 256))[2] == 0 and checks(1, 1.0, 1, (256, 256, 257))[2] == 1 and checks(1, 1.0, 65536, (1, 1, 1))[2] == 2
    assert checks(1, 1.0, 1, (2048, 1024, 1024))[3] == 0


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_host_plan_equals_the_twin(runners, which):
    """random states on the four edge dims, the three weights, dyadic and non-dyadic scalars; the sanitised build is the same program
    with its own main: nothing is preloaded"""
    for d, dims in enumerate(EDGE_DIMS):
        origin, h, trunc = edge_grid(dims)
        for w0 in WEIGHTS:
            for kind in ("mixed", "empty", "saturated"):
                rng = np.random.default_rng(100 * d + w0 % 7)
                N = rng.choice([0, 1, 2, 3], size=dims).astype(np.int32)
                S = (N * rng.integers(-16384, 16385, size=dims)).astype(np.int32)
                state = hand_set((S, N), w0, kind, d + w0)
                s, tr = ((2.0, 0.25) if kind == "mixed" and w0 == 3 else (0.37 + d, trunc))
                want_rows = tpo.rows(state, origin, h, w0)
                f = planted_values(len(want_rows["row_index"]), s, tr, d + w0)
                want_state, want_counts = tpo.vote(state, f, s, tr, w0)
                got = run_complete(runners[which], state, origin, h, tr, s, w0, f)
                assert np.array_equal(got["row_index"], want_rows["row_index"]), (dims, w0, kind)
                assert np.array_equal(got["points"].view(np.uint32), want_rows["points"].view(np.uint32)), (dims, w0, kind)
                assert np.array_equal(got["sum"], want_state[0]) and np.array_equal(got["n"], want_state[1]), (dims, w0, kind)
                assert np.array_equal(got["counts"], want_counts), (dims, w0, kind)
                assert (kind != "empty" or got["counts"][0] == N.size) and (kind != "saturated" or got["counts"][0] == 0)
    out = subprocess.run([runners[which]], input="complete 1 1 2 1 5\n" + _hex([0, 0, 0, 1, 1, 1]) + "\n0 0\n0 0\n" + _hex([0] * 5), capture_output=True, text=True)
    assert out.returncode == 4                                                    # five values for two eligible samples


# ------------------------------------------------------------------------------------------------ the library, host side only
def test_symbols_and_bindings():
    from livingscenes_amd import _lib, build, ops
    from livingscenes_amd.lib_more import more_solver
    from livingscenes_amd.lib_more.more_solver import More_Solver, solve_sequence_completed
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "livingscenes_hip.h")).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and name + "(" in header, name
        res, args = _lib.SIGNATURES[name]
        assert getattr(lib, name).restype is res and list(getattr(lib, name).argtypes) == list(args)
    assert [len(_lib.SIGNATURES[n][1]) for n in NAMES] == [3, 16, 16, 4, 17, 17]
    assert int(lib.ls_version()) == _lib.ABI_VERSION == 107 and "#define LS_ABI_VERSION 107" in header
    before = header.split("#define LS_ABI_VERSION")[0]
    assert "ls_tsdf_prior_rows_f32 / ls_tsdf_prior_rows_batch_f32, ls_tsdf_prior_vote_f32 / ls_tsdf_prior_vote_batch_f32" in before
    assert "w = max(w0 - n, 0)" in header and "q = (int) floor(t * 16384 + 0.5)" in header and "A NaN f casts no vote" in header
    assert "tsdfprior.hip" in build.SOURCES and build.PACKED_FP32_GUARD["tsdfprior.hip"] == []
    csrc = os.path.join(REPO, "livingscenes_amd", "csrc")
    plan_h = open(os.path.join(csrc, "tsdfprior_plan.h")).read()
    assert "#include <hip" not in plan_h and '#include "ls_' not in plan_h and "contract(off)" in plan_h and '#include "fuse_plan.h"' in plan_h
    assert "fp::fuse_position(" in plan_h and all(f"LS_CP_HD {t} {n}(" in plan_h for t, n in (("long long", "prior_weight"), ("void", "prior_row"),
                                                                                              ("int", "prior_quantise"), ("int", "prior_vote")))
    kernels = open(os.path.join(csrc, "tsdfprior.hip")).read()
    assert "hipMalloc" not in kernels and "Synchronize" not in kernels and "atomicCAS" not in kernels and kernels.count("atomicAdd(") == 1
    assert kernels.count("LS_PRIOR_PASS(\"") == 4 and kernels.count("scan_top_block<") == 1 and "Arena" in kernels and "contract(off)" in kernels
    for f in (ops.tsdf_prior_rows, ops.tsdf_prior_rows_batch):
        sig = inspect.signature(f).parameters
        assert list(sig) == ["state", "origin", "voxel", "weight", "packed"] and sig["packed"].default is False
        assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY and sig[k].default is inspect.Parameter.empty for k in ("origin", "voxel", "weight"))
    for f in (ops.tsdf_complete, ops.tsdf_complete_batch):
        sig = inspect.signature(f).parameters
        assert list(sig) == ["state", "values", "rows", "s", "trunc", "weight"]
        assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY and sig[k].default is inspect.Parameter.empty for k in ("s", "trunc", "weight"))
    assert ops.PRIOR_COUNT == ("eligible", "voted", "skipped_nonfinite", "untouched")
    sig = inspect.signature(More_Solver._complete_fusion_batch).parameters
    assert list(sig) == ["self", "fusion", "code", "slots", "weight", "max_rows"] and sig["weight"].default is inspect.Parameter.empty
    assert sig["weight"].kind is inspect.Parameter.KEYWORD_ONLY and sig["max_rows"].default == 1 << 20 and sig["slots"].default is None
    assert list(inspect.signature(More_Solver._completed_mesh_batch).parameters) == ["fusion", "completed"]
    assert "deepsdf" in More_Solver._complete_fusion_batch.__doc__ and "NONE IS RECOMMENDED" in More_Solver._complete_fusion_batch.__doc__
    sig = inspect.signature(solve_sequence_completed).parameters
    assert list(sig) == ["solver", "ref", "rescans", "complete_weight", "complete_mesh", "kw"] and sig["complete_mesh"].default is True
    assert sig["complete_weight"].default is inspect.Parameter.empty and "NONE IS RECOMMENDED" in solve_sequence_completed.__doc__
    assert "complete_weight" not in inspect.signature(more_solver.solve_sequence).parameters


def test_solve_sequence_completed_refuses_before_device_work():
    from livingscenes_amd.lib_more.more_solver import solve_sequence_completed
    with pytest.raises(ValueError, match="fuse_res"):
        solve_sequence_completed(None, None, [], complete_weight=2)
    for bad in (0, -1, 65536, 1.5, None, True, "2"):
        with pytest.raises(ValueError, match="weight"):
            solve_sequence_completed(None, None, [], complete_weight=bad, fuse_res=16)
    with pytest.raises(TypeError):
        solve_sequence_completed(None, None, [], fuse_res=16)                    # no default


def test_workspace_sizes():
    from livingscenes_amd import _lib
    lib = _lib.load()
    a256 = lambda x: -(-x // 256) * 256                                        # noqa: E731
    one, batch = lib.ls_tsdf_prior_rows_workspace_bytes, lib.ls_tsdf_prior_rows_batch_workspace_bytes
    assert one(0, 4, 4) == 0 and one(4, -1, 4) == 0 and one(2048, 1024, 1024) == 0 and batch(0, 4, 4, 4) == 0 and batch(65536, 1, 1, 1) == 0
    assert one(256, 256, 256) > 0 and one(256, 256, 257) == 0                  # 4096 blocks of 4096 samples, and one sample more
    for P, dims in ((1, (1, 1, 1)), (1, (1, 1, 65)), (1, (1, 64, 64)), (3, (16, 16, 17)), (1, (1, 1, 4097)), (64, (64, 64, 64))):
        nblk = -(-dims[0] * dims[1] * dims[2] // 4096)
        want = a256(8 * 6 * P) + a256(8 * P * nblk) + a256(8 * P * nblk * 64)
        assert batch(P, *dims) == want and (P != 1 or one(*dims) == want), (P, dims)
    assert batch(64, 64, 64, 64) * 32 < 64 * 64 ** 3 * 8                        # the workspace is a small fraction of the state


GOOD = dict(P=2, nx=4, ny=4, nz=4, weight=2, cap=64, rows=10)


def _rows_call(lib, single=False, origin=None, voxel=None, ws=True, ws_bytes=0, null=(), **kw):
    """the rows entries with made-up buffers: only for calls the host checks refuse before anything is dereferenced"""
    a = dict(GOOD, **kw)
    P = 1 if single else a["P"]
    ints, buf = (ctypes.c_int * 4096)(), (ctypes.c_double * 4096)()
    o = np.ascontiguousarray(np.zeros((max(P, 1), 3)) if origin is None else origin, np.float64)
    h = np.ascontiguousarray(np.full(max(P, 1), 0.01) if voxel is None else voxel, np.float64)
    p = {k: (None if k in null else ints) for k in ("n", "points", "row_inst", "row_index", "row_off", "counts")}
    optr = None if "origin" in null else o.ctypes.data
    tail = (p["points"], p["row_inst"], p["row_index"], a["cap"], p["row_off"], p["counts"], buf if ws else None, ws_bytes, None)
    if single:
        rc = lib.ls_tsdf_prior_rows_f32(p["n"], a["nx"], a["ny"], a["nz"], a["weight"], optr, float(h[0]), *tail)
    else:
        rc = lib.ls_tsdf_prior_rows_batch_f32(P, p["n"], a["nx"], a["ny"], a["nz"], a["weight"], optr, None if "voxel" in null else h.ctypes.data, *tail)
    return rc, lib.ls_last_error().decode()


def _vote_call(lib, single=False, s=None, trunc=None, ws=True, ws_bytes=0, null=(), alias=False, **kw):
    a = dict(GOOD, **kw)
    P = 1 if single else a["P"]
    ints, outs, buf = (ctypes.c_int * 4096)(), (ctypes.c_int * 4096)(), (ctypes.c_double * 4096)()
    sv = np.ascontiguousarray(np.full(max(P, 1), 1.5) if s is None else s, np.float64)
    tr = np.ascontiguousarray(np.full(max(P, 1), 0.04) if trunc is None else trunc, np.float64)
    p = {k: (None if k in null else (outs if k in ("sum_out", "n_out") and not alias else ints)) for k in ("sum", "n", "values", "sum_out", "n_out", "counts")}
    tail = (p["values"], a["rows"], p["sum_out"], p["n_out"], p["counts"], buf if ws else None, ws_bytes, None)
    if single:
        rc = lib.ls_tsdf_prior_vote_f32(p["sum"], p["n"], a["nx"], a["ny"], a["nz"], a["weight"], float(sv[0]), float(tr[0]), *tail)
    else:
        rc = lib.ls_tsdf_prior_vote_batch_f32(P, p["sum"], p["n"], a["nx"], a["ny"], a["nz"], a["weight"], None if "s" in null else sv.ctypes.data,
                                              None if "trunc" in null else tr.ctypes.data, *tail)
    return rc, lib.ls_last_error().decode()


def test_every_host_refusal():
    """each returns its code before the device is touched: the buffers are host memory, and this test runs without a GPU"""
    from livingscenes_amd import _lib
    lib = _lib.load()
    INVALID, WORKSPACE = -1, -3
    for single in (False, True):
        last = 0 if single else 1
        for fn, name in ((_rows_call, "tsdf_prior_rows"), (_vote_call, "tsdf_prior_vote")):
            name += "" if single else "_batch"
            call = functools.partial(fn, lib, single)
            for dims in (dict(nx=0), dict(ny=-1), dict(nz=0)):
                rc, msg = call(**dims)
                assert rc == INVALID and msg.startswith(name + ":") and "dims must be at least 1" in msg, msg
            rc, msg = call(nx=2048, ny=1024, nz=1024)
            assert rc == INVALID and "reaches 2^31" in msg, msg
            rc, msg = call(nx=256, ny=256, nz=257, P=1)
            assert rc == INVALID and "exceeds 4096 blocks of 4096 samples" in msg, msg
            for bad in (0, -3, 65536):
                rc, msg = call(weight=bad)
                assert rc == INVALID and "weight must be in 1..65535" in msg, (bad, msg)
            rc, msg = call(ws=False, ws_bytes=1 << 30)
            assert rc == WORKSPACE, msg
            query = "ls_tsdf_prior_rows" + ("" if single else "_batch") + "_workspace_bytes"
            need = getattr(lib, query)(*(() if single else (2,)), 4, 4, 4)
            rc, msg = call(ws_bytes=need - 1, weight=65535)
            assert rc == WORKSPACE and f"{need - 1} < required {need}" in msg and query in msg, msg
        call = functools.partial(_rows_call, lib, single)
        for bad in (0.0, -0.01, NAN, INF):
            rc, msg = call(voxel=[0.01, bad][-1:] if single else [0.01, bad])
            assert rc == INVALID and f"problem {last}" in msg and "voxel must be finite and > 0" in msg, (bad, msg)
        for bad in (NAN, INF, -INF):
            o = np.zeros((last + 1, 3))
            o[-1, 1] = bad
            rc, msg = call(origin=o)
            assert rc == INVALID and f"problem {last}" in msg and "origin must be finite" in msg, (bad, msg)
        rc, msg = call(null=("n",))
        assert rc == INVALID and "null n" in msg, msg
        rc, msg = call(null=("origin",))
        assert rc == INVALID and "null origin / voxel" in msg, msg
        rc, msg = call(null=("row_off",))
        assert rc == INVALID and "null row_off" in msg, msg
        for k in ("points", "row_inst", "row_index"):
            rc, msg = call(null=(k,))
            assert rc == INVALID and "come together" in msg, (k, msg)
        rc, msg = call(cap=-1)
        assert rc == INVALID and "negative capacity" in msg, msg
        rc, msg = call(null=("points", "row_inst", "row_index", "counts"), cap=0)      # a sizing call: only the workspace is short
        assert rc == WORKSPACE, msg
        call = functools.partial(_vote_call, lib, single)
        for bad in (0.0, -1.0, NAN, INF, -INF):
            rc, msg = call(s=[1.5, bad][-1:] if single else [1.5, bad])
            assert rc == INVALID and f"problem {last}" in msg and "s must be finite and > 0" in msg, (bad, msg)
            rc, msg = call(trunc=[0.04, bad][-1:] if single else [0.04, bad])
            assert rc == INVALID and f"problem {last}" in msg and "trunc must be finite and > 0" in msg, (bad, msg)
        for k in ("sum", "n"):
            rc, msg = call(null=(k,))
            assert rc == INVALID and "null sum / n" in msg, (k, msg)
        for k in ("sum_out", "n_out"):
            rc, msg = call(null=(k,))
            assert rc == INVALID and "null sum_out / n_out" in msg, (k, msg)
        rc, msg = call(null=("values",))
        assert rc == INVALID and "null values" in msg, msg
        rc, msg = call(null=("values",), rows=0)                                       # no row: the values may be null
        assert rc == WORKSPACE, msg
        rc, msg = call(rows=-1)
        assert rc == INVALID and "negative row count" in msg, msg
        rc, msg = call(null=("counts",))
        assert rc == INVALID and "null counts" in msg, msg
        rc, msg = call(alias=True)
        assert rc == INVALID and "separate pair" in msg, msg
    for fn in (_rows_call, _vote_call):
        for P in (0, -1):
            rc, msg = fn(lib, P=P)
            assert rc == INVALID and "P must be at least 1" in msg, msg
        rc, msg = fn(lib, P=65536, nx=1, ny=1, nz=1)
        assert rc == INVALID and "outside 1..65535" in msg, msg
    rc, msg = _rows_call(lib, null=("voxel",))
    assert rc == INVALID and "null origin / voxel" in msg, msg
    for k in ("s", "trunc"):
        rc, msg = _vote_call(lib, null=(k,))
        assert rc == INVALID and "null s / trunc" in msg, msg


def test_ops_refuse_on_the_host():
    import torch
    from livingscenes_amd import _lib, ops
    cpu = (torch.zeros(2, 2, 2, dtype=torch.int32), torch.zeros(2, 2, 2, dtype=torch.int32))
    with pytest.raises(_lib.LsError, match="no CPU fallback and converts nothing"):
        ops.tsdf_prior_rows(cpu, origin=np.zeros(3), voxel=0.1, weight=1)
    with pytest.raises(_lib.LsError, match="no CPU fallback and converts nothing"):
        ops.tsdf_complete(cpu, torch.zeros(0), (None, None, None, [0, 0], None), s=1.0, trunc=0.1, weight=1)
    with pytest.raises(ValueError, match="state is the pair"):
        ops.tsdf_prior_rows_batch(cpu[0], origin=np.zeros(3), voxel=0.1, weight=1)


# ------------------------------------------------------------------------------------------------ the capability, on the twins alone
def test_the_twins_close_the_sphere_that_the_cameras_left_open():
    """the inputs of tests/test_hip_tsdf_prior.py's capability test, reference only: the observed mesh has boundary edges; the
    completed mesh (weight 2, the exact sphere field) has none and no edge with more than two faces"""
    state, origin, h, trunc, centre, *_ = sphere_case()
    s, w0 = 1.3, 2
    vo, fo_ = fo.mesh(state, origin, h, 1)
    open_edges, _ = boundary_edges(fo_)
    assert len(fo_) > 100 and open_edges > 0 and (state[1] == 0).sum() > 1000
    r = tpo.rows(state, origin, h, w0)
    done, counts = tpo.vote(state, sphere_field(r["points"], centre, 0.3, s), s, trunc, w0)
    assert counts[2] == 0 and counts[1] == counts[0] > 0 and (done[1] >= w0).all()
    vc, fc = fo.mesh(done, origin, h, w0)
    assert boundary_edges(fc) == (0, 0) and len(fc) > len(fo_)
    err = np.abs(np.linalg.norm(vc - centre, axis=1) - 0.3)
    assert err.max() < h                                                         # a sphere, not a shell at the band's end
    # where no sample a vertex's cubes read received a vote (n >= 2 all around it), the vertex is the observed mesh's, bit for bit
    solid = least_seen_around(state[1], vc, origin, h) >= w0
    seen = {row.tobytes() for row in vo}
    assert solid.sum() > 50 and all(row.tobytes() in seen for row in vc[solid])
