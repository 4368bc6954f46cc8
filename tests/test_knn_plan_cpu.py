"""What a k-NN build launches -- which kernel of knn.hip / knn_mfma.hip / knn_xyz.hip on what grid, the image launches in front of the fused
kernel, the merge behind a split tile kernel, the scratch -- is decided by one pure host function (csrc/knn_plan.h).  Every path is bit-exact
against the oracle, so no numerical test notices a changed choice; this one does: the plan, compiled on its own with the host compiler, must name
the kernel with its template arguments, the grid and the workgroup size of every launch of every case in tests/golden/knn_launches.json -- a
kernel trace recorded from the library as it was before the family's dispatch code became this function (tests/tools/record_gemm_launches.py
--family knn; tests/test_hip_parity.py holds the same cases to the oracle and to the recorded hashes).  No GPU needed."""
import importlib.util
import itertools
import os
import subprocess
import sys

import pytest

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TOOLS = os.path.join(REPO, "tests", "tools")
FIELDS = ("B", "Nd", "dst_n", "Ns", "C", "K", "fma", "valu_only", "seeded", "self", "has_scratch")
# KnnKernel enumerator -> the main launch's kernel, FMA aside
ENUMERATORS = {"XYZ_SINGLE": "ls::knn_xyz_kernel<{f}, true>", "XYZ_CHUNKED": "ls::knn_xyz_kernel<{f}, false>", "SMALL": "ls::knn_small_kernel<{f}>",
               "TILE": "ls::knn_kernel<32, {f}>", "FUSED_32_T1": "ls::knn_fused_kernel<32, {f}, 1>", "FUSED_32_T2": "ls::knn_fused_kernel<32, {f}, 2>",
               "FUSED_32_T4": "ls::knn_fused_kernel<32, {f}, 4>", "FUSED_64_T1": "ls::knn_fused_kernel<64, {f}, 1>", "FUSED_64_T2": "ls::knn_fused_kernel<64, {f}, 2>",
               "FUSED_64_T4": "ls::knn_fused_kernel<64, {f}, 4>"}
SIDE = ("ls::knn_prep_f16_tile_kernel<6, 3>", "ls::knn_prep_f16_tile_kernel<12, 4>", "ls::knn_merge_kernel")


def _tool(name):
    if TOOLS not in sys.path:
        sys.path.insert(0, TOOLS)
    spec = importlib.util.spec_from_file_location(name, os.path.join(TOOLS, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def rec():
    return _tool("record_gemm_launches")


@pytest.fixture(scope="module")
def record(rec):
    return rec.load("knn")


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    """[KnnTraits dict] -> [dict(launches [[name, grid, workgroup]] as the trace reports them, kernel, splits, tiles_per_split, ns_pad, tpw, stats,
    scratch_bytes, used_bytes)]"""
    exe = str(tmp_path_factory.mktemp("knn_plan") / "knn_plan_dump")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(REPO, "livingscenes_amd", "csrc"),
                    os.path.join(TOOLS, "knn_plan_dump.cpp"), "-o", exe], check=True)

    def run(traits):
        lines = [" ".join(str(int(t[f])) for f in FIELDS) for t in traits]
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(lines)
        res = []
        for line in out:
            launches, side = line.split(" # ")
            side = side.split()
            r = dict(zip(("splits", "tiles_per_split", "ns_pad", "tpw", "stats", "scratch_bytes", "used_bytes"), (int(v) for v in side[1:])), kernel=side[0])
            r["launches"] = [[n, [int(g) * int(b), 1, 1], [int(b), 1, 1]] for n, g, b in (l.split("|") for l in launches.split(";"))]
            res.append(r)
        return res
    return run


def test_the_record_lists_the_ladder(rec, record):
    want = {f"{rec.MODES[0]}:{key}" for key, _ in rec.knn_ladder()}
    assert want == set(record), "the ladder and the record list different cases: re-record (see the recorder's docstring)"
    assert all(v["sha256"] and v["status"] == 0 for v in record.values()), "two recordings from the library before the plan agreed on every case"


def test_the_plan_names_every_recorded_launch(rec, record, plan):
    cases = rec.knn_ladder()
    keys = [f"{rec.MODES[0]}:{key}" for key, _ in cases]
    planned = dict(zip(keys, plan([rec.knn_traits(c) for _, c in cases])))
    # the whole sequence in order: the image launches, the kernel, the merge
    wrong = {k: (planned[k]["launches"], record[k]["launches"]) for k in keys if planned[k]["launches"] != [l[:3] for l in record[k]["launches"]]}
    assert not wrong, f"{len(wrong)} of {len(keys)} cases: the plan differs from the recorded launches (planned, recorded): {dict(list(wrong.items())[:4])}"
    # the enumerator list and the record cover each other, with and without FMA
    names = {l[0] for k in keys for l in record[k]["launches"]}
    mains = {n.format(f=f) for n in ENUMERATORS.values() for f in ("false", "true")}
    assert names == mains | set(SIDE), (names - mains - set(SIDE), (mains | set(SIDE)) - names)
    for k in keys:
        assert ENUMERATORS[planned[k]["kernel"]].format(f="true" if "contract=1" in k else "false") in {l[0] for l in record[k]["launches"]}, k
    # where ops.knn brings no scratch (the sizing call asks for none), having one would change nothing
    bare = [(k, c) for k, (_, c) in zip(keys, cases) if planned[k]["scratch_bytes"] == 0]
    assert len(bare) > 10
    for (k, _), p in zip(bare, plan([rec.knn_traits(c, has_scratch=0) for _, c in bare])):
        assert p == planned[k], k


def test_the_odd_rules_of_the_choice(plan):
    """Stated in comments of knn_plan.h; kept, not tidied away."""
    t = lambda **kw: dict(dict(B=2, Nd=32, dst_n=32, Ns=128, C=32, K=16, fma=0, valu_only=0, seeded=0, self=0, has_scratch=1), **kw)
    got = [p["kernel"] for p in plan([t(seeded=1), t(), t(seeded=1, C=64), t(C=64), t(seeded=1, has_scratch=0), t(Nd=33, dst_n=33, has_scratch=0),
                                      t(Nd=33, dst_n=33, Ns=1025, has_scratch=0), t(seeded=1, valu_only=1)])]
    assert got == ["FUSED_32_T1", "SMALL", "FUSED_64_T1", "SMALL", "SMALL", "TILE", "TILE", "SMALL"]
    split, bare = plan([t(Nd=33, dst_n=33, Ns=1025), t(Nd=33, dst_n=33, Ns=1025, has_scratch=0)])
    assert (split["splits"], split["tiles_per_split"], len(split["launches"])) == (9, 2, 2) and (bare["splits"], bare["tiles_per_split"], len(bare["launches"])) == (1, 17, 1)
    # the sizing ignores Nd <= 32: an un-seeded 32-query call is sized for the fused kernel and runs the small one
    assert plan([t()])[0]["scratch_bytes"] == plan([t(seeded=1)])[0]["scratch_bytes"] > 0


def test_plan_invariants_over_the_ladders_values_crossed(plan):
    Bs, Nds, Cs = (1, 2, 255, 256), (7, 32, 33, 70, 128), (1, 32, 64, 96, 128, 256)
    Nss = (32, 64, 65, 128, 130, 256, 257, 512, 513, 1024, 1025, 1100)
    traits = [dict(B=B, Nd=Nd, dst_n=Ns if self else Nd, Ns=Ns, C=C, K=16, fma=0, valu_only=vo, seeded=sd, self=self, has_scratch=hs)
              for B, Nd, Ns, C, hs, sd, vo, self in itertools.product(Bs, Nds, Nss, Cs, (0, 1), (0, 1), (0, 1), (0, 1))]
    assert len(traits) > 10 ** 4
    res = plan(traits)
    bytes_of, seen = {}, set()
    for t, p in zip(traits, res):
        fused, tile = p["kernel"].startswith("FUSED"), p["kernel"] == "TILE"
        seen.add(p["kernel"])
        if tile:
            assert p["splits"] * p["tiles_per_split"] * 64 >= t["Ns"] > (p["splits"] - 1) * p["tiles_per_split"] * 64, (t, p)
        assert (p["launches"][-1][0] == "ls::knn_merge_kernel") == (p["splits"] > 1) and (tile or p["splits"] == 1), (t, p)
        if fused:
            assert t["C"] in (32, 64) and p["ns_pad"] <= 1024 and p["tpw"] * 8 * 32 >= p["ns_pad"] >= t["Ns"] and p["tpw"] in (1, 2, 4), (t, p)
            assert len(p["launches"]) == (2 if t["self"] else 3), (t, p)
        assert p["stats"] == int(fused), (t, p)
        assert p["scratch_bytes"] >= p["used_bytes"], (t, p)
        if not t["has_scratch"]:
            assert not fused and p["splits"] == 1 and p["used_bytes"] == 0, (t, p)
        # one size per shape and flags: hints and the scratch itself do not move it
        key = tuple(t[f] for f in ("B", "Nd", "dst_n", "Ns", "C", "valu_only", "self"))
        assert bytes_of.setdefault(key, p["scratch_bytes"]) == p["scratch_bytes"], (t, p)
    assert seen == set(ENUMERATORS)
