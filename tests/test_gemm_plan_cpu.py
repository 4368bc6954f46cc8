"""Which GEMM kernel runs a problem, and on what grid, is decided by one pure host function (csrc/gemm_plan.h).  The wide, the tiled and the
persistent kernels agree to the bit, so no numerical test notices a changed choice; this one does: the plan, compiled on its own with the host
compiler, must name the kernel, the grid and the workgroup size of every launch in tests/golden/gemm_launches.json -- a kernel trace recorded from
the library as it was before the dispatch code became this function (tests/tools/record_gemm_launches.py), in all three arithmetic modes.
No GPU needed."""
import importlib.util
import os
import subprocess

import pytest

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FIELDS = ("M", "N", "K", "lda", "ldw", "pieces", "gather", "masked", "may_split", "latency", "has_planes", "wants_out_rowmax", "C", "npts", "has_G_or_cs",
          "a_parts", "has_a_rowmax", "has_w_rowmax")


def recorder():
    spec = importlib.util.spec_from_file_location("record_gemm_launches", os.path.join(REPO, "tests", "tools", "record_gemm_launches.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def record():
    return recorder().load()


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gemm_plan") / "gemm_plan_dump")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(REPO, "livingscenes_amd", "csrc"),
                    os.path.join(REPO, "tests", "tools", "gemm_plan_dump.cpp"), "-o", exe], check=True)
    return exe


def test_the_record_lists_the_ladder(record):
    rec = recorder()
    want = {f"{mode}:{key}" for mode in rec.MODES for key, _, _ in rec.cases_of(mode)}
    assert want == set(record), "the ladder and the record list different cases: re-record (see the recorder's docstring)"


def test_the_plan_names_every_recorded_launch(record, dump):
    rec = recorder()
    traits = {f"{mode}:{key}": tr for mode in rec.MODES for key, tr, _ in rec.cases_of(mode)}     # (None: the tool cannot state them)
    keys = sorted(k for k, v in record.items() if v["status"] == 0 and traits[k] is not None)
    lines, owner = [], []
    for k in keys:
        mode = rec.MODES.index(k.split(":", 1)[0])
        for t in traits[k]:
            lines.append(" ".join(str(int(v)) for v in [mode, t["form"] == "vn"] + [t.get(f, 0) for f in FIELDS]))
            owner.append(k)
    out = subprocess.run([dump], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(lines)
    planned = {k: [] for k in keys}
    for k, line in zip(owner, out):
        for launch in line.split(";"):
            name, gx, gy, block = launch.split("|")
            planned[k].append([name, [int(gx) * int(block), int(gy), 1], [int(block), 1, 1]])
    wrong = {k: (planned[k], [l[:3] for l in record[k]["launches"]]) for k in keys if planned[k] != [l[:3] for l in record[k]["launches"]]}
    assert not wrong, f"{len(wrong)} of {len(keys)} cases: the plan differs from the recorded launches (planned, recorded): {dict(list(wrong.items())[:4])}"
    # every kernel family and every arithmetic mode is in the comparison, and so are the refusals' neighbours
    names = {l[0] for k in keys for l in record[k]["launches"]}
    for family in ("gemm_f32_kernel<false", "gemm_f32_kernel<true, 3>", "gemm_f32_kernel<true, 2>", "gemm_f32_kernel<true, 22>", "gemm_h2_kernel<true, true>",
                   "gemm_h2_kernel<false, false>", "gemm_w2_kernel<false, false>", "gemm_w2_kernel<true, true>", "gemm_smallk_kernel<32, true>", "gemm_h2_smallk_kernel<64, true>",
                   "gemm_splitk_reduce_kernel", "gemm_vn_direct_kernel", "gemm_vn_smallk_kernel", "gemm_vn_kernel"):
        assert any(family in n for n in names), family
    assert {k.split(":", 1)[0] for k in keys} == set(rec.MODES)
