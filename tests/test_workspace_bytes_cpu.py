"""The sizes the ls_*_workspace_bytes / ls_*_state_bytes queries report are the library's contract with its callers: every model-free query on
the ladder of tests/tools/record_workspace_bytes.py must answer what tests/golden/workspace_bytes.json holds -- recorded from the library as
it was before the operators' private workspace cutters were replaced by ls::Arena (csrc/ls_workspace.h).  Host arithmetic: no GPU needed.
(The queries that need a model handle: tests/test_hip_workspace.py.)"""
import importlib.util
import json
import os

import pytest

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def recorder():
    spec = importlib.util.spec_from_file_location("record_workspace_bytes", os.path.join(REPO, "tests", "tools", "record_workspace_bytes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def lib():
    from livingscenes_amd import _lib, build
    build.build()
    return _lib.load()


def test_model_free_workspace_sizes_are_the_recorded_ones(lib):
    rec = recorder()
    with open(os.path.join(rec.GOLDEN, "workspace_bytes.json")) as f:
        want = json.load(f)
    cases = rec.ladder()
    assert {rec.key(n, a) for n, a in cases} == set(want), "the ladder and the record list different cases: re-record (see the recorder's docstring)"
    got = {rec.key(n, a): int(getattr(lib, n)(*a)) for n, a in cases}
    wrong = {k: (want[k], got[k]) for k in want if got[k] != want[k]}
    assert not wrong, f"{len(wrong)} sizes differ from the record (recorded, now): {dict(list(wrong.items())[:8])}"
    # every query of the ladder is exercised with arguments it sizes and with arguments it refuses (the ICP and single marching-cubes queries
    # refuse nothing: a constant, and 256 bytes for a volume without a cube)
    for name in {n for n, _ in cases} - {"ls_icp_workspace_bytes", "ls_mcubes_workspace_bytes"}:
        vals = [want[rec.key(n, a)] for n, a in cases if n == name]
        assert any(v > 0 for v in vals) and any(v == 0 for v in vals), name
    assert all(v % 256 == 0 for k, v in want.items() if k.startswith(("ls_mesh_", "ls_reg_", "ls_mise_", "ls_mcubes_", "ls_fps_")))
