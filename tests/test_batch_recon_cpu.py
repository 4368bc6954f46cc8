"""Host side of the batched reconstruction leg, without a GPU: the thread-pool decimation (mesh_extractor2.simplify_mesh_arrays_batch)
against serial simplify_mesh_arrays on the inputs of tests/golden/simplify.npz, its default thread count, and the C ABI of the ragged
mesh metrics (ls_mesh_*_batch_f64: version, symbols, workspace helpers)."""
import numpy as np
import pytest

from livingscenes_amd import _lib, mesh_extractor2


def _inputs(g):
    return [(g[n + "_v"], g[n + "_f"]) for n in ("sphere", "torus", "open_sheet", "flat")]


@pytest.mark.parametrize("threads", [1, 4])
def test_simplify_batch_equals_serial(golden, threads):
    meshes = _inputs(golden("simplify"))
    for target, agg in ((150, 5.0), (400, 7.0)):
        serial = [mesh_extractor2.simplify_mesh_arrays(v, f, target, agg) for v, f in meshes]
        # every mesh twice: more meshes than threads, and the same input decimated on two workers at once
        got = mesh_extractor2.simplify_mesh_arrays_batch(meshes + meshes, target, agg, threads=threads)
        assert len(got) == 2 * len(meshes)
        for (v, f), (vs, fs) in zip(got, serial + serial):
            assert v.dtype == np.float64 and f.dtype == np.int64
            assert np.array_equal(v, vs) and np.array_equal(f, fs)


def test_simplify_batch_takes_mesh_objects_and_empty_list(golden):
    v, f = _inputs(golden("simplify"))[1]
    got = mesh_extractor2.simplify_mesh_arrays_batch([mesh_extractor2.SimpleMesh(v, f)], 200, 5.0, threads=2)
    want = mesh_extractor2.simplify_mesh_arrays(v, f, 200, 5.0)
    assert np.array_equal(got[0][0], want[0]) and np.array_equal(got[0][1], want[1])
    assert mesh_extractor2.simplify_mesh_arrays_batch([], 200) == []
    with pytest.raises(ValueError):
        mesh_extractor2.simplify_mesh_arrays_batch([(v, f)], 200, threads=0)


def test_default_threads_follows_omp_num_threads(monkeypatch):
    import os
    monkeypatch.setenv("OMP_NUM_THREADS", "3")
    assert mesh_extractor2.default_threads() == 3
    monkeypatch.setenv("OMP_NUM_THREADS", "24")
    assert mesh_extractor2.default_threads() == 24
    monkeypatch.delenv("OMP_NUM_THREADS")
    assert mesh_extractor2.default_threads() == min(16, len(os.sched_getaffinity(0)))


def test_abi_107_exports_batch_metrics():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 107 and lib.ls_version() == 107
    for name in ("ls_mesh_contains_batch_f64", "ls_mesh_distance_batch_f64", "ls_mesh_sample_batch_f64",
                 "ls_mesh_contains_batch_workspace_bytes", "ls_mesh_distance_batch_workspace_bytes", "ls_mesh_sample_batch_workspace_bytes"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES


def test_batch_workspace_helpers():
    lib = _lib.load()
    # invalid arguments -> 0
    for M, nf, R in ((-1, 10, 512), (2, -1, 512), (2, 2 ** 31, 512), (2, 10, 1), (2, 10, 4097)):
        assert lib.ls_mesh_contains_batch_workspace_bytes(M, nf, R) == 0
    for M, nf in ((-1, 10), (2, -1), (2, 2 ** 31)):
        assert lib.ls_mesh_distance_batch_workspace_bytes(M, nf) == 0
        assert lib.ls_mesh_sample_batch_workspace_bytes(M, nf) == 0
    # valid: grows with M and with the faces; contains holds R^2 cells per mesh, distance at most 8 nf_total + M cells
    c1, c2 = lib.ls_mesh_contains_batch_workspace_bytes(1, 1000, 64), lib.ls_mesh_contains_batch_workspace_bytes(2, 1000, 64)
    assert 0 < c1 < c2 and c2 - c1 >= 64 * 64 * (4 + 8)
    d = [lib.ls_mesh_distance_batch_workspace_bytes(4, nf) for nf in (0, 1000, 100000)]
    assert 0 < d[0] < d[1] < d[2]
    assert d[2] < lib.ls_mesh_distance_workspace_bytes(100000) * 4      # not M x 128^3
    s = [lib.ls_mesh_sample_batch_workspace_bytes(M, 5000) for M in (1, 8)]
    assert 0 < s[0] < s[1]
