"""CPU tests of the mesh metrics (csrc/meshmetrics.hip, livingscenes_amd/evaluate.py): the numpy restatement of check_mesh_contains
(tests/meshmetrics_oracle.py, which the GPU tests hold the device to) equals the reference's own output (tests/golden/mesh_contains.npz),
the new C entry points refuse bad arguments on the host before any launch, and PLY meshes round-trip through rscan."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meshmetrics_oracle as mo  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from livingscenes_amd import _lib, build
    build.build()
    return _lib.load()


def test_oracle_parity_equals_reference_fixture(golden):
    g = golden("mesh_contains")
    names = [str(n) for n in g["cases"]]
    assert set(names) == {"cube", "icosphere", "torus", "mcubes", "flat", "unreferenced"}
    for name in names:
        V, F, P, want = g[f"{name}_V"], g[f"{name}_F"], g[f"{name}_P"], g[f"{name}_inside"]
        got = mo.contains(V, F, P)
        assert np.array_equal(got, want), (name, int((got != want).sum()))
        if name == "flat":
            assert not want.any()
    # the hash only selects candidates: on these meshes the brute-force parity count agrees
    for name in ("cube", "icosphere", "torus"):
        assert np.array_equal(mo.contains(g[f"{name}_V"], g[f"{name}_F"], g[f"{name}_P"], brute=True), g[f"{name}_inside"]), name


def test_oracle_distance_and_sampler_basics():
    V, F = mo.cube()
    P = np.array([[0.5, 0.5, 0.5], [2.0, 0.5, 0.5], [0.5, 0.5, 1.25], [1.1, 1.1, 1.1]])
    d = mo.distance(V, F, P, 1.0)
    assert d[0] == 0.5 and d[1] == np.inf and d[2] == 0.25 and abs(d[3] - np.sqrt(3) * 0.1) < 1e-15
    # a degenerate (collinear) triangle is its longest edge
    a, b, c = np.zeros(3), np.array([1.0, 0, 0]), np.array([2.0, 0, 0])
    assert abs(mo.point_triangle_d2(np.array([1.5, 1.0, 0]), a, b, c) - 1.0) < 1e-15
    assert abs(mo.point_triangle_d2(np.array([3.0, 0, 0]), a, a, a) - 9.0) < 1e-15
    u = mo.uniforms(7, np.arange(100000, dtype=np.uint64))
    assert u.min() >= 0 and u.max() < 1 and abs(u.mean() - 0.5) < 0.01
    pts, face, _, _ = mo.sample(V, F, 1000, seed=3)
    assert face.min() >= 0 and face.max() < len(F)
    assert np.all(mo.distance(V, F, pts, 0.1) < 1e-15)


def test_mesh_entry_points_validate_arguments_without_device(lib):
    P = ctypes.c_void_p
    ws = lib.ls_mesh_contains_workspace_bytes(100, 512)
    assert ws > 0 and lib.ls_mesh_contains_workspace_bytes(100, 1) == 0 and lib.ls_mesh_contains_workspace_bytes(-1, 512) == 0
    # nf >= 0, hash resolution range, non-null arrays when n > 0, workspace size
    assert lib.ls_mesh_contains_f64(P(16), 8, P(16), -1, P(16), 10, 512, P(16), P(16), 10, P(16), P(16), ws, None) == -1
    assert b"negative" in lib.ls_last_error()
    assert lib.ls_mesh_contains_f64(P(16), 8, P(16), 100, P(16), 10, 1, P(16), P(16), 10, P(16), P(16), ws, None) == -1
    assert b"hash_resolution" in lib.ls_last_error()
    assert lib.ls_mesh_contains_f64(None, 8, P(16), 100, P(16), 10, 512, P(16), P(16), 10, P(16), P(16), ws, None) == -1
    assert lib.ls_mesh_contains_f64(P(16), 8, P(16), 100, None, 10, 512, P(16), P(16), 10, P(16), P(16), ws, None) == -1
    assert lib.ls_mesh_contains_f64(P(16), 8, P(16), 100, P(16), 10, 512, P(16), P(16), 10, None, P(16), ws, None) == -1
    assert lib.ls_mesh_contains_f64(P(16), 8, P(16), 100, P(16), 10, 512, P(16), P(16), 10, P(16), P(16), ws - 1, None) == -3
    assert b"workspace" in lib.ls_last_error()
    dws = lib.ls_mesh_distance_workspace_bytes(100)
    assert dws > 0
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert lib.ls_mesh_distance_f64(P(16), 8, P(16), 100, P(16), 10, bad, P(16), P(16), 10, P(16), P(16), dws, None) == -1
        assert b"max_dist" in lib.ls_last_error()
    assert lib.ls_mesh_distance_f64(P(16), 8, P(16), 100, P(16), 10, 0.1, None, P(16), 10, P(16), P(16), dws, None) == -1
    assert lib.ls_mesh_distance_f64(P(16), 8, P(16), 100, P(16), 10, 0.1, P(16), P(16), 10, P(16), None, 0, None) == -3
    sws = lib.ls_mesh_sample_workspace_bytes(100)
    assert sws > 0
    assert lib.ls_mesh_sample_f64(P(16), 8, P(16), 100, 0, 1, P(16), None, P(16), sws, None) == -1
    assert b"count" in lib.ls_last_error()
    assert lib.ls_mesh_sample_f64(P(16), 8, P(16), 0, 10, 1, P(16), None, P(16), sws, None) == -1
    assert lib.ls_mesh_sample_f64(P(16), 8, P(16), 100, 10, 1, None, None, P(16), sws, None) == -1
    assert lib.ls_mesh_sample_f64(P(16), 8, P(16), 100, 10, 1, P(16), None, P(16), sws - 1, None) == -3


def test_python_metrics_refuse_cpu_and_bad_meshes():
    import torch
    from livingscenes_amd import _lib, evaluate, ops
    V, F = mo.cube()
    with pytest.raises(_lib.LsError):
        ops.mesh_contains(torch.from_numpy(V), torch.from_numpy(F.astype(np.int32)), torch.zeros(4, 3, dtype=torch.float64))
    with pytest.raises(_lib.LsError, match="float64"):
        ops.mesh_distance(torch.from_numpy(V).float(), torch.from_numpy(F.astype(np.int32)), torch.zeros(4, 3, dtype=torch.float64), 0.1)
    assert evaluate.get_threshold_percentage(np.array([0.1, 0.2, 0.3, 0.4]), [0.2, 0.35]) == [0.5, 0.75]


@pytest.mark.parametrize("binary", ["little", "big", None])
@pytest.mark.parametrize("face_types", [("uchar", "int"), ("uint8", "uint32")])
def test_ply_mesh_roundtrip(tmp_path, binary, face_types):
    from livingscenes_amd import rscan
    V, F = mo.icosphere(1)
    V = V * 1.7 + [10.0, -7.0, 3.0]
    p = str(tmp_path / "m.ply")
    rscan.write_ply_mesh(p, V, F, binary=binary, face_types=face_types)
    v, f = rscan.load_ply_mesh(p)
    assert v.dtype == np.float64 and f.dtype == np.int64
    assert np.array_equal(v, V) and np.array_equal(f, F)
    assert np.allclose(rscan.load_ply_vertices(p), V.astype(np.float32))


def test_ply_mesh_extra_properties_and_polygons(tmp_path):
    """float vertices with colours, a face property after the index list, a quad (split into a fan), big-endian"""
    from livingscenes_amd import rscan
    V = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    hdr = ("ply\nformat binary_big_endian 1.0\nelement vertex 5\nproperty float x\nproperty float y\nproperty float z\n"
           "property uchar red\nelement face 2\nproperty list uchar int vertex_indices\nproperty uchar flags\nend_header\n")
    body = b"".join(v.astype(">f4").tobytes() + b"\x07" for v in V)
    body += np.array([4], ">u1").tobytes() + np.array([0, 1, 2, 3], ">i4").tobytes() + b"\x01"
    body += np.array([3], ">u1").tobytes() + np.array([0, 1, 4], ">i4").tobytes() + b"\x02"
    p = tmp_path / "q.ply"
    p.write_bytes(hdr.encode() + body)
    v, f = rscan.load_ply_mesh(str(p))
    assert np.array_equal(v, V.astype(np.float64))
    assert f.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 4]]
    a = tmp_path / "a.ply"
    a.write_text("ply\nformat ascii 1.0\nelement vertex 5\nproperty float x\nproperty float y\nproperty float z\n"
                 "element face 2\nproperty list uchar int vertex_indices\nend_header\n"
                 + "".join(" ".join(str(c) for c in r) + "\n" for r in V.tolist()) + "4 0 1 2 3\n3 0 1 4\n")
    v, f = rscan.load_ply_mesh(str(a))
    assert np.array_equal(v, V.astype(np.float64)) and f.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 4]]
