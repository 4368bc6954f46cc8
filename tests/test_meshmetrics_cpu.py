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


# ---- the workspace sizes are part of the C contract: pinned to the values of the first release of these operators
WS_NF = (0, 1, 100, 4096, 4097, 10 ** 6, -1)      # -1: rejected (0 bytes)
WS_R = (2, 64, 512, 4096, 1, 4097)                # 1, 4097: rejected
WS_M = (0, 1, 5, 128, -1)                         # -1: rejected
WS_DISTANCE = (  # [nf]
    25170176, 25170688, 25180160, 25563392, 25563904, 121170176, 0,
)
WS_SAMPLE = (  # [nf]
    0, 768, 2304, 65792, 66304, 16002048, 0,
)
WS_CONTAINS = (  # [nf][R]
    1024, 49664, 3146496, 201359616, 0, 0,
    1536, 50176, 3147008, 201360128, 0, 0,
    10240, 58880, 3155712, 201368832, 0, 0,
    361472, 410112, 3506944, 201720064, 0, 0,
    361984, 410624, 3507456, 201720576, 0, 0,
    88001024, 88049664, 91146496, 289359616, 0, 0,
    0, 0, 0, 0, 0, 0,
)
WS_DISTANCE_BATCH = (  # [nf][M]
    256, 1280, 2048, 30720, 0,
    1536, 1792, 2560, 31744, 0,
    20224, 20736, 21504, 50432, 0,
    786944, 787712, 788480, 817152, 0,
    787968, 788224, 788992, 818176, 0,
    192016128, 192016896, 192017664, 192046336, 0,
    0, 0, 0, 0, 0,
)
WS_SAMPLE_BATCH = (  # [nf][M]
    256, 512, 512, 6400, 0,
    1024, 1024, 1024, 7168, 0,
    2560, 2560, 2560, 8704, 0,
    66048, 66048, 66048, 72192, 0,
    66560, 66560, 66560, 72704, 0,
    16002304, 16002304, 16002304, 16008448, 0,
    0, 0, 0, 0, 0,
)
WS_CONTAINS_BATCH = (  # [nf][M][R]
    256, 256, 256, 256, 0, 0,
    1280, 49920, 3146752, 201359872, 0, 0,
    2048, 247296, 15732480, 1006798080, 0, 0,
    35328, 6321408, 402747648, 25774027008, 0, 0,
    0, 0, 0, 0, 0, 0,
    768, 768, 768, 768, 0, 0,
    1792, 50432, 3147264, 201360384, 0, 0,
    2560, 247808, 15732992, 1006798592, 0, 0,
    35840, 6321920, 402748160, 25774027520, 0, 0,
    0, 0, 0, 0, 0, 0,
    9472, 9472, 9472, 9472, 0, 0,
    10496, 59136, 3155968, 201369088, 0, 0,
    11264, 256512, 15741696, 1006807296, 0, 0,
    44544, 6330624, 402756864, 25774036224, 0, 0,
    0, 0, 0, 0, 0, 0,
    360704, 360704, 360704, 360704, 0, 0,
    361728, 410368, 3507200, 201720320, 0, 0,
    362496, 607744, 16092928, 1007158528, 0, 0,
    395776, 6681856, 403108096, 25774387456, 0, 0,
    0, 0, 0, 0, 0, 0,
    361216, 361216, 361216, 361216, 0, 0,
    362240, 410880, 3507712, 201720832, 0, 0,
    363008, 608256, 16093440, 1007159040, 0, 0,
    396288, 6682368, 403108608, 25774387968, 0, 0,
    0, 0, 0, 0, 0, 0,
    88000256, 88000256, 88000256, 88000256, 0, 0,
    88001280, 88049920, 91146752, 289359872, 0, 0,
    88002048, 88247296, 103732480, 1094798080, 0, 0,
    88035328, 94321408, 490747648, 25862027008, 0, 0,
    0, 0, 0, 0, 0, 0,
    0, 0, 0, 0, 0, 0,
    0, 0, 0, 0, 0, 0,
    0, 0, 0, 0, 0, 0,
    0, 0, 0, 0, 0, 0,
    0, 0, 0, 0, 0, 0,
)


def test_mesh_workspace_sizes_are_pinned(lib):
    it = {k: iter(v) for k, v in (("d", WS_DISTANCE), ("s", WS_SAMPLE), ("c", WS_CONTAINS), ("db", WS_DISTANCE_BATCH), ("sb", WS_SAMPLE_BATCH),
                                  ("cb", WS_CONTAINS_BATCH))}
    for nf in WS_NF:
        assert lib.ls_mesh_distance_workspace_bytes(nf) == next(it["d"]), nf
        assert lib.ls_mesh_sample_workspace_bytes(nf) == next(it["s"]), nf
        for R in WS_R:
            assert lib.ls_mesh_contains_workspace_bytes(nf, R) == next(it["c"]), (nf, R)
        for M in WS_M:
            assert lib.ls_mesh_distance_batch_workspace_bytes(M, nf) == next(it["db"]), (M, nf)
            assert lib.ls_mesh_sample_batch_workspace_bytes(M, nf) == next(it["sb"]), (M, nf)
            for R in WS_R:
                assert lib.ls_mesh_contains_batch_workspace_bytes(M, nf, R) == next(it["cb"]), (M, nf, R)
    assert all(next(i, None) is None for i in it.values())
    # every rejected argument gives 0, every accepted one a multiple of 256
    for (nf, R), b in zip([(nf, R) for nf in WS_NF for R in WS_R], WS_CONTAINS):
        assert (b == 0) == (nf < 0 or R in (1, 4097)) and b % 256 == 0


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
