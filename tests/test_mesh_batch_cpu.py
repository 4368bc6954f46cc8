"""Host side of the batched MISE octrees and the batched marching cubes, without a GPU: the C ABI of the *_batch ops (symbols, size queries,
and the argument checks, which run before the first HIP call)."""
import ctypes
import os

import numpy as np
import pytest

from livingscenes_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "livingscenes_hip.h")
SYMBOLS = {"ls_mise_batch_state_bytes": "size_t", "ls_mise_init_batch": "int", "ls_mise_query_batch": "int", "ls_mise_update_batch": "int",
           "ls_mise_to_dense_batch": "int", "ls_mcubes_batch_workspace_bytes": "size_t", "ls_marching_cubes_batch_f64": "int"}
INVALID, WORKSPACE = -1, -3


def _hp(a):
    return ctypes.c_void_p(a.ctypes.data)


def _refused(rc, *words):
    msg = _lib.load().ls_last_error().decode()
    return rc == INVALID and all(w in msg for w in words), (rc, msg)


def test_abi_exports_the_mesh_batch_ops_and_keeps_its_version():
    lib = _lib.load()
    header = open(HEADER).read()
    for name, res in SYMBOLS.items():
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
        assert f"{res} {name}(" in header, name
    assert lib.ls_version() == 107 == _lib.ABI_VERSION      # added symbols only: the argument layouts of the existing ones are unchanged


def test_mise_batch_state_is_b_single_states_and_the_block_sums():
    lib = _lib.load()
    one = lib.ls_mise_state_bytes(4, 2)
    assert one % 256 == 0
    for B in (1, 2, 520):
        n = lib.ls_mise_batch_state_bytes(B, 4, 2)
        nblk = -(-17 ** 3 // 4096)
        assert n % 256 == 0 and B * one + (B * nblk + 1) * 4 <= n < B * one + (B * nblk + 1) * 4 + 256
    for B, res0, depth in ((0, 4, 2), (-1, 4, 2), (65536, 1, 0), (2, 0, 2), (2, 4, 8), (2, 2048, 0)):
        assert lib.ls_mise_batch_state_bytes(B, res0, depth) == 0, (B, res0, depth)
    # B * (R+1)^3 < 2^31: 129^3 = 2 146 689 lattice points
    assert lib.ls_mise_batch_state_bytes(1000, 32, 2) > 0 and lib.ls_mise_batch_state_bytes(1001, 32, 2) == 0


def test_mcubes_batch_workspace_query():
    q = _lib.load().ls_mcubes_batch_workspace_bytes
    for B, nx, ny, nz in ((0, 8, 8, 8), (-3, 8, 8, 8), (2, 0, 8, 8), (2, 8, -1, 8), (2, 8, 8, 0), (65536, 2, 2, 2)):
        assert q(B, nx, ny, nz) == 0, (B, nx, ny, nz)
    assert 0 < q(1, 8, 8, 8) < q(2, 8, 8, 8) < q(64, 8, 8, 8)
    assert q(3, 1, 8, 8) > 0                                  # volumes without a cube: empty meshes, still a valid call
    # 15 * B * nx*ny*nz < 2^31: 131^3 = 2 248 091 samples -> B <= 63
    assert q(63, 131, 131, 131) > 0 and q(64, 131, 131, 131) == 0
    assert q(1, 523, 523, 523) > 0 and q(1, 524, 524, 524) == 0


def test_mise_batch_entry_points_check_their_arguments_before_the_device():
    lib = _lib.load()
    buf = np.zeros(1 << 12, np.uint8)
    p = _hp(buf)
    big = lib.ls_mise_batch_state_bytes(2, 4, 2)
    assert lib.ls_mise_init_batch(None, big, 2, 4, 2, None) == INVALID
    for B in (0, 65536):
        ok, why = _refused(lib.ls_mise_init_batch(p, 1 << 40, B, 4, 2, None), "B=")
        assert ok, why
    ok, why = _refused(lib.ls_mise_init_batch(p, 1 << 40, 1001, 32, 2, None), "2^31")
    assert ok, why
    assert lib.ls_mise_init_batch(p, 1 << 40, 2, 4, 9, None) == INVALID
    assert lib.ls_mise_init_batch(p, 2 * lib.ls_mise_state_bytes(4, 2), 2, 4, 2, None) == WORKSPACE      # the block sums are part of the state
    assert "batch state" in lib.ls_last_error().decode()

    query = lambda *a: lib.ls_mise_query_batch(*a, None)
    for missing in range(5):
        a = [p, 2, 4, 2, 1.1, p, p, p, 100, p]
        a[(0, 5, 6, 7, 9)[missing]] = None
        assert query(*a) == INVALID, missing
    assert query(p, 2, 4, 2, 1.1, p, p, p, -1, p) == INVALID
    ok, why = _refused(query(p, 0, 4, 2, 1.1, p, p, p, 100, p), "B=0")
    assert ok, why
    ok, why = _refused(query(p, 1001, 32, 2, 1.1, p, p, p, 100, p), "2^31")
    assert ok, why

    update = lambda *a: lib.ls_mise_update_batch(*a, None)
    assert update(None, 2, 4, 2, 0.0, p, p, p, 10) == INVALID
    for missing in (5, 6, 7):
        a = [p, 2, 4, 2, 0.0, p, p, p, 10]
        a[missing] = None
        assert update(*a) == INVALID, missing
    assert update(p, 2, 4, 2, 0.0, p, p, p, -1) == INVALID
    assert update(p, 65536, 4, 2, 0.0, p, p, p, 10) == INVALID
    ok, why = _refused(update(p, 2, 4, 2, 0.0, p, p, p, 2 * 17 ** 3 + 1), "values for 2 octrees")
    assert ok, why

    dense = lambda *a: lib.ls_mise_to_dense_batch(*a, None)
    assert dense(None, 2, 4, 2, p) == INVALID and dense(p, 2, 4, 2, None) == INVALID
    assert dense(p, 0, 4, 2, p) == INVALID and dense(p, 65536, 4, 2, p) == INVALID and dense(p, 2, 0, 2, p) == INVALID


def test_marching_cubes_batch_checks_its_arguments_before_the_device():
    lib = _lib.load()
    buf = np.zeros(1 << 12, np.uint8)
    p = _hp(buf)
    mc = lambda vol, B, dims, off, ws, ws_bytes: lib.ls_marching_cubes_batch_f64(vol, B, *dims, 0.0, None, 0, None, 0, off, ws, ws_bytes, None)
    need = lib.ls_mcubes_batch_workspace_bytes(2, 8, 8, 8)
    assert mc(None, 2, (8, 8, 8), p, p, need) == INVALID
    assert mc(p, 2, (8, 8, 8), None, p, need) == INVALID
    assert mc(p, 2, (8, 8, 8), p, None, need) == INVALID
    for B in (0, -1, 65536):
        ok, why = _refused(mc(p, B, (8, 8, 8), p, p, need), "B=")
        assert ok, why
    assert mc(p, 2, (8, 0, 8), p, p, need) == INVALID
    ok, why = _refused(mc(p, 64, (131, 131, 131), p, p, 1 << 40), "2^31")
    assert ok, why
    ok, why = _refused(mc(p, 1, (2048, 2048, 2048), p, p, 1 << 40), "too large")
    assert ok, why
    assert lib.ls_marching_cubes_batch_f64(p, 2, 8, 8, 8, 0.0, None, -1, None, 0, p, p, need, None) == INVALID
    assert mc(p, 2, (8, 8, 8), p, p, need - 1) == WORKSPACE
