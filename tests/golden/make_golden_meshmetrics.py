#!/usr/bin/env python3
"""tests/golden/mesh_contains.npz: the reference's own libmesh.check_mesh_contains on a set of meshes and points (dev container only).

    python tests/golden/make_golden_meshmetrics.py

The reference's triangle_hash.pyx is compiled OUT OF TREE into /tmp/trihash_build (cython + g++, as build_ref_native.py does: nothing
is copied into the repository, nothing is written to the reference tree); its inside_mesh.py is loaded by path as `libmesh.inside_mesh`
with the compiled module registered as `libmesh.triangle_hash`, and run unchanged.

Cases: a unit cube (its vertical faces have n_2 == 0), an icosphere, a torus (genus 1), a marching-cubes mesh of a small random field
(oracle/mcubes.py, the CPU restatement of the reference's libmcubes), a flat mesh, and a cube with unreferenced far-away vertices.  Points:
a lattice through the mesh's corners that hits vertices and edges exactly and reaches past the bounding box, the bounding box's faces,
and random points.  Stored per case: <case>_V, <case>_F, <case>_P, <case>_inside (bool).
"""
import importlib.util
import os
import subprocess
import sys
import sysconfig
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
LIBMESH = "/root/reference/lib_shape_prior/core/models/utils/occnet_utils/utils/libmesh"
OUT_DIR = "/tmp/trihash_build"


def load_reference():
    os.makedirs(OUT_DIR, exist_ok=True)
    gen = os.path.join(OUT_DIR, "triangle_hash.cpp")
    so = os.path.join(OUT_DIR, "triangle_hash" + sysconfig.get_config_var("EXT_SUFFIX"))
    subprocess.check_call([sys.executable, "-m", "cython", "--cplus", "-3", "-o", gen, os.path.join(LIBMESH, "triangle_hash.pyx")])
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-std=c++14", "-w", "-DNPY_NO_DEPRECATED_API=0",
                           "-I" + sysconfig.get_paths()["include"], "-I" + np.get_include(), gen, "-o", so])
    pkg = types.ModuleType("libmesh")
    pkg.__path__ = []
    sys.modules["libmesh"] = pkg
    spec = importlib.util.spec_from_file_location("libmesh.triangle_hash", so)
    th = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(th)
    sys.modules["libmesh.triangle_hash"] = th
    spec = importlib.util.spec_from_file_location("libmesh.inside_mesh", os.path.join(LIBMESH, "inside_mesh.py"))
    im = importlib.util.module_from_spec(spec)
    sys.modules["libmesh.inside_mesh"] = im
    spec.loader.exec_module(im)
    return im.check_mesh_contains


class Mesh:
    def __init__(self, V, F):
        self.vertices, self.faces = np.asarray(V, np.float64), np.asarray(F, np.int64)


def lattice_points(V, F, rng, n_rand=600):
    used = V[np.unique(F)]
    lo, hi = used.min(0), used.max(0)
    ext = np.where(hi > lo, hi - lo, 1.0)
    # 9 steps across the box: the corners of an axis-aligned mesh (cube) and its edge midpoints are lattice points
    ax = [lo[a] + ext[a] * np.arange(-2, 11) / 8 for a in range(3)]
    g = np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)
    faces = []
    for a in range(3):   # points ON the bounding box's faces
        for side in (lo[a], hi[a]):
            p = lo + rng.random((40, 3)) * ext
            p[:, a] = side
            faces.append(p)
    rand = lo - 0.2 * ext + rng.random((n_rand, 3)) * 1.4 * ext
    return np.concatenate([g, used[:200], np.concatenate(faces), rand])


def cases():
    import meshmetrics_oracle as mo
    from oracle import mcubes
    rng = np.random.default_rng(11)
    out = {"cube": mo.cube(), "icosphere": mo.icosphere(2)}
    V, F = mo.torus()
    out["torus"] = (V, F)
    field = rng.standard_normal((14, 14, 14))
    field[[0, -1]] = field[:, [0, -1]] = field[:, :, [0, -1]] = 3.0     # closed surface
    mv, mf = mcubes.marching_cubes(field, 0.0)
    out["mcubes"] = (np.asarray(mv, np.float64) / 13.0, np.asarray(mf, np.int64))
    xs = np.linspace(0, 1, 5)
    fv = np.array([[x, y, 0.0] for x in xs for y in xs])
    ff = [[i * 5 + j, (i + 1) * 5 + j, (i + 1) * 5 + j + 1] for i in range(4) for j in range(4)] + \
         [[i * 5 + j, (i + 1) * 5 + j + 1, i * 5 + j + 1] for i in range(4) for j in range(4)]
    out["flat"] = (fv, np.array(ff))
    cv, cf = mo.cube()
    far = np.array([[100.0, -50.0, 3.0], [-40.0, 80.0, -90.0]])
    out["unreferenced"] = (np.concatenate([far[:1], cv, far[1:]]), cf + 1)
    return {k: (np.asarray(v, np.float64), np.asarray(f, np.int64)) for k, (v, f) in out.items()}, rng


def main():
    check_mesh_contains = load_reference()
    data = {}
    cs, rng = cases()
    for name, (V, F) in cs.items():
        P = lattice_points(V, F, rng)
        inside = np.asarray(check_mesh_contains(Mesh(V, F), P), bool)
        data.update({f"{name}_V": V, f"{name}_F": F.astype(np.int32), f"{name}_P": P, f"{name}_inside": inside})
        print(f"{name}: {len(F)} faces, {len(P)} points, {int(inside.sum())} inside")
    path = os.path.join(HERE, "mesh_contains.npz")
    np.savez_compressed(path, cases=np.array(sorted(cs)), **data)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
