"""Makes tests/golden/render_pointcloud.npz: a 7 x 5 fp32 depth map with zeros and what the REFERENCE's own pointcloud (utils/render.py)
returns for it.  The reference module imports trimesh and pyrender at its top, which pointcloud does not use: stub modules stand in for
them in sys.modules.  Run where the reference checkout is (no GPU needed):

    python scripts/dev/make_render_golden.py /path/to/reference
"""
import importlib.util
import os
import sys
import types

import numpy as np

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))


def main(ref_root):
    for name in ("trimesh", "pyrender"):
        sys.modules.setdefault(name, types.ModuleType(name))
    spec = importlib.util.spec_from_file_location("reference_render", os.path.join(ref_root, "utils", "render.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    rng = np.random.Generator(np.random.Philox(key=[7, 5]))
    depth = (0.5 + 2.0 * rng.random((7, 5))).astype(np.float32)
    depth[rng.random((7, 5)) < 0.4] = 0.0
    depth[0, 0], depth[6, 4], depth[3, 2] = np.float32(1.25), 0.0, np.float32(0.75)   # a corner hit, a corner miss, an exact value
    # the reference's constants are for 100 x 100 images; pointcloud uses k alone, so a 7 x 5 map is within its contract
    xyz = ref.pointcloud(depth)
    out = os.path.join(REPO, "tests", "golden", "render_pointcloud.npz")
    np.savez(out, depth=depth, xyz=xyz, k=ref.k)
    print(out, depth.shape, xyz.shape, xyz.dtype, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
