"""A CPU experiment with the twins alone (no device): what the completion of a fused state does to the analytic sphere of the
scene-memory rows (r = 0.4, 40^3, trunc = 4 h, analytic depth maps of 100 x 100) fused from 3 of its 8 views.

    python scripts/tsdf_prior_experiment.py

The "prior" is the exact distance to the sphere, and the same field of a sphere one voxel too large; the weights 1, 2 and 8.  Printed
per case: faces, boundary edges, and the max / rms distance of the completed mesh's vertices from the true sphere on the OBSERVED part
(every sample around the vertex seen at least once) and on the rest; and the spurious walls: faces with a vertex farther than
sqrt(3) h + the prior's own offset from the true sphere -- a +t observation next to a -t belief makes the field cross 0 where no
surface is.  Nothing here recommends a weight."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import fuse_oracle as fo  # noqa: E402
import tsdf_prior_oracle as tpo  # noqa: E402
from test_depth_fuse_cpu import sphere_state  # noqa: E402
from test_tsdf_prior_cpu import boundary_edges, least_seen_around, sphere_field  # noqa: E402


def main():
    (S, N), origin, h = sphere_state(views=3)
    r, trunc, centre, s = 0.4, 4 * h, np.zeros(3), 1.0
    vo, fo_ = fo.mesh((S, N), origin, h, 1)
    e = np.abs(np.linalg.norm(vo, axis=1) - r)
    print(f"observed: {int((N > 0).sum())} of {N.size} samples seen; {len(fo_)} faces, {boundary_edges(fo_)[0]} boundary edges, max {e.max() / h:.2f} h, "
          f"rms {np.sqrt((e ** 2).mean()) / h:.3f} h")
    for name, grow in (("exact", 0.0), ("1 h too large", h)):
        for w0 in (1, 2, 8):
            rows = tpo.rows((S, N), origin, h, w0)
            done, counts = tpo.vote((S, N), sphere_field(rows["points"], centre, r + grow, s), s, trunc, w0)
            v, f = fo.mesh(done, origin, h, w0)
            err = np.abs(np.linalg.norm(v, axis=1) - r)
            obs = least_seen_around(N, v, origin, h) >= 1
            wall = err > np.sqrt(3) * h + grow
            walls = int(wall[f].any(1).sum())
            fmt = lambda x: f"max {x.max() / h:.2f} h rms {np.sqrt((x ** 2).mean()) / h:.3f} h" if len(x) else "none"   # noqa: E731
            print(f"prior {name:13s} weight {w0}: rows {counts[0]}; {len(f)} faces, {boundary_edges(f)[0]} boundary edges; observed part ({int(obs.sum())} "
                  f"vertices) {fmt(err[obs])}; rest ({int((~obs).sum())}) {fmt(err[~obs])}; faces in spurious walls {walls}")


if __name__ == "__main__":
    main()
