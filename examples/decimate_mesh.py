#!/usr/bin/env python3
"""Shrinking an extracted mesh without losing what it is measured for: an ellipsoid density field -> `generate_mesh` (marching
cubes on the GPU) -> `weld` (coincident vertices merged, what trimesh's process=True does) -> `decimate` by vertex clustering with
the quadric representative, and with the plain cluster mean for comparison -> `measure` before and after.  The quadric keeps the
volume to a fraction of a percent at a tenth of the faces; the mean shrinks the body.  Writes the full and the decimated OBJ.
Nothing beyond torch and numpy is needed (no trimesh).

  python examples/decimate_mesh.py [out_dir] [resolution=64] [cell_in_spacings=2.5]

The object is the ellipsoid with semi-axes (0.6, 0.45, 0.3): its volume is 4/3 pi 0.6 0.45 0.3."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sw-nerf_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np

AXES = (0.6, 0.45, 0.3)


def ellipsoid_field(resolution):
    x = np.linspace(-1., 1., resolution)
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    f = 1. - np.sqrt((X / AXES[0]) ** 2 + (Y / AXES[1]) ** 2 + (Z / AXES[2]) ** 2)
    col = np.stack([(X + 1) / 2, (Y + 1) / 2, (Z + 1) / 2], -1)
    return f.astype(np.float32), col.astype(np.float32), (X, Y, Z)


def report(tag, m):
    print(f"{tag}: {m.n_vertices} vertices, {m.n_faces} faces, closed = {m.closed}, Euler characteristic {m.euler}, "
          f"area {m.area:.5f}, volume {m.volume:.5f}")


def main(out_dir, resolution=64, cells=2.5):
    from swnerf import mesh
    os.makedirs(out_dir, exist_ok=True)
    density, colour, xyz = ellipsoid_field(resolution)
    h = 2. / (resolution - 1)
    raw = mesh.generate_mesh(density, colour, xyz, density_threshold=0.)
    welded = mesh.weld(raw)
    quadric = mesh.decimate(welded, cell=cells * h, placement="quadric")
    mean = mesh.decimate(welded, cell=cells * h, placement="mean")
    before, after, after_mean = welded.measure(), quadric.measure(), mean.measure()
    report("extracted and welded ", before)
    report("decimated (quadric)  ", after)
    report("decimated (mean)     ", after_mean)
    print(f"volume kept: {100 * after.volume / before.volume:.2f} % (quadric), {100 * after_mean.volume / before.volume:.2f} % (mean); "
          f"the ellipsoid's is {4. / 3. * np.pi * AXES[0] * AXES[1] * AXES[2]:.5f}")
    full_path, small_path = os.path.join(out_dir, "mesh_full.obj"), os.path.join(out_dir, "mesh_decimated.obj")
    welded.export(full_path)
    quadric.export(small_path)
    print(f"wrote {full_path} and {small_path}")
    return before, after, after_mean, full_path, small_path


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else "/tmp/swnerf_decimate_mesh_example"
    R = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    c = float(sys.argv[3]) if len(sys.argv) > 3 else 2.5
    main(out, R, c)
