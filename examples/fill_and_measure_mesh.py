#!/usr/bin/env python3
"""Measuring an object that stands on the floor of its bounds box: a sphere density field whose lower part leaves the box ->
`generate_mesh` (marching cubes on the GPU) leaves the surface open where the object meets the box -> `measure` says closed=False
and its volume is not that of the solid -> `fill_holes` caps every boundary loop with a fan around its mean -> `measure` says
closed=True, and the volume is the spherical cap's.  Writes the filled OBJ.  Nothing beyond torch and numpy is needed (no trimesh).

  python examples/fill_and_measure_mesh.py [out_dir] [resolution=64]

The object is the sphere of radius 0.6 centred (0, 0, -0.7) in the box [-1, 1]^3: the part above z = -1 is a cap of height 0.9."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sw-nerf_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np

RADIUS, CENTRE_Z = 0.6, -0.7


def sphere_field(resolution):
    x = np.linspace(-1., 1., resolution)
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    f = RADIUS - np.sqrt(X ** 2 + Y ** 2 + (Z - CENTRE_Z) ** 2)
    col = np.stack([(X + 1) / 2, (Y + 1) / 2, (Z + 1) / 2], -1)
    return f.astype(np.float32), col.astype(np.float32), (X, Y, Z)


def report(tag, m):
    print(f"{tag}: {m.n_vertices} vertices, {m.n_faces} faces, closed={m.closed}, boundary edges {m.boundary_edges}, "
          f"area {m.area:.5f}, volume {m.volume:.5f}")


def main(out_dir, resolution=64):
    from swnerf import mesh
    os.makedirs(out_dir, exist_ok=True)
    density, colour, xyz = sphere_field(resolution)
    raw = mesh.generate_mesh(density, colour, xyz, density_threshold=0.)
    filled = mesh.fill_holes(raw)
    before, after = raw.measure(), filled.measure()
    report("as extracted", before)
    report("holes filled", after)
    h = CENTRE_Z + RADIUS + 1.
    exact = np.pi * h * h * (3 * RADIUS - h) / 3
    info = filled.fill_info
    print(f"{info['loops']} loop(s), {info['filled_edges']} boundary edges filled with {info['new_faces']} faces; "
          f"the cap's volume is {exact:.5f}: {100 * after.volume / exact:.2f} % after, {100 * before.volume / exact:.2f} % before")
    path = os.path.join(out_dir, "mesh_filled.obj")
    filled.export(path)
    print(f"wrote {path}")
    return before, after, path


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else "/tmp/swnerf_fill_and_measure_mesh_example"
    R = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    main(out, R)
