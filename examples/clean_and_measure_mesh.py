#!/usr/bin/env python3
"""The last step of the reference's scale-aware chain - taking a number off the real-scaled mesh - with what exists offline: a
synthetic density field with floaters (an ellipsoid "object" and seeded specks of density all over the bounds, as a trained NeRF's
`--threshold` iso-surface has them) -> `generate_mesh` (marching cubes on the GPU) -> `clean` (largest connected component,
optional Taubin smoothing) -> `transform_mesh` with a given scale (what `cal_scale` returns from the markers; see
transform_mesh_aruco_like.py) -> `measure`.  Prints extents, area and volume before and after cleaning and writes both OBJs.
Nothing beyond torch and numpy is needed (no trimesh).

  python examples/clean_and_measure_mesh.py [out_dir] [resolution=96] [scale=0.25] [smooth_iterations=10]

The object is the ellipsoid with semi-axes (0.6, 0.45, 0.3) in grid units: at scale s its extents are 2 s (0.6, 0.45, 0.3), its
volume 4/3 pi s^3 0.6 0.45 0.3 - the raw mesh's extents are the whole box instead."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sw-nerf_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np

AXES = (0.6, 0.45, 0.3)


def floater_field(resolution, n_floaters=40, seed=7):
    """-> (density [R,R,R] float32, colour [R,R,R,3] float32, (X, Y, Z)): positive inside the ellipsoid and inside n_floaters small
    balls scattered through [-1, 1]^3 away from it"""
    x = np.linspace(-1., 1., resolution)
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    f = 1. - np.sqrt((X / AXES[0]) ** 2 + (Y / AXES[1]) ** 2 + (Z / AXES[2]) ** 2)
    rng = np.random.default_rng(seed)
    placed = 0
    while placed < n_floaters:
        c = rng.uniform(-0.9, 0.9, 3)
        r = rng.uniform(0.04, 0.09)
        if np.sqrt(((c / np.array(AXES)) ** 2).sum()) < 1.4:          # keep the specks off the object
            continue
        f = np.maximum(f, (r - np.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2)) / r)
        placed += 1
    col = np.stack([(X + 1) / 2, (Y + 1) / 2, (Z + 1) / 2], -1)
    return f.astype(np.float32), col.astype(np.float32), (X, Y, Z)


def report(tag, m):
    e = "none" if m.extents is None else " x ".join(f"{x:.4f}" for x in m.extents)
    print(f"{tag}: {m.n_vertices} vertices, {m.n_faces} faces, {m.n_components} component(s), closed = {m.closed}, "
          f"extents {e}, area {m.area:.5f}, volume {m.volume:.5f}")


def main(out_dir, resolution=96, scale=0.25, smooth_iterations=10):
    from swnerf import mesh, markers
    os.makedirs(out_dir, exist_ok=True)
    density, colour, xyz = floater_field(resolution)
    raw = mesh.generate_mesh(density, colour, xyz, density_threshold=0.)
    cleaned = mesh.clean(raw, keep=1, smooth_iterations=smooth_iterations)          # same as generate_mesh(..., clean={...})
    M = np.eye(4)
    raw_path, clean_path = os.path.join(out_dir, "mesh_raw_scaled.obj"), os.path.join(out_dir, "mesh_clean_scaled.obj")
    raw_scaled = markers.transform_mesh(raw, raw_path, scale, M)
    clean_scaled = markers.transform_mesh(cleaned, clean_path, scale, M)
    before, after = raw_scaled.measure(), clean_scaled.measure()
    report("raw    ", before)
    report("cleaned", after)
    want = 4. / 3. * np.pi * scale ** 3 * AXES[0] * AXES[1] * AXES[2]
    print(f"ellipsoid at scale {scale}: extents {' x '.join(f'{2 * scale * a:.4f}' for a in AXES)}, volume {want:.5f}")
    print(f"wrote {raw_path} and {clean_path}")
    return before, after, raw_path, clean_path


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else "/tmp/swnerf_clean_mesh_example"
    R = int(sys.argv[2]) if len(sys.argv) > 2 else 96
    s = float(sys.argv[3]) if len(sys.argv) > 3 else 0.25
    it = int(sys.argv[4]) if len(sys.argv) > 4 else 10
    main(out, R, s, it)
