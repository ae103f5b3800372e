#!/usr/bin/env python3
"""Capture g21_markers.npz from the UNMODIFIED reference: nerf/transform_mesh.py's undistort_points, get_ray_direction,
calculate_3d_corners (scipy's least_squares inside triangulate_point) and calculate_transform_matrix.  Only arrays are recorded:
the inputs and outputs of those four functions.  cv2, trimesh, matplotlib and the reference's utils are not on this path: empty
stand-in modules.

The scene is consistent in the reference's OWN reading of a pose (centre -R^T t, rays R [x, y, +1] after the forward distortion
model), so its triangulation recovers the corners; next to the least_squares answer the file stores its distance to the closed
form swnerf.markers.triangulate_corners(convention="reference") - asserted here to be below 1e-5 of the marker edge."""
import importlib.util
import os
import sys
import types

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
REF = "/root/reference"
for name in ["cv2", "cv2.aruco", "trimesh", "matplotlib", "matplotlib.pyplot", "mpl_toolkits", "mpl_toolkits.mplot3d", "utils"]:
    sys.modules[name] = types.ModuleType(name)
sys.modules["cv2"].aruco = sys.modules["cv2.aruco"]
sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
sys.modules["mpl_toolkits.mplot3d"].Axes3D = None
sys.modules["utils"].config_parser = None
spec = importlib.util.spec_from_file_location("ref_transform_mesh", os.path.join(REF, "nerf", "transform_mesh.py"))
ref = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref)
sys.path.insert(0, os.path.join(ROOT, "sw-nerf_amd"))
from swnerf import markers  # noqa: E402


def random_rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def main():
    rng = np.random.default_rng(21)
    edge = 0.08
    intr = dict(fl_x=1450., fl_y=1462., cx=961.5, cy=538.25, k1=0.04, k2=-0.01, p1=0.0015, p2=-0.0008)
    Rm = random_rotation(rng)
    centre = np.array([0.1, -0.05, 0.2])
    world = (0.5 * edge * np.array([[-1, 1, 0], [1, 1, 0], [1, -1, 0], [-1, -1, 0]], np.float64)) @ Rm.T + centre
    poses, corners = [], []
    while len(poses) < 7:
        cpos = centre + rng.normal(size=3) * 0.4
        z = centre - cpos
        z /= np.linalg.norm(z)                                   # the reference's rays look down +z of R
        x = np.cross(z, rng.normal(size=3))
        x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z], 1)
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R, -R @ cpos                       # so that -R^T t is the centre
        cam = (world - cpos) @ R
        target = cam[:, :2] / cam[:, 2:3]
        n = target.copy()                                        # invert the forward model by fixed-point iteration
        for _ in range(60):
            n = n - (ref.undistort_points(n, intr["k1"], intr["k2"], intr["p1"], intr["p2"]) - target)
        poses.append(T)
        corners.append(np.stack([n[:, 0] * intr["fl_x"] + intr["cx"], n[:, 1] * intr["fl_y"] + intr["cy"]], 1)[None])
    poses, corners = np.stack(poses), np.stack(corners)         # [m,4,4], [m,1,4,2] (cv2 returns (1,4,2) per marker)

    und_in = rng.uniform(-0.6, 0.6, (32, 2))
    und_out = ref.undistort_points(und_in, intr["k1"], intr["k2"], intr["p1"], intr["p2"])
    params = lambda T: (intr["fl_x"], intr["fl_y"], intr["cx"], intr["cy"], intr["k1"], intr["k2"], intr["p1"], intr["p2"], T)
    rays = np.stack([ref.get_ray_direction(c, params(T)) for c, T in zip(corners, poses)])
    frame_info = [{"frame": {"transform_matrix": T.tolist()}, "corners": c} for c, T in zip(corners, poses)]
    ref_world = ref.calculate_3d_corners(frame_info, intr)
    closed = markers.triangulate_corners(corners[:, 0], poses, intr, convention="reference")
    dist = np.linalg.norm(ref_world - closed, axis=1)
    assert dist.max() < 1e-5 * edge, dist
    assert np.abs(ref_world - world).max() < 1e-4 * edge, np.abs(ref_world - world).max()

    tm_in = np.concatenate([ref_world[None], rng.normal(size=(5, 4, 3))])
    tm_out = np.stack([ref.calculate_transform_matrix(c) for c in tm_in])
    out = os.path.join(HERE, "g21_markers.npz")
    np.savez(out, edge=np.float64(edge), intrinsics=np.array([intr[k] for k in ("fl_x", "fl_y", "cx", "cy", "k1", "k2", "p1", "p2")]),
             poses=poses, corners=corners, rays=rays, undistort_in=und_in, undistort_out=und_out, world=world,
             least_squares_world=ref_world, closed_form_distance=dist, transform_in=tm_in, transform_out=tm_out)
    print(f"wrote {out}: max |least_squares - closed form| = {dist.max():.3e} ({dist.max() / edge:.3e} of the edge)")


if __name__ == "__main__":
    main()
