#!/usr/bin/env python3
"""The reference's nerf/transform_mesh.py flow on the MI355X path, end to end, on a synthetic scene (no photographed marker is
available offline): a planar 4 x 4 marker of known edge in a world of arbitrary unit, eight nerf-convention cameras on a ring
(tests/marker_ref.py renders their photos), a dataset directory as load_custom_data expects it (transforms.json, images_ori/),
then `cal_scale` - marker detection on the GPU, triangulation of the four corners, scale and the rotation that turns the
marker's normal to +z - and `transform_mesh` on an OBJ.  Nothing beyond torch and numpy is needed (no cv2, scipy, trimesh).

  python examples/transform_mesh_aruco_like.py [out_dir] [real_length=0.296]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sw-nerf_amd"), ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np
import torch


def main(out_dir, real_length=0.08 * 3.7):
    import marker_ref
    from swnerf import markers, mesh, png
    scene = marker_ref.make_scene()
    os.makedirs(os.path.join(out_dir, "images_ori"), exist_ok=True)
    meta = dict(fl_x=scene["fx"], fl_y=scene["fy"], cx=scene["cx"], cy=scene["cy"], k1=0., k2=0., p1=0., p2=0., frames=[])
    for k, (frame, pose) in enumerate(zip(scene["frames"], scene["poses"])):
        png.write_png(os.path.join(out_dir, "images_ori", f"{k:03d}.png"), np.repeat(frame[..., None], 3, -1))
        meta["frames"].append(dict(file_path=f"images/{k:03d}.png", transform_matrix=pose.tolist()))
    with open(os.path.join(out_dir, "transforms.json"), "w") as fh:
        json.dump(meta, fh)
    # the mesh extract_mesh would have left: here a small pyramid standing on the marker, in the world's arbitrary unit
    c3 = scene["corners3d"]
    n = np.cross(c3[1] - c3[0], c3[2] - c3[0])
    n /= np.linalg.norm(n)
    verts = np.concatenate([c3, c3.mean(0, keepdims=True) - 0.05 * n]).astype(np.float32)
    faces = np.array([[0, 1, 4], [1, 2, 4], [2, 3, 4], [3, 0, 4], [0, 2, 1], [0, 3, 2]], np.int32)
    src = mesh.Mesh(verts, faces, np.tile(n.astype(np.float32), (5, 1))).export(os.path.join(out_dir, "mesh.obj"))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    scale, M = markers.cal_scale(out_dir, real_length)                    # transform_mesh.py:326
    dt = time.perf_counter() - t0
    dst = os.path.join(out_dir, "transformed_mesh.obj")
    out = markers.transform_mesh(src, dst, scale, M)                      # transform_mesh.py:327
    edges = np.linalg.norm(out.vertices[:4] - np.roll(out.vertices[:4], -1, axis=0), axis=1)
    print(f"scale {scale:.5f} (true {real_length / scene['edge']:.5f}) in {dt:.3f} s; marker edge in the mesh {edges.mean():.5f} "
          f"(real {real_length:.5f}); M n = {np.round(M[:3, :3] @ n, 4).tolist()} -> {dst}")
    return scale, M, dst


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else "/tmp/swnerf_transform_mesh_example"
    main(out, float(sys.argv[2]) if len(sys.argv) > 2 else 0.08 * 3.7)
