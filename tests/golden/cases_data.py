"""Seeded INPUTS of the golden case G18 (dataset loaders): two D-NeRF blender scenes and one custom scene, as the frames of
their transforms files.  Imported by make_golden_data.py (which writes them to disk and runs the reference's unmodified loaders
on them) and by tests/test_data_host.py (which writes the same directories for swnerf.data)."""
import json
import os

import numpy as np

from swnerf import synth

IMG_HW = (16, 16)                        # every frame of the three scenes
DNERF_SKIP, CUSTOM_SKIP, CUSTOM_SEED = 2, 2, 7
CUSTOM_INTR = {"fl_x": 21.5, "fl_y": 22.25, "cx": 7.75, "cy": 8.5}


def _pose(theta, phi):
    return synth.pose_spherical(float(theta), float(phi), 4.0).astype(float).tolist()


def g18_dnerf_frames(with_time):
    """{split: frames}.  with_time: every frame carries its 'time' (train ends at 1); else the loader derives t / (len - 1)."""
    out = {}
    for s, n in (("train", 9), ("val", 5), ("test", 7)):
        out[s] = []
        for i in range(n):
            f = {"file_path": f"./{s}/r_{i:03d}", "transform_matrix": _pose(17 * i + 3 * len(s), -30.0 + 2 * i)}
            if with_time:
                f["time"] = (i / (n - 1)) ** 2 if s != "train" else i / (n - 1)
            out[s].append(f)
    return out


def g18_dnerf_render_frames():
    return [{"transform_matrix": _pose(29 * i, -20.0 - i)} for i in range(6)]


def g18_custom_frames(n=13):
    return [{"file_path": f"images/f_{i:02d}.png", "transform_matrix": _pose(23 * i + 1, -35.0 + 3 * i)} for i in range(n)]


def write_dnerf_scene(base, with_time, touch):
    """touch(path): creates the image file"""
    for s, fr in g18_dnerf_frames(with_time).items():
        os.makedirs(os.path.join(base, s), exist_ok=True)
        for f in fr:
            touch(os.path.join(base, f["file_path"] + ".png"))
        with open(os.path.join(base, f"transforms_{s}.json"), "w") as fp:
            json.dump({"camera_angle_x": synth.LEGO_CAMERA_ANGLE_X, "frames": fr}, fp)
    if with_time:
        with open(os.path.join(base, "transforms_render.json"), "w") as fp:
            json.dump({"camera_angle_x": synth.LEGO_CAMERA_ANGLE_X, "frames": g18_dnerf_render_frames()}, fp)


def write_custom_scene(base, touch):
    os.makedirs(os.path.join(base, "images"), exist_ok=True)
    frames = g18_custom_frames()
    for f in frames:
        touch(os.path.join(base, f["file_path"]))
    with open(os.path.join(base, "transforms.json"), "w") as fp:
        json.dump(dict(CUSTOM_INTR, frames=frames), fp)
