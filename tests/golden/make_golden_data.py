#!/usr/bin/env python3
"""Capture g18_data.npz: the reference's dataloader/load_blender_dnerf.py and dataloader/load_custom_data.py run, unmodified, on
tiny SYNTHETIC on-disk scenes (cases_data.py) written to a temp dir.  The image reader and cv2 are stubbed as in
make_golden_cameras.py (imageio / cv2 are absent offline): blank frames of the right size, RGB for the custom scene so that its
alpha append runs.  Pinned: poses, times, render poses and times, hwf, K and split sizes - nothing that depends on a pixel."""
import os
import random
import sys
import tempfile
import types

import numpy as np

sys.dont_write_bytecode = True
os.environ.setdefault("MPLBACKEND", "Agg")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "..", "sw-nerf_amd"))
import cases_data  # noqa: E402

imageio = types.ModuleType("imageio")
imageio.imread = lambda f: np.zeros(cases_data.IMG_HW + (3 if "custom" in f else 4,), np.uint8)
sys.modules["imageio"] = imageio
cv2 = types.ModuleType("cv2")
cv2.INTER_AREA = 3
cv2.resize = lambda img, wh, interpolation=None: np.zeros((wh[1], wh[0], img.shape[-1]), img.dtype)
sys.modules["cv2"] = cv2
sys.path.insert(0, "/root/reference")
from dataloader import load_blender_dnerf, load_custom_data  # noqa: E402


def _np(x):
    return x.numpy() if hasattr(x, "numpy") else np.asarray(x)


def main():
    tmp = tempfile.mkdtemp(prefix="swnerf_golden_")
    touch = lambda p: open(p, "wb").close()
    out = {}
    for with_time, scene in ((True, "timed"), (False, "untimed")):
        base = os.path.join(tmp, f"dnerf_{scene}")
        cases_data.write_dnerf_scene(base, with_time, touch)
        for half in (False, True):
            imgs, poses, times, render_poses, render_times, hwf, i_split = load_blender_dnerf.load_blender_data(
                base, half_res=half, testskip=cases_data.DNERF_SKIP)
            tag = f"dn_{scene}_{'half' if half else 'full'}"
            out.update({f"{tag}_poses": poses, f"{tag}_times": times, f"{tag}_render": _np(render_poses), f"{tag}_render_times": _np(render_times),
                        f"{tag}_hwf": np.array(hwf, np.float64), f"{tag}_split": np.array([len(s) for s in i_split]),
                        f"{tag}_imshape": np.array(imgs.shape)})
    base = os.path.join(tmp, "custom_scene")
    cases_data.write_custom_scene(base, touch)
    for half in (False, True):
        random.seed(cases_data.CUSTOM_SEED)
        imgs, poses, render_poses, K, hwf, i_split = load_custom_data.load_custom_data(base, half_res=half, testskip=cases_data.CUSTOM_SKIP)
        tag = f"cu_{'half' if half else 'full'}"
        out.update({f"{tag}_poses": poses, f"{tag}_render": _np(render_poses), f"{tag}_K": np.asarray(K, np.float64),
                    f"{tag}_hwf": np.array(hwf, np.float64), f"{tag}_split": np.array([len(s) for s in i_split]),
                    f"{tag}_imshape": np.array(imgs.shape)})
    np.savez_compressed(os.path.join(HERE, "g18_data.npz"), **out)
    print("g18_data.npz", os.path.getsize(os.path.join(HERE, "g18_data.npz")) // 1024, "KiB")


if __name__ == "__main__":
    main()
