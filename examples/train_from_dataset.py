#!/usr/bin/env python3
"""From a dataset DIRECTORY to a trained net with nothing in between: writes a small Blender-layout scene (transforms_train /
val / test.json and RGBA PNG frames, png.write_png) of a synthetic picture - no dataset is available offline - loads it with
`data.load_dataset` (the host inflates, the device undoes the PNG filters and, with half_res, takes the area mean) and hands the
dict to `runner.train` as it is.  The frames stay uint8 RGBA on the device; the batch kernel composites the drawn pixels on white.
From the command line the run ends as the reference's does, with the spiral of the render poses as two Motion-JPEG .avi files
(i_video = the last iteration; main(..., video=True)).

  python examples/train_from_dataset.py [out_dir] [H=32] [n_train=6] [steps=20] [half_res=0]
"""
import json
import os
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sw-nerf_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np
import torch


def write_scene(base, H, W, n_train, n_val=2, n_test=2):
    """A disc whose colour turns with the view angle on a transparent background, seen from the blender sphere."""
    from swnerf import png, synth
    y, x = np.mgrid[0:H, 0:W]
    r = np.hypot((y + .5) / H - .5, (x + .5) / W - .5)
    k = 0
    for s, n in (("train", n_train), ("val", n_val), ("test", n_test)):
        os.makedirs(os.path.join(base, s), exist_ok=True)
        frames = []
        for i in range(n):
            theta = 360.0 * k / (n_train + n_val + n_test)
            rgba = np.zeros((H, W, 4), np.uint8)
            rgba[..., 0] = 255 * (0.5 + 0.5 * np.cos(np.deg2rad(theta)))
            rgba[..., 1] = np.clip(255 * (1 - 2 * r), 0, 255)
            rgba[..., 2] = 255 * (0.5 + 0.5 * np.sin(np.deg2rad(theta)))
            rgba[..., 3] = np.where(r < 0.4, 255, 0)
            png.write_png(os.path.join(base, s, f"r_{i}.png"), rgba)
            frames.append({"file_path": f"./{s}/r_{i}", "transform_matrix": synth.pose_spherical(theta, -30.0, 4.0).astype(float).tolist()})
            k += 1
        with open(os.path.join(base, f"transforms_{s}.json"), "w") as fp:
            json.dump({"camera_angle_x": synth.LEGO_CAMERA_ANGLE_X, "frames": frames}, fp)


def main(out_dir, H=32, n_train=6, steps=20, half_res=False, device="cuda:0", video=False):
    from swnerf import data, runner
    dev = torch.device(device)
    scene = os.path.join(out_dir, "scene")
    write_scene(scene, H, H, n_train)
    side = H // 2 if half_res else H
    args = SimpleNamespace(expname="train_from_dataset", basedir=out_dir, datadir=scene, dataset_type="blender", half_res=bool(half_res),
                           testskip=1, netdepth=8, netwidth=256, netdepth_fine=8, netwidth_fine=256, lrate=5e-4, lrate_decay=500,
                           netchunk=1024 * 64, no_reload=True, ft_path=None, N_samples=32, N_importance=32, perturb=1.,
                           use_viewdirs=True, i_embed=0, multires=10, multires_views=4, raw_noise_std=0., white_bkgd=True,
                           no_ndc=False, lindisp=False, chunk=1024 * 32, N_rand=min(512, side * side), no_batching=True,
                           precrop_iters=0, precrop_frac=.5, i_print=max(steps // 4, 1), i_weights=steps, i_testset=10 ** 9,
                           N_iters=steps, seed=0, i_video=steps if video else 10 ** 9)
    d = data.load_dataset(args, device=dev)
    print(f"loaded {tuple(d['images'].shape)} {d['images'].dtype} on {d['images'].device}; hwf {d['hwf']}, near {d['near']}, far {d['far']}, "
          f"split {[len(s) for s in d['i_split']]}")
    torch.manual_seed(0)
    np.random.seed(0)
    record = runner.train(args, d, device=dev)
    print(f"trained {len(record)} steps of {args.N_rand} rays: loss {record[0]['loss']:.4f} -> {record[-1]['loss']:.4f}")
    if video:                                                                  # nerf/run.py:726-733: the spiral after the last iteration
        print("video:", os.path.join(out_dir, args.expname, "{}_spiral_{:06d}_rgb.avi".format(args.expname, steps)), "and ..._disp.avi")
    return d, record


if __name__ == "__main__":
    a = sys.argv
    main(a[1] if len(a) > 1 else "/tmp/swnerf_dataset_example", int(a[2]) if len(a) > 2 else 32, int(a[3]) if len(a) > 3 else 6,
         int(a[4]) if len(a) > 4 else 20, bool(int(a[5])) if len(a) > 5 else False, video=True)
