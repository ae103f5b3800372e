#!/usr/bin/env python3
"""Fit a small synthetic picture with swnerf.fit2d (the flow of the reference's 2d_pos_encoding/main.py): a 96 x 64 picture
generated in code, Model(2 + 4 L, layer_num) with AdamW and ExponentialLR, a few epochs of 512-pixel batches, then the fitted
picture as a PNG.
  python examples/fit_image_2d.py [--epochs 10] [--out /tmp/fit2d]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sw-nerf_amd"), ROOT):
    sys.path.insert(0, p)
import __graft_entry__  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--epochs", type=int, default=10)
ap.add_argument("--L", type=int, default=10)
ap.add_argument("--layer_num", type=int, default=4)
ap.add_argument("--regularization", type=float, default=0.1)
ap.add_argument("--out", default="/tmp/fit2d")
a = ap.parse_args()
__graft_entry__.compile_library_locked()               # before the GPU is initialised

import numpy as np  # noqa: E402
import torch  # noqa: E402
from swnerf import fit2d, runner  # noqa: E402

W, H = 96, 64
ys, xs = np.mgrid[0:H, 0:W]
img = np.stack([0.5 + 0.5 * np.sin(xs / 7.0), 0.5 + 0.5 * np.cos(ys / 5.0), ((xs // 12 + ys // 8) % 2).astype(float)], -1)
os.makedirs(a.out, exist_ok=True)
args = argparse.Namespace(L=a.L, layer_num=a.layer_num, regularization=a.regularization, epochs=a.epochs, picture_dir="synthetic.png",
                          checkpoint_save=a.out, checkpoint_load=None, output_dir=a.out, v=True)
torch.manual_seed(0)
model, optimizer, scheduler, start, _ = runner.create_fit2d(args, device="cuda")
data = fit2d.picture_tensors((255 * img).astype(np.uint8))[:2]
metrics = fit2d.train(data, model, optimizer, scheduler, args, W, H)
path = fit2d.test(W, H, model, args)
pic = fit2d.get_picture(W, H, model, args)
print(f"grey PSNR {float(metrics['PSNR'][-1]):.2f} dB after {a.epochs} epochs; picture mse {float(((pic - img) ** 2).mean()):.5f}; wrote {path}")
