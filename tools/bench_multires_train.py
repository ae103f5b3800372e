#!/usr/bin/env python3
"""What one joint iteration of the MultiRes D-NeRF runner costs with and without the PatchBatcher, at the blender shape: frames of
800 x 800, 4 levels, patches 32 / 16 / 8 / 4 (1360 rays), 64 + 128 samples.  Prints a markdown table of
  * the time to produce the step's data: one swnerf_patch_batch launch against get_rays of a whole frame per level + slices,
  * the time of the loss and its gradients on ready-made colours: one swnerf_multires_loss launch (+ backward) against the
    op-by-op path (F.mse_loss per level, reconstruct_and_compute_loss, autograd),
  * ms per joint step (runner.multires_train_loss + backward + every optimizer's step) with batcher=None and with a batcher, each
    as the mean of GROUPS groups of STEPS steps with the groups' spread (max - min).
  python tools/bench_multires_train.py [H=800] [n_images=20] [netwidth=256]"""
import os
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sw-nerf_amd"), ROOT):
    sys.path.insert(0, p)
import numpy as np
import torch
import torch.nn.functional as F
from swnerf import synth, runner, pyramid, batching
from swnerf.ray import get_rays

dev = torch.device("cuda:0")
H = W = int(sys.argv[1]) if len(sys.argv) > 1 else 800
N_IMG = int(sys.argv[2]) if len(sys.argv) > 2 else 20
WIDTH = int(sys.argv[3]) if len(sys.argv) > 3 else 256
LEVELS, GROUPS, STEPS = 4, 5, 20
focal = float(0.5 * W / np.tan(0.5 * synth.LEGO_CAMERA_ANGLE_X))
poses = torch.from_numpy(np.stack([synth.pose_spherical(360.0 * i / N_IMG, -30.0, 4.0) for i in range(N_IMG)]).astype(np.float32)).to(dev)
times = torch.linspace(0., 1., N_IMG, device=dev)
images = torch.rand((N_IMG, H, W, 3), device=dev)
pyr_images = pyramid.generate_laplacian_pyramid_batch(images, levels=LEVELS)
pyr_hwf = runner.pyramid_hwf([H, W, focal], LEVELS)
patch = runner.multires_patch_sizes(LEVELS)
args = SimpleNamespace(expname="bench", basedir="/nonexistent", layer_num=LEVELS, nerf_type="direct_temporal", netdepth=8, netwidth=WIDTH,
                       netdepth_fine=8, netwidth_fine=WIDTH, use_two_models_for_fine=False, not_zero_canonical=False, lrate=5e-4,
                       netchunk=1024 * 64, chunk=1024 * 32, no_reload=True, ft_path=None, N_samples=64, N_importance=128, perturb=1.,
                       use_viewdirs=True, raw_noise_std=0., dataset_type="blender", white_bkgd=True, no_ndc=False, lindisp=False,
                       do_half_precision=False, global_optimization_epoch=0)
trains, _, _, _, optimizers = runner.create_multires(args, device=dev)
for kw in trains:
    kw.update(near=2., far=6.)
b = batching.PatchBatcher(images, pyr_images, poses, times, pyr_hwf, 2., 6., device=dev)
coords = lambda i: batching.patch_corners(batching.batch_key(0, i, 2), pyr_hwf, 32, i)


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def data_ops(i):
    out = []
    for (H_l, W_l, f_l), (y, x), ps, level in zip(pyr_hwf, coords(i), patch, pyr_images):
        ro, rd = get_rays(H_l, W_l, float(f_l), poses[i % N_IMG, :3, :4])
        out.append((ro[y:y + ps, x:x + ps].reshape(-1, 3), rd[y:y + ps, x:x + ps].reshape(-1, 3), level[i % N_IMG][y:y + ps, x:x + ps]))
    return out


def loss_ops(rgbs, rgb0s, targets, full):
    loss = 0
    for r, r0, t in zip(rgbs, rgb0s, targets):
        loss = loss + F.mse_loss(r.reshape(t.shape), t) + F.mse_loss(r0.reshape(t.shape), t)
    loss = loss + pyramid.reconstruct_and_compute_loss([r.reshape(t.shape).unsqueeze(0) for r, t in zip(rgbs, targets)], full)[1]
    loss.backward()


def joint_groups(batcher):
    step = [0]

    def one():
        step[0] += 1
        i = step[0]
        loss = runner.multires_train_loss(i, i % N_IMG, images, pyr_images, poses, times, pyr_hwf, patch, trains, args,
                                          patch_coords=coords(i), batcher=batcher)[0]
        loss.backward()
        for opt in optimizers:
            opt.step()
            opt.zero_grad()
    return [timed(one, STEPS) for _ in range(GROUPS)]


k = [0]


def new_data():
    k[0] += 1
    return b.batch(k[0] % N_IMG, coords(k[0]), patch)


_, targets, full = b.batch(0, coords(1), patch)
leaves = lambda: [torch.rand(t.numel() // 3, 3, device=dev, requires_grad=True) for t in targets]
rgbs, rgb0s = leaves(), leaves()
fmt = lambda g: f"{np.mean(g):.2f} (spread {max(g) - min(g):.2f})"
print(f"| {N_IMG} frames of {H}x{W}, 4 levels, patches 32/16/8/4, 64+128 samples, width {WIDTH}, fp32, 1x MI355X | op by op | two launches |")
print("|---|---|---|")
print(f"| the step's rays and targets (ms) | {timed(lambda: data_ops(k[0] + 1), 50):.3f} | {timed(new_data, 200):.3f} |")
print(f"| loss + gradients on ready-made colours (ms) | {timed(lambda: loss_ops(rgbs, rgb0s, targets, full), 100):.3f} | "
      f"{timed(lambda: batching.multires_loss(rgbs, rgb0s, targets, full, True)[0].backward(), 100):.3f} |")
print(f"| one joint step (ms/step) | {fmt(joint_groups(None))} | {fmt(joint_groups(b))} |")
