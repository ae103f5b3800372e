#!/usr/bin/env python3
"""What the device batch path and runner.train cost, at the blender shape: 100 images of 800 x 800, N_rand 4096, 64 + 128 samples,
static NeRF and D-NeRF.  Prints a markdown table of
  * the time to produce one batch with swnerf_train_batch (RayBatcher.image_batch, device sampler),
  * the time to produce the same kind of batch through the standalone ops, as nerf/run.py:652-681 does: host
    np.random.choice(H * W, N_rand, replace=False), get_rays of the whole image, three gathers, pack_ray_batch,
  * ms per step of runner.train / train_dnerf, against a bare step (tools/bench_train.py's: render + img2mse + backward + Adam) that
    is handed a ready-made batch, each as the mean of GROUPS groups of STEPS steps with the groups' spread (max - min),
  * peak device memory of use_batching (RayBatcher.global_batch) over the images themselves, against the 2.3 GB ray table
    (100 x 640 000 x 36 B) the reference keeps.
  python tools/bench_batching.py [H=800] [n_images=100] [N_rand=4096]"""
import os
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sw-nerf_amd"), ROOT):
    sys.path.insert(0, p)
import numpy as np
import torch
from swnerf import synth, runner, render, render_dnerf, ray, batching

dev = torch.device("cuda:0")
H = W = int(sys.argv[1]) if len(sys.argv) > 1 else 800
N_IMG = int(sys.argv[2]) if len(sys.argv) > 2 else 100
N_RAND = int(sys.argv[3]) if len(sys.argv) > 3 else 4096
GROUPS, STEPS, WARM = 5, 20, 3
focal = float(0.5 * W / np.tan(0.5 * synth.LEGO_CAMERA_ANGLE_X))
K = np.array([[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]])
poses = np.stack([synth.pose_spherical(360.0 * i / N_IMG, -30.0, 4.0) for i in range(N_IMG)]).astype(np.float32)
times = np.linspace(0., 1., N_IMG).astype(np.float32)
images = torch.rand((N_IMG, H, W, 3), device=dev)                                # 768 MB at the default shape
poses_dev = torch.from_numpy(poses).to(dev)
img2mse = lambda x, y: torch.mean((x - y) ** 2)


def args_for(dnerf, tmp, **over):
    a = dict(expname="bench", basedir=tmp, netdepth=8, netwidth=256, netdepth_fine=8, netwidth_fine=256, lrate=5e-4, lrate_decay=500,
             netchunk=1024 * 64, no_reload=True, ft_path=None, N_samples=64, N_importance=128, perturb=1., use_viewdirs=True, i_embed=0,
             multires=10, multires_views=4, raw_noise_std=0., dataset_type="blender", white_bkgd=True, no_ndc=False, lindisp=False,
             chunk=1024 * 32, N_rand=N_RAND, no_batching=True, precrop_iters=0, precrop_frac=.5, i_print=10 ** 9, i_weights=10 ** 9,
             i_testset=10 ** 9, N_iters=WARM + STEPS, N_iter=WARM + STEPS, seed=0, nerf_type="direct_temporal", not_zero_canonical=False,
             use_two_models_for_fine=False, do_half_precision=False, add_tv_loss=False, tv_loss_weight=1e-4, precrop_iters_time=0)
    a.update(over)
    return SimpleNamespace(**a)


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def parent_batch(dnerf, img_i):
    """nerf/run.py:652-681 / run_dnerf.py:657-683 on the standalone ops."""
    target = images[img_i]
    rays_o, rays_d = ray.get_rays(H, W, focal if dnerf else K, poses_dev[img_i, :3, :4])
    select = torch.from_numpy(np.random.choice(H * W, size=[N_RAND], replace=False)).to(dev)
    ys, xs = select // W, select % W
    o, d, target_s = rays_o[ys, xs], rays_d[ys, xs], target[ys, xs]
    return render.pack_ray_batch(o, d, 2., 6., frame_time=float(times[img_i]) if dnerf else None), target_s, (o, d)


def bare_step_groups(dnerf, tmp):
    """The parent's step on a ready-made batch: GROUPS means of STEPS steps."""
    create = runner.create_dnerf if dnerf else runner.create_nerf
    train_kw, _, _, _, opt = create(args_for(dnerf, tmp), device=dev)
    train_kw.update(near=2., far=6.)
    _, target, (o, d) = parent_batch(dnerf, 0)
    rays = torch.stack([o, d], 0)

    def step():
        if dnerf:
            rgb, _, _, extras = render_dnerf.render(H, W, focal, chunk=1024 * 32, rays=rays, frame_time=float(times[1]), retraw=True, **train_kw)
        else:
            rgb, _, _, extras = render.render(H, W, K, chunk=1024 * 32, rays=rays, retraw=True, **train_kw)
        opt.zero_grad()
        loss = img2mse(rgb, target)
        if 'rgb0' in extras:
            loss = loss + img2mse(extras['rgb0'], target)
        loss.backward()
        opt.step()
    return [timed(step, STEPS) for _ in range(GROUPS)]


def train_groups(dnerf, tmp):
    data = (images, poses, poses[:1], [H, W, focal], [list(range(N_IMG)), [], []]) + ((times,) if dnerf else ()) + (2., 6.)
    out = []
    for _ in range(GROUPS):
        mark = {}

        def on_step(i, opt):
            if i == WARM:
                torch.cuda.synchronize()
                mark["t0"] = time.perf_counter()
        (runner.train_dnerf if dnerf else runner.train)(args_for(dnerf, tmp), data, device=dev, hooks={"on_step": on_step})
        torch.cuda.synchronize()
        out.append((time.perf_counter() - mark["t0"]) / STEPS * 1e3)
    return out


tmp = "/tmp/swnerf_bench_batching"
print(f"| {N_IMG} images of {H}x{W}, N_rand {N_RAND}, 64+128 samples, fp32, 1x MI355X | static NeRF | D-NeRF |")
print("|---|---|---|")
rows = {k: [] for k in ("new", "old", "bare", "train")}
for dnerf in (False, True):
    b = batching.RayBatcher(images, poses, [H, W, focal] if dnerf else K, list(range(N_IMG)), 2., 6., times=times if dnerf else None, device=dev)
    step = [0]

    def new_batch():
        step[0] += 1
        return b.image_batch(step[0] % N_IMG, N_RAND, step[0])
    rows["new"].append(timed(new_batch, 200))
    rows["old"].append(timed(lambda: parent_batch(dnerf, 3), 50))
    del b
    rows["bare"].append(bare_step_groups(dnerf, tmp))
    rows["train"].append(train_groups(dnerf, tmp))
fmt = lambda g: f"{np.mean(g):.2f} (spread {max(g) - min(g):.2f})"
print(f"| one batch, swnerf_train_batch (ms) | {rows['new'][0]:.3f} | {rows['new'][1]:.3f} |")
print(f"| one batch, standalone ops + host choice (ms) | {rows['old'][0]:.3f} | {rows['old'][1]:.3f} |")
print(f"| bare step on a ready-made batch (ms/step) | {fmt(rows['bare'][0])} | {fmt(rows['bare'][1])} |")
print(f"| runner.train step, batch and loss included (ms/step) | {fmt(rows['train'][0])} | {fmt(rows['train'][1])} |")
for name, i in (("static", 0), ("D-NeRF", 1)):
    excess = np.mean(rows['train'][i]) - np.mean(rows['bare'][i]) - rows['new'][i]
    spread = max(rows['bare'][i]) - min(rows['bare'][i])
    print(f"{name}: train step - (bare step + batch) = {excess:+.2f} ms; spread of the bare step {spread:.2f} ms; "
          f"bar (excess <= spread) {'met' if excess <= spread else 'NOT met'}; new batch faster than standalone: {rows['new'][i] < rows['old'][i]}")
torch.cuda.empty_cache()
torch.cuda.reset_peak_memory_stats()
base = torch.cuda.memory_allocated()
b = batching.RayBatcher(images, poses, K, list(range(N_IMG)), 2., 6., device=dev)
for _ in range(20):
    b.global_batch(N_RAND)
torch.cuda.synchronize()
print(f"use_batching: peak device memory over the images {((torch.cuda.max_memory_allocated() - base) / 2**20):.2f} MiB "
      f"(the reference's ray table: {N_IMG * H * W * 36 / 1e9:.2f} GB)")
