#!/usr/bin/env python3
"""The MultiRes D-NeRF flow (multires_dnerf/multires_dnerf.py) on the MI355X path with what exists offline: a small
synthetic time-varying image set, its Laplacian pyramid (swnerf.pyramid), one DirectTemporalNeRF per level
(`create_multires`), a few joint iterations (`multires_train_loss`, one Adam per level), a MultiRes checkpoint, and one
frame rendered level by level at pyramid resolution and reconstructed (`render_path_multires(level_hwf="pyramid")`) to PNG.

  python examples/multires_lego_like.py [out_dir] [side=64] [iters=4] [netwidth=64]
"""
import os
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sw-nerf_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np
import torch


def synthetic_scene(n, side, dev):
    """n frames of a smooth pattern that moves with time, on a ring of poses"""
    from swnerf import synth
    yy, xx = np.meshgrid(np.linspace(0, 1, side), np.linspace(0, 1, side), indexing="ij")
    times = np.linspace(0.0, 1.0, n).astype(np.float32)
    imgs = np.stack([np.stack([0.5 + 0.4 * np.sin(6 * xx + 2 * t + c) * np.cos(5 * yy - c) for c in range(3)], -1) for t in times])
    poses = np.stack([synth.pose_spherical(360.0 * i / n, -30.0, 4.0) for i in range(n)]).astype(np.float32)
    return torch.from_numpy(imgs.astype(np.float32)).to(dev), torch.from_numpy(poses).to(dev), torch.from_numpy(times).to(dev)


def main(out_dir, side=64, iters=4, netwidth=64, device="cuda:0"):
    from swnerf import checkpoint, pyramid, runner
    dev = torch.device(device)
    os.makedirs(os.path.join(out_dir, "multires"), exist_ok=True)
    args = SimpleNamespace(expname="multires", basedir=out_dir, layer_num=4, nerf_type="direct_temporal", netdepth=8, netwidth=netwidth,
                           netdepth_fine=8, netwidth_fine=netwidth, use_two_models_for_fine=False, not_zero_canonical=False,
                           lrate=5e-4, netchunk=1024 * 64, chunk=1024 * 32, no_reload=True, ft_path=None, N_samples=16, N_importance=16,
                           perturb=1., use_viewdirs=True, raw_noise_std=0., dataset_type="blender", white_bkgd=True, no_ndc=False,
                           lindisp=False, do_half_precision=False, global_optimization_epoch=2)
    images, poses, times = synthetic_scene(5, side, dev)
    focal = 0.5 * side / np.tan(0.5 * 0.6911112070083618)
    pyr_images = pyramid.generate_laplacian_pyramid_batch(images, levels=args.layer_num)
    pyr_hwf = runner.pyramid_hwf([side, side, focal], args.layer_num)
    trains, tests, starts, grad_vars, optimizers = runner.create_multires(args, device=dev)
    for kw in trains + tests:
        kw.update({"near": 2., "far": 6.})
    patch = [32 // 2 ** l for l in range(args.layer_num)]
    rng = np.random.default_rng(0)
    for i in range(1, iters + 1):
        img_i = int(rng.integers(len(images)))
        loss, per_level, global_loss, global_psnr, _ = runner.multires_train_loss(i, img_i, images, pyr_images, poses, times, pyr_hwf,
                                                                                  patch, trains, args)
        loss.backward()
        for opt in optimizers:
            opt.step()
            opt.zero_grad()
        print(f"[multires] iter {i}: loss {float(loss):.5f}  levels {[round(float(l), 5) for l in per_level]}  "
              f"global {float(global_loss):.5f} ({float(global_psnr):.2f} dB)", flush=True)
    path = checkpoint.save_multires(out_dir, "multires", iters, iters, [kw["network_fn"] for kw in trains],
                                    [kw["network_fine"] for kw in trains], optimizers)
    frames, per_level = runner.render_path_multires(poses[:1], times[2:3], [side, side, focal], args.chunk, tests,
                                                    level_hwf="pyramid", savedir=os.path.join(out_dir, "multires", "testset"))
    print(f"[multires] checkpoint {path}; frame {frames.shape[1:]} from levels {[p.shape[1:3] for p in per_level]} -> "
          f"{os.path.join(out_dir, 'multires', 'testset', 'estim', '000.png')}", flush=True)
    return frames, per_level, path


if __name__ == "__main__":
    a = sys.argv[1:]
    main(a[0] if a else "multires_out", *[int(v) for v in a[1:4]])
