#!/usr/bin/env python3
"""The MultiRes D-NeRF flow (multires_dnerf/multires_dnerf.py) on the MI355X path with what exists offline: a small
synthetic time-varying image set trained through `runner.train_multires` - the Laplacian pyramid (swnerf.pyramid), one
DirectTemporalNeRF per level (`create_multires`), the private phase of every level, the joint iterations on the PatchBatcher
and the fused pyramid loss, MultiRes checkpoints and log.txt - and then one frame rendered level by level at pyramid
resolution and reconstructed (`render_path_multires(level_hwf="pyramid")`) to PNG.

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


def synthetic_scene(n, side):
    """n frames of a smooth pattern that moves with time, on a ring of poses (numpy)"""
    from swnerf import synth
    yy, xx = np.meshgrid(np.linspace(0, 1, side), np.linspace(0, 1, side), indexing="ij")
    times = np.linspace(0.0, 1.0, n).astype(np.float32)
    imgs = np.stack([np.stack([0.5 + 0.4 * np.sin(6 * xx + 2 * t + c) * np.cos(5 * yy - c) for c in range(3)], -1) for t in times])
    poses = np.stack([synth.pose_spherical(360.0 * i / n, -30.0, 4.0) for i in range(n)]).astype(np.float32)
    return imgs.astype(np.float32), poses, times


def main(out_dir, side=64, iters=4, netwidth=64, device="cuda:0"):
    from swnerf import runner
    dev = torch.device(device)
    private = 2
    args = SimpleNamespace(expname="multires", basedir=out_dir, layer_num=4, nerf_type="direct_temporal", netdepth=8, netwidth=netwidth,
                           netdepth_fine=8, netwidth_fine=netwidth, use_two_models_for_fine=False, not_zero_canonical=False,
                           lrate=5e-4, lrate_decay=250, netchunk=1024 * 64, chunk=1024 * 32, no_reload=True, ft_path=None, N_samples=16,
                           N_importance=16, perturb=1., use_viewdirs=True, raw_noise_std=0., dataset_type="blender", white_bkgd=True,
                           no_ndc=False, lindisp=False, do_half_precision=False, global_optimization_epoch=private,
                           N_iter=private + iters, N_rand=32, no_batching=True, precrop_iters=0, precrop_frac=.5, precrop_iters_time=0,
                           add_tv_loss=False, tv_loss_weight=1e-4, i_print=1, i_weights=private + iters, i_testset=10 ** 9, seed=0)
    images, poses, times = synthetic_scene(5, side)
    focal = 0.5 * side / np.tan(0.5 * 0.6911112070083618)
    data = (images, poses, poses[:1], [side, side, focal], [list(range(5)), [], []], times, 2., 6.)
    record = runner.train_multires(args, data, device=dev)
    for r in record["joint"]:
        print(f"[multires] iter {r['step']}: loss {r['loss']:.5f}  levels {[round(l, 5) for l in r['levels']]}  global {r['global_loss']:.5f}",
              flush=True)
    path = os.path.join(out_dir, "multires", '{:06d}.tar'.format(private + iters))
    args.no_reload = False                                          # the nets as the run left them, from its last checkpoint
    _, tests, _, _, _ = runner.create_multires(args, device=dev)
    for kw in tests:
        kw.update({"near": 2., "far": 6.})
    frames, per_level = runner.render_path_multires(torch.from_numpy(poses[:1]).to(dev), torch.from_numpy(times[2:3]).to(dev),
                                                    [side, side, focal], args.chunk, tests, level_hwf="pyramid",
                                                    savedir=os.path.join(out_dir, "multires", "testset"))
    print(f"[multires] checkpoint {path}; frame {frames.shape[1:]} from levels {[p.shape[1:3] for p in per_level]} -> "
          f"{os.path.join(out_dir, 'multires', 'testset', 'estim', '000.png')}", flush=True)
    return frames, per_level, path


if __name__ == "__main__":
    a = sys.argv[1:]
    main(a[0] if a else "multires_out", *[int(v) for v in a[1:4]])
