#!/usr/bin/env python3
"""Scoring a render directory with all three numbers of the reference's result tables - PSNR, SSIM and LPIPS - on the GPU.

LPIPS needs two weight files per trunk: torchvision's checkpoint (features.N.weight / .bias) and the lpips package's linear
layers (lin0..4.model.1.weight).  This project ships neither and fetches nothing, so the example writes SEEDED stand-ins in
both formats into <out_dir>/lpips_weights - the numbers it prints are therefore not comparable with published LPIPS values;
point `lpips_weights` (or $SWNERF_LPIPS_DIR) at a directory with the real alexnet-owt-7be5be79.pth / alex.pth and
vgg16-397923af.pth / vgg.pth to get those.

  1. nerf/run.py --render_only --render_test: runner.render_test(..., lpips_weights=dir) renders the test poses of a seeded
     net and writes metrics.json with "psnr", "ssim" and "lpips" (AlexNet, called as the reference calls it), and with video=True
     the reference's video.mp4 as video.avi (Motion-JPEG);
  2. d_nerf/metrics.ipynb: the frames go to estim/ and gt/ as PNGs and runner.evaluate_dir(dir, lpips_weights=dir) writes
     metrics.txt with 'mse', 'psnr', 'ssim' and 'lpips' (VGG, inputs mapped to [-1, 1], the mean over the frames).

  python examples/score_render_dir.py [out_dir] [H=64] [n_poses=3]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sw-nerf_amd"), ROOT, os.path.join(ROOT, "examples")):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np
import torch


def write_seeded_weights(d, seed=0):
    """both trunks in torchvision's key layout and both lin files in the package's: He-normal convolutions, biases of 0.1,
    non-negative lin weights"""
    from swnerf import lpips
    os.makedirs(d, exist_ok=True)
    g = torch.Generator().manual_seed(seed)
    for net in ("alex", "vgg"):
        trunk = {}
        for i, ci, co, k, _, _ in lpips.CONVS[net]:
            trunk[f"features.{i}.weight"] = torch.randn(co, ci, k, k, generator=g) * (2.0 / (ci * k * k)) ** 0.5
            trunk[f"features.{i}.bias"] = torch.full((co,), 0.1)
        lin = {f"lin{j}.model.1.weight": torch.rand(1, c, 1, 1, generator=g) for j, c in enumerate(lpips.tap_channels(net))}
        torch.save(trunk, os.path.join(d, lpips.TRUNK_NAMES[net]))
        torch.save(lin, os.path.join(d, f"{net}.pth"))
    return d


def main(out_dir, H=64, n_poses=3, device="cuda:0"):
    import render_only_lego_like as ro
    from swnerf import synth, runner, cameras, model
    from swnerf.png import write_png
    from swnerf.ray import to8b
    dev = torch.device(device)
    weights = write_seeded_weights(os.path.join(out_dir, "lpips_weights"))
    # the "ground truth": the seeded nets rendered with 64 + 128 samples (examples/render_only_lego_like.py)
    gt, _, _ = ro.main(out_dir, H=H, n_poses=n_poses, device=device)
    # the model under test: the same nets with a quarter of the samples
    nets = []
    for seed, ab in (synth.NET_COARSE, synth.NET_FINE):
        m = model.vallina_NeRF(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=5, skips=[4], use_viewdirs=True)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.nerf_state_dict(seed, alpha_bias=ab).items()})
        nets.append(m.to(dev).eval())
    from types import SimpleNamespace
    args = SimpleNamespace(expname="scored", basedir=out_dir, netdepth=8, netwidth=256, netdepth_fine=8, netwidth_fine=256,
                           lrate=5e-4, netchunk=1024 * 64, no_reload=True, ft_path=None, N_samples=16, N_importance=32, perturb=0.,
                           use_viewdirs=True, i_embed=0, multires=10, multires_views=4, raw_noise_std=0., dataset_type="blender",
                           white_bkgd=True, no_ndc=False, lindisp=False, chunk=1024 * 32)
    _, test_kw, _, _, _ = runner.create_nerf(args, device=dev)
    test_kw["network_fn"].load_state_dict(nets[0].state_dict())
    test_kw["network_fine"].load_state_dict(nets[1].state_dict())
    test_kw.update(near=2., far=6.)
    Hh, W, focal = cameras.blender_hwf(H, H, synth.LEGO_CAMERA_ANGLE_X)
    K = cameras.intrinsics(Hh, W, focal)
    poses = torch.from_numpy(cameras.blender_render_poses(n_poses)).to(dev)
    scored = os.path.join(out_dir, "renderonly_test")
    with torch.no_grad():
        rgbs, m1 = runner.render_test(poses, (Hh, W, focal), K, args.chunk, test_kw, gt, scored, lpips_weights=weights, video=True)
    print("metrics.json:", json.dumps(m1))
    # the notebook's directory layout: estim/ and gt/ ('000.png' is the canonical frame the notebook skips)
    for sub, frames in (("estim", rgbs), ("gt", gt)):
        os.makedirs(os.path.join(scored, sub), exist_ok=True)
        for i, f in enumerate(np.concatenate([frames[:1], frames])):
            write_png(os.path.join(scored, sub, "{:03d}.png".format(i)), to8b(f))
    m2 = runner.evaluate_dir(scored, lpips_weights=weights)
    print("metrics.txt: ", m2)
    return m1, m2, scored


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else "/tmp/swnerf_example"
    main(out, int(sys.argv[2]) if len(sys.argv) > 2 else 64, int(sys.argv[3]) if len(sys.argv) > 3 else 3)
