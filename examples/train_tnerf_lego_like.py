#!/usr/bin/env python3
"""`runner.train_tnerf` end to end with what exists offline: a TEACHER T-NeRF (the seeded synthetic net of swnerf.synth, no
dataset is available) rendered to a handful of small frames on the blender sphere, each at its own frame time, and a STUDENT
with a freshly initialised net trained on those frames by the loop of t_nerf/run_tnerf.py:596-800 - batches drawn and packed
on the device (swnerf.batching), the fused T-NeRF training pass (forward and backward on HIP kernels), Adam, the lr decay, a
checkpoint at the end.  Prints the PSNR of a held-out view / time before and after.

  python examples/train_tnerf_lego_like.py [out_dir] [H=32] [n_train=6] [steps=300]
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


def main(out_dir, H=32, n_train=6, steps=300, device="cuda:0"):
    from swnerf import synth, runner, render_tnerf, cameras
    dev = torch.device(device)
    W = H
    os.makedirs(out_dir, exist_ok=True)
    args = SimpleNamespace(expname="train_tnerf_lego_like", basedir=out_dir, netdepth=8, lrate=5e-4, lrate_decay=500, netchunk=1024 * 64,
                           no_reload=True, ft_path=None, N_samples=64, perturb=1., use_viewdirs=True, i_embed=0, multires=10,
                           multires_views=4, raw_noise_std=0., dataset_type="blender", white_bkgd=True, no_ndc=False, lindisp=False,
                           chunk=1024 * 32, N_rand=min(1024, H * W), no_batching=True, precrop_iters=0, precrop_frac=.5,
                           precrop_iters_time=0, nerf_type="original", do_half_precision=False, fused_train=True,
                           i_print=max(steps // 5, 1), i_weights=steps, i_testset=10 ** 9, N_iter=steps, seed=0)
    H, W, focal = cameras.blender_hwf(H, W, synth.LEGO_CAMERA_ANGLE_X)
    # --- the teacher's frames: n_train views around the sphere at times 0 .. 1, and one held-out view / time between two of them
    _, teacher_kw, _, _, _ = runner.create_tnerf(args, device=dev)
    teacher_kw['network_fn'].load_state_dict({k: torch.from_numpy(v) for k, v in synth.tnerf_state_dict(141).items()})
    teacher_kw.update(near=2., far=6.)
    thetas = [360.0 * i / n_train for i in range(n_train)] + [180.0 / n_train]
    times = np.array([i / max(n_train - 1, 1) for i in range(n_train)] + [0.5 / max(n_train - 1, 1)], np.float32)
    poses = np.stack([synth.pose_spherical(t, -30.0, 4.0) for t in thetas]).astype(np.float32)
    with torch.no_grad():
        images, _ = render_tnerf.render_path(torch.from_numpy(poses).to(dev), [float(t) for t in times], (H, W, focal), args.chunk, teacher_kw)
    images = np.ascontiguousarray(images, dtype=np.float32)
    i_split = [list(range(n_train)), [], [n_train]]
    data = (images, poses, poses[n_train:], [H, W, focal], i_split, times, 2., 6.)

    def held_out_psnr():
        _, test_kw, _, _, _ = runner.create_tnerf(SimpleNamespace(**{**vars(args), "no_reload": False}), device=dev)
        test_kw.update(near=2., far=6.)
        with torch.no_grad():
            rgbs, _ = render_tnerf.render_path(torch.from_numpy(poses[n_train:]).to(dev), [float(times[n_train])], (H, W, focal), args.chunk, test_kw)
        return float(-10. * np.log10(np.mean((rgbs[0] - images[n_train]) ** 2)))

    torch.manual_seed(0)
    np.random.seed(0)
    before = held_out_psnr()                                   # no checkpoint yet: a freshly initialised net
    torch.manual_seed(0)
    record = runner.train_tnerf(args, data, device=dev)        # writes out_dir/train_tnerf_lego_like/{steps:06d}.tar
    after = held_out_psnr()                                    # reloads that checkpoint
    print(f"trained {len(record)} steps of {args.N_rand} rays on {n_train} frames of {H}x{W}: "
          f"loss {record[0]['loss']:.4f} -> {record[-1]['loss']:.4f}")
    print(f"held-out PSNR: before {before:.2f} dB, after {after:.2f} dB")
    return before, after, record


if __name__ == "__main__":
    a = sys.argv
    main(a[1] if len(a) > 1 else os.path.join(os.path.expanduser("~"), "swnerf_train_tnerf_example"), int(a[2]) if len(a) > 2 else 32,
         int(a[3]) if len(a) > 3 else 6, int(a[4]) if len(a) > 4 else 300)
