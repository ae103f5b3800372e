#!/usr/bin/env python3
"""The reference's nerf/extract_mesh.py flow on the MI355X path, end to end, with what exists offline (the counterpart of
render_only_lego_like.py): a checkpoint in the reference's `.tar` format (synthetic seeded weights - no trained lego
checkpoint is available), `create_nerf` with the option names of configs/lego.txt, then `nerf_to_mesh` over
extract_mesh.py's bounds - grid query and marching cubes on the GPU, the field never leaves the device - and `mesh.obj`.
Nothing beyond torch and numpy is needed (no skimage, no trimesh).

  python examples/extract_mesh_lego_like.py [out_dir] [resolution=128] [threshold=0.5]

The reference's default threshold (8) is for trained nets; the seeded net's raw sigma spans about [-2, 2]."""
import os
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sw-nerf_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
import torch

BOUNDS = [(-1., 1.), (-1., 2.), (-4., 2.)]                                # nerf/extract_mesh.py:148


def main(out_dir, resolution=128, threshold=0.5, num_views=100, device="cuda:0"):
    from swnerf import synth, runner, checkpoint, model, mesh
    dev = torch.device(device)
    os.makedirs(out_dir, exist_ok=True)
    # --- a checkpoint as the reference's train() writes it (nerf/run.py:716-724): here from the seeded synthetic nets
    nets = []
    for seed, ab in (synth.NET_COARSE, synth.NET_FINE):
        m = model.vallina_NeRF(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=5, skips=[4], use_viewdirs=True)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.nerf_state_dict(seed, alpha_bias=ab).items()})
        nets.append(m)
    checkpoint.save_checkpoint(out_dir, "lego_like", 200000, 200001, nets[0], nets[1], None)
    # --- what nerf/load_model.py builds from configs/lego.txt: the reloaded fine net is the one extract_mesh.py queries
    args = SimpleNamespace(expname="lego_like", basedir=out_dir, netdepth=8, netwidth=256, netdepth_fine=8, netwidth_fine=256,
                           lrate=5e-4, netchunk=1024 * 64, no_reload=False, ft_path=None, N_samples=64, N_importance=128, perturb=1.,
                           use_viewdirs=True, i_embed=0, multires=10, multires_views=4, raw_noise_std=0., dataset_type="blender",
                           white_bkgd=True, no_ndc=False, lindisp=False, chunk=1024 * 32)
    train_kw, test_kw, start, grad_vars, optimizer = runner.create_nerf(args, device=dev)
    assert start == 200001, "the checkpoint was not reloaded"
    net = test_kw["network_fine"].eval()
    with torch.no_grad():
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        m = mesh.nerf_to_mesh(net, BOUNDS, resolution=resolution, density_threshold=threshold, num_views=num_views)
        torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    path = m.export(os.path.join(out_dir, args.expname, "mesh.obj"))      # extract_mesh.py:186-188
    print(f"{resolution}^3 x {num_views} views -> {len(m.vertices)} vertices, {len(m.faces)} faces in {dt:.3f} s -> {path}")
    return path


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else "/tmp/swnerf_mesh_example"
    R = int(sys.argv[2]) if len(sys.argv) > 2 else 128
    thr = float(sys.argv[3]) if len(sys.argv) > 3 else 0.5
    main(out, R, thr)
