#!/usr/bin/env python3
"""Mesh extraction of a DYNAMIC scene on the MI355X path (the counterpart of extract_mesh_lego_like.py for d_nerf/): a seeded
DirectTemporalNeRF (synthetic weights - no trained D-NeRF checkpoint is available offline), then `mesh_sequence` over
extract_mesh.py's bounds at three frame times - per time one fused grid query (deformation net, gamma(x + dx), canonical trunk
once per point, the view branch per direction) and one marching-cubes pass on the GPU - and one OBJ per time.
Nothing beyond torch and numpy is needed (no skimage, no trimesh).

  python examples/extract_mesh_dnerf_like.py [out_dir] [resolution=64] [num_views=100] [threshold=0.0]

The reference's default threshold (8) is for trained nets; the seeded net's raw sigma spans about [-1.3, 1.7]."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sw-nerf_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
import torch

BOUNDS = [(-1., 1.), (-1., 2.), (-4., 2.)]                                # nerf/extract_mesh.py:148
TIMES = (0.0, 0.5, 1.0)


def main(out_dir, resolution=64, num_views=100, threshold=0.0, times=TIMES, device="cuda:0"):
    from swnerf import synth, model, embedder, mesh
    dev = torch.device(device)
    embed_fn, input_ch = embedder.get_embedder(10, 3, 0)
    net = model.DirectTemporalNeRF(D=8, W=256, input_ch=input_ch, input_ch_views=27, input_ch_time=21, output_ch=5, skips=[4],
                                   use_viewdirs=True, embed_fn=embed_fn, zero_canonical=True)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.dnerf_state_dict(synth.NET_DNERF[0], alpha_bias=synth.NET_DNERF[1]).items()})
    net = net.to(dev).eval()
    with torch.no_grad():
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        meshes = mesh.mesh_sequence(net, BOUNDS, times, resolution=resolution, density_threshold=threshold, num_views=num_views,
                                    out_dir=out_dir)
        torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    paths = [os.path.join(out_dir, "mesh_{:03d}.obj".format(i)) for i in range(len(meshes))]
    for t, m, p in zip(times, meshes, paths):
        print(f"t = {t}: {resolution}^3 x {num_views} views -> {len(m.vertices)} vertices, {len(m.faces)} faces -> {p}")
    print(f"{len(meshes)} meshes in {dt:.3f} s")
    return paths


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else "/tmp/swnerf_mesh_dnerf_example"
    R = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    V = int(sys.argv[3]) if len(sys.argv) > 3 else 100
    thr = float(sys.argv[4]) if len(sys.argv) > 4 else 0.0
    main(out, R, V, thr)
