#!/usr/bin/env python3
"""Throughput of the Laplacian-pyramid kernels (csrc/pyramid_kernels.hip) at N frames of H x W x 3 fp32 and
`levels` levels, timed with device events after warm-up.  Prints ONE JSON line:
  per kernel at level 0 (down, up_axpy with a base, up_adjoint): ms (median of --repeats) and GB/s on the minimal byte
    count (every operand read once, every output written once), next to a float4 device copy measured in the same run
    and the 6.29 TB/s copy rate tools/bench_satellites.py reports;
  per operation (generate, reconstruct, reconstruct forward + backward through autograd): ms and GB/s on the minimal
    bytes of the whole operation, and the same operation written with F.conv2d / F.interpolate on torch (NCHW views of
    the same NHWC data, as the reference does it);
  with --frame-side S: one render_path_multires frame of S x S in both level_hwf modes (four width-256 level nets).
  python tools/bench_pyramid.py [--frames 200] [--h 800] [--w 800] [--levels 4] [--repeats 10] [--warmup 3] [--frame-side 400]"""
import argparse
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sw-nerf_amd"), ROOT):
    sys.path.insert(0, p)

COPY_RATE = 6.29e12                      # B/s, what a float4 device copy reaches on this part (tools/bench_satellites.py)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--h", type=int, default=800)
    ap.add_argument("--w", type=int, default=800)
    ap.add_argument("--levels", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frame-side", type=int, default=0)
    a = ap.parse_args()
    import numpy as np
    import torch
    import torch.nn.functional as F
    from swnerf import pyramid, runner, synth
    assert torch.cuda.is_available(), "bench_pyramid needs the MI355X"
    dev = torch.device("cuda:0")
    n, h, w, c, levels = a.frames, a.h, a.w, 3, a.levels

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms))

    def entry(ms, nbytes):
        return {"ms": round(ms, 4), "min_bytes": int(nbytes), "GBps": round(nbytes / ms / 1e6, 1),
                "of_copy_rate": round(nbytes / (ms * 1e-3) / COPY_RATE, 3)}

    px = [n * (h >> l) * (w >> l) * c * 4 for l in range(levels)]            # bytes of one image set per level
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.rand((n, h, w, c), generator=g, device=dev)
    res = {"tool": "bench_pyramid", "frames": n, "h": h, "w": w, "levels": levels}

    y = torch.empty_like(x)
    res["copy"] = entry(timed(lambda: y.copy_(x)), 2 * px[0])
    del y

    wt = pyramid.create_gaussian_kernel(3, 1.0, 1).reshape(-1).to(dev)
    res["down"] = entry(timed(lambda: pyramid.down(x, wt, 3)), px[0] + px[1])
    coarse = pyramid.down(x, wt, 3)
    res["up_axpy"] = entry(timed(lambda: pyramid.up_axpy(coarse, (h, w), base=x, alpha=-1.0)), px[1] + 2 * px[0])
    res["up_adjoint"] = entry(timed(lambda: pyramid.up_adjoint(x, (h >> 1, w >> 1))), px[0] + px[1])
    del coarse

    # whole operations.  generate: level l reads g_l twice (down, subtract) in the minimal two-kernel form counted ONCE here (the
    # algorithmic minimum: input read once, every level written once); reconstruct: every level read once, the frame written once
    gen_bytes = px[0] + sum(px)
    rec_bytes = sum(px) + px[0]
    res["generate"] = entry(timed(lambda: pyramid.generate_laplacian_pyramid_batch(x, levels=levels)), gen_bytes)
    pyr = pyramid.generate_laplacian_pyramid_batch(x, levels=levels)
    res["reconstruct"] = entry(timed(lambda: pyramid.reconstruct_image_from_pyramid_batch(pyr)), rec_bytes)

    def fwd_bwd(rec, lv):
        for l in lv:
            l.grad = None
        rec(lv).backward(gradient=x)                                         # upstream gradient: any frame-sized tensor

    lv = [p.clone().requires_grad_(True) for p in pyr]
    res["reconstruct_fwd_bwd"] = entry(timed(lambda: fwd_bwd(pyramid.reconstruct_image_from_pyramid_batch, lv)), 2 * rec_bytes)
    del lv

    # the same operations on torch ops, as the reference writes them (NCHW views of the NHWC data)
    kern = pyramid.create_gaussian_kernel(3, 1.0, c).to(dev)

    def t_generate(img):
        gs = [img.permute(0, 3, 1, 2)]
        for _ in range(levels - 1):
            gs.append(F.interpolate(F.conv2d(gs[-1], kern, padding=1, groups=c), scale_factor=0.5, mode="bilinear", align_corners=False))
        return [(gs[i] - F.interpolate(gs[i + 1], size=gs[i].shape[2:], mode="bilinear", align_corners=False)).permute(0, 2, 3, 1)
                for i in range(levels - 1)] + [gs[-1].permute(0, 2, 3, 1)]

    def t_reconstruct(lv_):
        r = lv_[-1].permute(0, 3, 1, 2)
        for i in range(len(lv_) - 2, -1, -1):
            r = F.interpolate(r, size=lv_[i].shape[1:3], mode="bilinear", align_corners=False) + lv_[i].permute(0, 3, 1, 2)
        return r.permute(0, 2, 3, 1)

    with torch.no_grad():
        res["torch_generate"] = entry(timed(lambda: t_generate(x)), gen_bytes)
        res["torch_reconstruct"] = entry(timed(lambda: t_reconstruct(pyr)), rec_bytes)
    lv = [p.clone().requires_grad_(True) for p in pyr]
    res["torch_reconstruct_fwd_bwd"] = entry(timed(lambda: fwd_bwd(t_reconstruct, lv)), 2 * rec_bytes)
    del lv, pyr, x
    torch.cuda.empty_cache()

    if a.frame_side:
        s = a.frame_side
        args = types.SimpleNamespace(layer_num=4, use_viewdirs=True, N_importance=128, N_samples=64, nerf_type="direct_temporal",
                                     netdepth=8, netwidth=256, netdepth_fine=8, netwidth_fine=256, use_two_models_for_fine=False,
                                     not_zero_canonical=False, netchunk=1 << 16, lrate=5e-4, basedir="", expname="", ft_path=None,
                                     no_reload=True, perturb=0.0, white_bkgd=True, raw_noise_std=0.0, dataset_type="blender",
                                     no_ndc=False, lindisp=False, do_half_precision=False)
        torch.manual_seed(0)
        _, tests, *_ = runner.create_multires(args, device=dev)
        for kw in tests:
            kw.update({"near": 2.0, "far": 6.0})
        pose = torch.from_numpy(synth.pose_spherical(30.0, -30.0, 4.0)).to(dev)[None]
        tms = torch.tensor([0.5], device=dev)
        focal = 0.5 * s / np.tan(0.5 * 0.6911112070083618)
        for mode in ("pyramid", "reference"):
            runner.render_path_multires(pose, tms, [s // 4, s // 4, focal / 4], 1 << 15, tests, level_hwf=mode)      # warm-up, small
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            runner.render_path_multires(pose, tms, [s, s, focal], 1 << 15, tests, level_hwf=mode)
            torch.cuda.synchronize()
            res[f"frame_{mode}_s"] = round(time.perf_counter() - t0, 3)
        res["frame_side"] = s
    print(json.dumps(res))


if __name__ == "__main__":
    main()
