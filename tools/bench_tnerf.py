#!/usr/bin/env python3
"""T-NeRF throughput on one MI355X; prints ONE JSON line.
  fused pass (csrc/tnerf_kernels.hip) and op path (TNeRF.forward on the generic GEMMs): rays/s at 4096 rays x 64 samples and
  for a 400x400 frame (t_nerf/configs/lego.txt: half_res, 64 samples, white_bkgd); the fused pass's fraction of the fp32 MFMA
  roofline (157.3 TF) counted on the EXECUTED MACs (139 264 per sample + the per-ray prefix), the reference's count beside it;
  the op-path training step (ms, peak GiB) at N_rand 500 and 4096.
  --train: the training step alone, the op path and the fused training pass (render_tnerf.fused_train) side by side in the same
  process at N_rand 500 and 4096 x 64 samples: median of --reps steps after 3 warm-up steps, peak memory of each, their ratio, and
  the fused step's share of the fp32 MFMA roofline on its EXECUTED MACs (forward + dX chain + weight-gradient GEMMs).
Run: python tools/bench_tnerf.py [--reps 20] [--train]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "sw-nerf_amd"), ROOT]

PEAK = 157.3e12
MACS_EXEC = 139264            # per sample: layer 0 64x128, 6 x 128x128, layer 5 192x128, folded layer_9 128x64
MACS_PREFIX = 2 * 32 * 128 + 32 * 64   # per ray: the gamma(t) columns of layers 0 and 5, the gamma(d) columns of layer_9 (padded k-tiles)
MACS_REF = 162816             # the reference's per-sample count
MACS_BWD_DX = 480 * 4 * 2048 // 32     # per sample: the dX chain's 480 steps (W9f^T 4x2, layers.7..1 4x4) of four 32x32x2 MFMAs per 32-sample tile
MACS_BWD_DW = 7 * 128 * 128 + 2 * 128 * 96 + 64 * 128 + 64 * 32 + 4 * 128 + 4 * 64   # per sample: the weight-gradient GEMMs (wgrad.py kind "tnerf")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--train", action="store_true", help="time the op-path and the fused training step side by side")
    a = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    import numpy as np
    import torch
    from swnerf import synth, render_tnerf
    from swnerf.model import TNeRF
    from swnerf.embedder import get_embedder
    dev = torch.device("cuda:0")
    net = TNeRF(8, 63, 27, 21).to(dev)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.tnerf_state_dict(141).items()})
    embed_fn, _ = get_embedder(10, 3, 0)            # these names: tnerf_plan finds the encoders in the closure by them
    embedtime_fn, _ = get_embedder(10, 1, 0)
    embeddirs_fn, _ = get_embedder(4, 3, 0)
    q = lambda inputs, viewdirs, ts, network_fn: render_tnerf.run_network(inputs, viewdirs, ts, network_fn, embed_fn=embed_fn,
                                                                         embeddirs_fn=embeddirs_fn, embedtime_fn=embedtime_fn, netchunk=1024 * 64)
    K, c2w = synth.lego_camera(400, 400)

    def rays(n, seed=1):
        o, d = synth.pick_rays(400, 400, K, c2w, n, seed) if n < 160000 else synth.rays_numpy(400, 400, K, c2w)
        o, d = torch.from_numpy(np.ascontiguousarray(o)).reshape(-1, 3).to(dev), torch.from_numpy(np.ascontiguousarray(d)).reshape(-1, 3).to(dev)
        one = torch.ones_like(d[:, :1])
        return torch.cat([o, d, 2 * one, 6 * one, 0.5 * one, d / d.norm(dim=-1, keepdim=True)], -1).contiguous()

    def timeit(fn, reps):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts))

    if a.train:
        res = {"metric": "tnerf_train", "reps": a.reps, "macs_exec_per_sample_step": MACS_EXEC + MACS_BWD_DX + MACS_BWD_DW}
        opt = torch.optim.Adam(net.parameters(), lr=5e-4)
        for n in (500, 4096):
            rb = rays(n, seed=2)
            tgt = torch.full((n, 3), 0.5, device=dev)

            def step(fused):
                with render_tnerf.fused_train(fused):
                    out = render_tnerf.render_rays(rb, net, q, 64, perturb=1., white_bkgd=True)
                loss = ((out["rgb_map"] - tgt) ** 2).mean()
                opt.zero_grad()
                loss.backward()
                opt.step()
            for tag, fused in (("op", False), ("fused", True)):
                for _ in range(3):
                    step(fused)
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                res[f"{tag}_{n}_ms"] = timeit(lambda: step(fused), a.reps) * 1e3
                res[f"{tag}_{n}_peak_gib"] = torch.cuda.max_memory_allocated() / 2 ** 30
            res[f"speedup_{n}"] = res[f"op_{n}_ms"] / res[f"fused_{n}_ms"]
            res[f"fused_{n}_roofline"] = 2 * (MACS_EXEC + MACS_BWD_DX + MACS_BWD_DW) * 64 * n / (res[f"fused_{n}_ms"] * 1e-3) / PEAK
        print(json.dumps(res), flush=True)
        return
    res = {"metric": "tnerf", "macs_exec_per_sample": MACS_EXEC, "macs_ref_per_sample": MACS_REF}
    # the op path in ONE network call (netchunk None): with the reference's 65536 a 400x400 frame's 10.24 M rows leave a ragged
    # last chunk, which batchify's torch.cat rejects exactly as the reference does
    encs = (embed_fn, embeddirs_fn, embedtime_fn)
    plain = lambda inputs, viewdirs, ts, network_fn: render_tnerf.run_network(inputs, viewdirs, ts, network_fn, embed_fn=encs[0],
                                                                             embeddirs_fn=encs[1], embedtime_fn=encs[2], netchunk=None)
    with torch.no_grad():
        assert render_tnerf.tnerf_plan(q, net) == (10, 4, 10) and render_tnerf.tnerf_plan(plain, net) is None
    for tag, n in (("4096", 4096), ("frame400", 160000)):
        rb = rays(n)
        with torch.no_grad():
            t = timeit(lambda: render_tnerf.render_rays(rb, net, q, 64, white_bkgd=True), a.reps)
            res[f"fused_{tag}_ms"] = t * 1e3
            res[f"fused_{tag}_rays_per_s"] = n / t
            res[f"fused_{tag}_roofline"] = 2 * (MACS_EXEC * 64 + MACS_PREFIX) * n / t / PEAK
            t = timeit(lambda: render_tnerf.render_rays(rb, net, plain, 64, white_bkgd=True), max(3, a.reps // 4))
            res[f"op_{tag}_rays_per_s"] = n / t
    opt = torch.optim.Adam(net.parameters(), lr=5e-4)
    for n in (500, 4096):
        rb = rays(n, seed=2)
        tgt = torch.full((n, 3), 0.5, device=dev)

        def step():
            out = render_tnerf.render_rays(rb, net, q, 64, perturb=1., white_bkgd=True)
            loss = ((out["rgb_map"] - tgt) ** 2).mean()
            opt.zero_grad()
            loss.backward()
            opt.step()
        torch.cuda.reset_peak_memory_stats()
        res[f"train_{n}_ms"] = timeit(step, max(3, a.reps // 2)) * 1e3
        res[f"train_{n}_peak_gib"] = torch.cuda.max_memory_allocated() / 2 ** 30
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
