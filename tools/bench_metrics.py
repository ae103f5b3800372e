#!/usr/bin/env python3
"""Throughput of the GPU image metrics (swnerf_image_metrics): N frames of H x W x 3 fp32 in both SSIM
modes, one C-ABI call per batch (4 launches), timed with device events after warm-up.  Prints ONE JSON line:
  ms per batch (median of --repeats) and frames/s; GB/s against the algorithmic minimum (each input read once,
  2 N H W 3 4 B) and against the bytes the two-pass design reads (the stats pass reads both inputs once, the SSIM pass
  every tile with its halo); the fraction of the 6.29 TB/s copy rate; for context the float64 numpy restatement
  (tests/metrics_ref.py) on --cpu-frames frames, and the python-level image_metrics call (chunking included).
  python tools/bench_metrics.py [--frames 200] [--h 800] [--w 800] [--repeats 10] [--warmup 3] [--cpu-frames 1]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sw-nerf_amd"), os.path.join(ROOT, "tests"), ROOT):
    sys.path.insert(0, p)

COPY_RATE = 6.29e12                      # B/s, MI355X device copy rate
TW, TH = 64, 16                          # metrics_kernels.hip MT_TW / MT_TH


def design_bytes(n, h, w, k):
    """bytes the stats pass and the SSIM pass read: both inputs once, then every tile's input rows x columns (halo included)"""
    ho, wo = h - k + 1, w - k + 1
    tile_px = 0
    for y0 in range(0, ho, TH):
        rows = min(TH + k - 1, h - y0)
        for x0 in range(0, wo, TW):
            tile_px += rows * min(TW + k - 1, w - x0)
    return 2 * n * h * w * 3 * 4 + 2 * n * tile_px * 3 * 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--h", type=int, default=800)
    ap.add_argument("--w", type=int, default=800)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-frames", type=int, default=1)
    a = ap.parse_args()
    import numpy as np
    import torch
    from swnerf import _lib, metrics
    import metrics_ref
    assert torch.cuda.is_available(), "bench_metrics needs the MI355X"
    dev = torch.device("cuda:0")
    n, h, w = a.frames, a.h, a.w
    g = torch.Generator(device=dev).manual_seed(0)
    gt = torch.rand((n, h, w, 3), generator=g, device=dev)
    pred = (gt + 0.05 * torch.randn((n, h, w, 3), generator=g, device=dev)).contiguous()
    L = _lib.lib()
    st = _lib.stream_of(gt)
    res = {"tool": "bench_metrics", "frames": n, "h": h, "w": w, "algorithmic_min_bytes": 2 * n * h * w * 3 * 4}
    for name, mode, k in (("skimage", _lib.SSIM_SKIMAGE, 7), ("gauss11", _lib.SSIM_GAUSS11, 11)):
        ws = torch.empty(L.swnerf_metrics_workspace_bytes(n, h, w, mode), dtype=torch.uint8, device=dev)
        outs = [torch.empty(n, dtype=torch.float64, device=dev) for _ in range(4)]

        def call():
            _lib.check(L.swnerf_image_metrics(_lib.ptr(pred), _lib.ptr(gt), n, h, w, mode, _lib.RANGE_GT, 0.0, 1,
                                              _lib.ptr(ws), *[_lib.ptr(o) for o in outs], None, st), "image_metrics")
        for _ in range(a.warmup):
            call()
        torch.cuda.synchronize()
        times = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        ms = float(np.median(times))
        t0 = time.perf_counter()
        r = metrics.image_metrics(pred, gt, mode=name, data_range="gt", clip_pred=True)
        torch.cuda.synchronize()
        py_ms = 1e3 * (time.perf_counter() - t0)
        assert torch.equal(r["ssim"], outs[3]) and torch.equal(r["psnr"], outs[1])
        db = design_bytes(n, h, w, k)
        c = min(a.cpu_frames, n)
        p_h, g_h = pred[:c].cpu().numpy(), gt[:c].cpu().numpy()
        t0 = time.perf_counter()
        ref = metrics_ref.batch(p_h, g_h, metrics_ref.SKIMAGE if mode == _lib.SSIM_SKIMAGE else metrics_ref.GAUSS11,
                                clip_pred=True)
        cpu_ms = 1e3 * (time.perf_counter() - t0) / c
        res[name] = {
            "ms_per_batch": round(ms, 3), "ms_spread": [round(min(times), 3), round(max(times), 3)],
            "frames_per_s": round(n / (ms / 1e3), 1),
            "gbps_vs_algorithmic_min": round(res["algorithmic_min_bytes"] / (ms / 1e3) / 1e9, 1),
            "design_bytes": db, "gbps_vs_design_bytes": round(db / (ms / 1e3) / 1e9, 1),
            "frac_of_copy_rate": round(res["algorithmic_min_bytes"] / (ms / 1e3) / COPY_RATE, 3),
            "python_image_metrics_ms": round(py_ms, 2),
            "cpu_float64_ms_per_frame": round(cpu_ms, 1),
            "max_abs_ssim_err_vs_float64": float(np.abs(outs[3][:c].cpu().numpy() - ref["ssim"]).max()),
            "mean_ssim": float(outs[3].mean()),
        }
        del ws, outs, r
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
