#!/usr/bin/env python3
"""Throughput of LPIPS on the GPU (swnerf.metrics.LPIPS; DESIGN.md 6f "LPIPS"): --frames pairs of H x W frames through both
trunks, timed with device events after warm-up.  Prints ONE JSON line, per trunk:
  ms for the whole set (median of --repeats) and per frame pair; the multiply-adds the convolutions execute (both images of a
  pair, every layer) and the achieved TFLOP/s on them against the 157.3 TFLOP/s fp32-MFMA peak; per layer, from one chunk timed
  step by step: ms and TFLOP/s of every convolution, ms of every pooling and tap step;
  the same net evaluated with torch.nn.functional.conv2d / max_pool2d (NCHW) on the same device on --torch-frames pairs, ms per
  pair and the largest difference between the two results.
  python tools/bench_lpips.py [--frames 200] [--h 800] [--w 800] [--repeats 3] [--warmup 1] [--torch-frames 2] [--nets alex,vgg]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sw-nerf_amd"), os.path.join(ROOT, "tests"), ROOT):
    sys.path.insert(0, p)

PEAK = 157.3e12                           # fp32 MFMA, FLOP/s


def conv_table(net, h, w):
    """per convolution: (features index, cin, cout, k, stride, pad, h_in, w_in, h_out, w_out, MACs per image)"""
    from swnerf import lpips
    rows = []
    for pos, (i, ci, co, k, s, p) in enumerate(lpips.CONVS[net]):
        win = lpips.POOL_BEFORE[net].get(pos)
        if win:
            h, w = (h - win) // 2 + 1, (w - win) // 2 + 1
        ho, wo = lpips.conv_out(h, k, s, p), lpips.conv_out(w, k, s, p)
        rows.append((i, ci, co, k, s, p, h, w, ho, wo, ho * wo * k * k * ci * co))
        h, w = ho, wo
    return rows


def timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return out, e0.elapsed_time(e1)


def per_layer(model, x, m):
    """one chunk of m pairs, every step timed on its own -> list of (step, ms)"""
    import torch
    from swnerf import lpips
    convs, lins = model._params()[0], model._params()[1]
    steps, tap = [], 0
    total = torch.zeros(m, dtype=torch.float64, device=x.device)
    for pos, (i, _, co, k, s, p) in enumerate(lpips.CONVS[model.net]):
        win = lpips.POOL_BEFORE[model.net].get(pos)
        if win:
            x, ms = timed(lambda: lpips.maxpool2d_nhwc(x, win))
            steps.append((f"pool{win} before features.{i}", ms))
        w, b = convs[pos]
        packed = lpips.pack_conv_weight(model._packs, pos, w)
        x, ms = timed(lambda: lpips.conv2d_nhwc(x, packed, b, co, k, s, p, relu=True))
        steps.append((f"features.{i}", ms))
        if pos in lpips.TAPS[model.net]:
            _, ms = timed(lambda: lpips.lpips_layer(x[:m], x[m:], lins[tap], out=total, accumulate=tap > 0))
            steps.append((f"tap{tap} after features.{i}", ms))
            tap += 1
    return steps


def torch_lpips(net, trunk, lin, a, b):
    """the same graph in torch on the device (NCHW): a, b [m,3,H,W] already normalised to the network's input range"""
    import torch
    import lpips_ref as R
    dev = a.device
    tr = {k: v.to(dev) for k, v in trunk.items()}
    shift = torch.tensor(R.SHIFT, device=dev).view(1, 3, 1, 1)
    scale = torch.tensor(R.SCALE, device=dev).view(1, 3, 1, 1)
    x = (torch.cat([a, b]) - shift) / scale
    val = 0
    for j, t in enumerate(R.taps(net, tr, x)):
        val = val + R.layer(t[:a.shape[0]], t[a.shape[0]:], lin[f"lin{j}.model.1.weight"].to(dev).reshape(-1))
    return val


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--h", type=int, default=800)
    ap.add_argument("--w", type=int, default=800)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--torch-frames", type=int, default=2)
    ap.add_argument("--nets", default="alex,vgg")
    a = ap.parse_args()
    import numpy as np
    import torch
    from swnerf import metrics
    import lpips_ref as R
    assert torch.cuda.is_available(), "bench_lpips needs the MI355X"
    dev = torch.device("cuda:0")
    n, h, w = a.frames, a.h, a.w
    g = torch.Generator(device=dev).manual_seed(0)
    gt = torch.rand((n, h, w, 3), generator=g, device=dev)
    pred = (gt + 0.05 * torch.randn((n, h, w, 3), generator=g, device=dev)).clamp_(0, 1)
    res = {"tool": "bench_lpips", "frames": n, "h": h, "w": w, "peak_tflops": PEAK / 1e12}
    for net in a.nets.split(","):
        trunk, lin = R.seeded_weights(net)
        model = metrics.LPIPS(net, weights=(trunk, lin), device=dev)
        table = conv_table(net, h, w)
        macs = 2 * n * sum(r[-1] for r in table)
        call = lambda: model(pred, gt, normalize=True, layout="nhwc")
        for _ in range(a.warmup):
            call()
        torch.cuda.synchronize()
        times = []
        for _ in range(a.repeats):
            out, ms = timed(call)
            times.append(ms)
        ms = float(np.median(times))
        chunk = min(n, max(1, (1 << 30) // model.live_bytes(h, w)))
        print(f"[bench_lpips] {net}: {ms:.1f} ms for {n} pairs, chunks of {chunk}", file=sys.stderr, flush=True)
        x = torch.cat([pred[:chunk], gt[:chunk]])
        x = (((2 * x - 1) - model._params()[2]) / model._params()[3]).contiguous()
        per_layer(model, x, chunk)                                             # warm
        steps = per_layer(model, x, chunk)
        by_index = {f"features.{r[0]}": r for r in table}
        layers = []
        for name, t in steps:
            row = {"step": name, "ms_per_chunk": round(t, 4)}
            if name in by_index:
                r = by_index[name]
                row.update({"cin": r[1], "cout": r[2], "kernel": r[3], "stride": r[4], "pad": r[5], "in_hw": [r[6], r[7]], "out_hw": [r[8], r[9]],
                            "gmac_per_image": round(r[-1] / 1e9, 4), "tflops": round(2 * 2 * chunk * r[-1] / (t / 1e3) / 1e12, 2)})
            layers.append(row)
        entry = {"ms": round(ms, 2), "ms_spread": [round(min(times), 2), round(max(times), 2)], "ms_per_pair": round(ms / n, 4),
                 "gmac_per_pair": round(macs / n / 1e9, 3), "tflop_total": round(2 * macs / 1e12, 3),
                 "tflops": round(2 * macs / (ms / 1e3) / 1e12, 2), "frac_of_peak": round(2 * macs / (ms / 1e3) / PEAK, 3),
                 "chunk_pairs": chunk, "mean_lpips": float(out.mean()), "layers": layers}
        m = min(a.torch_frames, n)
        if m > 0:
            pa, pb = (2 * pred[:m] - 1).permute(0, 3, 1, 2).contiguous(), (2 * gt[:m] - 1).permute(0, 3, 1, 2).contiguous()
            with torch.no_grad():
                torch_lpips(net, trunk, lin, pa, pb)                           # warm (the library picks its kernels here)
                torch.cuda.synchronize()
                ref, tms = timed(lambda: torch_lpips(net, trunk, lin, pa, pb))
            entry["torch_conv2d"] = {"pairs": m, "ms_per_pair": round(tms / m, 4), "speedup": round((tms / m) / (ms / n), 2),
                                     "max_abs_diff": float((ref.double() - out[:m].reshape(-1).double()).abs().max())}
            print(f"[bench_lpips] {net}: torch conv2d {tms / m:.2f} ms per pair", file=sys.stderr, flush=True)
        res[net] = entry
        del model
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
