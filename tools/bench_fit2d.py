#!/usr/bin/env python3
"""Timing of 2-D image fitting on the MI355X: get_picture at the reference's two picture sizes, and one
training step at batch 512 (forward / backward / AdamW) against the same step in plain torch ops (tests/fit2d_ref.py's
module on the GPU).  Warm-up, then the median of 20 timed runs (device events around each run).  Prints one JSON line.
  python tools/bench_fit2d.py [--runs 20] [--warmup 5]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sw-nerf_amd"), ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import __graft_entry__  # noqa: E402

PEAK_TFLOPS = 157.3                                   # fp32 MFMA at 2.4 GHz
MACS_PER_PIXEL = 24576 + 9 * 65536                    # executed: layer 0 on three k-tiles (96 x 256), nine 256 x 256 layers


def median_ms(fn, runs, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    __graft_entry__.compile_library_locked()           # before the GPU is initialised
    import torch
    import fit2d_ref as R
    from swnerf import fit2d, synth
    dev = torch.device("cuda:0")
    L, n = 20, 10
    sd = synth.fit2d_state_dict(1601, 4 * L + 2, n)
    model = fit2d.Model(4 * L + 2, n)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    model = model.to(dev).eval()
    res = {"peak_tflops": PEAK_TFLOPS, "macs_per_pixel": MACS_PER_PIXEL, "runs": a.runs, "picture": [], "train_step": {}}
    for W, H in ((1368, 1080), (2273, 1279)):
        blob = model.packed()
        out = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
        from swnerf import _lib
        lib, st = _lib.lib(), _lib.stream_of(out)
        run = lambda: _lib.check(lib.swnerf_fit2d_picture(_lib.ptr(blob), H, W, L, n, _lib.ptr(out), None, st), "fit2d_picture")
        med, lo, hi = median_ms(run, a.runs, a.warmup)
        tflops = 2 * MACS_PER_PIXEL * H * W / (med * 1e-3) / 1e12
        res["picture"].append({"width": W, "height": H, "ms": round(med, 3), "ms_min": round(lo, 3), "ms_max": round(hi, 3),
                               "mpixels_per_s": round(H * W / (med * 1e-3) / 1e6, 2), "tflops": round(tflops, 2),
                               "roofline": round(tflops / PEAK_TFLOPS, 4)})
    # the training step on one fixed batch of 512
    g = torch.Generator().manual_seed(1)
    x = (torch.rand(512, 4 * L + 2, generator=g) * 2 - 1).to(dev)
    tgt = torch.rand(512, 3, generator=g).to(dev)
    for name in ("hip", "torch"):
        torch.manual_seed(0)
        if name == "hip":
            m = fit2d.Model(4 * L + 2, n).to(dev).train()
            lossf = lambda o: fit2d.fit_loss(o, tgt, 0.1)[0]
        else:
            m = R.module(4 * L + 2, n, 256, 3, dtype=torch.float32, device=dev).train()
            lossf = lambda o: R.loss(o, tgt, 0.1)
        opt = torch.optim.AdamW(m.parameters(), lr=0.001)

        def step():
            opt.zero_grad()
            lossf(m(x)).backward()
            opt.step()
        med, lo, hi = median_ms(step, a.runs, a.warmup)
        res["train_step"][name] = {"ms": round(med, 3), "ms_min": round(lo, 3), "ms_max": round(hi, 3)}
    res["train_step"]["hip_over_torch"] = round(res["train_step"]["hip"]["ms"] / res["train_step"]["torch"]["ms"], 3)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
