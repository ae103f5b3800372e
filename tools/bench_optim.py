#!/usr/bin/env python3
"""The optimizer phase alone: torch.optim.Adam with its defaults, torch.optim.Adam(fused=True) and swnerf.optim.Adam (AdamW for the
fit2d set) on the parameter sets of the runners, gradients in place, nothing else on the GPU.
  (a) nerf    coarse + fine vallina_NeRF 8 x 256                       (runner.create_nerf)
  (b) dnerf   the D-NeRF pair (DirectTemporalNeRF 8 x 256) x 2         (create_dnerf with use_two_models_for_fine)
  (c) fit2d   fit2d.Model(2 + 4 * 20, 10), AdamW                       (create_fit2d)
Per optimizer: GPU time of step() between two device events and host time of the step() call (perf_counter around the call, no
synchronise inside), each the median of 10 after 3 warm-up steps.  Then ONE tensor of 64 Mi floats: the step's GB/s (7 arrays of
4 bytes move per element: p, g, m, v read, p, m, v written) beside Tensor.copy_ of the same tensor (2 arrays) in the same run.
  python tools/bench_optim.py [--json out.json]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sw-nerf_amd"), ROOT):
    sys.path.insert(0, p)
import __graft_entry__ as ge

ge.compile_library_locked()                     # before the GPU is initialised
import torch
from swnerf import fit2d, model, optim

assert torch.cuda.is_available(), "bench_optim.py needs the MI355X"
DEV = torch.device("cuda:0")
WARMUP, REPS = 3, 10


def timed(fn):
    """-> (median GPU ms, median host ms) of fn() over REPS after WARMUP"""
    gpu, host = [], []
    for k in range(WARMUP + REPS):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        e1.record()
        torch.cuda.synchronize()
        if k >= WARMUP:
            gpu.append(e0.elapsed_time(e1))
            host.append((t1 - t0) * 1e3)
    return statistics.median(gpu), statistics.median(host)


def param_sets():
    net = dict(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=5, skips=[4], use_viewdirs=True)
    nerf = [p for _ in range(2) for p in model.vallina_NeRF(**net).to(DEV).parameters()]
    dnerf = [p for _ in range(2) for p in model.DirectTemporalNeRF(input_ch_time=21, **net).to(DEV).parameters()]
    f2d = list(fit2d.Model(input_dimension=2 + 4 * 20, layer_num=10).to(DEV).parameters())
    return {"nerf": (nerf, False), "dnerf": (dnerf, False), "fit2d": (f2d, True)}


def optimizers(params, adamw):
    kw = dict(lr=1e-3) if adamw else dict(lr=5e-4, betas=(0.9, 0.999))
    t = torch.optim.AdamW if adamw else torch.optim.Adam
    return {"torch": t(params, **kw), "torch_fused": t(params, fused=True, **kw), "swnerf": (optim.AdamW if adamw else optim.Adam)(params, **kw)}


def main():
    torch.manual_seed(0)
    out = {"sets": {}, "large": {}}
    for name, (params, adamw) in param_sets().items():
        for p in params:
            p.grad = torch.randn_like(p) * 1e-3
        row = {"tensors": len(params), "floats": sum(p.numel() for p in params), "launches": len({r[0] for r in optim.launch_plan([p.numel() for p in params])})}
        for which, opt in optimizers(params, adamw).items():
            g, h = timed(opt.step)
            row[which] = {"gpu_ms": g, "host_ms": h}
        out["sets"][name] = row
        print(f"{name}: {row['tensors']} tensors, {row['floats']} floats, {row['launches']} fused launches | " +
              " | ".join(f"{w} gpu {row[w]['gpu_ms'] * 1e3:.1f} us host {row[w]['host_ms'] * 1e3:.1f} us" for w in ("torch", "torch_fused", "swnerf")), flush=True)
    n = 1 << 26
    big = torch.nn.Parameter(torch.randn(n, device=DEV))
    big.grad = torch.randn(n, device=DEV) * 1e-3
    dst = torch.empty(n, device=DEV)
    g, _ = timed(lambda: dst.copy_(big.detach()))
    out["large"]["copy_"] = {"gpu_ms": g, "GBps": 2 * 4 * n / g / 1e6}
    for which, opt in optimizers([big], False).items():
        g, h = timed(opt.step)
        out["large"][which] = {"gpu_ms": g, "host_ms": h, "GBps": 7 * 4 * n / g / 1e6}
        del opt
    print("64 Mi floats: " + " | ".join(f"{w} {v['gpu_ms']:.3f} ms {v['GBps']:.0f} GB/s" for w, v in out["large"].items()), flush=True)
    print(json.dumps(out))
    if "--json" in sys.argv:
        path = sys.argv[sys.argv.index("--json") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
