#!/usr/bin/env python3
"""The grouped 256 x 256 weight-gradient launch of one 393 216-row chunk of a training step, alone on the GPU, in both arithmetics
side by side: swnerf_gemm_tn_group (fp32 MFMA) and swnerf_gemm_tn_group_x3 (split-bf16 MFMA; the B2 rider of the skip layer then
goes out as its own fp32 launch).  Six plain items, and the step's seven (six plain + pts_linears.5 with its gamma(x) rider).
ms per call (events around 10+ calls), GB/s on the operand bytes of the main GEMMs.    probe_gemm_group_x3.py [M]"""
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sw-nerf_amd"), ROOT):
    sys.path.insert(0, p)
import torch
from swnerf import _lib, wgrad

dev = torch.device("cuda:0")
L = _lib.lib()
M = int(sys.argv[1]) if len(sys.argv) > 1 else 393216
grad = torch.randn((M, 2432), device=dev)
act = torch.randn((M, 2432), device=dev)
xs = torch.randn((M, 96), device=dev)
C = [torch.zeros((256, 319), device=dev) for _ in range(8)]
bias = [torch.zeros(256, device=dev) for _ in range(8)]
c5s = torch.zeros((256, 64), device=dev)
st = _lib.stream_of(grad)


def group(n_rider):
    def f():
        g = wgrad._Group(st)
        for l in (1, 2, 3, 4, 6, 7):
            wgrad._gemm_tn(L, g, M, grad, 256 * l, 256, act, 256 * (l - 1), 256, C[l], 0, bias[l])
        if n_rider:
            wgrad._gemm_tn_fused(L, g, M, grad, 1280, act, 1024, C[5], 63, bias[5], B2=xs, b2_col=0, Ni2=64, C2=c5s, c2_col=0)
        g.launch(L, M)
    return f


def timeit(f):
    for _ in range(3):
        f()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = 10
    e0.record()
    for _ in range(reps):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


print(f"M = {M} rows")
print("| grouped launch | fp32 ms | bf16x3 ms | fp32 / bf16x3 | bf16x3 GB/s (A and B of the main GEMMs) |")
print("|---|---|---|---|---|")
for name, n_rider, items in (("six plain items", 0, 6), ("the step's seven: six plain + one with the B2 rider", 1, 7)):
    t = {}
    for mode in ("fp32", "bf16x3"):
        wgrad.set_precision(mode)
        t[mode] = timeit(group(n_rider))
    wgrad.set_precision("fp32")
    print(f"| {name} | {t['fp32']:.3f} | {t['bf16x3']:.3f} | {t['fp32'] / t['bf16x3']:.2f} | {items * 2 * M * 1024 / t['bf16x3'] / 1e6:.0f} |")
