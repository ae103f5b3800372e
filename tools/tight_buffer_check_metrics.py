#!/usr/bin/env python3
"""Out-of-bounds guard for the image-metrics entry point (swnerf_image_metrics), in the manner of
tools/tight_buffer_check.py: both operands, the workspace and every output end exactly where a torch allocation of at
least 10 MB whose size is a multiple of 2 MB ends (the caching allocator then maps exactly that much), so a read or write
past the last element leaves the mapping and faults instead of touching a neighbour.  Heights and widths are ragged
(not multiples of the 64 x 16 tile, rows not multiples of 16 bytes), so the last tile's halo, the scalar row tails and the
last stats block all reach the end of the operands.
  tight_buffer_check_metrics.py <case> [<case> ...]   cases: {skimage,gauss11}_{map,nomap}
  tight_buffer_check_metrics.py list
tests/test_00_a_metrics_tight_buffers.py starts it as a child process."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sw-nerf_amd"), ROOT):
    sys.path.insert(0, p)
CASES = ["skimage_map", "skimage_nomap", "gauss11_map", "gauss11_nomap"]
if len(sys.argv) < 2 or sys.argv[1] == "list":
    print(" ".join(CASES))
    sys.exit(0)
for c in sys.argv[1:]:
    if c not in CASES:
        raise SystemExit(f"unknown case {c!r}; `list` prints them")

import torch
from swnerf import _lib

dev = torch.device("cuda:0")
MB2 = 2 << 20


def tight_bytes(n):
    return max(10 << 20, (n + MB2 - 1) // MB2 * MB2)


def tail(nbytes, dtype, shape):
    """a tensor of `shape` that ends exactly at the end of a tight allocation"""
    es = torch.empty((), dtype=dtype).element_size()
    buf = torch.empty(tight_bytes(nbytes) // es, dtype=dtype, device=dev)
    n = 1
    for s in shape:
        n *= s
    return buf[buf.numel() - n:].view(shape)


def run(case):
    L = _lib.lib()
    mode = _lib.SSIM_SKIMAGE if case.startswith("skimage") else _lib.SSIM_GAUSS11
    k = 7 if mode == _lib.SSIM_SKIMAGE else 11
    for (n, h, w) in ((3, 517, 389), (2, 211, 1203)):
        shape = (n, h, w, 3)
        # filled from host tensors: no device temporaries whose freed blocks could land inside a later tight allocation
        host_gt = torch.rand(shape)
        host_pred = (host_gt + 0.05 * torch.randn(shape)).float()
        pred = tail(4 * n * h * w * 3, torch.float32, shape)
        gt = tail(4 * n * h * w * 3, torch.float32, shape)
        pred.copy_(host_pred)
        gt.copy_(host_gt)
        wsb = L.swnerf_metrics_workspace_bytes(n, h, w, mode)
        ws = tail(wsb, torch.uint8, (wsb,))
        outs = [tail(8 * n, torch.float64, (n,)) for _ in range(4)]
        mp = tail(4 * n * (h - k + 1) * (w - k + 1) * 3, torch.float32, (n, h - k + 1, w - k + 1, 3)) if case.endswith("_map") else None
        mp_ptr = _lib.ptr(mp) if mp is not None else None
        _lib.check(L.swnerf_image_metrics(_lib.ptr(pred), _lib.ptr(gt), n, h, w, mode, _lib.RANGE_GT, 0.0, 1, _lib.ptr(ws),
                                          *[_lib.ptr(o) for o in outs], mp_ptr, _lib.stream_of(pred)), "image_metrics")
        torch.cuda.synchronize()
        mse, psnr, rng, ssim = (o.cpu() for o in outs)
        assert bool(torch.isfinite(ssim).all()) and bool((ssim > 0.3).all()) and bool((ssim < 1).all()), ssim
        assert bool((mse > 0).all()) and bool((rng > 0.99).all()), (mse, rng)
        if mp is not None:
            m = mp.double().reshape(n, -1).mean(1).cpu()
            assert torch.allclose(m, ssim, atol=1e-6), (m, ssim)
        del pred, gt, ws, outs, mp
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


for c in sys.argv[1:]:
    run(c)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    print(f"{c}: ok", flush=True)
