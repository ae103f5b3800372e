#!/usr/bin/env python3
"""Out-of-bounds guard for the Laplacian-pyramid entry points (swnerf_pyramid_down / _up_axpy / _up_adjoint), in the manner
of tools/tight_buffer_check_metrics.py: every operand and every output ends exactly where a torch allocation of at least
10 MB whose size is a multiple of 2 MB ends (the caching allocator then maps exactly that much), so a read or write past
the last element leaves the mapping and faults instead of touching a neighbour.  Sizes are ragged and odd (17 x 31,
9 x 13, 37 x 53: rows that are no multiple of 16 bytes, a dropped last row and column), so the blur taps, the `+1`
neighbour of the upsample, the 4-float runs and the gather ranges of the adjoint all reach the end of their operands.
Every result is compared with the same call on ordinary allocations, bit for bit.
  tight_buffer_check_pyramid.py <case> [<case> ...]
  tight_buffer_check_pyramid.py list
tests/test_00_a_pyramid_tight_buffers.py starts it as a child process."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sw-nerf_amd"), ROOT):
    sys.path.insert(0, p)
CASES = ["down_k3", "down_k5", "up_axpy_base", "up_axpy_nobase", "up_axpy_same_size", "up_adjoint"]
if len(sys.argv) < 2 or sys.argv[1] == "list":
    print(" ".join(CASES))
    sys.exit(0)
for c in sys.argv[1:]:
    if c not in CASES:
        raise SystemExit(f"unknown case {c!r}; `list` prints them")

import torch
from swnerf import _lib, pyramid

dev = torch.device("cuda:0")
MB2 = 2 << 20
SHAPES = [(2, 17, 31, 3), (3, 9, 13, 3), (1, 37, 53, 4), (2, 16, 20, 1)]


def tail(host):
    """a device copy of `host` that ends exactly at the end of a tight allocation"""
    n = host.numel()
    buf = torch.empty(max(10 << 20, (4 * n + MB2 - 1) // MB2 * MB2) // 4, dtype=torch.float32, device=dev)
    t = buf[buf.numel() - n:].view(host.shape)
    t.copy_(host)
    return t


def run(case):
    L = _lib.lib()
    g = torch.Generator().manual_seed(len(case))
    for (n, h, w, c) in SHAPES:
        H, W = 2 * h + 1, 2 * w + 1                          # the fine side of the upsample cases: odd, not 2x
        if case.startswith("down"):
            k = int(case[-1])
            x = torch.rand((n, h, w, c), generator=g)
            wt = pyramid.create_gaussian_kernel(k, 1.0, 1).reshape(-1)
            call = lambda x_, wt_, out: L.swnerf_pyramid_down(_lib.ptr(x_), n, h, w, c, _lib.ptr(wt_), k, _lib.ptr(out), _lib.stream_of(out))
            ins, out_shape = [x, wt], (n, h // 2, w // 2, c)
        elif case == "up_adjoint":
            x = torch.rand((n, H, W, c), generator=g)
            call = lambda x_, out: L.swnerf_pyramid_up_adjoint(_lib.ptr(x_), n, H, W, c, h, w, _lib.ptr(out), _lib.stream_of(out))
            ins, out_shape = [x], (n, h, w, c)
        else:
            if case == "up_axpy_same_size":
                H, W = h, w
            x = torch.rand((n, h, w, c), generator=g)
            ins, out_shape = [x], (n, H, W, c)
            if case == "up_axpy_nobase":
                call = lambda x_, out: L.swnerf_pyramid_up_axpy(_lib.ptr(x_), n, h, w, c, None, 0.5, H, W, _lib.ptr(out), _lib.stream_of(out))
            else:
                ins.append(torch.rand((n, H, W, c), generator=g))
                call = lambda x_, b_, out: L.swnerf_pyramid_up_axpy(_lib.ptr(x_), n, h, w, c, _lib.ptr(b_), -1.0, H, W, _lib.ptr(out), _lib.stream_of(out))
        # filled from host tensors: no device temporaries whose freed blocks could land inside a later tight allocation
        tight = [tail(t) for t in ins]
        out_t = tail(torch.zeros(out_shape))
        _lib.check(call(*tight, out_t), case)
        torch.cuda.synchronize()
        loose = [t.to(dev) for t in ins]
        out_l = torch.zeros(out_shape, device=dev)
        _lib.check(call(*loose, out_l), case)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out_t).all()) and float(out_t.abs().max()) > 0, (case, (n, h, w, c))
        assert torch.equal(out_t, out_l), (case, (n, h, w, c), float((out_t - out_l).abs().max()))
        del tight, out_t, loose, out_l
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


for c in sys.argv[1:]:
    run(c)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    print(f"{c}: ok", flush=True)
