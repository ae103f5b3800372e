#!/usr/bin/env python3
"""Out-of-bounds guard for swnerf_jpeg_decode, in the manner of tools/tight_buffer_check_images.py: the coefficients, the
quantisation tables, the scratch planes and the output each end exactly where a torch allocation of at least 10 MB whose size is
a multiple of 2 MB ends (the caching allocator then maps exactly that much), so a read or write past the last element leaves the
mapping and faults instead of touching a neighbour.  1 x 1 is one MCU of which one pixel is stored; 17 x 23 has partial MCUs in
both directions and an RGB row of 69 bytes, so pixel quads end on every alignment; 257 x 9 is tall, three pixels short of an
MCU's width and taller than a workgroup has lanes.  Every result is compared with the same call on ordinary allocations, bit for
bit, and with the host statement of the arithmetic in tests/jpeg_ref.py.
  tight_buffer_check_jpeg.py <case> [<case> ...]
  tight_buffer_check_jpeg.py list
tests/test_00_a_jpeg_tight_buffers.py starts it as a child process."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sw-nerf_amd"), ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
SIZES = [(1, 1), (17, 23), (257, 9)]
CASES = [f"decode_{s}_c{c}" for s in ("420", "444") for c in (3, 4)]
if len(sys.argv) < 2 or sys.argv[1] == "list":
    print(" ".join(CASES))
    sys.exit(0)
for c in sys.argv[1:]:
    if c not in CASES:
        raise SystemExit(f"unknown case {c!r}; `list` prints them")

import numpy as np
import torch
import jpeg_ref
from swnerf import _lib

dev = torch.device("cuda:0")
MB2 = 2 << 20


def tail(host):
    """a device copy of `host` that ends exactly at the end of a tight allocation"""
    nbytes = host.numel() * host.element_size()
    buf = torch.empty(max(10 << 20, (nbytes + MB2 - 1) // MB2 * MB2), dtype=torch.uint8, device=dev)
    t = buf[buf.numel() - nbytes:].view(host.dtype).view(host.shape)
    t.copy_(host)
    return t


def run(case):
    L = _lib.lib()
    _, s, c = case.split("_")
    sampling, cout = {"420": _lib.JPEG_420, "444": _lib.JPEG_444}[s], int(c[1])
    for (H, W) in SIZES:
        n = 2
        ncoef = int(L.swnerf_jpeg_coef_count(H, W, 3, sampling))
        rng = np.random.default_rng(H * 100 + W + cout)
        coef = np.zeros((n, ncoef), np.int16)
        coef[:, ::64] = rng.integers(-1000, 1001, (n, ncoef // 64))                          # DC terms across the sample range
        coef.reshape(-1)[rng.integers(0, n * ncoef, n * ncoef // 8)] = rng.integers(-300, 301, n * ncoef // 8)
        qt = rng.integers(1, 9, (n, 3, 64)).astype(np.uint16)
        want = np.stack([jpeg_ref.decode(coef[k], qt[k], H, W, 3, sampling) for k in range(n)])
        outs = []
        for place in (tail, lambda t: t.to(dev)):
            ops = [place(torch.from_numpy(coef)), place(torch.from_numpy(qt.view(np.int16))), place(torch.zeros((n * ncoef,), dtype=torch.uint8)),
                   place(torch.zeros((n, H, W, cout), dtype=torch.uint8))]
            _lib.check(L.swnerf_jpeg_decode(_lib.ptr(ops[0]), _lib.ptr(ops[1]), n, H, W, 3, sampling, cout, _lib.ptr(ops[2]), _lib.ptr(ops[3]),
                                            _lib.stream_of(ops[3])), (case, H, W))
            torch.cuda.synchronize()
            outs.append(ops[3].cpu().numpy())
            del ops
            torch.cuda.empty_cache()
        assert np.array_equal(outs[0], outs[1]), (case, H, W)
        assert np.array_equal(outs[0][..., :3], want), (case, H, W)
        assert cout == 3 or (outs[0][..., 3] == 255).all(), (case, H, W)


for c in sys.argv[1:]:
    run(c)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    print(f"{c}: ok", flush=True)
