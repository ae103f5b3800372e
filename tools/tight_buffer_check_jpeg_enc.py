#!/usr/bin/env python3
"""Out-of-bounds guard for swnerf_jpeg_encode, in the manner of tools/tight_buffer_check_jpeg.py: the frames, the quantisation
tables, the scratch planes and the coefficients each end exactly where a torch allocation of at least 10 MB whose size is a
multiple of 2 MB ends (the caching allocator then maps exactly that much), so a read or write past the last element leaves the
mapping and faults instead of touching a neighbour.  1 x 1 is one MCU of which one pixel exists; 17 x 23 has partial MCUs in
both directions and dummy luma blocks at 4:2:0; 257 x 9 is tall, narrow and has more blocks than a workgroup has lanes.  Every
result is compared with the same call on ordinary allocations, bit for bit, and with the host statement of the arithmetic in
tests/jpeg_enc_ref.py.  The same inputs go through tests/jpeg_enc_host_main.cpp on the CPU first (tests/test_jpeg_enc_host.py).
  tight_buffer_check_jpeg_enc.py <case> [<case> ...]      the first failure ends the run
  tight_buffer_check_jpeg_enc.py list
tests/test_00_a_jpeg_enc_tight_buffers.py starts it as a child process."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sw-nerf_amd"), ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
SIZES = [(1, 1), (17, 23), (257, 9)]
CASES = [f"encode_{s}_{t}_c{c}" for s in ("420", "444") for t in ("u8", "f32") for c in (3, 4)]
if len(sys.argv) < 2 or sys.argv[1] == "list":
    print(" ".join(CASES))
    sys.exit(0)
for c in sys.argv[1:]:
    if c not in CASES:
        raise SystemExit(f"unknown case {c!r}; `list` prints them")

import numpy as np
import torch
import jpeg_enc_ref
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
    _, s, t, c = case.split("_")
    sampling = {"420": _lib.JPEG_420, "444": _lib.JPEG_444}[s]
    inputs = {name: px for name, px, _ in jpeg_enc_ref.tight_cases()}
    qt2 = jpeg_enc_ref.quant_tables(90)
    qt = np.ascontiguousarray(qt2[[0, 1, 1]])
    for (H, W) in SIZES:
        px = inputs[f"{H}x{W}_{s}_{t}_{c}"]
        n = px.shape[0]
        ncoef = int(L.swnerf_jpeg_coef_count(H, W, 3, sampling))
        u8 = px if px.dtype == np.uint8 else jpeg_enc_ref.to8b(px)
        want = np.stack([jpeg_enc_ref.coefficients(u8[k], qt2, 3, sampling) for k in range(n)])
        outs = []
        for place in (tail, lambda x: x.to(dev)):
            ops = [place(torch.from_numpy(px)), place(torch.from_numpy(qt.view(np.int16))), place(torch.zeros((n * ncoef,), dtype=torch.uint8)),
                   place(torch.zeros((n, ncoef), dtype=torch.int16))]
            _lib.check(L.swnerf_jpeg_encode(_lib.ptr(ops[0]), int(px.dtype == np.uint8), n, H, W, px.shape[3], 0.0, _lib.ptr(ops[1]), 3, sampling,
                                            _lib.ptr(ops[2]), _lib.ptr(ops[3]), _lib.stream_of(ops[3])), (case, H, W))
            torch.cuda.synchronize()
            outs.append(ops[3].cpu().numpy())
            del ops
            torch.cuda.empty_cache()
        assert np.array_equal(outs[0], outs[1]), (case, H, W)
        assert np.array_equal(outs[0], want), (case, H, W)


for c in sys.argv[1:]:
    run(c)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    print(f"{c}: ok", flush=True)
