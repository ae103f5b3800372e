#!/usr/bin/env python3
"""Out-of-bounds guard for swnerf_adam_step (csrc/optim_kernels.hip), in the manner of tools/tight_buffer_check_batching.py: p, g,
m and v of every tensor end exactly where a torch allocation of at least 10 MB whose size is a multiple of 2 MB ends, so a read or
write past the last element leaves the mapping and faults instead of touching a neighbour.
  vec         sizes that are multiples of 4 (4, 256, 4096, 9216): every pointer 16-byte aligned, the last float4 ends the allocation
  vec_ragged  1, 3, 255, 257, 4099 floats from a 16-byte aligned start: the vector path with its masked tail; the 1..3 floats
              between the tensor's end and the allocation's end hold a sentinel that must survive (a float4 store over the tail
              would stay inside the mapping)
  scalar      1, 3, 255, 256, 257, 4099 floats that END the allocation: an unaligned start wherever the size is no multiple of 4
  multi       34 tensors of 5 floats and one of 4099 (two launches: over the tensor cap), AdamW, per-tensor steps and rates
Every result is compared with the same call on ordinary allocations, bit for bit.
  tight_buffer_check_optim.py <case> [<case> ...]
  tight_buffer_check_optim.py list
tests/test_00_a_optim_tight_buffers.py starts it as a child process."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sw-nerf_amd"), ROOT):
    sys.path.insert(0, p)
CASES = ["vec", "vec_ragged", "scalar", "multi"]
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
SENTINEL = 12345.5


def tail(host, pad=0):
    """a device copy of `host` that ends `pad` floats before the end of a tight allocation; -> (tensor, the pad floats or None)"""
    nbytes = (host.numel() + pad) * 4
    buf = torch.empty(max(10 << 20, (nbytes + MB2 - 1) // MB2 * MB2), dtype=torch.uint8, device=dev)
    f = buf[buf.numel() - nbytes:].view(torch.float32)
    f[host.numel():] = SENTINEL
    t = f[:host.numel()]
    t.copy_(host)
    return t, (f[host.numel():] if pad else None)


def plain(host, pad=0):
    return host.to(dev), None


def run(case):
    lib = _lib.lib()
    g_ = torch.Generator().manual_seed(len(case))
    sizes = {"vec": [4, 256, 4096, 9216], "vec_ragged": [1, 3, 255, 257, 4099], "scalar": [1, 3, 255, 256, 257, 4099],
             "multi": [5] * 34 + [4099]}[case]
    n = len(sizes)
    host = [[torch.randn(s, generator=g_) for s in sizes], [torch.randn(s, generator=g_) for s in sizes],
            [0.1 * torch.randn(s, generator=g_) for s in sizes], [torch.rand(s, generator=g_) for s in sizes]]      # p g m v
    steps = [1.0 + (i % 3) for i in range(n)] if case == "multi" else [2.0] * n
    lrs = [1e-3 * (1 + i % 2) for i in range(n)]
    wds = [0.01] * n
    res = []
    for place in (tail, plain):
        pad = (lambda s: (-s) % 4) if case == "vec_ragged" else (lambda s: 0)
        placed = [[place(t, pad(t.numel())) for t in arr] for arr in host]
        dv = [[t for t, _ in arr] for arr in placed]
        if place is tail:
            for arr in dv:
                for t in arr:
                    end = t.data_ptr() + 4 * (t.numel() + pad(t.numel()))
                    assert end % MB2 == 0, "the operand does not end its allocation"
                    if case in ("vec", "vec_ragged"):
                        assert t.data_ptr() % 16 == 0
            if case == "scalar":
                assert any(t.data_ptr() % 16 for t in dv[0])
        arr = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])
        dbl = lambda xs: (ctypes.c_double * n)(*xs)
        _lib.check(lib.swnerf_adam_step(n, arr(dv[0]), arr(dv[1]), arr(dv[2]), arr(dv[3]), (ctypes.c_int64 * n)(*sizes), dbl(steps), dbl(lrs),
                                        dbl(wds), 0.9, 0.999, 1e-8, int(case == "multi"), 1.0, _lib.stream_of(dv[0][0])), case)
        torch.cuda.synchronize()
        for a in placed:
            for _, canary in a:
                if canary is not None and canary.numel():
                    assert bool((canary == SENTINEL).all()), (case, "a store went past the tensor's last element")
        res.append([[t.cpu() for t in a] for a in dv])
        del placed, dv
        torch.cuda.empty_cache()
    for which, (a, b, h) in enumerate(zip(res[0], res[1], host)):
        for i, (x, y, h0) in enumerate(zip(a, b, h)):
            assert bool(torch.isfinite(x).all()), (case, which, i)
            assert torch.equal(x, y), (case, which, i, float((x - y).abs().max()))
            if which == 1:
                assert torch.equal(x, h0), (case, "the gradient was written")
            else:
                assert not torch.equal(x, h0), (case, which, i, "not updated")


for c in sys.argv[1:]:
    run(c)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    print(f"{c}: ok", flush=True)
