#!/usr/bin/env python3
"""Out-of-bounds guard for the dataset image entry points (swnerf_png_unfilter, swnerf_area_resize), in the manner of
tools/tight_buffer_check_pyramid.py: every operand and every output ends exactly where a torch allocation of at least 10 MB
whose size is a multiple of 2 MB ends (the caching allocator then maps exactly that much), so a read or write past the last
element leaves the mapping and faults instead of touching a neighbour.  The filtered scanlines are 1 + W * bpp bytes a row, so
with bpp = 3 nothing is 4-byte aligned and a load wider than a byte at the last pixel would cross the end; the resize cases end
on an odd byte count (c = 3 bytes) and on a fractional footprint whose last cell is the last of the image.  Every result is
compared with the same call on ordinary allocations, bit for bit.
  tight_buffer_check_images.py <case> [<case> ...]
  tight_buffer_check_images.py list
tests/test_00_a_images_tight_buffers.py starts it as a child process."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sw-nerf_amd"), ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
UNFILTER_HW = [(1, 1), (17, 31), (257, 9)]
CASES = [f"unfilter_bpp{b}" for b in (3, 4)] + [f"resize_{t}_c{c}_{k}" for t in ("u8", "f32") for c in (3, 4) for k in ("2x", "frac")]
if len(sys.argv) < 2 or sys.argv[1] == "list":
    print(" ".join(CASES))
    sys.exit(0)
for c in sys.argv[1:]:
    if c not in CASES:
        raise SystemExit(f"unknown case {c!r}; `list` prints them")

import numpy as np
import torch
import png_ref
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


def both(call, ins, outs, what):
    """call(*ins, *outs) on tight and on ordinary allocations -> the tight outputs, equal bit for bit to the ordinary ones"""
    tight_in, tight_out = [tail(t) for t in ins], [tail(t) for t in outs]
    _lib.check(call(*tight_in, *tight_out), what)
    torch.cuda.synchronize()
    loose_in, loose_out = [t.to(dev) for t in ins], [t.to(dev) for t in outs]
    _lib.check(call(*loose_in, *loose_out), what)
    torch.cuda.synchronize()
    for a, b in zip(tight_out, loose_out):
        assert torch.equal(a, b), what
    res = [t.cpu() for t in tight_out]
    del tight_in, tight_out, loose_in, loose_out
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return res


def run(case):
    L = _lib.lib()
    if case.startswith("unfilter"):
        bpp = int(case[-1])
        for (H, W) in UNFILTER_HW:
            n = 2
            imgs = [png_ref.image(H, W, bpp, seed=10 * H + k) for k in range(n)]
            rows = np.stack([png_ref.filter_rows(im, png_ref.row_types(H, seed=H + W + k)) for k, im in enumerate(imgs)])
            call = lambda f, o, s: L.swnerf_png_unfilter(_lib.ptr(f), n, H, W, bpp, _lib.ptr(o), _lib.ptr(s), _lib.stream_of(o))
            out, status = both(call, [torch.from_numpy(rows.reshape(n, -1))],
                               [torch.zeros((n, H, W, bpp), dtype=torch.uint8), torch.full((n,), -1, dtype=torch.int32)], (case, H, W))
            assert status.tolist() == [0] * n, (case, H, W, status.tolist())
            assert np.array_equal(out.numpy(), np.stack(imgs)), (case, H, W)
        return
    _, t, c, kind = case.split("_")
    c = int(c[1])
    g = torch.Generator().manual_seed(len(case) + c)
    for (n, H, W, h, w) in ([(2, 18, 34, 9, 17), (1, 6, 2, 3, 1)] if kind == "2x" else [(2, 17, 31, 5, 7), (1, 9, 13, 4, 6)]):
        src = torch.randint(0, 256, (n, H, W, c), generator=g, dtype=torch.uint8) if t == "u8" else torch.rand((n, H, W, c), generator=g)
        call = lambda s, d: L.swnerf_area_resize(_lib.ptr(s), int(t == "u8"), n, H, W, c, h, w, _lib.ptr(d), _lib.stream_of(d))
        out, = both(call, [src], [torch.zeros((n, h, w, c))], (case, H, W))
        assert bool(torch.isfinite(out).all()) and float(out.max()) > 0 and float(out.max()) <= 1, (case, H, W)


for c in sys.argv[1:]:
    run(c)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    print(f"{c}: ok", flush=True)
