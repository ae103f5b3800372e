#!/usr/bin/env python3
"""Out-of-bounds guard for the LPIPS entry points (swnerf_conv2d_pack, swnerf_conv2d_nhwc, swnerf_maxpool2d_nhwc,
swnerf_lpips_layer), in the manner of tools/tight_buffer_check.py: every operand, the workspace and every output end exactly
where a torch allocation of at least 10 MB whose size is a multiple of 2 MB ends (the caching allocator then maps exactly that
much), so a read or write past the last element leaves the mapping and faults instead of touching a neighbour.  Sizes are
ragged: pixel counts that are no multiple of the 128-pixel tile, channel counts that are no multiple of the 64 / 128 column
tile or of 4, K that is no multiple of the 32-deep chunk, windows that hang over every image border - so the last tile's
gather, the last weight rows, the last pooling window and the last pixel group all reach the end of their operands.
  tight_buffer_check_lpips.py <case> [<case> ...]   cases: pack conv_vec conv_scalar pool layer
  tight_buffer_check_lpips.py list
tests/test_00_a_lpips_tight_buffers.py starts it as a child process."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sw-nerf_amd"), ROOT):
    sys.path.insert(0, p)
CASES = ["pack", "conv_vec", "conv_scalar", "pool", "layer"]
if len(sys.argv) < 2 or sys.argv[1] == "list":
    print(" ".join(CASES))
    sys.exit(0)
for c in sys.argv[1:]:
    if c not in CASES:
        raise SystemExit(f"unknown case {c!r}; `list` prints them")

import torch
import torch.nn.functional as F
from swnerf import _lib

dev = torch.device("cuda:0")
MB2 = 2 << 20


def tight_bytes(n):
    return max(10 << 20, (n + MB2 - 1) // MB2 * MB2)


def tail(dtype, shape, src=None):
    """a tensor of `shape` that ends exactly at the end of a tight allocation, filled from the host tensor `src`"""
    es = torch.empty((), dtype=dtype).element_size()
    n = 1
    for s in shape:
        n *= s
    buf = torch.empty(tight_bytes(n * es) // es, dtype=dtype, device=dev)
    t = buf[buf.numel() - n:].view(shape)
    if src is not None:
        t.copy_(src.reshape(shape))
    return t


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def conv(L, x, wt, b, k, s, p, relu):
    """x [N,C,H,W], wt [co,ci,k,k], b [co] host tensors -> the kernel's output, every device operand tight"""
    n, ci, h, w = x.shape
    co = wt.shape[0]
    ho, wo = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    dx, dw, db = tail(torch.float32, (n, h, w, ci), nhwc(x)), tail(torch.float32, (co, ci, k, k), wt), tail(torch.float32, (co,), b)
    packed, out = tail(torch.float32, (k * k * ci, co)), tail(torch.float32, (n, ho, wo, co))
    st = _lib.stream_of(dx)
    _lib.check(L.swnerf_conv2d_pack(_lib.ptr(dw), co, ci, k, _lib.ptr(packed), st), "conv2d_pack")
    _lib.check(L.swnerf_conv2d_nhwc(_lib.ptr(dx), n, h, w, ci, _lib.ptr(packed), _lib.ptr(db), co, k, s, p,
                                    _lib.ACT_RELU if relu else _lib.ACT_NONE, _lib.ptr(out), st), "conv2d_nhwc")
    torch.cuda.synchronize()
    return packed.cpu(), out.cpu()


def run(case):
    L = _lib.lib()
    g = torch.Generator().manual_seed(3)
    if case in ("pack", "conv_vec", "conv_scalar"):
        shapes = {"pack": [(1, 5, 37, 4, 4, 11, 1, 5), (1, 8, 72, 3, 3, 1, 1, 0)],
                  "conv_vec": [(2, 8, 72, 67, 45, 3, 1, 1), (1, 64, 192, 13, 9, 5, 1, 2), (3, 4, 64, 21, 19, 3, 2, 0)],
                  "conv_scalar": [(2, 3, 37, 131, 97, 11, 4, 2), (2, 3, 64, 41, 37, 3, 1, 1), (1, 5, 131, 9, 30, 7, 3, 5)]}[case]
        for n, ci, co, h, w, k, s, p in shapes:
            x = torch.randn(n, ci, h, w, generator=g)
            wt = torch.randn(co, ci, k, k, generator=g) * (2.0 / (ci * k * k)) ** 0.5
            b = 0.1 * torch.randn(co, generator=g)
            for relu in (False, True):
                packed, out = conv(L, x, wt, b, k, s, p, relu)
                assert torch.equal(packed.view(k, k, ci, co), wt.permute(2, 3, 1, 0)), (case, n, ci, co)
                want = F.conv2d(x, wt, b, stride=s, padding=p)
                want = nhwc(torch.relu(want) if relu else want)
                assert torch.allclose(out, want, rtol=1e-3, atol=1e-4), (case, (n, ci, co, h, w, k, s, p), float((out - want).abs().max()))
    elif case == "pool":
        for n, c, h, w in ((3, 64, 37, 51), (2, 5, 40, 33), (1, 4, 3, 3)):
            x = torch.randn(n, c, h, w, generator=g)
            for win in (2, 3):
                ho, wo = (h - win) // 2 + 1, (w - win) // 2 + 1
                dx, out = tail(torch.float32, (n, h, w, c), nhwc(x)), tail(torch.float32, (n, ho, wo, c))
                _lib.check(L.swnerf_maxpool2d_nhwc(_lib.ptr(dx), n, h, w, c, win, _lib.ptr(out), _lib.stream_of(dx)), "maxpool2d_nhwc")
                torch.cuda.synchronize()
                assert torch.equal(out.cpu(), nhwc(F.max_pool2d(x, kernel_size=win, stride=2))), (case, n, c, h, w, win)
    else:
        for n, c, h, w in ((3, 64, 37, 51), (2, 5, 23, 19), (2, 512, 3, 2), (1, 192, 1, 1)):
            f0 = torch.relu(torch.randn(n, c, h, w, generator=g))
            f1 = torch.relu(f0 + 0.3 * torch.randn(n, c, h, w, generator=g))
            lin = torch.rand(c, generator=g)
            d0, d1, dl = tail(torch.float32, (n, h, w, c), nhwc(f0)), tail(torch.float32, (n, h, w, c), nhwc(f1)), tail(torch.float32, (c,), lin)
            wsb = L.swnerf_lpips_layer_workspace_bytes(n, h, w)
            ws, out, mp = tail(torch.uint8, (wsb,)), tail(torch.float64, (n,)), tail(torch.float32, (n, h, w))
            for m in (mp, None):
                _lib.check(L.swnerf_lpips_layer(_lib.ptr(d0), _lib.ptr(d1), _lib.ptr(dl), n, h, w, c, 0, _lib.ptr(ws), _lib.ptr(out),
                                                _lib.ptr(m), _lib.stream_of(d0)), "lpips_layer")
                torch.cuda.synchronize()
                n0 = f0 / (f0.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
                n1 = f1 / (f1.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
                want = ((n0 - n1).pow(2) * lin.view(1, c, 1, 1)).sum(1)
                assert torch.allclose(out.cpu(), want.double().mean(dim=(1, 2)), rtol=1e-4), (case, n, c, h, w)
            assert torch.allclose(mp.cpu(), want, rtol=1e-3, atol=1e-6), (case, n, c, h, w)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


for c in sys.argv[1:]:
    run(c)
    print(f"{c}: ok", flush=True)
