#!/usr/bin/env python3
"""Out-of-bounds guard for the training-batch entry points (csrc/batch_kernels.hip), in the manner of
tools/tight_buffer_check_fit2d.py: every operand and every output ends exactly where a torch allocation of at least 10 MB
whose size is a multiple of 2 MB ends, so a read or write past the last element leaves the mapping and faults instead of
touching a neighbour.  Sizes are ragged (3 images of 37 x 53; batches of 1, 255, 257 and 1000 rays - a lone ray, the LDS block
edge and the dword tail; rows of 8, 11 and 12 columns; float32 RGB and uint8 RGBA images, whose last pixel ends the allocation).
Every result is compared with the same call on ordinary allocations, bit for bit.
  tight_buffer_check_batching.py <case> [<case> ...]
  tight_buffer_check_batching.py list
tests/test_00_a_batching_tight_buffers.py starts it as a child process."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sw-nerf_amd"), ROOT):
    sys.path.insert(0, p)
CASES = ["perm", "batch_perm_f32", "batch_perm_u8", "batch_ids_f32", "batch_ids_u8", "loss", "loss_rgb0"]
if len(sys.argv) < 2 or sys.argv[1] == "list":
    print(" ".join(CASES))
    sys.exit(0)
for c in sys.argv[1:]:
    if c not in CASES:
        raise SystemExit(f"unknown case {c!r}; `list` prints them")

import numpy as np
import torch
from swnerf import _lib, synth

dev = torch.device("cuda:0")
MB2 = 2 << 20
N_IMG, H, W = 3, 37, 53
NS = (1, 255, 257, 1000)


def tail(host):
    """a device copy of `host` that ends exactly at the end of a tight allocation"""
    nbytes = host.numel() * host.element_size()
    buf = torch.empty(max(10 << 20, (nbytes + MB2 - 1) // MB2 * MB2), dtype=torch.uint8, device=dev)
    t = buf[buf.numel() - nbytes:].view(host.dtype).view(host.shape)
    t.copy_(host)
    return t


def both(case, ins, outs, call):
    """call(ins..., outs...) on tight and on ordinary allocations; the outputs must agree bit for bit"""
    res = []
    for place in (tail, lambda t: t.to(dev)):
        i_, o_ = [None if t is None else place(t) for t in ins], [None if t is None else place(t) for t in outs]
        _lib.check(call(*i_, *o_), case)
        torch.cuda.synchronize()
        res.append([None if t is None else t.cpu() for t in o_])
        del i_, o_
        torch.cuda.empty_cache()
    for a, b in zip(*res):
        if a is not None:
            assert bool(torch.isfinite(a.float()).all()), case
            assert torch.equal(a, b), (case, float((a.float() - b.float()).abs().max()))
    return res[0]


def run(case):
    lib = _lib.lib()
    g = torch.Generator().manual_seed(len(case))
    st = _lib.stream_of(torch.empty(1, device=dev))
    P = _lib.ptr
    if case == "perm":
        for n, k0, count in ((1, 0, 1), (37, 0, 37), (3 * H * W, 5000, 883), (1 << 33, 1 << 32, 1000)):
            both(case, [], [torch.zeros(count, dtype=torch.int64)], lambda o: lib.swnerf_perm_indices(12345, n, k0, count, P(o), st))
        return
    if case.startswith("loss"):
        for N in (1, 33, 4096):
            rgb, rgb0, tg = (torch.rand(N, 3, generator=g) for _ in range(3))
            if case == "loss":
                both(case, [rgb, tg], [torch.zeros(2, dtype=torch.float64), torch.zeros(3), torch.zeros(N, 3)],
                     lambda r, t, s, l, d: lib.swnerf_photo_loss(P(r), None, P(t), N, P(s), P(l), P(d), None, st))
            else:
                both(case, [rgb, rgb0, tg], [torch.zeros(2, dtype=torch.float64), torch.zeros(3), torch.zeros(N, 3), torch.zeros(N, 3)],
                     lambda r, r0, t, s, l, d, d0: lib.swnerf_photo_loss(P(r), P(r0), P(t), N, P(s), P(l), P(d), P(d0), st))
        return
    u8 = case.endswith("u8")
    ch = 4 if u8 else 3
    images = (torch.randint(0, 256, (N_IMG, H, W, ch), generator=g, dtype=torch.uint8) if u8 else torch.rand(N_IMG, H, W, ch, generator=g))
    c2w = torch.from_numpy(np.stack([synth.pose_spherical(30. + 50. * i, -30., 4.)[:3, :4] for i in range(N_IMG)]).astype(np.float32))
    times = torch.linspace(0, 1, N_IMG)
    i_train = torch.tensor([2, 0, 1], dtype=torch.int64)
    domain = N_IMG * H * W
    focal = 0.5 * W / np.tan(0.5 * synth.LEGO_CAMERA_ANGLE_X)
    for n in NS:
        for cols, ndc in ((8, 0), (11, 1), (12, 0)):
            ids = torch.randint(0, domain, (n,), generator=g, dtype=torch.int64) if "_ids_" in case else None
            if ids is not None:
                ids[-1] = domain - 1                                 # the last pixel of the last image: its last channel ends the allocation
            k0 = domain - n                                          # permutation mode: the END of the epoch
            def call(im, cw, tm, it, idd, rb, tg, io):
                return lib.swnerf_train_batch(P(im), int(u8), ch, N_IMG, H, W, P(cw), P(tm), P(it), N_IMG, 0, 0, H, W, focal, focal, 0., 0., 1,
                                              2., 6., cols, ndc, focal, int(u8), 99, k0, n, P(idd), P(rb), P(tg), P(io), st)
            rb, tg, io = both(case, [images, c2w, times, i_train, ids], [torch.zeros(n, cols), torch.zeros(n, 3), torch.zeros(n, dtype=torch.int64)], call)
            assert int(io.min()) >= 0 and int(io.max()) < domain
            if ids is None:
                assert len(set(io.tolist())) == n                     # drawn without replacement


for c in sys.argv[1:]:
    run(c)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    print(f"{c}: ok", flush=True)
