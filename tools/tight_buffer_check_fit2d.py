#!/usr/bin/env python3
"""Out-of-bounds guard for the 2-D fitting entry points (csrc/fit2d_kernels.hip), in the manner of
tools/tight_buffer_check_pyramid.py: every operand and every output ends exactly where a torch allocation of at least 10 MB
whose size is a multiple of 2 MB ends, so a read or write past the last element leaves the mapping and faults instead of
touching a neighbour.  Sizes are ragged (1961 rows, 33 x 257, 513 x 96; M = 1 / 31 / 33 / 1961 rows of 96 floats holding 82
encoded columns, so the last row's allocation stops at its last column).  Every result is compared with the same call on
ordinary allocations, bit for bit.
  tight_buffer_check_fit2d.py <case> [<case> ...]
  tight_buffer_check_fit2d.py list
tests/test_00_a_fit2d_tight_buffers.py starts it as a child process."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sw-nerf_amd"), ROOT, os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)
CASES = ["encode", "bn_forward", "bn_backward", "bn_apply", "loss", "pack", "forward", "picture_f32", "picture_u8", "picture_both"]
if len(sys.argv) < 2 or sys.argv[1] == "list":
    print(" ".join(CASES))
    sys.exit(0)
for c in sys.argv[1:]:
    if c not in CASES:
        raise SystemExit(f"unknown case {c!r}; `list` prints them")

import numpy as np
import torch
from swnerf import _lib
import cases_fit2d as C

dev = torch.device("cuda:0")
MB2 = 2 << 20
N_LAYERS, L = 3, 20
BN_SHAPES = [(33, 257), (513, 96)]


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


def params_host():
    sd = C.synth.fit2d_state_dict(77, 4 * L + 2, N_LAYERS)
    return [torch.from_numpy(v) for k, v in sd.items() if not k.endswith("num_batches_tracked")]


def pack_call(lib, st):
    def call(*a):
        ts, blob = a[:-1], a[-1]
        arr = (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
        return lib.swnerf_pack_fit2d(arr, N_LAYERS, L, 1e-5, _lib.ptr(blob), st)
    return call


def run(case):
    lib = _lib.lib()
    g = torch.Generator().manual_seed(len(case))
    st = _lib.stream_of(torch.empty(1, device=dev))
    P = _lib.ptr
    if case == "encode":
        pos = torch.from_numpy(C.grid())
        n = pos.shape[0]
        for Lb in (0, 4, 23):
            both(case, [pos], [torch.zeros(n, 4 * Lb + 2)], lambda p, o: lib.swnerf_encode2d(P(p), n, 52.0, 36.0, Lb, P(o), st))
        return
    if case.startswith("bn_"):
        for (M, Cc) in BN_SHAPES:
            a, dy = torch.randn(M, Cc, generator=g), torch.randn(M, Cc, generator=g)
            gam, bet = torch.rand(Cc, generator=g) + 0.5, torch.rand(Cc, generator=g)
            rm, rv = torch.rand(Cc, generator=g), torch.rand(Cc, generator=g) + 0.5
            nws = lib.swnerf_bn_workspace_bytes(M, Cc)
            ws = torch.zeros(nws // 8, dtype=torch.float64) if nws else None
            for relu in (0, 1):
                if case == "bn_apply":
                    both(case, [a, gam, bet, rm, rv], [torch.zeros(M, Cc)],
                         lambda a_, g_, b_, m_, v_, y: lib.swnerf_bn_apply(P(a_), M, Cc, relu, P(g_), P(b_), P(m_), P(v_), 1e-5, P(y), st))
                    continue
                fwd = lambda a_, g_, b_, y, mu, is_, m_, v_, w: lib.swnerf_bn_forward_train(P(a_), M, Cc, relu, P(g_), P(b_), 1e-5, 0.1, P(y), P(mu),
                                                                                          P(is_), P(m_), P(v_), P(w), st)
                y, mu, is_, _, _, _ = both(case, [a, gam, bet], [torch.zeros(M, Cc), torch.zeros(Cc), torch.zeros(Cc), rm.clone(), rv.clone(), ws], fwd)
                if case == "bn_backward":
                    both(case, [dy, a, gam, mu, is_], [torch.zeros(M, Cc), torch.zeros(Cc), torch.zeros(Cc), ws],
                         lambda d_, a_, g_, m_, i_, dx, dg, db, w: lib.swnerf_bn_backward(P(d_), P(a_), M, Cc, relu, P(g_), P(m_), P(i_), P(dx), P(dg),
                                                                                          P(db), P(w), st))
        return
    if case == "loss":
        M = 33
        o, t = torch.rand(M, 3, generator=g) * 2 - 0.5, torch.rand(M, 3, generator=g)
        both(case, [o, t], [torch.zeros(2, dtype=torch.float64), torch.zeros(M, 3)],
             lambda o_, t_, s, gr: lib.swnerf_fit2d_loss(P(o_), P(t_), M, 0.1, P(s), P(gr), st))
        return
    nblob = lib.swnerf_fit2d_packed_floats(N_LAYERS)
    (blob,) = both("pack", params_host(), [torch.zeros(nblob)], pack_call(lib, st))
    if case == "pack":
        return
    if case == "forward":
        ldx = 96
        for M in (1, 31, 33, 1961):
            x = torch.rand((M - 1) * ldx + 4 * L + 2, generator=g) * 2 - 1          # the last row stops at its last encoded column
            both(case, [blob, x], [torch.zeros(M, 3)], lambda b, x_, o: lib.swnerf_fit2d_forward(P(b), P(x_), M, ldx, L, N_LAYERS, P(o), st))
        return
    H, W = C.GRID_H, C.GRID_W
    f = torch.zeros(H, W, 3) if case != "picture_u8" else None
    u = torch.zeros(H, W, 3, dtype=torch.uint8) if case != "picture_f32" else None
    both(case, [blob], [f, u], lambda b, f_, u_: lib.swnerf_fit2d_picture(P(b), H, W, L, N_LAYERS, P(f_), P(u_), st))


for c in sys.argv[1:]:
    run(c)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    print(f"{c}: ok", flush=True)
