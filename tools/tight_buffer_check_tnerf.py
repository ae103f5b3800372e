#!/usr/bin/env python3
"""Out-of-bounds guard for the T-NeRF entry points, in the manner of tools/tight_buffer_check.py: every operand and output
ends exactly where a torch allocation of at least 10 MB whose size is a multiple of 2 MB ends (the caching allocator then
maps exactly that much), so a read or write past the last element leaves the mapping and faults instead of touching a
neighbour.  Every result is compared bit for bit with the same call on ordinary allocations.
  tight_buffer_check_tnerf.py <case> [<case> ...]   cases: pack (swnerf_pack_net kind 3: the 24 tensors, the blob),
                                                    pass_coarse (the fused pass: linear / stratified depths + noise, every
                                                    optional output), pass_zvals (given depths + noise, every output),
                                                    elu_gemm (swnerf_linear_act with ELU, 16-byte and 4-byte operand
                                                    paths, and swnerf_elu_grad)
  tight_buffer_check_tnerf.py list
tests/test_00_a_tnerf_tight_buffers.py starts it as a child process."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sw-nerf_amd"), ROOT):
    sys.path.insert(0, p)
CASES = ["pack", "pass_coarse", "pass_zvals", "elu_gemm"]
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
L = _lib.lib()
_keep = []                                   # tight allocations stay alive until the process ends: no reuse inside a case


def tail(host):
    """a copy of the host tensor `host` that ends exactly at the end of a tight allocation"""
    n = host.numel()
    nbytes = max(10 << 20, (4 * n + MB2 - 1) // MB2 * MB2)
    buf = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    _keep.append(buf)
    t = buf[buf.numel() - n:].view(host.shape)
    t.copy_(host)
    return t


def empty_tail(shape):
    return tail(torch.full(shape, float("nan")))


NAMES = ([f"layers.{i}.0.{p}" for i in range(8) for p in ("weight", "bias")]
         + [f"{n}.0.{p}" for n in ("density", "feature", "layer_9", "color") for p in ("weight", "bias")])
SD = {k: torch.from_numpy(v) for k, v in synth.tnerf_state_dict(141).items()}
NF = L.swnerf_packed_floats(3)


def pack(tight):
    ps = [tail(SD[n]) if tight else SD[n].to(dev) for n in NAMES]
    out = empty_tail((NF,)) if tight else torch.empty(NF, device=dev)
    arr = (ctypes.c_void_p * 24)(*[p.data_ptr() for p in ps])
    _lib.check(L.swnerf_pack_net(3, arr, 10, 4, 10, _lib.ptr(out), _lib.stream_of(out)), "pack_net")
    torch.cuda.synchronize()
    return out


def rays(n, seed):
    K, c2w = synth.lego_camera(400, 400)
    o, d = synth.pick_rays(400, 400, K, c2w, n, seed)
    o, d = torch.from_numpy(o), torch.from_numpy(d)
    one = torch.ones((n, 1))
    return torch.cat([o, d, 2 * one, 6 * one, 0.375 * one, d / d.norm(dim=-1, keepdim=True)], -1).float().contiguous()


def fused(tight, zvals):
    N, S = 1027, 75                                      # a partial workgroup (N % 4 = 3) and a partial tile (S % 32 = 11)
    g = torch.Generator().manual_seed(5)
    host = {"rb": rays(N, 9), "noise": torch.rand((N, S), generator=g) * 0.5}
    if zvals:
        host["z_vals"] = torch.sort(torch.rand((N, S), generator=g) * 4 + 2, -1).values.contiguous()
    else:
        host["t_rand"] = torch.rand((N, S), generator=g)
    packed = pack(tight)
    inp = {k: (tail(v) if tight else v.to(dev)) for k, v in host.items()}
    shapes = {"rgb_map": (N, 3), "disp_map": (N,), "acc_map": (N,), "depth_map": (N,), "weights": (N, S), "raw": (N, S, 4),
              "z_out": (N, S)}
    out = {k: (empty_tail(s) if tight else torch.full(s, float("nan"), device=dev)) for k, s in shapes.items()}
    a = _lib.PassArgs()
    a.ray_batch, a.n_rays, a.cols, a.kind, a.packed = inp["rb"].data_ptr(), N, 12, 3, packed.data_ptr()
    a.L_pos, a.L_dir, a.L_time, a.n_samples, a.white_bkgd = 10, 4, 10, S, 1
    for k in ("z_vals", "t_rand", "noise"):
        if k in inp:
            setattr(a, k, inp[k].data_ptr())
    for k, t in out.items():
        setattr(a, k, t.data_ptr())
    _lib.check(L.swnerf_render_pass(a, _lib.stream_of(packed)), "render_pass")
    torch.cuda.synchronize()
    for k, t in out.items():
        assert bool(torch.isfinite(t).all()), k
    return {k: v.cpu() for k, v in out.items()}


def elu_gemm(tight):
    res = []
    g = torch.Generator().manual_seed(7)
    for M, K, N in ((4097, 84, 128), (1031, 155, 64), (301, 128, 1)):     # 16-byte path; 4-byte path (K % 4 != 0); 64-row kernel
        x = torch.randn((M, K), generator=g) * 2
        w = torch.randn((N, K), generator=g) / np.sqrt(K)
        b = torch.randn((N,), generator=g) * 0.1
        xt, wt, bt = ((tail(x), tail(w), tail(b)) if tight else (x.to(dev), w.to(dev), b.to(dev)))
        y = empty_tail((M, N)) if tight else torch.empty((M, N), device=dev)
        _lib.check(L.swnerf_linear_act(_lib.ptr(xt), K, M, K, _lib.ptr(wt), _lib.ptr(bt), N, _lib.ACT_ELU, _lib.ptr(y), N,
                                       _lib.stream_of(y)), "linear_act")
        dy = tail(torch.randn((M, N), generator=g)) if tight else torch.randn((M, N), generator=g).to(dev)
        _lib.check(L.swnerf_elu_grad(_lib.ptr(dy), _lib.ptr(y), M * N, _lib.stream_of(y)), "elu_grad")
        torch.cuda.synchronize()
        res += [y.cpu(), dy.cpu()]
    return res


def run(case):
    if case == "pack":
        a, b = pack(True).cpu(), pack(False).cpu()
        assert torch.equal(a, b)
    elif case in ("pass_coarse", "pass_zvals"):
        a, b = fused(True, case == "pass_zvals"), fused(False, case == "pass_zvals")
        for k in a:
            assert torch.equal(a[k], b[k]), k
        assert float(a["acc_map"].min()) < 0.9 and float(a["acc_map"].max()) > 0.9
    else:
        for x, y in zip(elu_gemm(True), elu_gemm(False)):
            assert torch.equal(x, y)


for c in sys.argv[1:]:
    run(c)
    torch.cuda.synchronize()
    print(f"{c}: ok", flush=True)
