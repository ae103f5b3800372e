#!/usr/bin/env python3
"""Out-of-bounds guard for the entry points of the fused T-NeRF training pass, in the manner of tools/tight_buffer_check_tnerf.py:
every operand and output ends exactly where a torch allocation of at least 10 MB whose size is a multiple of 2 MB ends, so a
read or write past the last element leaves the mapping and faults.  Every result is compared bit for bit with the same call on
ordinary allocations.  Sizes: 5 rays (a workgroup with dead waves) x 33 samples (a second tile with one sample).
  tight_buffer_check_tnerf_train.py <case> [<case> ...]   cases: pack_bwd (swnerf_pack_net_bwd_tnerf), train_forward
                                                          (swnerf_render_pass_train_tnerf: act, xs, raw, z_out, the maps),
                                                          backward (swnerf_render_pass_backward_tnerf with noise and every
                                                          optional gradient input), finish (swnerf_tnerf_feature_finish)
  tight_buffer_check_tnerf_train.py list
tests/test_00_a_tnerf_train_tight_buffers.py starts it as a child process."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sw-nerf_amd"), ROOT):
    sys.path.insert(0, p)
CASES = ["pack_bwd", "train_forward", "backward", "finish"]
if len(sys.argv) < 2 or sys.argv[1] == "list":
    print(" ".join(CASES))
    sys.exit(0)
for c in sys.argv[1:]:
    if c not in CASES:
        raise SystemExit(f"unknown case {c!r}; `list` prints them")

import torch
from swnerf import _lib, synth

dev = torch.device("cuda:0")
MB2 = 2 << 20
L = _lib.lib()
_keep = []                                   # tight allocations stay alive until the process ends: no reuse inside a case
N, S = 5, 33


def tail(host):
    """a copy of the host tensor `host` that ends exactly at the end of a tight allocation"""
    n = host.numel()
    nbytes = max(10 << 20, (4 * n + MB2 - 1) // MB2 * MB2)
    buf = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    _keep.append(buf)
    t = buf[buf.numel() - n:].view(host.shape)
    t.copy_(host)
    return t


def place(host, tight):
    return tail(host) if tight else host.to(dev)


def blank(shape, tight):
    return place(torch.full(shape, float("nan")), tight)


NAMES = ([f"layers.{i}.0.{p}" for i in range(8) for p in ("weight", "bias")]
         + [f"{n}.0.{p}" for n in ("density", "feature", "layer_9", "color") for p in ("weight", "bias")])
SD = {k: torch.from_numpy(v) for k, v in synth.tnerf_state_dict(141).items()}


def pack(tight, bwd):
    ps = [place(SD[n], tight) for n in NAMES]
    out = blank((L.swnerf_packed_bwd_tnerf_floats() if bwd else L.swnerf_packed_floats(3),), tight)
    arr = (ctypes.c_void_p * 24)(*[p.data_ptr() for p in ps])
    if bwd:
        _lib.check(L.swnerf_pack_net_bwd_tnerf(arr, 10, 4, 10, _lib.ptr(out), _lib.stream_of(out)), "pack_net_bwd_tnerf")
    else:
        _lib.check(L.swnerf_pack_net(3, arr, 10, 4, 10, _lib.ptr(out), _lib.stream_of(out)), "pack_net")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
    return out


def rays(n, seed):
    K, c2w = synth.lego_camera(400, 400)
    o, d = synth.pick_rays(400, 400, K, c2w, n, seed)
    o, d = torch.from_numpy(o), torch.from_numpy(d)
    one = torch.ones((n, 1))
    return torch.cat([o, d, 2 * one, 6 * one, 0.375 * one, d / d.norm(dim=-1, keepdim=True)], -1).float().contiguous()


def forward(tight):
    g = torch.Generator().manual_seed(5)
    host = {"rb": rays(N, 9), "noise": torch.rand((N, S), generator=g) * 0.5, "t_rand": torch.rand((N, S), generator=g)}
    packed = pack(tight, False)
    inp = {k: place(v, tight) for k, v in host.items()}
    rows = L.swnerf_train_rows(N, S)
    shapes = {"rgb_map": (N, 3), "disp_map": (N,), "acc_map": (N,), "raw": (N, S, 4), "z_out": (N, S)}
    out = {k: blank(s, tight) for k, s in shapes.items()}
    act, xs = blank((rows, L.swnerf_tnerf_act_floats_per_row()), tight), blank((rows, L.swnerf_tnerf_xs_floats_per_row()), tight)
    a = _lib.PassArgs()
    a.ray_batch, a.n_rays, a.cols, a.kind, a.packed = inp["rb"].data_ptr(), N, 12, 3, packed.data_ptr()
    a.L_pos, a.L_dir, a.L_time, a.n_samples, a.white_bkgd = 10, 4, 10, S, 1
    a.t_rand, a.noise = inp["t_rand"].data_ptr(), inp["noise"].data_ptr()
    for k, t in out.items():
        setattr(a, k, t.data_ptr())
    _lib.check(L.swnerf_render_pass_train_tnerf(a, _lib.ptr(act), _lib.ptr(xs), _lib.stream_of(packed)), "render_pass_train_tnerf")
    torch.cuda.synchronize()
    out.update(act=act, xs=xs)
    for k, t in out.items():
        assert bool(torch.isfinite(t).all()), k          # every padded row of act / xs is written
    return inp, out


def backward(tight):
    inp, f = forward(tight)
    g = torch.Generator().manual_seed(6)
    ups = {"g_rgb": torch.randn((N, 3), generator=g), "g_disp": torch.randn((N,), generator=g), "g_acc": torch.randn((N,), generator=g),
           "g_raw": torch.randn((N, S, 4), generator=g) * 0.01}
    ups = {k: place(v, tight) for k, v in ups.items()}
    packed_bwd = pack(tight, True)
    rows = L.swnerf_train_rows(N, S)
    grad, d_raw = blank((rows, L.swnerf_tnerf_act_floats_per_row()), tight), blank((rows, 4), tight)
    _lib.check(L.swnerf_render_pass_backward_tnerf(_lib.ptr(packed_bwd), _lib.ptr(f["act"]), _lib.ptr(f["raw"]), _lib.ptr(f["z_out"]),
                                                   _lib.ptr(inp["rb"]), 12, _lib.ptr(inp["noise"]), N, S, 1, _lib.ptr(ups["g_rgb"]),
                                                   _lib.ptr(ups["g_disp"]), _lib.ptr(ups["g_acc"]), _lib.ptr(ups["g_raw"]), _lib.ptr(grad),
                                                   _lib.ptr(d_raw), _lib.stream_of(grad)), "render_pass_backward_tnerf")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(grad).all()) and bool(torch.isfinite(d_raw).all())
    assert float(grad.abs().max()) > 0 and float(d_raw.view(N, -1, 4)[:, S:].abs().max()) == 0      # rows past S carry zero gradients
    return {"grad": grad.cpu(), "d_raw": d_raw.cpu()}


def finish(tight):
    g = torch.Generator().manual_seed(8)
    r = lambda *s: torch.randn(*s, generator=g)
    host = dict(G=r(64, 128), db9=r(64), W9=SD["layer_9.0.weight"], Wf=SD["feature.0.weight"], bf=SD["feature.0.bias"], a4w=r(4, 128), a4b=r(4),
                dW9=r(64, 155), dWf=r(128, 128), dbf=r(128), dWd=r(1, 128), dbd=r(1))
    t = {k: place(v, tight) for k, v in host.items()}
    _lib.check(L.swnerf_tnerf_feature_finish(*[_lib.ptr(t[k]) for k in ("G", "db9", "W9")], 155, *[_lib.ptr(t[k]) for k in ("Wf", "bf", "a4w", "a4b", "dW9")],
                                             155, *[_lib.ptr(t[k]) for k in ("dWf", "dbf", "dWd", "dbd")], _lib.stream_of(t["G"])), "tnerf_feature_finish")
    torch.cuda.synchronize()
    return {k: t[k].cpu() for k in ("dW9", "dWf", "dbf", "dWd", "dbd")}


def same(a, b):
    for k in a:
        assert torch.equal(a[k], b[k]), k


def run(case):
    if case == "pack_bwd":
        assert torch.equal(pack(True, True).cpu(), pack(False, True).cpu())
    elif case == "train_forward":
        same({k: v.cpu() for k, v in forward(True)[1].items()}, {k: v.cpu() for k, v in forward(False)[1].items()})
    elif case == "backward":
        same(backward(True), backward(False))
    else:
        same(finish(True), finish(False))


for c in sys.argv[1:]:
    run(c)
    torch.cuda.synchronize()
    print(f"{c}: ok", flush=True)
