#!/usr/bin/env python3
"""Out-of-bounds guard for the grid query of the time-conditioned nets (swnerf_query_points_time), in the manner of
tools/tight_buffer_check.py: the packed blob, the points, the directions and both outputs end exactly where a torch allocation of
at least 10 MB whose size is a multiple of 2 MB ends (the caching allocator then maps exactly that much), so a read or write past
the last element leaves the mapping and faults instead of touching a neighbour.  Every operand is the TAIL of such an allocation;
the point count is no multiple of 32, so the last wave carries rows past M (they read row M-1 and store nothing).
  tight_buffer_check_query.py <case> [<case> ...]    cases: query_dnerf (deformation pass: shared directions with dx_out, then one
                                                     direction per point), query_dnerf_t0 (the t == 0 / zero_canonical branch:
                                                     canonical blob alone, dx_out = 0), query_tnerf (shared directions)
  tight_buffer_check_query.py list
tests/test_00_a_query_tight_buffers.py starts it as a child process."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sw-nerf_amd"), ROOT):
    sys.path.insert(0, p)
CASES = ["query_dnerf", "query_dnerf_t0", "query_tnerf"]
if len(sys.argv) < 2 or sys.argv[1] == "list":
    print(" ".join(CASES))
    sys.exit(0)
for c in sys.argv[1:]:
    if c not in CASES:
        raise SystemExit(f"unknown case {c!r}; `list` prints them")

import torch
from swnerf import _lib, synth, model, embedder

dev = torch.device("cuda:0")
MB2 = 2 << 20
M, V = (1 << 20) - 37, 8                         # 32767 whole tiles and one of 27 rows; the last workgroup has an idle wave


def tight_bytes(n):
    return max(10 << 20, (n + MB2 - 1) // MB2 * MB2)


def tail(shape):
    """a float32 tensor of `shape` that ends exactly at the end of a tight allocation"""
    n = 1
    for s in shape:
        n *= s
    buf = torch.empty(tight_bytes(4 * n) // 4, dtype=torch.float32, device=dev)
    return buf[buf.numel() - n:].view(shape)


def tail_of(host):
    """the host tensor, uploaded into the tail of a tight allocation (built on the host: no device temporaries whose freed blocks
    the caching allocator could hand out inside a later tight allocation)"""
    t = tail(tuple(host.shape))
    t.copy_(host)
    return t


def dnerf_net():
    embed_fn, c10 = embedder.get_embedder(10, 3, 0)
    m = model.NeRF.get_by_name("direct_temporal", D=8, W=256, input_ch=c10, output_ch=5, skips=[4], input_ch_views=27, input_ch_time=21,
                               use_viewdirs=True, embed_fn=embed_fn, zero_canonical=True)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.dnerf_state_dict(3, alpha_bias=-1.0).items()})
    return m.to(dev).eval()


def tnerf_net():
    m = model.TNeRF(depth=8, in_feat=63, dir_feat=27, time_feat=21, net_dim=128, skip_layer=4)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.tnerf_state_dict(141).items()})
    return m.to(dev).eval()


def run(case):
    L = _lib.lib()
    g = torch.Generator().manual_seed(5)
    kind, packed, Lp, Ld, Lt = (tnerf_net() if case == "query_tnerf" else dnerf_net()).packed()
    packed = tail_of(packed.cpu())
    pts = tail_of(torch.rand((M, 3), generator=g) * 4 - 2)
    d = torch.randn((V, 3), generator=g)
    dirs = tail_of(d / d.norm(dim=-1, keepdim=True))
    out = tail((M, 4))
    dx = None if case == "query_tnerf" else tail((M, 3))
    t, run_deform = (0.0, 0) if case == "query_dnerf_t0" else (0.5, 1)
    st = _lib.stream_of(pts)
    _lib.check(L.swnerf_query_points_time(kind, _lib.ptr(packed), _lib.ptr(pts), M, _lib.ptr(dirs), V, 1, t, run_deform, Lp, Ld, Lt,
                                          _lib.ptr(out), _lib.ptr(dx), st), case)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
    if case == "query_dnerf":
        assert bool(torch.isfinite(dx).all()) and float(dx.abs().max()) > 0
        d1 = torch.randn((M, 3), generator=g)
        rows = tail_of(d1 / d1.norm(dim=-1, keepdim=True))
        out1, dx1 = tail((M, 4)), tail((M, 3))
        _lib.check(L.swnerf_query_points_time(kind, _lib.ptr(packed), _lib.ptr(pts), M, _lib.ptr(rows), M, 0, t, run_deform, Lp, Ld, Lt,
                                              _lib.ptr(out1), _lib.ptr(dx1), st), case)
        torch.cuda.synchronize()
        assert torch.equal(dx1, dx) and torch.equal(out1[:, 3], out[:, 3]) and bool(torch.isfinite(out1).all())
    elif case == "query_dnerf_t0":
        assert float(dx.abs().max()) == 0.0


for c in sys.argv[1:]:
    run(c)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    print(f"{c}: ok", flush=True)
