#!/usr/bin/env python3
"""Out-of-bounds guard for the marching-cubes entry points (swnerf_mc_count / swnerf_mc_emit), in the manner of
tools/tight_buffer_check.py: every operand, the workspace and every output end exactly where a torch allocation of at least
10 MB whose size is a multiple of 2 MB ends (the caching allocator then maps exactly that much), so a read or write past
the last element leaves the mapping and faults instead of touching a neighbour.  Outputs are the TAILS of such
allocations, sized by the counts the count pass returns.
  tight_buffer_check_mesh.py <case> [<case> ...]     cases: mc_ld1 (dense [nx,ny,nz] field, [nx,ny,nz,3] colours),
                                                     mc_ld4 (sigma / rgb columns of a [nx,ny,nz,4] query output)
  tight_buffer_check_mesh.py list
tests/test_00_a_mesh_tight_buffers.py starts it as a child process."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sw-nerf_amd"), ROOT):
    sys.path.insert(0, p)
CASES = ["mc_ld1", "mc_ld4"]
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


def tight_bytes(n):
    return max(10 << 20, (n + MB2 - 1) // MB2 * MB2)


def tail(nbytes, dtype, shape):
    """a tensor of `shape` that ends exactly at the end of a tight allocation"""
    es = torch.empty((), dtype=dtype).element_size()
    buf = torch.empty(tight_bytes(nbytes) // es, dtype=dtype, device=dev)
    n = 1
    for s in shape:
        n *= s
    return buf[buf.numel() - n:].view(shape)


def field(shape):
    """a wavy field whose surface reaches every face of the grid, the last points included (built on the host: no device
    temporaries whose freed blocks the caching allocator could hand out inside a later tight allocation)"""
    ii = [torch.arange(s, dtype=torch.float32) for s in shape]
    X, Y, Z = torch.meshgrid(*ii, indexing="ij")
    return torch.sin(X * 0.37) + torch.cos(Y * 0.23) + torch.sin(Z * 0.51 + 0.3) - 0.2


def run(case):
    L = _lib.lib()
    if case == "mc_ld1":
        shape = (160, 128, 128)                                  # 2^21 * 1.25 floats = 10 MB exactly
        f = tail(4 * 160 * 128 * 128, torch.float32, shape)
        f.copy_(field(shape))
        cols = tail(12 * 160 * 128 * 128, torch.float32, shape + (3,))
        cols.copy_(torch.rand(shape + (3,)))
        fp, cp, ld, cld = f, cols, 1, 3
    else:
        shape = (80, 128, 128)                                   # [80,128,128,4] = 20 MB
        q = tail(16 * 80 * 128 * 128, torch.float32, shape + (4,))
        h = torch.rand(shape + (4,))
        h[..., 3] = field(shape)
        q.copy_(h)
        fp, cp, ld, cld = q[..., 3], q[..., :3], 4, 4
    nx, ny, nz = shape
    st = _lib.stream_of(fp)
    wsb = L.swnerf_mc_workspace_bytes(nx, ny, nz)
    ws = tail(wsb, torch.uint8, (wsb,))
    tot = tail(16, torch.int64, (2,))
    _lib.check(L.swnerf_mc_count(_lib.ptr(fp), nx, ny, nz, ld, 0.0, _lib.ptr(ws), _lib.ptr(tot), st), "mc_count")
    V, F = (int(x) for x in tot.cpu())
    assert V > 100000 and F > 100000, (V, F)
    verts = tail(12 * V, torch.float32, (V, 3))
    normals = tail(12 * V, torch.float32, (V, 3))
    vcol = tail(12 * V, torch.float32, (V, 3))
    faces = tail(12 * F, torch.int32, (F, 3))
    f3 = (ctypes.c_float * 3)(1.0, 1.0, 1.0)
    z3 = (ctypes.c_float * 3)(0.0, 0.0, 0.0)
    _lib.check(L.swnerf_mc_emit(_lib.ptr(fp), _lib.ptr(cp), nx, ny, nz, ld, cld, 0.0, f3, z3, _lib.ptr(ws), V, F,
                                _lib.ptr(verts), _lib.ptr(faces), _lib.ptr(normals), _lib.ptr(vcol), st), "mc_emit")
    torch.cuda.synchronize()
    assert int(faces.min()) == 0 and int(faces.max()) == V - 1
    hi = torch.tensor([nx - 1, ny - 1, nz - 1], dtype=torch.float32, device=dev)
    assert bool((verts >= 0).all()) and bool((verts <= hi).all())


for c in sys.argv[1:]:
    run(c)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    print(f"{c}: ok", flush=True)
