#!/usr/bin/env python3
"""Out-of-bounds guard for the mesh hole-filling entry points (swnerf_mesh_boundary, _boundary_loops, _fill_emit), in the manner of
tools/tight_buffer_check_meshsimp.py: every operand, every output and the workspace end exactly where a torch allocation of at
least 10 MB whose size is a multiple of 2 MB ends (the caching allocator then maps exactly that much), so a read or write past the
last element leaves the mapping and faults instead of touching a neighbour.  The shapes are three vertices with one face (a loop
of 3: one face, no vertex), a tetrahedron without its base (4 / 3, a loop of 3) and the 360 / 358 open sphere of
tests/meshops_ref.py (a loop of 52: a fan).  Every result is compared with the same call on ordinary allocations, bit for bit,
and with tests/meshfill_ref.py.
  tight_buffer_check_meshfill.py <case> [<case> ...]
  tight_buffer_check_meshfill.py list
tests/test_00_a_meshfill_tight_buffers.py starts it as a child process."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sw-nerf_amd"), ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
SHAPES = ["v3f1", "tet_open", "open_sphere"]
CALLS = ["boundary", "loops", "emit"]
CASES = [f"{c}-{s}" for c in CALLS for s in SHAPES]
if len(sys.argv) < 2 or sys.argv[1] == "list":
    print(" ".join(CASES))
    sys.exit(0)
for c in sys.argv[1:]:
    if c not in CASES:
        raise SystemExit(f"unknown case {c!r}; `list` prints them")

import numpy as np
import torch
import meshops_ref as R
import meshfill_ref as H
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
    for a, b in zip(tight_out[1:], loose_out[1:]):                 # [0] is the workspace
        assert torch.equal(a, b), what
    res = [t.cpu() for t in tight_out]
    del tight_in, tight_out, loose_in, loose_out
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return res


def mesh_of(shape):
    if shape == "v3f1":
        return np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]], np.int32)
    if shape == "tet_open":
        return np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32), np.array([[0, 1, 3], [1, 2, 3], [2, 0, 3]], np.int32)
    v, f, _ = R.fixtures()["open_sphere"]
    assert (len(v), len(f)) == (360, 358)
    return v, f


def run(case):
    L = _lib.lib()
    name, shape = case.split("-")
    v, f = mesh_of(shape)
    V, F = len(v), len(f)
    col = np.abs(v[:, ::-1]).copy()
    w = H.fill(v, f, col)
    b = H.boundary(f, V)
    nb, nl, M = len(b["bhe"]), len(w["table"]), len(w["loop_vertices"])
    cap = nb // 3
    tv, tf, tc = torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(col)
    i32 = lambda *shape: torch.full(shape, -1, dtype=torch.int32)
    f32 = lambda *shape: torch.full(shape, -1., dtype=torch.float32)
    ws = torch.zeros(L.swnerf_mesh_fill_workspace_bytes(V, F), dtype=torch.uint8)                     # ends with its allocation too
    bhe, bnext = torch.from_numpy(b["bhe"].astype(np.int32)), torch.from_numpy(b["next"].astype(np.int32))
    fan = w["table"][:, 1] >= 4
    vnew = torch.from_numpy(np.concatenate([[0], np.cumsum(fan)]).astype(np.int32))
    fnew = torch.from_numpy(np.concatenate([[0], np.cumsum(np.where(fan, w["table"][:, 1], 1))]).astype(np.int32))
    loop_offsets, loop_vertices = torch.from_numpy(w["loop_offsets"].astype(np.int32)), torch.from_numpy(w["loop_vertices"].astype(np.int32))
    if name == "boundary":
        call = lambda fa, wk, he, nx, cnt: L.swnerf_mesh_boundary(_lib.ptr(fa), V, F, _lib.ptr(wk), _lib.ptr(he), _lib.ptr(nx), _lib.ptr(cnt),
                                                                   _lib.stream_of(fa))
        _, he, nx, cnt = both(call, [tf], [ws, i32(3 * F), i32(3 * F), i32(2)], case)
        assert cnt.tolist() == [nb, 0] and torch.equal(he[:nb], bhe) and torch.equal(nx[:nb], bnext), case
        assert bool((he[nb:] == -1).all()) and bool((nx[nb:] == -1).all()), case
    elif name == "loops":
        call = lambda fa, he, nx, wk, tb, lo, lv, vn, fn, cnt: L.swnerf_mesh_boundary_loops(
            _lib.ptr(fa), _lib.ptr(he), _lib.ptr(nx), V, F, nb, 0, _lib.ptr(wk), _lib.ptr(tb), _lib.ptr(lo), _lib.ptr(lv), _lib.ptr(vn), _lib.ptr(fn),
            _lib.ptr(cnt), _lib.stream_of(fa))
        _, tb, lo, lv, vn, fn, cnt = both(call, [tf, bhe, bnext], [ws, i32(cap, 2), i32(cap + 1), i32(nb), i32(cap + 1), i32(cap + 1), i32(8)], case)
        info = w["info"]
        assert cnt.tolist() == [nl, M, info["filled_loops"], info["filled_edges"], info["new_vertices"], info["new_faces"], 0, 0], case
        assert np.array_equal(tb[:nl].numpy(), w["table"]) and torch.equal(lo[:nl + 1], loop_offsets) and torch.equal(lv[:M], loop_vertices), case
        assert torch.equal(vn[:nl + 1], vnew) and torch.equal(fn[:nl + 1], fnew), case
    else:
        Vo, Fo = len(w["verts"]), len(w["faces"])
        call = lambda ve, fa, co, lo, lv, vn, fn, wk, vo, fo, cout, st: L.swnerf_mesh_fill_emit(
            _lib.ptr(ve), _lib.ptr(fa), _lib.ptr(co), V, F, _lib.ptr(lo), _lib.ptr(lv), _lib.ptr(vn), _lib.ptr(fn), nl, M, _lib.ptr(wk), Vo, Fo,
            _lib.ptr(vo), _lib.ptr(fo), _lib.ptr(cout), _lib.ptr(st), _lib.stream_of(ve))
        _, vo, fo, co, st = both(call, [tv, tf, tc, loop_offsets, loop_vertices, vnew, fnew], [ws, f32(Vo, 3), i32(Fo, 3), f32(Vo, 3), i32(1)], case)
        assert st.tolist() == [0] and vo.numpy().tobytes() == w["verts"].tobytes() and np.array_equal(fo.numpy(), w["faces"]), case
        assert co.numpy().tobytes() == w["colors"].tobytes(), case
        assert (Vo - V, Fo - F) == ((1, 52) if shape == "open_sphere" else (0, 1)), case


for c in sys.argv[1:]:
    run(c)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    print(f"{c}: ok", flush=True)
