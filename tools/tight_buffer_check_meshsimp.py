#!/usr/bin/env python3
"""Out-of-bounds guard for the mesh welding and decimation entry points (swnerf_mesh_cluster, _collapse, _collapse_emit in its three
placements), in the manner of tools/tight_buffer_check_meshops.py: every operand, every output and the workspace end exactly
where a torch allocation of at least 10 MB whose size is a multiple of 2 MB ends (the caching allocator then maps exactly that
much), so a read or write past the last element leaves the mapping and faults instead of touching a neighbour.  The shapes are
one vertex with one (degenerate) face, three vertices with one face, and the 360 / 716 sphere of tests/mc_numpy.py at a cell of
2.5 spacings (one cell per vertex for v3f1, so that its face survives).  Every result is compared with the same call on ordinary
allocations, bit for bit, and with tests/meshsimp_ref.py.
  tight_buffer_check_meshsimp.py <case> [<case> ...]
  tight_buffer_check_meshsimp.py list
tests/test_00_a_meshsimp_tight_buffers.py starts it as a child process."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sw-nerf_amd"), ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
SHAPES = ["v1f1", "v3f1", "sphere"]
CALLS = ["cluster", "collapse", "emit_weld", "emit_mean", "emit_quadric"]
CASES = [f"{c}_{s}" for c in CALLS for s in SHAPES]
if len(sys.argv) < 2 or sys.argv[1] == "list":
    print(" ".join(CASES))
    sys.exit(0)
for c in sys.argv[1:]:
    if c not in CASES:
        raise SystemExit(f"unknown case {c!r}; `list` prints them")

import numpy as np
import torch
import mc_numpy
import meshops_ref as R
import meshsimp_ref as S
from swnerf import _lib

dev = torch.device("cuda:0")
MB2 = 2 << 20
PLACE = {"weld": 0, "mean": 1, "quadric": 2}


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
    """-> (verts, faces, cell)"""
    if shape == "v1f1":
        return np.array([[0.25, -1., 3.]], np.float32), np.zeros((1, 3), np.int32), 0.5
    if shape == "v3f1":
        return np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]], np.int32), 0.75
    field, h = mc_numpy.sphere(16)
    v, f, _ = R.mc(field, 0., h)
    assert (len(v), len(f)) == (360, 716)
    return v, f, float(np.float32(2.5 * h))


def run(case):
    L = _lib.lib()
    name, shape = case.rsplit("_", 1)
    v, f, h = mesh_of(shape)
    V, F = len(v), len(f)
    tv, tf = torch.from_numpy(v), torch.from_numpy(f)
    nrm, col = torch.from_numpy(v[:, ::-1].copy()), torch.from_numpy(np.abs(v))
    i32 = lambda *shape: torch.full(shape, -1, dtype=torch.int32)
    f32 = lambda *shape: torch.full(shape, -1., dtype=torch.float32)
    wsz = lambda Fw: torch.zeros(L.swnerf_mesh_simplify_workspace_bytes(V, Fw), dtype=torch.uint8)      # ends with its allocation too
    c = S.cluster(v, h)
    k = S.collapse(f, c["vlabel"], V)
    vlabel = torch.from_numpy(c["vlabel"].astype(np.int32))
    used = np.zeros(V + 1, np.int64)
    used[k["labels"]] = 1
    vmap = torch.from_numpy(np.concatenate([[0], np.cumsum(used)[:-1]]).astype(np.int32))
    fpos = torch.from_numpy(np.concatenate([[0], np.cumsum(k["keep"])]).astype(np.int32))
    Vo, Fo = k["V_out"], k["F_out"]
    if name == "cluster":
        call = lambda ve, w, lab, org, cnt: L.swnerf_mesh_cluster(_lib.ptr(ve), V, None, h, _lib.ptr(w), _lib.ptr(lab), _lib.ptr(org), _lib.ptr(cnt),
                                                                  _lib.stream_of(ve))
        _, lab, org, cnt = both(call, [tv], [wsz(0), i32(V), f32(3), i32(3)], case)
        assert cnt.tolist() == [c["clusters"], 0, 0] and np.array_equal(lab.numpy(), c["vlabel"]) and org.numpy().tobytes() == c["origin"].tobytes(), case
    elif name == "collapse":
        call = lambda fa, lab, w, vm, fp, cnt: L.swnerf_mesh_collapse(_lib.ptr(fa), _lib.ptr(lab), V, F, _lib.ptr(w), _lib.ptr(vm), _lib.ptr(fp),
                                                                      _lib.ptr(cnt), _lib.stream_of(fa))
        _, vm, fp, cnt = both(call, [tf, vlabel], [wsz(F), i32(V + 1), i32(F + 1), i32(5)], case)
        assert cnt.tolist() == [Vo, Fo, k["degenerate"], k["duplicate"], 0] and torch.equal(vm, vmap) and torch.equal(fp, fpos), case
    else:
        placement = name[len("emit_"):]
        w = S.simplify(v, f, nrm.numpy(), col.numpy(), h, placement)
        org = torch.from_numpy(c["origin"].copy())
        call = lambda ve, fa, no, co, lab, vm, fp, og, wk, vo, fo, nout, cout, st: L.swnerf_mesh_collapse_emit(
            _lib.ptr(ve), _lib.ptr(fa), _lib.ptr(no), _lib.ptr(co), _lib.ptr(lab), _lib.ptr(vm), _lib.ptr(fp), _lib.ptr(og), h, V, F, PLACE[placement],
            1e-3, _lib.ptr(wk), Vo, Fo, _lib.ptr(vo), _lib.ptr(fo), _lib.ptr(nout), _lib.ptr(cout), _lib.ptr(st), _lib.stream_of(ve))
        _, vo, fo, no, co, st = both(call, [tv, tf, nrm, col, vlabel, vmap, fpos, org], [wsz(F), f32(Vo, 3), i32(Fo, 3), f32(Vo, 3), f32(Vo, 3), i32(1)],
                                     case)
        assert st.tolist() == [0] and vo.numpy().tobytes() == w["verts"].tobytes() and np.array_equal(fo.numpy(), w["faces"]), case
        assert co.numpy().tobytes() == w["colors"].tobytes(), case
        assert no.numpy().tobytes() == (w["normals"] if placement == "weld" else np.full((Vo, 3), -1., np.float32)).tobytes(), case
        if shape == "v3f1":
            assert (Vo, Fo) == (3, 1), case
        if shape == "sphere":
            assert Vo > 20 and Fo > 40, case


for c in sys.argv[1:]:
    run(c)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    print(f"{c}: ok", flush=True)
