#!/usr/bin/env python3
"""Out-of-bounds guard for the mesh clean-up and measurement entry points (swnerf_mesh_components, _compact, _incidence,
_smooth_step, _vertex_normals, _measure), in the manner of tools/tight_buffer_check_images.py: every operand, every output and the
workspace end exactly where a torch allocation of at least 10 MB whose size is a multiple of 2 MB ends (the caching allocator
then maps exactly that much), so a read or write past the last element leaves the mapping and faults instead of touching a
neighbour.  The shapes are one vertex with one (degenerate) face, three vertices with one face, and the 360 / 716 sphere of
tests/mc_numpy.py; [V,3] float32 and [F,3] int32 rows are 12 bytes, so a 16-byte access at the last row would cross the end.
Every result is compared with the same call on ordinary allocations, bit for bit, and with tests/meshops_ref.py.
  tight_buffer_check_meshops.py <case> [<case> ...]
  tight_buffer_check_meshops.py list
tests/test_00_a_meshops_tight_buffers.py starts it as a child process."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sw-nerf_amd"), ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
SHAPES = ["v1f1", "v3f1", "sphere"]
CALLS = ["components", "compact", "incidence", "smooth_step", "vertex_normals", "measure"]
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


def mesh_of(shape):
    if shape == "v1f1":
        return np.array([[0.25, -1., 3.]], np.float32), np.zeros((1, 3), np.int32)
    if shape == "v3f1":
        return np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]], np.int32)
    field, h = mc_numpy.sphere(16)
    v, f, _ = R.mc(field, 0., h)
    assert (len(v), len(f)) == (360, 716)
    return v, f


def run(case):
    L = _lib.lib()
    name, shape = case.rsplit("_", 1)
    v, f = mesh_of(shape)
    V, F = len(v), len(f)
    tv, tf = torch.from_numpy(v), torch.from_numpy(f)
    ws = torch.zeros(L.swnerf_mesh_workspace_bytes(V, F), dtype=torch.uint8)          # the workspace ends with its allocation too
    i32 = lambda *shape: torch.full(shape, -1, dtype=torch.int32)
    f32 = lambda *shape: torch.full(shape, -1., dtype=torch.float32)
    offsets, items = (torch.from_numpy(a) for a in R.incidence(f, V))
    if name == "components":
        call = lambda fa, w, lab, tab, cnt: L.swnerf_mesh_components(_lib.ptr(fa), V, F, _lib.ptr(w), _lib.ptr(lab), _lib.ptr(tab), _lib.ptr(cnt),
                                                                     _lib.stream_of(fa))
        _, lab, tab, cnt = both(call, [tf], [ws, i32(V), i32(V, 3), i32(2)], case)
        wl, wt = R.component_table(f, V)
        assert cnt.tolist() == [len(wt), 0] and np.array_equal(lab.numpy(), wl) and np.array_equal(tab.numpy()[:len(wt)], wt), case
    elif name == "compact":
        wl, wt = R.component_table(f, V)
        rows = R.select(wt, 1)
        Vo, Fo = int(rows[:, 2].sum()), int(rows[:, 1].sum())
        nrm, col = torch.from_numpy(v[:, ::-1].copy()), torch.from_numpy(np.abs(v))
        call = lambda ve, fa, no, co, lab, kept, w, vo, fo, nout, cout: L.swnerf_mesh_compact(
            _lib.ptr(ve), _lib.ptr(fa), _lib.ptr(no), _lib.ptr(co), _lib.ptr(lab), V, F, _lib.ptr(kept), len(rows), _lib.ptr(w), Vo, Fo,
            _lib.ptr(vo), _lib.ptr(fo), _lib.ptr(nout), _lib.ptr(cout), _lib.stream_of(ve))
        _, vo, fo, no, co = both(call, [tv, tf, nrm, col, torch.from_numpy(wl.astype(np.int32)), torch.from_numpy(rows[:, 0].astype(np.int32))],
                                 [ws, f32(Vo, 3), i32(Fo, 3), f32(Vo, 3), f32(Vo, 3)], case)
        wv, wf, wn, wc = R.compact(v, f, wl, rows[:, 0], nrm.numpy(), col.numpy())
        assert np.array_equal(vo.numpy(), wv) and np.array_equal(fo.numpy(), wf) and np.array_equal(no.numpy(), wn) and np.array_equal(co.numpy(), wc), case
    elif name == "incidence":
        call = lambda fa, w, off, it, st: L.swnerf_mesh_incidence(_lib.ptr(fa), V, F, _lib.ptr(w), _lib.ptr(off), _lib.ptr(it), _lib.ptr(st),
                                                                  _lib.stream_of(fa))
        _, off, it, st = both(call, [tf], [ws, i32(V + 1), i32(3 * F), i32(1)], case)
        assert st.tolist() == [0] and torch.equal(off, offsets) and torch.equal(it, items), case
    elif name == "smooth_step":
        call = lambda ve, fa, off, it, out: L.swnerf_mesh_smooth_step(_lib.ptr(ve), _lib.ptr(fa), _lib.ptr(off), _lib.ptr(it), V, F, 0.5,
                                                                      _lib.ptr(out), _lib.stream_of(ve))
        out, = both(call, [tv, tf, offsets, items], [f32(V, 3)], case)
        assert out.numpy().tobytes() == R.smooth_step(v, f, 0.5).tobytes(), case
    elif name == "vertex_normals":
        call = lambda ve, fa, off, it, out: L.swnerf_mesh_vertex_normals(_lib.ptr(ve), _lib.ptr(fa), _lib.ptr(off), _lib.ptr(it), V, F,
                                                                         _lib.ptr(out), _lib.stream_of(ve))
        out, = both(call, [tv, tf, offsets, items], [f32(V, 3)], case)
        assert np.abs(out.numpy().astype(np.float64) - R.vertex_normals(v, f)).max() <= 2.0 ** -23, case
    else:
        call = lambda ve, fa, off, it, w, val, cnt: L.swnerf_mesh_measure(_lib.ptr(ve), _lib.ptr(fa), _lib.ptr(off), _lib.ptr(it), V, F, _lib.ptr(w),
                                                                          _lib.ptr(val), _lib.ptr(cnt), _lib.stream_of(ve))
        _, val, cnt = both(call, [tv, tf, offsets, items], [ws, torch.full((16,), -1., dtype=torch.float64), torch.full((8,), -1, dtype=torch.int64)], case)
        w = R.measure(v, f)
        assert cnt.tolist() == [w["referenced_vertices"], w["edges"], w["boundary_edges"], w["nonmanifold_edges"], w["n_components"], w["euler"],
                                int(w["closed"]), 0], case
        bound = 2 * F * 2.0 ** -53 * np.abs(w["terms"]).sum(0)                         # F additions per sum (tests/test_gpu_meshops.py)
        assert (np.abs(val.numpy()[:5] - w["sums"]) <= bound).all(), (case, val.numpy()[:5].tolist(), w["sums"].tolist())
        assert np.array_equal(val.numpy()[5:8], w["bbox_min"]) and np.array_equal(val.numpy()[8:11], w["bbox_max"]), case


for c in sys.argv[1:]:
    run(c)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    print(f"{c}: ok", flush=True)
