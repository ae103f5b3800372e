#!/usr/bin/env python3
"""Mesh hole filling (swnerf.meshops boundary / loops / emit, csrc/meshfill_kernels.hip) on a mesh that is already on the device, in
the manner of tools/bench_meshsimp.py, on two meshes: the unpadded R^3 noise mesh extracted by swnerf.mesh.marching_cubes (many
short loops) and one long loop, the cone fan(n) of tests/meshops_ref.py with its faces permuted (next jumps at random).  Per phase
- boundary (corner lists, classify, scan, compact, next), loops (pointer jumping, ranks,
scans), emit (copy, faces, means) - and for fill_holes_arrays as a whole: the median, minimum and maximum of `--reps` timed calls
after a warm-up call (device events around the call).  Beside each time: the bytes the phase has to move at the least, the rate
that makes, and its share of the plain device copy measured in the same run; the loops phase also reports its launches.  For
context the numpy replay of tests/meshfill_ref.py is timed once on the host.
Prints ONE JSON line.
  python tools/bench_meshfill.py [--resolution 256] [--fan 1048576] [--reps 20] [--json out.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sw-nerf_amd"), ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import __graft_entry__ as ge

ge.compile_library_locked()                     # before the GPU is initialised
import numpy as np
import torch
import mc_numpy
import meshops_ref
import meshfill_ref
from swnerf import _lib, mesh, meshops

ap = argparse.ArgumentParser()
ap.add_argument("--resolution", type=int, default=256)
ap.add_argument("--fan", type=int, default=1 << 20)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--json", default=None)
opt = ap.parse_args()
assert torch.cuda.is_available(), "bench_meshfill.py needs the MI355X"
DEV = torch.device("cuda:0")


def event_ms(fn, reps):
    fn()                                                                     # warm-up: allocator, code objects
    torch.cuda.synchronize()
    ts, r = [], None
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return ts, r


src = torch.empty((256 << 20,), dtype=torch.uint8, device=DEV)
dst = torch.empty_like(src)
copy_ts, _ = event_ms(lambda: dst.copy_(src), opt.reps)
copy_gbs = 2 * src.numel() / float(np.median(copy_ts)) / 1e6                  # read + write
del src, dst
res = {"reps": opt.reps, "copy_GBps": round(copy_gbs, 1), "meshes": {}}


def bench(name, v, fa, c):
    V, F = int(v.shape[0]), int(fa.shape[0])
    L, st = _lib.lib(), _lib.stream_of(v)
    ws = meshops._fill_workspace(V, F, DEV)
    out = {"V": V, "F": F, "workspace_MB": round(ws.numel() / 1e6, 1), "stages": {}}

    def report(stage, ts, nbytes=None, **extra):
        med = float(np.median(ts))
        e = {"ms": round(med, 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4)}
        if nbytes is not None:
            rate = nbytes / med / 1e6
            e.update(least_MB=round(nbytes / 1e6, 2), GBps=round(rate, 1), share_of_copy=round(rate / copy_gbs, 4))
        e.update(extra)
        out["stages"][stage] = e

    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=DEV)
    bhe, bnext, counts = i32(3 * F), i32(3 * F), i32(2)
    boundary = lambda: _lib.check(L.swnerf_mesh_boundary(_lib.ptr(fa), V, F, _lib.ptr(ws), _lib.ptr(bhe), _lib.ptr(bnext), _lib.ptr(counts), st),
                                  "mesh_boundary")
    ts, _ = event_ms(boundary, opt.reps)
    nb = int(counts[0])
    report("boundary", ts, 12 * F + 8 * nb)
    cap = nb // 3
    table, lo, lv, vnew, fnew, cnt = i32(cap, 2), i32(cap + 1), i32(nb), i32(cap + 1), i32(cap + 1), i32(8)
    loops = lambda: _lib.check(L.swnerf_mesh_boundary_loops(_lib.ptr(fa), _lib.ptr(bhe), _lib.ptr(bnext), V, F, nb, 0, _lib.ptr(ws), _lib.ptr(table),
                                                            _lib.ptr(lo), _lib.ptr(lv), _lib.ptr(vnew), _lib.ptr(fnew), _lib.ptr(cnt), st), "mesh_boundary_loops")
    ts, _ = event_ms(loops, opt.reps)
    nl, M, _, _, Vn, Fn = (int(x) for x in cnt[:6].cpu())
    rounds = max(0, int(nb - 1).bit_length())
    report("loops", ts, 8 * nb + 4 * nb + 20 * nl, rounds=rounds, launches=2 * rounds + 16)
    out.update(boundary_edges=nb, loops=nl, longest_loop=int(table[:nl, 1].max()) if nl else 0, new_vertices=Vn, new_faces=Fn)
    Vo, Fo = V + Vn, F + Fn
    vo, fo, status = torch.empty((Vo, 3), dtype=torch.float32, device=DEV), i32(Fo, 3), i32(1)
    co = torch.empty_like(vo)
    emit = lambda: _lib.check(L.swnerf_mesh_fill_emit(_lib.ptr(v), _lib.ptr(fa), _lib.ptr(c), V, F, _lib.ptr(lo), _lib.ptr(lv), _lib.ptr(vnew),
                                                      _lib.ptr(fnew), nl, M, _lib.ptr(ws), Vo, Fo, _lib.ptr(vo), _lib.ptr(fo), _lib.ptr(co),
                                                      _lib.ptr(status), st), "mesh_fill_emit")
    report("emit", event_ms(emit, opt.reps)[0], 24 * V + 12 * F + 24 * Vo + 12 * Fo + 4 * M + 24 * M)
    report("fill_holes_arrays", event_ms(lambda: meshops.fill_holes_arrays(v, fa, None, c), max(3, opt.reps // 4))[0])
    hv, hf, hc = v.cpu().numpy(), fa.cpu().numpy(), c.cpu().numpy()
    t0 = time.perf_counter()
    w = meshfill_ref.fill(hv, hf, hc)
    out["numpy_replay_s"] = round(time.perf_counter() - t0, 3)
    assert np.array_equal(fo.cpu().numpy(), w["faces"]) and vo.cpu().numpy().tobytes() == w["verts"].tobytes()
    res["meshes"][name] = out


R = opt.resolution
f = torch.from_numpy(mc_numpy.noise((R, R, R), seed=5, pad=False)).to(DEV)
col = torch.rand(tuple(f.shape) + (3,), device=DEV)
v, fa, n, c = mesh.marching_cubes(f, 0.3, colors=col)
del f, col, n
bench(f"noise{R}", v, fa, c)
del v, fa, c
hv, hf = meshops_ref.fan(opt.fan)
bench(f"fan{opt.fan}", torch.from_numpy(hv).to(DEV), torch.from_numpy(meshfill_ref.permuted(hf, 1)).to(DEV), torch.rand((len(hv), 3), device=DEV))
line = json.dumps(res)
print(line)
if opt.json:
    with open(opt.json, "w") as fh:
        fh.write(line + "\n")
