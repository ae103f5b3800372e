#!/usr/bin/env python3
"""Mesh welding and decimation by vertex clustering (swnerf.meshops cluster / collapse / emit, csrc/meshsimp_kernels.hip) on a mesh
that is already on the device, in the manner of tools/bench_meshops.py: the R^3 noise mesh extracted by
swnerf.mesh.marching_cubes, at cells of 2 and 4 grid spacings.  Per phase - cluster (table insert and labels), collapse (corner
lists, degenerate / duplicate faces, the two scans), emit in each placement (weld, mean, quadric; mean and quadric build their
member / corner lists) - and for decimate_arrays as a whole (quadric, normals recomputed): the median, minimum and maximum of
`--reps` timed calls after a warm-up call (device events around the call; cluster and collapse read their counts back, so they
include that synchronisation).  Beside each time: the bytes the phase has to move at the least (from V, F, V', F'), the rate that
makes, and its share of the plain device copy measured in the same run.
Prints ONE JSON line.
  python tools/bench_meshsimp.py [--resolution 256] [--reps 20] [--json out.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sw-nerf_amd"), ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import __graft_entry__ as ge

ge.compile_library_locked()                     # before the GPU is initialised
import numpy as np
import torch
import mc_numpy
from swnerf import _lib, mesh, meshops

ap = argparse.ArgumentParser()
ap.add_argument("--resolution", type=int, default=256)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--json", default=None)
opt = ap.parse_args()
assert torch.cuda.is_available(), "bench_meshsimp.py needs the MI355X"
DEV = torch.device("cuda:0")
RES = opt.resolution


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


def least_bytes(V, F, Vo, Fo):
    """the bytes each phase cannot avoid: every input read once, every output written once (workspace traffic not counted)"""
    return {"cluster": 12 * V + 4 * V, "collapse": 12 * F + 4 * V + 4 * (V + 1) + 4 * (F + 1),
            "emit_weld": 12 * F + 4 * V + 4 * (V + 1) + 4 * (F + 1) + 36 * Vo + 36 * Vo + 12 * Fo,
            "emit_mean": 12 * F + 4 * V + 4 * (V + 1) + 4 * (F + 1) + 24 * V + 24 * Vo + 12 * Fo,
            "emit_quadric": 12 * F + 4 * V + 4 * (V + 1) + 4 * (F + 1) + 24 * V + 24 * Vo + 12 * Fo}


src = torch.empty((256 << 20,), dtype=torch.uint8, device=DEV)
dst = torch.empty_like(src)
copy_ts, _ = event_ms(lambda: dst.copy_(src), opt.reps)
copy_gbs = 2 * src.numel() / float(np.median(copy_ts)) / 1e6                  # read + write
del src, dst
res = {"resolution": RES, "reps": opt.reps, "copy_GBps": round(copy_gbs, 1), "cells": {}}

f = torch.from_numpy(mc_numpy.noise((RES - 2,) * 3, seed=5)).to(DEV)
col = torch.rand(tuple(f.shape) + (3,), device=DEV)
v, fa, n, c = mesh.marching_cubes(f, 0.3, colors=col)
del f, col
V, F = int(v.shape[0]), int(fa.shape[0])
res.update(V=V, F=F)
ws = meshops._simplify_workspace(V, F, DEV)
res["workspace_MB"] = round(ws.numel() / 1e6, 1)
L, st = _lib.lib(), _lib.stream_of(v)

for cells in (2., 4.):
    h = float(np.float32(cells))                                             # the mesh is in index space: one spacing = 1
    vlabel, clusters, origin = meshops._cluster(v, h, None, ws)
    vmap, fpos, (Vo, Fo, ndeg, ndup) = meshops._collapse(fa, vlabel, V, ws)
    out = {"clusters": clusters, "V_out": Vo, "F_out": Fo, "degenerate": ndeg, "duplicate": ndup, "stages": {}}
    least = least_bytes(V, F, Vo, Fo)

    def report(stage, ts, nbytes=None):
        med = float(np.median(ts))
        e = {"ms": round(med, 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4)}
        if nbytes is not None:
            rate = nbytes / med / 1e6
            e.update(least_MB=round(nbytes / 1e6, 2), GBps=round(rate, 1), share_of_copy=round(rate / copy_gbs, 4))
        out["stages"][stage] = e

    report("cluster", event_ms(lambda: meshops._cluster(v, h, None, ws), opt.reps)[0], least["cluster"])
    report("collapse", event_ms(lambda: meshops._collapse(fa, vlabel, V, ws), opt.reps)[0], least["collapse"])
    vo = torch.empty((Vo, 3), dtype=torch.float32, device=DEV)
    no, co = torch.empty_like(vo), torch.empty_like(vo)
    fo = torch.empty((Fo, 3), dtype=torch.int32, device=DEV)
    status = torch.empty(1, dtype=torch.int32, device=DEV)
    for placement, code in meshops.PLACEMENTS.items():
        emit = lambda: _lib.check(L.swnerf_mesh_collapse_emit(_lib.ptr(v), _lib.ptr(fa), _lib.ptr(n), _lib.ptr(c), _lib.ptr(vlabel), _lib.ptr(vmap),
                                                              _lib.ptr(fpos), _lib.ptr(origin), h, V, F, code, 1e-3, _lib.ptr(ws), Vo, Fo, _lib.ptr(vo),
                                                              _lib.ptr(fo), _lib.ptr(no), _lib.ptr(co), _lib.ptr(status), st), "mesh_collapse_emit")
        report("emit_" + placement, event_ms(emit, opt.reps)[0], least["emit_" + placement])
    report("decimate_quadric_with_normals", event_ms(lambda: meshops.decimate_arrays(v, fa, n, c, cell=h), max(3, opt.reps // 4))[0])
    res["cells"][f"{cells:g}"] = out
    del vo, no, co, fo, vlabel, vmap, fpos
line = json.dumps(res)
print(line)
if opt.json:
    with open(opt.json, "w") as fh:
        fh.write(line + "\n")
