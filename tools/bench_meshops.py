#!/usr/bin/env python3
"""Mesh clean-up and measurement (swnerf.meshops, csrc/meshops_kernels.hip) on meshes that are already on the device, as
generate_mesh(..., clean=...) runs it: a noise field (thousands of components, the union-find's and the atomics' hard case) and a
sphere (one component: every count lands on one address) at R^3, extracted by swnerf.mesh.marching_cubes.  Per stage - components
(with its host copy of the table), compaction of the largest component, incidence, one smoothing step, normals, measure - and for
clean(keep=1, smooth_iterations=10 and 1) + measure together: the median, minimum and maximum of `--reps` timed calls after a warm-up call
(device events around the call; stages that read a count back include that synchronisation).  Beside each time: the bytes the
stage has to move at the least (from V and F), the rate that makes, and its share of the plain device copy measured in the same
run.  The one comparison is the numpy replay of tests/meshops_ref.py on the host for the same mesh and one smoothing iteration
(informational: the replay is written to be read, not to be fast).
Prints ONE JSON line.
  python tools/bench_meshops.py [--resolution 256] [--reps 20] [--no-replay] [--json out.json]"""
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
import meshops_ref as R
from swnerf import mesh, meshops

ap = argparse.ArgumentParser()
ap.add_argument("--resolution", type=int, default=256)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--no-replay", action="store_true")
ap.add_argument("--json", default=None)
opt = ap.parse_args()
assert torch.cuda.is_available(), "bench_meshops.py needs the MI355X"
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
    """the bytes each stage cannot avoid: every input read once, every output written once"""
    csr = 4 * (V + 1) + 12 * F
    return {"components": 12 * F + 4 * V, "compaction": 36 * V + 12 * F + 4 * V + 36 * Vo + 12 * Fo, "incidence": 12 * F + csr,
            "smooth_step": 12 * V + 12 * F + csr + 12 * V, "normals": 12 * V + 12 * F + csr + 12 * V, "measure": 12 * V + 12 * F + csr}


src = torch.empty((256 << 20,), dtype=torch.uint8, device=DEV)
dst = torch.empty_like(src)
copy_ts, _ = event_ms(lambda: dst.copy_(src), opt.reps)
copy_gbs = 2 * src.numel() / float(np.median(copy_ts)) / 1e6                  # read + write
del src, dst
res = {"resolution": RES, "reps": opt.reps, "copy_GBps": round(copy_gbs, 1), "meshes": {}}


def bench(name, field, level):
    f = torch.from_numpy(field).to(DEV)
    col = torch.rand(field.shape + (3,), device=DEV)
    v, fa, n, c = mesh.marching_cubes(f, level, colors=col)
    del f, col
    V, F = int(v.shape[0]), int(fa.shape[0])
    out = {"V": V, "F": F, "stages": {}}
    vlabel, table = meshops.components(fa, V)
    rows = meshops.select_components(table, 1)
    Vo, Fo = int(rows[:, 2].sum()), int(rows[:, 1].sum())
    out.update(components=int(len(table)), largest_component_faces=Fo)
    inc = meshops.vertex_faces(fa, V)
    out["max_valence"] = int((inc[0][1:] - inc[0][:-1]).max())
    least = least_bytes(V, F, Vo, Fo)

    def report(stage, ts, nbytes=None):
        med = float(np.median(ts))
        e = {"ms": round(med, 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4)}
        if nbytes is not None:
            rate = nbytes / med / 1e6
            e.update(least_MB=round(nbytes / 1e6, 2), GBps=round(rate, 1), share_of_copy=round(rate / copy_gbs, 4))
        out["stages"][stage] = e

    report("components", event_ms(lambda: meshops.components(fa, V), opt.reps)[0], least["components"])
    report("compaction", event_ms(lambda: meshops._compact(v, fa, n, c, vlabel, rows), opt.reps)[0], least["compaction"])
    report("incidence", event_ms(lambda: meshops.vertex_faces(fa, V), opt.reps)[0], least["incidence"])
    report("smooth_step", event_ms(lambda: meshops.smooth_step(v, fa, 0.5, incidence=inc), opt.reps)[0], least["smooth_step"])
    report("normals", event_ms(lambda: meshops.vertex_normals(v, fa, incidence=inc), opt.reps)[0], least["normals"])
    report("measure", event_ms(lambda: meshops.measure_raw(v, fa, incidence=inc), opt.reps)[0], least["measure"])

    def clean_and_measure(iterations):
        cv, cf, cn, cc = meshops.clean_arrays(v, fa, n, c, keep=1, smooth_iterations=iterations)
        return meshops.measure_raw(cv, cf)

    report("clean10_plus_measure", event_ms(lambda: clean_and_measure(10), max(3, opt.reps // 4))[0])
    report("clean1_plus_measure", event_ms(lambda: clean_and_measure(1), max(3, opt.reps // 4))[0])
    if not opt.no_replay:
        hv, hf = v.cpu().numpy(), fa.cpu().numpy()
        t0 = time.perf_counter()
        wl, wt = R.component_table(hf, V)
        cv, cf = R.compact(hv, hf, wl, R.select(wt, 1)[:, 0])
        sv = R.smooth(cv, cf, 1)
        R.vertex_normals(sv, cf)
        R.measure(sv, cf)
        out["numpy_replay_clean1_plus_measure_s"] = round(time.perf_counter() - t0, 2)
    res["meshes"][name] = out
    del v, fa, n, c, vlabel, inc
    torch.cuda.empty_cache()


bench("noise", mc_numpy.noise((RES - 2,) * 3, seed=5), 0.3)
bench("sphere", mc_numpy.sphere(RES)[0], 0.)
line = json.dumps(res)
print(line)
if opt.json:
    with open(opt.json, "w") as fh:
        fh.write(line + "\n")
