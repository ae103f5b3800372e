#!/usr/bin/env python3
"""Mesh rendering (swnerf.meshrender, csrc/meshrender_kernels.hip) on meshes that are already on the device, in the manner of
tools/bench_meshfill.py: the raster pass (z-buffer memset + the (view, face) launch) and the resolve pass timed separately - the
median, minimum and maximum of `--reps` timed calls after a warm-up call, device events around the call - on
  noise<R>      the unpadded R^3 noise mesh of tools/bench_meshops.py extracted by swnerf.mesh.marching_cubes (faces about a pixel wide),
                at `--side`^2 for 1 view and for `--views` views in one call
  decimated     the same mesh through vertex clustering with cell 4 (faces a few pixels wide)
  big1000       1000 triangles, each about the size of the image: the wave tier's worst case
Beside each time: the bytes the pass has to move at the least (raster: faces + gathered vertices per view and the z-buffer twice;
resolve: the z-buffer once and the six outputs), the rate that makes and its share of the plain device copy measured in the same
run; the four counters of the raster pass (the pairs taken by the wave tier among them) and the hits per second.
Prints ONE JSON line.
  python tools/bench_meshrender.py [--resolution 256] [--side 800] [--views 40] [--reps 10] [--json out.json]"""
import argparse
import ctypes
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
import meshrender_ref
from swnerf import _lib, mesh, meshops

ap = argparse.ArgumentParser()
ap.add_argument("--resolution", type=int, default=256)
ap.add_argument("--side", type=int, default=800)
ap.add_argument("--views", type=int, default=40)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--json", default=None)
opt = ap.parse_args()
assert torch.cuda.is_available(), "bench_meshrender.py needs the MI355X"
DEV = torch.device("cuda:0")


def event_ms(fn, reps):
    fn()                                                                     # warm-up: allocator, code objects
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return ts


src = torch.empty((256 << 20,), dtype=torch.uint8, device=DEV)
dst = torch.empty_like(src)
copy_ts = event_ms(lambda: dst.copy_(src), opt.reps)
copy_gbs = 2 * src.numel() / float(np.median(copy_ts)) / 1e6                  # read + write
del src, dst
res = {"reps": opt.reps, "copy_GBps": round(copy_gbs, 1), "side": opt.side, "cases": {}}


def circle(verts, n, focal_fill=1.15):
    """n poses on a tilted circle around the mesh's box centre and the focal length at which its bounding sphere fills the image"""
    lo, hi = verts.amin(0).cpu().numpy(), verts.amax(0).cpu().numpy()
    centre, radius = (lo + hi) / 2, float(np.linalg.norm(hi - lo)) / 2
    dist = 2.7 * radius
    poses = np.stack([meshrender_ref.pose(2 * np.pi * (k + 0.25) / n, -0.45, dist, centre) for k in range(n)])
    return poses, float(opt.side / 2 * dist / (radius * focal_fill))


def bench(name, v, fa, c, n_views, poses=None, focal=None):
    V, F, H, W = int(v.shape[0]), int(fa.shape[0]), opt.side, opt.side
    if poses is None:
        poses, focal = circle(v, n_views)
    N = len(poses)
    L, st = _lib.lib(), _lib.stream_of(v)
    c2w = torch.from_numpy(np.ascontiguousarray(poses, np.float32)).to(DEV)
    ws = torch.empty(int(L.swnerf_mesh_render_workspace_bytes(N, H, W)), dtype=torch.uint8, device=DEV)
    counts = torch.empty(4, dtype=torch.int64, device=DEV)
    cam = (N, H, W, focal, focal, 0., 0., 1)
    raster = lambda: _lib.check(L.swnerf_mesh_render_raster(_lib.ptr(v), _lib.ptr(fa), V, F, _lib.ptr(c2w), *cam, 0., float("inf"), 0, _lib.ptr(ws),
                                                            _lib.ptr(counts), st), "mesh_render_raster")
    new = lambda *tail, dtype=torch.float32: torch.empty((N, H, W) + tail, dtype=dtype, device=DEV)
    rgb, depth, disp, acc, face, bary = new(3), new(), new(), new(), new(dtype=torch.int32), new(3)
    bg = (ctypes.c_float * 3)(1., 1., 1.)
    resolve = lambda: _lib.check(L.swnerf_mesh_render_resolve(_lib.ptr(v), _lib.ptr(fa), None, _lib.ptr(c), V, F, _lib.ptr(c2w), *cam, 0, bg, _lib.ptr(ws),
                                                              _lib.ptr(rgb), _lib.ptr(depth), _lib.ptr(disp), _lib.ptr(acc), _lib.ptr(face),
                                                              _lib.ptr(bary), st), "mesh_render_resolve")
    out = {"V": V, "F": F, "views": N, "focal": round(focal, 1), "zbuffer_MB": round(8 * N * H * W / 1e6, 1), "stages": {}}

    def report(stage, ts, nbytes, **extra):
        med = float(np.median(ts))
        rate = nbytes / med / 1e6
        out["stages"][stage] = dict(ms=round(med, 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4), least_MB=round(nbytes / 1e6, 2),
                                    GBps=round(rate, 1), share_of_copy=round(rate / copy_gbs, 4), **extra)

    ts = event_ms(raster, opt.reps)
    bad, behind, wide, hits = (int(x) for x in counts.cpu())
    med = float(np.median(ts))
    report("raster", ts, N * 48 * F + 16 * N * H * W, bad_faces=bad, pairs_behind=behind, pairs_wide=wide, hits=hits,
           Mpairs_per_s=round(N * F / med / 1e3, 1), Mhits_per_s=round(hits / med / 1e3, 1))
    report("resolve", event_ms(resolve, opt.reps), 8 * N * H * W + 40 * N * H * W)
    out["covered_pixels"] = int((face >= 0).sum())
    res["cases"][name] = out
    print(name, json.dumps(out), file=sys.stderr, flush=True)


R = opt.resolution
f = torch.from_numpy(mc_numpy.noise((R, R, R), seed=5, pad=False)).to(DEV)
col = torch.rand(tuple(f.shape) + (3,), device=DEV)
v, fa, n, c = mesh.marching_cubes(f, 0.3, colors=col)
del f, col, n
bench(f"noise{R}_1view", v, fa, c, 1)
bench(f"noise{R}_{opt.views}views", v, fa, c, opt.views)
dv, df, _, dc = meshops.simplify_arrays(v, fa, None, c, cell=4.0)
del v, fa, c
bench("decimated_1view", dv, df, dc, 1)
bench(f"decimated_{opt.views}views", dv, df, dc, opt.views)
del dv, df, dc
# 1000 triangles in planes z = -k / 1000 below a camera at z = 2 that looks down -z: each covers the image and more
rng = np.random.default_rng(2)
ang = rng.random(1000) * 2 * np.pi
tri = np.stack([np.stack([3 * np.cos(ang + q), 3 * np.sin(ang + q), -np.arange(1000) / 1000.], 1) for q in (0., 2.1, 4.2)], 1).astype(np.float32)
cam = np.array([[[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 2.0]]], np.float32)
bench("big1000", torch.from_numpy(tri.reshape(-1, 3)).to(DEV), torch.arange(3000, dtype=torch.int32, device=DEV).reshape(1000, 3),
      torch.rand((3000, 3), device=DEV), 1, poses=cam, focal=float(opt.side))
line = json.dumps(res)
print(line)
if opt.json:
    with open(opt.json, "w") as fh:
        fh.write(line + "\n")
