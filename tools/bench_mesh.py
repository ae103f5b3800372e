#!/usr/bin/env python3
"""Throughput of the mesh-extraction grid query (nerf/extract_mesh.py sample_grid: resolution^3 points x
100 view directions through model_fine) on one MI355X: fused shared-direction kernel vs the reference's
loop structure (one full network query per view direction) on the same kernels; then marching cubes (swnerf_mc_count /
swnerf_mc_emit) per pass on a sphere and a noise field, and nerf_to_mesh against the query alone.
  python tools/bench_mesh.py              everything
  python tools/bench_mesh.py --mc 512     only the marching-cubes passes at 512^3 (for a rocprofv3 --kernel-trace --stats run)
  python tools/bench_mesh.py --dnerf      only the grid query of the seeded DirectTemporalNeRF at t = 0.5 (swnerf_query_points_time) against
  python tools/bench_mesh.py --tnerf      / TNeRF                    the op path (embed + one full network call per direction)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sw-nerf_amd"), ROOT):
    sys.path.insert(0, p)
import numpy as np
import torch
from swnerf import synth, model, mesh

dev = torch.device("cuda:0")
net = model.vallina_NeRF(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=5, skips=[4], use_viewdirs=True)
net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.nerf_state_dict(synth.NET_FINE[0], alpha_bias=synth.NET_FINE[1]).items()})
net = net.to(dev).eval()
R, V = 128, 100
bounds = [(-1., 1.), (-1., 2.), (-4., 2.)]
ax = [np.linspace(b[0], b[1], R) for b in bounds]
X, Y, Z = np.meshgrid(*ax, indexing="ij")
pts = torch.tensor(np.stack([X.ravel(), Y.ravel(), Z.ravel()], -1), dtype=torch.float32, device=dev)
dirs = torch.tensor(mesh.generate_viewdirs(V), dtype=torch.float32, device=dev)
M = pts.shape[0]
MC_ONLY = [int(sys.argv[sys.argv.index("--mc") + 1])] if "--mc" in sys.argv else None

# ---------------------------------------------------------------- time-conditioned nets at one frame time (swnerf_query_points_time)
PEAK_TFLOPS = 157.3                                                              # fp32 MFMA, 2.4 GHz
MFMA_FLOP = 32 * 32 * 2 * 2                                                      # one v_mfma_f32_32x32x2_f32


def timed_query_row(which, t=0.5):
    """fused query, then - same process, after a shared warm-up - the op path (what the parent of this feature had to run): the
    embedders and one full network call per direction, on 1/16 of the grid, extrapolated"""
    from swnerf import embedder
    e10, e4, et = embedder.get_embedder(10, 3, 0)[0], embedder.get_embedder(4, 3, 0)[0], embedder.get_embedder(10, 1, 0)[0]
    if which == "dnerf":
        tnet = model.DirectTemporalNeRF(D=8, W=256, input_ch=63, input_ch_views=27, input_ch_time=21, output_ch=5, skips=[4],
                                        use_viewdirs=True, embed_fn=e10, zero_canonical=True)
        tnet.load_state_dict({k: torch.from_numpy(v) for k, v in synth.dnerf_state_dict(synth.NET_DNERF[0], alpha_bias=synth.NET_DNERF[1]).items()})
        # per 32 points (swnerf_common.h): TIME 32 + deformation (SW_DEFORM_STEPS - 32) 1920 + canonical trunk 1920 steps, views loop 144 per direction
        mfma = 4 * (32 + 1920 + 1920) + 4 * 144 * V
    else:
        tnet = model.TNeRF(depth=8, in_feat=63, dir_feat=27, time_feat=21, net_dim=128, skip_layer=4)
        tnet.load_state_dict({k: torch.from_numpy(v) for k, v in synth.tnerf_state_dict(141).items()})
        # T0 16 + T5 16 + MAIN without layer_9 (544 - 32) steps, DIR 8 + layer_9 32 per direction
        mfma = 4 * (16 + 16 + 512) + 4 * (8 + 32) * V
    tnet = tnet.to(dev).eval()
    sub = pts[:M // 16]

    def op_path(v):
        d = dirs[v:v + 1].expand(sub.shape[0], 3)
        te = et(torch.full((sub.shape[0], 1), t, device=dev))
        if which == "dnerf":
            return tnet(torch.cat([e10(sub), e4(d)], -1), [te, te])[0]
        ed = e4(d)
        return tnet(torch.cat([e10(sub), ed], -1), ed, te).reshape(-1, 4)

    with torch.no_grad():
        mesh.query_points(tnet, pts[:4096], dirs, True, frame_time=t)             # shared warm-up: pack, kernels, allocator
        op_path(0)
        torch.cuda.synchronize()
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            out = mesh.query_points(tnet, pts, dirs, True, frame_time=t)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        t_fused = min(ts)
        t0 = time.perf_counter()
        acc = torch.zeros((sub.shape[0], 4), device=dev)
        for v in range(V):
            acc += op_path(v)
        torch.cuda.synchronize()
        t_loop = (time.perf_counter() - t0) * 16
        err = float((acc[:, :3] / V - out[:M // 16, :3]).abs().max())
    tf = (M / 32) * mfma * MFMA_FLOP / t_fused / 1e12
    print(f"| {which} grid {R}^3 = {M:,} points x {V} view directions at t = {t} | fused query (swnerf_query_points_time) | {t_fused*1e3:.1f} ms | "
          f"{M*V/t_fused/1e6:.0f} M point-views/s | {mfma} MFMAs per 32 points: {tf:.1f} TFLOP/s executed = {tf / PEAK_TFLOPS * 100:.1f} % of the fp32-MFMA peak |")
    print(f"| same, op path: embed + one full network call per direction (extrapolated from 1/16 of the grid) | | {t_loop*1e3:.0f} ms | "
          f"{M*V/t_loop/1e6:.0f} M point-views/s | {t_loop / t_fused:.1f} x the fused query |")
    print(f"| max abs difference of the view-averaged colours between the two | {err:.2e} | | | |")


if "--dnerf" in sys.argv or "--tnerf" in sys.argv:
    for which in ("dnerf", "tnerf"):
        if "--" + which in sys.argv:
            timed_query_row(which)
    sys.exit(0)
if not MC_ONLY:
    with torch.no_grad():
        mesh.query_points(net, pts[:4096], dirs, True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = mesh.query_points(net, pts, dirs, True)
        torch.cuda.synchronize()
        t_fused = time.perf_counter() - t0
        sub = pts[:M // 16]                                # the per-view loop on 1/16 of the grid, scaled
        t0 = time.perf_counter()
        acc = torch.zeros((sub.shape[0], 4), device=dev)
        for v in range(V):
            acc += mesh.query_points(net, sub, dirs[v:v + 1].expand(sub.shape[0], 3).contiguous(), False)
        torch.cuda.synchronize()
        t_loop = (time.perf_counter() - t0) * 16
        err = float((acc[:, :3] / V - out[:M // 16, :3]).abs().max())
    flop_fused = M * 2 * (593408 - 20480 - 18432 + V * (18432 + 128 * 3 + 283 * 128 - 18432))   # informational only
    print(f"| grid {R}^3 = {M:,} points x {V} view directions | fused shared-direction query | {t_fused*1e3:.0f} ms | {M*V/t_fused/1e6:.0f} M point-views/s |")
    print(f"| same, one full network query per direction (the reference's loop, extrapolated from 1/16 of the grid) | | {t_loop*1e3:.0f} ms | {M*V/t_loop/1e6:.0f} M point-views/s |")
    print(f"| max abs difference of the view-averaged colours between the two | {err:.2e} | | |")

# ---------------------------------------------------------------- marching cubes (swnerf_mc_count / swnerf_mc_emit)
import ctypes
from swnerf import _lib
COPY_TBS = 6.29                                                                  # README: device copy rate


def mc_field(kind, R):
    g = torch.Generator(device=dev).manual_seed(7)
    if kind == "sphere":
        x = torch.linspace(-1, 1, R, device=dev)
        X, Y, Z = torch.meshgrid(x, x, x, indexing="ij")
        return 0.6 - torch.sqrt(X * X + Y * Y + Z * Z)
    f = torch.randn((R, R, R), device=dev, generator=g)
    for a in range(3):
        f = (f + f.roll(1, a) + f.roll(-1, a)) / 3
    return f


def mc_passes(f, ld, level, reps=5):
    """ms of the count pass (classify + tile scan) and of the emit pass (vertices + triangles), best of `reps`"""
    L = _lib.lib()
    R = f.shape[0]
    if ld == 4:
        q = torch.zeros((R, R, R, 4), device=dev)
        q[..., 3] = f
        fp, cp = q[..., 3], q[..., :3]
    else:
        fp, cp = f.contiguous(), None
    st = _lib.stream_of(fp)
    ws = torch.empty(L.swnerf_mc_workspace_bytes(R, R, R), dtype=torch.uint8, device=dev)
    tot = torch.empty(2, dtype=torch.int64, device=dev)
    one, zero = (ctypes.c_float * 3)(1, 1, 1), (ctypes.c_float * 3)(0, 0, 0)
    count = lambda: _lib.check(L.swnerf_mc_count(_lib.ptr(fp), R, R, R, ld, level, _lib.ptr(ws), _lib.ptr(tot), st), "mc_count")
    count()
    V, F = (int(x) for x in tot.cpu())
    verts, normals = torch.empty((V, 3), device=dev), torch.empty((V, 3), device=dev)
    faces = torch.empty((F, 3), dtype=torch.int32, device=dev)
    vcol = torch.empty((V, 3), device=dev) if cp is not None else None
    emit = lambda: _lib.check(L.swnerf_mc_emit(_lib.ptr(fp), _lib.ptr(cp), R, R, R, ld, 4 if cp is not None else 0, level, one, zero,
                                               _lib.ptr(ws), V, F, _lib.ptr(verts), _lib.ptr(faces), _lib.ptr(normals), _lib.ptr(vcol), st),
                              "mc_emit")
    best = []
    for fn in (count, emit):
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        best.append(min(ts))
    return best[0], best[1], V, F


print()
print("| marching cubes | ld | V | F | count ms | count GB/s (6 B/point) | emit ms | emit GB/s | total ms |")
print("|---|---|---|---|---|---|---|---|---|")
for kind in ("sphere", "noise"):
    for Rg in MC_ONLY or (128, 256, 512):
        f = mc_field(kind, Rg)
        for ld in (1, 4):
            tc, te, nV, nF = mc_passes(f, ld, 0.0)
            N = Rg ** 3
            gc = 6 * N / tc / 1e6
            ge = (8 * N + (48 if ld == 4 else 36) * nV + 12 * nF) / te / 1e6
            print(f"| {kind} {Rg}^3 | {ld} | {nV:,} | {nF:,} | {tc:.3f} | {gc:.0f} ({gc / COPY_TBS / 10:.0f} % of copy) | {te:.3f} | {ge:.0f} | {tc + te:.3f} |")
        del f
        torch.cuda.empty_cache()

with torch.no_grad():
    Rm = 0 if MC_ONLY else 128
    for _ in range(2 if Rm else 0):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        qq = mesh.sample_grid(bounds, Rm, net, num_views=V, on_device=True)
        torch.cuda.synchronize()
        t_q = time.perf_counter() - t0
        t0 = time.perf_counter()
        mc = mesh.marching_cubes(qq[..., 3], 0.5, colors=qq[..., :3])
        torch.cuda.synchronize()
        t_mc = time.perf_counter() - t0
        t0 = time.perf_counter()
        mm = mesh.nerf_to_mesh(net, bounds, resolution=Rm, density_threshold=0.5, num_views=V)
        torch.cuda.synchronize()
        t_m = time.perf_counter() - t0
if Rm:
    print(f"| nerf_to_mesh {Rm}^3 x {V} views (query + marching cubes + host copy of the mesh) | {t_m*1e3:.1f} ms | query alone {t_q*1e3:.1f} ms | "
          f"+{(t_m / t_q - 1) * 100:.1f} % | {len(mm.faces):,} faces |")
    print(f"| marching_cubes alone on that [R,R,R,4] query output (ld = 4, colours, incl. the count read-back) | {t_mc*1e3:.2f} ms | "
          f"{t_mc / t_q * 100:.2f} % of the query |")
