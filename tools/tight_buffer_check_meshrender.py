#!/usr/bin/env python3
"""Out-of-bounds guard for the mesh-rendering entry points (swnerf_mesh_render_raster, _render_resolve, swnerf_mesh_view_compare), in
the manner of tools/tight_buffer_check_meshfill.py: every operand, every output and the z-buffer end exactly where a torch allocation
of at least 10 MB whose size is a multiple of 2 MB ends (the caching allocator then maps exactly that much), so a read or write past
the last element - a pixel one past the image, a face or a vertex one past the mesh - leaves the mapping and faults instead of
touching a neighbour.  The shapes are one triangle over the whole of a 5 x 3 image (the wave tier, an image smaller than a wave), the
360 / 716 sphere of tests/meshops_ref.py from three views at 48 x 40 (both tiers) and the same sphere with its last face and
last vertex in use by a face that straddles the camera plane (whole-image box).  Every result is compared with the same call on
ordinary allocations, bit for bit, and with tests/meshrender_ref.py.
  tight_buffer_check_meshrender.py <case> [<case> ...]
  tight_buffer_check_meshrender.py list
tests/test_00_a_meshrender_tight_buffers.py starts it as a child process."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sw-nerf_amd"), ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
SHAPES = ["tri_5x3", "sphere_3views", "straddle_last"]
CALLS = ["raster", "resolve", "compare"]
CASES = [f"{c}-{s}" for c in CALLS for s in SHAPES]
if len(sys.argv) < 2 or sys.argv[1] == "list":
    print(" ".join(CASES))
    sys.exit(0)
for c in sys.argv[1:]:
    if c not in CASES:
        raise SystemExit(f"unknown case {c!r}; `list` prints them")

import numpy as np
import torch
import meshrender_ref as M
from swnerf import _lib

dev = torch.device("cuda:0")
MB2 = 2 << 20
FOCAL = 60.0


def tail(host):
    """a device copy of `host` that ends exactly at the end of a tight allocation"""
    nbytes = host.numel() * host.element_size()
    buf = torch.empty(max(10 << 20, (nbytes + MB2 - 1) // MB2 * MB2), dtype=torch.uint8, device=dev)
    t = buf[buf.numel() - nbytes:].view(host.dtype).view(host.shape)
    t.copy_(host)
    return t


def both(call, ins, outs, what, first=0):
    """call(*ins, *outs) on tight and on ordinary allocations -> the tight outputs, equal bit for bit to the ordinary ones from
    outs[first] on"""
    tight_in, tight_out = [tail(t) for t in ins], [tail(t) for t in outs]
    _lib.check(call(*tight_in, *tight_out), what)
    torch.cuda.synchronize()
    loose_in, loose_out = [t.to(dev) for t in ins], [t.to(dev) for t in outs]
    _lib.check(call(*loose_in, *loose_out), what)
    torch.cuda.synchronize()
    for a, b in zip(tight_out[first:], loose_out[first:]):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), what
    res = [t.cpu() for t in tight_out]
    del tight_in, tight_out, loose_in, loose_out
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return res


def scene_of(shape):
    """-> verts, faces, poses, H, W"""
    cases = M.cases()
    if shape == "tri_5x3":
        v, f, p = cases["whole_image"]
        return v, f, p[:1], 3, 5
    v, f, p = cases["sphere"]
    if shape == "sphere_3views":
        return v, f, p, 40, 48
    cam = M.special_meshes()["straddles"][2]
    v = np.concatenate([v * np.float32(0.3), [[0.1, 0.3, 3.5]]]).astype(np.float32)      # the last vertex is behind the camera at z = 2
    f = np.concatenate([f, [[0, 1, len(v) - 1]]]).astype(np.int32)
    return v, f, cam, 40, 48


def run(case):
    L = _lib.lib()
    name, shape = case.split("-")
    v, f, poses, H, W = scene_of(shape)
    V, F, N = len(v), len(f), len(poses)
    intr = M.intrinsics(H, W, focal=FOCAL)
    col = M.vertex_colors(v)
    want = M.render(v, f, H, W, intr, poses, colors=col, background=(0.5, 0.25, 0.125))
    tv, tf, tc, tp = torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(col), torch.from_numpy(np.ascontiguousarray(poses))
    assert L.swnerf_mesh_render_workspace_bytes(N, H, W) >= 8 * N * H * W
    ws = torch.zeros(8 * N * H * W, dtype=torch.uint8)             # the words in use, not the rounded size: the one after the last pixel is unmapped
    f32 = lambda *s: torch.full(s, -1., dtype=torch.float32)
    cam = (N, H, W, FOCAL, FOCAL, 0., 0., 1)
    raster = lambda ve, fa, po, wk, cnt: L.swnerf_mesh_render_raster(_lib.ptr(ve), _lib.ptr(fa), V, F, _lib.ptr(po), *cam, 0., float("inf"), 0,
                                                                      _lib.ptr(wk), _lib.ptr(cnt), _lib.stream_of(ve))
    if name == "raster":
        wk, cnt = both(raster, [tv, tf, tp], [ws, torch.zeros(4, dtype=torch.int64)], case)
        assert cnt.tolist() == want["counts"].tolist(), (case, cnt.tolist(), want["counts"].tolist())
        keys = wk.numpy()[:8 * N * H * W].view(np.uint64)
        face = np.where(keys == M.EMPTY, -1, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)).reshape(N, H * W)
        assert np.array_equal(face, want["face"]), case
        assert (keys >> np.uint64(32))[face.reshape(-1) >= 0].astype(np.uint32).tobytes() == want["depth"][want["acc"] > 0].tobytes(), case
    elif name == "resolve":
        bg = (ctypes.c_float * 3)(0.5, 0.25, 0.125)

        def call(ve, fa, co, po, wk, rgb, depth, disp, acc, face, bary):
            cnt = torch.zeros(4, dtype=torch.int64, device=dev)
            rc = raster(ve, fa, po, wk, cnt)
            return rc or L.swnerf_mesh_render_resolve(_lib.ptr(ve), _lib.ptr(fa), None, _lib.ptr(co), V, F, _lib.ptr(po), *cam, 0, bg, _lib.ptr(wk),
                                                      _lib.ptr(rgb), _lib.ptr(depth), _lib.ptr(disp), _lib.ptr(acc), _lib.ptr(face), _lib.ptr(bary),
                                                      _lib.stream_of(ve))
        outs = [ws, f32(N, H * W, 3), f32(N, H * W), f32(N, H * W), f32(N, H * W), torch.full((N, H * W), -7, dtype=torch.int32), f32(N, H * W, 3)]
        _, rgb, depth, disp, acc, face, bary = both(call, [tv, tf, tc, tp], outs, case, first=1)
        assert np.array_equal(face.numpy(), want["face"]), case
        for got, key in ((rgb, "rgb"), (depth, "depth"), (disp, "disp"), (acc, "acc"), (bary, "bary")):
            assert got.numpy().tobytes() == want[key].tobytes(), (case, key)
    else:
        rng = np.random.default_rng(5)
        acc, depth = want["acc"].reshape(N, H, W), want["depth"].reshape(N, H, W)
        frames = rng.integers(0, 256, (N, H, W, 4), dtype=np.uint8)
        ref_depth = (depth + rng.standard_normal(depth.shape).astype(np.float32) * np.float32(0.01)).astype(np.float32)
        wc, wsum = M.compare(acc, depth, frames[..., 3], ref_depth)
        call = lambda a, d, al, rd, cnt, sm: L.swnerf_mesh_view_compare(_lib.ptr(a), _lib.ptr(d), _lib.ptr(al), 1, 4, 3, _lib.ptr(rd), N, H, W, _lib.ptr(cnt),
                                                                         _lib.ptr(sm), _lib.stream_of(a))
        cnt, sm = both(call, [torch.from_numpy(acc.copy()), torch.from_numpy(depth.copy()), torch.from_numpy(frames), torch.from_numpy(ref_depth)],
                       [torch.zeros((N, 4), dtype=torch.int64), torch.zeros((N, 3), dtype=torch.float64)], case)
        assert np.array_equal(cnt.numpy(), wc) and sm.numpy().tobytes() == wsum.tobytes(), case


for c in sys.argv[1:]:
    run(c)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    print(f"{c}: ok", flush=True)
