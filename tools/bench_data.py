#!/usr/bin/env python3
"""Loading a dataset's frames: the host path (png.read_png of every file, then numpy: / 255 and, for half_res, the 2 x 2 mean)
beside images.load_pngs (host inflate, device unfilter and area mean) in the same run, on a synthetic set shaped like lego's
test split at testskip=8 plus train and val: 138 frames of 800 x 800 RGBA whose rows are all Paeth, the common case for Blender
renders.  The host path is timed on --host-frames frames (default 2: it unfilters byte by byte in Python, about 4 s a frame) and
scaled to the whole set; the device path loads all of them, twice, and the second pass is reported (the first pays the pinned
staging and the page cache).  Prints ONE JSON line.
  python tools/bench_data.py [--frames 138] [--size 800] [--host-frames 2] [--json out.json]"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sw-nerf_amd"), ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import __graft_entry__ as ge

ge.compile_library_locked()                     # before the GPU is initialised
import numpy as np
import torch
import png_ref
from swnerf import images, png

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=138)
ap.add_argument("--size", type=int, default=800)
ap.add_argument("--host-frames", type=int, default=2)
ap.add_argument("--json", default=None)
opt = ap.parse_args()
assert torch.cuda.is_available(), "bench_data.py needs the MI355X"
DEV = torch.device("cuda:0")
N, S = opt.frames, opt.size

with tempfile.TemporaryDirectory(prefix="swnerf_bench_data_") as tmp:
    # a render-like picture: smooth shading plus a little noise inside a disc, transparent outside; 8 distinct frames, cycled
    y, x = np.mgrid[0:S, 0:S]
    r = np.hypot(y / S - .5, x / S - .5)
    rng = np.random.default_rng(0)
    paths = []
    for k in range(N):
        path = os.path.join(tmp, f"r_{k:03d}.png")
        if k < 8:
            img = np.zeros((S, S, 4), np.uint8)
            for c in range(3):
                img[..., c] = np.clip(128 + 100 * np.sin((x + 31 * k) / (40. + 10 * c)) * np.cos(y / 55.) + rng.integers(-3, 4, (S, S)), 0, 255)
            img[..., 3] = np.where(r < .45, 255, 0)
            img[..., :3] *= (img[..., 3:] > 0)
            png_ref.write_png(path, img, 4)
        else:
            with open(paths[k % 8], "rb") as src, open(path, "wb") as dst:
                dst.write(src.read())
        paths.append(path)
    file_mb = sum(os.path.getsize(p) for p in paths) / 2 ** 20

    t0 = time.perf_counter()
    inflated = [png.read_png_filtered(p) for p in paths]
    inflate_s = time.perf_counter() - t0
    del inflated

    nh = max(1, min(opt.host_frames, N))
    t0 = time.perf_counter()
    host = [png.read_png(p) for p in paths[:nh]]
    host_read_s = (time.perf_counter() - t0) * N / nh
    t0 = time.perf_counter()
    f = (np.array(host) / 255.).astype(np.float32)
    host_float_s = (time.perf_counter() - t0) * N / nh
    t0 = time.perf_counter()
    f.reshape(nh, S // 2, 2, S // 2, 2, 3).mean((2, 4))
    host_half_s = (time.perf_counter() - t0) * N / nh

    def load(**kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = images.load_pngs(paths, DEV, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    first_s, out = load()
    np.testing.assert_array_equal(out[0].cpu().numpy()[..., :3], host[0])
    del out
    full_s, out = load()
    del out
    half_s, out = load(out_hw=(S // 2, S // 2))
    del out

    # the device work alone: unfilter and 2x area mean of the whole set, already on the device
    filt = torch.from_numpy(np.stack([np.frombuffer(png.read_png_filtered(p)[0], np.uint8) for p in paths[:8]])).to(DEV)
    filt = filt.repeat((N + 7) // 8, 1)[:N].contiguous()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    px = images.unfilter(filt, S, S, 4)
    images.area_resize(px, S // 2, S // 2)
    torch.cuda.synchronize()
    ev[0].record()
    px = images.unfilter(filt, S, S, 4)
    ev[1].record()
    images.area_resize(px, S // 2, S // 2)
    ev[2].record()
    torch.cuda.synchronize()

res = {"bench": "data", "frames": N, "size": S, "files_mib": round(file_mb, 1), "host_frames_timed": nh,
       "host_read_png_s": round(host_read_s, 2), "host_to_float_s": round(host_float_s, 3), "host_half_res_s": round(host_half_s, 3),
       "host_inflate_only_s": round(inflate_s, 3), "load_pngs_first_s": round(first_s, 3), "load_pngs_s": round(full_s, 3),
       "load_pngs_half_res_s": round(half_s, 3), "unfilter_kernel_ms": round(ev[0].elapsed_time(ev[1]), 3),
       "area_resize_kernel_ms": round(ev[1].elapsed_time(ev[2]), 3),
       "speedup_full": round((host_read_s + host_float_s) / full_s, 1), "speedup_half_res": round((host_read_s + host_float_s + host_half_s) / half_s, 1)}
line = json.dumps(res)
print(line)
if opt.json:
    with open(opt.json, "w") as fp:
        fp.write(line + "\n")
