#!/usr/bin/env python3
"""Writing a render video: video.write_video of 120 frames of 800 x 800 x 3 float32 (a smooth synthetic render with some
texture, host numpy as render_path returns it) split into its stages - upload, the two kernels of swnerf_jpeg_encode (device
events), the device-to-host copy of the coefficients, the host Huffman coding (one thread, and the pool of 4 as encode_jpegs runs
it) and the file write - beside the PNG path of render_path (to8b + png.write_png per frame) and, when PIL imports, PIL's JPEG
encode of the same frames at the same quality.  Second passes are reported (the first pays pinned staging and allocator warm-up).
Prints ONE JSON line.
  python tools/bench_video.py [--frames 120] [--size 800] [--quality 90] [--png-frames 8] [--json out.json]"""
import argparse
import io
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sw-nerf_amd"), ROOT):
    sys.path.insert(0, p)
import __graft_entry__ as ge

ge.compile_library_locked()                     # before the GPU is initialised
import numpy as np
import torch
from swnerf import _lib, images, png, video
from swnerf.checkpoint import to8b

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=120)
ap.add_argument("--size", type=int, default=800)
ap.add_argument("--quality", type=int, default=90)
ap.add_argument("--png-frames", type=int, default=8)
ap.add_argument("--json", default=None)
opt = ap.parse_args()
assert torch.cuda.is_available(), "bench_video.py needs the MI355X"
DEV = torch.device("cuda:0")
N, S, Q = opt.frames, opt.size, opt.quality
L = _lib.lib()


def frames():
    rng = np.random.default_rng(0)
    y, x = np.mgrid[0:S, 0:S].astype(np.float32) / np.float32(S)
    out = np.empty((N, S, S, 3), np.float32)
    for k in range(N):
        a = np.float32(2 * np.pi * k / N)
        base = np.stack([0.5 + 0.5 * np.sin(6 * x + a), 0.5 + 0.5 * np.cos(5 * y - a), 0.5 + 0.5 * np.sin(4 * (x + y) + 2 * a)], -1)
        out[k] = base + rng.normal(0, 0.02, (S, S, 3)).astype(np.float32)
    return out


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), r


def main():
    x = frames()
    res = {"frames": N, "size": S, "quality": Q, "input_MiB": x.nbytes / 2 ** 20}
    with tempfile.TemporaryDirectory(prefix="swnerf_bench_video_") as tmp:
        path = os.path.join(tmp, "v.avi")
        for _ in range(2):
            t0 = time.perf_counter()
            video.write_video(path, x, fps=30, quality=Q)
            res["write_video_s"] = time.perf_counter() - t0
        res["avi_MiB"] = os.path.getsize(path) / 2 ** 20
        # the stages, one after another
        sampling = _lib.JPEG_420
        ncoef = int(L.swnerf_jpeg_coef_count(S, S, 3, sampling))
        bound = int(L.swnerf_jpeg_file_bound(S, S, 3, sampling))
        qt = np.empty((2, 64), np.uint16)
        L.swnerf_jpeg_quant_tables(Q, qt.ctypes.data)
        pinned = torch.from_numpy(x).pin_memory()
        for _ in range(2):
            res["upload_ms"], d = event_ms(lambda: pinned.to(DEV, non_blocking=True))
        qt_dev = torch.from_numpy(np.ascontiguousarray(qt[[0, 1, 1]]).view(np.int16)).to(DEV)
        coef = torch.empty((N, ncoef), dtype=torch.int16, device=DEV)
        planes = torch.empty((N, ncoef), dtype=torch.uint8, device=DEV)

        def encode():
            _lib.check(L.swnerf_jpeg_encode(_lib.ptr(d), 0, N, S, S, 3, 0.0, _lib.ptr(qt_dev), 3, sampling, _lib.ptr(planes), _lib.ptr(coef),
                                            _lib.stream_of(coef)), "jpeg_encode")
        for _ in range(3):
            res["both_kernels_ms"], _ = event_ms(encode)
        host = torch.empty((N, ncoef), dtype=torch.int16).pin_memory()
        for _ in range(2):
            res["d2h_ms"], _ = event_ms(lambda: host.copy_(coef, non_blocking=True))
        rows = host.numpy()
        t0 = time.perf_counter()
        jpegs = [images._jpeg_write_host(rows[k], qt, S, S, 3, sampling, bound) for k in range(N)]
        res["huffman_1_thread_ms"] = 1e3 * (time.perf_counter() - t0)
        t0 = time.perf_counter()
        with ThreadPoolExecutor(max_workers=images._JPEG_WORKERS) as pool:
            list(pool.map(lambda k: images._jpeg_write_host(rows[k], qt, S, S, 3, sampling, bound), range(N)))
        res["huffman_pool_ms"] = 1e3 * (time.perf_counter() - t0)
        t0 = time.perf_counter()
        video.write_avi(path, jpegs, S, S, 30)
        res["file_write_ms"] = 1e3 * (time.perf_counter() - t0)
        res["jpeg_MiB"] = sum(len(j) for j in jpegs) / 2 ** 20
        # the PNG path of render_path, on --png-frames frames, scaled
        k = min(opt.png_frames, N)
        t0 = time.perf_counter()
        for i in range(k):
            png.write_png(os.path.join(tmp, f"{i:03d}.png"), to8b(x[i]))
        res["png_path_s_scaled"] = (time.perf_counter() - t0) * N / k
        try:
            from PIL import Image
        except ImportError:
            Image = None
        if Image is not None:
            t0 = time.perf_counter()
            same = 0
            for i in range(N):
                buf = io.BytesIO()
                Image.fromarray(to8b(x[i]), "RGB").save(buf, format="JPEG", quality=Q, subsampling=2)
                same += buf.getvalue() == jpegs[i]
            res["pil_encode_s"] = time.perf_counter() - t0
            res["frames_equal_to_pil"] = same
    line = json.dumps(res)
    print(line)
    if opt.json:
        with open(opt.json, "w") as f:
            f.write(line + "\n")


main()
