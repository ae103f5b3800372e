#!/usr/bin/env python3
"""Loading a dataset's frames: the host path (png.read_png of every file, then numpy: / 255 and, for half_res, the 2 x 2 mean)
beside images.load_pngs (host inflate, device unfilter and area mean) in the same run, on a synthetic set shaped like lego's
test split at testskip=8 plus train and val: 138 frames of 800 x 800 RGBA whose rows are all Paeth, the common case for Blender
renders.  The host path is timed on --host-frames frames (default 2: it unfilters byte by byte in Python, about 4 s a frame) and
scaled to the whole set; the device path loads all of them, twice, and the second pass is reported (the first pays the pinned
staging and the page cache).
JPEG rows (when PIL imports, which writes the files; skipped otherwise), after the same warm-up in the same process: 20 frames
of 1008 x 756 at 4:2:0 and 4 frames of 4032 x 3024 loaded with factor 8, each as the host route (PIL decode, the copy to the
device and, for factor 8, area_resize) beside images.load_pngs, and the new route split into host Huffman decoding (one thread),
the host-to-device copy of coefficients and tables, and the two kernels (device events, second pass).  --skip-png leaves the PNG
rows out.  Prints ONE JSON line.
  python tools/bench_data.py [--frames 138] [--size 800] [--host-frames 2] [--skip-png] [--json out.json]"""
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
from swnerf import _lib, images, png

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=138)
ap.add_argument("--size", type=int, default=800)
ap.add_argument("--host-frames", type=int, default=2)
ap.add_argument("--skip-png", action="store_true")
ap.add_argument("--json", default=None)
opt = ap.parse_args()
assert torch.cuda.is_available(), "bench_data.py needs the MI355X"
DEV = torch.device("cuda:0")
N, S = opt.frames, opt.size


def png_rows():
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

    res = {"frames": N, "size": S, "files_mib": round(file_mb, 1), "host_frames_timed": nh,
           "host_read_png_s": round(host_read_s, 2), "host_to_float_s": round(host_float_s, 3), "host_half_res_s": round(host_half_s, 3),
           "host_inflate_only_s": round(inflate_s, 3), "load_pngs_first_s": round(first_s, 3), "load_pngs_s": round(full_s, 3),
           "load_pngs_half_res_s": round(half_s, 3), "unfilter_kernel_ms": round(ev[0].elapsed_time(ev[1]), 3),
           "area_resize_kernel_ms": round(ev[1].elapsed_time(ev[2]), 3),
           "speedup_full": round((host_read_s + host_float_s) / full_s, 1), "speedup_half_res": round((host_read_s + host_float_s + host_half_s) / half_s, 1)}
    return res


def jpeg_rows():
    """-> {name: value}; {} without PIL"""
    try:
        from PIL import Image
    except ImportError:
        return {"jpeg": "skipped: PIL does not import, nothing can write the files"}
    out = {}
    with tempfile.TemporaryDirectory(prefix="swnerf_bench_jpeg_") as tmp:
        for tag, n, (H, W), factor in (("jpeg_1008x756", 20, (756, 1008), 1), ("jpeg_4032x3024_f8", 4, (3024, 4032), 8)):
            # a photograph-like picture: smooth shading, edges and sensor-like noise; 4 distinct frames, cycled
            y, x = np.mgrid[0:H, 0:W]
            rng = np.random.default_rng(1)
            paths = []
            for k in range(n):
                path = os.path.join(tmp, f"{tag}_{k:03d}.jpg")
                if k < 4:
                    img = np.stack([128 + 90 * np.sin((x + 57 * k) / (60. + 25 * c)) * np.cos(y / 83.) + 40 * ((x // 97 + y // 71) % 2)
                                    + rng.normal(0, 6, (H, W)) for c in range(3)], -1)
                    Image.fromarray(np.clip(img, 0, 255).astype(np.uint8), "RGB").save(path, "JPEG", quality=90, subsampling=2)
                else:
                    with open(paths[k % 4], "rb") as src, open(path, "wb") as dst:
                        dst.write(src.read())
                paths.append(path)
            hw = None if factor == 1 else (H // factor, W // factor)

            def host_route():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                px = torch.from_numpy(np.stack([np.asarray(Image.open(p).convert("RGB")) for p in paths])).to(DEV)
                res = px if hw is None else images.area_resize(px, *hw)
                torch.cuda.synchronize()
                return time.perf_counter() - t0, res

            def device_route():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = images.load_pngs(paths, DEV, out_hw=hw)
                torch.cuda.synchronize()
                return time.perf_counter() - t0, res

            host_route(), device_route()                                     # warm-up: page cache, pinned staging, code objects
            host_s, device_s = [], []
            for _ in range(3):                                               # alternating, so that drift hits both alike
                t, a = host_route()
                host_s.append(t)
                t, b = device_route()
                device_s.append(t)
            assert torch.equal(a, b), tag
            # the stages of the new route, one after the other
            heads = [images._jpeg_header(open(p, "rb").read(), p) for p in paths]
            t0 = time.perf_counter()
            coefs = [j.coefficients() for j in heads]
            entropy_s = time.perf_counter() - t0
            j = heads[0]
            coef_h = torch.from_numpy(np.concatenate(coefs)).pin_memory()
            qt_h = torch.from_numpy(np.concatenate([h.qt for h in heads]).view(np.int16)).pin_memory()
            L, ptr = _lib.lib(), _lib.ptr
            planes = torch.empty((n * j.ncoef,), dtype=torch.uint8, device=DEV)
            px = torch.empty((n, H, W, 3), dtype=torch.uint8, device=DEV)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            for rep in range(2):
                ev[0].record()
                coef, qt = coef_h.to(DEV, non_blocking=True), qt_h.to(DEV, non_blocking=True)
                ev[1].record()
                _lib.check(L.swnerf_jpeg_decode(ptr(coef), ptr(qt), n, H, W, j.ncomp, j.sampling, 3, ptr(planes), ptr(px), _lib.stream_of(px)), tag)
                ev[2].record()
                torch.cuda.synchronize()
            # the two launches of one call cannot be told apart by events: their split is read from a kernel trace of this tool
            # (rocprofv3 --kernel-trace --stats -- python tools/bench_data.py --skip-png), a run of its own
            out.update({f"{tag}_frames": n, f"{tag}_files_mib": round(sum(os.path.getsize(p) for p in paths) / 2 ** 20, 2),
                        f"{tag}_pil_route_s": round(min(host_s), 4), f"{tag}_load_pngs_s": round(min(device_s), 4),
                        f"{tag}_pil_route_all_s": [round(t, 4) for t in host_s], f"{tag}_load_pngs_all_s": [round(t, 4) for t in device_s],
                        f"{tag}_host_entropy_1thread_ms": round(entropy_s * 1e3, 2), f"{tag}_h2d_ms": round(ev[0].elapsed_time(ev[1]), 3),
                        f"{tag}_kernels_ms": round(ev[1].elapsed_time(ev[2]), 3),
                        f"{tag}_coef_mib": round(coef_h.numel() * 2 / 2 ** 20, 1), f"{tag}_speedup": round(min(host_s) / min(device_s), 2)})
    return out


res = {"bench": "data"}
if not opt.skip_png:
    res.update(png_rows())
res.update(jpeg_rows())
line = json.dumps(res)
print(line)
if opt.json:
    with open(opt.json, "w") as fp:
        fp.write(line + "\n")
