#!/usr/bin/env python3
"""Marker detection (swnerf.markers, csrc/marker_kernels.hip) on n frames of H x W x 3 uint8 that are already on the device, as
cal_scale runs it on images_ori/: per-stage and total times from device events.  The frames hold a few markers (rendered small by
tests/marker_ref.py and enlarged on the device) under Gaussian noise, so the thresholded image has the speckle of a photo.
Stages, for one radius each: grey + threshold (swnerf_marker_mask), labels (swnerf_marker_label), components
(swnerf_marker_candidates); then the whole swnerf_marker_detect over both radii, which adds refinement, decoding and the merge.
Beside each time: ns per pixel, and the bytes per pixel a plain device copy (measured here, read + write) moves in that time,
against the bytes the stage has to move at the least.  Second passes are reported.  Prints ONE JSON line.
  python tools/bench_markers.py [--frames 4] [--height 3000] [--width 4000] [--noise 3] [--json out.json]"""
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
import marker_ref
from swnerf import markers

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=4)
ap.add_argument("--height", type=int, default=3000)
ap.add_argument("--width", type=int, default=4000)
ap.add_argument("--noise", type=float, default=3.)
ap.add_argument("--json", default=None)
opt = ap.parse_args()
assert torch.cuda.is_available(), "bench_markers.py needs the MI355X"
DEV = torch.device("cuda:0")
N, H, W = opt.frames, opt.height, opt.width
RADII = (11, 41)
# the least each stage moves, bytes per pixel: mask = 3 in, grey out and in twice, uint16 row sums out and in, mask out; labels =
# mask in, labels out, in for the border pass, in and out for the flattening; components = the area table cleared and added to,
# labels and table read by the two scan passes and the four reduction passes
LEAST = {"mask": 3 + 1 + 2 + 2 + 2 + 1, "label": 1 + 4 + 4 + 8, "components": 4 + 8 + 2 * 8 + 4 * 8}


def make_frames():
    f = 8
    h, w = H // f, W // f
    rng = np.random.default_rng(0)
    small = []
    for k in range(N):
        quads = []
        for _ in range(3):
            side = rng.uniform(0.08, 0.2) * h
            ang = rng.uniform(0, 2 * np.pi)
            Rm = np.array([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]])
            c = [rng.uniform(0.25 * w, 0.75 * w), rng.uniform(0.25 * h, 0.75 * h)]
            quads.append((np.array([[-.5, -.5], [.5, -.5], [.5, .5], [-.5, .5]]) * side) @ Rm.T + c)
        small.append(marker_ref.render_marker(h, w, quads, [marker_ref.random_bits(rng) for _ in quads], ss=2))
    g = torch.from_numpy(np.stack(small)).to(DEV).float()
    g = torch.nn.functional.interpolate(g[:, None], size=(H, W), mode="bilinear", align_corners=False)[:, 0]
    gen = torch.Generator(device=DEV).manual_seed(0)
    g = g + opt.noise * torch.randn(g.shape, device=DEV, generator=gen)
    return g.clamp(0, 255).round().to(torch.uint8)[..., None].repeat(1, 1, 1, 3).contiguous()


def event_ms(fn, reps=3):
    fn()                                                                     # first pass: allocator warm-up
    torch.cuda.synchronize()
    best, r = None, None
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = fn()
        b.record()
        b.synchronize()
        t = a.elapsed_time(b)
        best = t if best is None else min(best, t)
    return best, r


frames = make_frames()
px = N * H * W
ws = torch.empty((markers.workspace_bytes(N, H, W),), dtype=torch.uint8, device=DEV)
src = torch.empty((px * 4,), dtype=torch.uint8, device=DEV)
dst = torch.empty_like(src)
copy_ms, _ = event_ms(lambda: dst.copy_(src))
copy_gbs = 2 * src.numel() / copy_ms / 1e6                                   # read + write
res = {"frames": N, "height": H, "width": W, "noise": opt.noise, "workspace_bytes_per_pixel": ws.numel() / px,
       "copy_GBps": round(copy_gbs, 1), "stages": {}}


def report(name, ms, least=None):
    e = {"ms": round(ms, 3), "ms_per_frame": round(ms / N, 3), "ns_per_pixel": round(ms * 1e6 / px, 4),
         "copy_equivalent_bytes_per_pixel": round(ms * 1e-3 * copy_gbs * 1e9 / px, 1)}
    if least is not None:
        e["least_bytes_per_pixel"] = least
    res["stages"][name] = e


for r in RADII:
    ms, (grey, mask) = event_ms(lambda: markers.dark_mask(frames, r))
    report(f"mask_r{r}", ms, LEAST["mask"])
    ms, labels = event_ms(lambda: markers.label(mask))
    report(f"label_r{r}", ms, LEAST["label"])
    ms, (rows, count) = event_ms(lambda: markers.candidates(labels, 100, capacity=4096))
    report(f"components_r{r}", ms, LEAST["components"])
    res["stages"][f"components_r{r}"]["components_per_frame"] = count.cpu().tolist()
    res["stages"][f"mask_r{r}"]["dark_fraction"] = round(float(mask.float().mean()), 4)
ms, (quads, payload, count) = event_ms(lambda: markers.detect_raw(frames, RADII, workspace=ws))
report("detect_total", ms)
res["markers_per_frame"] = count.cpu().tolist()
line = json.dumps(res)
print(line)
if opt.json:
    with open(opt.json, "w") as fh:
        fh.write(line + "\n")
