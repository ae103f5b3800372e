#!/usr/bin/env python3
"""Capture g19_jpeg.npz: small JPEG files and the pixels libjpeg decodes from them.  PIL (Pillow, on libjpeg-turbo) is the decoder
the reference's imageio.imread ends in, so `np.asarray(Image.open(f).convert("RGB"))` is what its loaders see.  Seeded numpy
images are encoded by PIL; the file bytes are stored as uint8 arrays (`<case>_jpg`) beside the expected pixels (`<case>_rgb`),
with PIL's and libjpeg's version strings.  The cases are the smallest at which each rule of the decode can go wrong:
  1x1 4:2:0                              the smallest image
  2x3, 5x4 at 4:2:2 and 4:2:0            a chroma plane of at most 2 columns: plain replication
  6x5 4:2:0                              3 chroma columns, the first width the triangle filter runs at
  17x23, 16x16, 33x9 at 4:4:4/4:2:2/4:2:0  odd sizes, partial MCUs, exactly one MCU
  9x35 grayscale                         a single component
  40x56 4:2:0, restart interval 2        restart markers
  24x16 4:2:0 at quality 30, 75, 100     one geometry, three sets of tables
  17x23 progressive                      not decodable natively
Strong noise at quality 100 makes the clamps of the inverse DCT and of the colour conversion fire."""
import io
import os
import sys

import numpy as np
import PIL
from PIL import Image, features

HERE = os.path.dirname(os.path.abspath(__file__))
SUB = {"444": 0, "422": 1, "420": 2}
# (H, W, sampling, quality, extra save options, suffix)
CASES = [(1, 1, "420", 100, {}, "")]
CASES += [(H, W, s, 100, {}, "") for (H, W) in ((2, 3), (5, 4)) for s in ("422", "420")]
CASES += [(6, 5, "420", 100, {}, "")]
CASES += [(H, W, s, 100, {}, "") for (H, W) in ((17, 23), (16, 16), (33, 9)) for s in ("444", "422", "420")]
CASES += [(9, 35, "gray", 100, {}, "")]
CASES += [(40, 56, "420", 100, {"restart_marker_blocks": 2}, "_rst2")]
CASES += [(24, 16, "420", q, {}, f"_q{q}") for q in (30, 75, 100)]
CASES += [(17, 23, "420", 90, {"progressive": True}, "_prog")]


def name(H, W, s, suffix):
    return f"{H}x{W}_{s}{suffix}"


def picture(H, W, gray, quality, seed):
    rng = np.random.default_rng(seed)
    shape = (H, W) if gray else (H, W, 3)
    if quality == 100:
        noise = rng.integers(0, 256, shape, dtype=np.uint8)                     # strong noise, half of it black or white: the clamps fire
        return np.where(rng.random(shape) < .5, noise, 255 * rng.integers(0, 2, shape, dtype=np.uint8)).astype(np.uint8)
    y, x = np.mgrid[0:H, 0:W]
    base = 128 + 90 * np.sin(x / 3.) * np.cos(y / 4.)
    img = base[..., None] * np.array([1., .8, 1.1]) if not gray else base
    return np.clip(img + rng.integers(-40, 41, shape), 0, 255).astype(np.uint8)


def main():
    out = {"pil_version": np.array(PIL.__version__),
           "libjpeg_version": np.array(f"{'libjpeg-turbo' if features.check_feature('libjpeg_turbo') else 'libjpeg'} "
                                       f"{features.version('jpg')}")}
    names = []
    for k, (H, W, s, q, extra, suffix) in enumerate(CASES):
        gray = s == "gray"
        img = picture(H, W, gray, q, 1900 + k)
        buf = io.BytesIO()
        opts = dict(quality=q, **extra)
        if not gray:
            opts["subsampling"] = SUB[s]
        Image.fromarray(img, "L" if gray else "RGB").save(buf, "JPEG", **opts)
        data = buf.getvalue()
        rgb = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        assert rgb.shape == (H, W, 3)
        n = name(H, W, s, suffix)
        names.append(n)
        out[n + "_jpg"] = np.frombuffer(data, np.uint8)
        out[n + "_rgb"] = rgb
        dri = b"\xff\xdd" in data
        print(f"{n}: {len(data)} bytes, clamped pixels {int((rgb == 0).sum() + (rgb == 255).sum())}, DRI {dri}")
    out["names"] = np.array(names)
    path = os.path.join(HERE, "g19_jpeg.npz")
    np.savez_compressed(path, **out)
    print("g19_jpeg.npz", os.path.getsize(path) // 1024, "KiB", out["pil_version"], out["libjpeg_version"])


if __name__ == "__main__":
    sys.dont_write_bytecode = True
    main()
