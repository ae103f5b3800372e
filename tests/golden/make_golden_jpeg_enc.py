"""Writes g20_jpeg_enc.npz: input pixels and the files PIL (libjpeg) makes of them - what swnerf.images.encode_jpegs must
reproduce byte for byte.  Runs on the CPU and needs PIL; the tests only read the .npz.
  sizes (H x W)  1x1; 8x8 (a dummy luma row and column at 4:2:0); 24x8 (a dummy column); 17x23; 40x72 (a dummy luma row);
                 50x35 (the last chroma row averages two different rows, an odd width, partial blocks)
  each at        4:4:4, 4:2:2, 4:2:0 and grey (the green channel), qualities 8, 50, 90, 100, content random / ramp / flat
  stack          three 17x23 frames of different content, 4:2:0 at quality 90
  float          float32 frames around the to8b boundaries (k / 255 and both neighbours, < 0, > 1, NaN) and a disparity-like
                 stack with its np.max as divisor; expected = PIL's file of numpy's to8b with the NaN positions set to 0
  qt             the DQT tables of PIL's files at every quality 1..100, natural order
All files are stored in ONE byte array with offsets (the headers repeat, so it compresses well)."""
import io
import os

import numpy as np
import PIL
from PIL import Image, features

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = [(1, 1), (8, 8), (24, 8), (17, 23), (40, 72), (50, 35)]
SAMPLINGS = ["444", "422", "420", "gray"]
QUALITIES = [8, 50, 90, 100]
CONTENTS = ["random", "ramp", "flat"]
ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


def pil_jpeg(img, quality, sampling):
    buf = io.BytesIO()
    if sampling == "gray":
        Image.fromarray(img, "L").save(buf, format="JPEG", quality=quality)
    else:
        Image.fromarray(img, "RGB").save(buf, format="JPEG", quality=quality, subsampling={"444": 0, "422": 1, "420": 2}[sampling])
    return buf.getvalue()


def content(kind, H, W, rng):
    if kind == "random":
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if kind == "ramp":
        y, x = np.mgrid[0:H, 0:W]
        return np.stack([(3 * x + 2 * y) % 256, (255 - 4 * y - x) % 256, (5 * x * y // max(1, W)) % 256], -1).astype(np.uint8)
    return (np.array([200, 37, 90]) + rng.integers(0, 2, (H, W, 3))).astype(np.uint8)          # near-constant


def to8b(x):
    with np.errstate(invalid="ignore"):
        v = 255 * np.clip(x, 0, 1)
        return np.where(np.isnan(v), 0, v).astype(np.uint8)


def dqt_tables(data):
    """[2][64] natural order from the two DQT segments of a PIL RGB file"""
    out, p = np.zeros((2, 64), np.uint8), 2
    while data[p + 1] != 0xDA:
        n = (data[p + 2] << 8) | data[p + 3]
        if data[p + 1] == 0xDB:
            seg = data[p + 4:p + 2 + n]
            for q in range(0, len(seg), 65):
                out[seg[q] & 15, ZIGZAG] = np.frombuffer(seg[q + 1:q + 65], np.uint8)
        p += 2 + n
    return out


def main():
    rng = np.random.default_rng(20261019)
    out, blob, index = {}, bytearray(), []

    def add(name, data):
        index.append((name, len(blob), len(data)))
        blob.extend(data)

    for (H, W) in SIZES:
        for kind in CONTENTS:
            img = content(kind, H, W, rng)
            out[f"px_{H}x{W}_{kind}"] = img
            for s in SAMPLINGS:
                for q in QUALITIES:
                    add(f"{H}x{W}_{kind}_{s}_q{q}", pil_jpeg(img[..., 1].copy() if s == "gray" else img, q, s))
    stack = np.stack([content(k, 17, 23, rng) for k in CONTENTS])
    out["stack_px"] = stack
    for k in range(3):
        add(f"stack_{k}", pil_jpeg(stack[k], 90, "420"))
    # float32 around the to8b boundaries: 16 x 24 x 3 values
    ks = np.array([0, 1, 2, 63, 64, 127, 128, 129, 200, 254, 255], np.float32) / np.float32(255)
    vals = np.concatenate([ks, np.nextafter(ks, np.float32(-1)), np.nextafter(ks, np.float32(2)),
                           np.array([-0.5, -1e-8, -0.0, 1.0000001, 1.5, 1e30, -1e30, np.inf, -np.inf, np.nan, np.nan], np.float32)]).astype(np.float32)
    f = rng.random((2, 16, 24, 3), dtype=np.float32) * np.float32(1.2) - np.float32(0.1)
    f.reshape(-1)[rng.permutation(f.size)[:4 * vals.size]] = np.tile(vals, 4)
    out["float_px"] = f
    for k in range(2):
        add(f"float_{k}", pil_jpeg(to8b(f[k]), 90, "420"))
    disp = (rng.random((2, 16, 24), dtype=np.float32) * np.float32(7.3)).astype(np.float32)
    disp[0, 3, 5] = np.nan
    disp[1, 0, 0] = np.float32(9.125)                                                            # the maximum
    out["disp_px"] = disp
    out["disp_max"] = np.float32(np.nanmax(disp))
    for k in range(2):
        add(f"disp_{k}", pil_jpeg(np.repeat(to8b(disp[k] / out["disp_max"])[..., None], 3, -1), 90, "420"))
    flat = np.full((8, 8, 3), 128, np.uint8)
    out["qt"] = np.stack([dqt_tables(pil_jpeg(flat, q, "444")) for q in range(1, 101)])
    out["names"] = np.array([n for n, _, _ in index])
    out["offsets"] = np.array([[o, n] for _, o, n in index], np.int64)
    out["files"] = np.frombuffer(bytes(blob), np.uint8)
    out["pil_version"] = np.array(PIL.__version__)
    out["libjpeg_version"] = np.array("jpeg " + str(features.version("jpg")) + (" (turbo)" if features.check_feature("libjpeg_turbo") else ""))
    path = os.path.join(HERE, "g20_jpeg_enc.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(index), "files")


if __name__ == "__main__":
    main()
