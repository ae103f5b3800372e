"""Helper of the image tests: the FORWARD PNG filters (all five types, vectorised - a forward filter reads only unfiltered
bytes, so no byte waits for another) with per-row types drawn from a seed, and a writer that emits such a stream as a valid PNG
(zlib + struct, no PIL)."""
import struct
import zlib

import numpy as np


def image(H, W, c, seed):
    """uint8 [H,W,c]: smooth ramps plus noise, so that every filter type sees small and wrapping differences"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    base = (3 * y[..., None] + 5 * x[..., None] + 40 * np.arange(c)) % 256
    noise = rng.integers(0, 256, (H, W, c)) * (rng.random((H, W, c)) < 0.5)
    return ((base + noise) % 256).astype(np.uint8)


def row_types(H, seed):
    return np.random.default_rng(seed).integers(0, 5, H)


def filter_rows(img, types):
    """img uint8 [H,W,c], types [H] in 0..4 (a scalar: every row) -> uint8 [H, 1 + W*c]: the scanlines a PNG encoder would deflate"""
    H, W, c = img.shape
    types = np.broadcast_to(np.asarray(types), (H,)).astype(np.int64)
    raw = img.reshape(H, W * c).astype(np.int64)
    a = np.concatenate([np.zeros((H, c), np.int64), raw[:, :-c]], 1) if W > 1 else np.zeros_like(raw)
    b = np.concatenate([np.zeros((1, W * c), np.int64), raw[:-1]], 0)
    cc = np.concatenate([np.zeros((H, c), np.int64), b[:, :-c]], 1) if W > 1 else np.zeros_like(raw)
    p = a + b - cc
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - cc)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, cc))
    pred = np.stack([np.zeros_like(raw), a, b, (a + b) >> 1, paeth])[types, np.arange(H)]
    return np.concatenate([types[:, None], (raw - pred) % 256], 1).astype(np.uint8)


def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)


def write_png(filename, img, types, idat_chunks=1):
    """img uint8 [H,W,3|4] as an 8-bit non-interlaced PNG whose rows carry the filter `types`; the deflate stream is cut into
    idat_chunks IDAT chunks"""
    H, W, c = img.shape
    z = zlib.compress(filter_rows(img, types).tobytes(), 6)
    cuts = [len(z) * k // idat_chunks for k in range(idat_chunks + 1)]
    body = b"".join(_chunk(b"IDAT", z[cuts[k]:cuts[k + 1]]) for k in range(idat_chunks))
    with open(filename, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, {3: 2, 4: 6}[c], 0, 0, 0)) + body + _chunk(b"IEND", b""))
