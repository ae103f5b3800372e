"""Minimal PNG writer and reader (zlib + struct).  write_png is the output side of render_path: the reference calls
`imageio.imwrite(filename, to8b(rgb))` (nerf/run.py:210-213, d_nerf/run_dnerf.py:222-230); imageio is not a
dependency of this package.  8-bit grey, grey+alpha, RGB or RGBA, no interlacing, filter type 0.  read_png is the input
side of the D-NeRF metrics notebook (`imageio.imread` of estim/ and gt/ frames): 8-bit RGB or RGBA (alpha dropped), no
interlacing, all five filter types, any number of IDAT chunks; anything else is refused.  read_png_filtered stops after the
inflate: the dataset loaders (swnerf.images.load_pngs) undo the filters on the device."""
import struct
import zlib

import numpy as np


def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)


def write_png(filename, img):
    """img: uint8 array [H,W], [H,W,1|2|3|4]."""
    a = np.asarray(img)
    if a.dtype != np.uint8:
        raise TypeError(f"write_png expects uint8 (use to8b), got {a.dtype}")
    if a.ndim == 2:
        a = a[..., None]
    if a.ndim != 3 or a.shape[2] not in (1, 2, 3, 4) or a.shape[0] == 0 or a.shape[1] == 0:
        raise ValueError(f"write_png: unsupported image shape {a.shape}")
    h, w, c = a.shape
    color_type = {1: 0, 2: 4, 3: 2, 4: 6}[c]
    raw = np.concatenate([np.zeros((h, 1), np.uint8), np.ascontiguousarray(a).reshape(h, w * c)], axis=1).tobytes()
    png = (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, color_type, 0, 0, 0))
           + _chunk(b"IDAT", zlib.compress(raw, 6)) + _chunk(b"IEND", b""))
    with open(filename, "wb") as f:
        f.write(png)


def _unfilter(raw, h, w, bpp):
    """PNG filter types 0-4 (None, Sub, Up, Average, Paeth) of h scanlines of w * bpp bytes, each led by its type byte"""
    stride = w * bpp
    if len(raw) != h * (stride + 1):
        raise ValueError(f"read_png: image data holds {len(raw)} bytes, expected {h * (stride + 1)}")
    rows = np.frombuffer(raw, np.uint8).reshape(h, stride + 1)
    out = np.zeros((h, stride), np.uint8)
    prev = np.zeros(stride, np.int32)
    for y in range(h):
        ft, line = int(rows[y, 0]), rows[y, 1:].astype(np.int32)
        if ft == 0:
            cur = line
        elif ft == 2:
            cur = (line + prev) & 0xff
        elif ft in (1, 3, 4):
            cur = np.zeros(stride, np.int32)
            for x in range(stride):                      # depends on the byte bpp to the left: sequential
                a = int(cur[x - bpp]) if x >= bpp else 0
                b = int(prev[x])
                if ft == 1:
                    pred = a
                elif ft == 3:
                    pred = (a + b) >> 1
                else:
                    c = int(prev[x - bpp]) if x >= bpp else 0
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
                cur[x] = (int(line[x]) + pred) & 0xff
        else:
            raise ValueError(f"read_png: unknown filter type {ft} on row {y}")
        out[y] = cur
        prev = cur
    return out


def _read_scanlines(filename):
    """Signature, chunk and CRC checks, IHDR validation and the inflate -> (filtered scanlines, h, w, channels)"""
    with open(filename, "rb") as f:
        data = f.read()
    if data[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError(f"read_png: {filename} is not a PNG file")
    pos, ihdr, idat = 8, None, []
    while pos + 8 <= len(data):
        n, tag = struct.unpack(">I", data[pos:pos + 4])[0], data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + n]
        if len(body) != n or pos + 12 + n > len(data):
            raise ValueError(f"read_png: {filename}: truncated {tag!r} chunk")
        if struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] != zlib.crc32(tag + body) & 0xffffffff:
            raise ValueError(f"read_png: {filename}: CRC mismatch in {tag!r} chunk")
        if tag == b"IHDR":
            ihdr = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat.append(body)
        elif tag == b"IEND":
            break
        elif tag == b"PLTE" or not (tag[0] & 0x20):
            raise ValueError(f"read_png: {filename}: critical chunk {tag!r} is not supported")
        pos += 12 + n
    if ihdr is None or not idat:
        raise ValueError(f"read_png: {filename}: no IHDR or no IDAT chunk")
    w, h, depth, color, comp, filt, interlace = ihdr
    if depth != 8 or color not in (2, 6) or comp != 0 or filt != 0 or interlace != 0 or w == 0 or h == 0:
        raise ValueError(f"read_png: {filename}: only 8-bit RGB / RGBA non-interlaced PNGs are supported "
                         f"(bit depth {depth}, colour type {color}, interlace {interlace})")
    return zlib.decompress(b"".join(idat)), h, w, 3 if color == 2 else 4


def read_png_filtered(filename):
    """-> (filtered, H, W, channels): the inflated scanlines as bytes, H rows of 1 + W * channels bytes, each led by its filter-type
    byte - what swnerf.images.unfilter undoes on the device.  The file checks and refusals are read_png's, message for message;
    nothing is unfiltered and the alpha channel stays."""
    raw, h, w, c = _read_scanlines(filename)
    if len(raw) != h * (w * c + 1):
        raise ValueError(f"read_png: image data holds {len(raw)} bytes, expected {h * (w * c + 1)}")
    return raw, h, w, c


def read_png(filename):
    """-> uint8 [H,W,3].  8-bit RGB or RGBA (alpha dropped), non-interlaced; raises ValueError on anything else."""
    raw, h, w, c = _read_scanlines(filename)
    img = _unfilter(raw, h, w, c).reshape(h, w, c)
    return np.ascontiguousarray(img[..., :3])
