"""Render videos (every trainer of the reference ends its i_video / render_only / render_test branch with
imageio.mimwrite(path + 'rgb.mp4', to8b(rgbs), fps=30, quality=8)): a Motion-JPEG AVI - baseline JPEG frames, encoded on the
device (swnerf.images.encode_jpegs: libjpeg's bytes), in a RIFF container written here.  It needs no codec library; ffmpeg, VLC,
OpenCV and browsers' players read it.  MJPEG `.avi` replaces the reference's H.264 `.mp4` (DESIGN.md 6k "JPEG encode")."""
import os
import struct
from fractions import Fraction

import numpy as np

AVI_MAX_BYTES = (1 << 31) - 1            # plain AVI (no OpenDML): 32-bit sizes and index offsets that players read as signed
_AVIF_HASINDEX, _AVIIF_KEYFRAME = 0x10, 0x10


def _chunk(fourcc, payload):
    return fourcc + struct.pack("<I", len(payload)) + payload + (b"\0" if len(payload) & 1 else b"")


def _headers(n, H, W, fps, sizes):
    """the `hdrl` list: avih, and one stream list with strh (vids / MJPG) and strf (BITMAPINFOHEADER)"""
    rate = Fraction(fps).limit_denominator(100000)
    if rate <= 0:
        raise ValueError(f"swnerf.video: fps must be positive, got {fps!r}")
    biggest = max(sizes, default=0)
    avih = struct.pack("<14I", int(round(1e6 / rate)), int(biggest * rate) + 1, 0, _AVIF_HASINDEX, n, 0, 1, biggest, W, H, 0, 0, 0, 0)
    strh = b"vidsMJPG" + struct.pack("<IHHIIIIIIIIhhHH", 0, 0, 0, 0, rate.denominator, rate.numerator, 0, n, biggest, 0xFFFFFFFF, 0, 0, 0, W, H)
    strf = struct.pack("<IiiHH4sIiiII", 40, W, H, 1, 24, b"MJPG", W * H * 3, 0, 0, 0, 0)
    strl = b"strl" + _chunk(b"strh", strh) + _chunk(b"strf", strf)
    return b"hdrl" + _chunk(b"avih", avih) + _chunk(b"LIST", strl)


def avi_bytes(sizes, header_len):
    """the size of the file write_avi makes of frames of these sizes"""
    movi = 4 + sum(8 + s + (s & 1) for s in sizes)
    return 12 + 8 + header_len + 8 + movi + 8 + 16 * len(sizes)


def write_avi(path, jpeg_bytes_list, H, W, fps=30):
    """The container step alone, on the host: RIFF 'AVI ' { LIST hdrl { avih, LIST strl { strh, strf } }, LIST movi { one '00dc'
    chunk per frame, padded to even length }, idx1 { one key-frame entry per frame, offsets from the 'movi' tag } }.  Written to
    a temporary name beside `path` and renamed at the end.  ValueError (and no file) when the file would pass 2 GiB: plain AVI has
    no OpenDML index."""
    frames = [bytes(f) for f in jpeg_bytes_list]
    if not frames:
        raise ValueError("swnerf.video.write_avi: no frames")
    H, W = int(H), int(W)
    sizes = [len(f) for f in frames]
    hdrl = _headers(len(frames), H, W, fps, sizes)
    total = avi_bytes(sizes, len(hdrl))
    if total > AVI_MAX_BYTES:
        raise ValueError(f"swnerf.video.write_avi: {path} would have {total} bytes; plain AVI ends at 2 GiB (write fewer frames per "
                         "file, or a lower quality)")
    movi_len = 4 + sum(8 + s + (s & 1) for s in sizes)
    index, off = [], 4                                                   # offsets count from the 'movi' tag
    for s in sizes:
        index.append(b"00dc" + struct.pack("<III", _AVIIF_KEYFRAME, off, s))
        off += 8 + s + (s & 1)
    path = os.fspath(path)
    tmp = f"{path}.tmp{os.getpid()}"
    try:
        with open(tmp, "wb") as f:
            f.write(b"RIFF" + struct.pack("<I", total - 8) + b"AVI ")
            f.write(_chunk(b"LIST", hdrl))
            f.write(b"LIST" + struct.pack("<I", movi_len) + b"movi")
            for data in frames:
                f.write(_chunk(b"00dc", data))
            f.write(_chunk(b"idx1", b"".join(index)))
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return path


def write_video(path, frames, fps=30, quality=90, subsampling="4:2:0", divisor=None):
    """frames: what swnerf.images.encode_jpegs takes ([N,H,W,1|3|4] or [N,H,W], uint8 or float32, a device tensor or a numpy
    array; floats become bytes as to8b does, of x / divisor when given) -> an MJPEG AVI at `path`, YCbCr frames at JPEG `quality`."""
    from . import images
    x, _ = images._as_frames(frames)
    jpegs = images.encode_jpegs(x, quality=quality, subsampling=subsampling, divisor=divisor)
    return write_avi(path, jpegs, int(x.shape[1]), int(x.shape[2]), fps)


def mimwrite(uri, ims, fps=30, quality=8, **ignored):
    """Call-compatible stand-in for imageio.mimwrite(uri, ims, fps=30, quality=8): the extension is replaced by .avi, imageio's
    quality 0..10 maps to JPEG quality 50 + 5 quality (the reference's 8 gives 90); other keywords are ignored.  -> the path written."""
    path = os.path.splitext(os.fspath(uri))[0] + ".avi"
    if isinstance(ims, (list, tuple)):
        ims = np.stack([np.asarray(i) for i in ims])
    q = 90 if quality is None else int(min(max(50 + 5 * float(quality), 1), 100))
    return write_video(path, ims, fps=fps, quality=q)
