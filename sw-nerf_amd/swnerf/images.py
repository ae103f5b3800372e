"""The image stage of the dataset loaders (dataloader/*.py: `imageio.imread` of every frame, `cv2.resize(..., INTER_AREA)` for
half_res): the host parses chunks and inflates (swnerf.png.read_png_filtered), the device undoes the PNG row filters and
down-samples (csrc/image_kernels.hip).  The filtered bytes are exactly as large as the pixels and have to reach
the device anyway, so loading costs about what zlib costs.  There is no CPU path: png.read_png is the host reader."""
import os
import struct

import numpy as np
import torch

from . import _lib
from .png import read_png_filtered

_JPEG = (".jpg", ".jpeg")


def _device(device):
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if dev.type != "cuda":
        raise RuntimeError(f"swnerf.images: images are decoded on the GPU (got device {dev}); swnerf.png.read_png is the host reader")
    return dev


def _dev_tensor(t, name, dtypes):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"swnerf.images: {name} must be a torch.Tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise RuntimeError(f"swnerf.images: {name} must live on the GPU (got device {t.device}); there is no CPU path")
    if t.dtype not in dtypes:
        raise TypeError(f"swnerf.images: {name} must be {' or '.join(str(d) for d in dtypes)}, got {t.dtype}")
    return t.contiguous()


def _unfilter_into(filtered, n, H, W, c, out, status):
    """one launch; filtered / out / status: device tensors (or views) of n images"""
    _lib.check(_lib.lib().swnerf_png_unfilter(_lib.ptr(filtered), n, H, W, c, _lib.ptr(out), _lib.ptr(status), _lib.stream_of(out)),
               "png_unfilter")


def _raise_bad_rows(status, names=None):
    bad = torch.nonzero(status).reshape(-1).tolist()
    if bad:
        i = bad[0]
        who = f"image {i}" + (f" ({names[i]})" if names is not None else "")
        raise ValueError(f"swnerf.images.unfilter: {who}: unknown filter type on row {int(status[i]) - 1}")


def unfilter(filtered, H, W, channels):
    """filtered: device uint8, N * H * (1 + W * channels) bytes - the inflated scanlines of N PNGs of H x W pixels, each row led by
    its filter-type byte (png.read_png_filtered) -> uint8 [N,H,W,channels] on the same device.  ValueError names the first image
    and row whose type byte is not one of the five filters."""
    H, W, c = int(H), int(W), int(channels)
    filtered = _dev_tensor(filtered, "filtered", (torch.uint8,))
    per = H * (1 + W * c)
    if c not in (3, 4) or H < 1 or W < 1:
        raise ValueError(f"swnerf.images.unfilter: {H} x {W} x {c}: sizes are positive and channels 3 or 4")
    if filtered.numel() % per:
        raise ValueError(f"swnerf.images.unfilter: {filtered.numel()} bytes are no multiple of the {per} of one {H} x {W} x {c} image")
    n = filtered.numel() // per
    out = torch.empty((n, H, W, c), dtype=torch.uint8, device=filtered.device)
    status = torch.zeros((n,), dtype=torch.int32, device=filtered.device)
    if n:
        _unfilter_into(filtered, n, H, W, c, out, status)
        _raise_bad_rows(status.cpu())
    return out


def _resize_into(src, dst):
    n, H, W, c = (int(s) for s in src.shape)
    _lib.check(_lib.lib().swnerf_area_resize(_lib.ptr(src), int(src.dtype == torch.uint8), n, H, W, c, int(dst.shape[1]), int(dst.shape[2]),
                                             _lib.ptr(dst), _lib.stream_of(dst)), "area_resize")


def area_resize(images, h, w):
    """images: device [N,H,W,c] (or [H,W,c]) uint8 or float32, c in 1..4 -> float32 [N,h,w,c] (or [h,w,c]): the area mean that
    cv2.resize(..., INTER_AREA) defines for down-scaling, weights and sums in fp64, each output rounded once; a byte converts as
    (float)((double)u / 255.).  h == H, w == W is that conversion alone.  Up-scaling raises ValueError."""
    images = _dev_tensor(images, "images", (torch.uint8, torch.float32))
    single = images.dim() == 3
    x = images[None] if single else images
    if x.dim() != 4 or not 1 <= x.shape[-1] <= 4:
        raise ValueError(f"swnerf.images.area_resize: images must be [N,H,W,1..4], got {tuple(images.shape)}")
    h, w = int(h), int(w)
    if not (1 <= h <= x.shape[1] and 1 <= w <= x.shape[2]):
        raise ValueError(f"swnerf.images.area_resize: {x.shape[1]} x {x.shape[2]} -> {h} x {w} is not a down-scale")
    dst = torch.empty((x.shape[0], h, w, x.shape[3]), dtype=torch.float32, device=x.device)
    if dst.numel():
        _resize_into(x, dst)
    return dst[0] if single else dst


def image_size(path):
    """(H, W, channels) from the file's header alone: the IHDR chunk of a PNG; PIL for .jpg / .jpeg"""
    if path.lower().endswith(_JPEG):
        with _pil().open(path) as im:
            return im.size[1], im.size[0], 3
    with open(path, "rb") as f:
        head = f.read(33)
    if len(head) < 33 or head[:8] != b"\x89PNG\r\n\x1a\n" or head[12:16] != b"IHDR":
        raise ValueError(f"read_png: {path} is not a PNG file")
    w, h, depth, color = struct.unpack(">IIBB", head[16:26])
    return h, w, {0: 1, 2: 3, 4: 2, 6: 4}.get(color, 0)


def _pil():
    try:
        from PIL import Image
    except ImportError as e:
        raise RuntimeError("swnerf.images.load_pngs: .jpg / .jpeg frames are decoded by PIL, which is not installed; "
                           "convert them to 8-bit PNG (this package decodes only PNG itself)") from e
    return Image


def _read_host(path):
    """-> (bytes-like, H, W, channels, filtered?)"""
    if path.lower().endswith(_JPEG):
        with _pil().open(path) as im:
            a = np.ascontiguousarray(np.asarray(im.convert("RGB"), dtype=np.uint8))
        return a.reshape(-1), a.shape[0], a.shape[1], 3, False
    raw, h, w, c = read_png_filtered(path)
    return np.frombuffer(raw, np.uint8), h, w, c, True


def load_pngs(paths, device=None, out_hw=None, chunk_bytes=256 << 20, alpha=None):
    """Every file of `paths` (8-bit RGB / RGBA PNGs of one size; .jpg / .jpeg through PIL when it imports) as ONE device tensor in
    `paths` order: uint8 [N,H,W,c], or with out_hw = (h, w) - or a callable (H, W) -> (h, w) - float32 [N,h,w,c] from area_resize.
    The host inflates runs of files of one kind into pinned staging (two buffers of at most chunk_bytes) and copies without
    blocking, so the inflate of the next run overlaps the copy, unfilter and resize of this one.
    ValueError: files of different sizes; RGB and RGBA mixed - unless alpha="add", which appends an opaque alpha (255) to RGB
    frames as load_custom_data does; a filter-type byte above 4 (names the file and row)."""
    dev = _device(device)
    paths = [os.fspath(p) for p in paths]
    if not paths:
        raise ValueError("swnerf.images.load_pngs: no files")
    if alpha not in (None, "add"):
        raise ValueError(f"swnerf.images.load_pngs: alpha must be None or 'add', got {alpha!r}")
    first = _read_host(paths[0])
    H, W, c0 = first[1:4]
    c_out = 4 if alpha == "add" else c0
    if callable(out_hw):
        out_hw = out_hw(H, W)
    if out_hw is not None:
        out_hw = (int(out_hw[0]), int(out_hw[1]))
        if not (1 <= out_hw[0] <= H and 1 <= out_hw[1] <= W):
            raise ValueError(f"swnerf.images.load_pngs: {H} x {W} -> {out_hw[0]} x {out_hw[1]} is not a down-scale")
    n = len(paths)
    result = torch.empty((n, H, W, c_out), dtype=torch.uint8, device=dev) if out_hw is None else \
        torch.empty((n,) + out_hw + (c_out,), dtype=torch.float32, device=dev)
    status = torch.zeros((n,), dtype=torch.int32, device=dev)
    per_max = H * (1 + W * 4)
    per_run = max(1, min(n, int(chunk_bytes) // per_max))
    staging = [torch.empty((per_run * per_max,), dtype=torch.uint8).pin_memory() for _ in range(2 if n > per_run else 1)]
    copied = [None] * len(staging)                                   # the event after the last copy out of each staging buffer
    stream = torch.cuda.current_stream(dev)

    def flush(k, start, count, c, filtered):
        """files start .. start + count - 1 lie in staging[k]: copy, unfilter, widen, resize - all enqueued, nothing waits"""
        per = H * (1 + W * c) if filtered else H * W * c
        with torch.cuda.device(dev):
            d = staging[k][:count * per].to(dev, non_blocking=True)
            copied[k] = torch.cuda.Event()
            copied[k].record(stream)
            direct = out_hw is None and c == c_out
            px = result[start:start + count] if direct else torch.empty((count, H, W, c), dtype=torch.uint8, device=dev)
            if filtered:
                _unfilter_into(d, count, H, W, c, px, status[start:start + count])
            else:
                px.copy_(d.view(count, H, W, c))
            if c != c_out:                                               # alpha="add": RGB frames get an opaque alpha
                px = torch.cat([px, torch.full((count, H, W, 1), 255, dtype=torch.uint8, device=dev)], -1)
            if out_hw is not None:
                _resize_into(px, result[start:start + count])
            elif not direct:
                result[start:start + count].copy_(px)

    k, start, count, run_kind, off = 0, 0, 0, None, 0
    for i, p in enumerate(paths):
        raw, h, w, c, filtered = first if i == 0 else _read_host(p)
        if (h, w) != (H, W):
            raise ValueError(f"swnerf.images.load_pngs: {p} is {h} x {w}, {paths[0]} is {H} x {W}: one call loads one size")
        if c != c0 and alpha != "add":
            raise ValueError(f"swnerf.images.load_pngs: {p} has {c} channels, {paths[0]} has {c0}: pass alpha='add' to append "
                             "an opaque alpha to RGB frames")
        if count and (run_kind != (c, filtered) or count == per_run):
            flush(k, start, count, *run_kind)
            k, start, count, off = (k + 1) % len(staging), i, 0, 0
        if count == 0:
            run_kind = (c, filtered)
            if copied[k] is not None:
                copied[k].synchronize()                                  # the copy out of this staging buffer has finished
        staging[k].numpy()[off:off + raw.shape[0]] = raw
        off += raw.shape[0]
        count += 1
    flush(k, start, count, *run_kind)
    _raise_bad_rows(status.cpu(), paths)                                 # the one wait: also ends every copy out of staging
    return result
