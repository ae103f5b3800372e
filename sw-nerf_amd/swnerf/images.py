"""The image stage of the dataset loaders (dataloader/*.py: `imageio.imread` of every frame, `cv2.resize(..., INTER_AREA)` for
half_res): the host parses chunks and inflates (swnerf.png.read_png_filtered), the device undoes the PNG row filters and
down-samples (csrc/image_kernels.hip).  The filtered bytes are exactly as large as the pixels and have to reach
the device anyway, so loading costs about what zlib costs.  There is no CPU path: png.read_png is the host reader.
Baseline JPEG frames go the same way: the host reads markers and the Huffman stream (csrc/jpeg_host.h), the device dequantises,
inverts the DCT, up-samples chroma and converts colour with libjpeg's integer arithmetic (csrc/jpeg_kernels.hip), so the pixels
are imageio.imread's byte for byte.  A JPEG that is not decodable natively (progressive, arithmetic-coded, ...) goes to PIL.
The way back - encode_jpegs / write_jpeg, the frames of swnerf.video - is the same split run backwards: the device converts,
down-samples, transforms and quantises (csrc/jpeg_enc_kernels.hip), the host writes the Huffman stream (csrc/jpeg_enc_host.h), and
the file is what libjpeg writes for the same pixels, quality and sampling, byte for byte."""
import ctypes
import os
import struct
from concurrent.futures import ThreadPoolExecutor

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


class _Jpeg:
    """the header of a natively decodable JPEG file and its bytes; coefficients() is the Huffman decode"""

    def __init__(self, data, info, qt, name):
        self.data, self.name = data, name
        self.H, self.W, self.ncomp, self.sampling = (int(v) for v in info[:4])
        self.qt = qt[:self.ncomp * 64]
        self.ncoef = int(_lib.lib().swnerf_jpeg_coef_count(self.H, self.W, self.ncomp, self.sampling))
        self.kind = ("jpeg", self.ncomp, self.sampling)

    def coefficients(self):
        """int16 [ncoef]; ValueError names the file when its entropy-coded segment is corrupt"""
        coef = np.empty((self.ncoef,), np.int16)
        rc = _lib.lib().swnerf_jpeg_entropy(self.data, len(self.data), coef.ctypes.data, self.ncoef)     # ctypes drops the GIL
        if rc == _lib.E_DATA:
            raise ValueError(f"swnerf.images: {self.name}: {_lib.lib().swnerf_last_error().decode('utf-8', 'replace')}")
        _lib.check(rc, "jpeg_entropy")
        return coef


def _jpeg_header(data, name="<bytes>"):
    """-> _Jpeg, or None when the file is "not decodable here" (another decoder's turn).  No GPU call."""
    info = (ctypes.c_int32 * _lib.JPEG_INFO_LEN)()
    qt = np.zeros((_lib.JPEG_QT_LEN,), np.uint16)
    rc = _lib.lib().swnerf_jpeg_header(data, len(data), info, qt.ctypes.data)
    if rc == _lib.E_UNSUPP:
        return None
    _lib.check(rc, "jpeg_header")
    return _Jpeg(data, list(info), qt, name)


def _jpeg_decode_into(coef, qt, n, H, W, ncomp, sampling, out):
    """coef: the int16 coefficients of n images, qt: their uint16 tables [n * ncomp * 64], on the device (any dtype of the right
    byte count) -> out uint8 [n,H,W,3|4]; two launches, nothing waits"""
    planes = torch.empty((coef.numel() * coef.element_size() // 2,), dtype=torch.uint8, device=out.device)
    _lib.check(_lib.lib().swnerf_jpeg_decode(_lib.ptr(coef), _lib.ptr(qt), n, H, W, ncomp, sampling, int(out.shape[-1]),
                                             _lib.ptr(planes), _lib.ptr(out), _lib.stream_of(out)), "jpeg_decode")


_JPEG_WORKERS = 4                                                        # Huffman decoding ahead of the device; never more than 8


def decode_jpegs(files, device=None, channels=3):
    """files: the bytes of N baseline JPEG files of one size -> uint8 [N,H,W,channels] on the device, channels 3 (RGB) or 4 (alpha
    255): libjpeg's default decode byte for byte.  The host decodes the Huffman streams (a few files side by side), the device does
    the rest, one launch pair per run of files of one sampling.  ValueError: a file that is not decodable natively (progressive,
    arithmetic-coded, 12-bit, CMYK, RGB-coded, unusual sampling, several scans - the message says which), a corrupt
    entropy-coded segment, files of different sizes."""
    dev = _device(device)
    if channels not in (3, 4):
        raise ValueError(f"swnerf.images.decode_jpegs: channels must be 3 or 4, got {channels!r}")
    heads = []
    for i, data in enumerate(files):
        j = _jpeg_header(bytes(data), f"file {i}")
        if j is None:
            raise ValueError(f"swnerf.images.decode_jpegs: file {i}: {_lib.lib().swnerf_last_error().decode('utf-8', 'replace')}")
        if heads and (j.H, j.W) != (heads[0].H, heads[0].W):
            raise ValueError(f"swnerf.images.decode_jpegs: file {i} is {j.H} x {j.W}, file 0 is {heads[0].H} x {heads[0].W}: one call decodes one size")
        heads.append(j)
    if not heads:
        raise ValueError("swnerf.images.decode_jpegs: no files")
    out = torch.empty((len(heads), heads[0].H, heads[0].W, channels), dtype=torch.uint8, device=dev)
    with ThreadPoolExecutor(max_workers=min(_JPEG_WORKERS, len(heads))) as pool:
        coefs = list(pool.map(_Jpeg.coefficients, heads))
    start = 0
    while start < len(heads):
        end = start + 1
        while end < len(heads) and heads[end].kind == heads[start].kind:
            end += 1
        with torch.cuda.device(dev):
            coef = torch.from_numpy(np.concatenate(coefs[start:end])).to(dev)
            qt = torch.from_numpy(np.concatenate([j.qt for j in heads[start:end]]).view(np.int16)).to(dev)
            j = heads[start]
            _jpeg_decode_into(coef, qt, end - start, j.H, j.W, j.ncomp, j.sampling, out[start:end])
        start = end
    return out


def image_size(path):
    """(H, W, channels) from the file's header alone: the IHDR chunk of a PNG; the frame header of a .jpg / .jpeg (PIL when the
    file is not decodable natively)"""
    if path.lower().endswith(_JPEG):
        with open(path, "rb") as f:
            j = _jpeg_header(f.read(), path)
        if j is not None:
            return j.H, j.W, 3
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
        raise RuntimeError("swnerf.images.load_pngs: this .jpg / .jpeg frame is not a baseline JPEG this package decodes itself "
                           "(8-bit, Huffman-coded, one scan, gray or YCbCr at 4:4:4 / 4:2:2 / 4:2:0); such files are decoded by PIL, "
                           "which is not installed; convert them to baseline JPEG or 8-bit PNG") from e
    return Image


def _read_host(path):
    """-> (bytes, H, W, channels, kind, tables): kind True = filtered PNG scanlines, False = plain pixels, ("jpeg", components,
    sampling) = the int16 coefficients of a natively decodable JPEG, with its quantisation tables (None otherwise)"""
    if path.lower().endswith(_JPEG):
        with open(path, "rb") as f:
            j = _jpeg_header(f.read(), path)
        if j is not None:
            return j.coefficients().view(np.uint8), j.H, j.W, 3, j.kind, j.qt.view(np.uint8)
        with _pil().open(path) as im:
            a = np.ascontiguousarray(np.asarray(im.convert("RGB"), dtype=np.uint8))
        return a.reshape(-1), a.shape[0], a.shape[1], 3, False, None
    raw, h, w, c = read_png_filtered(path)
    return np.frombuffer(raw, np.uint8), h, w, c, True, None


def load_pngs(paths, device=None, out_hw=None, chunk_bytes=256 << 20, alpha=None):
    """Every file of `paths` (8-bit RGB / RGBA PNGs and .jpg / .jpeg files of one size) as ONE device tensor in `paths` order:
    uint8 [N,H,W,c], or with out_hw = (h, w) - or a callable (H, W) -> (h, w) - float32 [N,h,w,c] from area_resize.
    The host inflates (PNG) or Huffman-decodes (baseline JPEG) runs of files of one kind into pinned staging (two buffers of at
    most chunk_bytes, sized from the first file) and copies without blocking, so the host work of the next run overlaps the copy,
    unfilter / inverse DCT and resize of this one; when a .jpg / .jpeg is among them, the next few files are read ahead on a small
    thread pool.  A JPEG that is not decodable natively is decoded by PIL when it imports (RuntimeError naming PIL otherwise).
    ValueError: files of different sizes; 3 and 4 channels mixed - unless alpha="add", which appends an opaque alpha (255) to RGB
    frames as load_custom_data does; a PNG filter-type byte above 4 (names the file and row); a corrupt entropy-coded segment of
    a JPEG (names the file)."""
    dev = _device(device)
    paths = [os.fspath(p) for p in paths]
    if not paths:
        raise ValueError("swnerf.images.load_pngs: no files")
    if alpha not in (None, "add"):
        raise ValueError(f"swnerf.images.load_pngs: alpha must be None or 'add', got {alpha!r}")
    any_jpeg = any(p.lower().endswith(_JPEG) for p in paths)
    pool = ThreadPoolExecutor(max_workers=min(_JPEG_WORKERS, len(paths))) if any_jpeg and len(paths) > 1 else None
    try:
        return _load(paths, dev, out_hw, chunk_bytes, alpha, any_jpeg, pool)
    finally:
        if pool is not None:
            pool.shutdown(wait=True, cancel_futures=True)


def _load(paths, dev, out_hw, chunk_bytes, alpha, any_jpeg, pool):
    n = len(paths)
    ahead = {}                                                           # index -> future of _read_host

    def read(i):
        if pool is None:
            return _read_host(paths[i])
        for j in range(i, min(n, i + 2 * _JPEG_WORKERS)):
            if j not in ahead:
                ahead[j] = pool.submit(_read_host, paths[j])
        return ahead.pop(i).result()

    first = read(0)
    H, W, c0 = first[1:4]
    c_out = 4 if alpha == "add" else c0
    if callable(out_hw):
        out_hw = out_hw(H, W)
    if out_hw is not None:
        out_hw = (int(out_hw[0]), int(out_hw[1]))
        if not (1 <= out_hw[0] <= H and 1 <= out_hw[1] <= W):
            raise ValueError(f"swnerf.images.load_pngs: {H} x {W} -> {out_hw[0]} x {out_hw[1]} is not a down-scale")
    result = torch.empty((n, H, W, c_out), dtype=torch.uint8, device=dev) if out_hw is None else \
        torch.empty((n,) + out_hw + (c_out,), dtype=torch.float32, device=dev)
    status = torch.zeros((n,), dtype=torch.int32, device=dev)
    per_max = max(H * (1 + W * 4), int(first[0].shape[0]))               # a JPEG's coefficients are 2 bytes each, planes padded to MCUs
    per_run = max(1, min(n, int(chunk_bytes) // per_max))
    staging = [torch.empty((per_run * per_max,), dtype=torch.uint8).pin_memory() for _ in range(2 if n > per_run else 1)]
    tables = [torch.empty((per_run * 2 * _lib.JPEG_QT_LEN,), dtype=torch.uint8).pin_memory() for _ in staging] if any_jpeg else None
    copied = [None] * len(staging)                                   # the event after the last copy out of each staging buffer
    stream = torch.cuda.current_stream(dev)

    def flush(k, start, count, nbytes, c, kind):
        """files start .. start + count - 1 lie in staging[k]: copy, unfilter / inverse DCT, widen, resize - all enqueued, nothing waits"""
        jpeg = isinstance(kind, tuple)
        with torch.cuda.device(dev):
            d = staging[k][:nbytes].to(dev, non_blocking=True)
            q = tables[k][:count * kind[1] * 128].to(dev, non_blocking=True) if jpeg else None
            copied[k] = torch.cuda.Event()
            copied[k].record(stream)
            c_px = c_out if jpeg else c                                  # the JPEG kernel writes the opaque alpha itself
            direct = out_hw is None and c_px == c_out
            px = result[start:start + count] if direct else torch.empty((count, H, W, c_px), dtype=torch.uint8, device=dev)
            if jpeg:
                _jpeg_decode_into(d, q, count, H, W, kind[1], kind[2], px)
            elif kind:
                _unfilter_into(d, count, H, W, c, px, status[start:start + count])
            else:
                px.copy_(d.view(count, H, W, c))
            if c_px != c_out:                                            # alpha="add": RGB frames get an opaque alpha
                px = torch.cat([px, torch.full((count, H, W, 1), 255, dtype=torch.uint8, device=dev)], -1)
            if out_hw is not None:
                _resize_into(px, result[start:start + count])
            elif not direct:
                result[start:start + count].copy_(px)

    k, start, count, run_kind, off = 0, 0, 0, None, 0
    for i, p in enumerate(paths):
        raw, h, w, c, kind, qt = first if i == 0 else read(i)
        if (h, w) != (H, W):
            raise ValueError(f"swnerf.images.load_pngs: {p} is {h} x {w}, {paths[0]} is {H} x {W}: one call loads one size")
        if c != c0 and alpha != "add":
            raise ValueError(f"swnerf.images.load_pngs: {p} has {c} channels, {paths[0]} has {c0}: pass alpha='add' to append "
                             "an opaque alpha to RGB frames")
        need = int(raw.shape[0])
        if count and (run_kind != (c, kind) or count == per_run or off + need > staging[k].numel()):
            flush(k, start, count, off, *run_kind)
            k, start, count, off = (k + 1) % len(staging), i, 0, 0
        if count == 0:
            run_kind = (c, kind)
            if copied[k] is not None:
                copied[k].synchronize()                                  # the copy out of this staging buffer has finished
            if need > staging[k].numel():                                # a JPEG with more coefficients than the first file's
                staging[k] = torch.empty((need,), dtype=torch.uint8).pin_memory()
        staging[k].numpy()[off:off + need] = raw
        if qt is not None:
            tables[k].numpy()[count * qt.shape[0]:(count + 1) * qt.shape[0]] = qt
        off += need
        count += 1
    flush(k, start, count, off, *run_kind)
    _raise_bad_rows(status.cpu(), paths)                                 # the one wait: also ends every copy out of staging
    return result


# ---- encode ---------------------------------------------------------------------------------------------------------------
_SUBSAMPLING = {"4:4:4": "JPEG_444", "4:2:2": "JPEG_422", "4:2:0": "JPEG_420"}


def _as_frames(frames):
    """-> (tensor or ndarray [N,H,W,c], single): [N,H,W,1|3|4]; a 3-D input whose last side is 1, 3 or 4 is ONE frame [H,W,c],
    any other 3-D input is [N,H,W]; 2-D is one [H,W] frame"""
    if not isinstance(frames, (torch.Tensor, np.ndarray)):
        frames = np.asarray(frames)
    shape = tuple(frames.shape)
    if len(shape) == 2:
        return frames[None, :, :, None], True
    if len(shape) == 3:
        return (frames[None], True) if shape[-1] in (1, 3, 4) else (frames[..., None], False)
    if len(shape) == 4 and shape[-1] in (1, 3, 4):
        return frames, False
    raise ValueError(f"swnerf.images.encode_jpegs: frames must be [N,H,W,1|3|4], [N,H,W], [H,W,1|3|4] or [H,W], got {shape}")


def _jpeg_write_host(coef, qt, H, W, ncomp, sampling, bound):
    """one frame's int16 coefficients (host) -> the bytes of its file; ctypes drops the GIL for the call"""
    out = np.empty((bound,), np.uint8)
    n = _lib.lib().swnerf_jpeg_write(coef.ctypes.data, coef.shape[0], qt.ctypes.data, H, W, ncomp, sampling, out.ctypes.data, bound)
    if n < 0:
        _lib.check(int(n), "jpeg_write")
    return out[:n].tobytes()


def encode_jpegs(frames, quality=90, subsampling="4:2:0", divisor=None, components=None, device=None, chunk_bytes=256 << 20):
    """frames: a device tensor or a numpy array, uint8 or float32, [N,H,W,1|3|4] (alpha ignored), [N,H,W], or one frame without
    the leading N (a 3-D input whose last side is 1, 3 or 4 is one frame) -> the bytes of N baseline JPEG files: what libjpeg
    (PIL's Image.save(format="JPEG", quality=quality, subsampling=...)) writes for the same pixels, byte for byte.  A float sample
    becomes a byte as the reference's to8b does, (uint8)(255 * clip(x, 0, 1)), of x / divisor when a divisor is given
    (to8b(disps / np.max(disps))); NaN gives 0.  components: 3 (YCbCr; the default, also for 1-channel input, which players handle
    most reliably) or 1 (a grey file; needs 1-channel input).  The device converts, down-samples, transforms and quantises in
    chunks of at most chunk_bytes (host arrays go up through pinned staging); while it works on one chunk, the coefficients of the
    chunk before are Huffman-coded on the small thread pool decode_jpegs uses."""
    L = _lib.lib()
    x, _ = _as_frames(frames)
    on_host = not isinstance(x, torch.Tensor)
    if on_host:
        if x.dtype not in (np.uint8, np.float32):
            raise TypeError(f"swnerf.images.encode_jpegs: frames must be uint8 or float32, got {x.dtype}")
        x = np.ascontiguousarray(x)
        dev = _device(device)
    else:
        x = _dev_tensor(x, "frames", (torch.uint8, torch.float32))
        dev = x.device
    n, H, W, cin = (int(v) for v in x.shape)
    ncomp = 3 if components is None else int(components)
    if ncomp not in (1, 3) or (ncomp == 1 and cin != 1):
        raise ValueError(f"swnerf.images.encode_jpegs: components must be 3, or 1 for 1-channel input; got {components!r} for {cin} channel(s)")
    if subsampling not in _SUBSAMPLING:
        raise ValueError(f"swnerf.images.encode_jpegs: subsampling must be one of {', '.join(_SUBSAMPLING)}, got {subsampling!r}")
    sampling = _lib.JPEG_444 if ncomp == 1 else getattr(_lib, _SUBSAMPLING[subsampling])
    if not (1 <= H <= 65535 and 1 <= W <= 65535):
        raise ValueError(f"swnerf.images.encode_jpegs: frame size {H} x {W} outside 1..65535")
    if n == 0:
        return []
    is_u8 = x.dtype in (np.uint8, torch.uint8)
    qt = np.empty((2, 64), np.uint16)
    _lib.check(L.swnerf_jpeg_quant_tables(int(quality), qt.ctypes.data), "jpeg_quant_tables")
    ncoef = int(L.swnerf_jpeg_coef_count(H, W, ncomp, sampling))
    bound = int(L.swnerf_jpeg_file_bound(H, W, ncomp, sampling))
    per_in = H * W * cin * (1 if is_u8 else 4)
    per_run = max(1, min(n, int(chunk_bytes) // max(per_in, 2 * ncoef)))
    runs = [(s, min(n, s + per_run)) for s in range(0, n, per_run)]
    two = 2 if len(runs) > 1 else 1
    host_coef = [torch.empty((per_run, ncoef), dtype=torch.int16).pin_memory() for _ in range(two)]
    staging = [torch.empty((per_run * per_in,), dtype=torch.uint8).pin_memory() for _ in range(two)] if on_host else None
    done = [None] * two                                                  # the event after the copy into host_coef[k]
    futures = [[] for _ in runs]
    with torch.cuda.device(dev), ThreadPoolExecutor(max_workers=min(_JPEG_WORKERS, n)) as pool:
        stream = torch.cuda.current_stream(dev)
        qt_dev = torch.from_numpy(np.ascontiguousarray(qt[[0, 1, 1][:ncomp]]).view(np.int16)).to(dev)

        def huffman(r):
            """run r has been enqueued: wait for its coefficients and hand its frames to the pool"""
            k = r % two
            done[k].synchronize()
            rows = host_coef[k].numpy()
            futures[r] = [pool.submit(_jpeg_write_host, rows[i], qt, H, W, ncomp, sampling, bound) for i in range(runs[r][1] - runs[r][0])]

        for r, (a, b) in enumerate(runs):
            k = r % two
            if r >= two:
                for f in futures[r - two]:                               # host_coef[k] (and staging[k]) are free again
                    f.result()
            if on_host:
                src = x[a:b].reshape(-1).view(np.uint8)
                staging[k].numpy()[:src.shape[0]] = src
                d = staging[k][:src.shape[0]].to(dev, non_blocking=True)
            else:
                d = x[a:b]
            coef = torch.empty((b - a, ncoef), dtype=torch.int16, device=dev)
            planes = torch.empty((b - a, ncoef), dtype=torch.uint8, device=dev)
            _lib.check(L.swnerf_jpeg_encode(_lib.ptr(d), int(is_u8), b - a, H, W, cin, float(divisor) if divisor else 0.0, _lib.ptr(qt_dev),
                                            ncomp, sampling, _lib.ptr(planes), _lib.ptr(coef), _lib.stream_of(coef)), "jpeg_encode")
            host_coef[k][:b - a].copy_(coef, non_blocking=True)
            done[k] = torch.cuda.Event()
            done[k].record(stream)
            if r:
                huffman(r - 1)                                           # overlaps the device's work on run r
        huffman(len(runs) - 1)
        return [f.result() for fs in futures for f in fs]


def encode_coefficients(frames, qt, subsampling="4:2:0", divisor=None, components=None):
    """the device half of encode_jpegs alone: frames as encode_jpegs takes them, but on the device; qt: uint16 [2][64] natural
    order (luma, chroma) -> int16 [N, coef_count] on the device, in the layout swnerf_jpeg_entropy produces"""
    L = _lib.lib()
    x, _ = _as_frames(frames)
    x = _dev_tensor(x, "frames", (torch.uint8, torch.float32))
    n, H, W, cin = (int(v) for v in x.shape)
    ncomp = 3 if components is None else int(components)
    sampling = _lib.JPEG_444 if ncomp == 1 else getattr(_lib, _SUBSAMPLING[subsampling])
    ncoef = int(L.swnerf_jpeg_coef_count(H, W, ncomp, sampling))
    qt = np.ascontiguousarray(np.asarray(qt, np.uint16).reshape(2, 64)[[0, 1, 1][:ncomp]])
    with torch.cuda.device(x.device):
        qt_dev = torch.from_numpy(qt.view(np.int16)).to(x.device)
        coef = torch.empty((n, ncoef), dtype=torch.int16, device=x.device)
        planes = torch.empty((n, ncoef), dtype=torch.uint8, device=x.device)
        _lib.check(L.swnerf_jpeg_encode(_lib.ptr(x), int(x.dtype == torch.uint8), n, H, W, cin, float(divisor) if divisor else 0.0,
                                        _lib.ptr(qt_dev), ncomp, sampling, _lib.ptr(planes), _lib.ptr(coef), _lib.stream_of(coef)), "jpeg_encode")
    return coef


def write_jpeg(path, img, quality=90, subsampling="4:2:0", divisor=None, components=None, device=None):
    """one frame ([H,W,1|3|4] or [H,W]; a device tensor or a numpy array, uint8 or float32) as a baseline JPEG file - the lossy
    sibling of png.write_png; the arguments are encode_jpegs'"""
    x, single = _as_frames(img)
    if not single:
        raise ValueError(f"swnerf.images.write_jpeg: one frame [H,W,1|3|4] or [H,W], got {tuple(img.shape)}")
    data = encode_jpegs(x, quality, subsampling, divisor, components, device)[0]
    with open(path, "wb") as f:
        f.write(data)
