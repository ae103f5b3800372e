"""Counterpart of the reference's multires_dnerf/pyramid.py on the HIP kernels of csrc/pyramid_kernels.hip:
the Laplacian pyramid of NHWC frames that the MultiRes D-NeRF runner trains one DirectTemporalNeRF per level on.

  create_gaussian_kernel(kernel_size, sigma, channels=3)                      pyramid.py:8-24 (host glue, torch)
  generate_laplacian_pyramid_batch(images, levels=4, kernel_size=3, sigma=1.0)  pyramid.py:46-80
  reconstruct_image_from_pyramid_batch(laplacian_pyramid)                       pyramid.py:82-98, differentiable
  reconstruct_and_compute_loss(pyramid_outputs, target)                         multires_dnerf.py:487-497

All image arithmetic runs in three kernels: swnerf_pyramid_down (blur + 1/2 downsample fused), swnerf_pyramid_up_axpy
(out = base + alpha * upsample(coarse)) and swnerf_pyramid_up_adjoint (the transpose of the upsample, for backward).
There is no CPU implementation: the images must be, or are sent to, the GPU."""
import numpy as np
import torch

from . import _lib

MAX_KERNEL = 7
CHUNK_BYTES = 1 << 30                   # level 0 of one chunk, as in swnerf.metrics


def create_gaussian_kernel(kernel_size, sigma, channels=3):
    """pyramid.py:8-24: the normalised fp32 window, repeated to (channels, 1, k, k) as F.conv2d(groups=channels) takes it."""
    coords = torch.arange(kernel_size, dtype=torch.float32) - (kernel_size - 1) / 2
    grid = torch.meshgrid(coords, coords, indexing="ij")
    kernel = torch.exp(-(grid[0] ** 2 + grid[1] ** 2) / (2 * sigma ** 2))
    kernel = kernel / kernel.sum()
    kernel = kernel.unsqueeze(0).unsqueeze(0)
    return kernel.repeat(channels, 1, 1, 1)


def _device(t):
    if isinstance(t, torch.Tensor) and t.is_cuda:
        return t.device
    if not torch.cuda.is_available():
        raise RuntimeError("swnerf.pyramid: no GPU - the pyramid is HIP kernels with no CPU implementation")
    return torch.device("cuda", torch.cuda.current_device())


def _check_nhwc(shape, name):
    if len(shape) != 4:
        raise ValueError(f"swnerf.pyramid: {name} must be [N,H,W,C], got shape {tuple(shape)}")
    if not 1 <= shape[3] <= 4:
        raise NotImplementedError(f"swnerf.pyramid: {name} has {shape[3]} channels; 1..4 are built")
    if shape[1] < 1 or shape[2] < 1:
        raise ValueError(f"swnerf.pyramid: {name} is empty: shape {tuple(shape)}")


def _check_kernel_size(kernel_size):
    k = int(kernel_size)
    if k != kernel_size or k < 1 or k % 2 == 0 or k > MAX_KERNEL:
        raise ValueError(f"swnerf.pyramid: kernel_size must be odd and at most {MAX_KERNEL}, got {kernel_size!r}")
    return k


def down(x, weights, kernel_size):
    """box2x2(blur_k(x)): x [N,H,W,C] device fp32 -> [N,H//2,W//2,C]; weights: device fp32 [k*k]."""
    x = _lib.dev_f32(x, "images")
    n, h, w, c = x.shape
    out = torch.empty((n, h // 2, w // 2, c), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().swnerf_pyramid_down(_lib.ptr(x), n, h, w, c, _lib.ptr(weights), kernel_size, _lib.ptr(out),
                                              _lib.stream_of(x)), "pyramid_down")
    return out


def up_axpy(coarse, size, base=None, alpha=1.0):
    """base + alpha * up(coarse) at size (H, W) (bilinear, align_corners=False); base None: alpha * up(coarse)."""
    coarse = _lib.dev_f32(coarse, "coarse")
    n, h, w, c = coarse.shape
    H, W = int(size[0]), int(size[1])
    if base is not None:
        base = _lib.dev_f32(base, "base")
        if tuple(base.shape) != (n, H, W, c):
            raise ValueError(f"swnerf.pyramid: base is {tuple(base.shape)}, expected {(n, H, W, c)}")
    out = torch.empty((n, H, W, c), dtype=torch.float32, device=coarse.device)
    _lib.check(_lib.lib().swnerf_pyramid_up_axpy(_lib.ptr(coarse), n, h, w, c, _lib.ptr(base), float(alpha), H, W, _lib.ptr(out),
                                                 _lib.stream_of(coarse)), "pyramid_up_axpy")
    return out


def up_adjoint(g_out, size):
    """transpose of up: g_out [N,H,W,C] -> [N,h,w,C] for size (h, w); a gather in a fixed order (bit-identical runs)."""
    g_out = _lib.dev_f32(g_out, "g_out")
    n, H, W, c = g_out.shape
    h, w = int(size[0]), int(size[1])
    out = torch.empty((n, h, w, c), dtype=torch.float32, device=g_out.device)
    _lib.check(_lib.lib().swnerf_pyramid_up_adjoint(_lib.ptr(g_out), n, H, W, c, h, w, _lib.ptr(out), _lib.stream_of(g_out)),
               "pyramid_up_adjoint")
    return out


def generate_laplacian_pyramid_batch(images, levels=4, kernel_size=3, sigma=1.0, chunk_frames=None):
    """pyramid.py:46-80: images [N,H,W,C] -> list of `levels` NHWC tensors on the GPU, level l of size (H // 2^l, W // 2^l):
    g_0 = images, g_{l+1} = down(g_l), level l = g_l - up(g_{l+1}), the last level = g_{levels-1}.
    The reference builds one Gaussian level more than it uses; here levels - 1 are built, so min(H, W) >= 2^(levels-1) is
    enough.  Host images (numpy, CPU tensors) are sent in chunks of `chunk_frames` frames (default: CHUNK_BYTES of level
    0), and device images are processed in such chunks too, so the Gaussian levels of only one chunk are alive at a time."""
    levels = int(levels)
    if levels < 1:
        raise ValueError(f"swnerf.pyramid: levels must be at least 1, got {levels}")
    k = _check_kernel_size(kernel_size)
    if not isinstance(images, torch.Tensor):
        images = torch.from_numpy(np.ascontiguousarray(images))
    _check_nhwc(images.shape, "images")
    n, h, w, c = images.shape
    if min(h, w) < 2 ** (levels - 1):
        raise ValueError(f"swnerf.pyramid: {levels} levels need min(H, W) >= {2 ** (levels - 1)}, got images of {h} x {w}")
    dev = _device(images)
    if levels == 1:
        return [images.to(device=dev, dtype=torch.float32)]
    weights = create_gaussian_kernel(k, sigma, 1).reshape(-1).to(dev)
    sizes = [(h >> l, w >> l) for l in range(levels)]
    out = [torch.empty((n, hl, wl, c), dtype=torch.float32, device=dev) for hl, wl in sizes]
    chunk = int(chunk_frames) if chunk_frames else max(1, CHUNK_BYTES // (h * w * c * 4))
    L = _lib.lib()
    for s in range(0, n, chunk):
        e = min(n, s + chunk)
        g = images[s:e].to(device=dev, dtype=torch.float32).contiguous()
        for l in range(levels - 1):
            nxt = out[l + 1][s:e] if l + 1 == levels - 1 else None          # the last Gaussian level IS the last pyramid level
            if nxt is None:
                nxt = down(g, weights, k)
            else:
                _lib.check(L.swnerf_pyramid_down(_lib.ptr(g), e - s, sizes[l][0], sizes[l][1], c, _lib.ptr(weights), k,
                                                 _lib.ptr(nxt), _lib.stream_of(g)), "pyramid_down")
            _lib.check(L.swnerf_pyramid_up_axpy(_lib.ptr(nxt), e - s, sizes[l + 1][0], sizes[l + 1][1], c, _lib.ptr(g), -1.0,
                                                sizes[l][0], sizes[l][1], _lib.ptr(out[l][s:e]), _lib.stream_of(g)),
                       "pyramid_up_axpy")
            g = nxt
    return out


class _Reconstruct(torch.autograd.Function):
    """r = lap[-1]; r = lap[i] + up(r) for i = len-2 .. 0.  Backward: every level receives the running gradient unchanged,
    and up^T of it goes down to the next level."""

    @staticmethod
    def forward(ctx, *levels):
        ctx.sizes = [tuple(l.shape[1:3]) for l in levels]
        return _reconstruct_raw(levels)

    @staticmethod
    def backward(ctx, g):
        g = _lib.dev_f32(g, "grad")
        grads = [g]
        for i in range(1, len(ctx.sizes)):
            g = up_adjoint(g, ctx.sizes[i])
            grads.append(g)
        return tuple(gi if need else None for gi, need in zip(grads, ctx.needs_input_grad))


def _reconstruct_raw(levels):
    r = _lib.dev_f32(levels[-1], "laplacian_pyramid[-1]")
    if len(levels) == 1:
        return r.clone()
    for i in range(len(levels) - 2, -1, -1):
        r = up_axpy(r, levels[i].shape[1:3], base=levels[i], alpha=1.0)
    return r


def reconstruct_image_from_pyramid_batch(laplacian_pyramid):
    """pyramid.py:82-98: the sum of the levels, each upsampled to the size of the one above it: NHWC levels (a list, or a
    stacked tensor [levels, N, H, W, C] of equal-size levels - the reference passes both) -> [N, H_0, W_0, C].
    Differentiable with respect to every level; a call outside autograd skips the bookkeeping."""
    levels = list(laplacian_pyramid.unbind(0)) if isinstance(laplacian_pyramid, torch.Tensor) else list(laplacian_pyramid)
    if not levels:
        raise ValueError("swnerf.pyramid: an empty pyramid")
    dev = None
    for l in levels:
        if not isinstance(l, torch.Tensor):
            raise TypeError(f"swnerf.pyramid: pyramid levels must be torch tensors, got {type(l).__name__}")
        _check_nhwc(l.shape, "a pyramid level")
        dev = l.device if l.is_cuda and dev is None else dev
    n, c = levels[0].shape[0], levels[0].shape[3]
    if any(l.shape[0] != n or l.shape[3] != c for l in levels):
        raise ValueError(f"swnerf.pyramid: levels differ in batch or channels: {[tuple(l.shape) for l in levels]}")
    if dev is None:
        dev = _device(None)
    levels = [l if l.is_cuda else l.to(dev) for l in levels]
    if torch.is_grad_enabled() and any(l.requires_grad for l in levels):
        return _Reconstruct.apply(*levels)
    return _reconstruct_raw([l.detach() for l in levels])


def reconstruct_and_compute_loss(pyramid_outputs, target_images):
    """multires_dnerf.py:487-497: (reconstruction of frame 0 [H,W,C], its MSE against target_images, PSNR = 10 log10(1 / MSE))."""
    reconstructed = reconstruct_image_from_pyramid_batch(pyramid_outputs)[0]
    loss = torch.nn.functional.mse_loss(reconstructed, target_images)
    psnr = 10 * torch.log10(1 / loss)
    return reconstructed, loss, psnr
