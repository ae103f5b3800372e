"""numpy float64 restatement of the Laplacian pyramid of multires_dnerf/pyramid.py on NHWC arrays: the 3x3 (k x k) Gaussian
blur with zero padding, the 2x2 box that F.interpolate(scale_factor=0.5, bilinear, align_corners=False) computes, the
bilinear upsample `up` to an arbitrary size with align_corners=False, its transpose in scatter form, generate and
reconstruct.  Everything, the source coordinates included, is float64: the distance of an fp32 implementation from this
is that implementation's own rounding."""
import numpy as np


def gaussian_kernel(kernel_size, sigma):
    """create_gaussian_kernel's [k, k] window, float64"""
    c = np.arange(kernel_size, dtype=np.float64) - (kernel_size - 1) / 2
    g = np.exp(-(c[:, None] ** 2 + c[None, :] ** 2) / (2 * sigma ** 2))
    return g / g.sum()


def blur(x, kernel):
    """k x k cross-correlation, zero padding k // 2; x [N,H,W,C]"""
    x = np.asarray(x, np.float64)
    k = kernel.shape[0]
    r = k // 2
    n, h, w, c = x.shape
    p = np.zeros((n, h + 2 * r, w + 2 * r, c))
    p[:, r:r + h, r:r + w] = x
    out = np.zeros_like(x)
    for a in range(k):
        for b in range(k):
            out += kernel[a, b] * p[:, a:a + h, b:b + w]
    return out


def box(x):
    """mean of pixels (2i, 2j) .. (2i+1, 2j+1); an odd last row / column is dropped"""
    h2, w2 = x.shape[1] // 2, x.shape[2] // 2
    x = x[:, :2 * h2, :2 * w2]
    return 0.25 * (x[:, 0::2, 0::2] + x[:, 0::2, 1::2] + x[:, 1::2, 0::2] + x[:, 1::2, 1::2])


def down(x, kernel):
    return box(blur(x, kernel))


def axis(n_in, n_out):
    """-> i0, i1 (int), lam (float64) of every output index"""
    d = np.arange(n_out, dtype=np.float64)
    s = np.maximum((d + 0.5) * n_in / n_out - 0.5, 0.0)
    i0 = np.floor(s).astype(np.int64)
    i0 = np.minimum(i0, n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, s - i0


def up(x, size):
    x = np.asarray(x, np.float64)
    H, W = size
    y0, y1, ly = axis(x.shape[1], H)
    x0, x1, lx = axis(x.shape[2], W)
    lx = lx[None, None, :, None]
    ly = ly[None, :, None, None]
    top = (1 - lx) * x[:, y0][:, :, x0] + lx * x[:, y0][:, :, x1]
    bot = (1 - lx) * x[:, y1][:, :, x0] + lx * x[:, y1][:, :, x1]
    return (1 - ly) * top + ly * bot


def up_adjoint(g, size):
    """transpose of up: g [N,H,W,C] -> [N,h,w,C], scatter form"""
    g = np.asarray(g, np.float64)
    h, w = size
    n, H, W, c = g.shape
    y0, y1, ly = axis(h, H)
    x0, x1, lx = axis(w, W)
    rows = np.zeros((n, h, W, c))
    np.add.at(rows, (slice(None), y0), g * (1 - ly)[None, :, None, None])
    np.add.at(rows, (slice(None), y1), g * ly[None, :, None, None])
    out = np.zeros((n, h, w, c))
    np.add.at(out, (slice(None), slice(None), x0), rows * (1 - lx)[None, None, :, None])
    np.add.at(out, (slice(None), slice(None), x1), rows * lx[None, None, :, None])
    return out


def generate(x, levels=4, kernel_size=3, sigma=1.0):
    x = np.asarray(x, np.float64)
    k = gaussian_kernel(kernel_size, sigma)
    g = [x]
    for _ in range(levels - 1):
        g.append(down(g[-1], k))
    return [g[i] - up(g[i + 1], g[i].shape[1:3]) for i in range(levels - 1)] + [g[-1]]


def reconstruct(pyr):
    r = np.asarray(pyr[-1], np.float64)
    for i in range(len(pyr) - 2, -1, -1):
        r = up(r, pyr[i].shape[1:3]) + np.asarray(pyr[i], np.float64)
    return r


def reconstruct_adjoint(g, sizes):
    """gradients of sum(reconstruct(pyr) * g) with respect to every level; sizes = [(h_l, w_l)]"""
    out = [np.asarray(g, np.float64)]
    for i in range(1, len(sizes)):
        out.append(up_adjoint(out[-1], sizes[i]))
    return out
