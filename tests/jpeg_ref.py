"""Helper of the JPEG tests: the numpy statement of libjpeg's default decode after the entropy stage - dequantise, the "islow"
inverse DCT, the "fancy" chroma up-sampling, YCbCr -> RGB - from coefficient planes laid out as swnerf_jpeg_entropy writes them.
int32 arrays wrap as the C code's unsigned arithmetic does.  tests/test_jpeg_host.py checks it against g19_jpeg.npz."""
import numpy as np

I32 = np.int32


def _idct_1d(i, shift):
    c = lambda v: I32(v)
    z1 = (i[2] + i[6]) * c(4433)
    t2, t3 = z1 - i[6] * c(15137), z1 + i[2] * c(6270)
    t0, t1 = (i[0] + i[4]) << c(13), (i[0] - i[4]) << c(13)
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o0, o1, o2, o3 = i[7], i[5], i[3], i[1]
    z1, z2, z3, z4 = o0 + o3, o1 + o2, o0 + o2, o1 + o3
    z5 = (z3 + z4) * c(9633)
    o0, o1, o2, o3 = o0 * c(2446), o1 * c(16819), o2 * c(25172), o3 * c(12299)
    z1, z2, z3, z4 = z1 * c(-7373), z2 * c(-20995), z3 * c(-16069) + z5, z4 * c(-3196) + z5
    o0, o1, o2, o3 = o0 + z1 + z3, o1 + z2 + z4, o2 + z2 + z3, o3 + z1 + z4
    outs = [t10 + o3, t11 + o2, t12 + o1, t13 + o0, t13 - o0, t12 - o1, t11 - o2, t10 - o3]
    return [(x + c(1 << (shift - 1))) >> c(shift) for x in outs]


def plane(coef, q, by, bx):
    """coef int16 [by * bx * 64], q [64] -> uint8-valued int32 [by * 8, bx * 8]"""
    with np.errstate(over="ignore"):
        v = (coef.astype(I32).reshape(-1, 64) * np.asarray(q).astype(I32)[None, :]).reshape(by, bx, 8, 8)
        cols = np.stack(_idct_1d([v[:, :, r, :] for r in range(8)], 11), 2)                      # [by, bx, 8 rows, 8]
        rows = np.stack(_idct_1d([cols[:, :, :, c] for c in range(8)], 18), 3)
    return np.clip(rows + 128, 0, 255).transpose(0, 2, 1, 3).reshape(by * 8, bx * 8)


def _up_h(P):
    """[rows, dw] -> [rows, 2 dw], the 2:1 triangle filter along a row (replication at dw <= 2)"""
    dw = P.shape[1]
    if dw <= 2:
        return np.repeat(P, 2, 1)
    out = np.empty((P.shape[0], 2 * dw), I32)
    out[:, 2::2] = (3 * P[:, 1:] + P[:, :-1] + 1) >> 2
    out[:, 1:-1:2] = (3 * P[:, :-1] + P[:, 1:] + 2) >> 2
    out[:, 0], out[:, -1] = P[:, 0], P[:, -1]
    return out


def _up_hv(P):
    """[dh, dw] -> [2 dh, 2 dw]"""
    dh, dw = P.shape
    if dw <= 2:
        return np.repeat(np.repeat(P, 2, 0), 2, 1)
    out = np.empty((2 * dh, 2 * dw), I32)
    for y in range(2 * dh):
        r = y >> 1
        far = (r + 1 if r < dh - 1 else r) if y & 1 else (r - 1 if r > 0 else r)
        s = 3 * P[r] + P[far]
        out[y, 2::2] = (3 * s[1:] + s[:-1] + 8) >> 4
        out[y, 1:-1:2] = (3 * s[:-1] + s[1:] + 7) >> 4
        out[y, 0], out[y, -1] = (4 * s[0] + 8) >> 4, (4 * s[-1] + 7) >> 4
    return out


def decode(coef, qt, H, W, ncomp, sampling):
    """coef int16 [jpeg_coef_count], qt [ncomp, 64], sampling 0 / 1 / 2 (4:4:4, 4:2:2, 4:2:0) -> uint8 [H, W, 3]"""
    qt = np.asarray(qt).reshape(ncomp, 64)
    hs, vs = (2 if ncomp == 3 and sampling else 1), (2 if ncomp == 3 and sampling == 2 else 1)
    mx, my = -(-W // (8 * hs)), -(-H // (8 * vs))
    n0 = mx * hs * my * vs * 64
    Y = plane(coef[:n0], qt[0], my * vs, mx * hs)[:H, :W]
    if ncomp == 1:
        return np.repeat(Y[..., None], 3, -1).astype(np.uint8)
    dw, dh = -(-W // hs), -(-H // vs)
    chroma = []
    for c in (1, 2):
        P = plane(coef[n0 + (c - 1) * mx * my * 64:n0 + c * mx * my * 64], qt[c], my, mx)[:dh, :dw].astype(I32)
        P = P if sampling == 0 else _up_h(P) if sampling == 1 else _up_hv(P)
        chroma.append(P[:H, :W] - 128)
    cb, cr = chroma
    rgb = np.stack([Y + ((91881 * cr + 32768) >> 16), Y + ((-22554 * cb - 46802 * cr + 32768) >> 16), Y + ((116130 * cb + 32768) >> 16)], -1)
    return np.clip(rgb, 0, 255).astype(np.uint8)
