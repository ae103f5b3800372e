"""Helper of the image tests: the float64 numpy statement of the area mean that cv2.resize(..., INTER_AREA) defines for
down-scaling.  With sy = H / h, sx = W / w, destination pixel (i, j) weighs source cell (y, x) by
overlap([i sy, (i+1) sy), [y, y+1)) * overlap([j sx, (j+1) sx), [x, x+1)) / (sy sx)."""
import numpy as np


def to_float(u8):
    """bytes as the loaders and the batch kernel convert them: float32(u / 255.)"""
    return (np.asarray(u8).astype(np.float64) / 255.).astype(np.float32)


def axis_weights(n_dst, n_src):
    s = n_src / n_dst
    i, y = np.arange(n_dst, dtype=np.float64)[:, None], np.arange(n_src, dtype=np.float64)[None, :]
    return np.clip(np.minimum((i + 1) * s, y + 1) - np.maximum(i * s, y), 0., None) / s          # [n_dst, n_src], rows sum to 1


def area_mean(images, h, w):
    """images [N,H,W,c] float32 (or uint8: converted with to_float) -> float64 [N,h,w,c]"""
    x = np.asarray(images)
    x = (to_float(x) if x.dtype == np.uint8 else x).astype(np.float64)
    return np.einsum("iy,nyxc,jx->nijc", axis_weights(h, x.shape[1]), x, axis_weights(w, x.shape[2]), optimize=False)
