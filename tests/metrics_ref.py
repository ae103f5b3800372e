"""float64 numpy restatement of the image metrics (swnerf.metrics / metrics_kernels.hip) for the tests: explicit windows
through sliding_window_view, not the kernel's separable order.
  mode 0 (skimage structural_similarity, win_size=7, channel_axis=2): uniform 7x7 mean, sample covariance (x 49/48),
         the mean of S over the pixels whose window lies inside the image (= skimage's crop by 3)
  mode 1 (d_nerf/metrics.ipynb SSIM): 11x11 Gaussian (sigma 1.5, normalised 1-D weights, outer product), population
         covariance, valid windows (conv2d without padding)"""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

SKIMAGE, GAUSS11 = 0, 1


def gauss_weights(w=11, sigma=1.5):
    g = np.exp(-((np.arange(w) - w // 2) ** 2) / (2.0 * sigma ** 2))
    return g / g.sum()


def window(mode):
    if mode == SKIMAGE:
        return np.full((7, 7), 1.0 / 49.0), 49.0 / 48.0
    g = gauss_weights()
    return np.outer(g, g), 1.0


def ssim_map(pred, gt, mode, R):
    """pred, gt [H,W,3] -> S [H-w+1, W-w+1, 3] float64"""
    x, y = np.asarray(pred, np.float64), np.asarray(gt, np.float64)
    W2, cov = window(mode)
    k = W2.shape[0]

    def filt(a):
        return np.einsum("hwcij,ij->hwc", sliding_window_view(a, (k, k), axis=(0, 1)), W2)
    ux, uy = filt(x), filt(y)
    vx = cov * (filt(x * x) - ux * ux)
    vy = cov * (filt(y * y) - uy * uy)
    vxy = cov * (filt(x * y) - ux * uy)
    R = float(R)
    C1, C2 = (0.01 * R) ** 2, (0.03 * R) ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        A1, A2 = 2 * ux * uy + C1, 2 * vxy + C2
        B1, B2 = ux ** 2 + uy ** 2 + C1, vx + vy + C2
        return (A1 * A2) / (B1 * B2)


def ssim(pred, gt, mode, R):
    return float(ssim_map(pred, gt, mode, R).mean())


def mse(pred, gt):
    """squared float32 differences, averaged in float64 (skimage's mean_squared_error of float32 images)"""
    d = (np.asarray(pred, np.float32) - np.asarray(gt, np.float32)).astype(np.float64)
    return float(np.mean(d * d))


def psnr(m, R):
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(10 * np.log10(np.float64(R) ** 2 / np.float64(m)))


def gt_range(gt):
    g = np.asarray(gt, np.float32)
    return float(g.max() - g.min())                                # a float32 difference, as nerf/run.py:56


def pred_rule(preds):
    p = np.asarray(preds, np.float32)
    mx, mn = p.max(), p.min()
    return (255.0 if mx > 128 else 1.0) - (-1.0 if mn < -0.5 else 0.0)


def batch(preds, gts, mode, data_range="gt", clip_pred=False):
    """-> dict of float64 arrays [N]: mse, psnr, range, ssim (what swnerf.metrics.image_metrics returns)"""
    preds = np.asarray(preds, np.float32)
    gts = np.asarray(gts, np.float32)
    if clip_pred:
        preds = np.clip(preds, 0.0, 1.0)
    out = {k: [] for k in ("mse", "psnr", "range", "ssim")}
    rule = pred_rule(preds) if data_range == "pred_rule" else None
    for p, g in zip(preds, gts):
        R = gt_range(g) if data_range == "gt" else (rule if rule is not None else float(data_range))
        m = mse(p, g)
        out["mse"].append(m)
        out["range"].append(R)
        out["psnr"].append(psnr(m, R))
        out["ssim"].append(ssim(p, g, mode, R))
    return {k: np.array(v, np.float64) for k, v in out.items()}
