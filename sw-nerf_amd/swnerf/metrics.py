"""Image-quality metrics on the GPU: the evaluation step after render_path.

The reference scores a model two ways, and neither runs on this stack (skimage and lpips are not installed):
  - nerf/run.py:557-596 (`--render_only --render_test`) calls `calculate_metrics(gt, pred)` (:49-61) per test frame:
    np.clip(pred, 0, 1), data_range = gt.max() - gt.min(), skimage's `peak_signal_noise_ratio` and
    `structural_similarity(win_size=7, multichannel=True, channel_axis=2)`;
  - d_nerf/metrics.ipynb reads estim/*.png and gt/*.png, and scores the whole batch with its MSE / PSNR / SSIM classes
    (11x11 Gaussian window, population covariance, L from the prediction's range).
Both run here through one batched HIP entry point, swnerf_image_metrics: `image_metrics` is the batch interface,
`peak_signal_noise_ratio` / `structural_similarity` / `calculate_metrics` accept the reference's calls verbatim, and
`MSE` / `PSNR` / `SSIM` / `estim_error` mirror the notebook.  LPIPS (swnerf.lpips: the AlexNet / VGG16 trunks on HIP convolutions)
is computed when the caller supplies the two weight files it needs; this project ships none, and without a model
`calculate_metrics` returns None in its place and the dicts carry no 'lpips'."""
import math

import numpy as np
import torch

from . import _lib
from .lpips import LPIPS, LPIPS_notebook  # noqa: F401

MODES = {"skimage": _lib.SSIM_SKIMAGE, "gauss11": _lib.SSIM_GAUSS11}
WINDOW = {_lib.SSIM_SKIMAGE: 7, _lib.SSIM_GAUSS11: 11}
CHUNK_BYTES = 1 << 30                   # per operand and chunk: 200 frames of 800x800x3 go through in two chunks


def _mode(mode):
    if isinstance(mode, str):
        if mode not in MODES:
            raise ValueError(f"swnerf.metrics: mode must be one of {sorted(MODES)}, got {mode!r}")
        return MODES[mode]
    if mode not in WINDOW:
        raise ValueError(f"swnerf.metrics: unknown SSIM mode {mode!r}")
    return int(mode)


def _frames(a, name, layout):
    """-> (array or tensor, (N, H, W)); HWC [H,W,3] is one frame.  Host data stays where it is until its chunk is sent."""
    if isinstance(a, torch.Tensor):
        if a.is_complex() or not a.is_floating_point():
            raise NotImplementedError(f"swnerf.metrics: {name} must be floating point, got {a.dtype}")
    else:
        a = np.asarray(a)
        if a.dtype.kind != "f":
            raise NotImplementedError(f"swnerf.metrics: {name} must be floating point, got {a.dtype}")
    if a.ndim == 3:
        a = a[None]
    if a.ndim != 4:
        raise ValueError(f"swnerf.metrics: {name} must be [N,H,W,3] or [H,W,3], got shape {tuple(a.shape)}")
    c = a.shape[3] if layout == "nhwc" else a.shape[1]
    if c != 3:
        raise NotImplementedError(f"swnerf.metrics: {name} has {c} channels; only RGB (3) is built")
    n, h, w = (a.shape[0], a.shape[1], a.shape[2]) if layout == "nhwc" else (a.shape[0], a.shape[2], a.shape[3])
    return a, (n, h, w)


def _to_device(a, s, e, dev, layout):
    x = a[s:e]
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.ascontiguousarray(x))
    x = x.to(device=dev, dtype=torch.float32, non_blocking=False)
    if layout == "nchw":
        x = x.permute(0, 2, 3, 1)
    return x.contiguous()


def _device(pred, gt):
    for a in (pred, gt):
        if isinstance(a, torch.Tensor) and a.is_cuda:
            return a.device
    if not torch.cuda.is_available():
        raise RuntimeError("swnerf.metrics: no GPU - the metrics are HIP kernels with no CPU implementation")
    return torch.device("cuda", torch.cuda.current_device())


def _rule_parts(L):
    """the notebook's range L = max_val - min_val back to (max_val, min_val): 1 -> (1, 0), 2 -> (1, -1), 255, 256"""
    return (255.0 if L >= 255.0 else 1.0), (-1.0 if L in (2.0, 256.0) else 0.0)


def image_metrics(pred, gt, *, mode, data_range="gt", clip_pred=False, want_map=False, chunk_frames=None, _layout="nhwc"):
    """Per-frame MSE, PSNR and SSIM of pred against gt on the GPU.

    pred, gt: [N,H,W,3] or [H,W,3] float frames (numpy, CPU or CUDA tensors); host data is sent in chunks of
    `chunk_frames` frames (default: CHUNK_BYTES per operand).  mode: "skimage" (uniform 7x7 window, sample covariance:
    structural_similarity(win_size=7, channel_axis=2)) or "gauss11" (metrics.ipynb).  data_range: a number, "gt"
    (per frame gt.max() - gt.min()) or "pred_rule" (the notebook's rule over the whole batch of pred).  clip_pred clips
    pred to [0, 1] first.  -> dict of float64 CUDA tensors [N]: mse, psnr, range, ssim, and with want_map the per-pixel
    S [N, H-w+1, W-w+1, 3] float32 as "map"."""
    m = _mode(mode)
    pred, ps = _frames(pred, "pred", _layout)
    gt, gs = _frames(gt, "gt", _layout)
    if ps != gs:
        raise ValueError(f"swnerf.metrics: pred and gt differ in shape: {tuple(pred.shape)} vs {tuple(gt.shape)}")
    n, h, w = ps
    win = WINDOW[m]
    if h < win or w < win:
        raise ValueError(f"swnerf.metrics: a {h}x{w} image is smaller than the {win}x{win} SSIM window")
    if isinstance(data_range, str):
        if data_range not in ("gt", "pred_rule"):
            raise ValueError(f"swnerf.metrics: data_range must be a number, 'gt' or 'pred_rule', got {data_range!r}")
        rmode, fixed = (_lib.RANGE_GT if data_range == "gt" else _lib.RANGE_PRED_RULE), 0.0
    else:
        rmode, fixed = _lib.RANGE_FIXED, float(data_range)
    dev = _device(pred, gt)
    L = _lib.lib()
    f64 = dict(dtype=torch.float64, device=dev)
    out = {k: torch.empty(n, **f64) for k in ("mse", "psnr", "range", "ssim")}
    smap = torch.empty((n, h - win + 1, w - win + 1, 3), dtype=torch.float32, device=dev) if want_map else None
    if n == 0:
        if want_map:
            out["map"] = smap
        return out
    chunk = int(chunk_frames) if chunk_frames else max(1, CHUNK_BYTES // (h * w * 3 * 4))
    chunk = min(chunk, n)
    ws = torch.empty(max(1, L.swnerf_metrics_workspace_bytes(chunk, h, w, m)), dtype=torch.uint8, device=dev)
    spans = [(s, min(n, s + chunk)) for s in range(0, n, chunk)]

    def run(s, e, rm, fx):
        p, g = _to_device(pred, s, e, dev, _layout), _to_device(gt, s, e, dev, _layout)
        mp = None if smap is None else _lib.ptr(smap[s:e])
        _lib.check(L.swnerf_image_metrics(_lib.ptr(p), _lib.ptr(g), e - s, h, w, m, rm, fx, int(bool(clip_pred)),
                                          _lib.ptr(ws), _lib.ptr(out["mse"][s:e]), _lib.ptr(out["psnr"][s:e]),
                                          _lib.ptr(out["range"][s:e]), _lib.ptr(out["ssim"][s:e]), mp, _lib.stream_of(p)),
                   "image_metrics")

    for s, e in spans:
        run(s, e, rmode, fixed)
    if rmode == _lib.RANGE_PRED_RULE and len(spans) > 1:
        # the rule is over the whole batch: combine the per-chunk rules and redo the chunks that saw a different one
        per = [float(out["range"][s]) for s, _ in spans]
        hi = max(_rule_parts(r)[0] for r in per)
        lo = min(_rule_parts(r)[1] for r in per)
        for (s, e), r in zip(spans, per):
            if r != hi - lo:
                run(s, e, _lib.RANGE_FIXED, hi - lo)
    if want_map:
        out["map"] = smap
    return out


# ---- skimage.metrics, as nerf/run.py calls it ----------------------------------------------------------------------
def _hwc_pair(a, b, who):
    sa, sb = tuple(np.shape(a)), tuple(np.shape(b))
    if sa != sb:
        raise ValueError(f"swnerf.metrics.{who}: input images must have the same dimensions, got {sa} and {sb}")
    if len(sa) != 3:
        raise NotImplementedError(f"swnerf.metrics.{who}: only [H,W,3] images are built, got shape {sa}")


def peak_signal_noise_ratio(image_true, image_test, *, data_range=None):
    """skimage.metrics.peak_signal_noise_ratio for [H,W,3] float images: 10 log10(data_range^2 / MSE)."""
    _hwc_pair(image_true, image_test, "peak_signal_noise_ratio")
    if data_range is None:
        raise ValueError("swnerf.metrics.peak_signal_noise_ratio: float images need an explicit data_range")
    r = image_metrics(image_test, image_true, mode="skimage", data_range=float(data_range))
    return np.float64(r["psnr"][0].item())


def structural_similarity(im1, im2, *, win_size=None, gradient=False, data_range=None, channel_axis=None,
                          gaussian_weights=False, full=False, **kwargs):
    """skimage.metrics.structural_similarity for [H,W,3] float images with channel_axis=2 (or -1), the 7x7 uniform
    window and the sample covariance - what nerf/run.py:57 asks for.  `multichannel=True` (which recent skimage ignores
    next to channel_axis) is accepted.  Other options raise NotImplementedError."""
    multichannel = kwargs.pop("multichannel", None)
    K1, K2 = kwargs.pop("K1", 0.01), kwargs.pop("K2", 0.03)
    sample_cov = kwargs.pop("use_sample_covariance", True)
    if kwargs:
        raise NotImplementedError(f"swnerf.metrics.structural_similarity: options {sorted(kwargs)} are not built")
    if win_size not in (None, 7):
        raise NotImplementedError(f"swnerf.metrics.structural_similarity: win_size={win_size}; only 7 is built")
    if gaussian_weights or gradient or full:
        raise NotImplementedError("swnerf.metrics.structural_similarity: gaussian_weights, gradient and full are not built")
    if K1 != 0.01 or K2 != 0.03 or not sample_cov:
        raise NotImplementedError("swnerf.metrics.structural_similarity: only K1=0.01, K2=0.03, use_sample_covariance=True")
    if channel_axis is None and multichannel:
        channel_axis = -1
    if channel_axis not in (2, -1):
        raise NotImplementedError(f"swnerf.metrics.structural_similarity: channel_axis={channel_axis}; only HWC (2) is built")
    _hwc_pair(im1, im2, "structural_similarity")
    if data_range is None:
        raise ValueError("swnerf.metrics.structural_similarity: float images need an explicit data_range")
    r = image_metrics(im2, im1, mode="skimage", data_range=float(data_range))
    return np.float64(r["ssim"][0].item())


def _lpips_gt_pred(lpips_model, gts, preds):
    """the reference's call, nerf/run.py:59-60: lpips_model(gt, np.clip(pred, 0, 1)) on [0, 1] values with the package's default
    normalize=False - the reference does NOT map them to the [-1, 1] the network was trained on; mirrored as it is"""
    if isinstance(preds, torch.Tensor):
        preds = preds.clamp(0.0, 1.0)
    else:
        preds = np.clip(np.asarray(preds), 0.0, 1.0)
    return lpips_model(gts, preds, normalize=False, layout="nhwc")


def calculate_metrics(gt, pred, lpips_model=None):
    """nerf/run.py:49-61: (psnr, ssim, lpips) of one [H,W,3] frame, pred clipped to [0, 1], data_range = gt.max() - gt.min().
    lpips_model: a metrics.LPIPS (the reference builds net='alex'); the third value is then its [1,1,1,1] tensor for
    (gt, clipped pred), passed as the reference passes them: [0, 1] values with normalize=False.  Without a model it is None."""
    _hwc_pair(gt, pred, "calculate_metrics")
    r = image_metrics(pred, gt, mode="skimage", data_range="gt", clip_pred=True)
    lp = None if lpips_model is None else _lpips_gt_pred(lpips_model, gt, pred)
    return np.float64(r["psnr"][0].item()), np.float64(r["ssim"][0].item()), lp


def batch_metrics(gts, preds, lpips_model=None):
    """calculate_metrics over a batch of frames in one call: -> (psnr list, ssim list) of Python floats, and with a
    lpips_model a third list, the LPIPS of every (gt, clipped pred) pair."""
    r = image_metrics(preds, gts, mode="skimage", data_range="gt", clip_pred=True)
    if lpips_model is None:
        return r["psnr"].cpu().tolist(), r["ssim"].cpu().tolist()
    lp = _lpips_gt_pred(lpips_model, gts, preds)
    return r["psnr"].cpu().tolist(), r["ssim"].cpu().tolist(), lp.reshape(-1).cpu().tolist()


# ---- d_nerf/metrics.ipynb: NCHW batches, (pred, gt) order -----------------------------------------------------------
def _nchw(pred, gt):
    return image_metrics(pred, gt, mode="gauss11", data_range="pred_rule", _layout="nchw")


class MSE(object):
    """mean((pred - gt)^2) over the batch (equal-size frames: the mean of the per-frame MSEs), a 0-d float64 tensor"""
    def __call__(self, pred, gt):
        return _nchw(pred, gt)["mse"].mean()


class PSNR(object):
    """10 log10(1 / MSE) of the batch"""
    def __call__(self, pred, gt):
        return 10 * torch.log10(1 / _nchw(pred, gt)["mse"].mean())


class SSIM(object):
    """the notebook's SSIM: 11x11 Gaussian window (sigma 1.5), population covariance over valid windows,
    L = (255 if max(pred) > 128 else 1) - (-1 if min(pred) < -0.5 else 0); size_average=False gives one value per frame"""
    def __call__(self, y_pred, y_true, w_size=11, size_average=True, full=False):
        if w_size != 11 or full:
            raise NotImplementedError("swnerf.metrics.SSIM: only w_size=11 and full=False are built")
        s = _nchw(y_pred, y_true)["ssim"]
        return s.mean() if size_average else s


def estim_error(estim, gt, lpips_model=None):
    """the notebook's estim_error: {'mse', 'psnr', 'ssim'} of NCHW batches, one kernel pass; with a lpips_model (an
    LPIPS_notebook, or a metrics.LPIPS, which is then called as the notebook's class calls it) also 'lpips'"""
    r = _nchw(estim, gt)
    mse = float(r["mse"].mean())
    errors = {"mse": mse, "psnr": 10 * math.log10(1 / mse) if mse != 0 else math.inf, "ssim": float(r["ssim"].mean())}
    if lpips_model is not None:
        lp = torch.mean(lpips_model(estim, gt, normalize=True)) if isinstance(lpips_model, LPIPS) else lpips_model(estim, gt)
        errors["lpips"] = float(lp)
    return errors
