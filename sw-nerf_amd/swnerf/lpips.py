"""LPIPS v0.1 on the GPU (DESIGN.md 6f "LPIPS"): the third number of the reference's result tables.

nerf/run.py:49-61 builds `lpips.LPIPS(net='alex')`, d_nerf/metrics.ipynb `lpips.LPIPS(net='vgg')`; the package is not on this
stack and is not needed: the metric is a fixed small CNN.  The trunk (torchvision's AlexNet / VGG16 `features`) runs on the HIP
implicit-GEMM convolution and pooling kernels, each tap on the fused normalise / difference / 1x1 / spatial-mean kernel
(csrc/lpips_kernels.hip).  The weights are the two ordinary state-dict files the user already has - torchvision's trunk
checkpoint and the package's five 1x1 "lin" layers; nothing is ever fetched.  No CPU path, no autograd."""
import glob
import os

import numpy as np
import torch

from . import _lib, packing

SHIFT = (-.030, -.088, -.188)          # the package's ScalingLayer
SCALE = (.458, .448, .450)
CHUNK_BYTES = 1 << 30                  # live activations per chunk of frame pairs

# (features index, cin, cout, kernel, stride, pad); taps are the ReLU outputs of the listed positions
CONVS = {
    "alex": [(0, 3, 64, 11, 4, 2), (3, 64, 192, 5, 1, 2), (6, 192, 384, 3, 1, 1), (8, 384, 256, 3, 1, 1), (10, 256, 256, 3, 1, 1)],
    "vgg": [(i, ci, co, 3, 1, 1) for i, ci, co in (
        (0, 3, 64), (2, 64, 64), (5, 64, 128), (7, 128, 128), (10, 128, 256), (12, 256, 256), (14, 256, 256),
        (17, 256, 512), (19, 512, 512), (21, 512, 512), (24, 512, 512), (26, 512, 512), (28, 512, 512))],
}
TAPS = {"alex": (0, 1, 2, 3, 4), "vgg": (1, 3, 6, 9, 12)}                 # conv positions whose ReLU output is a tap
POOL_BEFORE = {"alex": {1: 3, 2: 3}, "vgg": {2: 2, 4: 2, 7: 2, 10: 2}}      # conv position -> pooling window in front of it
TRUNK_FILES = {"alex": "alexnet*.pth", "vgg": "vgg16*.pth"}
TRUNK_NAMES = {"alex": "alexnet-owt-7be5be79.pth", "vgg": "vgg16-397923af.pth"}


def tap_channels(net):
    return [CONVS[net][p][2] for p in TAPS[net]]


def _wanted(net):
    return (f"swnerf.metrics.LPIPS(net={net!r}) needs two weight files and fetches nothing: (1) torchvision's trunk checkpoint "
            f"{TRUNK_NAMES[net]} (normally under ~/.cache/torch/hub/checkpoints), keys features.N.weight / .bias; (2) the lpips "
            f"package's linear layers lpips/weights/v0.1/{net}.pth (in its site-packages directory), keys lin0..4.model.1.weight.  "
            f"Pass weights=(trunk, lin) as state dicts or paths, or a directory holding {TRUNK_FILES[net]} and {net}.pth, or set "
            "SWNERF_LPIPS_DIR (or args.lpips_weights) to such a directory.")


def _state_dict(x, what):
    if isinstance(x, (str, os.PathLike)):
        if not os.path.isfile(x):
            raise FileNotFoundError(f"swnerf.metrics.LPIPS: {what} file {os.fspath(x)!r} not found")
        x = torch.load(x, map_location="cpu", weights_only=True)
    if not hasattr(x, "keys"):
        raise TypeError(f"swnerf.metrics.LPIPS: {what} must be a state dict or a path, got {type(x).__name__}")
    return x


def _tensor(sd, key, shape):
    if key not in sd:
        raise ValueError(f"swnerf.metrics.LPIPS: key {key!r} is missing")
    t = torch.as_tensor(sd[key])
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"swnerf.metrics.LPIPS: {key!r} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    return t.detach().to(torch.float32).contiguous()


def load_weights(net, weights=None, args=None):
    """-> (convs [(weight [cout,cin,k,k], bias [cout])], lins [[C]]) as float32 CPU tensors, validated key by key.
    weights: (trunk, lin), each a state dict or a path, or a directory; absent: $SWNERF_LPIPS_DIR, then args.lpips_weights."""
    if net not in CONVS:
        raise ValueError(f"swnerf.metrics.LPIPS: net must be 'alex' or 'vgg', got {net!r} (squeeze / vgg19 / resnet are not built)")
    if weights is None:
        weights = os.environ.get("SWNERF_LPIPS_DIR") or getattr(args, "lpips_weights", None)
    if weights is None:
        raise FileNotFoundError(_wanted(net))
    if isinstance(weights, (str, os.PathLike)):
        d = os.fspath(weights)
        trunks = sorted(glob.glob(os.path.join(d, TRUNK_FILES[net])))
        lin = os.path.join(d, f"{net}.pth")
        if not os.path.isdir(d) or not trunks or not os.path.isfile(lin):
            raise FileNotFoundError(f"no {TRUNK_FILES[net]} and {net}.pth in {d!r}.  " + _wanted(net))
        weights = (trunks[0], lin)
    if not isinstance(weights, (tuple, list)) or len(weights) != 2:
        raise TypeError("swnerf.metrics.LPIPS: weights must be (trunk, lin) or a directory")
    trunk, lin = _state_dict(weights[0], "trunk"), _state_dict(weights[1], "lin")
    convs = [(_tensor(trunk, f"features.{i}.weight", (co, ci, k, k)), _tensor(trunk, f"features.{i}.bias", (co,)))
             for i, ci, co, k, _, _ in CONVS[net]]
    lins = [_tensor(lin, f"lin{j}.model.1.weight", (1, c, 1, 1)).reshape(c) for j, c in enumerate(tap_channels(net))]
    return convs, lins


# ---- the three kernels ------------------------------------------------------------------------------------------------
def conv_out(h, k, s, p):
    return (h + 2 * p - k) // s + 1


def pack_conv_weight(cache, slot, weight):
    """weight [cout, cin, k, k] on the GPU -> the [k*k*cin, cout] stream of swnerf_conv2d_nhwc, through the weight-pack cache"""
    co, ci, k, k2 = weight.shape
    if k != k2:
        raise ValueError(f"swnerf.lpips: only square kernels are built, got {k}x{k2}")
    return packing.pack_weights(cache, slot, [weight], lambda L: weight.numel(),
                                lambda L, arr, blob, st: L.swnerf_conv2d_pack(arr[0], co, ci, k, blob, st), "conv2d_pack")


def conv2d_nhwc(x, packed, bias, cout, ksz, stride=1, pad=0, relu=False):
    """x [N,H,W,Cin] float32 CUDA, packed from pack_conv_weight -> act(conv + bias) [N,Ho,Wo,cout]"""
    x = _lib.dev_f32(x, "x")
    n, h, w, cin = x.shape
    ho, wo = conv_out(h, ksz, stride, pad), conv_out(w, ksz, stride, pad)
    out = torch.empty((n, max(ho, 0), max(wo, 0), cout), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().swnerf_conv2d_nhwc(_lib.ptr(x), n, h, w, cin, _lib.ptr(packed), _lib.ptr(bias), cout, ksz, stride, pad,
                                             _lib.ACT_RELU if relu else _lib.ACT_NONE, _lib.ptr(out), _lib.stream_of(x)), "conv2d_nhwc")
    return out


def maxpool2d_nhwc(x, window):
    """x [N,H,W,C] -> torch.max_pool2d(kernel_size=window, stride=2) of it, NHWC"""
    x = _lib.dev_f32(x, "x")
    n, h, w, c = x.shape
    out = torch.empty((n, max((h - window) // 2 + 1, 0), max((w - window) // 2 + 1, 0), c), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().swnerf_maxpool2d_nhwc(_lib.ptr(x), n, h, w, c, window, _lib.ptr(out), _lib.stream_of(x)), "maxpool2d_nhwc")
    return out


def lpips_layer(f0, f1, lin, out=None, accumulate=False, want_map=False):
    """One tap: f0, f1 [N,h,w,C], lin [C] -> float64 [N] (added to `out` with accumulate); with want_map also the per-pixel
    values [N,h,w] float32."""
    f0, f1, lin = _lib.dev_f32(f0, "f0"), _lib.dev_f32(f1, "f1"), _lib.dev_f32(lin, "lin")
    if f0.shape != f1.shape or f0.ndim != 4 or lin.numel() != f0.shape[3]:
        raise ValueError(f"swnerf.lpips.lpips_layer: shapes {tuple(f0.shape)}, {tuple(f1.shape)}, {tuple(lin.shape)} do not fit")
    n, h, w, c = f0.shape
    L = _lib.lib()
    if out is None:
        out, accumulate = torch.zeros(n, dtype=torch.float64, device=f0.device), False
    ws = torch.empty(max(8, L.swnerf_lpips_layer_workspace_bytes(n, h, w)), dtype=torch.uint8, device=f0.device)
    mp = torch.empty((n, h, w), dtype=torch.float32, device=f0.device) if want_map else None
    _lib.check(L.swnerf_lpips_layer(_lib.ptr(f0), _lib.ptr(f1), _lib.ptr(lin), n, h, w, c, int(bool(accumulate)), _lib.ptr(ws),
                                    _lib.ptr(out), _lib.ptr(mp), _lib.stream_of(f0)), "lpips_layer")
    return (out, mp) if want_map else out


# ---- the metric -------------------------------------------------------------------------------------------------------
def _frames(a, name, layout):
    if not isinstance(a, torch.Tensor):
        a = np.asarray(a)
        if a.dtype.kind not in "fu":
            raise NotImplementedError(f"swnerf.metrics.LPIPS: {name} must be floating point or uint8, got {a.dtype}")
    elif not (a.is_floating_point() or a.dtype == torch.uint8):
        raise NotImplementedError(f"swnerf.metrics.LPIPS: {name} must be floating point or uint8, got {a.dtype}")
    if a.ndim == 3:
        a = a[None]
    if a.ndim != 4:
        raise ValueError(f"swnerf.metrics.LPIPS: {name} must be 4-d ({layout}) or one 3-d frame, got shape {tuple(a.shape)}")
    n, h, w, c = a.shape if layout == "nhwc" else (a.shape[0], a.shape[2], a.shape[3], a.shape[1])
    if c != 3:
        raise ValueError(f"swnerf.metrics.LPIPS: {name} has {c} channels in layout {layout!r}; RGB (3) is wanted")
    return a, (n, h, w)


def _to_device(a, s, e, dev, layout):
    """frames s..e-1 as [m,H,W,3] float32 on the device; bytes are divided by 255"""
    x = a[s:e]
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.ascontiguousarray(x))
    u8 = x.dtype == torch.uint8
    x = x.to(device=dev, dtype=torch.float32)
    if u8:
        x = x / 255.
    if layout == "nchw":
        x = x.permute(0, 2, 3, 1)
    return x


class LPIPS(object):
    """lpips.LPIPS(net=..., version='0.1', spatial=False) in eval mode: model(in0, in1, normalize=False) -> [N,1,1,1] float32.

    weights: see load_weights.  Parameters live on `device` (default: the current GPU); inputs on the CPU are uploaded chunk
    by chunk.  Both images of a pair go through the trunk as one batch, so every weight tile is read once."""

    def __init__(self, net="alex", weights=None, device=None, args=None):
        convs, lins = load_weights(net, weights, args)
        self.net = net
        self._cpu = (convs, lins)
        self._dev = None
        self._packs = {}                                                   # the weight-pack cache (packing.py) of this model
        self.device = None if device is None else torch.device(device)
        if self.device is not None or torch.cuda.is_available():
            self._params()

    def _params(self):
        if self._dev is None:
            if not torch.cuda.is_available():
                raise RuntimeError("swnerf.metrics.LPIPS: no GPU - LPIPS runs on HIP kernels with no CPU implementation")
            if self.device is None:
                self.device = torch.device("cuda", torch.cuda.current_device())
            if self.device.type != "cuda":
                raise RuntimeError(f"swnerf.metrics.LPIPS: device must be a GPU, got {self.device}")
            convs, lins = self._cpu
            self._dev = ([(w.to(self.device), b.to(self.device)) for w, b in convs], [l.to(self.device) for l in lins],
                         torch.tensor(SHIFT, dtype=torch.float32, device=self.device),
                         torch.tensor(SCALE, dtype=torch.float32, device=self.device))
        return self._dev

    def live_bytes(self, h, w):
        """the largest input + output of one trunk step for ONE frame pair (two images)"""
        c, worst = 3, 0
        for pos, (_, _, co, k, s, p) in enumerate(CONVS[self.net]):
            win = POOL_BEFORE[self.net].get(pos)
            if win:
                h2, w2 = (h - win) // 2 + 1, (w - win) // 2 + 1
                worst = max(worst, (h * w + h2 * w2) * c)
                h, w = h2, w2
            h2, w2 = conv_out(h, k, s, p), conv_out(w, k, s, p)
            worst = max(worst, h * w * c + h2 * w2 * co)
            h, w, c = h2, w2, co
        return 2 * 4 * worst

    def features(self, x):
        """x [M,H,W,3] scaled input on the device -> the five tap feature maps, NHWC"""
        convs = self._params()[0]
        taps = []
        for pos, (_, _, co, k, s, p) in enumerate(CONVS[self.net]):
            win = POOL_BEFORE[self.net].get(pos)
            if win:
                x = maxpool2d_nhwc(x, win)
            w, b = convs[pos]
            x = conv2d_nhwc(x, pack_conv_weight(self._packs, pos, w), b, co, k, s, p, relu=True)
            if pos in TAPS[self.net]:
                taps.append(x)
        return taps

    def __call__(self, pred, gt, normalize=False, layout="nchw", chunk_frames=None):
        if layout not in ("nchw", "nhwc"):
            raise ValueError(f"swnerf.metrics.LPIPS: layout must be 'nchw' or 'nhwc', got {layout!r}")
        pred, ps = _frames(pred, "pred", layout)
        gt, gs = _frames(gt, "gt", layout)
        if ps != gs:
            raise ValueError(f"swnerf.metrics.LPIPS: the two inputs differ in shape: {tuple(pred.shape)} vs {tuple(gt.shape)}")
        n, h, w = ps
        _, lins, shift, scale = self._params()
        total = torch.zeros(n, dtype=torch.float64, device=self.device)
        chunk = int(chunk_frames) if chunk_frames else max(1, CHUNK_BYTES // max(1, self.live_bytes(h, w)))
        with torch.no_grad():
            for s in range(0, n, chunk):
                e = min(n, s + chunk)
                x = torch.cat([_to_device(pred, s, e, self.device, layout), _to_device(gt, s, e, self.device, layout)])
                if normalize:
                    x = 2 * x - 1
                x = ((x - shift) / scale).contiguous()
                for j, f in enumerate(self.features(x)):
                    lpips_layer(f[:e - s], f[e - s:], lins[j], out=total[s:e], accumulate=j > 0)
        return total.to(torch.float32).view(n, 1, 1, 1)

    forward = __call__


class LPIPS_notebook(object):
    """the LPIPS class of d_nerf/metrics.ipynb: the VGG trunk, NCHW inputs in [0, 1] mapped to [-1, 1] (normalized=True),
    torch.mean over the batch -> a 0-d tensor"""

    def __init__(self, weights=None, device=None, args=None):
        self.model = LPIPS("vgg", weights=weights, device=device, args=args)

    def __call__(self, y_pred, y_true, normalized=True):
        return torch.mean(self.model(y_pred, y_true, normalize=bool(normalized)))
