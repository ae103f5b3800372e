"""2-D image fitting (the reference's 2d_pos_encoding/: model.py, encoding.py, utils.py) on the HIP kernels of
csrc/fit2d_kernels.hip.  `Model` is 10 x (Linear -> ReLU -> BatchNorm1d) at width 256 and Linear(256, 3) on encode(pos, L).

Training runs layer by layer: generic.linear, then `_ReluBN` (swnerf_bn_forward_train / swnerf_bn_backward with the ReLU
in front).  There is no fused training pass: batch statistics couple all rows of a batch at every layer.  Eval mode at
hidden_dim 256 / output_dim 3 / input_dimension 4L + 2 (L <= 23) is one fused launch with every BatchNorm1d folded into the
next Linear (swnerf_pack_fit2d, swnerf_fit2d_forward / swnerf_fit2d_picture); any other eval shape runs layer by layer
(linear with the ReLU epilogue, then swnerf_bn_apply).  Parameters on the CPU are an error: there is no CPU fallback.
ExponentialLR stays torch's, and AdamW by default (runner.create_fit2d with args.optimizer = "fused": swnerf.optim.AdamW)."""
import os
import time

import numpy as np
import torch
import torch.nn as nn

from . import _lib, generic, packing
from .png import write_png

MAX_L = 23
MAX_FUSED_LAYERS = 64
BATCH = 512


def _need_cuda(t, what):
    if not t.is_cuda:
        raise RuntimeError(f"swnerf.fit2d: {what} must be on the GPU (call .to('cuda')); there is no CPU fallback")


def _bn_ws(M, C, device):
    n = _lib.lib().swnerf_bn_workspace_bytes(M, C)
    return torch.empty((n // 8,), dtype=torch.float64, device=device) if n else None


class _ReluBN(torch.autograd.Function):
    """BatchNorm1d(relu(a)) in training mode.  The running buffers are written by the kernel through raw pointers."""

    @staticmethod
    def forward(ctx, a, weight, bias, running_mean, running_var, eps, momentum, relu):
        L = _lib.lib()
        M, C = a.shape
        y = torch.empty_like(a)
        mean = torch.empty((C,), dtype=torch.float32, device=a.device)
        invstd = torch.empty_like(mean)
        _lib.check(L.swnerf_bn_forward_train(_lib.ptr(a), M, C, int(relu), _lib.ptr(weight), _lib.ptr(bias), eps, momentum, _lib.ptr(y),
                                             _lib.ptr(mean), _lib.ptr(invstd), _lib.ptr(running_mean), _lib.ptr(running_var),
                                             _lib.ptr(_bn_ws(M, C, a.device)), _lib.stream_of(a)), "bn_forward_train")
        ctx.relu = bool(relu)
        ctx.save_for_backward(a, weight, mean, invstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        a, weight, mean, invstd = ctx.saved_tensors
        L = _lib.lib()
        M, C = a.shape
        dy = generic._c32(dy)
        dx = torch.empty_like(a)
        dg = torch.empty((C,), dtype=torch.float32, device=a.device)
        db = torch.empty_like(dg)
        _lib.check(L.swnerf_bn_backward(_lib.ptr(dy), _lib.ptr(a), M, C, int(ctx.relu), _lib.ptr(weight), _lib.ptr(mean), _lib.ptr(invstd),
                                        _lib.ptr(dx), _lib.ptr(dg), _lib.ptr(db), _lib.ptr(_bn_ws(M, C, a.device)), _lib.stream_of(a)),
                   "bn_backward")
        return dx, dg, db, None, None, None, None, None


def relu_batch_norm(a, bn, relu=True):
    """`bn` (nn.BatchNorm1d, training mode) applied to relu(a) - or to a when relu is False - by the HIP kernels, differentiable.
    Updates bn.running_mean / running_var / num_batches_tracked like torch."""
    a = _lib.dev_f32(a, "a", bn.num_features)
    if a.dim() != 2:
        raise ValueError(f"swnerf.fit2d: BatchNorm1d input must be [M, C], got {tuple(a.shape)}")
    _need_cuda(bn.weight, "BatchNorm1d parameters")
    if a.shape[0] < 2:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(a.shape)}")
    if bn.momentum is None:
        raise NotImplementedError("swnerf.fit2d: BatchNorm1d(momentum=None) (cumulative average) is not built")
    rm, rv = (bn.running_mean, bn.running_var) if bn.track_running_stats else (None, None)
    y = _ReluBN.apply(a, bn.weight, bn.bias, rm, rv, float(bn.eps), float(bn.momentum), bool(relu))
    if bn.track_running_stats:
        bn.num_batches_tracked += 1
    return y


def batch_norm_eval(x, bn, relu=False):
    """The eval form of `bn`: x . s + t from the running buffers (swnerf_bn_apply)."""
    x = _lib.dev_f32(x, "x", bn.num_features)
    _need_cuda(bn.weight, "BatchNorm1d parameters")
    y = torch.empty_like(x)
    M, C = x.shape
    _lib.check(_lib.lib().swnerf_bn_apply(_lib.ptr(x), M, C, int(relu), _lib.ptr(bn.weight.detach()), _lib.ptr(bn.bias.detach()),
                                          _lib.ptr(bn.running_mean), _lib.ptr(bn.running_var), float(bn.eps), _lib.ptr(y),
                                          _lib.stream_of(x)), "bn_apply")
    return y


class Model(nn.Module):
    """2d_pos_encoding/model.py:2-43: the same nn.Sequential, built in the same order with the same Xavier re-initialisation, so
    state_dict keys and seed-0 initial values equal the reference's."""

    def __init__(self, input_dimension: int, layer_num: int, hidden_dim: int = 256, output_dim: int = 3):
        super().__init__()
        layers = []
        current_dim = input_dimension
        for i in range(layer_num):
            layers.extend([nn.Linear(current_dim, hidden_dim), nn.ReLU(inplace=True), nn.BatchNorm1d(hidden_dim)])
            current_dim = hidden_dim
        layers.append(nn.Linear(current_dim, output_dim))
        self.model = nn.Sequential(*layers)
        self._initialize_weights()
        self.input_dimension, self.layer_num, self.hidden_dim, self.output_dim = input_dimension, layer_num, hidden_dim, output_dim
        self._stats_version = 0          # bumped by every training forward: the kernels write the running buffers through raw
        self._pack_cache = {}            # pointers, so torch's _version does not see them

    def _initialize_weights(self):
        for layer in self.modules():
            if isinstance(layer, nn.Linear):
                nn.init.xavier_uniform_(layer.weight)
                if layer.bias is not None:
                    nn.init.zeros_(layer.bias)

    # -- structure
    def _blocks(self):
        m = self.model
        return [(m[3 * i], m[3 * i + 2]) for i in range(self.layer_num)], m[3 * self.layer_num]

    def fused_L(self):
        """the band count L when eval mode takes the fused pass, else None"""
        d = self.input_dimension
        if self.hidden_dim != 256 or self.output_dim != 3 or self.layer_num < 1 or self.layer_num > MAX_FUSED_LAYERS:
            return None
        if d < 2 or (d - 2) % 4 != 0 or (d - 2) // 4 > MAX_L:
            return None
        if any(not bn.track_running_stats or not bn.affine for _, bn in self._blocks()[0]):
            return None
        return (d - 2) // 4

    # -- the packed stream, cached
    def packed(self):
        """The fused pass's weight stream (swnerf_pack_fit2d), cached by swnerf.packing on every parameter and buffer plus
        _stats_version."""
        L = self.fused_L()
        if L is None:
            raise RuntimeError("swnerf.fit2d: this Model has no fused form (hidden_dim 256, output_dim 3, input_dimension 4L + 2, L <= 23)")
        blocks, head = self._blocks()
        eps = {float(bn.eps) for _, bn in blocks}
        if len(eps) != 1:
            raise NotImplementedError("swnerf.fit2d: BatchNorm1d layers with different eps")
        ts = [t for lin, bn in blocks for t in (lin.weight, lin.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var)]
        return packing.pack_weights(self._pack_cache, "fwd", ts + [head.weight, head.bias],
                                    lambda lib: lib.swnerf_fit2d_packed_floats(self.layer_num),
                                    lambda lib, arr, blob, st: lib.swnerf_pack_fit2d(arr, self.layer_num, L, eps.pop(), blob, st), "pack_fit2d",
                                    extra=(self._stats_version,), keyed_on=list(self.parameters()) + list(self.buffers()))

    # -- forward
    def forward_layers(self, x):
        """layer by layer, in the module's current mode"""
        blocks, head = self._blocks()
        h = _lib.dev_f32(x, "x", self.input_dimension)
        if self.training:
            for lin, bn in blocks:
                h = relu_batch_norm(generic.linear(h, lin, act=_lib.ACT_NONE), bn, relu=True)
            self._stats_version += 1
        else:
            for lin, bn in blocks:
                h = batch_norm_eval(generic.linear(h, lin, act=_lib.ACT_RELU), bn)
        return generic.linear(h, head, act=_lib.ACT_NONE)

    def forward(self, x):
        _need_cuda(next(self.parameters()), "module parameters")
        if x.dim() != 2:
            raise ValueError(f"swnerf.fit2d: Model input must be [M, {self.input_dimension}], got {tuple(x.shape)}")
        L = self.fused_L()
        if self.training or L is None:
            return self.forward_layers(x)
        # the fused pass has no backward: its output carries no graph (the reference evaluates under no_grad, utils.py:117)
        x = _lib.dev_f32(x, "x", self.input_dimension)
        out = torch.empty((x.shape[0], 3), dtype=torch.float32, device=x.device)
        _lib.check(_lib.lib().swnerf_fit2d_forward(_lib.ptr(self.packed()), _lib.ptr(x), x.shape[0], x.stride(0), L, self.layer_num,
                                                   _lib.ptr(out), _lib.stream_of(x)), "fit2d_forward")
        return out


# ---- encoding.py ------------------------------------------------------------------------------------------------------
def encode_normalised(pos, max_x, max_y, L):
    """encode with the maxima given (train() computes them once for the whole picture)"""
    pos = _lib.dev_f32(pos, "pos", 2)
    out = torch.empty((pos.shape[0], 4 * L + 2), dtype=torch.float32, device=pos.device)
    _lib.check(_lib.lib().swnerf_encode2d(_lib.ptr(pos), pos.shape[0], float(max_x), float(max_y), int(L), _lib.ptr(out),
                                          _lib.stream_of(pos)), "encode2d")
    return out


def encode(pos, L):
    """encoding.py:22-40: [x, y] -> [x, y, sin(2^i pi x), sin(2^i pi y), cos(2^i pi x), cos(2^i pi y), ...] with x, y normalised to
    [-1, 1] by the maxima over the given `pos`.  A picture one pixel wide (a maximum of 0) is refused: the reference divides by 0."""
    if not (0 <= L <= MAX_L):
        raise ValueError(f"swnerf.fit2d.encode: L {L} outside 0..{MAX_L}")
    pos = _lib.dev_f32(pos, "pos", 2)
    if pos.shape[0] == 0:
        return torch.empty((0, 4 * L + 2), dtype=torch.float32, device=pos.device)
    mx = pos.max(dim=0).values.tolist()
    if not (mx[0] > 0 and mx[1] > 0):
        raise ValueError(f"swnerf.fit2d.encode: max over pos is {mx}; both must be > 0")
    return encode_normalised(pos, mx[0], mx[1], L)


def load_picture(args):
    """encoding.py:4-20: positions [(H*W), 2] (x fastest), colours [(H*W), 3] in [0, 1], width, height.  Without PIL the picture
    (.png, or a baseline .jpg: libjpeg's pixels byte for byte) is decoded on the GPU by swnerf.images."""
    try:
        from PIL import Image
    except ImportError:
        from . import images
        return picture_tensors(images.load_pngs([args.picture_dir])[0, ..., :3].cpu().numpy())
    return picture_tensors(np.asarray(Image.open(args.picture_dir).convert('RGB')))


def picture_tensors(rgb_u8):
    """the tensors of load_picture from an [H, W, 3] uint8 array"""
    rgb_u8 = np.asarray(rgb_u8)
    height, width = rgb_u8.shape[:2]
    ys, xs = np.mgrid[0:height, 0:width]
    positions = torch.tensor(np.stack([xs.reshape(-1), ys.reshape(-1)], -1), dtype=torch.float32)
    colors = torch.tensor(rgb_u8.reshape(-1, 3) / 255.0, dtype=torch.float32)
    return positions, colors, width, height


# ---- utils.py ---------------------------------------------------------------------------------------------------------
def getfilename(args):
    picture_filename = os.path.splitext(os.path.basename(args.picture_dir))[0]
    return f"{picture_filename}_{args.L}_{args.layer_num}_{args.regularization}"


class _Loss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, out, target, reg):
        sums = torch.empty((2,), dtype=torch.float64, device=out.device)
        grad = torch.empty_like(out)
        _lib.check(_lib.lib().swnerf_fit2d_loss(_lib.ptr(out), _lib.ptr(target), out.shape[0], float(reg), _lib.ptr(sums), _lib.ptr(grad),
                                                _lib.stream_of(out)), "fit2d_loss")
        ctx.save_for_backward(grad)
        ctx.mark_non_differentiable(sums)
        return sums[0].float(), sums
    @staticmethod
    def backward(ctx, g, _):
        (grad,) = ctx.saved_tensors
        return grad * g, None, None


def fit_loss(output, color, regularization):
    """utils.py:56 in one launch: (mse_loss(output, color) + cliploss(output), sums) - sums is a float64 [2] device tensor holding
    that loss and the grey-scale mse of utils.py:62-64.  Differentiable in `output`; at the ties output == 0 or 1 the clip
    term's subgradient is 0 (torch: 0.25 * regularization / numel)."""
    output, color = _lib.dev_f32(output, "output", 3), _lib.dev_f32(color, "color", 3)
    if output.shape != color.shape or output.dim() != 2:
        raise ValueError(f"swnerf.fit2d.fit_loss: output {tuple(output.shape)} and color {tuple(color.shape)} must both be [M, 3]")
    return _Loss.apply(output, color, float(regularization))


def cliploss(input, args):
    """utils.py:12-14 (torch ops on the caller's device; train() uses the fused fit_loss)"""
    loss = torch.mean(torch.max(torch.max(torch.zeros_like(input), input - 1), torch.max(-input, torch.zeros_like(input))))
    return loss * args.regularization


def load_checkpoint(model, optimizer, args):
    checkpoint = torch.load(args.checkpoint_load, map_location=next(model.parameters()).device, weights_only=False)
    model.load_state_dict(checkpoint['model_state_dict'])
    optimizer.load_state_dict(checkpoint['optimizer_state_dict'])
    return checkpoint['cur_epoch'], checkpoint['metrics']


def save_checkpoint(model, optimizer, cur_epoch, metrics, args):
    filename = os.path.join(args.checkpoint_save, getfilename(args) + ".pth")
    checkpoint = {'cur_epoch': cur_epoch + 1,
                  'model_state_dict': model.state_dict(),
                  'optimizer_state_dict': optimizer.state_dict(),
                  'metrics': metrics}
    torch.save(checkpoint, filename)
    print(f"Checkpoint saved at epoch {cur_epoch+1} to {filename}")
    return filename


def _picture(width, height, model, L, want_f32=True, want_u8=False):
    _need_cuda(next(model.parameters()), "module parameters")
    if model.training:
        raise RuntimeError("swnerf.fit2d.get_picture: call model.eval() first (the reference's test() does)")
    if model.fused_L() != L:
        # any other shape: the layer-by-layer eval path on the encoded grid
        pos = picture_tensors(np.zeros((height, width, 3), np.uint8))[0].to(next(model.parameters()).device)
        with torch.no_grad():
            f = model(encode(pos, L)).reshape(height, width, 3).clamp(0, 1)
        return (f if want_f32 else None), ((255 * f).to(torch.uint8) if want_u8 else None)
    dev = next(model.parameters()).device
    f = torch.empty((height, width, 3), dtype=torch.float32, device=dev) if want_f32 else None
    u = torch.empty((height, width, 3), dtype=torch.uint8, device=dev) if want_u8 else None
    ref = f if f is not None else u
    _lib.check(_lib.lib().swnerf_fit2d_picture(_lib.ptr(model.packed()), height, width, L, model.layer_num, _lib.ptr(f), _lib.ptr(u),
                                               _lib.stream_of(ref)), "fit2d_picture")
    return f, u


def get_picture(width, height, model, args):
    """utils.py:103-126: the [H, W, 3] picture in [0, 1] as a numpy array - one swnerf_fit2d_picture launch."""
    return _picture(width, height, model, args.L)[0].cpu().numpy()


def get_picture_u8(width, height, model, args):
    """to8b(get_picture(...)) computed by the same launch"""
    return _picture(width, height, model, args.L, want_f32=False, want_u8=True)[1].cpu().numpy()


def test(width, height, model, args):
    """utils.py:88-101: the final picture as <output_dir>/<name>.png (swnerf.png; the reference's plt.imsave writes the same
    8-bit RGB, with an opaque alpha channel added)."""
    model.eval()
    path = os.path.join(args.output_dir, getfilename(args) + ".png")
    write_png(path, get_picture_u8(width, height, model, args))
    return path


def train(data, model, optimizer, scheduler, args, width, height):
    """utils.py:33-87.  `data` = (positions [HW, 2], colors [HW, 3]) as load_picture returns them (the reference passes a
    DataLoader over the encoded rows).  Normalised by the picture's maxima once; every epoch draws a torch.randperm on the
    device, each batch of 512 is gathered and encoded on the fly, the last short batch is kept.  The batch order is torch's
    device generator, not the DataLoader's RNG stream.  Loss and grey mse are accumulated on the device and read once per epoch."""
    pos, color = data
    dev = next(model.parameters()).device
    _need_cuda(next(model.parameters()), "module parameters")
    pos, color = _lib.dev_f32(pos.to(dev), "positions", 2), _lib.dev_f32(color.to(dev), "colors", 3)
    mx = pos.max(dim=0).values.tolist()
    if not (mx[0] > 0 and mx[1] > 0):
        raise ValueError(f"swnerf.fit2d.train: max over positions is {mx}; both must be > 0")
    epoch = args.epochs
    cur_epoch = 0
    metrics = {"MSE": [], "PSNR": []}
    if getattr(args, "checkpoint_load", None):
        cur_epoch, metrics = load_checkpoint(model, optimizer, args)
    n = pos.shape[0]
    iternum = (n + BATCH - 1) // BATCH
    start_time = time.time()
    for i in range(cur_epoch, epoch):
        model.train()
        totals = torch.zeros((2,), dtype=torch.float64, device=dev)
        perm = torch.randperm(n, device=dev)
        for b in range(iternum):
            idx = perm[b * BATCH:(b + 1) * BATCH]
            x = encode_normalised(pos[idx], mx[0], mx[1], args.L)
            optimizer.zero_grad()
            loss, sums = fit_loss(model(x), color[idx], args.regularization)
            loss.backward()
            optimizer.step()
            totals += sums
        avg_mse, avg_gray_mse = (totals / iternum).tolist()              # the one read of the epoch
        avg_gray_mse = torch.tensor(avg_gray_mse, device=dev)
        psnr = 10 * torch.log(1 / avg_gray_mse) / torch.log(torch.tensor(10.0))
        metrics["MSE"].append(avg_mse)
        metrics["PSNR"].append(psnr)
        if getattr(args, "v", False):
            print(f"Epoch {i+1}/{epoch} MSE: {avg_mse:.4f} PSNR: {psnr:.4f} time: {time.time()-start_time:.2f}s")
        if getattr(args, "checkpoint_save", None):
            save_checkpoint(model, optimizer, i, metrics, args)
        if (i + 1) % 20 == 0 and getattr(args, "output_dir", None):
            test(width, height, model, args)
        scheduler.step()
    if metrics["MSE"]:
        print(f"final mse: {metrics['MSE'][-1]}, final psnr: {metrics['PSNR'][-1]}")
    return metrics
