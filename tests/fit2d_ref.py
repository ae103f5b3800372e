"""Float64 restatement of the 2-D fitting arithmetic (2d_pos_encoding/encoding.py:22-40, model.py:6-43, utils.py:13,56,62-64), in
the manner of tests/tnerf_ref.py: what tests/test_fit2d_host.py checks against the golden G16 and what the GPU tests compare
the kernels with.  `module()` is the same net in plain torch ops (any dtype, any device): the float64 reference of the
training step, and the torch baseline of tools/bench_fit2d.py."""
import numpy as np
import torch
import torch.nn as nn

PI32 = np.float32(np.pi)


def normalise(pos, max_x=None, max_y=None):
    """2 * (pos / max) - 1 in float32, one rounding per operation"""
    pos = np.asarray(pos, np.float32)
    mx = np.array([pos[:, 0].max() if max_x is None else max_x, pos[:, 1].max() if max_y is None else max_y], np.float32)
    return (np.float32(2) * (pos / mx) - np.float32(1)).astype(np.float32)


def encode(pos, L, max_x=None, max_y=None):
    """float64 sin / cos of the float32 argument fl32(2^i pi) * xn (ONE float32 product); columns as encoding.py:29-38"""
    xn = normalise(pos, max_x, max_y)
    out = np.zeros((xn.shape[0], 4 * L + 2), np.float64)
    out[:, :2] = xn
    for i in range(L):
        a = ((PI32 * np.float32(2 ** i)) * xn).astype(np.float32).astype(np.float64)
        out[:, 4 * i + 2:4 * i + 4] = np.sin(a)
        out[:, 4 * i + 4:4 * i + 6] = np.cos(a)
    return out


def layer_num(sd):
    return (max(int(k.split(".")[1]) for k in sd)) // 3


def forward_eval(sd, x, eps=1e-5, want_pre=False):
    """Model.eval()(x) in float64; want_pre: also the pre-activations of every hidden layer"""
    h = np.asarray(x, np.float64)
    pre = []
    n = layer_num(sd)
    for i in range(n):
        a = h @ sd[f"model.{3 * i}.weight"].astype(np.float64).T + sd[f"model.{3 * i}.bias"].astype(np.float64)
        pre.append(a)
        s = sd[f"model.{3 * i + 2}.weight"].astype(np.float64) / np.sqrt(sd[f"model.{3 * i + 2}.running_var"].astype(np.float64) + eps)
        h = (np.maximum(a, 0) - sd[f"model.{3 * i + 2}.running_mean"].astype(np.float64)) * s + sd[f"model.{3 * i + 2}.bias"].astype(np.float64)
    out = h @ sd[f"model.{3 * n}.weight"].astype(np.float64).T + sd[f"model.{3 * n}.bias"].astype(np.float64)
    return (out, pre) if want_pre else out


def fold(sd, eps=1e-5):
    """the folded net of swnerf_pack_fit2d: [(W', b')] per Linear, float32 (fp64 product, one rounding)"""
    n = layer_num(sd)
    out = [(sd["model.0.weight"].astype(np.float32), sd["model.0.bias"].astype(np.float32))]
    for l in range(1, n + 1):
        b = 3 * (l - 1) + 2
        s = sd[f"model.{b}.weight"].astype(np.float64) / np.sqrt(sd[f"model.{b}.running_var"].astype(np.float64) + eps)
        t = sd[f"model.{b}.bias"].astype(np.float64) - sd[f"model.{b}.running_mean"].astype(np.float64) * s
        W = sd[f"model.{3 * l}.weight"].astype(np.float64)
        out.append(((W * s).astype(np.float32), (sd[f"model.{3 * l}.bias"].astype(np.float64) + W @ t).astype(np.float32)))
    return out


def forward_folded(folded, x):
    h = np.asarray(x, np.float64)
    for W, b in folded[:-1]:
        h = np.maximum(h @ W.astype(np.float64).T + b.astype(np.float64), 0)
    W, b = folded[-1]
    return h @ W.astype(np.float64).T + b.astype(np.float64)


def module(input_dimension, n_layers, hidden_dim=256, output_dim=3, sd=None, dtype=torch.float64, device="cpu"):
    """the net as plain torch modules, keys `model.N...` like the reference's"""
    layers, k = [], input_dimension
    for _ in range(n_layers):
        layers += [nn.Linear(k, hidden_dim), nn.ReLU(), nn.BatchNorm1d(hidden_dim)]
        k = hidden_dim
    layers.append(nn.Linear(k, output_dim))

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.model = nn.Sequential(*layers)

        def forward(self, x):
            return self.model(x)
    net = Net()
    if sd is not None:
        net.load_state_dict({k_: torch.from_numpy(np.asarray(v)) for k_, v in sd.items()})
    return net.to(device=device, dtype=dtype)


def loss(out, target, reg):
    """utils.py:56 with cliploss (utils.py:12-14), torch ops"""
    z = torch.zeros_like(out)
    clip = torch.mean(torch.max(torch.max(z, out - 1), torch.max(-out, z)))
    return torch.nn.functional.mse_loss(out, target) + clip * reg


def gray_mse(out, target):
    g = lambda c: 0.2989 * c[:, 0] + 0.5870 * c[:, 1] + 0.1140 * c[:, 2]
    return torch.nn.functional.mse_loss(g(out), g(target))


def train_step(sd, x, target, reg, n_layers, hidden_dim):
    """one training-mode step in float64: loss, grey mse, gradients by name, buffers after the step, the pre-activations"""
    net = module(x.shape[1], n_layers, hidden_dim, 3, sd).train()
    xt, tt = torch.from_numpy(np.asarray(x, np.float64)), torch.from_numpy(np.asarray(target, np.float64))
    pre = []
    hooks = [net.model[3 * i].register_forward_hook(lambda m, i_, o: pre.append(o.detach().numpy().copy())) for i in range(n_layers)]
    out = net(xt)
    for h in hooks:
        h.remove()
    l = loss(out, tt, reg)
    l.backward()
    grads = {k: p.grad.numpy() for k, p in net.named_parameters()}
    bufs = {k: b.detach().numpy() for k, b in net.named_buffers()}
    return float(l.detach()), float(gray_mse(out.detach(), tt)), grads, bufs, pre
