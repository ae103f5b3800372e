#!/usr/bin/env python3
"""Capture golden vectors G16 from the UNMODIFIED reference (build container only): 2d_pos_encoding/encoding.py `encode` and
model.py `Model` on the seeded inputs and weights of cases_fit2d.py, one training-mode step and a 5-step AdamW sequence with
utils.py's loss.  Only OUTPUTS (plus a checksum of the seeded inputs) are stored.
Run: python tests/golden/make_golden_fit2d.py"""
import importlib.util
import os
import sys
import types

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import cases_fit2d as C  # noqa: E402
import fit2d_ref as R    # noqa: E402

REF = "/root/reference/2d_pos_encoding"
for name in ("PIL", "PIL.Image", "tqdm", "matplotlib", "matplotlib.pyplot"):
    try:
        importlib.import_module(name)
    except Exception:
        sys.modules[name] = types.ModuleType(name)
        if "." in name:
            setattr(sys.modules[name.split(".")[0]], name.split(".")[1], sys.modules[name])

import torch  # noqa: E402


def _load(fname, name):
    sys.path.insert(0, REF)
    try:
        spec = importlib.util.spec_from_file_location(name, os.path.join(REF, fname))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.pop(0)
    return mod


ENC = _load("encoding.py", "ref_fit2d_encoding")
MODEL = _load("model.py", "ref_fit2d_model")
UTILS = _load("utils.py", "ref_fit2d_utils")
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
out = {"checksum": C.inputs_checksum()}

# encode on the grid.  A column depends on x alone or on y alone and a smaller L is a prefix of a larger one: the 53 (37)
# distinct x (y) rows of L = 23 are stored, after checking bit for bit that they reproduce the reference's output for every L
pos = C.grid()
full = {L: ENC.encode(T(pos), L).numpy() for L in C.ENCODE_LS}
e23 = full[23]
xcols = [0] + [4 * i + 2 + 2 * s for i in range(23) for s in (0, 1)]
ycols = [c + 1 for c in xcols]
enc_x, enc_y = e23[:C.GRID_W][:, xcols], e23[::C.GRID_W][:, ycols]
for L, e in full.items():
    want = np.zeros_like(e)
    for j, (cx, cy) in enumerate(zip(xcols, ycols)):
        if cx < 4 * L + 2:
            want[:, cx] = enc_x[pos[:, 0].astype(int), j]
            want[:, cy] = enc_y[pos[:, 1].astype(int), j]
    assert np.array_equal(want, e), L
out["enc_x"], out["enc_y"] = enc_x, enc_y
print("encode: band-19 |ref - float64| max", np.abs(full[20] - R.encode(pos, 20)).max())

# seed-0 initial state_dict: names, shapes, per-tensor sums
torch.manual_seed(0)
sd0 = MODEL.Model(input_dimension=82, layer_num=10).state_dict()
out["init_names"] = np.array(list(sd0.keys()))
out["init_shapes"] = np.array([(list(v.shape) + [0, 0])[:2] for v in sd0.values()], np.int64)
out["init_sums"] = np.array([float(v.double().sum()) for v in sd0.values()])

# Model.eval() on the grid
for name, (n, L, hid, _) in C.EVAL.items():
    sd = C.weights(name)
    net = MODEL.Model(4 * L + 2, n, hidden_dim=hid)
    net.load_state_dict({k: T(v) for k, v in sd.items()}, strict=True)
    net.eval()
    with torch.no_grad():
        y = net(T(full[L])).numpy()
    out[f"eval_{name}"] = y
    ref64 = R.forward_eval(sd, full[L].astype(np.float64))
    fold64 = R.forward_folded(R.fold(sd), full[L].astype(np.float64))
    print(f"{name}: out [{y.min():.2f}, {y.max():.2f}] std {y.std():.2f}; |ref - f64| {np.abs(y - ref64).max():.2e}, "
          f"|folded - f64| {np.abs(fold64 - ref64).max():.2e}")

# one training-mode step (utils.py:54-57) and the AdamW sequence (main.py:21-23)
t = C.TRAIN
idx, target = C.train_batch()
x = full[t["L"]][idx]
args = types.SimpleNamespace(regularization=t["reg"])


def fresh():
    net = MODEL.Model(4 * t["L"] + 2, t["layer_num"], hidden_dim=t["hidden_dim"])
    net.load_state_dict({k: T(v) for k, v in C.train_weights().items()}, strict=True)
    return net.train()


net = fresh()
o = net(T(x))
loss = torch.nn.functional.mse_loss(o, T(target)) + UTILS.cliploss(o, args)
loss.backward()
out["train_loss"] = np.array([float(loss)])
out["train_out"] = o.detach().numpy()
for k, p in net.named_parameters():
    out[f"train_grad_{k}"] = p.grad.numpy()
for k, b in net.named_buffers():
    out[f"train_buf_{k}"] = b.detach().numpy()
l64, g64, grads64, _, pre = R.train_step(C.train_weights(), x, target, t["reg"], t["layer_num"], t["hidden_dim"])
margin = min(float(np.abs(p).min()) for p in pre)
out_margin = min(float(np.abs(o.detach().numpy() - v).min()) for v in (0.0, 1.0))
print(f"train: loss {float(loss):.6f} (f64 {l64:.6f}); ReLU margin {margin:.2e}; clip-tie margin {out_margin:.2e}; "
      f"out [{float(o.min()):.2f}, {float(o.max()):.2f}]")
assert margin > 1e-5 and out_margin > 1e-5, "choose another TRAIN seed"
for k, g in grads64.items():
    print(f"  grad {k}: max {np.abs(g).max():.3e}, |ref - f64| / max {np.abs(out['train_grad_' + k] - g).max() / np.abs(g).max():.2e}")

net = fresh()
opt = torch.optim.AdamW(net.parameters(), lr=0.001)
sch = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.95)
losses = []
for k in range(C.ADAMW_STEPS):
    opt.zero_grad()
    o = net(T(x))
    loss = torch.nn.functional.mse_loss(o, T(target)) + UTILS.cliploss(o, args)
    loss.backward()
    opt.step()
    losses.append(float(loss))
    if k + 1 == C.ADAMW_SCHED_AFTER:
        sch.step()
out["adamw_losses"] = np.array(losses)
out["adamw_last_weight"] = net.model[3 * t["layer_num"]].weight.detach().numpy()
out["adamw_last_bias"] = net.model[3 * t["layer_num"]].bias.detach().numpy()
print("adamw losses", losses)
path = os.path.join(HERE, "g16_fit2d.npz")
np.savez_compressed(path, **out)
print("wrote g16_fit2d.npz", os.path.getsize(path), "bytes")
