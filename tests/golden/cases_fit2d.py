"""Seeded inputs and weights of the 2-D fitting golden vectors G16 (make_golden_fit2d.py; tests/test_fit2d_host.py,
tests/test_gpu_fit2d.py, tools/tight_buffer_check_fit2d.py).  Everything here is regenerated from seeds: the .npz holds
outputs only."""
import numpy as np

import cases
from cases import synth, checksum  # noqa: F401

GRID_W, GRID_H = 53, 37
ENCODE_LS = (0, 1, 4, 10, 20, 23)
# eval cases: name -> (layer_num, L, hidden_dim, weight seed); hidden 256 takes the fused pass, 64 the layer-by-layer one
EVAL = {"d10_L20": (10, 20, 256, 1601), "d1_L20": (1, 20, 256, 1602), "d3_L4": (3, 4, 256, 1603), "generic": (3, 4, 64, 1604)}
# the training step and the AdamW sequence: layer_num 3, hidden 64, L 4, 48 rows, reg 0.1.  The seed is one for which no
# pre-activation of the step lies within 1e-5 of zero in float64 (make_golden_fit2d.py asserts it, and prints the margin)
TRAIN = dict(layer_num=3, L=4, hidden_dim=64, rows=48, reg=0.1, seed=1611, data_seed=1612)
ADAMW_STEPS, ADAMW_SCHED_AFTER = 5, 3          # scheduler.step() once, after the third optimizer step


def grid(w=GRID_W, h=GRID_H):
    """pixel positions [(h*w), 2] = (x, y), x fastest (encoding.py:14)"""
    ys, xs = np.mgrid[0:h, 0:w]
    return np.stack([xs.reshape(-1), ys.reshape(-1)], -1).astype(np.float32)


def weights(name):
    n, L, hid, seed = EVAL[name]
    return synth.fit2d_state_dict(seed, 4 * L + 2, n, hid)


def train_weights():
    t = TRAIN
    return synth.fit2d_state_dict(t["seed"], 4 * t["L"] + 2, t["layer_num"], t["hidden_dim"])


def train_batch():
    """48 grid pixels (their positions within the 53 x 37 grid) and target colours spanning [0, 1]"""
    rng = np.random.default_rng(TRAIN["data_seed"])
    idx = rng.choice(GRID_W * GRID_H, TRAIN["rows"], replace=False)
    return idx.astype(np.int64), rng.uniform(0.0, 1.0, (TRAIN["rows"], 3)).astype(np.float32)


# ---- the shape sweep of the fused pass (tests/test_gpu_fit2d_shapes.py, tests/test_fit2d_host.py) -----------------------------
# name -> (group, L, layer_num, weight seed): hidden 256, 3 outputs, float64 fit2d_ref.forward_eval is the yardstick.  Not part of
# inputs_checksum(): G16 holds nothing of these.
SHAPES = {}
for _L in range(24):
    SHAPES[f"band_L{_L}"] = ("band", _L, 2, 1700 + _L)
for _n in (1, 2, 3, 9, 17, 33, 63, 64):
    SHAPES[f"depth_n{_n}"] = ("depth", 10, _n, 1730 + _n)
CORNERS = ("corner_L0_n1", "corner_L0_n64", "corner_L23_n1", "corner_L23_n64")
for _k, (_L, _n) in enumerate(((0, 1), (0, 64), (23, 1), (23, 64))):
    SHAPES[CORNERS[_k]] = ("corner", _L, _n, 1800 + _k)
SHAPES["rows_L12_n5"] = ("rows", 12, 5, 1810)
ROW_COUNTS = (1, 31, 32, 33, 127, 128, 129)
SHAPE_ROWS_SHALLOW, DEEP_FROM = 161, 17     # one full workgroup of 128 + one full tile of 32 + a single-row tile; 17+ layers: all 1961
# BatchNorm statistics the fold must survive: L 6, 3 layers; (a) eps 1e-3, (b) the default eps with running_var >= 1e-3
BN_L, BN_LAYERS, BN_SEED = 6, 3, 1820
BN_EPS = {"bn_a": 1e-3, "bn_b": 1e-5}
# shapes that must take the layer-by-layer route: name -> (input_dimension, layer_num, hidden_dim, output_dim, seed)
LAYERWISE = {"lw_d7": (7, 2, 256, 3, 1830), "lw_L24": (98, 2, 256, 3, 1831), "lw_hid255": (18, 3, 255, 3, 1832),
             "lw_hid257": (18, 3, 257, 3, 1833), "lw_out4": (18, 2, 256, 4, 1834), "lw_n65": (18, 65, 256, 3, 1835)}


def shape_weights(name):
    _, L, n, seed = SHAPES[name]
    return synth.fit2d_state_dict(seed, 4 * L + 2, n, 256)


def shape_rows(n_layers, seed):
    """indices into the 53 x 37 grid: a seeded subset of 161 pixels below 17 layers, every pixel from 17 layers on"""
    total = GRID_W * GRID_H
    if n_layers >= DEEP_FROM:
        return np.arange(total, dtype=np.int64)
    return np.sort(np.random.default_rng(seed + 5000).choice(total, SHAPE_ROWS_SHALLOW, replace=False)).astype(np.int64)


def bn_weights(which):
    """(state dict, eps).  Per layer, disjoint seeded channels: 8 with weight 0, 4 with running_var 0, 4 with running_var 1e-12,
    4 with running_mean +50, 4 with running_mean -50.  bn_b: the same net with running_var raised to at least 1e-3."""
    sd = synth.fit2d_state_dict(BN_SEED, 4 * BN_L + 2, BN_LAYERS, 256)
    rng = np.random.default_rng(BN_SEED + 1)
    for i in range(BN_LAYERS):
        ch = rng.permutation(256)[:24]
        p = f"model.{3 * i + 2}."
        sd[p + "weight"][ch[:8]] = 0.0
        sd[p + "running_var"][ch[8:12]] = 0.0
        sd[p + "running_var"][ch[12:16]] = 1e-12
        sd[p + "running_mean"][ch[16:20]] = 50.0
        sd[p + "running_mean"][ch[20:24]] = -50.0
        if which == "bn_b":
            sd[p + "running_var"] = np.maximum(sd[p + "running_var"], np.float32(1e-3))
    return sd, BN_EPS[which]


def layerwise_weights(name):
    d, n, hid, out, seed = LAYERWISE[name]
    return synth.fit2d_state_dict(seed, d, n, hid, out)


def layerwise_rows(name):
    """rows for a shape whose width is no encoding's (d = 7) or beyond the encoder's band limit (L = 24): seeded uniform (-1, 1)"""
    d, n, _, _, seed = LAYERWISE[name]
    return np.random.default_rng(seed + 5000).uniform(-1.0, 1.0, (SHAPE_ROWS_SHALLOW, d)).astype(np.float32)


def inputs_checksum():
    arrs = [grid(), *train_batch()]
    for name in sorted(EVAL):
        sd = weights(name)
        arrs += [sd[k] for k in sorted(sd)]
    sd = train_weights()
    return checksum(*arrs, *[sd[k] for k in sorted(sd)])
