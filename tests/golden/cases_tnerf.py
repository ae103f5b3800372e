"""Seeded inputs and weights of the T-NeRF golden vectors G14 (make_golden_tnerf.py; tests/test_tnerf_host.py,
tests/test_gpu_tnerf.py).  Everything here is regenerated from seeds: the .npz holds outputs only."""
import numpy as np

import cases
from cases import synth, legacy_rand, checksum  # noqa: F401

NET = dict(depth=8, in_feat=63, dir_feat=27, time_feat=21, net_dim=128, skip_layer=4)
WEIGHT_SEED = 141
FRAME_TIME = 0.375
N_RAYS = 128
N_SAMPLES = 64
N_ROWS = 96
KEEP = 16                      # rays whose raw / z_vals rows are stored


def weights():
    return synth.tnerf_state_dict(WEIGHT_SEED)


def rays(n=N_RAYS, seed=14):
    """[o, d, near, far, t, viewdirs] rows as run_tnerf.py:156-164 builds them (float32)."""
    g = cases.g7_inputs(n=n, seed=seed)
    o, d = g["rays_o"].astype(np.float32), g["rays_d"].astype(np.float32)
    vd = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)
    one = np.ones((n, 1), np.float32)
    return np.concatenate([o, d, 2.0 * one, 6.0 * one, np.float32(FRAME_TIME) * one, vd], -1).astype(np.float32)


def given_z(n=N_RAYS, S=N_SAMPLES, seed=15):
    rng = np.random.default_rng(seed)
    return np.sort(rng.uniform(2.0, 6.0, (n, S)), axis=-1).astype(np.float32)


def forward_rows(n=N_ROWS, seed=16):
    """points, one time, directions for TNeRF.forward rows (embedded by the caller)"""
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-1.5, 1.5, (n, 3)).astype(np.float32)
    d = rng.standard_normal((n, 3)).astype(np.float32)
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)
    return pts, d, np.full((n, 1), FRAME_TIME, np.float32)


# render_rays cases: name -> keyword arguments of render_rays (t_rand / noise: injected draws, legacy_rand)
CASES = {
    "det": dict(white_bkgd=True),
    "det_black": dict(white_bkgd=False),
    "lindisp": dict(white_bkgd=True, lindisp=True),
    "perturb": dict(white_bkgd=True, perturb=1.0),           # t_rand = legacy_rand(N, S)
    "zvals": dict(white_bkgd=True, z_vals=True),              # z_vals = given_z()
    "noise": dict(white_bkgd=False, raw_noise_std=1.0),       # noise = legacy_rand(N, S) * 1.0 (run_tnerf.py pytest hook)
}


def inputs_checksum():
    sd = weights()
    return checksum(rays(), given_z(), *forward_rows(), *[sd[k] for k in sorted(sd)])
