"""Seeded nets and rays for the embedder band counts other than (10, 4, 10) (tests/test_gpu_bands.py, tests/test_bands_host.py).

A net with L bands has input widths 3(1+2 L_pos) / 3(1+2 L_dir) / 1+2 L_time; the weights are He-normal draws of the
reference's shapes at those widths (swnerf.synth, the builders of the other golden cases), the opacity biases chosen with the
CPU oracle so that acc_map on the test rays is neither all 0 nor all 1 (tests/test_bands_host.py asserts it).

`widen` builds the (10, 4, 10) net that computes the same function: in the reference column order the lower bands are a
prefix of each encoded block, so the extra input columns get zero weights behind each block."""
import numpy as np

import cases
from cases import synth

# (L_pos, L_dir, L_time), chosen from the slot maps (csrc/swnerf_common.h sw_pos_col / sw_dir_col / sw_time_col):
# L_pos 0 = identity only (k-tile 0 of gamma(x) all pad), 1, 5 = k-tile 1 holds one component of a band and the identity,
# 6 = the band that straddles the two k-tiles, 9, 10; L_dir 0..4; L_time 0 (gamma(t) = t), 1, 4, 9, 10.
# (10, 4, 10) is the control row: the same harness at the sizes every other test runs.
TRIPLES = [(0, 0, 0), (1, 1, 1), (5, 2, 4), (6, 3, 9), (9, 4, 10), (10, 0, 0), (10, 4, 10)]
CONTROL = (10, 4, 10)
# the gradient cases (float64 autograd on the CPU side of each): a zero one, the straddling one, the control row
GRAD_TRIPLES = [(0, 0, 0), (6, 3, 9), (10, 4, 10)]
KINDS = ("canon", "noview", "dnerf", "tnerf")

# inference: a ragged last tile (S = 40 -> 32 + 8, fine 64), 37 rays = a workgroup with dead waves; and the smallest pass
N_RAYS, N_SAMPLES, N_IMPORTANCE = 37, 40, 24
FRAME_TIME = 0.5


def applicable(kind, bands):
    """The members of a triple that a net kind has (T-NeRF takes L_dir = 1 where the others take 0: TNeRF.forward reads vdir)"""
    Lp, Ld, Lt = bands
    if kind == "canon":
        return Lp, Ld, 0
    if kind == "noview":
        return Lp, 0, 0
    if kind == "tnerf":
        return Lp, max(Ld, 1), Lt
    return Lp, Ld, Lt


def triples(kind, of=None):
    """The distinct band triples of a net kind, in TRIPLES order"""
    out = []
    for b in (TRIPLES if of is None else of):
        a = applicable(kind, b)
        if a not in out:
            out.append(a)
    return out


def widths(bands):
    Lp, Ld, Lt = bands
    return 3 * (1 + 2 * Lp), 3 * (1 + 2 * Ld), 1 + 2 * Lt


# opacity bias per (kind, bands): the multiple of 0.25 that brings the mean acc_map of the CPU oracle's coarse pass on the test
# rays closest to 0.5 (the opacity of a He-normal net swings from all 0 to all 1 with the seed and the input width);
# test_bands_host.test_opacity_is_not_degenerate holds every case to 0.05 < mean acc < 0.95.  NOVIEW (1, 0, 0) takes the next step,
# -1.0: at -1.25 the reference's own resampled depths move in 37 of 2368 elements between its fp32 and float64 coarse weights,
# more than the 1 % the depth gate allows anyone (at -1.0: 1 element; the host test holds every case inside that gate)
ALPHA_BIAS = {
    ("canon", (0, 0, 0)): 0.5, ("canon", (1, 1, 0)): -1.0, ("canon", (5, 2, 0)): -2.0, ("canon", (6, 3, 0)): -0.75,
    ("canon", (9, 4, 0)): 0.5, ("canon", (10, 0, 0)): -1.75, ("canon", (10, 4, 0)): -1.25,
    ("noview", (0, 0, 0)): 0.0, ("noview", (1, 0, 0)): -1.0, ("noview", (5, 0, 0)): -1.25, ("noview", (6, 0, 0)): -0.75,
    ("noview", (9, 0, 0)): -0.5, ("noview", (10, 0, 0)): -0.75,
    ("dnerf", (0, 0, 0)): 1.5, ("dnerf", (1, 1, 1)): -0.75, ("dnerf", (5, 2, 4)): -0.5, ("dnerf", (6, 3, 9)): -1.0,
    ("dnerf", (9, 4, 10)): -0.25, ("dnerf", (10, 0, 0)): -1.5, ("dnerf", (10, 4, 10)): -0.5,
    ("tnerf", (0, 1, 0)): 0.5, ("tnerf", (1, 1, 1)): -0.75, ("tnerf", (5, 2, 4)): -1.25, ("tnerf", (6, 3, 9)): 0.75,
    ("tnerf", (9, 4, 10)): -0.25, ("tnerf", (10, 1, 0)): -1.25, ("tnerf", (10, 4, 10)): -0.5,
}


def weights(kind, bands, seed=0):
    """numpy state_dict of the net of `kind` at `bands` (reference parameter names and shapes)"""
    Cp, Cd, Ct = widths(applicable(kind, bands))
    s = 20251000 + 100 * KINDS.index(kind) + seed
    bias = ALPHA_BIAS[(kind, applicable(kind, bands))]
    if kind == "canon":
        return synth.nerf_state_dict(s, Cp, Cd, alpha_bias=bias)
    if kind == "noview":
        return synth.noview_state_dict(s, Cp, 5, alpha_bias=bias)
    if kind == "dnerf":
        return synth.dnerf_state_dict(s, Cp, Cd, Ct, alpha_bias=bias)
    return synth.tnerf_state_dict(s, Cp, Cd, Ct, density_bias=bias)


def _spread(w, blocks):
    """w [out, sum(have)] with column blocks [(have, want), ...]: each block padded with zero columns to `want`"""
    out, o = [], 0
    for have, want in blocks:
        out.append(w[:, o:o + have])
        out.append(np.zeros((w.shape[0], want - have), w.dtype))
        o += have
    assert o == w.shape[1], (o, w.shape)
    return np.ascontiguousarray(np.concatenate(out, 1))


def widen(kind, sd, bands):
    """The (10, 4, 10) state_dict (T-NeRF, static: the members they have) whose extra input columns are zero"""
    Cp, Cd, Ct = widths(applicable(kind, bands))
    out = dict(sd)
    if kind == "tnerf":
        W = 128
        out["layers.0.0.weight"] = _spread(sd["layers.0.0.weight"], [(Cp, 63), (Ct, 21)])
        out["layers.5.0.weight"] = _spread(sd["layers.5.0.weight"], [(Cp, 63), (Ct, 21), (W, W)])
        out["layer_9.0.weight"] = _spread(sd["layer_9.0.weight"], [(W, W), (Cd, 27)])
        return out
    W = 256
    p = "_occ." if kind == "dnerf" else ""
    out[p + "pts_linears.0.weight"] = _spread(sd[p + "pts_linears.0.weight"], [(Cp, 63)])
    out[p + "pts_linears.5.weight"] = _spread(sd[p + "pts_linears.5.weight"], [(Cp, 63), (W, W)])
    if kind != "noview":
        out[p + "views_linears.0.weight"] = _spread(sd[p + "views_linears.0.weight"], [(W, W), (Cd, 27)])
    if kind == "dnerf":
        out["_time.0.weight"] = _spread(sd["_time.0.weight"], [(Cp, 63), (Ct, 21)])
        out["_time.5.weight"] = _spread(sd["_time.5.weight"], [(Cp, 63), (W, W)])
    return out


def wide_bands(kind):
    return applicable(kind, CONTROL)


def shared_columns(kind, name, bands):
    """Column index (into the WIDE tensor) of every column of the narrow tensor `name`, or None when the tensor is not widened"""
    Cp, Cd, Ct = widths(applicable(kind, bands))
    W = 128 if kind == "tnerf" else 256
    r = np.arange
    table = {"layers.0.0.weight": [r(Cp), 63 + r(Ct)], "layers.5.0.weight": [r(Cp), 63 + r(Ct), 84 + r(W)],
             "layer_9.0.weight": [r(W), W + r(Cd)], "pts_linears.0.weight": [r(Cp)], "pts_linears.5.weight": [r(Cp), 63 + r(W)],
             "views_linears.0.weight": [r(W), W + r(Cd)], "_time.0.weight": [r(Cp), 63 + r(Ct)], "_time.5.weight": [r(Cp), 63 + r(W)]}
    key = name[len("_occ."):] if name.startswith("_occ.") else name
    if key not in table or (kind == "noview" and key == "views_linears.0.weight"):
        return None
    return np.concatenate(table[key])


def ray_batch(kind, n=N_RAYS, seed=7, t=FRAME_TIME):
    """[o, d, near, far (, t), viewdirs] rows as render() packs them (float32); NOVIEW: 8 columns"""
    g = cases.g8_inputs(n=n) if seed is None else cases.g7_inputs(n=n, seed=seed)
    o, d = g["rays_o"].astype(np.float32), g["rays_d"].astype(np.float32)
    vd = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)
    one = np.ones((n, 1), np.float32)
    cols = [o, d, 2.0 * one, 6.0 * one]
    if kind in ("dnerf", "tnerf"):
        cols.append(np.float32(t) * one)
    if kind != "noview":
        cols.append(vd)
    return np.concatenate(cols, -1).astype(np.float32)


# gradient cases: n <= 12 rays, S = 33 (a ragged tile), n no multiple of 4.  Ray seeds per (kind, bands) scanned on the CPU so
# that the float64 evaluation has no ReLU unit within 5e-6 of its kink (bands_ref.risky_units; test_bands_host asserts it).
GRAD_N, GRAD_S = 5, 33
GRAD_SEEDS = {("canon", (0, 0, 0)): 303, ("canon", (6, 3, 0)): 302, ("canon", (10, 4, 0)): 305,
              ("noview", (0, 0, 0)): 302, ("noview", (6, 0, 0)): 301, ("noview", (10, 0, 0)): 301,
              ("dnerf", (0, 0, 0)): 305, ("dnerf", (6, 3, 9)): 304, ("dnerf", (10, 4, 10)): 318,
              ("tnerf", (0, 1, 0)): 300, ("tnerf", (6, 3, 9)): 300, ("tnerf", (10, 4, 10)): 300}


def grad_rays(kind, bands):
    return ray_batch(kind, n=GRAD_N, seed=GRAD_SEEDS[(kind, applicable(kind, bands))])
