"""References of the fused passes at any embedder band count (tests/test_gpu_bands.py, tests/test_bands_host.py): the four
net kinds as one function of (kind, state_dict, ray batch, depths, bands), evaluated through the CPU oracle
(oracle.nerf_oracle, fp32 - what the reference computes) or in float64 on the fp32 encodings the reference forms.
Test infrastructure, like tnerf_ref.py and dnerf_ref.py."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import nerf_oracle as O

import cases_bands as CB


def sd_of(sd_np, dtype):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dtype) for k, v in sd_np.items()}


def tnerf_mlp(sd, ex, et, ed):
    """TNeRF.forward (model.py:152-210, depth 8, skip_layer 4) in the dtype of its operands -> [M, 4] = [relu(colour), sigma]"""
    f = lambda name, x: F.linear(x, sd[name + ".weight"], sd[name + ".bias"])
    inp = torch.cat([ex, et], -1)
    x = inp
    for i in range(8):
        x = F.elu(f(f"layers.{i}.0", x))
        if i == 4:
            x = torch.cat([inp, x], -1)
    sigma = f("density.0", x)
    x = F.elu(f("layer_9.0", torch.cat([f("feature.0", x), ed], -1)))
    return torch.cat([torch.relu(f("color.0", x)), sigma], -1)


def rows_ref(kind, sd_np, pts, dirs, t, bands, dtype=torch.float64):
    """The net of `kind` on M points: pts [M,3], dirs [M,3] (ignored by NOVIEW), one frame time t (DNERF / TNERF) -> (raw
    [M, 4 | 5], dx [M,3] | None).  Encodings in fp32 (embedder.py:33-42 as the runners call it), everything after in `dtype`."""
    Lp, Ld, Lt = CB.applicable(kind, bands)
    sd = sd_of(sd_np, dtype)
    ex = O.embed(pts.float(), Lp).to(dtype)
    ed = O.embed(dirs.float(), Ld).to(dtype)
    if kind == "canon":
        return O.nerf_mlp(sd, torch.cat([ex, ed], -1), ex.shape[1], ed.shape[1]), None
    if kind == "noview":
        return O.generic_mlp(sd, ex, 8, [4], ex.shape[1], 0, False), None
    et = O.embed(torch.full((pts.shape[0], 1), float(np.float32(t)), dtype=torch.float32), Lt).to(dtype)
    if kind == "tnerf":
        return tnerf_mlp(sd, ex, et, ed), None
    out, dx = O.dnerf_mlp(sd, torch.cat([ex, ed], -1), et, multires=Lp, input_ch=ex.shape[1], input_ch_views=ed.shape[1])
    return out, dx


def pass_ref(kind, sd_np, rb, z, bands, white_bkgd, dtype=torch.float32):
    """One render pass (nerf/run.py:385-400, run_dnerf.py:420-440, run_tnerf.py:470-500) of rays rb (cases_bands.ray_batch
    layout, CPU tensor) at depths z [n,S] -> dict rgb_map disp_map acc_map depth_map weights raw (, dx)."""
    n, S = z.shape
    rb, z = rb.float(), z.float()
    pts = (rb[:, None, 0:3] + rb[:, None, 3:6] * z[..., None]).reshape(-1, 3)
    dirs = rb[:, None, -3:].expand(n, S, 3).reshape(-1, 3)
    t = float(rb[0, 8]) if kind in ("dnerf", "tnerf") else None
    raw, dx = rows_ref(kind, sd_np, pts, dirs, t, bands, dtype)
    raw = raw.reshape(n, S, -1)
    rgb, disp, acc, w, depth = O.raw2outputs(raw[..., :4], z.to(dtype), rb[:, 3:6].to(dtype), 0., white_bkgd)
    out = dict(rgb_map=rgb, disp_map=disp, acc_map=acc, depth_map=depth, weights=w, raw=raw)
    if dx is not None:
        out["dx"] = dx.reshape(n, S, 3)
    return out


def coarse_z(rb, S):
    return O.coarse_z(rb[:, 6:7].float(), rb[:, 7:8].float(), S)


def resample_ref(z, weights, n_importance):
    """nerf/run.py:388-400 with perturb = 0 -> (sorted union [n, S + Ni], z_std [n])"""
    mid = .5 * (z[..., 1:] + z[..., :-1])
    zs = O.sample_pdf(mid, weights[..., 1:-1].float(), n_importance, det=True)
    return torch.sort(torch.cat([z, zs], -1), -1)[0], torch.std(zs, dim=-1, unbiased=False)


# ---- the gates: the ones the same quantity already has at (10, 4, 10) -----------------------------------------------------------
# test_gpu_parity.py: colours / acc 2e-5 abs (RGB_TOL), disparity 2e-5 abs + 1e-4 rel with equal NaN pattern, raw 1e-3 abs +
# 1e-4 rel (_cmp, also D-NeRF at t != 0), position_delta 1e-6 abs, coarse depths 1e-6 abs, z_std 2e-3 abs, the sorted union
# within one coarse interval per row and 99 % within 2e-5.  test_gpu_tnerf.py: |d raw| - 1e-4 |ref| < 2e-4.
# Two gates are NEW here, no fused-pass test held these outputs against the oracle before: `weights` are the terms acc_map sums,
# from the same arithmetic, so acc_map's gate; depth_map = sum w z with z <= far, so far times acc_map's gate.  (The standalone
# raw2outputs is held to 2e-6 + 2e-5 rel on EQUAL raw in test_gpu_parity.py; here raw itself differs by the MLP's rounding.)
FAR = 6.0
GATES = {"rgb_map": (2e-5, 0.0), "acc_map": (2e-5, 0.0), "weights": (2e-5, 0.0), "disp_map": (2e-5, 1e-4), "depth_map": (FAR * 2e-5, 0.0),
         "raw": (1e-3, 1e-4), "dx": (1e-6, 0.0), "z_out": (1e-6, 0.0), "z_std": (2e-3, 0.0)}
GATES_TNERF = dict(GATES, raw=(2e-4, 1e-4))
# per-row kernels (test_gpu_parity.test_mlp_forward_golden, test_gpu_query_time.py): raw 1e-4 + 1e-4 |ref|; D-NeRF at t != 0
# 1e-3 + 1e-4 |ref|; T-NeRF as above; position_delta 1e-6
ROW_GATES = {"canon": (1e-4, 1e-4), "noview": (1e-4, 1e-4), "dnerf": (1e-3, 1e-4), "dnerf_t0": (1e-4, 1e-4), "tnerf": (2e-4, 1e-4)}


def _np(a):
    return a.detach().cpu().double().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, np.float64)


def excess(got, ref, atol, rtol, what):
    """max of |got - ref| / (atol + rtol |ref|) over every element (NaN pattern must match; NaN elements count as equal)"""
    a, b = _np(got), _np(ref)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(np.isnan(a), np.isnan(b)), f"{what}: NaN pattern differs"
    if a.size == 0:
        return 0.0, 0.0
    d = np.abs(np.nan_to_num(a) - np.nan_to_num(b))
    return float(d.max()), float((d / (atol + rtol * np.abs(np.nan_to_num(b)))).max())


def check_pass(got, ref, kind, what, keys=None):
    """Every output of a pass against its reference at the gates above.  No element is left out (NaN disparity of rays with
    acc == 0 must be NaN on both sides).  -> {key: max |delta|}"""
    gates = GATES_TNERF if kind == "tnerf" else GATES
    worst = {}
    for k in (keys or [k for k in gates if k in got and k in ref]):
        atol, rtol = gates[k]
        worst[k], ex = excess(got[k], ref[k], atol, rtol, f"{what}:{k}")
        assert ex <= 1.0, f"{what}:{k}: max |delta| {worst[k]:.3e} is {ex:.2f} x the gate ({atol:g} + {rtol:g} |ref|)"
    return worst


def own_depth_error(kind, sd_np, rb, z, bands, n_importance):
    """(resampled depths from the reference's fp32 coarse weights, from its float64 coarse weights): what a 1e-7 difference in
    the weights does to the inverse CDF on this case - (u - cdf_lo) / denom with denom down to 1e-5 and the `denom < 1e-5 -> 1`
    branch (ray.py:148-149).  The inputs of a case are chosen so that this pair sits inside check_depths' gate."""
    w32 = pass_ref(kind, sd_np, rb, z, bands, True)["weights"]
    w64 = pass_ref(kind, sd_np, rb, z, bands, True, torch.float64)["weights"].float()
    return resample_ref(z, w32, n_importance)[0], resample_ref(z, w64, n_importance)[0]


def check_depths(z_got, z_ref, S, what, frac=0.99):
    """The sorted union of coarse depths and drawn samples, the gate of test_gpu_parity._cmp 'z_vals': every element within one
    coarse interval of its row (S coarse depths), and `frac` of them within 2e-5 - 0.99, and 0.9 for D-NeRF at t != 0 (the gate
    of test_render_rays_dnerf_golden, where gamma(x + dx) amplifies the rounding of dx in front of the coarse weights).
    -> number of elements that differ by more than 2e-5"""
    gz, rz = _np(z_got), _np(z_ref)
    assert gz.shape == rz.shape, (what, gz.shape, rz.shape)
    row_bound = (rz[:, -1:] - rz[:, :1]) / (S - 1.0) * 1.0001 + 1e-6
    d = np.abs(gz - rz)
    assert np.all(d <= row_bound), f"{what}: an element moved by more than one coarse interval"
    nfl = int((d > 2e-5).sum())
    assert nfl <= (1.0 - frac) * d.size, f"{what}: {nfl} of {d.size} depths differ by > 2e-5 (need {frac} of them within)"
    return nfl


def fmt(worst):
    return ", ".join(f"{k} {v:.2e}" for k, v in worst.items())


# ---- gradient cases ---------------------------------------------------------------------------------------------------------------
def risky_units(kind, sd_np, rb, z, bands, thr=5e-6):
    """How many ReLU units of the float64 evaluation lie within thr of the kink on the samples of rays rb at depths z (what the
    flip-aware checks would have to account for).  D-NeRF: x' taken from the float64 deformation net rounded to fp32 (the
    evaluation under test supplies its own on the GPU)."""
    import dnerf_ref
    import flipcheck
    import tnerf_train_ref
    Lp, Ld, Lt = CB.applicable(kind, bands)
    if kind == "tnerf":
        return tnerf_train_ref.risky_units({k: torch.from_numpy(v) for k, v in sd_np.items()}, rb, z, bands=(Lp, Ld, Lt), thr=thr)
    sd = sd_of(sd_np, torch.float64)
    n, S = z.shape
    with torch.no_grad():
        if kind == "dnerf":
            ex, et, ed, x = dnerf_ref.ray_encodings(rb, z, bands=(Lp, Ld, Lt))
            run = float(rb[0, 8]) != 0.0
            dxv = dnerf_ref.deform64(sd, ex.double(), et.double()).float() if run else torch.zeros((n * S, 3))
            pres = {}
            dnerf_ref.mlp64(sd, ex.double(), et.double(), ed.double(), x, dxv, pres=pres, run_deform=run, L_pos=Lp)
            pres = list(pres.values())
        else:
            pts = (rb[:, None, 0:3] + rb[:, None, 3:6] * z[..., None]).reshape(-1, 3)
            e = O.embed(pts, Lp)
            if kind == "canon":
                e = torch.cat([e, O.embed(rb[:, None, -3:].expand(n, S, 3).reshape(-1, 3), Ld)], -1)
            pres = []
            flipcheck._mlp64(sd, e.double(), pres=pres, Cpos=3 * (1 + 2 * Lp))
    return sum(int((p.abs() < thr).sum()) for p in pres)
