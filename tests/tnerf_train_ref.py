"""float64 yardsticks of the fused T-NeRF training pass (tests/test_gpu_tnerf_train.py, tests/test_tnerf_train_host.py):
the flip-aware gradient check of tnerf_ref.py with a render that also takes sigma noise and returns disp_map and raw (so that
losses on disp_map and on the returned raw can be checked), and the un-fold algebra of `feature` folded into `layer_9`."""
import numpy as np
import torch

import tnerf_ref as R


def render64(sd, rb, z, white_bkgd, flips=None, pres=None, noise=None, Lp=10, Ld=4, Lt=10):
    """tnerf_ref._render64 with `noise` [n,S] added to sigma in front of raw2outputs' ReLU (run_tnerf.py:367-374) and the outputs
    disp_map and raw = [relu(colour), sigma] besides rgb_map / acc_map.  pres: [colour pre-activation [M,3], sigma + noise [M,1]]"""
    n, S = z.shape
    o, d, vd = rb[:, 0:3], rb[:, 3:6], rb[:, 9:12]
    pts = (o[:, None, :] + d[:, None, :] * z[..., None]).reshape(-1, 3)
    ep = R.embed(pts, Lp).double()
    et = R.embed(rb[:, 8:9][:, None].expand(n, S, 1).reshape(-1, 1), Lt).double()
    ed = R.embed(vd[:, None].expand(n, S, 3).reshape(-1, 3), Ld).double()
    f = lambda name, x: torch.nn.functional.linear(x, sd[name + ".weight"], sd[name + ".bias"])

    def relu(i, pre):
        if pres is not None:
            pres.append(pre.detach())
        m = pre.detach() > 0
        if flips is not None and i in flips:
            m = m ^ flips[i]
        return pre * m
    inp = torch.cat([ep, et], -1)
    x = inp
    for i in range(8):
        x = torch.nn.functional.elu(f(f"layers.{i}.0", x))
        if i == 4:
            x = torch.cat([inp, x], -1)
    sigma = f("density.0", x)
    h9 = torch.nn.functional.elu(f("layer_9.0", torch.cat([f("feature.0", x), ed], -1)))
    rgb_raw = relu(0, f("color.0", h9)).reshape(n, S, 3)
    pre_sig = sigma if noise is None else sigma + noise.double().reshape(-1, 1)
    sig = relu(1, pre_sig).reshape(n, S)
    zd = z.double()
    dists = torch.cat([zd[..., 1:] - zd[..., :-1], torch.full_like(zd[..., :1], 1e10)], -1) * torch.norm(d.double()[:, None, :], dim=-1)
    alpha = 1. - torch.exp(-sig * dists)
    w = alpha * torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1. - alpha + 1e-10], -1), -1)[:, :-1]
    rgb = torch.sum(w[..., None] * torch.sigmoid(rgb_raw), -2)
    acc = torch.sum(w, -1)
    depth = torch.sum(w * zd, -1)
    disp = 1. / torch.max(1e-10 * torch.ones_like(depth), depth / acc)
    if white_bkgd:
        rgb = rgb + (1. - acc[..., None])
    return {"rgb_map": rgb, "acc_map": acc, "disp_map": disp, "raw": torch.cat([rgb_raw, sigma.reshape(n, S, 1)], -1)}


def risky_units(sd32, rb, z, noise=None, thr=5e-6, bands=(10, 4, 10)):
    """How many ReLU units (colour head, sigma) lie within thr of the kink in float64: a CPU quantity (flip_aware_check caps it at 400)."""
    pres = []
    with torch.no_grad():
        render64({k: v.double() for k, v in sd32.items()}, rb, z, True, pres=pres, noise=noise, Lp=bands[0], Ld=bands[1], Lt=bands[2])
    return sum(int((p.abs() < thr).sum()) for p in pres)


def flip_aware_check(sd32, rb, z, white_bkgd, ray_loss, gpu_grads, what, noise=None, thr=5e-6, rtol=2e-5, bands=(10, 4, 10), stats=None):
    """tnerf_ref.flip_aware_check over render64 (same method, same gate): ray_loss(ret, idx) sees disp_map and raw as well, and
    `noise` [n,S] is the sigma noise of the pass.  Returns (#flips, #risky)."""
    n, S = z.shape
    names = list(gpu_grads)
    sd = {k: v.double().requires_grad_(True) for k, v in sd32.items()}

    def grads(idx, flips=None, pres=None):
        for v in sd.values():
            v.grad = None
        ray_loss(render64(sd, rb[idx], z[idx], white_bkgd, flips, pres, None if noise is None else noise[idx], *bands), idx).backward()
        return torch.cat([(sd[k].grad if sd[k].grad is not None else torch.zeros_like(sd[k])).reshape(-1) for k in names])

    pres = []
    truth = grads(torch.arange(n), pres=pres)
    risky = [(l, int(r), int(u)) for l, p in enumerate(pres) for r, u in torch.nonzero(p.abs() < thr).tolist()]
    assert len(risky) <= 400, f"{what}: {len(risky)} units within {thr} of the kink - pick better conditioned inputs"
    cols = []
    for l, row, u in risky:
        ray = torch.tensor([row // S])
        fl = torch.zeros((S, pres[l].shape[1]), dtype=torch.bool)
        fl[row % S, u] = True
        cols.append(grads(ray, {l: fl}) - grads(ray))
    ours = torch.cat([gpu_grads[k].detach().double().cpu().reshape(-1) for k in names])
    diff = ours - truth
    flips = 0
    if cols:
        Dm = torch.stack(cols, 1)
        live = Dm.abs().max(0).values > 1e-3 * rtol * truth.abs().max()
        Dm = Dm[:, live]
        if Dm.shape[1]:
            c = torch.from_numpy(np.linalg.lstsq(Dm.numpy(), diff.numpy()[:, None], rcond=None)[0][:, 0])
            cr = c.round().clamp(0, 1)
            amb = (c - cr).abs() * Dm.abs().max(0).values
            bad = ((c - cr).abs() > 0.05) & (amb > 0.25 * rtol * truth.abs().max())
            assert not bool(bad.any()), f"{what}: flip coefficients {c[bad].tolist()} are not 0 / 1"
            diff = diff - Dm @ cr
            flips = int(cr.sum())
    o, worst = 0, 0.0
    for k in names:
        m = gpu_grads[k].numel()
        dd, scale = float(diff[o:o + m].abs().max()), max(float(truth[o:o + m].abs().max()), 1e-12)
        print(f"{what} {k}: {dd:.3e} of {scale:.3e} ({dd / scale:.2e})")
        assert dd <= rtol * scale, f"{what} {k}: {dd:.3e} of {scale:.3e} ({dd / scale:.2e}) after {flips} flips of {len(risky)} risky units"
        worst = max(worst, dd / scale)
        o += m
    if stats is not None:
        stats["worst"] = worst
    return flips, len(risky)


# ---- the un-fold: layer_9 on [feature(h7) | gamma(d)] run as ONE layer through W' = W9f . Wf, b' = W9f . bf + b9 ------------
def unfold(G, dbp, W9f, Wf, bf):
    """G = sum_rows d pre_9 (x) h7 [64,128], dbp = sum_rows d pre_9 [64]  ->  (d layer_9.weight[:, :128], d feature.weight,
    d feature.bias) of the unfolded two-layer form (numpy float64; what swnerf_tnerf_feature_finish evaluates in fp32)."""
    return G @ Wf.T + np.outer(dbp, bf), W9f.T @ G, W9f.T @ dbp
