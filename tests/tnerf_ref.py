"""A float64 torch restatement of TNeRF (model.py:152-210) and of render_rays / raw2outputs of t_nerf/run_tnerf.py
(:349-500), written for the tests: positional encodings in float32 (as the runner computes them), everything after in
float64.  Works on CPU or GPU tensors; differentiable in the weights."""
import torch


def embed(x, L):
    """[x, sin(2^0 x), cos(2^0 x), ..., sin(2^(L-1) x), cos(2^(L-1) x)] in float32 (embedder.py:33-42)"""
    x = x.float()
    out = [x]
    for k in range(L):
        out += [torch.sin(x * float(2 ** k)), torch.cos(x * float(2 ** k))]
    return torch.cat(out, -1)


def forward(sd, inp, vdir, dyn_t, in_feat=63, depth=8, skip_layer=4):
    """TNeRF.forward on float64 parameters `sd` (state_dict names) -> [M, 4]"""
    f = lambda name, x: torch.nn.functional.linear(x, sd[name + ".weight"], sd[name + ".bias"])
    inp = torch.cat([inp[:, :in_feat].double(), dyn_t.double()], -1)
    x = inp
    for i in range(depth):
        x = torch.nn.functional.elu(f(f"layers.{i}.0", x))
        if i % skip_layer == 0 and i > 0:
            x = torch.cat([inp, x], -1)
    sigma = f("density.0", x)
    x = torch.cat([f("feature.0", x), vdir.double()], -1)
    x = torch.nn.functional.elu(f("layer_9.0", x))
    rgb = torch.relu(f("color.0", x))
    return torch.cat([rgb, sigma], -1)


def coarse_z(rb, S, lindisp=False, t_rand=None):
    """run_tnerf.py:452-468 in float32 (the runner's own arithmetic)"""
    near, far = rb[:, 6:7], rb[:, 7:8]
    t = torch.linspace(0., 1., steps=S, device=rb.device)
    z = near * (1. - t) + far * t if not lindisp else 1. / (1. / near * (1. - t) + 1. / far * t)
    z = z.expand([rb.shape[0], S])
    if t_rand is not None:
        mids = .5 * (z[..., 1:] + z[..., :-1])
        upper = torch.cat([mids, z[..., -1:]], -1)
        lower = torch.cat([z[..., :1], mids], -1)
        z = lower + (upper - lower) * t_rand
    return z


def render_rays(sd, rb, S, z_vals=None, lindisp=False, t_rand=None, noise=None, white_bkgd=False, Lp=10, Ld=4, Lt=10):
    """render_rays + raw2outputs (run_tnerf.py:349-500) with the network in float64 -> dict rgb_map disp_map acc_map raw z_vals"""
    rb = rb.float()
    z = coarse_z(rb, S, lindisp, t_rand) if z_vals is None else z_vals.float()
    N = rb.shape[0]
    o, d, vd = rb[:, 0:3], rb[:, 3:6], rb[:, 9:12]
    pts = (o[:, None, :] + d[:, None, :] * z[..., None]).reshape(-1, 3)
    M = pts.shape[0]
    ep = embed(pts, Lp)
    et = embed(rb[:, 8:9][:, None].expand(N, S, 1).reshape(-1, 1), Lt)
    ed = embed(vd[:, None].expand(N, S, 3).reshape(-1, 3), Ld)
    raw = forward(sd, ep, ed, et, in_feat=ep.shape[1]).reshape(N, S, 4)
    zd = z.double()
    dists = torch.cat([zd[..., 1:] - zd[..., :-1], torch.full_like(zd[..., :1], 1e10)], -1) * torch.norm(d.double()[:, None, :], dim=-1)
    sig = raw[..., 3] + (0. if noise is None else noise.double())
    alpha = 1. - torch.exp(-torch.relu(sig) * dists)
    w = alpha * torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1. - alpha + 1e-10], -1), -1)[:, :-1]
    rgb = torch.sum(w[..., None] * torch.sigmoid(raw[..., :3]), -2)
    depth = torch.sum(w * zd, -1)
    acc = torch.sum(w, -1)
    disp = 1. / torch.max(1e-10 * torch.ones_like(depth), depth / acc)
    if white_bkgd:
        rgb = rgb + (1. - acc[..., None])
    return {"rgb_map": rgb, "disp_map": disp, "acc_map": acc, "raw": raw, "z_vals": z}


# ---- gradient parity that is immune to ReLU conditioning (the method of tests/flipcheck.py, for TNeRF) ------------------
# ELU is C1, so only the two ReLUs can put fp32 and float64 on different branches: the colour head's (model.py:188-189) and
# raw2outputs' relu on sigma (run_tnerf.py:357).  Every unit whose float64 pre-activation lies within `thr` of the kink gets the
# exact effect D_k of flipping its mask (the difference of two evaluations of its ray); the GPU gradient must equal
# truth + sum_k c_k D_k with every c_k in {0, 1}, up to `rtol` of each tensor's max.
def _render64(sd, rb, z, white_bkgd, flips=None, pres=None, Lp=10, Ld=4, Lt=10):
    n, S = z.shape
    o, d, vd = rb[:, 0:3], rb[:, 3:6], rb[:, 9:12]
    pts = (o[:, None, :] + d[:, None, :] * z[..., None]).reshape(-1, 3)
    ep = embed(pts, Lp).double()
    et = embed(rb[:, 8:9][:, None].expand(n, S, 1).reshape(-1, 1), Lt).double()
    ed = embed(vd[:, None].expand(n, S, 3).reshape(-1, 3), Ld).double()
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
    sig = relu(1, sigma).reshape(n, S)
    zd = z.double()
    dists = torch.cat([zd[..., 1:] - zd[..., :-1], torch.full_like(zd[..., :1], 1e10)], -1) * torch.norm(d.double()[:, None, :], dim=-1)
    alpha = 1. - torch.exp(-sig * dists)
    w = alpha * torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1. - alpha + 1e-10], -1), -1)[:, :-1]
    rgb = torch.sum(w[..., None] * torch.sigmoid(rgb_raw), -2)
    acc = torch.sum(w, -1)
    if white_bkgd:
        rgb = rgb + (1. - acc[..., None])
    return {"rgb_map": rgb, "acc_map": acc}


def flip_aware_check(sd32, rb, z, white_bkgd, ray_loss, gpu_grads, what, thr=5e-6, rtol=2e-5):
    """sd32: the net's fp32 state_dict (CPU tensors); rb [n,12], z [n,S] fp32 CPU; ray_loss(ret, idx) -> scalar, the loss of rays
    idx (the total loss is its sum over a partition of the rays); gpu_grads {name: tensor}.  Returns (#flips, #risky)."""
    import numpy as np
    n, S = z.shape
    names = list(gpu_grads)
    sd = {k: v.double().requires_grad_(True) for k, v in sd32.items()}

    def grads(idx, flips=None, pres=None):
        for v in sd.values():
            v.grad = None
        ray_loss(_render64(sd, rb[idx], z[idx], white_bkgd, flips, pres), idx).backward()
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
    o = 0
    for k in names:
        m = gpu_grads[k].numel()
        dd, scale = float(diff[o:o + m].abs().max()), max(float(truth[o:o + m].abs().max()), 1e-12)
        assert dd <= rtol * scale, f"{what} {k}: {dd:.3e} of {scale:.3e} ({dd / scale:.2e}) after {flips} flips of {len(risky)} risky units"
        o += m
    return flips, len(risky)
