"""A float64 restatement of DirectTemporalNeRF (model.py:128-151) and the ReLU-flip-aware gradient check of
tests/flipcheck.py for it (test infrastructure; uses the CPU oracle for raw2outputs and the encodings).

The D-NeRF net re-embeds x' = x + dx: gamma()'s top band multiplies a 1e-7 difference in dx by 512, so a float64 truth
evaluated at ITS OWN dx sits ~5e-5 from any fp32 evaluation and finds the ReLUs near their kink at the wrong point.  The
truth here therefore takes the VALUE of x' from the evaluation under test, x' = fl32(x + dx_value), and its GRADIENT from
the float64 graph: `xp = (x32 + dx_value).double() + (dx64 - dx64.detach())`, the device oracle.nerf_oracle.dnerf_mlp
uses in fp32.  Everything else is the method of flipcheck.py: every unit with |pre-activation| < thr in float64 gets the
exact effect D_k of flipping its mask, and the gradient under test must equal truth + sum_k c_k D_k with c_k in {0, 1}
up to `rtol` of each tensor's max.

Layers are numbered 0..7 = `_time.*`, 8..15 = `_occ.pts_linears.*`, 16 = `_occ.views_linears.0`."""
import numpy as np
import torch

from oracle import nerf_oracle as O

N_LAYERS = 17


def embed64(x, L=10):
    """gamma(x) in the dtype of x (float64 here), differentiable: [x, sin(2^k x), cos(2^k x) ...], embedder.py:33-42"""
    out = [x]
    for k in range(L):
        out += [torch.sin(x * float(2 ** k)), torch.cos(x * float(2 ** k))]
    return torch.cat(out, -1)


def _relu(i, pre, flips, pres):
    if pres is not None:
        pres[i] = pre.detach()
    m = pre.detach() > 0
    if flips is not None and i in flips:
        m = m ^ flips[i]
    return pre * m


def deform64(sd, ex, et, flips=None, pres=None):
    """query_time (model.py:128-136) in float64 on the encodings gamma(x) [M,63], gamma(t) [M,21] (the widths of the default
    bands; any others are taken from the operands) -> dx [M,3]"""
    lin = lambda name, x: x @ sd[name + ".weight"].T + sd[name + ".bias"]
    h = torch.cat([ex, et], -1)
    for i in range(8):
        h = _relu(i, lin(f"_time.{i}", h), flips, pres)
        if i == 4:
            h = torch.cat([ex, h], -1)
    return lin("_time_out", h)


def mlp64(sd, ex, et, ed, x32, dx_value, flips=None, pres=None, run_deform=True, detach_bands=(), L_pos=10):
    """DirectTemporalNeRF.forward (model.py:128-151) in float64 with the ReLUs written as masks.  sd: float64 parameters
    (state_dict names); ex / et / ed: the fp32 encodings gamma(x) [M,63], gamma(t) [M,21], gamma(d) [M,27] the reference
    forms, cast to float64; x32 [M,3] fp32, dx_value [M,3] fp32: x' takes its value from x32 + dx_value in fp32 (and its
    encoding's value from the fp32 encoding of that), its gradient from the float64 dx.  flips / pres: {layer: bool
    [M, units]} / dict that receives {layer: pre-activation}.  run_deform=False (t == 0 with zero_canonical, model.py:143-145):
    dx = 0 and only `_occ` is evaluated.  detach_bands (tests of the checker only): frequency bands k of gamma(x') whose
    sin / cos columns carry no gradient to x'.  L_pos: the bands of gamma(x') (ex is 3(1+2 L_pos) wide).  Returns (raw [M,4], dx [M,3])."""
    lin = lambda name, x: x @ sd[name + ".weight"].T + sd[name + ".bias"]
    if run_deform:
        dx = deform64(sd, ex, et, flips, pres)
        xp32 = x32 + dx_value                                        # model.py:147 as the evaluation under test rounds it
        xp = xp32.double() + (dx - dx.detach())
        g = embed64(xp, L_pos)
        if detach_bands:
            keep = torch.ones(g.shape[1], dtype=torch.bool)
            for k in detach_bands:
                keep[3 + 6 * k:9 + 6 * k] = False
            g = torch.where(keep, g, g.detach())
        pts = O.embed(xp32, L_pos).double() + (g - g.detach())
    else:
        dx = torch.zeros((ex.shape[0], 3), dtype=torch.float64)
        pts = ex
    h = pts
    for i in range(8):
        h = _relu(8 + i, lin(f"_occ.pts_linears.{i}", h), flips, pres)
        if i == 4:
            h = torch.cat([pts, h], -1)
    sigma = lin("_occ.alpha_linear", h)
    hv = _relu(16, lin("_occ.views_linears.0", torch.cat([lin("_occ.feature_linear", h), ed], -1)), flips, pres)
    return torch.cat([lin("_occ.rgb_linear", hv), sigma], -1), dx


class Truth:
    """The float64 graph of one pass over n units ("rays") of S rows each.  enc = (ex, et, ed, x32), fp32 [n*S, .];
    dx_value [n*S,3] fp32; compose: dict(z [n,S], rays_d [n,3], white_bkgd, noise [n,S] | None) or None (no compositing:
    the loss sees raw and position_delta only); second: (gamma(x2), gamma(t2)), fp32 [n*S, .], the inputs of a second evaluation of
    the deformation net alone whose dx the loss sees as position_delta_2 (the TV operand of run_dnerf.py:690-725), or None."""

    def __init__(self, sd_np, names, n, S, enc, dx_value, run_deform, compose, ray_loss, second=None, detach_bands=(), L_pos=10):
        self.sd = {k: v.double().requires_grad_(True) for k, v in O.to_torch_sd(sd_np).items()}
        self.names, self.n, self.S = list(names), n, S
        ex, et, ed, x32 = enc
        self.ex, self.et, self.ed = (a.double().reshape(n, S, -1) for a in (ex, et, ed))
        self.x32, self.dxv = x32.float().reshape(n, S, 3), dx_value.float().reshape(n, S, 3)
        self.run_deform, self.compose, self.ray_loss, self.detach_bands = run_deform, compose, ray_loss, detach_bands
        self.L_pos = L_pos
        self.second = None if second is None else tuple(a.double().reshape(n, S, -1) for a in second)     # (ex2, et2)

    def grads(self, idx, flips=None, pres=None, flips2=None, pres2=None):
        """d ray_loss(rays idx) / d every parameter in `names`, concatenated; flips / pres of the pass, flips2 / pres2 of
        the second deformation-net evaluation (rows = len(idx) * S)."""
        sd, S, m = self.sd, self.S, len(idx)
        for v in sd.values():
            v.grad = None
        flat = lambda a: a[idx].reshape(m * S, -1)
        raw, dx = mlp64(sd, flat(self.ex), flat(self.et), flat(self.ed), flat(self.x32), flat(self.dxv), flips, pres,
                        self.run_deform, self.detach_bands, self.L_pos)
        raw, dx = raw.reshape(m, S, 4), dx.reshape(m, S, 3)
        ret = {"raw": raw, "position_delta": dx}
        if self.compose is not None:
            c = self.compose
            raw_c = raw if c["noise"] is None else torch.cat([raw[..., :3], raw[..., 3:4] + c["noise"][idx].double()[..., None]], -1)
            rgb, disp, acc, _, _ = O.raw2outputs(raw_c, c["z"][idx].double(), c["rays_d"][idx].double(), 0., c["white_bkgd"])
            ret.update(rgb_map=rgb, disp_map=disp, acc_map=acc)
        if self.second is not None:
            ret["position_delta_2"] = deform64(sd, flat(self.second[0]), flat(self.second[1]), flips2, pres2).reshape(m, S, 3)
        loss = self.ray_loss(ret, idx)
        if loss.requires_grad:
            loss.backward()
        return torch.cat([(sd[k].grad if sd[k].grad is not None else torch.zeros_like(sd[k])).reshape(-1) for k in self.names])

    def named(self, flat):
        out, o = {}, 0
        for k in self.names:
            m = self.sd[k].numel()
            out[k] = flat[o:o + m].reshape(self.sd[k].shape).clone()
            o += m
        return out


def _check(T, gpu_grads, what, thr, rtol):
    """flipcheck.flip_aware_check's algorithm and constants on a Truth.  Returns (flips, risky, worst residual / max)."""
    n, S, names = T.n, T.S, T.names
    pres, pres2 = {}, {}
    truth = T.grads(torch.arange(n), pres=pres, pres2=pres2)
    risky = [(w, l, int(r), int(u)) for w, pp in enumerate((pres, pres2)) for l in sorted(pp)
             for r, u in torch.nonzero(pp[l].abs() < thr).tolist()]
    assert len(risky) <= 400, f"{what}: {len(risky)} units within {thr} of the kink - pick better conditioned inputs"
    cols, base = [], {}
    for w, l, row, u in risky:
        ray = row // S
        if ray not in base:
            base[ray] = T.grads(torch.tensor([ray]))
        f = torch.zeros((S, (pres, pres2)[w][l].shape[1]), dtype=torch.bool)
        f[row % S, u] = True
        cols.append(T.grads(torch.tensor([ray]), **{("flips", "flips2")[w]: {l: f}}) - base[ray])
    zero = lambda k: torch.zeros(T.sd[k].numel(), dtype=torch.float64)
    ours = torch.cat([zero(k) if gpu_grads[k] is None else gpu_grads[k].detach().double().cpu().reshape(-1) for k in names])
    diff = ours - truth
    flips = 0
    if cols:
        Dm = torch.stack(cols, 1)
        live = Dm.abs().max(0).values > 1e-3 * rtol * truth.abs().max()       # a flip of a unit no gradient reaches cannot be told
        Dm, units = Dm[:, live], [risky[i] for i in torch.nonzero(live)[:, 0].tolist()]
        if units:
            c = torch.from_numpy(np.linalg.lstsq(Dm.numpy(), diff.numpy()[:, None], rcond=None)[0][:, 0])
            cr = c.round().clamp(0, 1)
            # (flipcheck.py) a coefficient off 0 / 1 only matters if its column can be told from fp32 summation noise
            amb = (c - cr).abs() * Dm.abs().max(0).values
            bad = ((c - cr).abs() > 0.05) & (amb > 0.25 * rtol * truth.abs().max())
            assert not bool(bad.any()), f"{what}: flip coefficients {c[bad].tolist()} are not 0 / 1 (units {[units[i] for i in torch.nonzero(bad)[:, 0].tolist()]})"
            diff = diff - Dm @ cr
            flips = int(cr.sum())
    o, worst = 0, 0.0
    for k in names:
        m = T.sd[k].numel()
        d, scale = float(diff[o:o + m].abs().max()), max(float(truth[o:o + m].abs().max()), 1e-12)
        if float(truth[o:o + m].abs().max()) > 0:
            worst = max(worst, d / scale)
        assert d <= rtol * scale, f"{what} {k}: {d:.3e} of {scale:.3e} ({d / scale:.2e}) after accounting for {flips} ReLU flips of {len(risky)} risky units"
        o += m
    return flips, len(risky), worst


def ray_encodings(rb, z, t=None, bands=(10, 4, 10)):
    """The fp32 encodings the reference forms for the samples of rays rb [n,12] at depths z [n,S] (run_dnerf.py:46-83):
    (gamma(x) [n*S,63], gamma(t) [n*S,21], gamma(d) [n*S,27], x [n*S,3]) at the default bands = (L_pos, L_dir, L_time);
    t: another frame time than column 8."""
    n, S = z.shape
    pts = (rb[:, None, 0:3] + rb[:, None, 3:6] * z[..., None]).reshape(-1, 3)
    ft = rb[:, 8:9] if t is None else torch.full((n, 1), t, dtype=torch.float32)
    et = O.embed(ft[:, None].expand(n, S, 1).reshape(-1, 1), bands[2])
    ed = O.embed(rb[:, None, -3:].expand(n, S, 3).reshape(-1, 3), bands[1])
    return O.embed(pts, bands[0]), et, ed, pts


def ray_truth(sd_np, names, rb, z, white_bkgd, ray_loss, dx_value, second=None, noise=None, zero_canonical=True, detach_bands=(),
              bands=(10, 4, 10)):
    """The Truth of a render pass of rays rb [n,12] (frame time = column 8) at depths z [n,S]"""
    n, S = z.shape
    t = float(rb[0, 8])
    assert bool((rb[:, 8] == rb[0, 8]).all()), "Only accepts all points from same time"
    sec = None
    if second is not None:
        t2, z2 = second
        assert z2.shape == z.shape
        sec = ray_encodings(rb, z2, float(np.float32(t2)), bands)[:2]
    return Truth(sd_np, names, n, S, ray_encodings(rb, z, bands=bands), dx_value, not (t == 0. and zero_canonical),
                 dict(z=z, rays_d=rb[:, 3:6], white_bkgd=white_bkgd, noise=noise), ray_loss, sec, detach_bands, bands[0])


def flip_aware_check(sd_np, rb, z, white_bkgd, ray_loss, gpu_grads, what, dx_value, second=None, noise=None, thr=5e-6, rtol=2e-5,
                     stats=None, bands=(10, 4, 10)):
    """sd_np: the DirectTemporalNeRF's fp32 weights (numpy, state_dict names); rb [n,12] (frame time = column 8), z [n,S]
    fp32 CPU tensors; dx_value [n,S,3]: position_delta of the evaluation under test (ignored at t == 0);
    ray_loss(ret, idx) -> scalar: the loss restricted to rays idx (ret: rgb_map disp_map acc_map raw position_delta, and
    with second=(t2, z2) position_delta_2 = dx of the same rays at time t2 on depths z2, deformation net only) - the total
    loss must be the sum of it over a partition of the rays; gpu_grads {name: tensor | None}: a parameter reported as None
    is compared, as zeros, with the truth like any other.  Returns (#flips, #risky); stats (a dict) receives `worst`,
    the largest residual of a tensor over its max."""
    T = ray_truth(sd_np, list(gpu_grads), rb, z, white_bkgd, ray_loss, dx_value, second, noise, bands=bands)
    flips, risky, worst = _check(T, gpu_grads, what, thr, rtol)
    if stats is not None:
        stats["worst"] = worst
    return flips, risky


def flip_aware_check_rows(sd_np, ex, et, ed, row_loss, gpu_grads, what, dx_value, run_deform=True, thr=5e-6, rtol=2e-5, stats=None):
    """The same check at the module level (DirectTemporalNeRF.forward on rows of encodings): every row is a unit of its own,
    nothing is composited, row_loss(ret, idx) sees raw [m,1,4] and position_delta [m,1,3] of rows idx."""
    M = ex.shape[0]
    T = Truth(sd_np, list(gpu_grads), M, 1, (ex, et, ed, ex[:, :3]), dx_value, run_deform, None, row_loss)
    flips, risky, worst = _check(T, gpu_grads, what, thr, rtol)
    if stats is not None:
        stats["worst"] = worst
    return flips, risky


def float64_dx(sd_np, ex, et):
    """dx of the float64 deformation net on fp32 encodings (what the evaluation under test's position_delta is printed against)"""
    sd = {k: v.double() for k, v in O.to_torch_sd(sd_np).items() if k.startswith("_time")}
    with torch.no_grad():
        return deform64(sd, ex.double(), et.double())
