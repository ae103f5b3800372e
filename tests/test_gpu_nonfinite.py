"""NaN and Inf through the ray pipeline: the standalone ops (embed, sample_coarse, raw2outputs and its backward, sample_pdf with
merge and std), the tail every fused pass shares, the fused backward's compositing, poisoned ray rows and a poisoned weight.
The contract is DESIGN.md "Non-finite values":
  - tail arithmetic has the reference's non-finite pattern element for element - equal NaN positions, equal Inf signs - and its
    finite elements stay within the project's tolerances (compositing 2e-6 + 2e-5 |ref|, its backward 2e-6 + 2e-4 |ref|,
    sample_pdf 5e-5, z_std 1e-6 relative to the kernel's own samples);
  - a ray row with a non-finite o, d, near, far or frame time has NaN maps and weights; its raw / dx are only deterministic;
  - rays without a non-finite input keep their bits; no output element is ever left unwritten.
The references are the CPU oracle on float64 tensors and torch.sort on the CPU.  tests/test_nonfinite_host.py shows, without a GPU,
that the float32 and the float64 oracle agree on the pattern of every case used here (tests/density_regimes.py poison_*).
Every output is a Guarded buffer prefilled with the FINITE sentinel: a slot a kernel leaves unwritten shows as the sentinel
among NaNs, and no output may still hold it.

Before the fixes this module came with (composite.h comp_relu and the rgb flag of CompGrads, resample.h nan_last_lt, ray_rows.h
row_dnorm) the MI355X gave: sentinels left in z_sorted behind NaN weights (test 2), finite weights behind a NaN density (tests 1,
4, 5, 7), NaN colour gradients without an rgb upstream (tests 1, 5), finite maps for a NaN origin (test 6)."""
import copy

import numpy as np
import pytest
import torch

from density_regimes import (T, _np, bits, Guarded, SENTINEL, NAMES, comp_reference, same_nonfinite, POISONS, POISON_S, POISON_PDF,
                             POISON_NB, POISON_UPS, poison_comp_inputs, poison_pdf_inputs, poison_fused_noise)
from oracle import nerf_oracle as O
from test_gpu_fused_tail import (Gate, same, net_of, rays_of, VARIANTS, infer, train_forward, backward_abi, pdf_abi, first,
                                 B_SIGMA, N_REF, WANT, BWD_KINDS)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def hold(g, a, b, atol, rtol, key, what):
    """a against the float64 truth b: equal NaN positions and Inf signs, finite elements within atol + rtol |b|"""
    g.true(same_nonfinite(a, b), f"{what}: non-finite pattern differs (NaN {int(np.isnan(_np(a)).sum())} vs {int(np.isnan(_np(b)).sum())}, "
                                 f"Inf {int(np.isinf(_np(a)).sum())} vs {int(np.isinf(_np(b)).sum())})")
    g.close(a, b, atol, rtol, key, what)


def written(g, t, what):
    g.true(not bool((bits(t) == SENTINEL).any()), f"{what}: {int((bits(t) == SENTINEL).sum())} elements were never written")


def rows_equal(g, a, b, what):
    g.true(torch.equal(bits(a), bits(b)), f"{what}: clean rays differ in their bits from the call without the poison")


def clean_of(rays, n=N_REF):
    return np.setdiff1d(np.arange(n), rays)


# ------------------------------------------------------------------------------ 1. standalone raw2outputs, forward and backward
def r2o(raw, z, d, noise, white, what, g):
    from swnerf import _lib as L
    N, S = z.shape
    outs = [Guarded(s, DEV) for s in ((N, 3), (N,), (N,), (N, S), (N,))]
    L.check(L.lib().swnerf_raw2outputs(L.ptr(raw), L.ptr(z), L.ptr(d), L.ptr(noise), N, S, int(white), *[L.ptr(o.out) for o in outs],
                                       L.stream_of(raw)), "raw2outputs")
    for o, name in zip(outs, NAMES):
        o.check(f"{what} {name}")
        written(g, o.out, f"{what} {name}")
    return [o.out for o in outs]


def r2o_bwd(raw, z, d, noise, white, ups, which, what, g):
    from swnerf import _lib as L
    N, S = z.shape
    has = lambda k: which == k or (isinstance(which, tuple) and k in which)
    gp = [L.ptr(ups[k]) if has(k) else None for k in ("rgb", "disp", "acc", "depth", "weights")]
    out = Guarded((N, S, 4), DEV)
    L.check(L.lib().swnerf_raw2outputs_backward(L.ptr(raw), L.ptr(z), L.ptr(d), L.ptr(noise), N, S, int(white), *gp, L.ptr(out.out),
                                                L.stream_of(raw)), "raw2outputs_backward")
    out.check(what)
    written(g, out.out, what)
    return out.out


@pytest.mark.parametrize("where", ["density", "colour"])
@pytest.mark.parametrize("kind", list(POISONS))
@pytest.mark.parametrize("S", POISON_S)
def test_standalone_compositing_nonfinite(S, kind, where):
    """swnerf_raw2outputs and its backward, one NaN / +Inf / -Inf per odd ray in the density (through noise) or in a colour of raw, on
    samples 0, S-1, 31 | 32, 63 | 64: the five outputs and d_raw (upstream rgb, acc, depth, weights, the four together) against
    float64; clean rays bit-equal to the call on the clean rays alone."""
    raw_np, z_np, d_np, noise_np, ups_np, rays, _ = poison_comp_inputs(S, kind, where)
    clean = clean_of(rays)
    put = lambda a: T(np.ascontiguousarray(a)).to(DEV)
    raw, z, d, noise = (put(a) for a in (raw_np, z_np, d_np, noise_np))
    ups = {k: put(v) for k, v in ups_np.items()}
    craw, cz, cd, cnoise = (put(a[clean]) for a in (raw_np, z_np, d_np, noise_np))
    cups = {k: put(v[clean]) for k, v in ups_np.items()}
    g = Gate()
    for white in (False, True):
        what = f"raw2outputs S={S} {kind} in {where} white={white}"
        ref, ref_g = comp_reference(raw_np, z_np, d_np, noise_np, white, ups_np, True, upstream=POISON_UPS)
        outs = r2o(raw, z, d, noise, white, what, g)
        alone = r2o(craw, cz, cd, cnoise, white, what + " clean rays", g)
        for name, o, b, c in zip(NAMES, outs, ref, alone):
            hold(g, o, b, 2e-6, 2e-5, name, f"{what} {name}")
            rows_equal(g, o[clean], c, f"{what} {name}")
        if kind == "nan" and where == "density":
            g.true(all(bool(torch.isnan(outs[i][rays]).all()) for i in (0, 1, 2, 4)), f"{what}: a map of a ray with a NaN density is finite")
        for which in POISON_UPS:
            w2 = f"{what} d_raw from {which}"
            got = r2o_bwd(raw, z, d, noise, white, ups, which, w2, g)
            hold(g, got, ref_g[which], 2e-6, 2e-4, "d_raw", w2)
            rows_equal(g, got[clean], r2o_bwd(craw, cz, cd, cnoise, white, cups, which, w2 + " clean rays", g), w2)
    g.finish(f"standalone compositing S={S} {kind} {where}")


# ------------------------------------------------------------------------------------- 2. standalone sample_pdf, merge and std
def pdf(bins, w, Ni, u, z, what, g):
    """swnerf_sample_pdf plain and with merge + std, every output guarded -> (samples, z_sorted, z_std)"""
    N = bins.shape[0]
    plain, smp, zs, sd = Guarded((N, Ni), DEV), Guarded((N, Ni), DEV), Guarded((N, z.shape[1] + Ni), DEV), Guarded((N,), DEV)
    pdf_abi(bins, w, Ni, u, plain.out, None, None, None)
    pdf_abi(bins, w, Ni, u, smp.out, z, zs.out, sd.out)
    for o, name in ((plain, "samples (plain call)"), (smp, "samples"), (zs, "z_sorted"), (sd, "z_std")):
        o.check(f"{what} {name}")
        written(g, o.out, f"{what} {name}")
    g.true(same(plain.out, smp.out), f"{what}: the samples of the plain call differ from those of the merging call")
    return smp.out, zs.out, sd.out


def check_pdf(g, bins_np, w_np, u_np, z_np, Ni, rays, nan_samples, what):
    """nan_samples [N, Ni] bool: where the reference has NaN.  -> the device outputs"""
    put = lambda a: None if a is None else T(np.ascontiguousarray(a)).to(DEV)
    N, S = z_np.shape
    smp, zs, sd = pdf(put(bins_np), put(w_np), Ni, put(u_np), put(z_np), what, g)
    u64 = torch.linspace(0., 1., Ni).expand(N, Ni).double() if u_np is None else T(u_np).double()
    ref = O.sample_pdf(T(bins_np).double(), T(w_np).double(), Ni, u=u64.contiguous())
    g.true(np.array_equal(np.isnan(ref.numpy()), nan_samples), f"{what}: the reference's NaN samples are not where the case expects them")
    hold(g, smp, ref, 5e-5, 0.0, "samples", f"{what} samples")
    want = torch.sort(torch.cat([T(z_np), smp.cpu()], -1), -1)[0]
    g.true(same(zs.cpu(), want), f"{what}: z_sorted != sort(cat[z, samples]) ({int((bits(zs.cpu()) != bits(want)).sum())} slots)")
    s64 = smp.double().cpu()
    ref_sd = ((s64 - s64.mean(-1, keepdim=True)) ** 2).mean(-1).sqrt()
    hold(g, sd, ref_sd, 0.0, 1e-6, "z_std", f"{what} z_std")
    g.true(bool(torch.isnan(sd[torch.from_numpy(nan_samples.any(-1)).to(DEV)]).all()), f"{what}: z_std of a ray with NaN samples is finite")
    clean = clean_of(rays, N)
    alone = pdf(put(bins_np[clean]), put(w_np[clean]), Ni, None if u_np is None else put(u_np[clean]), put(z_np[clean]), what + " clean rays", g)
    for name, a, b in zip(("samples", "z_sorted", "z_std"), (smp, zs, sd), alone):
        rows_equal(g, a[clean], b, f"{what} {name}")
    return smp, zs, sd


@pytest.mark.parametrize("mode", ["det", "random"])
@pytest.mark.parametrize("S,Ni", POISON_PDF)
def test_standalone_sample_pdf_poisoned_weight(S, Ni, mode):
    """one NaN / +Inf / -Inf weight per odd ray, nb = 65, (S, Ni) in {(64,128), (64,1), (1,64), (128,64)}, det and random u: on those rays
    every sample is NaN, z_sorted is sort(cat[z, samples]) with the NaNs last and every slot written, z_std is NaN; clean rays
    bit-equal to the call without the poisoned rays."""
    g = Gate()
    for kind in POISONS:
        bins, w, u, z, rays, _ = poison_pdf_inputs(S, Ni, kind, mode)
        nan_samples = np.zeros((N_REF, Ni), bool)
        nan_samples[rays] = True
        what = f"sample_pdf S={S} Ni={Ni} {mode} {kind} weight"
        smp, zs, _ = check_pdf(g, bins, w, u, z, Ni, rays, nan_samples, what)
        g.true(bool(torch.isnan(zs[rays][:, S:]).all()) and torch.equal(bits(zs[rays][:, :S]), bits(T(z[rays]).to(DEV))),
               f"{what}: z_sorted of a poisoned ray is not [the coarse depths, NaN x Ni]")
    g.finish(f"sample_pdf poisoned weight S={S} Ni={Ni} {mode}")


@pytest.mark.parametrize("S,Ni", [p for p in POISON_PDF if p[1] > 1])
def test_standalone_sample_pdf_poisoned_draw(S, Ni):
    """one NaN draw in u on every odd ray: exactly that sample is NaN, the merge (through the bitonic sort of the samples) holds it in
    the last slot, z_std is NaN; every other ray keeps its bits."""
    g = Gate()
    bins, w, u, z, rays, j = poison_pdf_inputs(S, Ni, "nan", "random", target="u")
    nan_samples = np.zeros((N_REF, Ni), bool)
    nan_samples[rays, j] = True
    what = f"sample_pdf S={S} Ni={Ni} NaN draw"
    _, zs, _ = check_pdf(g, bins, w, u, z, Ni, rays, nan_samples, what)
    g.true(bool(torch.isnan(zs[rays][:, -1]).all()) and int(torch.isnan(zs).sum()) == len(rays), f"{what}: the one NaN is not in the last slot")
    g.finish(what)


# ------------------------------------------------------------------------------------------------ 3. embed and sample_coarse
@pytest.mark.parametrize("d,L", [(3, 10), (1, 4)])
def test_embed_nonfinite_rows(d, L):
    """rows holding NaN, +Inf and -Inf among 300 (more than one workgroup): the identity columns pass the value through, the sin / cos
    columns of that component are NaN (torch.sin(inf) is), the finite elements stay within 3e-7; every other row keeps its bits."""
    from swnerf import _lib as L_
    M = 300
    x = np.random.default_rng(d + L).uniform(-6, 6, (M, d)).astype(np.float32)
    bad = np.array([5, 150, 299])
    x[5, 0], x[150, d - 1], x[299, 0] = np.nan, np.inf, -np.inf
    g = Gate()

    def run(xs):
        xt = T(np.ascontiguousarray(xs)).to(DEV)
        out = Guarded((len(xs), d * (1 + 2 * L)), DEV)
        L_.check(L_.lib().swnerf_embed(L_.ptr(xt), len(xs), d, L, L_.ptr(out.out), L_.stream_of(xt)), "embed")
        out.check(f"embed d={d} L={L}")
        written(g, out.out, f"embed d={d} L={L} M={len(xs)}")
        return out.out
    got = run(x)
    ref = O.embed(T(x).double(), L)
    hold(g, got, ref, 3e-7, 0.0, "embed", f"embed d={d} L={L}")
    g.true(torch.equal(torch.nan_to_num(got[:, :d].cpu(), nan=-7.0), torch.nan_to_num(T(x), nan=-7.0)), "the identity columns do not pass x through")
    g.true(bool(torch.isnan(got[5, 0::d]).all()) and bool(torch.isnan(got[150, 2 * d - 1::d]).all()) and bool(torch.isnan(got[299, d::d]).all()),
           "a sin / cos column of a non-finite component is not NaN")
    clean = clean_of(bad, M)
    rows_equal(g, got[clean], run(x[clean]), f"embed d={d} L={L}")
    g.finish(f"embed d={d} L={L}")


@pytest.mark.parametrize("S", [3, 65])
def test_sample_coarse_nonfinite_near_far(S):
    """NaN near, NaN far, +Inf far, -Inf near on four of 37 rays, linear and in disparity, with and without jitter: the oracle's
    pattern (all NaN for a NaN bound), every other ray bit-equal to the call without those rays."""
    from swnerf import _lib as L_
    N = 37
    rng = np.random.default_rng(S)
    near = rng.uniform(0.5, 3.0, (N, 1)).astype(np.float32)
    far = (near + rng.uniform(0.5, 5.0, (N, 1))).astype(np.float32)
    bad = np.array([3, 10, 20, 30])
    near[3], far[10], far[20], near[30] = np.nan, np.nan, np.inf, -np.inf
    rb = np.concatenate([rng.standard_normal((N, 6)).astype(np.float32), near, far], 1)
    t_rand = rng.uniform(0, 1, (N, S)).astype(np.float32)
    clean = clean_of(bad, N)
    g = Gate()

    def run(rows, tr, lindisp, what):
        rt = T(np.ascontiguousarray(rows)).to(DEV)
        tt = None if tr is None else T(np.ascontiguousarray(tr)).to(DEV)
        gz, gp = Guarded((len(rows), S), DEV), Guarded((len(rows), S, 3), DEV)
        L_.check(L_.lib().swnerf_sample_coarse(L_.ptr(rt), len(rows), 8, S, int(lindisp), L_.ptr(tt), L_.ptr(gz.out), L_.ptr(gp.out),
                                               L_.stream_of(rt)), "sample_coarse")
        for o, name in ((gz, "z"), (gp, "pts")):
            o.check(f"{what} {name}")
            written(g, o.out, f"{what} {name}")
        return gz.out, gp.out
    for lindisp in (False, True):
        for tr in (None, t_rand):
            what = f"sample_coarse S={S} lindisp={lindisp} jitter={tr is not None}"
            z, pts = run(rb, tr, lindisp, what)
            ref = O.coarse_z(T(near), T(far), S, lindisp, None if tr is None else T(tr))
            hold(g, z, ref.double(), 0.0 if tr is None else 1e-6, 0.0, "z", what)
            g.true(bool(torch.isnan(z[[3, 10]]).all()), f"{what}: a depth of a ray with a NaN bound is finite")
            g.true(same(pts, T(rb[:, None, 0:3]).to(DEV) + T(rb[:, None, 3:6]).to(DEV) * z[..., None]), f"{what}: pts != o + d * z")
            zc, pc = run(rb[clean], None if tr is None else tr[clean], lindisp, what + " clean rays")
            rows_equal(g, z[clean], zc, f"{what} z")
            rows_equal(g, pts[clean], pc, f"{what} pts")
    g.finish(f"sample_coarse S={S}")


# ----------------------------------------------------------------------------------------------------- 4. the fused tail
def gpass(variant, rb, S, g, what, *, net=None, n_importance=0, white_bkgd=False, lindisp=False, **inputs):
    """infer() of tests/test_gpu_fused_tail.py at the ABI with every output a Guarded buffer: guards checked, no sentinel left"""
    import swnerf.render as render
    from swnerf import _lib
    kind, prec, deform, _, _ = VARIANTS[variant]
    net = net_of(kind) if net is None else net
    want, oc, terms = WANT + (["dx"] if kind == "dnerf" else []), 4, 0
    if kind.startswith("noview"):
        packed, Lp, oc = net.packed_noview()
        k, Ld, Lt = _lib.NET_NOVIEW, 0, 0
    else:
        k, packed, Lp, Ld, Lt = net.packed()
        terms = render._PRECISIONS[prec]
        if terms:
            packed, _, _ = net.packed_x3()
    ins = dict(z_vals=None, t_rand=None, noise=None, u=None)
    ins.update(inputs)
    a, out, _keep = render.pass_args(rb, k, packed, (Lp, Ld, Lt), S, oc, 0 if kind == "tnerf" else deform, ins, want, n_importance,
                                     lindisp=lindisp, white_bkgd=white_bkgd)
    guards = {name: Guarded(t.shape, DEV) for name, t in out.items()}
    for name, gd in guards.items():
        setattr(a, name, gd.out.data_ptr())
    L = _lib.lib()
    if terms:
        _lib.check(L.swnerf_render_pass_x3(a, terms, _lib.stream_of(rb)), "render_pass_x3")
    else:
        _lib.check(L.swnerf_render_pass(a, _lib.stream_of(rb)), "render_pass")
    for name, gd in guards.items():
        gd.check(f"{what} {name}")
        written(g, gd.out, f"{what} {name}")
    return {name: gd.out for name, gd in guards.items()}


@pytest.mark.parametrize("kind", list(POISONS))
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_fused_tail_nonfinite_density(variant, kind):
    """every fused pass, S in {33, 65}, one NaN / +Inf / -Inf density per odd ray through `noise`: compositing against the float64
    oracle on the pass's own raw and depths; z_fine / z_std (n_importance 64, det and random u) equal to the standalone op on the pass's
    weights and to the CPU sort; the training forward and the batches of 1, 3, 5 rays equal to the 41-ray inference pass."""
    net_kind, _, _, has_train, resamples = VARIANTS[variant]
    rb = rays_of(net_kind)
    d64 = rb[:, 3:6].double().cpu()
    g = Gate()
    for S in (33, 65):
        noise_np, zgiven, rays, _ = poison_fused_noise(S, kind, B_SIGMA)
        noise = T(noise_np).to(DEV)
        for white, kw in ((False, dict(noise=noise)), (True, dict(noise=noise, z_vals=T(zgiven).to(DEV)))):
            what = f"{variant} {kind} S={S} white={white} given depths={'z_vals' in kw}"
            out = gpass(variant, rb, S, g, what, white_bkgd=white, **kw)
            ref = O.raw2outputs(out["raw"][..., :4].double().cpu(), out["z_out"].double().cpu(), d64, 0., white, noise=T(noise_np).double())
            for name, b in zip(NAMES, ref):
                hold(g, out[name if name == "weights" else name + "_map"], b, 2e-6, 2e-5, name, f"{what} {name}")
            g.true(all(same(infer(variant, rb, S, white_bkgd=white, **kw)[k], out[k]) for k in out), f"{what}: the guarded call differs from render_pass")
            if has_train:
                tr, _ = train_forward(net_kind, rb, S, white_bkgd=white, **kw)
                for k in out:
                    g.true(same(tr[k], out[k]), f"{what}: training forward differs from the inference pass in {k}")
            for n in (1, 3, 5):
                small = infer(variant, rb[:n], S, white_bkgd=white, **first(kw, n))
                for k in out:
                    g.true(same(small[k], out[k][:n]), f"{what}: N={n} differs from the prefix of N={N_REF} in {k}")
        if not resamples:
            continue
        Ni = 64
        for u_np in (None, np.random.default_rng(S).uniform(0, 1, (N_REF, Ni)).astype(np.float32)):
            what = f"{variant} {kind} S={S} Ni={Ni} u={'det' if u_np is None else 'random'}"
            u = None if u_np is None else T(u_np).to(DEV)
            kw = dict(noise=noise, white_bkgd=True, n_importance=Ni, u=u)
            out = gpass(variant, rb, S, g, what, **kw)
            z, w = out["z_out"], out["weights"]
            smp, zs, sd = pdf((.5 * (z[:, 1:] + z[:, :-1])).contiguous(), w[:, 1:-1].contiguous(), Ni, u, z, what + " standalone", g)
            g.true(same(out["z_fine"], zs), f"{what}: z_fine of the pass != the standalone op on the pass's weights")
            g.true(same(out["z_std"], sd), f"{what}: z_std of the pass != the standalone op")
            g.true(same(zs.cpu(), torch.sort(torch.cat([z.cpu(), smp.cpu()], -1), -1)[0]), f"{what}: z_fine != sort(cat[z, samples])")
            g.worst["rays with NaN samples"] = g.worst.get("rays with NaN samples", 0) + int(torch.isnan(smp).any(-1).sum())
            if has_train and net_kind != "dnerf":               # (the D-NeRF training pass has no resampling)
                tr, _ = train_forward(net_kind, rb, S, **kw)
                for k in out:
                    g.true(same(tr[k], out[k]), f"{what}: training forward differs from the inference pass in {k}")
            for n in (1, 3, 5):
                small = infer(variant, rb[:n], S, **first(kw, n))
                for k in ("z_fine", "z_std", "weights"):
                    g.true(same(small[k], out[k][:n]), f"{what}: N={n} differs from the prefix of N={N_REF} in {k}")
    if resamples and kind == "nan":
        g.true(g.worst["rays with NaN samples"] > 0, "no case reached the merge with NaN samples")
    g.finish(f"fused tail {variant} {kind}")


# ------------------------------------------------------------------------------------------------- 5. the fused backward
N_BWD = 13                             # six poisoned rays: every boundary sample of S = 65
BWD_BATCHES = ((0, 5), (5, 8), (8, 9), (9, 13))
BWD_UPS = ("rgb", "acc", ("rgb", "acc"))      # of POISON_UPS what the fused backward's ABI has (no d depth_map, no d weights)


@pytest.mark.parametrize("S", (33, 65))
@pytest.mark.parametrize("kind", BWD_KINDS)
def test_fused_backward_nonfinite_d_raw(kind, S):
    """d_raw of every fused backward kernel on the saved buffers of a real training forward and CHOSEN raw / depths / noise with
    one poisoned density (noise) or colour (raw) per odd ray: against float64 autograd at 2e-6 + 2e-4 |ref| with an equal
    non-finite pattern; rows past S zero; guards intact; clean rays bit-equal to the launch with the poison replaced by 0.
    T-NeRF: raw's colours are OUTPUTS of its ReLU head, so d(pre-ReLU colour) is d_raw where raw > 0 and 0 elsewhere."""
    rb = rays_of(kind, N_BWD)
    from swnerf import _lib
    fwd, sv = train_forward(kind, rb, S)
    oc = 5 if kind == "noview5" else 4
    wide = 8 if kind.startswith("noview") else 4
    prow = (S + 31) // 32 * 32
    nact = _lib.lib().swnerf_tnerf_act_floats_per_row() if kind == "tnerf" else _lib.lib().swnerf_act_floats_per_row()
    grads = [torch.zeros((5 * prow, nact), device=DEV) for _ in range(2 if kind == "dnerf" else 1)]
    if kind == "dnerf":
        grads.append(torch.zeros((5 * prow, 4), device=DEV))
    d = _np(rb[:, 3:6])
    g = Gate()

    def launch(raw, z, noise, white, gr3, r0, r1, what):
        out = Guarded(((r1 - r0) * prow, wide), DEV)
        backward_abi(kind, sv, fwd, rb, r0, r1, S, raw, z, noise, white, gr3 + [None], out.out, grads)
        out.check(what)
        written(g, out.out, what)
        return out.out.reshape(r1 - r0, prow, wide)
    for poison in POISONS:
        for where in ("density", "colour"):
            raw_np, z_np, _, noise_np, ups_np, rays, j = poison_comp_inputs(S, poison, where, N=N_BWD)
            zero_raw, zero_noise = raw_np.copy(), noise_np.copy()
            zero_raw[rays, j, rays % 3] = np.where(where == "colour", 0.0, zero_raw[rays, j, rays % 3])
            zero_noise[rays, j] = np.where(where == "density", 0.0, zero_noise[rays, j])
            if oc == 5:
                fifth = np.random.default_rng(S).standard_normal((N_BWD, S, 1)).astype(np.float32)
                raw_np, zero_raw = np.concatenate([raw_np, fifth], -1), np.concatenate([zero_raw, fifth], -1)
            raw, z, noise, raw0, noise0 = (T(a).to(DEV) for a in (raw_np, z_np, noise_np, zero_raw, zero_noise))
            ups = {k: T(ups_np[k]).to(DEV) for k in ("rgb", "disp", "acc")}
            is_clean = np.isin(np.arange(N_BWD), rays, invert=True)
            for white in (False, True):
                _, ref = comp_reference(raw_np[..., :4], z_np, d, noise_np, white, ups_np, True, upstream=BWD_UPS)
                for which in BWD_UPS:
                    gr3 = [ups[k] if k in (which if isinstance(which, tuple) else (which,)) else None for k in ("rgb", "disp", "acc")]
                    want = ref[which].numpy().copy()
                    if kind == "tnerf":
                        want[..., :3] = np.where(raw_np[..., :3] > 0, want[..., :3], 0.0)
                    for r0, r1 in BWD_BATCHES:
                        what = f"{kind} S={S} {poison} in {where} N={r1 - r0} white={white} upstream={which}"
                        got = launch(raw, z, noise, white, gr3, r0, r1, what)
                        hold(g, got[:, :S, :4], want[r0:r1], 2e-6, 2e-4, "d_raw", what)
                        g.true(not bool(got[:, S:].any()), f"{what}: rows past S are not zero")
                        if wide == 8:
                            g.true(not bool(got[:, :, 4:].any()), f"{what}: columns 4..7 of d_raw8")
                        base = launch(raw0, z, noise0, white, gr3, r0, r1, what + " poison -> 0")
                        c = torch.from_numpy(is_clean[r0:r1]).to(DEV)
                        rows_equal(g, got[c], base[c], what)
    g.finish(f"fused backward d_raw {kind} S={S}")


# -------------------------------------------------------------------------------------------------- 6. poisoned ray rows
ROW_VARIANTS = ("canon", "noview5", "dnerf", "tnerf", "canon_x3")
MAPS = ("rgb_map", "disp_map", "acc_map", "depth_map", "weights")


@pytest.mark.parametrize("variant", ROW_VARIANTS)
def test_poisoned_ray_rows(variant):
    """one ray each with NaN in an origin component, a direction component, near, far and (where the row has one) the frame time,
    one with +Inf in a direction component: maps and weights of those rays are all NaN in the coarse pass (S = 33) and, after
    resampling (n_importance 64), in the fine pass on z_fine; raw and dx of those rays are the same bits in two calls (nothing else
    is asserted about them); every other ray is bit-equal to the pass on the clean rows alone."""
    net_kind, _, _, _, resamples = VARIANTS[variant]
    rb = rays_of(net_kind).clone()
    cols = {1: 0, 3: 4, 5: 6, 7: 7, 11: 3}
    if rb.shape[1] == 12:
        cols[9] = 8
    for r, c in cols.items():
        rb[r, c] = float("inf") if r == 11 else float("nan")
    bad = np.array(sorted(cols))
    clean = clean_of(bad)
    ci = torch.from_numpy(clean).to(DEV)
    S, Ni = 33, 64
    g = Gate()

    def both(S_, what, **kw):
        out = gpass(variant, rb, S_, g, what, white_bkgd=True, **kw)
        for k in MAPS:
            g.true(bool(torch.isnan(out[k][bad]).all()), f"{what}: {k} of a ray with a non-finite row holds {int((~torch.isnan(out[k][bad])).sum())} numbers")
        again = gpass(variant, rb, S_, g, what + " again", white_bkgd=True, **kw)
        for k in out:
            g.true(torch.equal(bits(out[k]), bits(again[k])), f"{what}: {k} differs between two calls")
        alone = gpass(variant, rb[ci].contiguous(), S_, g, what + " clean rows", white_bkgd=True, **{k: (v[ci].contiguous() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()})
        for k in out:
            rows_equal(g, out[k][ci], alone[k], f"{what} {k}")
            g.true(k in ("disp_map",) or bool(torch.isfinite(alone[k]).all()), f"{what}: {k} of a clean ray is not finite")
        return out
    coarse = both(S, f"{variant} rows coarse", **(dict(n_importance=Ni) if resamples else {}))
    if resamples:
        both(S + Ni, f"{variant} rows fine", z_vals=coarse["z_fine"].contiguous())
    g.finish(f"poisoned ray rows {variant}")


# ------------------------------------------------------------------------------------------------- 7. a poisoned weight
def train_forward_canon(net, rb, S):
    """the canon branch of test_gpu_fused_tail.train_forward on a given net"""
    import swnerf.render as render
    from swnerf import _lib
    L = _lib.lib()
    rows = L.swnerf_train_rows(rb.shape[0], S)
    new = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=DEV)
    sv = [new(rows, L.swnerf_act_floats_per_row()), new(L.swnerf_mask_floats(rows)), new(rows, L.swnerf_xs_floats_per_row())]
    k, packed, Lp, Ld, _ = net.packed()
    a, o, _keep = render.pass_args(rb, k, packed, (Lp, Ld, 0), S, 4, 0, dict(z_vals=None, t_rand=None, noise=None, u=None), WANT)
    _lib.check(L.swnerf_render_pass_train(a, *[_lib.ptr(t) for t in sv], _lib.stream_of(rb)), "render_pass_train")
    return o


@pytest.mark.parametrize("head", ["rgb_linear", "alpha_linear"])
def test_poisoned_weight_cannot_render_a_finite_image(head):
    """one NaN in the rgb head's bias: that channel of every ray's rgb_map is NaN; one in the density head's bias: every map and every
    weight of every ray is NaN - in the inference pass and in the training forward.  A diverged net shows in its image."""
    net = copy.deepcopy(net_of("canon"))
    net._pack_cache = {}
    with torch.no_grad():
        getattr(net, head).bias[0] = float("nan")
    rb = rays_of("canon")
    g = Gate()
    S = 33
    inf = gpass("canon", rb, S, g, f"NaN in {head}.bias", net=net)
    for name, out in (("inference pass", inf), ("training forward", train_forward_canon(net, rb, S))):
        if head == "rgb_linear":
            g.true(bool(torch.isnan(out["rgb_map"][:, 0]).all()), f"{name}: a ray's rgb_map is finite behind a NaN rgb bias")
            g.true(bool(torch.isfinite(out["acc_map"]).all()), f"{name}: acc_map does not depend on the colours")
        else:
            for k in MAPS:
                g.true(bool(torch.isnan(out[k]).all()), f"{name}: {k} is finite behind a NaN density bias")
        for k in inf:
            g.true(same(out[k], inf[k]), f"{name}: {k} differs from the inference pass")
    g.finish(f"poisoned weight {head}")
