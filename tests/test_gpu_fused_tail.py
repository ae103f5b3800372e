"""The tail every fused pass shares - depth sampling, raw2outputs, sample_pdf, the rank merge, z_std (csrc/render_pass.h,
composite.h, resample.h) - and the compositing backward of the fused backward kernels (render_pass.h comp_bwd_ray), at density
extremes and with no "mostly" clause: every element of every case is held to its reference.

A. Forward.  The seeded nets of the other GPU tests with the density head's weight row set to zero and its bias to B_SIGMA:
   raw[..., 3] comes back as B_SIGMA bit for bit, so the density of a sample is B_SIGMA + noise and a regime
   (tests/density_regimes.py: mild, wall, soft_then_wall, all_opaque, all_empty, spike) is imposed through the pass's `noise`
   operand.  The colours stay those of the net.
   - compositing: the oracle's raw2outputs on float64 tensors, fed the pass's own returned raw and depths and the injected noise
     (the MLP's rounding never enters), atol 2e-6 + rtol 2e-5 on rgb / acc / depth / weights / disparity, equal NaN pattern:
     the figures tests/test_gpu_op_domain.py holds the standalone op to.  The fused passes scan 32 mirrored lanes with
     __shfl_up and carry the transmittance in double from tile to tile; the standalone op scans 64 lanes with DPP.
   - a training forward is documented as "exactly swnerf_render_pass, same outputs": torch.equal on every output, so the float64
     check runs on the inference pass alone.  All four training forwards are bit-equal by design.
   - batches of 1, 3 and 5 rays are torch.equal to the prefix of the 41-ray batch (waves past the last ray change nothing).
   - resampling: z_fine and z_std are torch.equal to the STANDALONE op swnerf_sample_pdf (merge + std) fed the pass's own
     weights[:, 1:-1], mid-points, depths and u - resample.h says both run the same instructions; and the standalone op's samples,
     z_sorted and z_std are equal, bit for bit, to tests/resample_replay.py (numpy at the kernel's precisions, pinned to the
     reference by tests/test_resample_replay_host.py).  A ray may differ only if one cdf entry of the replay lies within 2^-40 of a
     float32 rounding boundary and flipping it reproduces the device's bits; at most one such ray per case.
B. Backward.  swnerf_render_pass_backward / _noview / _dnerf / _tnerf called at the ABI on saved buffers of a real training
   forward, with CHOSEN raw, depths, noise and upstream gradients: d_raw against float64 autograd of the oracle's raw2outputs,
   atol 2e-6 + rtol 2e-4 on every element (the figure of composite.h's backward in test_gpu_op_domain.py); rows past S exactly
   zero; sentinels around d_raw intact; grad finite.

Measured on MI355X: in each test's docstring.  The module takes 70 s, no case more than 2.3 s."""
import functools

import numpy as np
import pytest
import torch

import cases
import cases_bands as CB
import cases_tnerf
import resample_replay as RR
from density_regimes import T, _np, bits, Guarded, ALL_REGIMES, NAMES, comp_inputs, comp_reference
from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
B_SIGMA = 0.25                         # the density head's bias: what raw[..., 3] must come back as
N_REF = 41                             # 10 workgroups and one with three waves past the last ray
WANT = ["rgb_map", "disp_map", "acc_map", "depth_map", "weights", "raw", "z_out"]


class Gate:
    """collects the worst error and every miss, prints, then asserts: a failing case still shows all its figures"""

    def __init__(self):
        self.worst, self.misses = {}, []

    def close(self, a, b, atol, rtol, key, what):
        """every element: |a - b| <= atol + rtol |b|, equal NaN pattern; b is the float64 truth"""
        a, b = _np(a).astype(np.float64), _np(b).astype(np.float64)
        assert a.shape == b.shape, (what, a.shape, b.shape)
        if not np.array_equal(np.isnan(a), np.isnan(b)):
            self.misses.append(f"{what}: NaN pattern differs")
            return
        if a.size == 0:
            return
        err = np.abs(np.nan_to_num(a) - np.nan_to_num(b))
        excess = float((err - (atol + rtol * np.abs(np.nan_to_num(b)))).max())
        self.worst[key] = max(self.worst.get(key, 0.0), float(err.max()))
        if excess > 0.0:
            self.misses.append(f"{what}: max err {err.max():.3e}, worst excess over {atol:g} + {rtol:g} |ref| {excess:.3e}")

    def true(self, cond, what):
        if not bool(cond):
            self.misses.append(what)

    def finish(self, label):
        print(f"\n[fused-tail] {label}: " + ", ".join(f"{k} {v:d}" if isinstance(v, int) else f"{k} {v:.2e}" for k, v in self.worst.items()) + f"; {len(self.misses)} misses")
        assert not self.misses, f"{label}: {len(self.misses)} misses, first: " + " | ".join(self.misses[:5])


def same(a, b):
    return torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0))


# ---------------------------------------------------------------------------------------------------- nets and passes
@functools.lru_cache(maxsize=1)
def net_of(kind):
    """the seeded net of `kind` with a dead density head: weight row 0, bias B_SIGMA.  One net alive at a time."""
    import swnerf.model as model
    from swnerf.embedder import get_embedder
    if kind == "canon":
        sd, head, row = dict(cases.weights_static()[0]), "alpha_linear", 0
        m = model.vallina_NeRF(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=5, skips=[4], use_viewdirs=True)
    elif kind in ("noview4", "noview5"):
        oc = int(kind[-1])
        sd, head, row = dict(cases.g12_weights()[0]), "output_linear", 3
        sd["output_linear.weight"], sd["output_linear.bias"] = sd["output_linear.weight"][:oc].copy(), sd["output_linear.bias"][:oc].copy()
        m = model.vallina_NeRF(**dict(cases.G12_NET, output_ch=oc))
    elif kind == "dnerf":
        sd, head, row = dict(cases.weights_dnerf()), "_occ.alpha_linear", 0
        m = model.DirectTemporalNeRF(D=8, W=256, input_ch=63, input_ch_views=27, input_ch_time=21, output_ch=5, skips=[4],
                                     use_viewdirs=True, embed_fn=get_embedder(10, 3, 0)[0], zero_canonical=True)
    else:
        sd, head, row = dict(cases_tnerf.weights()), "density.0", 0
        m = model.TNeRF(**cases_tnerf.NET)
    w, b = sd[head + ".weight"].copy(), sd[head + ".bias"].copy()
    w[row], b[row] = 0.0, B_SIGMA
    sd[head + ".weight"], sd[head + ".bias"] = w, b
    m.load_state_dict({k: T(v) for k, v in sd.items()}, strict=True)
    return m.to(DEV).eval()


def bands_kind(kind):
    return "noview" if kind.startswith("noview") else kind


@functools.lru_cache(maxsize=None)
def rays_of(kind, n=N_REF):
    return T(CB.ray_batch(bands_kind(kind), n=n)).to(DEV)


# variant -> (net kind, precision, run_deform, has a training forward, resamples)
VARIANTS = {
    "canon": ("canon", "fp32", True, True, True),
    "canon_x3": ("canon", "bf16x3", True, False, True),
    "noview4": ("noview4", "fp32", True, True, True),
    "noview5": ("noview5", "fp32", True, True, True),
    "dnerf": ("dnerf", "fp32", True, True, True),
    "dnerf_static": ("dnerf", "fp32", False, False, True),
    "dnerf_x3": ("dnerf", "bf16x3", True, False, True),
    "tnerf": ("tnerf", "fp32", True, True, False),
}


def infer(variant, rb, S, **kw):
    import swnerf.render as render, swnerf.render_tnerf as rt
    kind, prec, deform, _, _ = VARIANTS[variant]
    net = net_of(kind)
    with torch.no_grad():
        if kind == "tnerf":
            return rt.render_pass_tnerf(rb, net, S, want=WANT, **kw)
        return render.render_pass(rb, net, S, want=WANT + (["dx"] if kind == "dnerf" else []), precision=prec, run_deform=deform, **kw)


def train_forward(kind, rb, S, *, z_vals=None, t_rand=None, noise=None, u=None, n_importance=0, lindisp=False, white_bkgd=False):
    """The training forward of `kind` at the C ABI with every output the pass has -> (outputs, saved buffers of the backward)"""
    import swnerf.render as render
    from swnerf import _lib
    net, L, N = net_of(kind), _lib.lib(), rb.shape[0]
    rows = L.swnerf_train_rows(N, S)
    new = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=DEV)
    inputs = dict(z_vals=z_vals, t_rand=t_rand, noise=noise, u=u)
    st = _lib.stream_of(rb)
    if kind == "tnerf":
        k, packed, Lp, Ld, Lt = net.packed()
        sv = dict(act=new(rows, L.swnerf_tnerf_act_floats_per_row()), xs=new(rows, L.swnerf_tnerf_xs_floats_per_row()))
        a, o, _keep = render.pass_args(rb, k, packed, (Lp, Ld, Lt), S, 4, 0, inputs, WANT, lindisp=lindisp, white_bkgd=white_bkgd)
        _lib.check(L.swnerf_render_pass_train_tnerf(a, _lib.ptr(sv["act"]), _lib.ptr(sv["xs"]), st), "render_pass_train_tnerf")
        return o, sv
    nact, nxs, nbits = L.swnerf_act_floats_per_row(), L.swnerf_xs_floats_per_row(), L.swnerf_mask_floats(rows)
    sv = dict(act=new(rows, nact), bits=new(nbits), xs=new(rows, nxs))
    if kind == "dnerf":
        k, packed, Lp, Ld, Lt = net.packed()
        sv.update(act_d=new(rows, nact), bits_d=new(nbits), xs_d=new(rows, nxs))
        a, o, _keep = render.pass_args(rb, k, packed, (Lp, Ld, Lt), S, 4, 1, inputs, WANT + ["dx"], lindisp=lindisp, white_bkgd=white_bkgd)
        _lib.check(L.swnerf_render_pass_train_dnerf(a, *[_lib.ptr(sv[n]) for n in ("act", "bits", "xs", "act_d", "bits_d", "xs_d")], st),
                   "render_pass_train_dnerf")
        return o, sv
    if kind == "canon":
        k, packed, Lp, Ld, _ = net.packed()
        out_ch = 4
    else:
        packed, Lp, out_ch = net.packed_noview()
        k, Ld = _lib.NET_NOVIEW, 0
    a, o, _keep = render.pass_args(rb, k, packed, (Lp, Ld, 0), S, out_ch, 0, inputs, WANT, n_importance, lindisp=lindisp, white_bkgd=white_bkgd)
    _lib.check(L.swnerf_render_pass_train(a, _lib.ptr(sv["act"]), _lib.ptr(sv["bits"]), _lib.ptr(sv["xs"]), st), "render_pass_train")
    return o, sv


# ------------------------------------------------------------------------------------------------- A1. compositing
S_COMP = (2, 31, 32, 33, 64, 65, 192, 255, 256)
S_GIVEN_ONLY = 364                     # beyond the training passes and the resampling: inference on given depths
MODES = ("plain", "lindisp", "t_rand", "ties")


def regime_noise(regime, S, N=N_REF):
    """-> (noise [N, S] that turns the constant B_SIGMA into the regime's densities, the regime's sorted depths)"""
    raw, z, _, _, _ = comp_inputs(regime, S, 1000 * S + ALL_REGIMES.index(regime), N=N)
    return (raw[..., 3] - np.float32(B_SIGMA)).astype(np.float32), z


def with_ties(z):
    """exact ties (dist = 0) every fifth sample and across the 31 | 32 and 63 | 64 boundaries; stays ascending"""
    z = z.copy()
    S = z.shape[1]
    for k in list(range(0, S - 1, 5)) + [31, 63]:
        if k + 1 < S:
            z[:, k + 1] = z[:, k]
    return z


def sampling(mode, S, zgiven):
    if mode == "ties":
        return dict(z_vals=T(with_ties(zgiven)).to(DEV))
    if mode == "t_rand":
        return dict(t_rand=T(np.random.default_rng(S).uniform(0, 1, (N_REF, S)).astype(np.float32)).to(DEV))
    return dict(lindisp=mode == "lindisp")


def first(kw, n):
    return {k: (v[:n] if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}


@pytest.mark.parametrize("regime", ALL_REGIMES)
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_fused_compositing_vs_float64(variant, regime):
    """Every fused pass, S in {2, 31, 32, 33, 64, 65, 192, 255, 256} x {plain, lindisp, t_rand, given depths with exact ties} x white
    on / off, and S = 364 on given depths: every element against the float64 oracle at 2e-6 + 2e-5 |ref|; the training forward
    and the batches of 1, 3, 5 rays torch.equal to the 41-ray inference pass.
    Measured, worst over the eight passes and six regimes: rgb 2.1e-7, disparity 9.8e-8, acc 1.2e-7, weights 8.7e-8, depth 5.5e-7 (on
    depths up to 6: the rtol part); every bit comparison equal.  Dropping the tile carry of composite.h (tried on a scratch build)
    fails mild and wall; spike does not depend on it: behind the one opaque sample every alpha is 0."""
    kind, _, _, has_train, _ = VARIANTS[variant]
    rb = rays_of(kind)
    d64 = rb[:, 3:6].double().cpu()
    g = Gate()
    for S in S_COMP + (S_GIVEN_ONLY,):
        noise_np, zgiven = regime_noise(regime, S)
        noise = T(noise_np).to(DEV)
        for mode in (MODES if S != S_GIVEN_ONLY else ("ties",)):
            kw = dict(sampling(mode, S, zgiven), noise=noise)
            for white in (False, True):
                what = f"{variant} {regime} S={S} {mode} white={white}"
                out = infer(variant, rb, S, white_bkgd=white, **kw)
                raw = out["raw"]
                g.true(torch.equal(bits(raw[..., 3]), bits(torch.full_like(raw[..., 3], B_SIGMA))), f"{what}: raw[..., 3] is not the head's bias")
                ref = O.raw2outputs(raw[..., :4].double().cpu(), out["z_out"].double().cpu(), d64, 0., white, noise=T(noise_np).double())
                for name, b in zip(NAMES, ref):
                    key = name if name == "weights" else name + "_map"
                    g.close(out[key], b, 2e-6, 2e-5, name, f"{what} {name}")
                if regime == "all_empty":
                    g.true(bool(torch.isnan(out["disp_map"]).all()) and float(out["acc_map"].abs().max()) == 0.0, f"{what}: an empty ray has acc != 0 or a disparity")
                if has_train and S <= 256:
                    tr, _ = train_forward(kind, rb, S, white_bkgd=white, **kw)
                    g.true(list(tr) == list(out), f"{what}: outputs of the training forward {list(tr)}")
                    for k in out:
                        g.true(same(tr[k], out[k]), f"{what}: training forward differs from the inference pass in {k}")
                for n in (1, 3, 5):
                    small = infer(variant, rb[:n], S, white_bkgd=white, **first(kw, n))
                    for k in out:
                        g.true(same(small[k], out[k][:n]), f"{what}: N={n} differs from the prefix of N={N_REF} in {k}")
    g.finish(f"compositing {variant} {regime}")


# -------------------------------------------------------------------------------------------------- A2. resampling
PAIRS = ((3, 1), (7, 5), (33, 95), (64, 128), (65, 37), (255, 64), (256, 768))
U_MODES = ("det", "sorted", "random")


def pdf_abi(bins, w, ns, u, smp, z, zs, sd):
    from swnerf import _lib as L_
    N, nb = bins.shape
    L_.check(L_.lib().swnerf_sample_pdf(L_.ptr(bins), L_.ptr(w), N, nb, ns, L_.ptr(u), L_.ptr(smp), L_.ptr(z),
                                        0 if z is None else z.shape[1], L_.ptr(zs), L_.ptr(sd), L_.stream_of(bins)), "sample_pdf")


def draws(mode, N, Ni, seed, cdf=None):
    """u [N, Ni] or None (det).  Random draws almost never enter a bin without mass (all of them together hold ~nb * 1e-5 of
    the cdf), so with `cdf` (the replay's, of the weights the op will see) up to half of each row is PLACED there: in the middle
    of bins whose cdf step is below 3e-5 - on either side of the den < 1e-5 rule - and, every fourth, on the bin's lower cdf
    value itself (searchsorted right=True)."""
    if mode == "det":
        return None
    rng = np.random.default_rng(seed)
    u = rng.uniform(0, 1, (N, Ni)).astype(np.float32)
    if cdf is not None and Ni > 4:
        den = np.diff(cdf, axis=-1)
        for r in range(N):
            k = rng.permutation(np.nonzero((den[r] > 0) & (den[r] < 3e-5))[0])[:(Ni - 2) // 2]
            inside = (0.5 * (cdf[r, k].astype(np.float64) + cdf[r, k + 1])).astype(np.float32)
            inside[::4] = cdf[r, k[::4]]
            u[r, 2:2 + len(k)] = inside
    if Ni > 2:
        u[:, 0], u[:, 1] = 0.0, 1.0                        # the two ends of the cdf
    return np.sort(u, -1) if mode == "sorted" else u


def low_mass_draws(w, u, Ni):
    """how many draws of the case land strictly inside a bin with den < 1e-5 (by the replay): what the rule decides"""
    cdf, _ = RR.cdf_of(w)
    uu = RR.linspace_u(len(cdf), Ni) if u is None else u
    n = 0
    for r in range(len(cdf)):
        hi = np.searchsorted(cdf[r], uu[r], side="right")
        b, a = np.maximum(hi - 1, 0), np.minimum(hi, cdf.shape[1] - 1)
        n += int(((cdf[r, a] - cdf[r, b] < np.float32(1e-5)) & (a > b) & (uu[r] != cdf[r, b])).sum())
    return n


def standalone_vs_replay(g, bins, w, z, Ni, u, what, expect_tie=False):
    """swnerf_sample_pdf (+ merge + std when z is given) on device operands against the replay -> (z_sorted, z_std, explained rays).
    expect_tie: the case must hold a sample that equals a coarse depth exactly (the tie rule of wave_rank_merge: coarse first)"""
    N = bins.shape[0]
    nan = lambda *shape: torch.full(shape, float("nan"), device=DEV)
    smp = nan(N, Ni)
    zs, sd = (nan(N, z.shape[1] + Ni), nan(N)) if z is not None else (None, None)
    ud = None if u is None else T(u).to(DEV)
    pdf_abi(bins, w, Ni, ud, smp, z, zs, sd)
    got = _np(smp)
    explained = RR.compare_samples(_np(bins), _np(w), u, got, what)
    g.worst["draws inside bins with den < 1e-5"] = g.worst.get("draws inside bins with den < 1e-5", 0) + low_mass_draws(_np(w), u, Ni)
    g.true(explained <= 1, f"{what}: {explained} rays need a rounding-boundary cdf entry")
    lo, hi = _np(bins)[:, :1], _np(bins)[:, -1:]
    g.true(np.isfinite(got).all() and (got >= lo).all() and (got <= hi).all(), f"{what}: a sample outside [bins[0], bins[-1]]")
    if z is not None:
        if expect_tie:
            g.true((got[:, :, None] == _np(z)[:, None, :]).any((1, 2)).all(), f"{what}: a ray holds no exact tie between its samples and depths")
        g.true(np.array_equal(_np(zs).view(np.int32), RR.merge(_np(z), got).view(np.int32)), f"{what}: z_sorted != sort(cat[z, samples])")
        g.true(np.array_equal(_np(sd).view(np.int32), RR.zstd(got).view(np.int32)), f"{what}: z_std {_np(sd)[:4]} != {RR.zstd(got)[:4]}")
    return zs, sd, explained


@pytest.mark.parametrize("regime", ALL_REGIMES)
@pytest.mark.parametrize("variant", [v for v, s in VARIANTS.items() if s[4]])
def test_fused_resampling_bits(variant, regime):
    """(S, Ni) in {(3,1), (7,5), (33,95), (64,128), (65,37), (255,64), (256,768)} x u absent / given sorted / given random (the
    bitonic fallback, sort_n padded past a non-power-of-two Ni): z_fine and z_std of the pass == the standalone op on the pass's
    own weights and depths == the replay, all bit for bit; the static training forwards == the inference pass.  Given u is
    placed inside the bins without mass (draws); the sorted mode runs on given depths with exact ties, which u = 0 draws.
    Measured: every comparison equal, no ray needed a rounding-boundary explanation; draws inside bins with den < 1e-5 per case:
    wall 18 600, spike 15 300, all_opaque 6 720, soft_then_wall 3 010, mild 10, all_empty 0 (its pdf is uniform)."""
    kind, _, _, has_train, _ = VARIANTS[variant]
    rb = rays_of(kind)
    g = Gate()
    explained = 0
    for S, Ni in PAIRS:
        noise_np, zgiven = regime_noise(regime, S)
        noise = T(noise_np).to(DEV)
        for um in U_MODES:
            what = f"{variant} {regime} S={S} Ni={Ni} u={um}"
            kw = dict(noise=noise, white_bkgd=True)
            if um == "sorted":                                  # given depths with exact ties: z[1] == z[0] is also bin edge 0, which u = 0 draws
                kw["z_vals"] = T(with_ties(zgiven)).to(DEV)
            if um == "random":                                  # jittered coarse depths under random u, as perturb = 1 has them
                kw["t_rand"] = T(np.random.default_rng(S + 1).uniform(0, 1, (N_REF, S)).astype(np.float32)).to(DEV)
            cdf = None if um == "det" else RR.cdf_of(_np(infer(variant, rb, S, **kw)["weights"])[:, 1:-1])[0]     # of the weights the resampling will see
            u = draws(um, N_REF, Ni, 100 * S + Ni, cdf)
            kw.update(n_importance=Ni, u=None if u is None else T(u).to(DEV))
            out = infer(variant, rb, S, **kw)
            z, w = out["z_out"], out["weights"]
            bins = (.5 * (z[:, 1:] + z[:, :-1])).contiguous()
            zs, sd, ex = standalone_vs_replay(g, bins, w[:, 1:-1].contiguous(), z, Ni, u, what, expect_tie=um == "sorted" and Ni > 2)
            explained += ex
            g.true(torch.equal(bits(out["z_fine"]), bits(zs)), f"{what}: z_fine of the pass != the standalone op on the pass's weights")
            g.true(torch.equal(bits(out["z_std"]), bits(sd)), f"{what}: z_std of the pass != the standalone op")
            g.true(bool((out["z_fine"][:, 1:] >= out["z_fine"][:, :-1]).all()), f"{what}: z_fine not ascending")
            if regime == "all_empty":
                g.true(float(w.abs().max()) == 0.0, f"{what}: weights of an empty ray")
            if has_train and kind != "dnerf":                   # (the D-NeRF training pass has no resampling)
                tr, _ = train_forward(kind, rb, S, **kw)
                for k in out:
                    g.true(same(tr[k], out[k]), f"{what}: training forward differs from the inference pass in {k}")
            for n in (1, 3, 5):
                small = infer(variant, rb[:n], S, **first(kw, n))
                for k in ("z_fine", "z_std", "weights"):
                    g.true(same(small[k], out[k][:n]), f"{what}: N={n} differs from the prefix of N={N_REF} in {k}")
    g.worst["rays explained by a rounding boundary"] = explained
    g.finish(f"resampling {variant} {regime}")


@pytest.mark.parametrize("ns", [1, 64, 2048])
@pytest.mark.parametrize("nb", [2, 3, 65, 1024])
def test_standalone_sample_pdf_low_mass_bins_vs_replay(nb, ns):
    """swnerf_sample_pdf alone where tests/test_gpu_op_domain.py::pdf_inputs never goes: the weights of wall, spike and empty
    rays (float64 compositing of the regime, rounded), most bins with den on either side of 1e-5, depths with exact ties.  Bit for
    bit to the replay.  Measured: equal everywhere.  On scratch builds, den < 1e-6 in place of den < 1e-5 fails every case with
    nb >= 65 and ns >= 64 (samples), and `<` in place of `<=` in the merge's tie rule fails every case that merges (z_sorted)."""
    g = Gate()
    explained = 0
    S = nb + 1
    for regime in ("wall", "spike", "all_empty"):
        raw, z, d, _, _ = comp_inputs(regime, S, 50 * nb + ns + ALL_REGIMES.index(regime), N=5)
        z = with_ties(z)                                        # z[1] == z[0]: bin edge 0 is a coarse depth, and u = 0 draws it
        w = comp_reference(raw, z, d, None, False, None, False)[0][3].float().numpy()
        for um in ("det", "random"):
            what = f"sample_pdf {regime} nb={nb} ns={ns} u={um}"
            u = draws(um, 5, ns, nb + ns, RR.cdf_of(w[:, 1:-1])[0])
            zd = T(z).to(DEV) if S + ns <= 2048 else None
            _, _, ex = standalone_vs_replay(g, T(RR.mid_bins(z)).to(DEV), T(w[:, 1:-1]).to(DEV), zd, ns, u, what,
                                            expect_tie=um == "det" or ns > 2)
            explained += ex
    g.worst["rays explained by a rounding boundary"] = explained
    # each of the five spike rays has nb - 2 empty bins with a cdf step of 0.9994e-5 and gets (ns - 2) / 2 draws placed in such bins
    g.true(ns < 64 or nb < 65 or g.worst["draws inside bins with den < 1e-5"] >= 5, "the case never enters the den < 1e-5 rule")
    g.finish(f"standalone sample_pdf nb={nb} ns={ns}")


# --------------------------------------------------------------------------------------------- B. d_raw of the backward kernels
S_BWD = (2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 192, 255, 256)
BWD_KINDS = ("canon", "noview4", "noview5", "dnerf", "tnerf")
BATCHES = ((0, 5), (5, 8), (8, 9))     # N = 5, 3, 1 on disjoint rays: together they see every spike position of density_regimes
UPS = ("rgb", "disp", "acc", ("rgb", "disp", "acc"))


def backward_abi(kind, sv, fwd, rb, r0, r1, S, raw, z, noise, white, gr, d_raw, grads):
    """one launch of the backward entry point of `kind` on rays r0:r1; gr: g_rgb, g_disp, g_acc, g_raw (None = NULL)"""
    from swnerf import _lib
    L, net, N = _lib.lib(), net_of(kind), rb.shape[0]
    p = lambda t, per=1: _lib.ptr(None if t is None else t[r0 * per:r1 * per])
    st = _lib.stream_of(rb)
    ups = [p(t) for t in gr]
    if kind == "tnerf":
        rc = L.swnerf_render_pass_backward_tnerf(_lib.ptr(net.packed_bwd()), p(sv["act"], sv["act"].shape[0] // N), p(raw), p(z), p(rb), 12, p(noise),
                                                 r1 - r0, S, int(white), *ups, _lib.ptr(grads[0]), _lib.ptr(d_raw), st)
    elif kind == "dnerf":
        per = sv["bits"].numel() // N
        rc = L.swnerf_render_pass_backward_dnerf(_lib.ptr(net.packed_bwd(_lib.BWD_DNERF_FUSED)), p(sv["bits"], per), p(sv["bits_d"], per), p(raw), p(z),
                                                 p(rb), rb.shape[1], p(noise), p(fwd["dx"]), None, r1 - r0, S, int(white), 10, *ups,
                                                 _lib.ptr(grads[0]), _lib.ptr(grads[1]), _lib.ptr(d_raw), _lib.ptr(grads[2]), st)
    elif kind == "canon":
        rc = L.swnerf_render_pass_backward(_lib.ptr(net.packed_bwd()), p(sv["bits"], sv["bits"].numel() // N), p(raw), p(z), p(rb), rb.shape[1],
                                           p(noise), r1 - r0, S, int(white), *ups, _lib.ptr(grads[0]), _lib.ptr(d_raw), st)
    else:
        rc = L.swnerf_render_pass_backward_noview(_lib.ptr(net.packed_bwd_noview()), p(sv["bits"], sv["bits"].numel() // N), p(raw), p(z), p(rb),
                                                  rb.shape[1], p(noise), r1 - r0, S, int(white), int(kind[-1]), *ups, _lib.ptr(grads[0]),
                                                  _lib.ptr(d_raw), st)
    _lib.check(rc, f"render_pass_backward {kind}")


@pytest.mark.parametrize("S", S_BWD)
@pytest.mark.parametrize("kind", BWD_KINDS)
def test_fused_backward_d_raw_vs_float64(kind, S):
    """d_raw of the fused backward kernel of `kind` on chosen raw / depths / noise: six regimes x white on / off x noise on /
    absent x upstream {g_rgb, g_disp, g_acc, all three} x {with, without g_raw} x N in {5, 3, 1}, every element against float64
    autograd of the oracle at 2e-6 + 2e-4 |ref|.
    Measured: max |err| 2.3e-7 over all five kernels, 576 launches per case.  Without the `lane == 63` edge of the
    suffix scan (scratch build; CANON at S = 32, 63, 64, 65, 256 tried) S = 65 and 256 fail; S = 64 cannot show it: the last sample's dist is 1e10, so its e, and with it its
    sigma gradient, is 0 whatever R is."""
    from swnerf import _lib
    rb = rays_of(kind, 9)
    fwd, sv = train_forward(kind, rb, S)                            # valid act / bits / xs (/ dx) for 9 rays
    oc = 5 if kind == "noview5" else 4
    wide = 8 if kind.startswith("noview") else 4
    prow = (S + 31) // 32 * 32
    nact = _lib.lib().swnerf_tnerf_act_floats_per_row() if kind == "tnerf" else _lib.lib().swnerf_act_floats_per_row()
    grads = [torch.zeros((5 * prow, nact), device=DEV) for _ in range(2 if kind == "dnerf" else 1)]
    if kind == "dnerf":
        grads.append(torch.zeros((5 * prow, 4), device=DEV))       # g_dx
    d = _np(rb[:, 3:6])
    g = Gate()
    launches = 0
    for regime in ALL_REGIMES:
        raw_np, z_np, _, noise_np, ups_np = comp_inputs(regime, S, 7000 * S + ALL_REGIMES.index(regime), N=9)
        rng = np.random.default_rng(S + 17)
        if oc == 5:
            raw_np = np.concatenate([raw_np, rng.standard_normal((9, S, 1)).astype(np.float32)], -1)
        graw_np = rng.standard_normal((9, S, oc)).astype(np.float32)
        raw, z, noise, graw = (T(a).to(DEV) for a in (raw_np, z_np, noise_np, graw_np))
        ups = {k: T(ups_np[k]).to(DEV) for k in ("rgb", "disp", "acc")}
        relu = (raw_np[..., :3] > 0) if kind == "tnerf" else None       # tnerf_train_kernels.hip: d(pre-ReLU colour), the mask is raw > 0
        for white in (False, True):
            for nz_np, nz in ((None, None), (noise_np, noise)):
                _, ref = comp_reference(raw_np[..., :4], z_np, d, nz_np, white, ups_np, True, upstream=UPS)
                for which in UPS:
                    gr3 = [ups[k] if k in (which if isinstance(which, tuple) else (which,)) else None for k in ("rgb", "disp", "acc")]
                    for gq_np, gq in ((None, None), (graw_np, graw)):
                        want = ref[which].numpy() + (0.0 if gq_np is None else gq_np[..., :4].astype(np.float64))
                        if relu is not None:
                            want[..., :3] *= relu
                        for r0, r1 in BATCHES:
                            n = r1 - r0
                            what = f"{kind} {regime} S={S} N={n} white={white} noise={nz is not None} upstream={which} g_raw={gq is not None}"
                            out = Guarded((n * prow, wide), DEV)
                            backward_abi(kind, sv, fwd, rb, r0, r1, S, raw, z, nz, white, gr3 + [gq], out.out, grads)
                            launches += 1
                            out.check(what)
                            got = _np(out.out).reshape(n, prow, wide)
                            g.close(got[:, :S, :4], want[r0:r1], 2e-6, 2e-4, "d_raw", what)
                            g.true(not got[:, S:].any(), f"{what}: rows past S are not zero")
                            if wide == 8:
                                fifth = gq_np[r0:r1, :, 4] if (oc == 5 and gq_np is not None) else np.zeros((n, S), np.float32)
                                g.true(np.array_equal(got[:, :S, 4], fifth) and not got[:, :, 5:].any(), f"{what}: columns 4..7 of d_raw8")
                            if regime == "all_empty":
                                sig = gq_np[r0:r1, :, 3] if gq_np is not None else np.zeros((n, S), np.float32)
                                g.true(np.array_equal(got[:, :S, 3], sig), f"{what}: an empty ray has a sigma gradient")
                            g.true(all(bool(torch.isfinite(t[:n * prow]).all()) for t in grads), f"{what}: grad holds NaN or Inf")
    g.worst["launches"] = launches
    g.finish(f"d_raw {kind} S={S}")
