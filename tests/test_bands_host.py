"""The CPU side of tests/test_gpu_bands.py: what the band-count cases rest on is checked here, without a GPU.

  * `cases_bands.widen` really builds the same function: the float64 evaluation of the widened (10, 4, 10) net equals the
    narrow net's on every output of a pass;
  * the nets are not degenerate (0.05 < mean acc < 0.95, as test_gpu_sharded.py asks of its scene);
  * the fp32 oracle alone stays inside every forward gate against float64 at every triple - so a kernel that misses a gate
    is a finding about the kernel, not about the gate;
  * the gradient cases have no ReLU unit within 5e-6 of its kink in float64;
  * the float64 helpers parametrised on the bands (flipcheck, dnerf_ref, tnerf_train_ref) agree with plain float64 autograd
    of bands_ref's own restatement at a band count other than the default."""
import numpy as np
import pytest
import torch

import bands_ref as BR
import cases_bands as CB

T = torch.from_numpy
CASES = [(k, b) for k in CB.KINDS for b in CB.triples(k)]
GRAD_CASES = [(k, b) for k in CB.KINDS for b in CB.triples(k, CB.GRAD_TRIPLES)]
ids = lambda cases: [f"{k}-{b[0]}.{b[1]}.{b[2]}" for k, b in cases]


def _passes(kind, sd, rb, bands, dtype):
    """coarse pass on the oracle's depths, resampling, fine pass on the fp32 oracle's resampled depths"""
    z = BR.coarse_z(rb, CB.N_SAMPLES)
    c = BR.pass_ref(kind, sd, rb, z, bands, True, dtype)
    zf, _ = BR.resample_ref(z, BR.pass_ref(kind, sd, rb, z, bands, True)["weights"], CB.N_IMPORTANCE)
    return c, BR.pass_ref(kind, sd, rb, zf, bands, True, dtype)


@pytest.mark.parametrize("kind,bands", CASES, ids=ids(CASES))
def test_widened_net_is_the_same_function(kind, bands):
    sd = CB.weights(kind, bands)
    wide = CB.widen(kind, sd, bands)
    assert {k: v.shape for k, v in wide.items()} == {k: v.shape for k, v in CB.weights(kind, CB.CONTROL).items()}
    rb = T(CB.ray_batch(kind))
    for a, b in zip(_passes(kind, sd, rb, bands, torch.float64), _passes(kind, wide, rb, CB.wide_bands(kind), torch.float64)):
        for k in a:
            assert torch.equal(torch.isnan(a[k]), torch.isnan(b[k])), k
            assert float((a[k].nan_to_num() - b[k].nan_to_num()).abs().max()) <= 1e-11 * max(1.0, float(a[k].nan_to_num().abs().max())), k
    for name, w in wide.items():                              # shared_columns is the inverse of widen
        cols = CB.shared_columns(kind, name, bands)
        assert np.array_equal(w if cols is None else w[:, cols], sd[name]), name
        if cols is not None:
            rest = np.setdiff1d(np.arange(w.shape[1]), cols)
            assert not w[:, rest].any(), name


@pytest.mark.parametrize("kind,bands", CASES, ids=ids(CASES))
def test_opacity_is_not_degenerate_and_fp32_oracle_is_inside_the_gates(kind, bands):
    sd = CB.weights(kind, bands)
    rb = T(CB.ray_batch(kind))
    p32, p64 = _passes(kind, sd, rb, bands, torch.float32), _passes(kind, sd, rb, bands, torch.float64)
    for which, a, b in zip(("coarse", "fine"), p32, p64):
        assert 0.05 < float(b["acc_map"].mean()) < 0.95, (which, float(b["acc_map"].mean()))
        worst = BR.check_pass(a, b, kind, f"fp32 oracle vs float64 {kind} {bands} {which}")
        print(f"\n[parity] fp32 oracle vs float64, {kind} {bands} {which}: {BR.fmt(worst)}")
    if kind != "tnerf":
        # the resampled depths: the fp32 oracle against the same oracle on its float64 weights, inside the depth gate
        z = BR.coarse_z(rb, CB.N_SAMPLES)
        za, zb = BR.own_depth_error(kind, sd, rb, z, bands, CB.N_IMPORTANCE)
        own = BR.check_depths(za, zb, CB.N_SAMPLES, "z_fine", 0.9 if kind == "dnerf" else 0.99)
        sa = BR.resample_ref(z, p32[0]["weights"], CB.N_IMPORTANCE)[1]
        sb = BR.resample_ref(z, p64[0]["weights"].float(), CB.N_IMPORTANCE)[1]
        BR.check_pass(dict(z_std=sa), dict(z_std=sb), kind, "z_std", keys=["z_std"])
        print(f"\n[parity] fp32 oracle vs float64 weights, {kind} {bands}: {own} of {za.numel()} resampled depths move by > 2e-5")
    # the smallest pass the reference allows
    rb3 = rb[:3]
    z = BR.coarse_z(rb3, 2)
    BR.check_pass(BR.pass_ref(kind, sd, rb3, z, bands, False), BR.pass_ref(kind, sd, rb3, z, bands, False, torch.float64), kind, "n=3 S=2")
    # D-NeRF's canonical-only branch
    if kind == "dnerf":
        rb0 = T(CB.ray_batch(kind, t=0.0))
        a, b = _passes(kind, sd, rb0, bands, torch.float32)[0], _passes(kind, sd, rb0, bands, torch.float64)[0]
        assert float(b["dx"].abs().max()) == 0.0
        BR.check_pass(a, b, kind, "t = 0")


@pytest.mark.parametrize("kind,bands", GRAD_CASES, ids=ids(GRAD_CASES))
def test_gradient_cases_are_well_conditioned(kind, bands):
    sd = CB.weights(kind, bands)
    rb = T(CB.grad_rays(kind, bands))
    z = BR.coarse_z(rb, CB.GRAD_S)
    assert BR.risky_units(kind, sd, rb, z, bands) == 0
    assert 0.05 < float(BR.pass_ref(kind, sd, rb, z, bands, True, torch.float64)["acc_map"].mean()) < 0.95


def _loss64(ret, idx, tgt, wd, wa, n):
    ok = ~torch.isnan(ret["disp_map"])
    return (((ret["rgb_map"] - tgt[idx].double()) ** 2).sum() / (3 * n)
            + 0.01 * (torch.where(ok, ret["disp_map"], torch.zeros_like(ret["disp_map"])) * wd[idx].double()).sum() / n
            + 0.1 * (ret["acc_map"] * wa[idx].double()).sum() / n)


@pytest.mark.parametrize("kind", CB.KINDS)
def test_band_parametrised_helpers_agree_with_plain_float64_autograd(kind):
    """The flip-aware checkers at bands (6, 3, 9), fed the float64 autograd gradients of bands_ref's restatement of the same
    pass in place of a kernel's: they must accept them (no risky unit on these rays, so nothing is fitted)."""
    import dnerf_ref
    import flipcheck
    import tnerf_train_ref
    bands = CB.applicable(kind, (6, 3, 9))
    sd_np = CB.weights(kind, bands)
    rb = T(CB.grad_rays(kind, bands))
    n, S = rb.shape[0], CB.GRAD_S
    z = BR.coarse_z(rb, S)
    rng = np.random.default_rng(11)
    tgt, wd, wa = (T(rng.uniform(0, 1, s).astype(np.float32)) for s in ((n, 3), (n,), (n,)))
    sd = {k: v.requires_grad_(True) for k, v in BR.sd_of(sd_np, torch.float64).items()}
    pts = (rb[:, None, 0:3] + rb[:, None, 3:6] * z[..., None]).reshape(-1, 3)
    dirs = rb[:, None, -3:].expand(n, S, 3).reshape(-1, 3)
    ret = BR.pass_ref(kind, sd_np, rb, z, bands, True, torch.float64)     # values
    # the same pass with gradients: rows_ref on tensors that require grad
    import oracle.nerf_oracle as O
    Lp, Ld, Lt = bands
    ex, ed = O.embed(pts, Lp).double(), O.embed(dirs, Ld).double()
    if kind == "canon":
        raw, dx = O.nerf_mlp(sd, torch.cat([ex, ed], -1), ex.shape[1], ed.shape[1]), None
    elif kind == "noview":
        raw, dx = O.generic_mlp(sd, ex, 8, [4], ex.shape[1], 0, False), None
    else:
        et = O.embed(torch.full((n * S, 1), CB.FRAME_TIME), Lt).double()
        if kind == "tnerf":
            raw, dx = BR.tnerf_mlp(sd, ex, et, ed), None
        else:
            raw, dx = O.dnerf_mlp(sd, torch.cat([ex, ed], -1), et, multires=Lp, input_ch=ex.shape[1], input_ch_views=ed.shape[1])
    raw = raw.reshape(n, S, -1)
    assert float((raw.detach() - ret["raw"]).abs().max()) < 1e-12
    rgb, disp, acc, _, _ = O.raw2outputs(raw[..., :4], z.double(), rb[:, 3:6].double(), 0., True)
    _loss64(dict(rgb_map=rgb, disp_map=disp, acc_map=acc), torch.arange(n), tgt, wd, wa, n).backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).float() for k, v in sd.items()}
    ray_loss = lambda r, idx: _loss64(r, idx, tgt, wd, wa, n)
    stats = {}
    if kind in ("canon", "noview"):
        if kind == "noview":
            grads = {k: g for k, g in grads.items() if not k.startswith("views_linears")}
        fl = flipcheck.flip_aware_check(sd_np, rb, z, True, ray_loss, grads, kind, bands=(Lp, Ld), stats=stats)
    elif kind == "dnerf":
        fl = dnerf_ref.flip_aware_check(sd_np, rb, z, True, ray_loss, grads, kind, dx.detach().float().reshape(n, S, 3), bands=bands, stats=stats)
    else:
        fl = tnerf_train_ref.flip_aware_check({k: T(v) for k, v in sd_np.items()}, rb, z, True, ray_loss, grads, kind, bands=bands, stats=stats)
    # fp32 rounding of the float64 gradients: 6e-8.  (D-NeRF: the checker's truth takes x' = fl32(x + dx), this graph the float64
    # sum - the 2e-5 gate of the checker itself is what holds there.)
    assert fl == (0, 0) and (kind == "dnerf" or stats["worst"] < 1e-6), (fl, stats)
