"""D-NeRF training gradients against the float64 evaluation with exact ReLU-flip accounting (tests/dnerf_ref.py), gate 2e-5
of each tensor's max: the module-level backward (`_DnerfTrain`), a training step with the TV loss on the op path, the fused
pass (swnerf_render_pass_train_dnerf / _backward_dnerf) at the shapes of test_fused_dnerf_training_pass_matches_op_path, and
seeded random shapes.  The truth is evaluated at the KERNEL's own x' = fl32(x + position_delta); every test also prints how
far that position_delta is from the float64 one (the fp32 CPU oracle's own distance: 1.3e-7)."""
import os

import numpy as np
import pytest
import torch

import cases
import dnerf_ref
from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
DX_ATOL = 1e-6                       # position_delta vs float64: the bound test_gpu_query_time.py holds the inference kernels to


@pytest.fixture(autouse=True)
def _grad():
    with torch.enable_grad():
        yield


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _dnerf_net(dev, sd_np):
    import swnerf.embedder as embedder, swnerf.model as model
    embed_fn, _ = embedder.get_embedder(10, 3, 0)
    m = model.DirectTemporalNeRF(D=8, W=256, input_ch=63, input_ch_views=27, input_ch_time=21, output_ch=5, skips=[4],
                                 use_viewdirs=True, embed_fn=embed_fn, zero_canonical=True)
    m.load_state_dict({k: T(v) for k, v in sd_np.items()})
    return m.to(dev)


def _query(netchunk):
    import swnerf.embedder as embedder, swnerf.render_dnerf as rd
    embed_fn, _ = embedder.get_embedder(10, 3, 0)
    embeddirs_fn, _ = embedder.get_embedder(4, 3, 0)
    embedtime_fn, _ = embedder.get_embedder(10, 1, 0)
    return lambda inputs, viewdirs, ts, network_fn: rd.run_network(inputs, viewdirs, ts, network_fn, embed_fn=embed_fn,
                                                                   embeddirs_fn=embeddirs_fn, embedtime_fn=embedtime_fn, netchunk=netchunk)


def _dx_distance(sd_np, rb, z, dx):
    """max |position_delta - float64 dx| on the samples of rays rb at depths z (0.0 at t == 0, where both are exactly zero)"""
    if float(rb[0, 8]) == 0.0:
        assert float(dx.abs().max()) == 0.0
        return 0.0
    ex, et, _, _ = dnerf_ref.ray_encodings(rb, z)
    d = float((dx.detach().cpu().reshape(-1, 3).double() - dnerf_ref.float64_dx(sd_np, ex, et)).abs().max())
    assert d <= DX_ATOL, f"position_delta is {d:.3e} from the float64 deformation net"
    return d


def _check(sd_np, rb, z, white, ray_loss, grads, what, dx, **kw):
    """-> 'F flips of R risky units, worst residual W, |dx - float64 dx| D' after the 2e-5 gate has held"""
    stats = {}
    ddx = _dx_distance(sd_np, rb, z, dx)
    flips, risky = dnerf_ref.flip_aware_check(sd_np, rb, z, white, ray_loss, grads, what, dx.detach().cpu(), stats=stats, **kw)
    return f"{flips} flips of {risky} risky units, worst residual {stats['worst']:.2e}, |dx - float64 dx| {ddx:.2e}"


class _Spy:
    """Counts the C entry points that get called (as test_reference_train_call_takes_the_fused_kernels does)."""

    def __init__(self, lib, calls):
        object.__setattr__(self, "_l", lib)
        object.__setattr__(self, "_calls", calls)

    def __getattr__(self, name):
        f = getattr(self._l, name)
        if not name.startswith("swnerf_"):
            return f

        def wrapped(*a, **k):
            self._calls[name] = self._calls.get(name, 0) + 1
            return f(*a, **k)
        return wrapped


OP_PATH_ENTRIES = ("swnerf_deform_forward_train", "swnerf_mlp_forward_train", "swnerf_embed", "swnerf_raw2outputs",
                   "swnerf_mlp_backward_dx_pts", "swnerf_deform_backward_dx")


def _spy(monkeypatch):
    from swnerf import _lib
    calls = {}
    real = _lib.lib()
    while isinstance(real, _Spy):                        # a test that calls this per case counts each case on the library itself
        real = real._l
    spy = _Spy(real, calls)
    monkeypatch.setattr(_lib, "lib", lambda: spy)
    return calls


# ---- a. module level, op path ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 32, 300])
def test_dnerf_module_backward_vs_float64(dev, M):
    """`_DnerfTrain` through DirectTemporalNeRF.forward at t = 0.5 on the inputs of test_dnerf_mlp_backward_matches_autograd:
    gradients on out and dx, then on dx alone (`_occ` must get exactly zero).  Rows are independent: each is a unit of one sample."""
    sd_np = cases.weights_dnerf()
    x = T(cases.g4_inputs()["x"][:M])
    t_emb = O.embed(torch.full((M, 1), 0.5), 10)
    rng = np.random.default_rng(19)
    G, Gdx = T(rng.standard_normal((M, 4)).astype(np.float32)), T(rng.standard_normal((M, 3)).astype(np.float32))
    net = _dnerf_net(dev, sd_np)
    ex, ed = x[:, :63], x[:, 63:]
    dx64 = dnerf_ref.float64_dx(sd_np, ex, t_emb)
    for dx_only in (False, True):
        net.zero_grad()
        out, dx = net(x.to(dev), [t_emb.to(dev), t_emb.to(dev)])
        loss = (dx * Gdx.to(dev)).sum()
        if not dx_only:
            loss = loss + (out * G.to(dev)).sum()
        loss.backward()

        def row_loss(ret, idx):
            L = (ret["position_delta"][:, 0] * Gdx[idx]).sum()
            return L if dx_only else L + (ret["raw"][:, 0] * G[idx]).sum()
        ddx = float((dx.detach().cpu().double() - dx64).abs().max())
        assert ddx <= DX_ATOL, f"dx is {ddx:.3e} from the float64 deformation net"
        stats = {}
        grads = {k: p.grad for k, p in net.named_parameters()}
        flips, risky = dnerf_ref.flip_aware_check_rows(sd_np, ex, t_emb, ed, row_loss, grads, f"module M={M} dx_only={dx_only}",
                                                       dx.detach().cpu(), stats=stats)
        if dx_only:
            assert all(g is not None and float(g.abs().max()) == 0.0 for k, g in grads.items() if k.startswith("_occ"))
        print(f"\n[parity] D-NeRF module backward M={M} {'dx only' if dx_only else 'out + dx'}: within 2e-5 of float64; {flips} flips of "
              f"{risky} risky units, worst residual {stats['worst']:.2e}, |dx - float64 dx| {ddx:.2e}")


# ---- b. training step with the TV loss on the op path ----------------------------------------------------------------------
def test_dnerf_tv_step_op_path_vs_float64(dev, monkeypatch):
    """The loss of test_dnerf_training_step_with_tv_loss (d_nerf/run_dnerf.py:690-725) at n = 40, S = 64, times 0.5 and 0.45 on
    shared depths, through render_rays on the differentiable op path."""
    import swnerf.render_dnerf as rd
    monkeypatch.setenv("SWNERF_TRAIN_OP_PATH", "1")
    calls = _spy(monkeypatch)
    sd_np = cases.weights_dnerf()
    n, S, tv_w = 40, 64, 0.1
    g = cases.g8_inputs(n=n)
    rb = lambda t: O.make_ray_batch(T(g["rays_o"]), T(g["rays_d"]), 2., 6., frame_time=t)
    target = T(np.random.default_rng(5).uniform(0, 1, (n, 3)).astype(np.float32))
    q = _query(1024)
    net = _dnerf_net(dev, sd_np)
    e1 = rd.render_rays(rb(0.5).to(dev), net, q, S, retraw=True, white_bkgd=True, perturb=0., raw_noise_std=0.)
    e0 = rd.render_rays(rb(0.45).to(dev), net, q, S, retraw=True, white_bkgd=True, z_vals=e1["z_vals"].detach())
    (torch.mean((e1["rgb_map"] - target.to(dev)) ** 2) + tv_w * (e1["position_delta"] - e0["position_delta"]).pow(2).sum()).backward()
    assert calls.get("swnerf_deform_forward_train") == 2 and not any(k.startswith("swnerf_render_pass_train") for k in calls)
    z = e1["z_vals"].detach().cpu()

    def ray_loss(r, idx):
        return ((r["rgb_map"] - target[idx].to(r["raw"])) ** 2).sum() / (3 * n) + tv_w * (r["position_delta"] - r["position_delta_2"]).pow(2).sum()
    res = _check(sd_np, rb(0.5), z, True, ray_loss, {k: p.grad for k, p in net.named_parameters()}, "TV step on the op path",
                 e1["position_delta"], second=(0.45, z))
    d2 = _dx_distance(sd_np, rb(0.45), z, e0["position_delta"])
    print(f"\n[parity] D-NeRF training step with TV loss, op path ({n} x {S} rows, t = 0.5 / 0.45): within 2e-5 of float64; {res} "
          f"(second time {d2:.2e})")


# ---- c. the fused pass --------------------------------------------------------------------------------------------------
def _fused_case(dev, monkeypatch, what, sd_c, sd_f, rb_of, t, t2, n, S, Ni, two, tv_w, kw, seed):
    """One training step through rd.render_rays on the fused kernels with the loss of
    test_fused_dnerf_training_pass_matches_op_path (image MSE, TV on shared depths at t2, a term on raw, a term on acc_map) plus a
    NaN-guarded disp_map term; every parameter gradient of the net(s) against float64.  -> the [parity] text"""
    import swnerf.render as render, swnerf.render_dnerf as rd
    monkeypatch.delenv("SWNERF_TRAIN_OP_PATH", raising=False)
    calls = _spy(monkeypatch)
    rng = np.random.default_rng(seed)
    S1 = S + Ni
    tgt = T(rng.uniform(0, 1, (n, 3)).astype(np.float32))
    wr = T((1e-3 * rng.standard_normal((n, S1, 4))).astype(np.float32))
    wd = T(rng.standard_normal(n).astype(np.float32))
    q = _query(1024 * 64)
    net = _dnerf_net(dev, sd_c)
    fine = _dnerf_net(dev, sd_f) if two else None                                # use_two_models_for_fine (run_dnerf.py:410-416)
    kw2 = dict(network_fine=fine, use_two_models_for_fine=two, white_bkgd=kw["white_bkgd"], retraw=True)
    rb1 = rb_of(t)
    e1 = rd.render_rays(rb1.to(dev), net, q, S, N_importance=Ni, lindisp=kw["lindisp"], perturb=kw["perturb"], raw_noise_std=kw["raw_noise_std"],
                        pytest=True, **kw2)
    c = lambda a: a.to(dev)
    ok = ~torch.isnan(e1["disp_map"])
    loss = torch.mean((e1["rgb_map"] - c(tgt)) ** 2) + (e1["raw"] * c(wr)).sum() + 0.05 * e1["acc_map"].mean() \
        + 0.01 * (torch.where(ok, e1["disp_map"], torch.zeros_like(e1["disp_map"])) * c(wd)).mean()
    e0 = None
    if tv_w:
        e0 = rd.render_rays(rb_of(t2).to(dev), net, q, S, N_importance=Ni, z_vals=e1["z_vals"].detach(), **kw2)
        loss = loss + tv_w * (e1["position_delta"] - e0["position_delta"]).pow(2).sum() / n
    if two:
        loss = loss + torch.mean((e1["rgb0"] - c(tgt)) ** 2) + 0.1 * e1["position_delta_0"].pow(2).sum() / n
    loss.backward()
    # the fused kernels ran, not quietly the op path
    deform1, deform2 = rd.runs_deform(net, t), bool(tv_w)
    passes = (2 if two else 1)
    n_dnerf = passes * int(deform1) + int(deform2)
    n_static = passes * int(not deform1)
    assert calls.get("swnerf_render_pass_train_dnerf", 0) == n_dnerf and calls.get("swnerf_render_pass_train", 0) == n_static, calls
    assert calls.get("swnerf_render_pass_backward_dnerf", 0) >= n_dnerf and calls.get("swnerf_render_pass_backward", 0) >= n_static, calls
    assert not any(k in calls for k in OP_PATH_ENTRIES), calls

    def draw(shape, scale):                                                      # what pytest=True draws: every draw restarts from seed 0
        np.random.seed(0)
        return T((np.random.rand(*shape) * scale).astype(np.float32))
    noise_of = lambda s: draw((n, s), kw["raw_noise_std"]) if kw["raw_noise_std"] > 0 else None
    z1 = e1["z_vals"].detach().cpu()
    assert z1.shape == (n, S1)

    def ray_loss(r, idx):                                                        # the final pass's part of the loss, as a sum over rays
        a = lambda t_: t_[idx].to(r["raw"])
        okr = ~torch.isnan(r["disp_map"])
        L = ((r["rgb_map"] - a(tgt)) ** 2).sum() / (3 * n) + (r["raw"] * a(wr)).sum() + 0.05 * r["acc_map"].sum() / n \
            + 0.01 * (torch.where(okr, r["disp_map"], torch.zeros_like(r["disp_map"])) * a(wd)).sum() / n
        if tv_w:
            L = L + tv_w * (r["position_delta"] - r["position_delta_2"]).pow(2).sum() / n
        return L
    second = (t2, z1) if tv_w else None
    final = fine if two else net
    res = _check(sd_f if two else sd_c, rb1, z1, kw["white_bkgd"], ray_loss, {k: p.grad for k, p in final.named_parameters()},
                 what + (" fine net" if two else ""), e1["position_delta"], second=second, noise=noise_of(S1))
    if e0 is not None:
        _dx_distance(sd_f if two else sd_c, rb_of(t2), z1, e0["position_delta"])
    if two:                                                                      # the coarse net on its own depths: rgb0 / position_delta_0
        t_rand = draw((n, S), 1.0) if kw["perturb"] > 0 else None
        with torch.no_grad():
            z0 = render.render_pass(rb1.to(dev), net, S, lindisp=kw["lindisp"], t_rand=None if t_rand is None else t_rand.to(dev),
                                    white_bkgd=kw["white_bkgd"], want=["z_out"], run_deform=deform1)["z_out"].cpu()
        coarse_loss = lambda r, idx: ((r["rgb_map"] - tgt[idx].to(r["raw"])) ** 2).sum() / (3 * n) + 0.1 * r["position_delta"].pow(2).sum() / n
        res0 = _check(sd_c, rb1, z0, kw["white_bkgd"], coarse_loss, {k: p.grad for k, p in net.named_parameters()}, what + " coarse net",
                      e1["position_delta_0"], noise=noise_of(S))
        res = f"fine {res}; coarse {res0}"
    return res


@pytest.mark.parametrize("n,S,Ni,t,two", [(40, 64, 128, 0.5, False), (21, 40, 0, 0.25, False), (12, 64, 128, 0.0, False), (10, 64, 64, 0.5, True)])
def test_fused_dnerf_pass_vs_float64(dev, monkeypatch, n, S, Ni, t, two):
    """swnerf_render_pass_train_dnerf / swnerf_render_pass_backward_dnerf at the shapes of
    test_fused_dnerf_training_pass_matches_op_path, several ragged backward chunks.  One model: the coarse pass runs under
    no_grad, the net is checked on the final depths (ret['z_vals']); two models: the coarse net on its own depths with rgb0 /
    position_delta_0, the fine net separately.  t == 0 (zero_canonical): the static fused pass on `_occ`, and `_time` trained
    by the TV term's second time alone."""
    import swnerf.render as render
    monkeypatch.setattr(render, "TRAIN_BWD_CHUNK_ROWS", 4096 if n != 40 else 393216)
    sd_np = cases.weights_dnerf()
    g = cases.g8_inputs(n=n)
    rb_of = lambda t_: O.make_ray_batch(T(g["rays_o"]), T(g["rays_d"]), 2., 6., frame_time=t_)
    kw = dict(white_bkgd=True, lindisp=False, perturb=0., raw_noise_std=0.)
    what = f"fused D-NeRF pass N={n} S={S}+{Ni} t={t} {'two models' if two else 'one model'}"
    res = _fused_case(dev, monkeypatch, what, sd_np, sd_np, rb_of, t, float(np.float32(t + 0.03)), n, S, Ni, two, 0.1, kw, seed=8 + n)
    print(f"\n[parity] {what}: every gradient within 2e-5 of float64; {res}")


# ---- d. random shapes ----------------------------------------------------------------------------------------------------
def test_random_dnerf_training_shapes(dev, monkeypatch):
    """The D-NeRF twin of test_random_training_shapes.  Seeded: the same cases every run (SWNERF_TRAIN_RANDOM_CASES of them)."""
    import swnerf.render as render
    rng = np.random.default_rng(4200)
    sd_np = cases.weights_dnerf()
    for case in range(int(os.environ.get("SWNERF_TRAIN_RANDOM_CASES", "10"))):
        n, S = int(rng.integers(1, 41)), int(rng.choice([2, 3, 17, 31, 32, 33, 48, 64, 65, 96, 127]))
        Ni = int(rng.choice([0, 1, 16, 40, 128]))
        if Ni:
            S = max(S, 3)                                                        # the resampling needs three coarse samples
            Ni = min(Ni, render.TRAIN_FUSED_MAX_SAMPLES - S)
        white, lindisp, jitter = bool(rng.integers(2)), bool(rng.integers(2)), bool(rng.integers(2))
        noise_std = float(rng.choice([0., 0.7]))
        monkeypatch.setattr(render, "TRAIN_BWD_CHUNK_ROWS", int(rng.choice([64, 1024, 393216])))
        t = 0.0 if rng.integers(5) == 0 else float(np.float32(1.0 - rng.uniform(0, 1)))      # (0, 1], as float32
        two = bool(rng.integers(2)) and Ni > 0
        tv_w = 0.1 * float(rng.integers(2))
        g = cases.g7_inputs(n=n, seed=6000 + 17 * case)
        rb_of = lambda t_: O.make_ray_batch(T(g["rays_o"]), T(g["rays_d"]), 2., 6., frame_time=t_)
        kw = dict(white_bkgd=white, lindisp=lindisp, perturb=1. if jitter else 0., raw_noise_std=noise_std)
        what = (f"case {case} n={n} S={S}+{Ni} t={t:.6f} {'two models' if two else 'one model'} tv={tv_w} white={white} lindisp={lindisp} "
                f"jitter={jitter} noise={noise_std}")
        res = _fused_case(dev, monkeypatch, what, sd_np, sd_np, rb_of, t, float(np.float32(t + 0.03)), n, S, Ni, two, tv_w, kw, seed=7000 + case)
        print(f"\n[parity] {what}: gradients within 2e-5 of float64; {res}")
