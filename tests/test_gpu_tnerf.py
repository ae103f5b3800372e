"""The T-NeRF path on the MI355X: the fused pass (csrc/tnerf_kernels.hip) against the reference's outputs (G14) and the
float64 restatement (tnerf_ref.py), the op path (TNeRF.forward on the generic GEMMs with ELU) against both, the device ELU,
gradients through render_rays, the reference's failures, and a short training loop through create_tnerf."""
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(ROOT, "sw-nerf_amd"), os.path.join(HERE, "golden"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import cases_tnerf as C  # noqa: E402
import tnerf_ref as R    # noqa: E402

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(HERE, "golden", "g14_tnerf.npz"))
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def net():
    from swnerf.model import TNeRF
    m = TNeRF(**C.NET)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in C.weights().items()}, strict=True)
    return m.to(DEV).eval()


def _query():
    from swnerf import render_tnerf
    from swnerf.embedder import get_embedder
    embed_fn, _ = get_embedder(10, 3, 0)
    embedtime_fn, _ = get_embedder(10, 1, 0)
    embeddirs_fn, _ = get_embedder(4, 3, 0)
    return lambda inputs, viewdirs, ts, network_fn: render_tnerf.run_network(
        inputs, viewdirs, ts, network_fn, embed_fn=embed_fn, embeddirs_fn=embeddirs_fn, embedtime_fn=embedtime_fn,
        netchunk=1024 * 64)


def _case(name, N=C.N_RAYS, S=C.N_SAMPLES):
    kw = dict(C.CASES[name])
    T = lambda a: torch.from_numpy(a).to(DEV)
    z = T(C.given_z()) if kw.pop("z_vals", False) else None
    tr = T(C.legacy_rand(N, S)) if kw.pop("perturb", 0) else None
    std = kw.pop("raw_noise_std", 0)
    nz = T(C.legacy_rand(N, S)) * std if std else None
    return dict(z_vals=z, t_rand=tr, noise=nz, **kw)


@pytest.mark.parametrize("name", list(C.CASES))
def test_fused_pass_vs_g14(net, name):
    from swnerf.render_tnerf import render_pass_tnerf
    rb = torch.from_numpy(C.rays()).to(DEV)
    with torch.no_grad():
        o = render_pass_tnerf(rb, net, C.N_SAMPLES, want=("rgb_map", "disp_map", "acc_map", "raw", "z_out"), **_case(name))
    o = {k: v.cpu().numpy() for k, v in o.items()}
    raw_ref = G[f"{name}_raw"]
    err = np.abs(o["raw"][:C.KEEP] - raw_ref)
    print(f"{name}: max |d raw| {err.max():.3e}, rel {(err / np.maximum(np.abs(raw_ref), 1e-3)).max():.3e}; "
          + ", ".join(f"{k} {np.abs(o[k] - G[f'{name}_{k}']).max():.3e}" for k in ("rgb_map", "acc_map", "disp_map")))
    # gates about 3x the errors measured on MI355X over all six cases: raw 9.3e-6 abs (values up to ~7),
    # rgb 7.2e-7, acc 4.2e-7, disp 1.5e-7
    assert np.all(err <= 3e-5 + 1e-5 * np.abs(raw_ref)), float(err.max())
    np.testing.assert_allclose(o["rgb_map"], G[f"{name}_rgb_map"], rtol=0, atol=2e-6)
    np.testing.assert_allclose(o["acc_map"], G[f"{name}_acc_map"], rtol=0, atol=2e-6)
    np.testing.assert_allclose(o["disp_map"], G[f"{name}_disp_map"], rtol=1e-5, atol=5e-7)
    if C.CASES[name].get("z_vals"):
        return
    np.testing.assert_array_equal(o["z_out"][:C.KEEP], G[f"{name}_z_vals"])


@pytest.mark.parametrize("n", [1, 3, 257, 301])
def test_fused_pass_ragged_vs_float64(net, n):
    from swnerf.render_tnerf import render_pass_tnerf
    rbn = C.rays(n=n, seed=40 + n)
    S = 40
    sd = {k: v.detach().double() for k, v in net.state_dict().items()}
    rb = torch.from_numpy(rbn).to(DEV)
    with torch.no_grad():
        o = render_pass_tnerf(rb, net, S, white_bkgd=True, want=("rgb_map", "disp_map", "acc_map", "raw"))
        r = R.render_rays(sd, rb, S, white_bkgd=True)
        for k in ("rgb_map", "acc_map"):
            assert float((o[k].double() - r[k]).abs().max()) < 2e-5, k
        assert float(((o["raw"].double() - r["raw"]).abs() - 1e-4 * r["raw"].abs()).max()) < 2e-4
        # chunks of the fused pass give the same bits as one launch
        parts = [render_pass_tnerf(rb[i:i + 64], net, S, white_bkgd=True, want=("rgb_map", "raw")) for i in range(0, n, 64)]
        assert torch.equal(torch.cat([p["rgb_map"] for p in parts]), o["rgb_map"])
        assert torch.equal(torch.cat([p["raw"] for p in parts]), o["raw"])


def test_render_rays_fused_vs_op_path(net):
    from swnerf import render_tnerf
    rb = torch.from_numpy(C.rays(n=64)).to(DEV)
    q = _query()
    with torch.no_grad():
        assert render_tnerf.tnerf_plan(q, net) == (10, 4, 10)
        f = render_tnerf.render_rays(rb, net, q, 64, retraw=True, white_bkgd=True)
        plain = lambda inputs, viewdirs, ts, network_fn: q(inputs, viewdirs, ts, network_fn)    # no encoders visible: op path
        assert render_tnerf.tnerf_plan(plain, net) is None
        u = render_tnerf.render_rays(rb, net, plain, 64, retraw=True, white_bkgd=True)
    assert set(f) == set(u) == {"rgb_map", "disp_map", "acc_map", "z_vals", "raw"}
    assert torch.equal(f["z_vals"], u["z_vals"])
    assert float((f["raw"] - u["raw"]).abs().max()) < 2e-4
    assert float((f["rgb_map"] - u["rgb_map"]).abs().max()) < 2e-5


def test_device_elu_accuracy():
    from swnerf import generic, _lib
    x = torch.linspace(-20., 0., 1 << 16, dtype=torch.float32, device=DEV)
    xs = torch.cat([x, torch.tensor([1e-8, 0.5, 3.0, -1e-30], device=DEV)])
    lin = torch.nn.Linear(32, 32).to(DEV)
    with torch.no_grad():
        lin.weight.copy_(torch.eye(32, device=DEV))
        lin.bias.zero_()
        X = torch.zeros((xs.numel(), 32), device=DEV)
        X[:, 5] = xs
        y = generic.linear(X, lin, act=_lib.ACT_ELU)[:, 5]
    ref = torch.where(xs.double() > 0, xs.double(), torch.expm1(xs.double()))
    err = float((y.double() - ref).abs().max())
    assert err <= 1.2e-7, err


def test_gradients_vs_float64(net):
    """loss.backward() through render_tnerf.render_rays (the op path under grad) against float64 autograd of the same
    function, with the colour and sigma ReLUs accounted for by their exact flip effects (tnerf_ref.flip_aware_check)."""
    from swnerf import render_tnerf
    from swnerf.model import TNeRF
    m = TNeRF(**C.NET).to(DEV)
    m.load_state_dict(net.state_dict())
    n, S = 48, 32
    rb = torch.from_numpy(C.rays(n=n, seed=77)).to(DEV)
    out = render_tnerf.render_rays(rb, m, _query(), S, white_bkgd=True)
    tgt = torch.rand((n, 3), generator=torch.Generator().manual_seed(3))
    loss = ((out["rgb_map"] - tgt.to(DEV)) ** 2).mean()
    loss.backward()
    ray_loss = lambda ret, idx: ((ret["rgb_map"] - tgt[idx].double()) ** 2).sum() / (n * 3)
    sd32 = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    flips, risky = R.flip_aware_check(sd32, rb.cpu(), out["z_vals"].detach().cpu(), True, ray_loss,
                                      {k: p.grad for k, p in m.named_parameters()}, "tnerf op path")
    print(f"gradients: {flips} ReLU flips of {risky} risky units")


@pytest.mark.parametrize("depth", [5, 9])
def test_reference_failures_reproduced(depth):
    from swnerf.model import TNeRF
    m = TNeRF(depth, 63, 27, 21).to(DEV)
    inp, vd, t = torch.rand(8, 90, device=DEV), torch.rand(8, 27, device=DEV), torch.rand(8, 21, device=DEV)
    with torch.no_grad(), pytest.raises(RuntimeError):
        m(inp, vd, t)
    with torch.no_grad(), pytest.raises(Exception):
        TNeRF(8, 63, 27, 21).to(DEV)(inp, None, t)


def test_training_loop_and_checkpoint(tmp_path):
    from swnerf import render_tnerf
    from swnerf.runner import create_tnerf
    from swnerf.checkpoint import save_checkpoint
    args = types.SimpleNamespace(multires=10, i_embed=0, use_viewdirs=True, multires_views=4, netdepth=8, netchunk=65536,
                                 nerf_type="original", lrate=5e-4, do_half_precision=False, ft_path=None, no_reload=False,
                                 perturb=1., N_samples=32, white_bkgd=True, raw_noise_std=0., dataset_type="blender",
                                 no_ndc=False, lindisp=False, basedir=str(tmp_path), expname="exp")
    torch.manual_seed(0)
    tr, te, start, gv, opt = create_tnerf(args, device=DEV)
    assert start == 0
    rb = torch.from_numpy(C.rays(n=256, seed=5)).to(DEV)
    kw = lambda d: {k: v for k, v in d.items() if k not in ("ndc", "use_viewdirs")}     # render()'s own options
    tgt = torch.full((256, 3), 0.3, device=DEV)
    losses = []
    for _ in range(30):
        out = render_tnerf.render_rays(rb, **kw(tr))
        loss = ((out["rgb_map"] - tgt) ** 2).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss))
    assert losses[-1] < 0.7 * losses[0], losses
    save_checkpoint(str(tmp_path), "exp", 30, 30, tr["network_fn"], None, opt)
    tr2, te2, start2, gv2, opt2 = create_tnerf(args, device=DEV)
    assert start2 == 30
    for a, b in zip(tr["network_fn"].state_dict().values(), tr2["network_fn"].state_dict().values()):
        assert torch.equal(a, b)
    with torch.no_grad():
        f1 = render_tnerf.render_rays(rb, **kw(te))
        f2 = render_tnerf.render_rays(rb, **kw(te2))
    assert torch.equal(f1["rgb_map"], f2["rgb_map"])


def test_render_and_render_path_frame(net, tmp_path):
    """render() and render_path() on a small frame: the fused pass through get_rays, the ray batch, batchify_rays and the
    reshape; equal to one direct launch on the same rays, and render_path writes the frames."""
    from swnerf import render_tnerf, synth
    from swnerf.ray import get_rays
    H = W = 48
    K, c2w = synth.lego_camera(H, W)
    q = _query()
    kw = dict(network_fn=net, network_query_fn=q, N_samples=40, white_bkgd=True, perturb=0., raw_noise_std=0., lindisp=False)
    with torch.no_grad():
        rgb, disp, acc, extras = render_tnerf.render(H, W, K[0][0], chunk=1000, c2w=torch.from_numpy(c2w[:3, :4]).to(DEV), ndc=False,
                                                     near=2., far=6., frame_time=0.375, use_viewdirs=True, **kw)
        assert rgb.shape == (H, W, 3) and disp.shape == (H, W) and acc.shape == (H, W) and extras["z_vals"].shape == (H, W, 40)
        o, d = get_rays(H, W, K[0][0], torch.from_numpy(c2w[:3, :4]).to(DEV))
        o, d = o.reshape(-1, 3).float(), d.reshape(-1, 3).float()
        vd = d / torch.norm(d, dim=-1, keepdim=True)
        one = torch.ones_like(d[:, :1])
        rb = torch.cat([o, d, 2. * one, 6. * one, 0.375 * one, vd], -1)
        ref = render_tnerf.render_pass_tnerf(rb, net, 40, white_bkgd=True)
        assert torch.equal(rgb.reshape(-1, 3), ref["rgb_map"]) and torch.equal(acc.reshape(-1), ref["acc_map"])
        assert 0.05 < float(acc.min()) and float(acc.max()) > 0.9
        poses = np.stack([c2w, c2w])
        kw2 = dict(kw, ndc=False, near=2., far=6., use_viewdirs=True)
        rgbs, disps = render_tnerf.render_path(torch.from_numpy(poses).to(DEV), [0.375, 0.375], (H, W, K[0][0]), 1000, kw2,
                                               savedir=str(tmp_path))
    assert rgbs.shape == (2, H, W, 3) and np.array_equal(rgbs[0], rgb.cpu().numpy())
    assert sorted(os.listdir(tmp_path / "estim")) == ["000.png", "001.png"]


def test_fused_path_keeps_reference_refusals(net):
    """Where run_network refuses, render_rays refuses on the fused path too: two frame times in one batch (the assertion of
    run_tnerf.py:52), and embd_time_discr False (nerf_type 'temporal': NotImplementedError)."""
    from swnerf import render_tnerf
    from swnerf.embedder import get_embedder
    rb = torch.from_numpy(C.rays(n=8)).to(DEV)
    rb2 = rb.clone()
    rb2[4:, 8] = 0.5
    q = _query()
    with torch.no_grad():
        with pytest.raises(AssertionError, match="same time"):
            render_tnerf.render_rays(rb2, net, q, 32)
        embed_fn, _ = get_embedder(10, 3, 0)
        embedtime_fn, _ = get_embedder(10, 1, 0)
        embeddirs_fn, _ = get_embedder(4, 3, 0)
        args = types.SimpleNamespace(nerf_type="temporal")
        qt = lambda inputs, viewdirs, ts, network_fn: render_tnerf.run_network(
            inputs, viewdirs, ts, network_fn, embed_fn=embed_fn, embeddirs_fn=embeddirs_fn, embedtime_fn=embedtime_fn,
            netchunk=1024 * 64, embd_time_discr=args.nerf_type != "temporal")
        assert render_tnerf.tnerf_plan(qt, net) is None
        with pytest.raises(NotImplementedError):
            render_tnerf.render_rays(rb, net, qt, 32)
