"""The fused T-NeRF training pass on the MI355X (csrc/tnerf_train_kernels.hip, swnerf.render_tnerf fused_train=True): the
forward against the inference pass bit for bit, loss.backward() against float64 autograd with ReLU-flip accounting
(tnerf_ref.flip_aware_check / tnerf_train_ref.flip_aware_check, gate 2e-5 of each tensor's max), chunking, the fall-backs to
the op path, the unchanged default, and runner.train_tnerf."""
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
import cases_tnerf as C        # noqa: E402
import tnerf_ref as R          # noqa: E402
import tnerf_train_ref as TR   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NEW_ENTRIES = ("swnerf_render_pass_train_tnerf", "swnerf_render_pass_backward_tnerf", "swnerf_pack_net_bwd_tnerf", "swnerf_tnerf_feature_finish")


def _net(grad=True):
    from swnerf.model import TNeRF
    m = TNeRF(**C.NET)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in C.weights().items()}, strict=True)
    m = m.to(DEV)
    for p in m.parameters():
        p.requires_grad_(grad)
    return m


@pytest.fixture(scope="module")
def net():
    return _net()


@pytest.fixture(scope="module")
def sd32():
    return {k: torch.from_numpy(v) for k, v in C.weights().items()}


def _query():
    from swnerf import render_tnerf
    from swnerf.embedder import get_embedder
    embed_fn, _ = get_embedder(10, 3, 0)
    embedtime_fn, _ = get_embedder(10, 1, 0)
    embeddirs_fn, _ = get_embedder(4, 3, 0)
    return lambda inputs, viewdirs, ts, network_fn: render_tnerf.run_network(
        inputs, viewdirs, ts, network_fn, embed_fn=embed_fn, embeddirs_fn=embeddirs_fn, embedtime_fn=embedtime_fn,
        netchunk=1024 * 64)


class _Counting:
    """A wrapper on the loaded library that counts calls per entry point."""

    def __init__(self, real):
        self._real, self.calls = real, {}

    def __getattr__(self, name):
        self.calls[name] = self.calls.get(name, 0) + 1
        return getattr(self._real, name)


@pytest.fixture
def counted():
    from swnerf import _lib
    real = _lib.lib()
    proxy = _Counting(real)
    _lib._lib = proxy
    try:
        yield proxy
    finally:
        _lib._lib = real


def _render_rays_ft(*a, **kw):
    """render_rays with the fused training pass switched on (render_rays itself keeps the reference's parameter list)"""
    from swnerf import render_tnerf
    with render_tnerf.fused_train():
        return render_tnerf.render_rays(*a, **kw)


def _grads(m):
    return {k: p.grad for k, p in m.named_parameters()}


# ---- 1. the TRAIN forward computes the inference pass's bits ------------------------------------------------------------------
_KEYS = ("rgb_map", "disp_map", "acc_map", "raw", "z_vals")


def _both(net, rb, S, **kw):
    from swnerf import render_tnerf
    q = _query()
    torch.manual_seed(11)
    with torch.no_grad():
        ref = render_tnerf.render_rays(rb, net, q, S, retraw=True, **kw)
    torch.manual_seed(11)
    out = _render_rays_ft(rb, net, q, S, retraw=True, **kw)
    assert out["rgb_map"].requires_grad and out["raw"].requires_grad
    for k in _KEYS:
        # bit for bit: torch.equal on the int32 views, so that a NaN disparity (acc == 0, kept as the reference keeps it,
        # ray.py:192) compares equal to the same NaN
        assert torch.equal(out[k].detach().contiguous().view(torch.int32), ref[k].contiguous().view(torch.int32)), (k, S, rb.shape[0], kw)


@pytest.mark.parametrize("n", [1, 3, 5, 257])
def test_forward_equals_inference_pass(net, n):
    rb = torch.from_numpy(C.rays(n=n, seed=20 + n)).to(DEV)
    for S in (2, 31, 32, 33, 64, 65):
        _both(net, rb, S, white_bkgd=True, perturb=1.)


@pytest.mark.parametrize("kw", [dict(white_bkgd=True, lindisp=True), dict(white_bkgd=False, raw_noise_std=1.), dict(white_bkgd=False, perturb=1.)],
                         ids=["lindisp", "zvals_noise", "black"])
def test_forward_equals_inference_pass_options(net, kw):
    n, S = 5, 33
    rb = torch.from_numpy(C.rays(n=n, seed=31)).to(DEV)
    if "raw_noise_std" in kw:
        kw = dict(kw, z_vals=torch.from_numpy(C.given_z(n=n, S=S)).to(DEV))
    _both(net, rb, S, **kw)


# ---- 2. gradients against float64 -----------------------------------------------------------------------------------------------
def test_gradients_case_a_vs_float64(sd32):
    """The op-path gradient test's input (tests/test_gpu_tnerf.py: n 48, S 32, seed 77, white background) through the fused pass;
    the loss uses rgb_map and acc_map, so both seeds of the compositing backward are live.  0 risky units (float64, CPU)."""
    from swnerf import render_tnerf
    m = _net()
    n, S = 48, 32
    rb = torch.from_numpy(C.rays(n=n, seed=77)).to(DEV)
    out = _render_rays_ft(rb, m, _query(), S, white_bkgd=True)
    tgt = torch.rand((n, 3), generator=torch.Generator().manual_seed(3))
    loss = ((out["rgb_map"] - tgt.to(DEV)) ** 2).mean() + 0.3 * out["acc_map"].mean()
    loss.backward()
    ray_loss = lambda ret, idx: ((ret["rgb_map"] - tgt[idx].double()) ** 2).sum() / (n * 3) + 0.3 * ret["acc_map"].sum() / n
    g = _grads(m)
    assert len(g) == 24 and all(v is not None for v in g.values())
    flips, risky = R.flip_aware_check(sd32, rb.cpu(), out["z_vals"].detach().cpu(), True, ray_loss, g, "tnerf fused (a)")
    print(f"(a): {flips} ReLU flips of {risky} risky units")


def test_gradients_case_b_ragged_tile(sd32):
    """n 5 (a workgroup with dead waves), S 40 (a ragged last tile); rays seed 81: 0 risky units (float64, CPU)."""
    from swnerf import render_tnerf
    m = _net()
    n, S = 5, 40
    rb = torch.from_numpy(C.rays(n=n, seed=81)).to(DEV)
    out = _render_rays_ft(rb, m, _query(), S, white_bkgd=True)
    tgt = torch.rand((n, 3), generator=torch.Generator().manual_seed(4))
    loss = ((out["rgb_map"] - tgt.to(DEV)) ** 2).mean() + 0.3 * out["acc_map"].mean()
    loss.backward()
    ray_loss = lambda ret, idx: ((ret["rgb_map"] - tgt[idx].double()) ** 2).sum() / (n * 3) + 0.3 * ret["acc_map"].sum() / n
    flips, risky = R.flip_aware_check(sd32, rb.cpu(), out["z_vals"].detach().cpu(), True, ray_loss, _grads(m), "tnerf fused (b)")
    print(f"(b): {flips} ReLU flips of {risky} risky units")


def test_gradients_case_c_noise_black(sd32):
    """n 7, S 65 (three tiles, the last with one sample), black background, sigma noise (seed 7); rays seed 91: 0 risky units
    (float64, CPU).  tnerf_ref's render takes no noise, so the check is tnerf_train_ref's (same method, same gate)."""
    from swnerf import render_tnerf
    m = _net()
    n, S = 7, 65
    rb = torch.from_numpy(C.rays(n=n, seed=91)).to(DEV)
    noise = torch.randn((n, S), generator=torch.Generator().manual_seed(7))
    out = render_tnerf.render_pass_train_tnerf(rb, m, S, noise=noise.to(DEV), white_bkgd=False)
    tgt = torch.rand((n, 3), generator=torch.Generator().manual_seed(5))
    loss = ((out["rgb_map"] - tgt.to(DEV)) ** 2).mean() + 0.3 * out["acc_map"].mean()
    loss.backward()
    ray_loss = lambda ret, idx: ((ret["rgb_map"] - tgt[idx].double()) ** 2).sum() / (n * 3) + 0.3 * ret["acc_map"].sum() / n
    flips, risky = TR.flip_aware_check(sd32, rb.cpu(), out["z"].detach().cpu(), False, ray_loss, _grads(m), "tnerf fused (c)", noise=noise)
    print(f"(c): {flips} ReLU flips of {risky} risky units")


# ---- 3. the disp_map and retraw seeds ---------------------------------------------------------------------------------------------
def test_gradients_disp_and_raw_seeds(sd32):
    """loss = mean(disp_map) + mean(raw * c): g_disp and g_raw are live, g_rgb and g_acc are NULL.  n 6, S 33; rays seed 61: 0
    risky units (float64, CPU)."""
    from swnerf import render_tnerf
    m = _net()
    n, S = 6, 33
    rb = torch.from_numpy(C.rays(n=n, seed=61)).to(DEV)
    c = torch.randn((n, S, 4), generator=torch.Generator().manual_seed(6))
    out = _render_rays_ft(rb, m, _query(), S, retraw=True, white_bkgd=True)
    loss = out["disp_map"].mean() + (out["raw"] * c.to(DEV)).mean()
    loss.backward()
    ray_loss = lambda ret, idx: ret["disp_map"].sum() / n + (ret["raw"] * c[idx].double()).sum() / (n * S * 4)
    flips, risky = TR.flip_aware_check(sd32, rb.cpu(), out["z_vals"].detach().cpu(), True, ray_loss, _grads(m), "tnerf fused disp/raw")
    print(f"disp/raw: {flips} ReLU flips of {risky} risky units")


# ---- 4. chunking ----------------------------------------------------------------------------------------------------------------
def test_gradients_accumulate_over_chunks():
    from swnerf import render_tnerf
    n, S = 96, 32
    rb = torch.from_numpy(C.rays(n=n, seed=55)).to(DEV)
    tgt = torch.rand((n, 3), generator=torch.Generator().manual_seed(8)).to(DEV)
    gs = []
    for chunk in (1024, 64):
        m = _net()
        out = render_tnerf.batchify_rays(rb, chunk, network_fn=m, network_query_fn=_query(), N_samples=S, white_bkgd=True, fused_train=True)
        (((out["rgb_map"] - tgt) ** 2).mean() + 0.3 * out["acc_map"].mean()).backward()
        gs.append(_grads(m))
    for k in gs[0]:
        dd, scale = float((gs[0][k] - gs[1][k]).abs().max()), float(gs[0][k].abs().max())
        assert dd <= 2e-5 * scale, (k, dd, scale)


# ---- 5. fall-backs ----------------------------------------------------------------------------------------------------------------
def test_fallbacks_to_the_op_path(net, counted):
    from swnerf import render_tnerf
    q = _query()
    rb = torch.from_numpy(C.rays(n=8, seed=41)).to(DEV)
    # S above the fused training pass's range
    a = _render_rays_ft(rb, net, q, 300, white_bkgd=True)
    b = render_tnerf.render_rays(rb, net, q, 300, white_bkgd=True)
    assert a["rgb_map"].requires_grad and torch.equal(a["rgb_map"], b["rgb_map"]) and torch.equal(a["acc_map"], b["acc_map"])
    # a closure without visible encoders
    plain = lambda inputs, viewdirs, ts, network_fn: q(inputs, viewdirs, ts, network_fn)
    a = render_tnerf.batchify_rays(rb, 1024, network_fn=net, network_query_fn=plain, N_samples=32, white_bkgd=True, fused_train=True)
    b = render_tnerf.render_rays(rb, net, plain, 32, white_bkgd=True)
    assert a["rgb_map"].requires_grad and torch.equal(a["rgb_map"], b["rgb_map"])
    assert not any(k in counted.calls for k in NEW_ENTRIES), counted.calls
    # the one-frame-time assertion of run_network
    rb2 = rb.clone()
    rb2[4:, 8] = 0.5
    with pytest.raises(AssertionError, match="same time"):
        _render_rays_ft(rb2, net, q, 32)


# ---- 6. the default is unchanged -----------------------------------------------------------------------------------------------
def test_default_keeps_the_op_path_under_grad(counted):
    from swnerf import render_tnerf
    m = _net()
    rb = torch.from_numpy(C.rays(n=8, seed=42)).to(DEV)
    out = render_tnerf.render_rays(rb, m, _query(), 32, retraw=True, white_bkgd=True)
    out["rgb_map"].sum().backward()
    assert not any(k in counted.calls for k in NEW_ENTRIES), counted.calls
    out = render_tnerf.batchify_rays(rb, 1024, network_fn=m, network_query_fn=_query(), N_samples=32, retraw=True, white_bkgd=True, fused_train=True)
    out["rgb_map"].sum().backward()
    assert all(counted.calls.get(k, 0) >= 1 for k in NEW_ENTRIES), counted.calls


# ---- 7. runner.train_tnerf ------------------------------------------------------------------------------------------------------
NEAR, FAR = 2.0, 6.0
TIMES = np.array([0.0, 0.5, 1.0], np.float32)


def _tn_args(tmp, **over):
    a = dict(expname="tloop", basedir=str(tmp), netdepth=8, lrate=5e-4, lrate_decay=500, netchunk=1024 * 64, no_reload=False, ft_path=None,
             N_samples=32, perturb=1., use_viewdirs=True, i_embed=0, multires=10, multires_views=4, raw_noise_std=0., dataset_type="blender",
             white_bkgd=True, no_ndc=False, lindisp=False, chunk=1024 * 32, N_rand=256, no_batching=True, precrop_iters=0, precrop_frac=.5,
             precrop_iters_time=0, nerf_type="original", do_half_precision=False, i_print=1000, i_weights=1000, i_testset=100000, N_iter=30, seed=0)
    a.update(over)
    return types.SimpleNamespace(**a)


def _tn_data(n_img=3, H=16, W=16, seed=2):
    from swnerf import synth
    rng = np.random.default_rng(seed)
    images = (0.3 + 0.1 * rng.uniform(0, 1, (n_img, H, W, 3))).astype(np.float32)
    poses = np.stack([synth.pose_spherical(30.0 + 40.0 * i, -30.0, 4.0) for i in range(n_img)]).astype(np.float32)
    focal = float(0.5 * W / np.tan(0.5 * synth.LEGO_CAMERA_ANGLE_X))
    return images, poses, poses[:1], [H, W, focal], [list(range(n_img)), [], []], TIMES, NEAR, FAR


@pytest.fixture(scope="module")
def tn_trained(tmp_path_factory):
    """30 fused steps at N_rand 256 on 3 images of 16 x 16 with times (a checkpoint at step 30), and the first 5 steps again with
    args.fused_train = False from the same seeds."""
    from swnerf import runner
    tmp = tmp_path_factory.mktemp("tn_train")
    data = _tn_data()
    final = {}

    def on_step(i, opt):
        if i == 30:
            final["params"] = [p.detach().clone() for p in opt.param_groups[0]["params"]]
    args = _tn_args(tmp / "fused", i_weights=30)
    torch.manual_seed(0)
    np.random.seed(0)
    rec = runner.train_tnerf(args, data, device=DEV, hooks={"on_step": on_step})
    torch.manual_seed(0)
    np.random.seed(0)
    rec_op = runner.train_tnerf(_tn_args(tmp / "op", N_iter=5, fused_train=False), data, device=DEV)
    return args, rec, rec_op, final["params"]


def test_train_tnerf_learns_and_records(tn_trained):
    from swnerf import batching
    args, rec, _, _ = tn_trained
    losses = [r["loss"] for r in rec]
    print("train_tnerf() losses", losses[0], "->", losses[-1])
    assert len(rec) == 30 and [r["step"] for r in rec] == list(range(1, 31))
    assert all(np.isfinite(losses)) and losses[-1] < 0.7 * losses[0], losses
    assert [r["lr"] for r in rec] == [batching.lr_at(args.lrate, args.lrate_decay, k) for k in range(30)]


def test_train_tnerf_checkpoint_reloads(tn_trained):
    from swnerf import runner
    args, _, _, params = tn_trained
    tr2, _, start2, _, _ = runner.create_tnerf(args, device=DEV)
    assert start2 == 29                                        # the global_step of iteration 30
    assert tr2.get("network_fine") is None
    for a, b in zip(params, tr2["network_fn"].parameters()):
        assert torch.equal(a, b)


def test_train_tnerf_fused_and_op_path_losses_agree(tn_trained):
    """The same seeds through loss.backward() on the fused kernels and on the op path: the first 5 losses.  Gate 1e-4 relative
    (the issue's guess; the measured differences are printed)."""
    _, rec, rec_op, _ = tn_trained
    rel = [abs(a["loss"] - b["loss"]) / abs(b["loss"]) for a, b in zip(rec[:5], rec_op)]
    print("fused vs op path, relative loss difference over 5 steps:", rel)
    assert len(rec_op) == 5 and max(rel) <= 1e-4, rel


def test_train_tnerf_numpy_sampler_first_batch_equals_a_hand_loop(tmp_path):
    """sampler="numpy": the first step's rays and targets are those of the reference's loop (run_tnerf.py:646-679) written by hand."""
    from swnerf import ray, render, runner
    H, W, N_rand = 16, 16, 64
    data = _tn_data()
    images, poses, _, hwf, i_split, times, near, far = data
    seen = {}
    args = _tn_args(tmp_path / "a", N_rand=N_rand, N_iter=1, precrop_iters=5, no_reload=True)
    np.random.seed(5)
    rec = runner.train_tnerf(args, data, device=DEV, sampler="numpy",
                             hooks={"on_batch": lambda i, img_i, rb, tg, ids: seen.update(i=i, img_i=img_i, rb=rb.clone(), tg=tg.clone())})
    assert len(rec) == 1 and rec[0]["step"] == 1
    np.random.seed(5)
    img_i = np.random.choice(i_split[0])
    target = torch.from_numpy(images[img_i]).to(DEV)
    rays_o, rays_d = ray.get_rays(H, W, hwf[2], torch.from_numpy(poses[img_i, :3, :4]).to(DEV))
    dH, dW = int(H // 2 * args.precrop_frac), int(W // 2 * args.precrop_frac)
    coords = torch.stack(torch.meshgrid(torch.linspace(H // 2 - dH, H // 2 + dH - 1, 2 * dH),
                                        torch.linspace(W // 2 - dW, W // 2 + dW - 1, 2 * dW), indexing="ij"), -1)
    coords = torch.reshape(coords, [-1, 2])
    select_inds = np.random.choice(coords.shape[0], size=[N_rand], replace=False)
    select_coords = coords[select_inds].long().to(DEV)
    o = rays_o[select_coords[:, 0], select_coords[:, 1]]
    d = rays_d[select_coords[:, 0], select_coords[:, 1]]
    target_s = target[select_coords[:, 0], select_coords[:, 1]]
    assert seen["i"] == 1 and seen["img_i"] == img_i
    assert seen["rb"].shape == (N_rand, 12) and bool((seen["rb"][:, 8] == float(times[img_i])).all())
    assert torch.equal(seen["rb"], render.pack_ray_batch(o, d, near, far, frame_time=float(times[img_i]), ndc=False))
    assert torch.equal(seen["tg"], target_s)


def test_train_tnerf_refuses_use_batching(tmp_path):
    from swnerf import runner
    with pytest.raises(NotImplementedError, match="frame time"):
        runner.train_tnerf(_tn_args(tmp_path, no_batching=False), _tn_data(), device=DEV)
