"""GPU tests of the fused multi-tensor Adam / AdamW step (csrc/optim_kernels.hip, swnerf/optim.py) and of args.optimizer = "fused"
in the runners.

  arithmetic     78 tensors (1, 3, 255, 256, 257, 4099 floats, 70 x 5 - three launches -, one 1 float into its storage: the scalar
                 path) in two param groups, gradients of magnitude 1e-8 .. 1e3 with exact zeros, after 1 and after 20 steps, against
                 a float64 evaluation of the formulas (tests/optim_ref.py).  Gate per array (p, exp_avg, exp_avg_sq, each over all
                 tensors): max(4 x d_ref, 4 fp32 ulps of the array's largest magnitude), d_ref = the distance of torch.optim.Adam /
                 AdamW (CPU, fp32, foreach=False, same inputs) from the same float64 evaluation, computed here.
  missing grads  every other tensor without a gradient on odd steps: bit-unchanged there, its step lags, the gate after 6 steps
  determinism    equal bits twice; grad_scale = 0.5 equals halved gradients bit for bit
  pack cache     after step() net.packed() is a new blob and the render is that of a twin with the same weights, bit for bit
  interchange    state_dict() passes between swnerf.optim and torch.optim in both directions, also through a checkpoint file
  runners        train / train_dnerf / create_fit2d with optimizer="fused"
Every test prints the figures it measured before it asserts."""
import copy
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import optim_ref as R
from swnerf import optim, synth

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NERF_BETAS = (0.9, 0.999)

# name: (class name, lr of group 0, lr of group 1, constructor arguments)
CASES = {
    "adam": ("Adam", 5e-4, 5e-4, dict(betas=NERF_BETAS, eps=1e-8, weight_decay=0)),
    "adam_l2": ("Adam", 5e-4, 5e-4, dict(betas=NERF_BETAS, eps=1e-8, weight_decay=0.01)),
    "adamw": ("AdamW", 5e-4, 5e-4, dict(betas=NERF_BETAS, eps=1e-8, weight_decay=0.01)),
    "adam_two_lr": ("Adam", 5e-4, 5e-3, dict(betas=NERF_BETAS, eps=1e-8, weight_decay=0)),
}
SNAPS = (1, 20)


def device_params(p0):
    """the tensors on the GPU; the last one is a view that starts 1 float into its storage (4 bytes off a 16-byte boundary)"""
    params = [torch.nn.Parameter(torch.from_numpy(a.copy()).to(DEV)) for a in p0[:-1]]
    buf = torch.zeros(p0[-1].size + 1, device=DEV)
    last = torch.nn.Parameter(buf[1:])
    with torch.no_grad():
        last.copy_(torch.from_numpy(p0[-1]))
    assert last.is_contiguous() and last.data_ptr() % 16 == 4 and all(p.data_ptr() % 16 == 0 for p in params)
    return params + [last]


def fused(case, params):
    cls, lr0, lr1, kw = CASES[case]
    return getattr(optim, cls)(R.groups(params, lr0, lr1), **kw)


_refs = {}


def reference(case, skip=None, steps=20, snaps=SNAPS):
    """(p0, grads, float64 snapshots, torch-CPU snapshots) of a case: computed once, shared, never modified"""
    key = (case, skip is not None, steps)
    if key not in _refs:
        cls, lr0, lr1, kw = CASES[case]
        p0, grads = R.make_params(), R.make_grads(steps, skip=skip)
        ref64 = R.run64(p0, grads, R.lrs_of(lr0, lr1), kw["betas"], kw["eps"], kw["weight_decay"], cls == "AdamW", snaps)
        cpu = R.torch_cpu(getattr(torch.optim, cls), p0, grads, lr0, lr1, snaps, **kw)
        _refs[key] = (p0, grads, ref64, cpu)
    return _refs[key]


def check_gate(what, got, ref64, cpu):
    ok = True
    for k, name in enumerate(("p", "exp_avg", "exp_avg_sq")):
        d_ref, d = R.dist(cpu[k], ref64[k]), R.dist(got[k], ref64[k])
        g = R.gate(ref64[k], d_ref)
        print(f"{what} {name}: |fused - f64| = {d:.3e}   |torch cpu - f64| = {d_ref:.3e}   gate = {g:.3e}   max|ref| = {np.abs(ref64[k]).max():.3e}")
        ok = ok and np.isfinite(got[k]).all() and d <= g
    assert got[3] == ref64[3] == cpu[3], "per-tensor step counts"
    assert ok, what


@pytest.mark.parametrize("case", list(CASES))
def test_arithmetic_against_float64(case):
    p0, grads, ref64, cpu = reference(case)
    params = device_params(p0)
    got = R.drive(fused(case, params), params, grads, SNAPS, device=DEV)
    for s in SNAPS:
        check_gate(f"{case} step {s}", got[s], ref64[s], cpu[s])
    # the group with another rate really moved at that rate: after step 1 every |dp| with g != 0 is ~ lr of its group
    if case == "adam_two_lr":
        dp = np.abs(got[1][0] - np.concatenate(p0))
        n0 = sum(R.SIZES[:R.GROUP0])
        g1 = np.concatenate(grads[0])
        big = np.abs(g1) > 1e-6                                                  # |g| >> eps: the first step is lr * sign(g)
        print("two rates: max |dp| group 0", dp[:n0][big[:n0]].max(), "group 1", dp[n0:][big[n0:]].max())
        assert np.allclose(dp[:n0][big[:n0]], 5e-4, rtol=0.02, atol=1e-7) and np.allclose(dp[n0:][big[n0:]], 5e-3, rtol=0.02, atol=1e-6)


def test_missing_gradients():
    skip = lambda s, i: s % 2 == 1 and i % 2 == 1                               # every other tensor, on odd steps
    p0, grads, ref64, cpu = reference("adam_l2", skip=skip, steps=6, snaps=(6,))
    params = device_params(p0)
    opt = fused("adam_l2", params)
    held = {}

    def on_step(s, when):
        if s % 2 == 0:
            return
        odd = [p for i, p in enumerate(params) if i % 2 == 1]
        now = [(p.detach().clone(), {k: v.clone() for k, v in opt.state.get(p, {}).items()}) for p in odd]
        if when == "before":
            held[s] = now
            return
        for (p_a, st_a), (p_b, st_b) in zip(held[s], now):
            assert torch.equal(p_a, p_b) and st_a.keys() == st_b.keys()
            assert all(torch.equal(st_a[k], st_b[k]) for k in st_a)             # p, m, v, step: bit-unchanged
    got = R.drive(opt, params, grads, (6,), device=DEV, on_step=on_step)
    T = got[6][3]
    print("step counts after 6 steps:", sorted(set(T)))
    assert all(t == (3 if i % 2 == 1 else 6) for i, t in enumerate(T))          # the skipped tensors lag
    for i, p in enumerate(params):
        st = opt.state[p]["step"]
        assert st.device.type == "cpu" and st.dtype == torch.float32 and st.dim() == 0
    check_gate("missing gradients, step 6", got[6], ref64[6], cpu[6])


def test_determinism_and_grad_scale():
    p0, grads, _, _ = reference("adamw")
    runs = []
    for _ in range(2):
        params = device_params(p0)
        runs.append(R.drive(fused("adamw", params), params, grads, (20,), device=DEV)[20])
    for a, b in zip(runs[0][:3], runs[1][:3]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # grad_scale = 0.5 against gradients halved on the host (an exact operation): one step, equal bits
    outs = []
    for scale, row in ((0.5, grads[0]), (1.0, [0.5 * g for g in grads[0]])):
        params = device_params(p0)
        opt = fused("adam_l2", params)
        for p, g in zip(params, row):
            p.grad = torch.from_numpy(g.astype(np.float32)).to(DEV)
        opt.step(grad_scale=scale)
        outs.append(R.snapshot(opt, params))
    for a, b in zip(outs[0][:3], outs[1][:3]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_refusals_on_the_gpu():
    w = torch.nn.Parameter(torch.zeros(4, 6, device=DEV))
    with pytest.raises(TypeError, match="float32"):
        optim.Adam([torch.nn.Parameter(torch.zeros(4, device=DEV, dtype=torch.float16))])
    with pytest.raises(ValueError, match="contiguous"):
        optim.Adam([torch.nn.Parameter(torch.zeros(6, 4, device=DEV).t())])
    opt = optim.Adam([w])
    w.grad = torch.zeros(4, 6, device=DEV).to_sparse()
    with pytest.raises(RuntimeError, match="sparse"):
        opt.step()
    w.grad = None
    opt.step()                                                                  # nothing has a gradient: nothing is launched
    assert len(opt.state) == 0
    opt.param_groups[0]["amsgrad"] = True                                       # as a loaded state_dict would set it
    w.grad = torch.ones(4, 6, device=DEV)
    with pytest.raises(NotImplementedError, match="amsgrad"):
        opt.step()
    assert set(optim.Adam([w]).param_groups[0]) == set(torch.optim.Adam([w]).param_groups[0])
    plain = lambda g: {k: v for k, v in g.items() if k != "params"}
    assert plain(optim.AdamW([w]).param_groups[0]) == plain(torch.optim.AdamW([w]).param_groups[0])
    assert plain(optim.Adam([w], lr=5e-4, weight_decay=0.01).param_groups[0]) == plain(torch.optim.Adam([w], lr=5e-4, weight_decay=0.01).param_groups[0])


# ---- the weight-pack cache ----------------------------------------------------------------------------------------------
def test_step_invalidates_the_pack_cache():
    from oracle import nerf_oracle as O
    from swnerf import model, render
    net = model.vallina_NeRF(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=5, skips=[4], use_viewdirs=True)
    seed, ab = synth.NET_FINE
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.nerf_state_dict(seed, alpha_bias=ab).items()})
    net = net.to(DEV).eval()
    K, c2w = synth.lego_camera(400, 400)
    o, d = synth.pick_rays(400, 400, K, c2w, 64, seed=9)
    rb = O.make_ray_batch(torch.from_numpy(o), torch.from_numpy(d), 2., 6.).to(DEV)
    shot = lambda n: render.render_pass(rb, n, 64, white_bkgd=True, want=["rgb_map"])["rgb_map"].clone()
    with torch.no_grad():
        before = shot(net)
    blob = net.packed()[1]
    assert net.packed()[1] is blob
    twin = copy.deepcopy(net)
    g = torch.Generator().manual_seed(3)
    for p in net.parameters():
        p.grad = torch.randn(p.shape, generator=g).to(DEV)
    optim.Adam(net.parameters(), lr=1e-2).step()
    new = net.packed()[1]
    assert new is not blob and net.packed()[1] is new
    twin.load_state_dict(net.state_dict())
    with torch.no_grad():
        after, want = shot(net), shot(twin)
    print("render moved by", float((after - before).abs().max()))
    assert not torch.equal(after, before) and bool(torch.isfinite(after).all())
    assert torch.equal(after, want) and torch.equal(new, twin.packed()[1])


# ---- state interchange ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("direction", ["fused_to_torch", "torch_to_fused"])
@pytest.mark.parametrize("case", ["adam_l2", "adamw"])
def test_state_dict_interchange(case, direction):
    cls, lr0, lr1, kw = CASES[case]
    p0, grads, _, _ = reference(case)
    make = {"fused": lambda ps: fused(case, ps), "torch": lambda ps: getattr(torch.optim, cls)(R.groups(ps, lr0, lr1), **kw)}
    src, dst = direction.split("_to_")
    pa = device_params(p0)
    a = make[src](pa)
    R.drive(a, pa, grads[:3], (), device=DEV)
    sd = a.state_dict()
    st0 = sd["state"][0]
    assert st0["step"].device.type == "cpu" and st0["step"].dtype == torch.float32 and float(st0["step"]) == 3.0
    assert st0["exp_avg"].is_cuda and st0["exp_avg"].dtype == torch.float32 and st0["exp_avg_sq"].is_cuda
    pb = device_params([p.detach().cpu().numpy().reshape(-1) for p in pa])
    b = make[dst](pb)
    b.load_state_dict(copy.deepcopy(sd))
    start = R.snapshot(a, pa)
    for x, y in zip(start[:3], R.snapshot(b, pb)[:3]):
        assert np.array_equal(x, y)
    assert R.snapshot(b, pb)[3] == start[3] == [3] * len(pa)
    # one more step on identical gradients: both within the gate of the float64 step from the common state
    ga = R.drive(a, pa, grads[3:4], (1,), device=DEV)[1]
    gb = R.drive(b, pb, grads[3:4], (1,), device=DEV)[1]
    state = tuple(R.split(x) for x in start[:3]) + (start[3],)
    ref64 = R.run64(None, grads[3:4], R.lrs_of(lr0, lr1), kw["betas"], kw["eps"], kw["weight_decay"], cls == "AdamW", (1,), state=state)[1]
    ours, theirs = (ga, gb) if src == "fused" else (gb, ga)
    check_gate(f"{case} {direction}: step 4", ours, ref64, theirs)


def test_checkpoint_written_with_fused_loads_into_torch(tmp_path):
    from swnerf import checkpoint, model
    torch.manual_seed(0)
    net = model.vallina_NeRF(D=2, W=32, input_ch=27, input_ch_views=15, output_ch=5, skips=[4], use_viewdirs=True).to(DEV)
    opt = optim.Adam(net.parameters(), lr=5e-4, betas=NERF_BETAS)
    for k in range(2):
        for p in net.parameters():
            p.grad = torch.randn_like(p)
        opt.step()
    path = checkpoint.save_checkpoint(str(tmp_path), "exp", 2, 2, net, None, opt)
    net2 = model.vallina_NeRF(D=2, W=32, input_ch=27, input_ch_views=15, output_ch=5, skips=[4], use_viewdirs=True).to(DEV)
    opt2 = torch.optim.Adam(net2.parameters(), lr=1e-3, betas=NERF_BETAS)
    start, used = checkpoint.reload_latest(str(tmp_path), "exp", net2, None, opt2, map_location=DEV)
    assert start == 2 and used == path and opt2.param_groups[0]["lr"] == 5e-4
    for p, q in zip(net.parameters(), net2.parameters()):
        assert torch.equal(p, q)
        for k in ("step", "exp_avg", "exp_avg_sq"):                            # (map_location moves `step` too: torch reads it from there)
            assert torch.equal(opt.state[p][k].cpu(), opt2.state[q][k].cpu()) and opt2.state[q][k].dtype == torch.float32, k
        assert opt2.state[q]["exp_avg"].device == q.device
    # and back into a fused one: a `step` that map_location put on the GPU returns to the host at the first step
    net3 = model.vallina_NeRF(D=2, W=32, input_ch=27, input_ch_views=15, output_ch=5, skips=[4], use_viewdirs=True).to(DEV)
    opt3 = optim.Adam(net3.parameters(), lr=1e-3, betas=NERF_BETAS)
    assert checkpoint.reload_latest(str(tmp_path), "exp", net3, None, opt3, map_location=DEV)[0] == 2
    for p, q in zip(net.parameters(), net2.parameters()):
        p.grad = torch.randn_like(p)
        q.grad = p.grad.clone()
    for p, r in zip(net.parameters(), net3.parameters()):
        r.grad = p.grad.clone()
    opt.step()
    opt2.step()                                                                 # torch's own step runs on the loaded groups and state
    opt3.step()
    for p, r in zip(net.parameters(), net3.parameters()):
        assert torch.equal(p, r) and opt3.state[r]["step"].device.type == "cpu" and float(opt3.state[r]["step"]) == 3.0
    worst = max(float((p - q).abs().max()) for p, q in zip(net.parameters(), net2.parameters()))
    print("one step after the reload: max |fused - torch| over the parameters", worst)
    assert worst <= 4 * 2.0 ** -23 * max(float(p.abs().max()) for p in net.parameters())


# ---- the runners ----------------------------------------------------------------------------------------------------------
def _nerf_args(tmp, **over):
    a = dict(expname="opt", basedir=str(tmp), netdepth=8, netwidth=256, netdepth_fine=8, netwidth_fine=256, lrate=5e-4, lrate_decay=500,
             netchunk=1024 * 64, no_reload=True, ft_path=None, N_samples=64, N_importance=128, perturb=1., use_viewdirs=True, i_embed=0,
             multires=10, multires_views=4, raw_noise_std=0., dataset_type="blender", white_bkgd=True, no_ndc=False, lindisp=False,
             chunk=1024 * 32, N_rand=256, no_batching=True, precrop_iters=0, precrop_frac=.5, i_print=1000, i_weights=10 ** 6,
             i_testset=10 ** 9, N_iters=20, seed=0)
    a.update(over)
    return SimpleNamespace(**a)


@pytest.fixture(scope="module")
def teacher_frames(tmp_path_factory):
    """3 frames of 16 x 16 of the seeded synthetic scene, as examples/train_lego_like.py renders them"""
    from swnerf import cameras, render, runner
    H = W = 16
    args = _nerf_args(tmp_path_factory.mktemp("teacher"))
    H, W, focal = cameras.blender_hwf(H, W, synth.LEGO_CAMERA_ANGLE_X)
    K = cameras.intrinsics(H, W, focal)
    _, kw, _, _, _ = runner.create_nerf(args, device=DEV)
    for net, (seed, ab) in ((kw['network_fn'], synth.NET_COARSE), (kw['network_fine'], synth.NET_FINE)):
        net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.nerf_state_dict(seed, alpha_bias=ab).items()})
    kw.update(near=2., far=6.)
    poses = np.stack([synth.pose_spherical(120.0 * i, -30.0, 4.0) for i in range(3)]).astype(np.float32)
    with torch.no_grad():
        images, _ = render.render_path(torch.from_numpy(poses).to(DEV), (H, W, focal), K, args.chunk, kw)
    return np.ascontiguousarray(images, dtype=np.float32), poses, [H, W, focal]


def test_train_with_the_fused_optimizer_tracks_torch(teacher_frames, tmp_path):
    """runner.train, 20 steps, the seeded device sampler.  The weight-gradient GEMMs add their row slices with float atomics, so two
    "torch" runs of one seed differ among themselves: d_torch = max over the steps of |loss_a - loss_b|.  The fused run must track
    the first torch run within max(d_torch, 20 steps x 4 fp32 ulps of the largest loss): the second term is the arithmetic gate's
    floor scaled by the step count, which the bit-equal case asks for, kept as a floor for every case - a bound that fell from 80 ulps
    at d_torch = 0 to 1 ulp at d_torch = 1 ulp would measure the luck of the atomics, not the optimizer."""
    from swnerf import runner
    images, poses, hwf = teacher_frames
    data = (images, poses, poses[:1], hwf, [[0, 1, 2], [], []], 2., 6.)
    recs, kinds = {}, {}
    for name, which in (("torch_a", "torch"), ("torch_b", "torch"), ("fused", "fused")):
        torch.manual_seed(0)
        np.random.seed(0)
        recs[name] = [r["loss"] for r in runner.train(_nerf_args(tmp_path / name, optimizer=which), data, device=DEV,
                                                      hooks={"on_step": lambda i, opt: kinds.__setitem__(name, type(opt))})]
    assert kinds["fused"] is optim.Adam and kinds["torch_a"] is torch.optim.Adam
    a, b, f = (np.array(recs[k], np.float64) for k in ("torch_a", "torch_b", "fused"))
    d_torch, d_fused = float(np.abs(a - b).max()), float(np.abs(f - a).max())
    floor = 20 * 4 * float(np.spacing(np.float32(max(a.max(), f.max()))))
    print(f"train(): step-1 loss fused {f[0]!r} torch {a[0]!r} {b[0]!r}; loss {f[0]:.6f} -> {f[-1]:.6f} (torch {a[0]:.6f} -> {a[-1]:.6f}); max |torch_a - torch_b| = {d_torch:.3e}, "
          f"max |fused - torch_a| = {d_fused:.3e}, floor = {floor:.3e}")
    assert len(f) == 20 and np.isfinite(f).all() and f[-1] < f[0]
    assert d_fused <= max(d_torch, floor)


def test_train_dnerf_with_the_fused_optimizer_skips_the_deformation_net_at_t0(teacher_frames, tmp_path):
    from swnerf import runner
    images, poses, hwf = teacher_frames
    times = np.array([0.0, 0.5, 1.0], np.float32)
    data = (images, poses, poses[:1], hwf, [[0, 1, 2], [], []], times, 2., 6.)
    a = vars(_nerf_args(tmp_path, N_rand=64, N_iter=6, optimizer="fused"))
    a.update(nerf_type="direct_temporal", not_zero_canonical=False, use_two_models_for_fine=False, do_half_precision=False,
             add_tv_loss=False, tv_loss_weight=0., precrop_iters_time=0)
    drawn, seen = [], {}

    def on_step(i, opt):
        seen["opt"] = opt
    torch.manual_seed(0)
    np.random.seed(3)
    rec = runner.train_dnerf(SimpleNamespace(**a), data, device=DEV,
                             hooks={"on_batch": lambda i, img_i, rb, tg, ids: drawn.append(int(img_i)), "on_step": on_step})
    n_t0 = sum(1 for k in drawn if times[k] == 0.0)
    print("train_dnerf(): frames drawn", drawn, "losses", [r["loss"] for r in rec])
    assert len(rec) == 6 and all(np.isfinite(r["loss"]) for r in rec)
    assert 0 < n_t0 < 6, "the seed must draw the t == 0 frame at least once and another one at least once"
    opt = seen["opt"]
    assert type(opt) is optim.Adam
    net = opt.param_groups[0]["params"]
    # train_dnerf does not hand the module out: a twin built from the same options names the parameters, in the same order
    twin_kw, _, _, twin_vars, _ = runner.create_dnerf(SimpleNamespace(**a), device=DEV)
    names = [n for n, _ in twin_kw["network_fn"].named_parameters()]
    assert [tuple(p.shape) for p in twin_vars] == [tuple(p.shape) for p in net] and len(names) == len(net)
    steps = {n: int(opt.state[p]["step"]) if opt.state.get(p) else 0 for n, p in zip(names, net)}
    time_steps = {v for n, v in steps.items() if n.startswith("_time")}
    other_steps = {v for n, v in steps.items() if not n.startswith("_time")}
    print("step counters: _time.*", time_steps, "others", other_steps)
    assert any(n.startswith("_time") for n in names)
    assert time_steps == {6 - n_t0} and other_steps == {6}


def test_fit2d_epoch_with_the_fused_optimizer(tmp_path):
    from swnerf import fit2d, runner
    args = SimpleNamespace(L=4, layer_num=2, regularization=0.1, picture_dir="pics/blob.jpg", checkpoint_save=None, checkpoint_load=None,
                           output_dir=None, epochs=1, v=False, optimizer="fused")
    torch.manual_seed(0)
    model, opt, sched, start, _ = runner.create_fit2d(args, device=DEV)
    assert type(opt) is optim.AdamW and opt.param_groups[0]["weight_decay"] == 0.01 and opt.param_groups[0]["decoupled_weight_decay"] is True
    H, W = 24, 32                                                               # 768 rows
    ys, xs = np.mgrid[0:H, 0:W]
    rgb = np.stack([xs * 255 // (W - 1), ys * 255 // (H - 1), (xs + ys) * 255 // (H + W - 2)], -1).astype(np.uint8)
    pos, color, w, h = fit2d.picture_tensors(rgb)
    m = fit2d.train((pos, color), model, opt, sched, args, w, h)
    print("fit2d: MSE of the epoch", m["MSE"], "lr", opt.param_groups[0]["lr"])
    assert len(m["MSE"]) == 1 and np.isfinite(m["MSE"][0]) and all(bool(torch.isfinite(p).all()) for p in model.parameters())
    assert opt.param_groups[0]["lr"] == pytest.approx(0.001 * 0.95)             # the scheduler drives the fused optimizer's group
    assert {int(opt.state[p]["step"]) for p in model.parameters()} == {2}       # one epoch: a batch of 512 and one of 256
