"""MultiRes D-NeRF on the GPU: the pyramid kernels (csrc/pyramid_kernels.hip) through swnerf.pyramid against the golden
G15 (the reference's multires_dnerf/pyramid.py on CPU) and the float64 restatement tests/pyramid_ref.py, and the level
runner of swnerf.runner (create_multires, multires_train_loss, render_path_multires).

Gate of every pyramid array: max(4 x ref_dist, 4 fp32 ulps at 1.0 = 4.8e-7) absolute, where ref_dist is the max abs
distance of the REFERENCE formulation from the restatement: stored in the fixture for its cases, and for every other
shape computed here from torch CPU fp32 F.conv2d / F.interpolate (and their autograd) - never from the code under test.
The 4x lets the kernels round differently from torch by no more than torch itself differs from exact arithmetic.
Each test prints its measured distances next to the gates (pytest -s); DESIGN.md 6g records them.

The level nets are compared with the same net evaluated in float64 from its state_dict AT the kernels' own sample depths
and position deltas: the depths come out of a discontinuous inverse CDF, and level 0 re-embeds x + dx in 20 bands
(2^19 x), so the float64 net is given float32(x + dx) as the kernels formed it and dx itself is checked on its own
(tests/test_gpu_generic.py does the same at 10 bands)."""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pyramid_ref as R
from make_golden_pyramid import CASES, LEVELS
from oracle import nerf_oracle as O
from swnerf import pyramid, render_dnerf, runner
from swnerf.render import pack_ray_batch

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g15_pyramid.npz")
FLOOR = 4 * 2.0 ** -23                  # 4 fp32 ulps at 1.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def g15():
    return dict(np.load(GOLDEN, allow_pickle=False))


def gate(ref_dist):
    return max(4.0 * float(ref_dist), FLOOR)


def check(got, want, ref_dist, what):
    got = got.detach().cpu().numpy().astype(np.float64) if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    d = float(np.abs(got - want).max()) if got.size else 0.0
    print(f"{what}: dist {d:.3e} gate {gate(ref_dist):.3e} (ref_dist {float(ref_dist):.3e})")
    assert d <= gate(ref_dist), (what, d, gate(ref_dist))
    return d


# ---- the reference formulation on torch CPU fp32 (for ref_dist of shapes outside the fixture) ---------------------------
def torch_generate(x, levels, k, sigma):
    """pyramid.py:46-80 with levels - 1 downsamples; x: CPU tensor NHWC (fp32 or fp64)"""
    c = x.shape[3]
    kern = pyramid.create_gaussian_kernel(k, sigma, c).to(x.dtype)
    g = [x.permute(0, 3, 1, 2)]
    for _ in range(levels - 1):
        b = F.conv2d(g[-1], kern, padding=k // 2, groups=c)
        g.append(F.interpolate(b, scale_factor=0.5, mode="bilinear", align_corners=False))
    lap = [g[i] - F.interpolate(g[i + 1], size=g[i].shape[2:], mode="bilinear", align_corners=False) for i in range(levels - 1)]
    return [l.permute(0, 2, 3, 1) for l in lap + [g[-1]]]


def torch_reconstruct(levels):
    lv = [l.permute(0, 3, 1, 2) for l in levels]
    r = lv[-1]
    for i in range(len(lv) - 2, -1, -1):
        r = F.interpolate(r, size=lv[i].shape[2:], mode="bilinear", align_corners=False) + lv[i]
    return r.permute(0, 2, 3, 1)


def dist(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


# ---- golden ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_generate_and_reconstruct_golden(dev, g15, name):
    """Measured on MI355X: worst level distance from the restatement 3.98e-7 (c, level 0; gate 1.49e-6), from
    the golden 2.38e-7; reconstruct 4.03e-7 (c; gate 1.61e-6)."""
    _, shape, k, sigma = CASES[name]
    x = g15[f"{name}_input"]
    rd = g15[f"{name}_ref_dist"]
    pyr = pyramid.generate_laplacian_pyramid_batch(torch.from_numpy(x).to(dev), levels=LEVELS, kernel_size=k, sigma=sigma)
    want = R.generate(x, LEVELS, k, sigma)
    assert len(pyr) == LEVELS
    for l in range(LEVELS):
        check(pyr[l], g15[f"{name}_level{l}"].astype(np.float64), rd[l], f"{name} level {l} vs golden")
        check(pyr[l], want[l], rd[l], f"{name} level {l} vs restatement")
    gold_levels = [g15[f"{name}_level{l}"] for l in range(LEVELS)]
    rec = pyramid.reconstruct_image_from_pyramid_batch([torch.from_numpy(a).to(dev) for a in gold_levels])
    check(rec, g15[f"{name}_recon"].astype(np.float64), rd[LEVELS], f"{name} reconstruct vs golden")
    check(rec, R.reconstruct(gold_levels), rd[LEVELS], f"{name} reconstruct vs restatement")
    # host input, chunked: the same bits
    pyr2 = pyramid.generate_laplacian_pyramid_batch(x, levels=LEVELS, kernel_size=k, sigma=sigma, chunk_frames=1)
    for a, b in zip(pyr, pyr2):
        assert torch.equal(a, b)


# ---- beyond the fixture ------------------------------------------------------------------------------------------------------
BEYOND = [((1, 8, 8, 3), 4), ((3, 100, 101, 3), 4), ((1, 64, 257, 1), 4), ((1, 33, 64, 4), 4), ((2, 21, 18, 3), 1), ((2, 21, 18, 3), 2)]


@pytest.mark.parametrize("shape,levels", BEYOND)
def test_generate_and_reconstruct_beyond_fixture(dev, shape, levels):
    x = np.random.Generator(np.random.PCG64(hash((shape, levels)) % 2 ** 31)).random(shape, dtype=np.float32)
    want = R.generate(x, levels)
    ref = [t.numpy() for t in torch_generate(torch.from_numpy(x), levels, 3, 1.0)]
    pyr = pyramid.generate_laplacian_pyramid_batch(torch.from_numpy(x).to(dev), levels=levels)
    assert len(pyr) == levels
    for l in range(levels):
        check(pyr[l], want[l], dist(ref[l], want[l]), f"{shape} L={levels} level {l}")
    if levels == 1:
        assert torch.equal(pyr[0].cpu(), torch.from_numpy(x))
    rec_ref = torch_reconstruct([torch.from_numpy(a) for a in ref]).numpy()
    rec = pyramid.reconstruct_image_from_pyramid_batch([torch.from_numpy(a).to(dev) for a in ref])
    check(rec, R.reconstruct(ref), dist(rec_ref, R.reconstruct(ref)), f"{shape} L={levels} reconstruct")
    # round trip: reconstruct(generate(x)) == x (the reference itself: 6e-8)
    check(pyramid.reconstruct_image_from_pyramid_batch(pyr), x.astype(np.float64), dist(rec_ref, x), f"{shape} L={levels} round trip")


# the remaining arms of the kernels' dispatch: kernel sizes 1 and 7 and two channels (ragged odd sizes, two frames)
OTHER_ARMS = [((2, 19, 23, 2), 3, 1.0), ((2, 19, 23, 3), 7, 2.0), ((1, 13, 18, 2), 7, 2.0), ((2, 19, 23, 3), 1, 1.0)]


@pytest.mark.parametrize("shape,k,sigma", OTHER_ARMS)
def test_generate_other_kernel_sizes_and_two_channels(dev, shape, k, sigma):
    levels = 3
    x = np.random.Generator(np.random.PCG64(1000 * k + shape[3])).random(shape, dtype=np.float32)
    want = R.generate(x, levels, k, sigma)
    ref = [t.numpy() for t in torch_generate(torch.from_numpy(x), levels, k, sigma)]
    pyr = pyramid.generate_laplacian_pyramid_batch(torch.from_numpy(x).to(dev), levels=levels, kernel_size=k, sigma=sigma)
    for l in range(levels):
        check(pyr[l], want[l], dist(ref[l], want[l]), f"{shape} k={k} level {l}")
    rec_ref = torch_reconstruct([torch.from_numpy(a) for a in ref]).numpy()
    rec = pyramid.reconstruct_image_from_pyramid_batch([torch.from_numpy(a).to(dev).requires_grad_(True) for a in ref])
    check(rec, R.reconstruct(ref), dist(rec_ref, R.reconstruct(ref)), f"{shape} k={k} reconstruct")


def test_round_trip_golden_cases(dev, g15):
    for name in sorted(CASES):
        _, _, k, sigma = CASES[name]
        x = g15[f"{name}_input"]
        pyr = pyramid.generate_laplacian_pyramid_batch(torch.from_numpy(x).to(dev), levels=LEVELS, kernel_size=k, sigma=sigma)
        check(pyramid.reconstruct_image_from_pyramid_batch(pyr), x.astype(np.float64), g15[f"{name}_roundtrip_dist"], f"{name} round trip")


def test_equal_size_reconstruct_is_the_exact_sum(dev):
    g = torch.Generator().manual_seed(5)
    lv = [(torch.rand((2, 19, 23, 3), generator=g) - 0.5).to(dev) for _ in range(4)]
    want = ((lv[3] + lv[2]) + lv[1]) + lv[0]                             # r = up(r) + lap[i], coarsest first
    assert torch.equal(pyramid.reconstruct_image_from_pyramid_batch(lv), want)
    assert torch.equal(pyramid.reconstruct_image_from_pyramid_batch(torch.stack(lv, 0)), want)
    # a view that is not 16-byte aligned takes the scalar path: the same bits
    flat = torch.zeros(4 * 2 * 19 * 23 * 3 + 1, device=dev)
    off = flat[1:].view(4, 2, 19, 23, 3)
    off.copy_(torch.stack(lv, 0))
    assert torch.equal(pyramid.reconstruct_image_from_pyramid_batch(list(off.unbind(0))), want)
    # up_axpy without a base, and with alpha = -1
    assert torch.equal(pyramid.up_axpy(lv[0], (19, 23)), lv[0])
    assert torch.equal(pyramid.up_axpy(lv[0], (19, 23), base=lv[1], alpha=-1.0), lv[1] - lv[0])


# ---- backward --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [[(32, 32), (16, 16), (8, 8), (4, 4)], [(37, 53), (18, 26), (9, 13), (4, 6)]])
def test_reconstruct_backward(dev, sizes):
    g = torch.Generator().manual_seed(11)
    n = 2
    lv_host = [torch.rand((n, h, w, 3), generator=g) for h, w in sizes]
    wgt = torch.rand((n, sizes[0][0], sizes[0][1], 3), generator=g)
    want = R.reconstruct_adjoint(wgt.numpy(), sizes)
    # ref_dist: torch CPU fp32 autograd against the restatement
    cpu = [l.clone().requires_grad_(True) for l in lv_host]
    (torch_reconstruct(cpu) * wgt).sum().backward()
    rd = [dist(c.grad.numpy(), w_) for c, w_ in zip(cpu, want)]

    def run():
        lv = [l.to(dev).requires_grad_(True) for l in lv_host]
        (pyramid.reconstruct_image_from_pyramid_batch(lv) * wgt.to(dev)).sum().backward()
        return [l.grad for l in lv]

    got = run()
    # second witness: torch float64 F.interpolate autograd on the device
    d64 = [l.to(dev).double().requires_grad_(True) for l in lv_host]
    (torch_reconstruct(d64) * wgt.to(dev).double()).sum().backward()
    for l in range(len(sizes)):
        check(got[l], want[l], rd[l], f"{sizes[0]} grad level {l} vs restatement")
        check(got[l], d64[l].grad.cpu().numpy(), rd[l], f"{sizes[0]} grad level {l} vs torch float64 autograd")
    for a, b in zip(got, run()):
        assert torch.equal(a, b)                                         # a gather in a fixed order: bit-identical runs
    # only some levels need a gradient
    lv = [l.to(dev) for l in lv_host]
    lv[2].requires_grad_(True)
    (pyramid.reconstruct_image_from_pyramid_batch(lv) * wgt.to(dev)).sum().backward()
    assert torch.equal(lv[2].grad, got[2]) and lv[0].grad is None
    with torch.no_grad():
        assert not pyramid.reconstruct_image_from_pyramid_batch(lv).requires_grad


# ---- the level runner ------------------------------------------------------------------------------------------------------
def _args(**over):
    a = dict(layer_num=4, use_viewdirs=True, N_importance=8, N_samples=8, nerf_type="direct_temporal", netdepth=8, netwidth=64,
             netdepth_fine=8, netwidth_fine=64, use_two_models_for_fine=False, not_zero_canonical=False, netchunk=1 << 16,
             lrate=5e-4, basedir="/nonexistent", expname="none", ft_path=None, no_reload=True, perturb=0.0, white_bkgd=True,
             raw_noise_std=0.0, dataset_type="blender", no_ndc=False, lindisp=False, do_half_precision=False,
             chunk=1 << 15, global_optimization_epoch=10, reproducible_wgrad=True)
    a.update(over)
    return types.SimpleNamespace(**a)


@pytest.fixture(scope="module")
def levels4(dev):
    torch.manual_seed(1234)
    out = runner.create_multires(_args(), device=dev)
    for kw in out[0] + out[1]:
        kw.update({"near": 2.0, "far": 6.0})
    return out


def _pose(dev):
    from swnerf import synth
    return torch.from_numpy(synth.pose_spherical(30.0, -30.0, 4.0)).to(dev)


@pytest.mark.parametrize("layer", [0, 1, 2, 3])
@pytest.mark.parametrize("t", [0.0, 0.5])
def test_level_shapes_render_and_backward(dev, levels4, layer, t):
    """16 rays x (8 + 8) samples through each level's nets (position / time / view bands (20, 8, 20), (10, 4, 10),
    (10, 4, 10) and the identity encoders), forward against float64 and a backward that reaches every parameter."""
    from swnerf import synth
    from swnerf.runner import MULTIRES_CHANNELS
    kw = levels4[0][layer]
    net = kw["network_fn"]
    Lp, Lt, Lv = MULTIRES_CHANNELS[layer]
    K, c2w = synth.lego_camera(64, 64)
    o, d = synth.pick_rays(64, 64, K, c2w, 16, seed=21 + layer)
    o, d = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    net.zero_grad()
    rgb, disp, acc, extras = render_dnerf.render(4, 4, float(K[0][0]), chunk=1 << 15, rays=(o, d), frame_time=t, retraw=True, **kw)
    assert rgb.shape == (16, 3) and bool(torch.isfinite(rgb).all())
    (rgb.sum() + 0.1 * acc.sum()).backward()
    for name, p in net.named_parameters():
        if t == 0.0 and name.startswith("_time"):
            continue                                                     # zero_canonical: the deformation net is not evaluated at t = 0
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    assert any(float(p.grad.abs().max()) > 0 for n_, p in net.named_parameters() if n_.startswith("_occ"))
    # float64, on the CPU, at the kernels' depths and position deltas
    sd = {k_: v.detach().cpu().double() for k_, v in net.state_dict().items()}
    z = extras["z_vals"].detach().cpu()
    dx_gpu = extras["position_delta"].detach().cpu()
    oc, dc = o.cpu(), d.cpu()
    pts = (oc[:, None, :] + dc[:, None, :] * z[:, :, None]).reshape(-1, 3)                   # fp32, as the op path forms them
    # the unit view directions as the ray-batch kernel forms them (level 0 encodes them in 20 bands)
    rb = pack_ray_batch(o, d, 2.0, 6.0, frame_time=t, ndc=False, H=4, W=4, focal=float(K[0][0]))
    assert torch.equal(rb[:, :6].cpu(), torch.cat([oc, dc], -1))
    views = rb[:, -3:].cpu()[:, None, :].expand(16, z.shape[1], 3).reshape(-1, 3)
    emb = lambda x, L: O.embed(x.double(), L)
    ch = lambda L: 3 * (1 + 2 * L) if L >= 0 else 3
    x64 = torch.cat([emb(pts, Lp), emb(views, Lv)], -1)
    t_emb = emb(torch.full((pts.shape[0], 1), t), Lt)
    raw64, dx64 = O.generic_dnerf_mlp(sd, x64, t_emb, 8, [4], ch(Lp), ch(Lv), True, multires=Lp)
    ddx = dist(dx_gpu.reshape(-1, 3), dx64)
    print(f"level {layer} t={t}: |dx - dx64| {ddx:.3e}, |dx| max {float(dx64.abs().max()):.3e}")
    assert ddx <= 2e-6
    if t != 0.0:                                                         # the canonical net at float32(x + dx) of the kernels' dx
        xs = emb(pts + dx_gpu.reshape(-1, 3), Lp)
        raw64 = O.generic_mlp(sd, torch.cat([xs, emb(views, Lv)], -1), 8, [4], ch(Lp), ch(Lv), True, prefix="_occ.")
    rgb64, _, acc64, _, _ = O.raw2outputs(raw64.reshape(16, z.shape[1], 4), z.double(), dc.double(), white_bkgd=True)
    drgb = dist(rgb.detach().cpu(), rgb64)
    print(f"level {layer} t={t}: |rgb - rgb64| {drgb:.3e} (gate 2e-5), |acc - acc64| {dist(acc.detach().cpu(), acc64):.3e}")
    assert drgb <= 2e-5


def _scene(dev, n=3, side=64):
    """a smooth seeded synthetic image set with poses and times"""
    from swnerf import synth
    rng = np.random.Generator(np.random.PCG64(77))
    yy, xx = np.meshgrid(np.linspace(0, 1, side), np.linspace(0, 1, side), indexing="ij")
    imgs = np.stack([np.stack([0.5 + 0.4 * np.sin(6 * xx + i + c) * np.cos(5 * yy - c) for c in range(3)], -1) for i in range(n)])
    imgs = np.clip(imgs + 0.02 * rng.standard_normal(imgs.shape), 0, 1).astype(np.float32)
    poses = np.stack([synth.pose_spherical(30.0 + 40 * i, -30.0, 4.0) for i in range(n)]).astype(np.float32)
    times = np.linspace(0.0, 1.0, n).astype(np.float32)
    return torch.from_numpy(imgs).to(dev), torch.from_numpy(poses).to(dev), torch.from_numpy(times).to(dev)


@pytest.fixture(scope="module")
def joint(dev, levels4):
    """the joint iteration on 64 x 64 synthetic images, patches 32 / 16 / 8 / 4, at i on both sides of the epoch"""
    trains = levels4[0]
    args = _args()
    images, poses, times = _scene(dev)
    focal = 0.5 * 64 / np.tan(0.5 * 0.6911112070083618)
    pyr_hwf = runner.pyramid_hwf([64, 64, focal], 4)
    pyr_images = pyramid.generate_laplacian_pyramid_batch(images, levels=4)
    patch = [32, 16, 8, 4]
    coords = [(16, 8), (8, 4), (4, 2), (2, 1)]
    nets = [kw["network_fn"] for kw in trains]
    call = lambda i, **kw: runner.multires_train_loss(i, 1, images, pyr_images, poses, times, pyr_hwf, patch, trains, args, **kw)

    def grads(i, only_levels=False):
        for net in nets:
            net.zero_grad()
        loss, per_level, gl, gpsnr, rec = call(i, patch_coords=coords)
        assert bool(torch.isfinite(loss)) and len(per_level) == 4 and rec.shape == (32, 32, 3)
        assert bool(torch.isfinite(gl)) and bool(torch.isfinite(gpsnr))
        (sum(per_level) if only_levels else loss).backward()
        return (loss.detach(), [p.detach() for p in per_level], gl.detach(),
                [[None if p.grad is None else p.grad.clone() for p in net.parameters()] for net in nets])

    return types.SimpleNamespace(nets=nets, call=call, coords=coords, hi=grads(10), lo=grads(9), only=grads(9, only_levels=True),
                                 only_again=grads(9, only_levels=True))


def test_joint_step(dev, joint):
    loss_hi, per_hi, gl_hi, g_hi = joint.hi                              # i >= global_optimization_epoch
    assert abs(float(loss_hi) - (sum(float(p) for p in per_hi) + float(gl_hi))) <= 1e-6 * max(1.0, float(loss_hi))
    for l, gs in enumerate(g_hi):
        for (name, _), gr in zip(joint.nets[l].named_parameters(), gs):
            assert gr is not None and bool(torch.isfinite(gr).all()), (l, name)
    loss_lo, per_lo, gl_lo, g_lo = joint.lo                              # below it: the per-level losses alone
    assert torch.equal(gl_lo, gl_hi) and all(torch.equal(a, b) for a, b in zip(per_lo, per_hi))
    assert float(loss_lo) == sum(float(p) for p in per_lo) or abs(float(loss_lo) - sum(float(p) for p in per_lo)) <= 1e-7
    # below the epoch the loss does not reach the reconstruction at all; from it on, it does
    for i, reaches in ((9, False), (10, True)):
        loss, _, _, _, rec = joint.call(i, patch_coords=joint.coords)
        (g,) = torch.autograd.grad(loss, rec, allow_unused=True)
        assert (g is not None) == reaches
    # ... and the global loss does change the gradients of every level
    for l in range(4):
        assert any(not torch.equal(a, b) for a, b in zip(g_lo[l], g_hi[l])), l
    # a drawn patch stays usable: coordinates from initialize_patches
    loss, *_ = joint.call(0)
    assert bool(torch.isfinite(loss))


def test_joint_step_gradients_below_epoch_bit_for_bit(dev, joint):
    """With i below global_optimization_epoch the parameter gradients equal those of the per-level losses alone, bit for bit.
    The two backward passes are the same launches on the same upstream gradients (test_joint_step shows that the loss does
    not reach the reconstruction), so this holds as far as one backward pass repeats itself.  The level nets are created
    with `reproducible_wgrad`: their weight gradients add the row slices in a fixed order (swnerf_gemm_tn_ordered) instead of
    with float atomics (swnerf_gemm_tn), under which two IDENTICAL passes were apart by 6.1e-5 on level 0 (16384 rows, max
    |grad| 785), 3.7e-8 on level 1, 1.2e-7 on level 2 and 0 on level 3 (one row slice).  The test prints both distances per
    level.  Measured on MI355X with the ordered sum: identical passes and the
    below-epoch pass against the per-level losses apart by 0 on all four levels (max |grad| 785, 0.43, 2.7, 0.038)."""
    for l, net in enumerate(joint.nets):
        rep = max(float((a - b).abs().max()) for a, b in zip(joint.only[3][l], joint.only_again[3][l]))
        low = max(float((a - b).abs().max()) for a, b in zip(joint.only[3][l], joint.lo[3][l]))
        mag = max(float(a.abs().max()) for a in joint.only[3][l])
        print(f"level {l}: max |grad| {mag:.3e}; identical passes apart by {rep:.3e}; below-epoch loss vs per-level losses apart by {low:.3e}")
    for l, net in enumerate(joint.nets):
        for (name, _), a, b in zip(net.named_parameters(), joint.lo[3][l], joint.only[3][l]):
            assert torch.equal(a, b), (l, name)


def test_render_path_multires(dev, levels4, tmp_path):
    tests = levels4[1]
    focal = 0.5 * 32 / np.tan(0.5 * 0.6911112070083618)
    poses = _pose(dev)[None]
    times = torch.tensor([0.5], device=dev)
    frames, per = runner.render_path_multires(poses, times, [32, 32, focal], 1 << 15, tests, level_hwf="reference")
    assert frames.shape == (1, 32, 32, 3) and [p.shape for p in per] == [(1, 32, 32, 3)] * 4
    assert np.array_equal(frames, ((per[3] + per[2]) + per[1]) + per[0])
    frames, per = runner.render_path_multires(poses, times, [32, 32, focal], 1 << 15, tests, level_hwf="pyramid", savedir=str(tmp_path))
    assert [p.shape for p in per] == [(1, 32, 32, 3), (1, 16, 16, 3), (1, 8, 8, 3), (1, 4, 4, 3)]
    want = pyramid.reconstruct_image_from_pyramid_batch([torch.from_numpy(p).to(dev) for p in per]).cpu().numpy()
    assert np.array_equal(frames, want)
    exact = R.reconstruct(per)
    check(torch.from_numpy(frames), exact, dist(torch_reconstruct([torch.from_numpy(p) for p in per]).numpy(), exact),
          "pyramid-mode frame vs restatement of its levels")
    assert os.path.exists(tmp_path / "estim" / "000.png") and os.path.exists(tmp_path / "layer_3" / "estim" / "000.png")
    with pytest.raises(ValueError):
        runner.render_path_multires(poses, times, [32, 32, focal], 1 << 15, tests, level_hwf="half")
