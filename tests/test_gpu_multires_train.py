"""GPU tests of the MultiRes training data path (csrc/patch_kernels.hip, swnerf.batching.PatchBatcher / multires_loss) and of
runner.train_multires.

  rows, targets   bit-equal to get_rays(H_l, W_l, focal_l, pose)[y:y+ph, x:x+pw] -> pack_ray_batch and to the slices of the pyramid
  reconstruction  bit-equal to pyramid.reconstruct_image_from_pyramid_batch on the same level patches
  loss, gradients against the float64 restatement tests/multires_loss_ref.py.  The tolerance is not fixed in advance: the op-by-op
                  path (the arithmetic of runner.multires_train_loss without a batcher: F.mse_loss per level, reconstruct_and_compute_loss,
                  autograd) is measured against the same float64 values on the same inputs, and the fused launch must stay within
                  2 x that error - for the loss scalars as a group and for the gradient elements as a group
  batcher switch  runner.multires_train_loss with and without a PatchBatcher on the same nets
  train_multires  both phases on a 6-frame synthetic set: checkpoints, log, moved parameters, options, equal bits on a second run
Every test prints the figures it measured before it asserts (pytest -s); DESIGN.md 6g records them."""
import os
import random
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import multires_loss_ref as M
from swnerf import batching, checkpoint, pyramid, runner, synth
from swnerf.ray import get_rays
from swnerf.render import pack_ray_batch

pytestmark = pytest.mark.gpu
NEAR, FAR = 2.0, 6.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def scene(n, H, W, seed=77):
    """a smooth seeded image set with poses and times (numpy)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    imgs = np.stack([np.stack([0.5 + 0.4 * np.sin(6 * xx + i + c) * np.cos(5 * yy - c) for c in range(3)], -1) for i in range(n)])
    imgs = np.clip(imgs + 0.02 * rng.standard_normal(imgs.shape), 0, 1).astype(np.float32)
    poses = np.stack([synth.pose_spherical(30.0 + 40 * i, -30.0 + 7 * i, 4.0) for i in range(n)]).astype(np.float32)
    times = np.linspace(0.0, 1.0, n).astype(np.float32)
    return imgs, poses, times


def focal_of(W):
    return float(0.5 * W / np.tan(0.5 * synth.LEGO_CAMERA_ANGLE_X))


def make_batcher(dev, H, W, levels, n=3):
    imgs, poses, times = scene(n, H, W)
    images = torch.from_numpy(imgs).to(dev)
    pyr_hwf = runner.pyramid_hwf([H, W, focal_of(W)], levels)
    pyr_images = pyramid.generate_laplacian_pyramid_batch(images, levels=levels)
    b = batching.PatchBatcher(images, pyr_images, poses, times, pyr_hwf, NEAR, FAR, device=dev)
    return types.SimpleNamespace(b=b, images=images, pyr_images=pyr_images, pyr_hwf=pyr_hwf, poses=torch.from_numpy(poses).to(dev),
                                 times=torch.from_numpy(times).to(dev), times_host=times)


MAIN = (40, 56, 4, [8, 4, 2, 1], [(3, 5), (2, 3), (1, 1), (4, 6)], [(8, 8), (4, 4), (2, 2), (1, 1)])
SHAPES = {
    "main": MAIN,
    "clipped": (36, 52, 4, [32, 16, 8, 4], [(2, 4), (1, 2), (2, 6), (1, 3)], [(32, 32), (16, 16), (7, 7), (3, 3)]),
    "whole_levels": (12, 20, 2, [32, 16], [(0, 0), (0, 0)], [(12, 20), (6, 10)]),
}


# ---- rows and targets -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_rows_and_targets_bit_for_bit(dev, name):
    H, W, levels, patch, coords, sizes = SHAPES[name]
    s = make_batcher(dev, H, W, levels)
    assert batching.clipped_patch_sizes(s.pyr_hwf, coords, patch) == sizes
    for img_i in (0, 2):
        rows, targets, full = s.b.batch(img_i, coords, patch)
        for l, ((H_l, W_l, f_l), (y, x), (ph, pw)) in enumerate(zip(s.pyr_hwf, coords, sizes)):
            ro, rd = get_rays(H_l, W_l, float(f_l), s.poses[img_i, :3, :4])
            want = pack_ray_batch(ro[y:y + ph, x:x + pw], rd[y:y + ph, x:x + pw].reshape(-1, 3), NEAR, FAR, frame_time=float(s.times_host[img_i]))
            assert rows[l].shape == (ph * pw, 12) and torch.equal(rows[l], want), (name, img_i, l)
            assert torch.equal(rows[l][:, 8], s.times[img_i].expand(ph * pw))
            assert torch.equal(targets[l], s.pyr_images[l][img_i][y:y + patch[l], x:x + patch[l]]), (name, img_i, l)
        y, x = coords[0]
        assert torch.equal(full, s.images[img_i][y:y + patch[0], x:x + patch[0]])


def test_patch_batcher_validation(dev):
    s = make_batcher(dev, 12, 20, 2)
    imgs, poses, times = scene(3, 12, 20)
    with pytest.raises(RuntimeError):
        batching.PatchBatcher(s.images, s.pyr_images, poses, times, s.pyr_hwf, NEAR, FAR, device="cpu")
    with pytest.raises(ValueError):
        batching.PatchBatcher(s.images, s.pyr_images[:1], poses, times, s.pyr_hwf, NEAR, FAR, device=dev)
    with pytest.raises(ValueError):
        batching.PatchBatcher(s.images[:, :10], s.pyr_images, poses, times, s.pyr_hwf, NEAR, FAR, device=dev)
    with pytest.raises(ValueError):
        batching.PatchBatcher(s.images, s.pyr_images, poses, times[:2], s.pyr_hwf, NEAR, FAR, device=dev)
    with pytest.raises(ValueError):
        s.b.batch(3, [(0, 0), (0, 0)], [32, 16])
    with pytest.raises(ValueError):
        s.b.batch(0, [(12, 0), (0, 0)], [32, 16])
    with pytest.raises(ValueError):
        batching.multires_loss([torch.zeros(4, 3, device=dev)], None, [torch.zeros(2, 3, 3, device=dev)], torch.zeros(2, 3, 3, device=dev), True)
    with pytest.raises(ValueError):
        batching.multires_loss([torch.zeros(33 * 2, 3, device=dev)], None, [torch.zeros(33, 2, 3, device=dev)], torch.zeros(33, 2, 3, device=dev), True)


# ---- the loss ---------------------------------------------------------------------------------------------------------------
def loss_inputs(sizes, seed, rgb0):
    g = torch.Generator().manual_seed(seed)
    r = lambda h, w: torch.rand(h, w, 3, generator=g)
    rgbs = [r(h, w).reshape(-1, 3) for h, w in sizes]
    rgb0s = [r(h, w).reshape(-1, 3) for h, w in sizes] if rgb0 else None
    targets = [r(h, w) - 0.3 for h, w in sizes]
    return rgbs, rgb0s, targets, r(*sizes[0])


def to_dev(ts, dev, grad=False):
    return None if ts is None else [t.to(dev).requires_grad_(grad) for t in ts]


@pytest.mark.parametrize("sizes", [[(8, 8), (4, 4), (2, 2), (1, 1)], [(32, 32), (16, 16), (7, 7), (3, 3)], [(12, 20), (6, 10)], [(5, 3)],
                                   [(3, 4), (3, 4)]], ids=["8421", "clipped_non_2x", "12x20", "one_level", "equal_sizes"])
def test_reconstruction_bit_for_bit(dev, sizes):
    rgbs, _, targets, full = loss_inputs(sizes, 3, False)
    out = batching.multires_loss(to_dev(rgbs, dev), None, to_dev(targets, dev), full.to(dev), True)
    want = pyramid.reconstruct_image_from_pyramid_batch([r.reshape(h, w, 3)[None].to(dev) for r, (h, w) in zip(rgbs, sizes)])[0]
    assert out[5].shape == want.shape and torch.equal(out[5], want)
    assert not out[5].requires_grad


def op_by_op(rgbs, rgb0s, targets, full, add_global):
    """the loss of runner.multires_train_loss without a batcher, from the rendered colours on: F.mse_loss per level,
    pyramid.reconstruct_and_compute_loss, autograd"""
    outs, per_level, per_level0, loss = [], [], [], 0
    for l, (rgb, tgt) in enumerate(zip(rgbs, targets)):
        ph, pw = tgt.shape[:2]
        rgb = rgb.reshape(ph, pw, 3)
        img_loss = F.mse_loss(rgb, tgt)
        per_level0.append(None)
        if rgb0s is not None:
            per_level0[-1] = F.mse_loss(rgb0s[l].reshape(ph, pw, 3), tgt)
            loss = loss + per_level0[-1]
        loss = loss + img_loss
        per_level.append(img_loss)
        outs.append(rgb.unsqueeze(0))
    rec, global_loss, psnr = pyramid.reconstruct_and_compute_loss(outs, full)
    if add_global:
        loss = loss + global_loss
    return loss, per_level, per_level0, global_loss, psnr, rec


def errors(out, ref, rgbs, rgb0s):
    """(max error of the loss scalars, max error of the gradient elements) against the float64 restatement"""
    loss, per_level, per_level0, global_loss = out[:4]
    d = lambda a, b: abs(float(a.detach()) - b)
    e_loss = max([d(loss, ref["loss"]), d(global_loss, ref["global_loss"])] + [d(a, b) for a, b in zip(per_level, ref["per_level"])]
                 + [d(a, b) for a, b in zip(per_level0, ref["per_level0"]) if b is not None])
    loss.backward()
    dist = lambda t, want: float(np.abs(t.grad.cpu().numpy().astype(np.float64).reshape(want.shape) - want).max())
    e_grad = max([dist(t, w) for t, w in zip(rgbs, ref["d_rgb"])] + ([] if rgb0s is None else [dist(t, w) for t, w in zip(rgb0s, ref["d_rgb0"])]))
    return e_loss, e_grad


@pytest.mark.parametrize("levels,add_global,rgb0", [(4, True, True), (4, True, False), (4, False, True), (4, False, False),
                                                    (1, True, True), (1, False, False)])
def test_loss_and_gradients_against_float64(dev, levels, add_global, rgb0):
    sizes = [(8, 8), (4, 4), (2, 2), (1, 1)][:levels]
    rgbs, rgb0s, targets, full = loss_inputs(sizes, 11 + levels, rgb0)
    ref = M.loss_and_grads([t.numpy() for t in rgbs], None if rgb0s is None else [t.numpy() for t in rgb0s], [t.numpy() for t in targets],
                           full.numpy(), add_global)
    t_dev, f_dev = to_dev(targets, dev), full.to(dev)
    a, a0 = to_dev(rgbs, dev, True), to_dev(rgb0s, dev, True)
    e_op = errors(op_by_op(a, a0, t_dev, f_dev, add_global), ref, a, a0)
    b, b0 = to_dev(rgbs, dev, True), to_dev(rgb0s, dev, True)
    fused = batching.multires_loss(b, b0, t_dev, f_dev, add_global)
    assert (fused[2][0] is not None) == rgb0 and len(fused[1]) == levels
    psnr64 = 10 * np.log10(1 / ref["global_loss"])
    e_fused = errors(fused, ref, b, b0)
    print(f"levels {levels} add_global {add_global} rgb0 {rgb0}: loss scalars op-by-op {e_op[0]:.3e} fused {e_fused[0]:.3e}; "
          f"gradients op-by-op {e_op[1]:.3e} fused {e_fused[1]:.3e}; psnr {float(fused[4]):.5f} vs {psnr64:.5f}")
    assert abs(float(fused[4]) - psnr64) <= 4 * 2.0 ** -23 * abs(psnr64)                 # formed in fp64, rounded once
    assert e_fused[0] <= 2 * e_op[0] and e_fused[1] <= 2 * e_op[1]


def test_backward_scales_the_stored_gradients(dev):
    rgbs, rgb0s, targets, full = loss_inputs([(8, 8), (4, 4)], 5, True)
    a, a0 = to_dev(rgbs, dev, True), to_dev(rgb0s, dev, True)
    batching.multires_loss(a, a0, to_dev(targets, dev), full.to(dev), True)[0].backward()
    b, b0 = to_dev(rgbs, dev, True), to_dev(rgb0s, dev, True)
    (batching.multires_loss(b, b0, to_dev(targets, dev), full.to(dev), True)[0] * 0.5).backward()
    for x, y in zip(a + a0, b + b0):
        assert torch.equal(x.grad * 0.5, y.grad)
    # one level without rgb0 among levels with it
    c, c0 = to_dev(rgbs, dev, True), [rgb0s[0].to(dev).requires_grad_(True), None]
    out = batching.multires_loss(c, c0, to_dev(targets, dev), full.to(dev), False)
    out[0].backward()
    assert out[2][1] is None and torch.equal(c0[0].grad, a0[0].grad)
    assert float(out[0].detach()) == pytest.approx(float(out[1][0]) + float(out[1][1]) + float(out[2][0]), rel=1e-6)


def test_two_calls_give_equal_bits(dev):
    sizes = [(32, 32), (16, 16), (7, 7), (3, 3)]
    rgbs, rgb0s, targets, full = loss_inputs(sizes, 9, True)
    runs = []
    for _ in range(2):
        a, a0 = to_dev(rgbs, dev, True), to_dev(rgb0s, dev, True)
        out = batching.multires_loss(a, a0, to_dev(targets, dev), full.to(dev), True)
        out[0].backward()
        runs.append([out[0].detach(), torch.stack(out[1]), torch.stack(out[2]), out[3], out[4], out[5]] + [t.grad for t in a + a0])
    for x, y in zip(*runs):
        assert torch.equal(x, y)
    s = make_batcher(dev, 36, 52, 4)
    one, two = (s.b.batch(1, SHAPES["clipped"][4], SHAPES["clipped"][3]) for _ in range(2))
    for x, y in zip(one[0] + one[1] + [one[2]], two[0] + two[1] + [two[2]]):
        assert torch.equal(x, y)


# ---- runner.multires_train_loss with and without the batcher ------------------------------------------------------------------
def level_args(tmp=None, **over):
    a = dict(layer_num=4, use_viewdirs=True, N_importance=0, N_samples=8, nerf_type="direct_temporal", netdepth=2, netwidth=64,
             netdepth_fine=2, netwidth_fine=64, use_two_models_for_fine=False, not_zero_canonical=False, netchunk=1 << 16,
             lrate=5e-4, lrate_decay=250, basedir="/nonexistent" if tmp is None else str(tmp), expname="mr", ft_path=None, no_reload=True,
             perturb=0.0, white_bkgd=True, raw_noise_std=0.0, dataset_type="blender", no_ndc=False, lindisp=False,
             do_half_precision=False, chunk=1 << 15, global_optimization_epoch=10, reproducible_wgrad=True)
    a.update(over)
    return types.SimpleNamespace(**a)


@pytest.mark.parametrize("n_importance,two_models", [(0, False), (4, False), (4, True)])
def test_batcher_switch(dev, n_importance, two_models):
    """N_importance = 4 with one model per level resamples from a no_grad coarse pass and has no rgb0, as in the reference; with
    use_two_models_for_fine the coarse net's rgb0 enters the loss.
    loss: both paths are compared with the float64 restatement on the colours the nets rendered (the rows are bit-equal, so both
    paths render the same colours); the two fp32 losses may differ by the op-by-op path's error e_op plus the fused path's, which
    is at most 2 e_op (test_loss_and_gradients_against_float64), and never by less than one fp32 rounding of the loss: gate
    max(3 e_op, ulp(loss)).  Parameter gradients: backward is linear in d_rgb and the two d_rgb differ by fp32 roundings (relative
    1.2e-7) of their terms; with the ordered weight-gradient sums the passes are otherwise the same launches, so the gradients of a
    net agree to 1e-6 max(1, max |grad|) - the form of the bound tests/test_gpu_pyramid.py uses for the joint step."""
    H, W, levels, patch, coords, sizes = MAIN
    s = make_batcher(dev, H, W, levels)
    args = level_args(N_importance=n_importance, use_two_models_for_fine=two_models)
    torch.manual_seed(4321)
    trains = runner.create_multires(args, device=dev)[0]
    for kw in trains:
        kw.update({"near": NEAR, "far": FAR})
    nets = [kw[k] for kw in trains for k in ("network_fn", "network_fine") if kw.get(k) is not None]
    seen = {}
    real = batching.multires_loss

    def spy(rgbs, rgb0s, targets, full, add_global):
        seen.update(rgbs=[r.detach().cpu().numpy() for r in rgbs], rgb0s=[None if r is None else r.detach().cpu().numpy() for r in rgb0s],
                    targets=[t.cpu().numpy() for t in targets], full=full.cpu().numpy())
        return real(rgbs, rgb0s, targets, full, add_global)

    def run(batcher):
        for net in nets:
            net.zero_grad()
        loss, per_level, gl, psnr, rec = runner.multires_train_loss(10, 1, s.images, s.pyr_images, s.poses, s.times, s.pyr_hwf, patch, trains,
                                                                    args, patch_coords=coords, batcher=batcher)
        loss.backward()
        return (loss.detach(), [p.detach() for p in per_level], gl.detach(), rec.detach(),
                [[p.grad.clone() for p in net.parameters() if p.grad is not None] for net in nets])
    plain = run(None)
    batching.multires_loss = spy
    try:
        fused = run(s.b)
    finally:
        batching.multires_loss = real
    assert all((r is not None) == two_models for r in seen["rgb0s"])
    ref = M.loss_and_grads(seen["rgbs"], seen["rgb0s"], seen["targets"], seen["full"], True)
    e_op, e_fused = abs(float(plain[0]) - ref["loss"]), abs(float(fused[0]) - ref["loss"])
    ulp = float(np.spacing(np.float32(ref["loss"])))
    print(f"N_importance {n_importance} two models {two_models}: loss {ref['loss']:.6f}; op-by-op off by {e_op:.3e}, with the batcher by {e_fused:.3e}, apart by "
          f"{abs(float(plain[0]) - float(fused[0])):.3e} (gate {max(3 * e_op, ulp):.3e})")
    assert abs(float(plain[0]) - float(fused[0])) <= max(3 * e_op, ulp)
    assert torch.equal(plain[3], fused[3])                                               # the reconstruction: the same kernels' arithmetic
    assert sum(float(g.abs().max()) > 0 for g in plain[4][0]) > 0
    for l in range(len(nets)):                                                           # (a net may see a zero gradient: the 1 x 1 patch is one ray)
        assert len(plain[4][l]) == len(fused[4][l]) > 0
        mag = max(float(g.abs().max()) for g in plain[4][l])
        apart = max(float((a - b).abs().max()) for a, b in zip(plain[4][l], fused[4][l]))
        print(f"  net {l}: max |grad| {mag:.3e}, the two paths apart by {apart:.3e} (gate {1e-6 * max(1.0, mag):.3e})")
        assert apart <= 1e-6 * max(1.0, mag)


# ---- train_multires ---------------------------------------------------------------------------------------------------------
def train_args(tmp, **over):
    a = vars(level_args(tmp, layer_num=2, netwidth=32, netwidth_fine=32, global_optimization_epoch=2, perturb=1.0))
    a.update(N_iter=4, N_rand=32, no_batching=True, precrop_iters=1, precrop_frac=.5, precrop_iters_time=2, add_tv_loss=True,
             tv_loss_weight=1e-4, i_print=2, i_weights=2, i_testset=4, seed=3)
    a.update(over)
    return types.SimpleNamespace(**a)


def train_data():
    imgs, poses, times = scene(6, 24, 24, seed=5)
    return (imgs, poses, poses[:1], [24, 24, focal_of(24)], [[0, 1, 2, 3, 5], [], [4]], times, NEAR, FAR)


def run_training(tmp, dev, **kw):
    over = {k: kw.pop(k) for k in list(kw) if k not in ("sampler", "private_target")}
    args = train_args(tmp, **over)
    random.seed(1)
    np.random.seed(1)
    torch.manual_seed(1)
    rec = runner.train_multires(args, train_data(), device=dev, **kw)
    return args, rec


def test_train_multires_end_to_end(dev, tmp_path):
    torch.manual_seed(1)
    before = [[p.detach().clone() for p in kw["network_fn"].parameters()] for kw in runner.create_multires(train_args(tmp_path / "init"), device=dev)[0]]
    args, rec = run_training(tmp_path, dev)
    base = os.path.join(str(tmp_path), "mr")
    assert [len(r) for r in rec["private"]] == [2, 2] and [r["step"] for r in rec["joint"]] == [1, 2, 3, 4]
    assert all(np.isfinite(r["loss"]) for r in rec["joint"]) and all(np.isfinite(r["loss"]) for lv in rec["private"] for r in lv)
    print("private", [[r["loss"] for r in lv] for lv in rec["private"]], "joint", [r["loss"] for r in rec["joint"]])
    assert sorted(f for f in os.listdir(base) if f.endswith(".tar")) == ["000000.tar", "000002.tar", "000004.tar"]
    log = open(os.path.join(base, "log.txt")).read()
    assert log.count("[TRAIN] Iter: 0 ") == 2 and "[TRAIN] Layer: 1 Iter: 2 " in log and "[GLOBAL OPT] Iter: 4 " in log
    assert os.path.exists(os.path.join(base, "testset_000004", "estim", "000.png"))
    # the checkpoint is the MultiRes format: load_multires reads every level back, and every level's parameters have moved
    torch.manual_seed(1)
    trains, _, _, _, opts = runner.create_multires(args, device=dev)
    for l, kw in enumerate(trains):
        assert checkpoint.load_multires(os.path.join(base, "000002.tar"), l, kw["network_fn"], kw.get("network_fine"), opts[l], map_location=dev) == 2
        moved = [not torch.equal(a, b) for a, b in zip(before[l], kw["network_fn"].parameters())]
        assert all(torch.isfinite(p).all() for p in kw["network_fn"].parameters())
        names = [n for n, _ in kw["network_fn"].named_parameters()]
        print(f"level {l}: {sum(moved)} of {len(moved)} parameter tensors moved; unmoved: {[n for n, m in zip(names, moved) if not m]}")
        assert all(moved), l
    # a resumed run starts its joint phase behind the newest checkpoint
    args2 = train_args(tmp_path, no_reload=False, N_iter=5)
    np.random.seed(2)
    rec2 = runner.train_multires(args2, train_data(), device=dev)
    assert [r["step"] for r in rec2["joint"]] == [5]


@pytest.mark.parametrize("kw", [dict(sampler="numpy"), dict(private_target="pyramid"), dict(optimizer="fused"), dict(N_importance=4, layer_num=1)],
                         ids=["numpy", "pyramid", "fused", "one_level_fine"])
def test_train_multires_options(dev, tmp_path, kw):
    args, rec = run_training(tmp_path, dev, **kw)
    assert [r["step"] for r in rec["joint"]] == [1, 2, 3, 4] and all(np.isfinite(r["loss"]) for r in rec["joint"])
    assert len(rec["private"]) == args.layer_num and os.path.exists(os.path.join(str(tmp_path), "mr", "000002.tar"))
    with pytest.raises(ValueError):
        runner.train_multires(args, train_data(), device=dev, sampler="torch")
    with pytest.raises(ValueError):
        runner.train_multires(args, train_data(), device=dev, private_target="level")


def test_train_multires_repeats_bit_for_bit(dev, tmp_path):
    run_training(tmp_path / "a", dev, i_testset=100)
    run_training(tmp_path / "b", dev, i_testset=100)
    for name in ("000002.tar", "000004.tar"):
        a, b = (torch.load(os.path.join(str(tmp_path / d), "mr", name), map_location="cpu", weights_only=False) for d in ("a", "b"))
        assert a.keys() == b.keys() and a["global_step"] == b["global_step"]
        for l in range(2):
            for k in a[f"network_fn_{l}"]:
                assert torch.equal(a[f"network_fn_{l}"][k], b[f"network_fn_{l}"][k]), (name, l, k)
            for sa, sb in zip(a[f"optimizer_{l}"]["state"].values(), b[f"optimizer_{l}"]["state"].values()):
                assert all(torch.equal(torch.as_tensor(sa[k]), torch.as_tensor(sb[k])) for k in sa)
