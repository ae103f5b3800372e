"""GPU tests of the training-batch kernels (csrc/batch_kernels.hip), swnerf.batching and runner.train / train_dnerf.

  rows, targets   bit-equal to the standalone path get_rays -> index -> pack_ray_batch and to images[i][ys, xs]: one arithmetic
  permutation     the device ids equal batching.perm_index_np; an epoch visits every ray once
  bytes           all 256 x 256 (colour, alpha) pairs bit-equal to the loaders' numpy float32 expression
  photo_loss      within 2 fp32 ulps of a float64 evaluation (one rounding of the fp64 sum, one of the scale), equal bits twice
  train()         the numpy sampler's first step equals a hand loop exactly; the default path learns, follows the lr formula,
                  writes a checkpoint and resumes from it; train_dnerf's time column, TV renders and refusal
(examples/train_lego_like.py runs as a child process from tests/test_00_a_batching_tight_buffers.py, which starts its children
before any test has initialised the GPU in the pytest process.)
Every test prints the figure it measured before it asserts."""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from swnerf import _lib, batching, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEAR, FAR = 2., 6.


def scene(n_img, H, W, ch=3, dtype=np.float32, seed=0):
    rng = np.random.default_rng(seed + 1000 * H + W)
    if dtype == np.uint8:
        images = rng.integers(0, 256, (n_img, H, W, ch), dtype=np.uint8)
    else:
        images = rng.uniform(0, 1, (n_img, H, W, ch)).astype(np.float32)
    poses = np.stack([synth.pose_spherical(30.0 + 47.0 * i, -30.0 + 9.0 * i, 4.0 + 0.1 * i) for i in range(n_img)]).astype(np.float32)
    times = np.linspace(0.0, 1.0, n_img).astype(np.float32) if n_img > 1 else np.array([0.25], np.float32)
    return images, poses, times


def intrinsics(H, W, branch):
    focal = float(0.5 * W / np.tan(0.5 * synth.LEGO_CAMERA_ANGLE_X))
    if branch == "focal":
        return [H, W, focal], focal, focal
    K = np.array([[focal, 0, 0.5 * W + 0.75], [0, 1.125 * focal, 0.5 * H - 1.5], [0, 0, 1]], np.float64)
    return K, K, focal


def reference_rows(H, W, get_rays_arg, ndc_focal, pose, ys, xs, cols, ndc, frame_time):
    """The parent path: all rays of the image, fancy indexing, pack_ray_batch."""
    from swnerf import ray, render
    rays_o, rays_d = ray.get_rays(H, W, get_rays_arg, torch.from_numpy(pose[:3, :4]).to(DEV))
    ys, xs = torch.as_tensor(ys, device=DEV), torch.as_tensor(xs, device=DEV)
    o, d = rays_o[ys, xs], rays_d[ys, xs]
    rb = render.pack_ray_batch(o, d, NEAR, FAR, frame_time=frame_time if cols == 12 else None, ndc=ndc, H=H, W=W, focal=ndc_focal)
    return rb[:, :8].contiguous() if cols == 8 else rb


VARIANTS = [(11, False, "K"), (11, True, "focal"), (8, False, "focal"), (8, True, "K"), (12, False, "focal"), (12, True, "focal")]


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
@pytest.mark.parametrize("H,W", [(5, 7), (37, 53)])
def test_ids_mode_equals_the_standalone_path(H, W, n):
    images, poses, times = scene(3, H, W)
    rng = np.random.default_rng(n + H)
    for v, (cols, ndc, branch) in enumerate(VARIANTS):
        hwf_or_K, get_rays_arg, focal = intrinsics(H, W, branch)
        ndc_focal = focal if branch == "focal" else float(hwf_or_K[0][0])
        b = batching.RayBatcher(images, poses, hwf_or_K, [0, 1, 2], NEAR, FAR, times=times if cols == 12 else None, ndc=ndc,
                                use_viewdirs=cols != 8, device=DEV)
        assert b.cols == cols
        for crop in (None, batching.precrop_crop(H, W, 0.5)):
            y0, x0, h, w = (0, 0, H, W) if crop is None else crop
            img_i = (v + (crop is not None)) % 3
            ids = rng.integers(0, h * w, n)
            ids[-1] = h * w - 1                                                  # the window's last pixel
            rb, target = b.image_batch(img_i, n, step=0, crop=crop, ids=ids)
            ys, xs = y0 + ids // w, x0 + ids % w
            want = reference_rows(H, W, get_rays_arg, ndc_focal, poses[img_i], ys, xs, cols, ndc, float(times[img_i]))
            assert rb.shape == (n, cols) and target.shape == (n, 3)
            assert torch.equal(rb, want), (cols, ndc, branch, crop, float((rb - want).abs().max()))
            assert np.array_equal(target.cpu().numpy(), images[img_i][ys, xs])
            if cols == 12:
                assert bool((rb[:, 8] == float(times[img_i])).all())


def _raw_batch(b, n, cols, ids, out_ptr, target):
    fx, fy, cx, cy, fb = b.intr
    one = ctypes.c_void_p(b.all_images.data_ptr())
    _lib.check(_lib.lib().swnerf_train_batch(
        _lib.ptr(b.images), 0, b.channels, b.n_images, b.H, b.W, _lib.ptr(b.c2w), _lib.ptr(b.times), one, 1, 0, 0, b.H, b.W,
        fx, fy, cx, cy, fb, b.near, b.far, cols, 0, fx, 0, 0, 0, n, _lib.ptr(ids), out_ptr, _lib.ptr(target), None,
        _lib.stream_of(target)), "train_batch")


@pytest.mark.parametrize("cols", [8, 11, 12])
def test_unaligned_output_takes_the_dword_path(cols):
    H, W, n = 37, 53, 600                                                        # two full blocks and a tail
    images, poses, times = scene(3, H, W)
    b = batching.RayBatcher(images, poses, intrinsics(H, W, "focal")[0], [0], NEAR, FAR, times=times if cols == 12 else None,
                            use_viewdirs=cols != 8, device=DEV)
    ids = torch.from_numpy(np.random.default_rng(cols).integers(0, H * W, n)).to(DEV)
    aligned, _ = b.image_batch(0, n, 0, ids=ids)
    assert aligned.data_ptr() % 16 == 0
    flat = torch.full((n * cols + 5,), -7.0, device=DEV)
    target = torch.empty((n, 3), device=DEV)
    _raw_batch(b, n, cols, ids, ctypes.c_void_p(flat.data_ptr() + 4), target)
    torch.cuda.synchronize()
    assert torch.equal(flat[1:1 + n * cols].reshape(n, cols), aligned)
    assert float(flat[0]) == -7.0 and bool((flat[1 + n * cols:] == -7.0).all())       # nothing written around the batch


def test_permutation_ids_equal_numpy():
    for key, n, k0, count in [(0, 1, 0, 1), (5, 37, 0, 37), (2 ** 63 + 11, 1000, 100, 900), (77, 2 ** 16 + 1, 0, 2 ** 16 + 1),
                              (1234567, 3 * 800 * 800, 1_900_000, 4096), (9, 2 ** 40 - 1, 2 ** 39, 513)]:
        got = batching.perm_indices(key, n, k0, count, DEV).cpu().numpy()
        want = batching.perm_index_np(key, n, np.arange(k0, k0 + count))
        assert np.array_equal(got, want), (key, n)


def test_image_batch_draw_is_the_keyed_permutation_and_repeats():
    H, W = 37, 53
    images, poses, _ = scene(3, H, W)
    b = batching.RayBatcher(images, poses, intrinsics(H, W, "K")[0], [0, 1, 2], NEAR, FAR, seed=3, device=DEV)
    crop = batching.precrop_crop(H, W, 0.5)
    rb1, t1, ids1 = b.image_batch(1, 300, step=17, crop=crop, return_ids=True)
    rb2, t2, ids2 = b.image_batch(1, 300, step=17, crop=crop, return_ids=True)
    assert torch.equal(rb1, rb2) and torch.equal(t1, t2) and torch.equal(ids1, ids2)
    want = batching.perm_index_np(batching.batch_key(3, 17, 0), crop[2] * crop[3], np.arange(300))
    assert np.array_equal(ids1.cpu().numpy(), want) and len(set(want.tolist())) == 300
    _, _, ids3 = b.image_batch(1, 300, step=18, crop=crop, return_ids=True)
    assert not torch.equal(ids1, ids3)
    rb4, t4 = b.image_batch(1, 300, step=0, crop=crop, ids=ids1)                # the same ids handed in: the same batch
    assert torch.equal(rb4, rb1) and torch.equal(t4, t1)
    with pytest.raises(RuntimeError, match="domain"):
        b.image_batch(1, crop[2] * crop[3] + 1, step=0, crop=crop)


def test_global_batch_epoch_visits_every_ray_once():
    H, W = 37, 53
    images, poses, _ = scene(4, H, W)
    i_train = [2, 0, 3]
    K, get_rays_arg, _ = intrinsics(H, W, "K")
    b = batching.RayBatcher(images, poses, K, i_train, NEAR, FAR, seed=1, device=DEV)
    domain = 3 * H * W
    rows, targets, ids, lens = [], [], [], []
    while b.cursor.epoch == 0:
        rb, tg, idd = b.global_batch(1000, return_ids=True)
        rows.append(rb); targets.append(tg); ids.append(idd); lens.append(rb.shape[0])
    assert lens == [1000] * 5 + [domain - 5000]
    ids = torch.cat(ids).cpu().numpy()
    assert np.array_equal(np.sort(ids), np.arange(domain))
    assert np.array_equal(ids, batching.perm_index_np(batching.batch_key(1, 0, 1), domain, np.arange(domain)))
    rows, targets = torch.cat(rows), torch.cat(targets).cpu().numpy()
    slot, rem = ids // (H * W), ids % (H * W)
    ys, xs = rem // W, rem % W
    for s, img in enumerate(i_train):                                            # every row is the ray of ITS image, pixel and pose
        m = slot == s
        want = reference_rows(H, W, get_rays_arg, float(K[0][0]), poses[img], ys[m], xs[m], 11, False, None)
        assert torch.equal(rows[torch.from_numpy(m).to(DEV)], want), img
        assert np.array_equal(targets[m], images[img][ys[m], xs[m]])
    _, _, nxt = b.global_batch(1000, return_ids=True)                            # the next epoch: a new key
    assert b.cursor.epoch == 1 and not np.array_equal(nxt.cpu().numpy(), ids[:1000])


@pytest.mark.parametrize("white", [False, True])
def test_uint8_rgba_all_colour_alpha_pairs(white):
    c, a = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    img = np.stack([c, 255 - c, c ^ 0x55, a], -1)[None]                          # [1, 256, 256, 4]: channel 0 x alpha = every pair
    pose = synth.pose_spherical(30., -30., 4.)[None].astype(np.float32)
    b = batching.RayBatcher(img, pose, [256, 256, 300.0], [0], NEAR, FAR, white_bkgd=white, device=DEV)
    assert b.images.dtype == torch.uint8                                         # kept as given
    _, target = b.image_batch(0, 65536, 0, ids=np.arange(65536))
    f = (img[0] / 255.).astype(np.float32)                                       # the loaders (load_blender.py)
    want = f[..., :3] * f[..., -1:] + (1. - f[..., -1:]) if white else f[..., :3]   # nerf/run.py:469-472
    assert want.dtype == np.float32
    got = target.cpu().numpy().reshape(256, 256, 3)
    print("uint8 RGBA, white", white, "mismatches", int((got != want).sum()))
    assert np.array_equal(got, want)


def test_uint8_rgb_and_float_rgba():
    H, W = 5, 7
    img8, poses, _ = scene(2, H, W, 3, np.uint8)
    b = batching.RayBatcher(img8, poses, [H, W, 9.0], [0, 1], NEAR, FAR, device=DEV)
    _, t = b.image_batch(1, 35, 0, ids=np.arange(35))
    assert np.array_equal(t.cpu().numpy().reshape(H, W, 3), (img8[1] / 255.).astype(np.float32))
    imgf, _, _ = scene(2, H, W, 4)
    for white in (False, True):
        b = batching.RayBatcher(imgf, poses, [H, W, 9.0], [0, 1], NEAR, FAR, white_bkgd=white, device=DEV)
        _, t = b.image_batch(0, 35, 0, ids=np.arange(35))
        f = imgf[0]
        want = f[..., :3] * f[..., -1:] + (1. - f[..., -1:]) if white else f[..., :3]
        assert np.array_equal(t.cpu().numpy().reshape(H, W, 3), want)


def test_bad_ids_give_nan_rows_and_read_nothing():
    H, W = 5, 7
    images, poses, _ = scene(2, H, W)
    b = batching.RayBatcher(images, poses, [H, W, 9.0], [0, 1], NEAR, FAR, device=DEV)
    rb, t = b.image_batch(0, 4, 0, ids=np.array([0, -1, 35, 34]))
    rb, t = rb.cpu().numpy(), t.cpu().numpy()
    assert np.isnan(rb[1:3]).all() and np.isnan(t[1:3]).all() and np.isfinite(rb[[0, 3]]).all() and np.isfinite(t[[0, 3]]).all()


def _ulps(got, ref64):
    ref64 = np.asarray(ref64, np.float64)
    return np.abs(np.asarray(got, np.float64) - ref64) / np.spacing(np.abs(ref64).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("with0", [False, True])
@pytest.mark.parametrize("N", [1, 33, 4096])
def test_photo_loss_against_float64(N, with0):
    g = torch.Generator().manual_seed(N + with0)
    rgb, rgb0, target = (torch.rand(N, 3, generator=g) for _ in range(3))
    runs = []
    for _ in range(2):
        x = rgb.to(DEV).requires_grad_(True)
        x0 = rgb0.to(DEV).requires_grad_(True) if with0 else None
        loss, img_loss, img_loss0 = batching.photometric_loss(x, target.to(DEV), x0)
        loss.backward()
        runs.append([loss.detach().cpu(), img_loss.detach().cpu(), x.grad.cpu()] + ([img_loss0.detach().cpu(), x0.grad.cpu()] if with0 else []))
    assert (img_loss0 is None) == (not with0)
    for a, b in zip(*runs):
        assert torch.equal(a, b)                                                 # bit-identical from run to run
    d, d0, t = rgb.double().numpy(), rgb0.double().numpy(), target.double().numpy()
    mse, mse0 = ((d - t) ** 2).mean(), ((d0 - t) ** 2).mean() if with0 else 0.0
    fig = [float(_ulps(runs[0][0].numpy(), mse + mse0)), float(_ulps(runs[0][1].numpy(), mse)),
           float(_ulps(runs[0][2].numpy(), 2 * (d - t) / (3 * N)).max())]
    if with0:
        fig += [float(_ulps(runs[0][3].numpy(), mse0)), float(_ulps(runs[0][4].numpy(), 2 * (d0 - t) / (3 * N)).max())]
    print(f"photo_loss N={N} rgb0={with0}: ulps from float64 (loss, mse, d_rgb[, mse0, d_rgb0]) = {fig}")
    assert max(fig) <= 2.0


# ---- train() ------------------------------------------------------------------------------------------------------------
def nerf_args(tmp, **over):
    a = dict(expname="loop", basedir=str(tmp), netdepth=8, netwidth=256, netdepth_fine=8, netwidth_fine=256, lrate=5e-4,
             lrate_decay=500, netchunk=1024 * 64, no_reload=False, ft_path=None, N_samples=64, N_importance=128, perturb=1.,
             use_viewdirs=True, i_embed=0, multires=10, multires_views=4, raw_noise_std=0., dataset_type="blender", white_bkgd=True,
             no_ndc=False, lindisp=False, chunk=1024 * 32, N_rand=256, no_batching=True, precrop_iters=0, precrop_frac=.5,
             i_print=1000, i_weights=1000, i_testset=100000, N_iters=25, seed=0)
    a.update(over)
    return SimpleNamespace(**a)


def nerf_data(n_img, H, W, seed=2):
    rng = np.random.default_rng(seed)
    images = rng.uniform(0, 1, (n_img, H, W, 3)).astype(np.float32)
    poses = np.stack([synth.pose_spherical(30.0 + 40.0 * i, -30.0, 4.0) for i in range(n_img)]).astype(np.float32)
    focal = float(0.5 * W / np.tan(0.5 * synth.LEGO_CAMERA_ANGLE_X))
    return images, poses, poses[:1], [H, W, focal], [list(range(n_img)), [], []], NEAR, FAR


def test_numpy_sampler_first_step_equals_a_hand_loop(tmp_path):
    """sampler="numpy" and the plain img2mse sum: the first step's batch and loss are those of the reference's loop
    (nerf/run.py:652-699) written by hand on get_rays -> indexing -> render.render -> img2mse, exactly."""
    from swnerf import ray, render, runner
    H, W, N_rand = 16, 16, 64
    data = nerf_data(3, H, W)
    images, poses, _, hwf, i_split, near, far = data
    img2mse = lambda x, y: torch.mean((x - y) ** 2)

    def plain(rgb, target, rgb0):
        a, b = img2mse(rgb, target), img2mse(rgb0, target)
        return a + b, a, b
    seen = {}
    args = nerf_args(tmp_path / "a", N_rand=N_rand, N_iters=1, precrop_iters=5, no_reload=True)
    torch.manual_seed(0)
    np.random.seed(5)
    rec = runner.train(args, data, device=DEV, sampler="numpy", loss_fn=plain,
                       hooks={"on_batch": lambda i, img_i, rb, tg, ids: seen.update(i=i, img_i=img_i, rb=rb.clone(), tg=tg.clone())})
    assert len(rec) == 1 and rec[0]["step"] == 1
    # ---- the hand loop
    torch.manual_seed(0)
    np.random.seed(5)
    train_kw, _, start, _, _ = runner.create_nerf(nerf_args(tmp_path / "b", no_reload=True), device=DEV)
    train_kw.update(near=near, far=far)
    K = np.array([[hwf[2], 0, 0.5 * W], [0, hwf[2], 0.5 * H], [0, 0, 1]])
    img_i = np.random.choice(i_split[0])
    target = torch.from_numpy(images[img_i]).to(DEV)
    rays_o, rays_d = ray.get_rays(H, W, K, torch.from_numpy(poses[img_i, :3, :4]).to(DEV))
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
    assert torch.equal(seen["rb"], render.pack_ray_batch(o, d, near, far, ndc=False)) and torch.equal(seen["tg"], target_s)
    rgb, disp, acc, extras = render.render(H, W, K, chunk=args.chunk, rays=(o, d), retraw=True, **train_kw)
    loss = img2mse(rgb, target_s) + img2mse(extras['rgb0'], target_s)
    print("train() loss", rec[0]["loss"], "hand loop", float(loss))
    assert rec[0]["loss"] == float(loss)


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """25 steps of the default sampler and loss on the nets of test_training_loop_through_create_nerf: one 16 x 16 frame of
    uniform noise with N_rand = 256, so every batch is the same 256 rays and targets in another order - the fixed batch of that
    test.  A checkpoint at step 25, then a second call that resumes from it."""
    from swnerf import runner
    tmp = tmp_path_factory.mktemp("train")
    data = nerf_data(1, 16, 16)
    lrs = []
    args = nerf_args(tmp, i_weights=25)
    torch.manual_seed(0)
    np.random.seed(0)
    rec = runner.train(args, data, device=DEV, hooks={"on_step": lambda i, opt: lrs.append([pg['lr'] for pg in opt.param_groups])})
    ckpt = torch.load(os.path.join(str(tmp), "loop", "000025.tar"), map_location="cpu", weights_only=False)
    rec2 = runner.train(nerf_args(tmp, i_weights=1000, N_iters=26), data, device=DEV)
    return args, rec, lrs, ckpt, rec2


def test_train_default_sampler_and_loss_learn(trained):
    _, rec, _, _, _ = trained
    losses = [r["loss"] for r in rec]
    print("train() losses", losses[0], "->", losses[-1])
    assert len(rec) == 25 and [r["step"] for r in rec] == list(range(1, 26))
    assert all(np.isfinite(losses)) and losses[-1] < 0.8 * losses[0], losses
    assert all(np.isfinite(r["psnr"]) for r in rec)


def test_train_learning_rate_follows_the_formula(trained):
    args, rec, lrs, _, _ = trained
    for k, (r, lr) in enumerate(zip(rec, lrs)):
        want = args.lrate * (0.1 ** (k / (args.lrate_decay * 1000)))            # global_step = k at iteration k + 1 (nerf/run.py:704-706)
        assert r["lr"] == want and all(v == want for v in lr), (k, lr, want)


def test_train_checkpoint_and_resume(trained):
    args, rec, _, ckpt, rec2 = trained
    assert ckpt["global_step"] == 24 and set(ckpt) == {"global_step", "network_fn_state_dict", "network_fine_state_dict", "optimizer_state_dict"}
    # the second call starts at the saved global_step: its first iteration is start + 1 and its lr continues the schedule
    assert [r["step"] for r in rec2] == [ckpt["global_step"] + 1, ckpt["global_step"] + 2]
    assert [r["lr"] for r in rec2] == [args.lrate * (0.1 ** (g / (args.lrate_decay * 1000))) for g in (24, 25)]
    assert rec2[0]["loss"] < 0.9 * rec[0]["loss"]                               # it went on from the trained nets, not from scratch


def dnerf_args(tmp, **over):
    a = vars(nerf_args(tmp, expname="dloop", N_rand=64, N_iter=6, no_reload=True))
    a.update(nerf_type="direct_temporal", not_zero_canonical=False, use_two_models_for_fine=False, do_half_precision=False,
             add_tv_loss=True, tv_loss_weight=1e-4, precrop_iters_time=0)
    a.update(over)
    return SimpleNamespace(**a)


def test_train_dnerf_time_column_tv_renders_and_refusal(tmp_path, monkeypatch):
    from swnerf import render_dnerf, runner
    images, poses, rp, hwf, i_split, near, far = nerf_data(3, 16, 16)
    times = np.array([0.0, 0.5, 1.0], np.float32)
    data = (images, poses, rp, hwf, i_split, times, near, far)
    calls, batches = [], []
    real = render_dnerf.batchify_rays

    def spy(rays_flat, chunk=1024 * 32, **kw):
        ret = real(rays_flat, chunk, **kw)
        calls.append((rays_flat.clone(), None if kw.get("z_vals") is None else kw["z_vals"].clone(), ret["z_vals"].detach().clone()))
        return ret
    monkeypatch.setattr(render_dnerf, "batchify_rays", spy)
    torch.manual_seed(0)
    np.random.seed(1)
    rec = runner.train_dnerf(dnerf_args(tmp_path), data, device=DEV,
                             hooks={"on_batch": lambda i, img_i, rb, tg, ids: batches.append((i, int(img_i), rb.clone()))})
    losses = [r["loss"] for r in rec]
    print("train_dnerf() losses", losses)
    assert len(rec) == 6 and all(np.isfinite(losses))
    assert len(batches) == 6 and len(calls) == 12                                # every step: the frame's render and ONE prev / next render
    for k, (i, img_i, rb) in enumerate(batches):
        assert rb.shape == (64, 12) and bool((rb[:, 8] == float(times[img_i])).all())     # the frame-time column is times[img_i]
        (rb_a, z_in_a, z_out_a), (rb_b, z_in_b, z_out_b) = calls[2 * k], calls[2 * k + 1]
        assert torch.equal(rb_a, rb) and z_in_a is None
        assert torch.equal(rb_b[:, :8], rb[:, :8]) and torch.equal(rb_b[:, 9:], rb[:, 9:])   # the same rays
        assert z_in_b is not None and torch.equal(z_in_b, z_out_a)                            # on the same depths
        t_other = rb_b[:, 8].unique()
        assert t_other.numel() == 1 and times[max(img_i - 1, 0)] <= float(t_other) <= times[min(img_i + 1, 2)]   # between the neighbours
    with pytest.raises(NotImplementedError):
        runner.train_dnerf(dnerf_args(tmp_path / "ub", no_batching=False), data, device=DEV)
