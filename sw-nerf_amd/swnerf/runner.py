"""`create_nerf` of the two runners (nerf/run.py:222-313, d_nerf/run_dnerf.py:238-352): what stands immediately before
the render path - embedders, the network(s), the `network_query_fn` closure, Adam, checkpoint reload - and returns
(render_kwargs_train, render_kwargs_test, start, grad_vars, optimizer) exactly as the reference does, so a `train()`
written against the reference only swaps its imports.  `args` is any object with the reference's option names
(utils.py config_parser / run_dnerf.py config_parser); the closure is built inside the function, which is how
`render.fused_plan` finds the encoders and sends `render_rays` to the fused HIP pass.
`render_test` and `evaluate_dir` are what follows the render path: the reference's scoring of test renders
(nerf/run.py:557-596 with calculate_metrics :49-61, and the last cell of d_nerf/metrics.ipynb) on the GPU metrics.
`train`, `train_dnerf` and `train_tnerf` are the runners' training loops from `create_nerf` on, with the batch and the loss made
on the device (swnerf.batching): one loop (`_train_loop`), and per runner its draw, render, extra loss and test-set
render.  `train_multires` is the MultiRes runner's: per level the D-NeRF iterations on that loop, then the joint iterations on
`multires_train_loss` with a `PatchBatcher` (DESIGN.md 6g "Training")."""
import json
import os
import random
from types import SimpleNamespace

import numpy as np
import torch

from . import metrics, pyramid, render, render_dnerf, render_tnerf, video
from .video import mimwrite
from .png import read_png, write_png
from .checkpoint import reload_latest, find_checkpoints, load_multires, save_multires, to8b
from .ray import get_rays
from .embedder import get_embedder
from .model import vallina_NeRF, NeRF, TNeRF


def _render_kwargs(args, network_query_fn, nets, extra=None):
    """(train, test) dictionaries.  nets: the runner's entries between 'perturb' and 'use_viewdirs', in its key order."""
    kw = {
        'network_query_fn': network_query_fn,
        'perturb': args.perturb,
        **nets,
        'use_viewdirs': args.use_viewdirs,
        'white_bkgd': args.white_bkgd,
        'raw_noise_std': args.raw_noise_std,
    }
    kw.update(extra or {})
    if args.dataset_type != 'llff' or args.no_ndc:               # nerf/run.py:296-299
        kw['ndc'] = False
        kw['lindisp'] = args.lindisp
    test = dict(kw)
    test['perturb'] = False                                      # nerf/run.py:301-303
    test['raw_noise_std'] = 0.
    return kw, test


def _coarse_fine(args, model, model_fine):
    return {'N_importance': args.N_importance, 'network_fine': model_fine, 'N_samples': args.N_samples, 'network_fn': model}


def _refuse_half_precision(args, creator):
    if getattr(args, "do_half_precision", False):
        raise NotImplementedError(f"swnerf.{creator}: do_half_precision (apex amp) is not built; the HIP path is fp32")


def _timed_encoders(args, pos, time, views):
    """The encoders of a runner with frame times, each from (multires, i_embed); `views` is a callable: its options are read
    only with use_viewdirs.  -> embed_fn, embedtime_fn, embeddirs_fn, input_ch, input_ch_time, input_ch_views"""
    embed_fn, input_ch = get_embedder(pos[0], 3, pos[1])
    embedtime_fn, input_ch_time = get_embedder(time[0], 1, time[1])
    input_ch_views, embeddirs_fn = 0, None
    if args.use_viewdirs:
        multires_views, i_embed = views()
        embeddirs_fn, input_ch_views = get_embedder(multires_views, 3, i_embed)
    return embed_fn, embedtime_fn, embeddirs_fn, input_ch, input_ch_time, input_ch_views


def _timed_query_fn(run_network, embed_fn, embeddirs_fn, embedtime_fn, netchunk, discr):
    # render.closure_embedders and render_tnerf._time_discr read embed_fn, embeddirs_fn, embedtime_fn and discr out of this lambda's
    # closure BY NAME: renaming one sends every render to the op path without an error
    return lambda inputs, viewdirs, ts, network_fn: run_network(
        inputs, viewdirs, ts, network_fn, embed_fn=embed_fn, embeddirs_fn=embeddirs_fn, embedtime_fn=embedtime_fn,
        netchunk=netchunk, embd_time_discr=discr)


def _device(device):
    if device is not None:
        return torch.device(device)
    return torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu")


def _set_wgrad_precision(args):
    """args.wgrad_precision (extra, "fp32" or "bf16x3"; absent: the process default, fp32 unless SWNERF_WGRAD_PRECISION says
    otherwise) selects the arithmetic of the grouped weight-gradient GEMMs for this runner's training (swnerf.wgrad.set_precision;
    DESIGN.md 6c).  This is not `do_half_precision`: parameters, activations, the optimizer and every other kernel stay fp32."""
    from . import wgrad
    wgrad.set_precision(_opt(args, 'wgrad_precision', wgrad.DEFAULT_PRECISION))


def _make_optimizer(args, creator, params, adamw=False, **kw):
    """Adam (AdamW with adamw) over `params`: torch.optim's, or with args.optimizer == "fused" (extra, default "torch") the
    multi-tensor HIP step of swnerf.optim - the same arithmetic, state and checkpoints."""
    which = _opt(args, 'optimizer', 'torch')
    if which == 'torch':
        mod = torch.optim
    elif which == 'fused':
        from . import optim as mod
    else:
        raise ValueError(f"swnerf.{creator}: optimizer must be 'torch' or 'fused', got {which!r}")
    return (mod.AdamW if adamw else mod.Adam)(params, **kw)


def create_nerf(args, device=None):
    """nerf/run.py:222-313 (static NeRF: coarse `vallina_NeRF` + fine one when N_importance > 0)."""
    device = _device(device)
    embed_fn, input_ch = get_embedder(args.multires, input_dims=3, i=args.i_embed)
    input_ch_views, embeddirs_fn = 0, None
    if args.use_viewdirs:
        embeddirs_fn, input_ch_views = get_embedder(args.multires_views, input_dims=3, i=args.i_embed)
    output_ch = 5 if args.N_importance > 0 else 4
    skips = [4]
    model = vallina_NeRF(D=args.netdepth, W=args.netwidth, input_ch=input_ch, output_ch=output_ch, skips=skips,
                         input_ch_views=input_ch_views, use_viewdirs=args.use_viewdirs).to(device)
    grad_vars = list(model.parameters())
    model_fine = None
    if args.N_importance > 0:
        model_fine = vallina_NeRF(D=args.netdepth_fine, W=args.netwidth_fine, input_ch=input_ch, output_ch=output_ch,
                                  skips=skips, input_ch_views=input_ch_views, use_viewdirs=args.use_viewdirs).to(device)
        grad_vars += list(model_fine.parameters())
    netchunk = args.netchunk
    network_query_fn = lambda inputs, viewdirs, network_fn: render.run_network(
        inputs, viewdirs, network_fn, embed_fn=embed_fn, embeddirs_fn=embeddirs_fn, netchunk=netchunk)
    _set_wgrad_precision(args)
    optimizer = _make_optimizer(args, "create_nerf", grad_vars, lr=args.lrate, betas=(0.9, 0.999))
    start, _ = reload_latest(args.basedir, args.expname, model, model_fine, optimizer, ft_path=args.ft_path,
                             no_reload=args.no_reload, map_location=device)
    train, test = _render_kwargs(args, network_query_fn, _coarse_fine(args, model, model_fine))
    return train, test, start, grad_vars, optimizer


def _create_dnerf(args, device, encoders, load, reproducible_wgrad=None, creator="create_dnerf"):
    """The D-NeRF pair behind create_dnerf and every level of create_multires.  load(model, model_fine, optimizer) -> start."""
    embed_fn, embedtime_fn, embeddirs_fn, input_ch, input_ch_time, input_ch_views = encoders
    output_ch = 5 if args.N_importance > 0 else 4
    skips = [4]
    make = lambda D, W: NeRF.get_by_name(args.nerf_type, D=D, W=W, input_ch=input_ch, output_ch=output_ch, skips=skips,
                                         input_ch_views=input_ch_views, input_ch_time=input_ch_time,
                                         use_viewdirs=args.use_viewdirs, embed_fn=embed_fn,
                                         zero_canonical=not args.not_zero_canonical).to(device)
    model = make(args.netdepth, args.netwidth)
    grad_vars = list(model.parameters())
    model_fine = None
    if args.use_two_models_for_fine:
        model_fine = make(args.netdepth_fine, args.netwidth_fine)
        grad_vars += list(model_fine.parameters())
    network_query_fn = _timed_query_fn(render_dnerf.run_network, embed_fn, embeddirs_fn, embedtime_fn, args.netchunk,
                                       args.nerf_type != "temporal")
    if reproducible_wgrad is not None:                       # generic.py: weight gradients summed in a fixed order, equal bits every pass
        for net in (model, model_fine):
            if net is not None:
                net.reproducible_wgrad = reproducible_wgrad
    _set_wgrad_precision(args)
    optimizer = _make_optimizer(args, creator, grad_vars, lr=args.lrate, betas=(0.9, 0.999))
    start = load(model, model_fine, optimizer)
    train, test = _render_kwargs(args, network_query_fn, _coarse_fine(args, model, model_fine),
                                 {'use_two_models_for_fine': args.use_two_models_for_fine})
    return train, test, start, grad_vars, optimizer


def _reload(args, device):
    return lambda model, model_fine, optimizer: reload_latest(args.basedir, args.expname, model, model_fine, optimizer, ft_path=args.ft_path,
                                                              no_reload=args.no_reload, map_location=device)[0]


def create_dnerf(args, device=None):
    """d_nerf/run_dnerf.py:238-352 (`create_nerf` of the D-NeRF runner): `NeRF.get_by_name(args.nerf_type, ...)`,
    the time encoder, `use_two_models_for_fine`.  fp32 only: `do_half_precision` (apex amp) is refused."""
    _refuse_half_precision(args, "create_dnerf")
    device = _device(device)
    pos = (args.multires, args.i_embed)
    return _create_dnerf(args, device, _timed_encoders(args, pos, pos, lambda: (args.multires_views, args.i_embed)), _reload(args, device))


def create_tnerf(args, device=None):
    """t_nerf/run_tnerf.py:238-345 (`create_nerf` of the T-NeRF runner): one TNeRF (width 128, skip_layer 4, depth
    args.netdepth), the time encoder at args.multires, N_importance forced to 0.  fp32 only: `do_half_precision` is refused."""
    _refuse_half_precision(args, "create_tnerf")
    device = _device(device)
    pos = (args.multires, args.i_embed)
    embed_fn, embedtime_fn, embeddirs_fn, input_ch, input_ch_time, input_ch_views = _timed_encoders(
        args, pos, pos, lambda: (args.multires_views, args.i_embed))
    model = TNeRF(depth=args.netdepth, in_feat=input_ch, dir_feat=input_ch_views, time_feat=input_ch_time, net_dim=128,
                  skip_layer=4).to(device)
    grad_vars = list(model.parameters())
    network_query_fn = _timed_query_fn(render_tnerf.run_network, embed_fn, embeddirs_fn, embedtime_fn, args.netchunk,
                                       args.nerf_type != "temporal")
    _set_wgrad_precision(args)
    optimizer = _make_optimizer(args, "create_tnerf", grad_vars, lr=args.lrate, betas=(0.9, 0.999))
    start = _reload(args, device)(model, None, optimizer)
    train, test = _render_kwargs(args, network_query_fn, {'N_importance': 0, 'network_fn': model, 'N_samples': args.N_samples})
    return train, test, start, grad_vars, optimizer


def create_fit2d(args, device=None):
    """2d_pos_encoding/main.py:19-24: Model(2 + 4 L, layer_num), AdamW(lr 1e-3), ExponentialLR(gamma 0.95); with
    args.checkpoint_load the model, the optimizer and the starting epoch come from that file (utils.py:15-21, 38-40 - the scheduler
    restarts, as in the reference).  Returns model, optimizer, scheduler, start epoch, metrics."""
    from . import fit2d
    device = _device(device)
    model = fit2d.Model(input_dimension=2 + 4 * args.L, layer_num=args.layer_num).to(device)
    _set_wgrad_precision(args)
    optimizer = _make_optimizer(args, "create_fit2d", model.parameters(), adamw=True, lr=0.001)
    scheduler = torch.optim.lr_scheduler.ExponentialLR(optimizer, gamma=0.95)
    start, metrics = 0, {"MSE": [], "PSNR": []}
    if getattr(args, "checkpoint_load", None):
        start, metrics = fit2d.load_checkpoint(model, optimizer, args)
    return model, optimizer, scheduler, start, metrics


# ---- MultiRes D-NeRF (multires_dnerf/multires_dnerf.py): one DirectTemporalNeRF per Laplacian-pyramid level -------------
MULTIRES_CHANNELS = [(20, 8, 20), (10, 4, 10), (10, 4, 10), (-1, -1, -1)]      # multires_dnerf.py:665, per level


def create_multires(args, device=None):
    """multires_dnerf.py:658-685 with its create_nerf(args, channels, layer) (:242-352): for every level the D-NeRF pair
    with that level's encoders - get_embedder(channels[0], 3, channels[0]) for position, channels[1] for TIME and
    channels[2] for the VIEWS (the reference's order; -1 is the identity encoder) -, one Adam per level, and the level's
    part of the newest MultiRes checkpoint.  -> the five lists (render_kwargs_train_list, render_kwargs_test_list,
    start_list, grad_vars_list, optimizer_list); near / far are left to the caller.  None of the level shapes is a fused
    shape: they run layer by layer on the generic kernels (swnerf/generic.py).  args.reproducible_wgrad (extra, optional,
    default False): the nets' weight gradients add their row slices in a fixed order (swnerf_gemm_tn_ordered) instead of with
    float atomics, so that a backward pass repeats bit for bit - slower on large batches.  fp32 only."""
    _refuse_half_precision(args, "create_multires")
    if not 1 <= args.layer_num <= len(MULTIRES_CHANNELS):
        raise ValueError(f"swnerf.create_multires: layer_num must be 1..{len(MULTIRES_CHANNELS)}, got {args.layer_num}")
    device = _device(device)
    ckpts = find_checkpoints(args.basedir, args.expname, args.ft_path)
    trains, tests, starts, grads, optimizers = [], [], [], [], []
    for layer, (L_pos, L_time, L_views) in enumerate(MULTIRES_CHANNELS[:args.layer_num]):
        def load(model, model_fine, optimizer):
            if len(ckpts) > 0 and not args.no_reload:
                return load_multires(ckpts[-1], layer, model, model_fine, optimizer, map_location=device)
            return 0
        encoders = _timed_encoders(args, (L_pos, L_pos), (L_time, L_time), lambda: (L_views, L_views))
        level = _create_dnerf(args, device, encoders, load, bool(getattr(args, "reproducible_wgrad", False)), "create_multires")
        for out, part in zip((trains, tests, starts, grads, optimizers), level):
            out.append(part)
    return trains, tests, starts, grads, optimizers


def pyramid_hwf(hwf, layer_num):
    """multires_dnerf.py:629-637: [H // 2^l, W // 2^l, focal / 2^l] per level."""
    H, W, focal = hwf
    H, W = int(H), int(W)
    out = []
    for layer in range(layer_num):
        scale = 2 ** layer
        if H // scale <= 0 or W // scale <= 0:
            raise ValueError(f"swnerf.pyramid_hwf: level {layer} of a {H} x {W} image is empty")
        out.append([H // scale, W // scale, focal / scale])
    return out


def get_random_patch_coords(H, W, patch_size, current_iter, n=4000, sigma_factor=4):
    """multires_dnerf.py:500-561: the (y, x) corner of a patch: before iteration n uniform over the central region, from
    then on normal around the centre (sigma = side / sigma_factor), clipped into the image."""
    if H <= patch_size or W <= patch_size:
        return 0, 0
    center_y = (H - patch_size) / 2
    center_x = (W - patch_size) / 2
    if current_iter < n:
        half_patch_area_y = H / 4
        half_patch_area_x = W / 4
        min_y = max(0, int(center_y - half_patch_area_y / 2))
        max_y = min(int(center_y + half_patch_area_y / 2), H - patch_size)
        min_x = max(0, int(center_x - half_patch_area_x / 2))
        max_x = min(int(center_x + half_patch_area_x / 2), W - patch_size)
        y = random.randint(min_y, max_y)
        x = random.randint(min_x, max_x)
    else:
        y = int(torch.normal(mean=center_y, std=H / sigma_factor, size=(1,)).item())
        x = int(torch.normal(mean=center_x, std=W / sigma_factor, size=(1,)).item())
        y = max(0, min(y, H - patch_size))
        x = max(0, min(x, W - patch_size))
    return y, x


def initialize_patches(pyr_hwf, base_patch_size=4, cur_iter=0):
    """multires_dnerf.py:562-585: one (y, x) per level, finest first: drawn at the COARSEST level with `base_patch_size`
    (the reference's train() passes its finest-level patch size, 32, here: kept as it is) and doubled level by level."""
    patch_coords = []
    for layer, (H, W, focal) in enumerate(pyr_hwf[::-1]):
        if layer == 0:
            y, x = get_random_patch_coords(H, W, base_patch_size, cur_iter)
        else:
            prev_y, prev_x = patch_coords[layer - 1]
            y, x = prev_y * 2, prev_x * 2
        patch_coords.append((y, x))
    return patch_coords[::-1]


def multires_train_loss(i, img_i, images, pyr_images, poses, times, pyr_hwf, patch_size_list, render_kwargs_train_list, args,
                        base_patch_size=32, patch_coords=None, batcher=None):
    """The body of the reference's joint iteration (multires_dnerf.py:909-996) up to, and excluding, backward(): per level a
    patch of rays of frame img_i rendered by that level's nets against the same patch of that level of the pyramid
    (mse of rgb, plus mse of rgb0 when present), then the levels' patches reconstructed through the pyramid against the
    patch of the full image, added to the loss once i >= args.global_optimization_epoch.  near / far come with the
    render kwargs.  `patch_coords` (extra, optional) fixes the per-level corners instead of drawing them.
    `batcher` (extra, optional): a swnerf.batching.PatchBatcher over the same images, pyramid, poses and times - every level's rows
    and targets then come from one launch and the whole loss with its gradients from one more (DESIGN.md 6g "Training"); of the
    returned values only `loss` then carries a gradient.
    -> (loss, per_level_losses, global_loss, global_psnr, reconstructed)."""
    if patch_coords is None:
        patch_coords = initialize_patches(pyr_hwf, base_patch_size=base_patch_size, cur_iter=i)
    if batcher is not None:
        from . import batching
        ray_batches, target_patches, full_patch = batcher.batch(img_i, patch_coords, patch_size_list)
        rgbs, rgb0s = [], []
        for rb, render_kwargs_train in zip(ray_batches, render_kwargs_train_list):
            rays_kw = {k: v for k, v in render_kwargs_train.items() if k not in _RENDER_ONLY_KEYS}
            if render_kwargs_train.get('ndc', True):
                raise NotImplementedError("swnerf.runner.multires_train_loss: a PatchBatcher makes no NDC rows (the MultiRes runner is blender-only)")
            if not render_kwargs_train.get('use_viewdirs', False):
                rb = rb[:, :9].contiguous()                              # run_dnerf.py:153-159
            rgb, disp, acc, extras = _render_packed_dnerf(rb, batcher.times_host[int(img_i)], args.chunk, rays_kw)
            rgbs.append(rgb)
            rgb0s.append(extras.get('rgb0'))
        loss, per_level, _, global_loss, global_psnr, reconstructed = batching.multires_loss(
            rgbs, rgb0s, target_patches, full_patch, i >= args.global_optimization_epoch)
        return loss, per_level, global_loss, global_psnr, reconstructed
    pyramid_outputs, per_level = [], []
    loss = 0
    for layer, render_kwargs_train in enumerate(render_kwargs_train_list):
        H_l, W_l, focal_l = pyr_hwf[layer]
        patch_size = patch_size_list[layer]
        y, x = patch_coords[layer]
        target_patch = pyr_images[layer][img_i][y:y + patch_size, x:x + patch_size, :3]
        rays_o, rays_d = get_rays(H_l, W_l, float(focal_l), poses[img_i, :3, :4])
        rays_o = rays_o[y:y + patch_size, x:x + patch_size].reshape(-1, 3)
        rays_d = rays_d[y:y + patch_size, x:x + patch_size].reshape(-1, 3)
        rgb, disp, acc, extras = render_dnerf.render(patch_size, patch_size, focal_l, chunk=args.chunk, rays=(rays_o, rays_d),
                                                     frame_time=times[img_i], retraw=True, **render_kwargs_train)
        ph, pw = target_patch.shape[0], target_patch.shape[1]
        rgb = rgb.reshape(ph, pw, 3)
        img_loss = torch.nn.functional.mse_loss(rgb, target_patch)
        if 'rgb0' in extras:
            loss = loss + torch.nn.functional.mse_loss(extras['rgb0'].reshape(ph, pw, 3), target_patch)
        loss = loss + img_loss
        per_level.append(img_loss)
        pyramid_outputs.append(rgb.unsqueeze(0))
    y, x = patch_coords[0]
    patch_size = patch_size_list[0]
    target = images[img_i][y:y + patch_size, x:x + patch_size, :3]
    reconstructed, global_loss, global_psnr = pyramid.reconstruct_and_compute_loss(pyramid_outputs, target)
    if i >= args.global_optimization_epoch:
        loss = loss + global_loss
    return loss, per_level, global_loss, global_psnr, reconstructed


def render_path_multires(render_poses, render_times, hwf, chunk, render_kwargs_test_list, level_hwf="reference", gt_imgs=None,
                         savedir=None):
    """The test-set / video render of the MultiRes runner (multires_dnerf.py:741-755): every level's frames, then their
    reconstruction.  level_hwf="reference": every level at `hwf`, as the reference does - reconstruct is then the exact
    fp32 sum of the levels; "pyramid": level l at pyramid_hwf(hwf)[l], 1 + 1/4 + 1/16 + ... of one frame's rays, and
    reconstruct upsamples through the pyramid kernels.  With `savedir` the levels' PNGs go to savedir/layer_{l}/estim/
    (render_dnerf.render_path) and the reconstructed frames to savedir/estim/.  gt_imgs: per level, or None.
    -> (frames [N,H,W,3], per_level_frames: list of [N,H_l,W_l,3]), numpy."""
    if level_hwf not in ("reference", "pyramid"):
        raise ValueError(f"swnerf.render_path_multires: level_hwf must be 'reference' or 'pyramid', got {level_hwf!r}")
    n_levels = len(render_kwargs_test_list)
    hwfs = pyramid_hwf(hwf, n_levels) if level_hwf == "pyramid" else [list(hwf)] * n_levels
    per_level = []
    with torch.no_grad():
        for layer, kw in enumerate(render_kwargs_test_list):
            H_l, W_l, focal_l = hwfs[layer]
            rgbs, _ = render_dnerf.render_path(render_poses, render_times, [int(H_l), int(W_l), focal_l], chunk, kw,
                                               gt_imgs=None if gt_imgs is None else gt_imgs[layer],
                                               savedir=None if savedir is None else os.path.join(savedir, f'layer_{layer}'))
            per_level.append(rgbs)
        dev = _device(None)
        frames = pyramid.reconstruct_image_from_pyramid_batch(
            [torch.from_numpy(np.ascontiguousarray(r, dtype=np.float32)).to(dev) for r in per_level]).cpu().numpy()
    if savedir is not None:
        os.makedirs(os.path.join(savedir, "estim"), exist_ok=True)
        for i, f in enumerate(frames):
            write_png(os.path.join(savedir, "estim", '{:03d}.png'.format(i)), to8b(f))
    return frames, per_level


def render_test(render_poses, hwf, K, chunk, render_kwargs, gt_imgs, savedir, render_factor=0, lpips_weights=None, video=False):
    """nerf/run.py:557-596 (`--render_only --render_test`): render.render_path, then calculate_metrics(gt, pred) of every
    frame (pred clipped to [0, 1], data_range = gt.max() - gt.min(), skimage's PSNR and 7x7 SSIM), all frames in one
    batched GPU call.  Writes savedir/metrics.json = {"psnr": [...], "ssim": [...]} (indent 4) and returns (rgbs, metrics).
    lpips_weights (or render_kwargs['lpips_weights']): what metrics.LPIPS takes as `weights`; the file then also holds
    "lpips": [...], the AlexNet LPIPS of every frame as the reference calls it.  Without it there is no such key.  video=True
    also writes the reference's video.mp4, as savedir/video.avi (swnerf.video.mimwrite: Motion-JPEG, quality 90, 30 fps); the
    default leaves savedir with the frames and metrics.json alone."""
    os.makedirs(savedir, exist_ok=True)
    if lpips_weights is None and 'lpips_weights' in render_kwargs:
        lpips_weights = render_kwargs['lpips_weights']
    if 'lpips_weights' in render_kwargs:
        render_kwargs = {k: v for k, v in render_kwargs.items() if k != 'lpips_weights'}
    rgbs, _ = render.render_path(render_poses, hwf, K, chunk, render_kwargs, gt_imgs=gt_imgs, savedir=savedir,
                                 render_factor=render_factor)
    if video:
        mimwrite(os.path.join(savedir, 'video.mp4'), rgbs, fps=30, quality=8)
    gts = gt_imgs.cpu().numpy() if isinstance(gt_imgs, torch.Tensor) else np.asarray(gt_imgs)
    if lpips_weights is None:
        psnr, ssim = metrics.batch_metrics(gts, rgbs)
        out = {"psnr": psnr, "ssim": ssim}
    else:
        psnr, ssim, lp = metrics.batch_metrics(gts, rgbs, lpips_model=metrics.LPIPS("alex", weights=lpips_weights))
        out = {"psnr": psnr, "ssim": ssim, "lpips": lp}
    with open(os.path.join(savedir, "metrics.json"), "w") as f:
        json.dump(out, f, indent=4)
    return rgbs, out


def _read_images_in_dir(imgs_dir):
    """metrics.ipynb read_images_in_dir: every file in sorted order but 000.png (the canonical space), / 255 as float32,
    NCHW"""
    names = sorted(os.listdir(imgs_dir))
    imgs = [np.transpose((read_png(os.path.join(imgs_dir, f)) / 255.).astype(np.float32), (2, 0, 1))
            for f in names if f != "000.png"]
    if not imgs:
        raise ValueError(f"swnerf.runner.evaluate_dir: no frames to score in {imgs_dir}")
    return np.stack(imgs)


def evaluate_dir(files_dir, lpips_weights=None, args=None):
    """The last cell of d_nerf/metrics.ipynb for a D-NeRF or T-NeRF render directory (render_path(..., save_also_gt=True)
    wrote files_dir/estim and files_dir/gt): estim_error of the two batches, written to files_dir/metrics.txt as str(dict).
    -> {'mse', 'psnr', 'ssim'}, and with lpips_weights (or args.lpips_weights; what metrics.LPIPS takes as `weights`) also
    'lpips', the notebook's VGG LPIPS; without them there is no such key."""
    estim = _read_images_in_dir(os.path.join(files_dir, "estim"))
    gt = _read_images_in_dir(os.path.join(files_dir, "gt"))
    if lpips_weights is None:
        lpips_weights = getattr(args, "lpips_weights", None)
    if lpips_weights is None:
        errors = metrics.estim_error(estim, gt)
    else:
        errors = metrics.estim_error(estim, gt, lpips_model=metrics.LPIPS_notebook(weights=lpips_weights))
    with open(os.path.join(files_dir, "metrics.txt"), "w") as f:
        f.write(str(errors))
    return errors


# ---- the extracted mesh from the project's cameras (swnerf.meshrender; DESIGN.md 6b "Mesh rendering") ------------------------
def render_path_mesh(m, render_poses, hwf, K, savedir=None, render_factor=0, shading="headlight", video=False):
    """The mesh twin of render.render_path: the mesh `m` (what mesh.render_views takes) from every pose of render_poses ([N,3,4] or
    [N,4,4]) in one call -> (rgbs [N,H,W,3], disps [N,H,W]) as numpy arrays.  hwf, K and render_factor are render_path's (K = None:
    the focal branch of hwf's focal).  With `savedir` every frame is written as '{:03d}.png' of to8b(rgb), and with video=True also
    savedir/video.avi (swnerf.video.mimwrite, as render_test writes it).  A pixel no face covers is white with disparity 0."""
    from . import meshrender
    H, W, focal = hwf
    H, W, focal = int(H), int(W), float(focal)
    if render_factor != 0:
        H, W, focal = H // render_factor, W // render_factor, focal / render_factor
        if K is not None:
            K = np.asarray(torch.as_tensor(K).cpu(), np.float64).copy()
            K[:2] /= render_factor
    if video and savedir is None:
        raise ValueError("swnerf.runner.render_path_mesh: video=True needs a savedir")
    out = meshrender.render_views(m, H, W, K, render_poses, shading=shading, white_bkgd=True, outputs=("rgb", "disp"), focal=focal)
    rgbs, disps = out["rgb"].cpu().numpy(), out["disp"].cpu().numpy()
    if savedir is not None:
        os.makedirs(savedir, exist_ok=True)
        for i, rgb in enumerate(rgbs):
            write_png(os.path.join(savedir, '{:03d}.png'.format(i)), to8b(rgb))
        if video:
            mimwrite(os.path.join(savedir, 'video.avi'), rgbs, fps=30, quality=8)
    return rgbs, disps


_SPLIT_ROWS = {"train": 0, "val": 1, "test": 2}


def evaluate_mesh(m, dataset, split="train", net_depths=None, savedir=None):
    """A mesh against the data it was extracted from: `m` is rendered from the poses of one split of `dataset` (the dict of
    data.load_dataset: images, poses, hwf, K, i_split) and its silhouette is compared with the alpha channel of the split's frames,
    read where the loaders keep them (device uint8 or float32 RGBA; frames without an alpha channel count as covered everywhere).
    net_depths: optionally the NeRF's depth_map of the same frames [n,H,W] (non-NDC rays: the unit of the mesh's depth), for the
    depth error over the pixels both cover.  -> dict of per-frame lists: frame (the dataset index), iou, depth_mae, depth_rmse,
    intersection, union, mesh_pixels, ref_pixels.  Nothing is written unless `savedir` is given: then savedir/mesh_eval.json holds the
    dict and '{:03d}.png' the headlight render of every frame."""
    from . import meshrender
    if split not in _SPLIT_ROWS:
        raise ValueError(f"swnerf.runner.evaluate_mesh: split must be one of {sorted(_SPLIT_ROWS)}, got {split!r}")
    d = dataset if isinstance(dataset, dict) else _train_data(dataset, False)
    H, W, focal = d['hwf']
    H, W, focal = int(H), int(W), float(focal)
    idx = np.asarray(d['i_split'][_SPLIT_ROWS[split]], dtype=np.int64).reshape(-1)
    images = torch.as_tensor(d['images'])
    if tuple(images.shape[1:3]) != (H, W):
        raise ValueError(f"swnerf.runner.evaluate_mesh: the frames are {tuple(images.shape[1:3])}, hwf says {(H, W)}")
    poses = torch.as_tensor(np.asarray(torch.as_tensor(d['poses']).cpu(), dtype=np.float32))[torch.from_numpy(idx)]
    if net_depths is not None and tuple(net_depths.shape) != (len(idx), H, W):
        raise ValueError(f"swnerf.runner.evaluate_mesh: net_depths must be {(len(idx), H, W)}, got {tuple(net_depths.shape)}")
    outputs = ("acc", "depth") + (("rgb",) if savedir is not None else ())
    out = meshrender.render_views(m, H, W, d.get('K'), poses, shading="headlight", white_bkgd=True, outputs=outputs, focal=focal)
    frames = images.to(out["acc"].device)[torch.from_numpy(idx).to(out["acc"].device)]
    alpha = frames if frames.shape[-1] == 4 else torch.ones((len(idx), H, W), dtype=torch.float32, device=frames.device)
    res = meshrender.compare_views(out, alpha=alpha, depth=net_depths)
    keys = ("iou", "depth_mae", "depth_rmse", "intersection", "union", "mesh_pixels", "ref_pixels")
    report = {"frame": idx.tolist(), **{k: res[k].tolist() for k in keys}}
    if savedir is not None:
        os.makedirs(savedir, exist_ok=True)
        for i, rgb in enumerate(out["rgb"].cpu().numpy()):
            write_png(os.path.join(savedir, '{:03d}.png'.format(i)), to8b(rgb))
        with open(os.path.join(savedir, "mesh_eval.json"), "w") as f:
            json.dump(report, f, indent=4)
    return report


# ---- train() of the two runners (nerf/run.py:598-796, d_nerf/run_dnerf.py:596-820) ---------------------------------------
_RENDER_ONLY_KEYS = ('ndc', 'near', 'far', 'use_viewdirs', 'c2w_staticcam')      # what render() consumes before render_rays


def _train_data(data, with_times):
    """The loaders' tuple (images, poses, render_poses, hwf, i_split[, times]) + (near, far), or a dict with those names
    (and optionally 'K')."""
    if isinstance(data, dict):
        d = dict(data)
    else:
        names = ['images', 'poses', 'render_poses', 'hwf', 'i_split'] + (['times'] if len(data) == 8 else []) + ['near', 'far']
        if len(data) != len(names):
            raise ValueError(f"swnerf.runner.train: data must be (images, poses, render_poses, hwf, i_split[, times], near, far), got {len(data)} entries")
        d = dict(zip(names, data))
    if with_times and d.get('times') is None:
        raise ValueError("swnerf.runner.train_dnerf: data carries no frame times")
    H, W, focal = d['hwf']
    d['hwf'] = [int(H), int(W), float(focal)]
    if d.get('K') is None:                                                       # nerf/run.py:518-523
        d['K'] = np.array([[float(focal), 0, 0.5 * int(W)], [0, float(focal), 0.5 * int(H)], [0, 0, 1]])
    return d


def _gt_rgb(images, idx, white_bkgd):
    """images[idx] as the reference holds them after loading: float32 RGB (bytes / 255., RGBA composited on white or cut)."""
    im = torch.as_tensor(images)[torch.as_tensor(np.asarray(idx, dtype=np.int64))].cpu().numpy()
    if im.dtype == np.uint8:
        im = (im / 255.).astype(np.float32)
    if im.shape[-1] == 4:
        im = im[..., :3] * im[..., -1:] + (1. - im[..., -1:]) if white_bkgd else im[..., :3]
    return im


def _render_poses_and_times(d, device, timed):
    """what the video branch renders: data['render_poses'] on the device and, for the runners with frame times, data['render_times']
    - linspace(0, 1, len(render_poses)) when the data carries none (the tuple form)"""
    poses = torch.as_tensor(np.asarray(torch.as_tensor(d['render_poses']).cpu(), dtype=np.float32)).to(device)
    if not timed:
        return poses, None
    times = d.get('render_times')
    if times is None:
        times = np.linspace(0., 1., poses.shape[0], dtype=np.float32)
    return poses, np.asarray(torch.as_tensor(times).cpu(), dtype=np.float32)


def _write_spiral(args, i, rgbs, disps, hooks):
    """{expname}_spiral_{i:06d}_rgb.avi and ..._disp.avi (nerf/run.py:726-733; the reference's .mp4): to8b(rgbs) and
    to8b(disps / np.max(disps)), both conversions on the device"""
    moviebase = os.path.join(args.basedir, args.expname, '{}_spiral_{:06d}_'.format(args.expname, i))
    os.makedirs(os.path.dirname(moviebase), exist_ok=True)
    if hooks and 'on_video' in hooks:
        hooks['on_video'](i, rgbs, disps)
    video.write_video(moviebase + 'rgb.avi', np.asarray(rgbs, dtype=np.float32), fps=30, quality=90)
    video.write_video(moviebase + 'disp.avi', np.asarray(disps, dtype=np.float32)[..., None], fps=30, quality=90, divisor=float(np.max(disps)))
    print('Done, saving', rgbs.shape, disps.shape)


class _Record:
    """Per-step loss / psnr / lr.  The losses stay on the device until `flush` (one transfer per i_print steps, no sync per step)."""

    def __init__(self):
        self.steps, self._pending = [], []

    def add(self, i, loss, img_loss, lr):
        self._pending.append((i, loss.detach(), img_loss.detach(), lr))

    def flush(self):
        if self._pending:
            from .embedder import mse2psnr
            loss = torch.stack([p[1] for p in self._pending]).reshape(-1)
            mse = torch.stack([p[2] for p in self._pending]).reshape(-1)
            loss, psnr = loss.cpu().tolist(), mse2psnr(mse).cpu().tolist()
            for (i, _, _, lr), l, p in zip(self._pending, loss, psnr):
                self.steps.append({'step': i, 'loss': l, 'psnr': p, 'lr': lr})
            self._pending = []
        return self.steps


def _opt(args, name, default):
    return getattr(args, name, default)


def _train_common(args, d, device, sampler, loss_fn, create, timed, images=None, hwf=None, seed=None):
    """create: the runner's creator (create_nerf / create_dnerf / create_tnerf), or a callable that hands over nets that exist
    (a level of create_multires); timed: the D-NeRF and T-NeRF runners build rays from hwf's focal and carry the frame time in
    column 8.  images / hwf / seed: what the batcher draws from instead of d['images'], d['hwf'] and args.seed (a pyramid level).
    -> what the loop and its four callables work on."""
    from . import batching
    if sampler not in ("device", "numpy"):
        raise ValueError(f"swnerf.runner.train: sampler must be 'device' or 'numpy', got {sampler!r}")
    device = _device(device)
    train_kw, test_kw, start, grad_vars, optimizer = create(args, device=device)
    bds = {'near': d['near'], 'far': d['far']}
    train_kw.update(bds)
    test_kw.update(bds)
    i_train = np.asarray(d['i_split'][0]).reshape(-1)
    batcher = batching.RayBatcher(d['images'] if images is None else images, d['poses'],
                                  (d['hwf'] if hwf is None else hwf) if timed else d['K'],       # the runners' own get_rays calls: focal there, K here
                                  i_train, d['near'], d['far'], times=d.get('times') if timed else None,
                                  ndc=train_kw.get('ndc', True), use_viewdirs=train_kw['use_viewdirs'], white_bkgd=args.white_bkgd,
                                  seed=_opt(args, 'seed', 0) if seed is None else seed, device=device)
    rays_kw = {k: v for k, v in train_kw.items() if k not in _RENDER_ONLY_KEYS}
    return SimpleNamespace(device=device, train_kw=train_kw, test_kw=test_kw, start=start, optimizer=optimizer, i_train=i_train,
                           batcher=batcher, rays_kw=rays_kw, loss_fn=loss_fn or batching.photometric_loss, sampler=sampler,
                           chunk=_opt(args, 'chunk', 1024 * 32))


def _image_draw(args, batcher, i, img_i, sampler, N_rand):
    """One `no_batching` batch of image img_i at iteration i (nerf/run.py:659-681)."""
    from . import batching
    crop = batching.precrop_crop(batcher.H, batcher.W, args.precrop_frac) if i < _opt(args, 'precrop_iters', 0) else None
    ids = None
    if sampler == "numpy":
        n_px = batcher.H * batcher.W if crop is None else crop[2] * crop[3]
        ids = np.random.choice(n_px, size=[N_rand], replace=False)
    return batcher.image_batch(img_i, N_rand, i, crop=crop, ids=ids, return_ids=True)


def _step_tail(args, i, global_step, optimizer, record, loss, img_loss, train_kw, hooks):
    """lr decay, checkpoint, print - the part of an iteration both runners share (nerf/run.py:702-753)."""
    from .batching import lr_at
    new_lrate = lr_at(args.lrate, args.lrate_decay, global_step)
    for param_group in optimizer.param_groups:
        param_group['lr'] = new_lrate
    record.add(i, loss, img_loss, new_lrate)
    if i % _opt(args, 'i_weights', 10000) == 0:
        from .checkpoint import save_checkpoint
        path = save_checkpoint(args.basedir, args.expname, i, global_step, train_kw['network_fn'], train_kw.get('network_fine'), optimizer)
        print('Saved checkpoints at', path)
    if i % _opt(args, 'i_print', 100) == 0:
        last = record.flush()[-1]
        print(f"[TRAIN] Iter: {i} Loss: {last['loss']}  PSNR: {last['psnr']}")
    if hooks and 'on_step' in hooks:
        hooks['on_step'](i, optimizer)


def _render_packed_dnerf(rb, t_host, chunk, rays_kw, **more):
    """render_dnerf's rays pass on a PACKED batch of one frame time.  The time is known here as the kernels read it (float32): no
    device->host read per chunk (render_dnerf._TIME_HINT).  -> (rgb, disp, acc, extras)"""
    token = render_dnerf._TIME_HINT.set((rb.untyped_storage().data_ptr(), float(t_host)))
    try:
        all_ret = render_dnerf.batchify_rays(rb, chunk, retraw=True, **more, **rays_kw)
    finally:
        render_dnerf._TIME_HINT.reset(token)
    return render.image_outputs(all_ret, (rb.shape[0], 3))


def _curriculum_draw(args, s):
    """draw(i) of the runners with frame times: one image among the first frames the time curriculum admits at iteration i
    (run_dnerf.py:650-655), then a no_batching batch of it."""
    from .batching import time_curriculum_max

    def draw(i):
        max_sample = time_curriculum_max(i, _opt(args, 'precrop_iters_time', 0), len(s.i_train))
        img_i = np.random.choice(s.i_train if max_sample is None else s.i_train[:max_sample])
        return (img_i,) + _image_draw(args, s.batcher, i, img_i, s.sampler, args.N_rand)
    return draw


def _train_loop(args, d, s, last_iter, hooks, draw, render_batch, render_testset, extra_loss=None, first_iter=None, step_tail=None,
                advance=True, render_video=None, i_video=50000):
    """Iterations s.start + 1 .. last_iter of the three runners (first_iter .. last_iter when given; step_tail: what follows
    optimizer.step() instead of _step_tail; advance=False: global_step stays at s.start; render_testset None: no test-set render -
    the private phase of train_multires).  What differs between the runners comes as callables:
    draw(i) -> (img_i, ray_batch, target, ids); render_batch(i, img_i, ray_batch) -> (rgb, rgb0 for loss_fn, state);
    extra_loss(state) -> a term added to loss_fn's loss before backward, or None for none; render_testset(i_test, poses_test, gt_imgs,
    savedir) under no_grad every i_testset iterations; render_video(i) -> (rgbs, disps) of the render poses under no_grad every
    args.i_video (default i_video) iterations, written as two .avi files (_write_spiral); None: no video.  -> the per-step record."""
    hooks = hooks or {}
    i_test = np.asarray(d['i_split'][2]).reshape(-1) if len(d['i_split']) > 2 else np.zeros(0, np.int64)
    global_step = s.start
    record = _Record()
    step_tail = step_tail or _step_tail
    for i in range(s.start + 1 if first_iter is None else first_iter, last_iter + 1):
        img_i, ray_batch, target_s, ids = draw(i)
        if 'on_batch' in hooks:
            hooks['on_batch'](i, img_i, ray_batch, target_s, ids)
        rgb, rgb0, state = render_batch(i, img_i, ray_batch)
        s.optimizer.zero_grad()
        loss, img_loss, img_loss0 = s.loss_fn(rgb, target_s, rgb0)
        if extra_loss is not None:
            loss = loss + extra_loss(state)
        loss.backward()
        s.optimizer.step()
        step_tail(args, i, global_step, s.optimizer, record, loss, img_loss, s.train_kw, hooks)
        if render_video is not None and i % _opt(args, 'i_video', i_video) == 0 and i > 0:
            with torch.no_grad():
                rgbs, disps = render_video(i)
            _write_spiral(args, i, rgbs, disps, hooks)
        if render_testset is not None and i % _opt(args, 'i_testset', 50000) == 0 and i > 0 and i_test.size:
            testsavedir = os.path.join(args.basedir, args.expname, 'testset_{:06d}'.format(i))
            poses_test = torch.as_tensor(np.asarray(d['poses'], dtype=np.float32)[i_test]).to(s.device)
            with torch.no_grad():
                render_testset(i_test, poses_test, _gt_rgb(d['images'], i_test, args.white_bkgd), testsavedir)
            print('Saved test set')
        global_step += int(advance)
    return record.flush()


def train(args, data, device=None, sampler="device", loss_fn=None, hooks=None):
    """The training loop of nerf/run.py:598-796 from `create_nerf` on: a batch from swnerf.batching.RayBatcher (use_batching
    over all training rays, or no_batching from one image with the precrop window), the render of the PACKED batch
    (render.batchify_rays + image_outputs, retraw=True), loss, backward, Adam, the lr decay, a checkpoint every i_weights, a
    print every i_print, render_test every i_testset, the spiral of data['render_poses'] every i_video (default 50000) as
    {expname}_spiral_{i:06d}_rgb.avi / _disp.avi (swnerf.video: Motion-JPEG where the reference writes .mp4).  TensorBoard and the
    config file are not written.

    args: the reference's option names (N_rand, no_batching, precrop_iters, precrop_frac, chunk, lrate, lrate_decay, i_print,
    i_weights, i_testset, ...; N_iters - extra, default 200000 - is the last iteration; seed - extra, default 0 - keys the
    device sampler).  data: (images, poses, render_poses, hwf, i_split, near, far) or a dict with those names (+ 'K').
    sampler: "device" draws the pixels on the GPU with the keyed permutation; "numpy" draws np.random.choice(..., replace=False)
    on the host as the reference does and hands the indices to the same kernel - the reference's random stream and rays.
    loss_fn(rgb, target, rgb0) -> (loss, img_loss, img_loss0): default batching.photometric_loss.
    hooks: {'on_batch': f(i, img_i, ray_batch, target, ids), 'on_step': f(i, optimizer), 'on_video': f(i, rgbs, disps) with the
    float frames before they are encoded}.
    -> the per-step record: a list of {'step', 'loss', 'psnr', 'lr'}."""
    d = _train_data(data, False)
    s = _train_common(args, d, device, sampler, loss_fn, create_nerf, False)

    def draw(i):
        if not args.no_batching:
            return (None,) + s.batcher.global_batch(args.N_rand, return_ids=True)
        img_i = np.random.choice(s.i_train)
        return (img_i,) + _image_draw(args, s.batcher, i, img_i, s.sampler, args.N_rand)

    def render_batch(i, img_i, ray_batch):
        all_ret = render.batchify_rays(ray_batch, s.chunk, retraw=True, **s.rays_kw)
        rgb, disp, acc, extras = render.image_outputs(all_ret, (ray_batch.shape[0], 3))
        return rgb, extras.get('rgb0'), None

    def render_testset(i_test, poses_test, gt_imgs, savedir):
        render_test(poses_test, d['hwf'], d['K'], s.chunk, s.test_kw, gt_imgs, savedir)

    def render_video(i):
        return render.render_path(_render_poses_and_times(d, s.device, False)[0], d['hwf'], d['K'], s.chunk, s.test_kw)
    return _train_loop(args, d, s, _opt(args, 'N_iters', 200000), hooks, draw, render_batch, render_testset, render_video=render_video)


def train_dnerf(args, data, device=None, sampler="device", loss_fn=None, hooks=None):
    """The training loop of d_nerf/run_dnerf.py:596-820 from `create_nerf` on; as `train`, plus the time curriculum
    precrop_iters_time (:650-655), the frame time of the drawn image in column 8 of the batch (read from the device table by the
    batch kernel) and, with add_tv_loss, the TV loss of :690-725: a second render of the SAME rays on extras['z_vals'].detach()
    at a random time between the frame and its previous / next one.  use_batching raises NotImplementedError, as the reference.
    Every i_video iterations (default 40000) the render poses at data['render_times'] (a dict's entry; linspace(0, 1, N) without
    one) go to frames_{expname}_spiral_{i:06d}_time/ and to {expname}_spiral_{i:06d}_rgb.avi / _disp.avi (run_dnerf.py:820-829).
    data: (images, poses, render_poses, hwf, i_split, times, near, far) or a dict.  args.N_iter is the last iteration.
    hooks: those of `train`, and 'on_tv': f(i, which, ray_batch_other, z_vals) before each prev / next render."""
    d = _train_data(data, True)
    if not args.no_batching:
        raise NotImplementedError("Time not implemented")                        # run_dnerf.py:634
    s = _train_common(args, d, device, sampler, loss_fn, create_dnerf, True)
    return _dnerf_loop(args, d, s, _opt(args, 'N_iter', _opt(args, 'N_iters', 200000)), hooks)


def _spiral_frames_dir(args, i):
    return os.path.join(args.basedir, args.expname, 'frames_{}_spiral_{:06d}_time/'.format(args.expname, i))


def _dnerf_loop(args, d, s, last_iter, hooks, testset=True, **loop_kw):
    """The D-NeRF iterations on what _train_common prepared: train_dnerf, and each level of train_multires' private phase
    (testset=False: no test-set render and no video; loop_kw: _train_loop's first_iter, step_tail, advance)."""
    times = s.batcher.times_host
    add_tv = bool(_opt(args, 'add_tv_loss', False))

    def render_packed(rb, t_host, **more):
        return _render_packed_dnerf(rb, t_host, s.chunk, s.rays_kw, **more)

    def render_batch(i, img_i, ray_batch):
        frame_time = times[img_i]
        rgb, disp, acc, extras = render_packed(ray_batch, frame_time)
        others = []
        if add_tv:
            frame_time_prev = times[img_i - 1] if img_i > 0 else None
            frame_time_next = times[img_i + 1] if img_i < times.shape[0] - 1 else None
            if frame_time_prev is not None and frame_time_next is not None:
                if np.random.rand() > .5:
                    frame_time_prev = None
                else:
                    frame_time_next = None
            for which, other in (('prev', frame_time_prev), ('next', frame_time_next)):
                if other is None:
                    continue
                u = np.float32(torch.rand(1)[0].item())
                rand_time = other + (frame_time - other) * u if which == 'prev' else frame_time + (other - frame_time) * u
                rb_other = s.batcher.with_time(ray_batch, float(rand_time))
                z = extras['z_vals'].detach()
                if hooks and 'on_tv' in hooks:
                    hooks['on_tv'](i, which, rb_other, z)
                others.append(render_packed(rb_other, np.float32(rand_time), z_vals=z)[3])
        return rgb, extras.get('rgb0'), (extras, others)

    def tv_loss(state):
        extras, others = state
        tv = 0
        for ex in others:
            tv = tv + ((extras['position_delta'] - ex['position_delta']).pow(2)).sum()
            if 'position_delta_0' in extras:
                tv = tv + ((extras['position_delta_0'] - ex['position_delta_0']).pow(2)).sum()
        return tv * args.tv_loss_weight

    def render_testset(i_test, poses_test, gt_imgs, savedir):
        render_dnerf.render_path(poses_test, torch.as_tensor(times[i_test]).to(s.device), d['hwf'], s.chunk, s.test_kw,
                                 gt_imgs=gt_imgs, savedir=savedir)

    def render_video(i):
        poses, render_times = _render_poses_and_times(d, s.device, True)
        return render_dnerf.render_path(poses, torch.as_tensor(render_times).to(s.device), d['hwf'], s.chunk, s.test_kw,
                                        savedir=_spiral_frames_dir(args, i))
    return _train_loop(args, d, s, last_iter, hooks, _curriculum_draw(args, s), render_batch, render_testset if testset else None,
                       tv_loss if add_tv else None, render_video=render_video if testset else None, i_video=40000, **loop_kw)


def train_tnerf(args, data, device=None, sampler="device", loss_fn=None, hooks=None):
    """The training loop of t_nerf/run_tnerf.py:596-800 from `create_nerf` on; as `train_dnerf` without the TV loss: the time
    curriculum precrop_iters_time (:646-651), a 12-column batch with the drawn image's frame time in column 8 (from the batcher's
    device table), render_tnerf.batchify_rays(..., retraw=True, fused_train=...), the single-net loss (rgb0 is None), Adam and
    the lr decay, a checkpoint every i_weights (network_fine None), render_tnerf.render_path every i_testset, the spiral frames and
    the two .avi files of `train_dnerf` every i_video (default 40000; run_tnerf.py:775-784).
    args.N_iter is the last iteration; args.fused_train (extra, default True) = False keeps loss.backward() on the op path.
    use_batching raises NotImplementedError: the reference's branch (:631-642) builds rays without a frame time and cannot run.
    data: (images, poses, render_poses, hwf, i_split, times, near, far) or a dict.  hooks: those of `train`."""
    d = _train_data(data, True)
    if not args.no_batching:
        raise NotImplementedError("swnerf.runner.train_tnerf: use_batching is not built - the reference's branch (run_tnerf.py:631-642) "
                                  "draws rays that carry no frame time and cannot run; pass no_batching=True")
    s = _train_common(args, d, device, sampler, loss_fn, create_tnerf, True)
    times = s.batcher.times_host
    fused = bool(_opt(args, 'fused_train', True))

    def render_batch(i, img_i, ray_batch):
        all_ret = render_tnerf.batchify_rays(ray_batch, s.chunk, retraw=True, fused_train=fused, **s.rays_kw)
        return render.image_outputs(all_ret, (ray_batch.shape[0], 3))[0], None, None

    def render_testset(i_test, poses_test, gt_imgs, savedir):
        render_tnerf.render_path(poses_test, [float(t) for t in times[i_test]], d['hwf'], s.chunk, s.test_kw, gt_imgs=gt_imgs, savedir=savedir)

    def render_video(i):
        poses, render_times = _render_poses_and_times(d, s.device, True)
        return render_tnerf.render_path(poses, [float(t) for t in render_times], d['hwf'], s.chunk, s.test_kw, savedir=_spiral_frames_dir(args, i))
    return _train_loop(args, d, s, _opt(args, 'N_iter', _opt(args, 'N_iters', 200000)), hooks, _curriculum_draw(args, s), render_batch,
                       render_testset, render_video=render_video, i_video=40000)


# ---- train() of the MultiRes runner (multires_dnerf/multires_dnerf.py:612-1068) -----------------------------------------------
MULTIRES_BASE_PATCH = 32                                                         # multires_dnerf.py:726


def multires_patch_sizes(layer_num, base_patch_size=MULTIRES_BASE_PATCH):
    """multires_dnerf.py:726-732: [base // 2^l] per level."""
    return [base_patch_size // (2 ** layer) for layer in range(layer_num)]


def _multires_draw(sampler, seed, i, pyr_hwf, i_train):
    """(patch_coords, img_i) of joint iteration i.  "numpy": initialize_patches (random.randint below iteration 4000, torch.normal
    from it on), THEN np.random.choice(i_train) - the reference's streams in the reference's order (multires_dnerf.py:909-914).
    "device": both from batching.batch_key(seed, i, 2) on the host - two scalars, so no launch and no sync: the corner from words
    0..3 (batching.patch_corners), the frame from word 4."""
    if sampler == "numpy":
        patch_coords = initialize_patches(pyr_hwf, base_patch_size=MULTIRES_BASE_PATCH, cur_iter=i)
        return patch_coords, np.random.choice(i_train)
    from . import batching
    key = batching.batch_key(seed, i, 2)
    patch_coords = batching.patch_corners(key, pyr_hwf, base_patch_size=MULTIRES_BASE_PATCH, cur_iter=i)
    return patch_coords, i_train[batching.key_randint(key, 4, 0, len(i_train) - 1)]


def train_multires(args, data, device=None, sampler="device", hooks=None, private_target="reference"):
    """The training loop of multires_dnerf/multires_dnerf.py:612-1068 from its `create_nerf` calls on (`create_multires`).

    Setup: the frames as float32 RGB (RGBA composited on white with white_bkgd, else cut), their Laplacian pyramid of
    args.layer_num levels, pyramid_hwf, patch sizes [32 // 2^l].
    Private phase (:761-904), for the levels from the coarsest to the finest: iterations 0 .. global_optimization_epoch - 1 of
    the D-NeRF step of `train_dnerf` (`_dnerf_loop`: time curriculum, precrop, TV loss) on that level's nets, rays from
    pyramid_hwf[l] through a RayBatcher of the level.  As in the reference the learning rate is that of the level's starting
    global_step throughout (its counter does not advance in this phase), a MultiRes checkpoint {i:06d}.tar is written when
    i % i_weights == 0 (i = 0 included) and a line goes to log.txt when i % i_print == 0.  A resumed run repeats this phase.
    private_target="reference": the target of level l is what the reference reads, images[img_i] indexed with LEVEL coordinates -
    the top-left H_l x W_l window of the full-resolution frame, not the level of the pyramid.  "pyramid": pyr_images[l].
    Joint phase (:905-1068), iterations start_list[0] + 1 .. args.N_iter: the patch corners and one frame (`sampler`), every
    level's patch rendered by its nets, the fused loss (`multires_train_loss` with a PatchBatcher: two launches for data, loss and
    gradients), one backward(), every optimizer's step() and zero_grad(), each level's learning rate from its own step counter,
    `save_multires` every i_weights, `render_path_multires` of the test poses (every level at hwf, as the reference; no gt) every
    i_testset, lines in log.txt every i_print; every i_video iterations (default 40000) 120 frames of the first render pose at
    times linspace(0, 1, 120), every level at hwf, reconstructed and written as {expname}_reconstructed_{i:06d}_rgb.avi
    (multires_dnerf.py:1027-1045; the levels' frames go to frames_layer_{l}_{i:06d}_time/).
    Not written: TensorBoard, the i_img panels, args.txt / config.txt; do_half_precision is refused.

    args: the reference's option names (layer_num, global_optimization_epoch, N_iter, N_rand, precrop_*, add_tv_loss, lrate,
    lrate_decay, i_print, i_weights, i_testset, ...; seed - extra, default 0; optimizer - extra, "torch" or "fused").
    data: (images, poses, render_poses, hwf, i_split, times, near, far) or a dict.  sampler: "numpy" consumes random, torch.normal
    and np.random as the reference does; "device" keys every draw by (seed, iteration).
    hooks: those of `train_dnerf` in the private phase (on_step gets the level's optimizer), and 'on_joint':
    f(i, img_i, patch_coords, loss) after each joint step.
    -> {'private': [per-step record of each level, finest first], 'joint': [{'step', 'loss', 'global_loss', 'levels'}]}."""
    from . import batching
    if private_target not in ("reference", "pyramid"):
        raise ValueError(f"swnerf.runner.train_multires: private_target must be 'reference' or 'pyramid', got {private_target!r}")
    if sampler not in ("device", "numpy"):
        raise ValueError(f"swnerf.runner.train_multires: sampler must be 'device' or 'numpy', got {sampler!r}")
    d = _train_data(data, True)
    device = _device(device)
    hooks = hooks or {}
    n_levels = args.layer_num
    n_all = int(torch.as_tensor(d['images']).shape[0])
    images = torch.from_numpy(np.ascontiguousarray(_gt_rgb(d['images'], np.arange(n_all), args.white_bkgd), dtype=np.float32)).to(device)
    pyr_images = pyramid.generate_laplacian_pyramid_batch(images, levels=n_levels)
    pyr_hwf = pyramid_hwf(d['hwf'], n_levels)
    patch_size_list = multires_patch_sizes(n_levels)
    trains, tests, start_list, grad_vars_list, optimizers = create_multires(args, device=device)
    nets = [kw['network_fn'] for kw in trains]
    fines = [kw.get('network_fine') for kw in trains]
    i_train = np.asarray(d['i_split'][0]).reshape(-1)
    seed = _opt(args, 'seed', 0)
    i_print, i_weights = _opt(args, 'i_print', 100), _opt(args, 'i_weights', 10000)
    os.makedirs(os.path.join(args.basedir, args.expname), exist_ok=True)
    log = os.path.join(args.basedir, args.expname, 'log.txt')

    def save(i):
        print('Saved checkpoints at', save_multires(args.basedir, args.expname, i, i, nets, fines, optimizers))

    def write_log(lines):
        with open(log, 'a') as f:
            f.write(''.join(line + '\n' for line in lines))

    def private_tail(args, i, global_step, optimizer, record, loss, img_loss, train_kw, hooks):
        new_lrate = batching.lr_at(args.lrate, args.lrate_decay, global_step)
        for param_group in optimizer.param_groups:
            param_group['lr'] = new_lrate
        record.add(i, loss, img_loss, new_lrate)
        if i % i_weights == 0:
            save(i)
        if i % i_print == 0:
            last = record.flush()[-1]
            write_log([f"[TRAIN] Iter: {i} Loss_fine: {last['loss']} PSNR: {last['psnr']}"])
        if hooks and 'on_step' in hooks:
            hooks['on_step'](i, optimizer)

    # the private phase
    private = [None] * n_levels
    for model_idx in reversed(range(n_levels)):
        H_l, W_l, focal_l = pyr_hwf[model_idx]
        level_images = pyr_images[model_idx] if private_target == "pyramid" else images[:, :H_l, :W_l]
        level = (trains[model_idx], tests[model_idx], start_list[model_idx], grad_vars_list[model_idx], optimizers[model_idx])
        s = _train_common(args, d, device, sampler, None, lambda args, device: level, True, images=level_images,
                          hwf=[H_l, W_l, focal_l], seed=batching.mix64(int(seed) + model_idx + 1))
        private[model_idx] = _dnerf_loop(args, d, s, args.global_optimization_epoch - 1, hooks, testset=False, first_iter=0,
                                         step_tail=private_tail, advance=False)

    # the joint phase
    batcher = batching.PatchBatcher(images, pyr_images, d['poses'], d['times'], pyr_hwf, d['near'], d['far'], device=device)
    poses_dev = torch.as_tensor(np.asarray(d['poses'], dtype=np.float32)).to(device)
    i_test = np.asarray(d['i_split'][2]).reshape(-1) if len(d['i_split']) > 2 else np.zeros(0, np.int64)
    global_steps = list(start_list)
    for optimizer in optimizers:
        optimizer.zero_grad()                                                    # (the reference does it per level inside the iteration)
    joint, pending = [], []
    for i in range(start_list[0] + 1, args.N_iter + 1):
        patch_coords, img_i = _multires_draw(sampler, seed, i, pyr_hwf, i_train)
        loss, per_level, global_loss, global_psnr, _ = multires_train_loss(
            i, img_i, images, pyr_images, poses_dev, batcher.times, pyr_hwf, patch_size_list, trains, args,
            base_patch_size=MULTIRES_BASE_PATCH, patch_coords=patch_coords, batcher=batcher)
        for layer, optimizer in enumerate(optimizers):
            new_lrate = batching.lr_at(args.lrate, args.lrate_decay, global_steps[layer])
            for param_group in optimizer.param_groups:
                param_group['lr'] = new_lrate
            global_steps[layer] += 1
        loss.backward()
        for optimizer in optimizers:
            optimizer.step()
            optimizer.zero_grad()
        pending.append((i, loss.detach(), global_loss, torch.stack(per_level)))
        if 'on_joint' in hooks:
            hooks['on_joint'](i, img_i, patch_coords, loss)
        if i % i_weights == 0:
            save(i)
        if i % i_print == 0 or i == args.N_iter:                                 # the losses leave the device here, not per step
            for step, l, g, levels in pending:
                joint.append({'step': step, 'loss': float(l), 'global_loss': float(g), 'levels': levels.tolist()})
            pending = []
        if i % i_print == 0:
            last = joint[-1]
            y, x = patch_coords[0]
            lines = [f"[TRAIN] Layer: {layer} Iter: {i} Loss_fine: {m:.6f} PSNR: {-10. * np.log10(m) if m > 0 else float('inf'):.2f}"
                     for layer, m in enumerate(last['levels'])]
            lines.append(f"[GLOBAL OPT] Iter: {i} Global Loss: {last['global_loss']:.6f} Global PSNR: {float(global_psnr):.2f}, Coords:{(y, x)}")
            write_log(lines)
            print(lines[-1])
        if i % _opt(args, 'i_testset', 50000) == 0 and i_test.size:
            testsavedir = os.path.join(args.basedir, args.expname, 'testset_{:06d}'.format(i))
            with torch.no_grad():
                render_path_multires(poses_dev[i_test], batcher.times[i_test], d['hwf'], _opt(args, 'chunk', 1024 * 32), tests,
                                     level_hwf="reference", savedir=testsavedir)
            print('Saved test set')
        if i % _opt(args, 'i_video', 40000) == 0:
            n = 120
            pose0 = _render_poses_and_times(d, device, False)[0][:1].expand(n, -1, -1)
            per_level = []
            with torch.no_grad():
                for layer, kw in enumerate(tests):
                    rgbs, _ = render_dnerf.render_path(pose0, torch.linspace(0, 1, n).to(device), d['hwf'], _opt(args, 'chunk', 1024 * 32), kw,
                                                       savedir=os.path.join(args.basedir, args.expname, f'frames_layer_{layer}_{i:06d}_time/'))
                    per_level.append(torch.from_numpy(np.ascontiguousarray(rgbs, dtype=np.float32)).to(device))
                frames = pyramid.reconstruct_image_from_pyramid_batch(per_level)
            video.write_video(os.path.join(args.basedir, args.expname, f'{args.expname}_reconstructed_{i:06d}_rgb.avi'), frames, fps=30, quality=90)
            print('Done, saving reconstructed video')
    return {'private': private, 'joint': joint}
