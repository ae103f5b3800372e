"""Counterparts of the render functions of the reference's T-NeRF runner (t_nerf/run_tnerf.py:27-210, 395-500): batchify,
run_network, batchify_rays, render, render_path and render_rays with the reference's parameter lists.

render_rays takes the fused T-NeRF pass (csrc/tnerf_kernels.hip: one wave per ray, the 8 x 128 ELU net in registers,
compositing in the same kernel) when `tnerf_plan` holds: no grad, a GPU TNeRF of depth 8 / width 128 / skip 4, the
closure's standard encoders with matching sizes, and embd_time_discr.  It keeps run_network's one-time-per-batch assertion.
Under grad with `fused_train=True` (opt-in) and 2 <= S <= 256 it takes the fused training pass instead (train_pass.py kind "tnerf",
csrc/tnerf_train_kernels.hip: the same forward that also saves activations, a one-wave-per-ray backward, TN GEMMs for dW).
Otherwise it takes the differentiable op path: the HIP sampling op,
`network_query_fn` (embedders + TNeRF.forward on the generic GEMMs with ELU) and the raw2outputs op with its backward.
The fused pass does not go through batchify, so it renders any ray count; on the op path, as in the reference, a sample
count that netchunk does not divide makes batchify's torch.cat fail ("Sizes of tensors must match")."""
import contextlib
import contextvars
import inspect
import os

import numpy as np
import torch

from . import _lib
from .embedder import to8b, EmbedFn
from .png import write_png
from .ray import get_rays, ndc_rays, raw2outputs
from .render import closure_embedders, wants_grad, sample_coarse, pass_args, result_dict, batchify_rays_with, image_outputs
from .train_pass import fused_train_pass, TRAIN_FUSED_MAX_SAMPLES
from .model import TNeRF

DEBUG = False

# The opt-in to the fused training pass.  render_rays keeps the reference's parameter list (tests pin it), so the switch travels
# beside it: a context variable (per thread / task, restored on exit), set by `with fused_train():` or by batchify_rays' keyword.
_FUSED_TRAIN = contextvars.ContextVar("swnerf_tnerf_fused_train", default=False)


@contextlib.contextmanager
def fused_train(on=True):
    """with fused_train(): render_rays calls under grad take the fused T-NeRF training pass where it applies (default: op path)."""
    tok = _FUSED_TRAIN.set(bool(on))
    try:
        yield
    finally:
        _FUSED_TRAIN.reset(tok)


def batchify(fn, chunk):
    """run_tnerf.py:27-45."""
    if chunk is None:
        return fn

    def ret(inputs_pos, viewdirs, dyn_t):
        out_list = []
        for i in range(0, inputs_pos.shape[0], chunk):
            out_list += [fn(inputs_pos[i:i + chunk], viewdirs[i:i + chunk], dyn_t[i:i + chunk])]
        return torch.cat(out_list, 0)
    return ret


def run_network(inputs, viewdirs, frame_time, fn, embed_fn, embeddirs_fn, embedtime_fn, netchunk=1024 * 64,
                embd_time_discr=True):
    """run_tnerf.py:48-87: one time per batch (asserted), embeddings of positions, times and directions, then the net."""
    assert len(torch.unique(frame_time)) == 1, "Only accepts all points from same time"
    embedded = embed_fn(torch.reshape(inputs, [-1, inputs.shape[-1]]))
    if not embd_time_discr:
        raise NotImplementedError
    B, N, _ = inputs.shape
    embedded_times = embedtime_fn(torch.reshape(frame_time[:, None].expand([B, N, 1]), [-1, 1]))
    embedded_dirs = None
    if viewdirs is not None:
        input_dirs_flat = torch.reshape(viewdirs[:, None].expand(inputs.shape), [-1, viewdirs.shape[-1]])
        embedded_dirs = embeddirs_fn(input_dirs_flat)
        embedded = torch.cat([embedded, embedded_dirs], -1)
    outputs_flat = batchify(fn, netchunk)(embedded, embedded_dirs, embedded_times)
    return torch.reshape(outputs_flat, list(inputs.shape[:-1]) + [outputs_flat.shape[-1]])


def _time_discr(network_query_fn):
    """False when the closure of network_query_fn selects embd_time_discr=False: create_nerf's lambda passes
    `args.nerf_type != "temporal"` (run_tnerf.py:276), create_tnerf's passes `discr`."""
    try:
        cv = inspect.getclosurevars(network_query_fn)
    except TypeError:
        return True
    names = {**cv.globals, **cv.nonlocals}
    if "discr" in names and not names["discr"]:
        return False
    args = names.get("args")
    return getattr(args, "nerf_type", None) != "temporal"


def tnerf_plan(network_query_fn, net, allow_train=False):
    """(L_pos, L_dir, L_time) when render_rays may take the fused T-NeRF pass: no grad (allow_train: or grad - the caller then
    takes the fused TRAINING pass), a TNeRF on the GPU with the fused shape, and the standard encoders in the closure with sizes
    matching the net; else None."""
    if not isinstance(net, TNeRF) or (wants_grad([net]) and not allow_train):
        return None
    bands = net.fused_bands()
    if bands is None or not next(net.parameters()).is_cuda:
        return None
    if not _time_discr(network_query_fn):
        return None                              # embd_time_discr False: the op path raises NotImplementedError, as the reference
    emb = closure_embedders(network_query_fn)
    ef, edf, etf = emb.get("embed_fn"), emb.get("embeddirs_fn"), emb.get("embedtime_fn")
    for e, dims, ch in ((ef, 3, net.in_feat), (edf, 3, net.dir_feat), (etf, 1, net.time_feat)):
        if not (isinstance(e, EmbedFn) and e.input_dims == dims and e.out_dim == ch):
            return None
    return bands


def render_pass_tnerf(ray_batch, net, n_samples, *, z_vals=None, lindisp=False, t_rand=None, noise=None, white_bkgd=False,
                      want=("rgb_map", "disp_map", "acc_map")):
    """One launch of swnerf_render_pass with kind SWNERF_NET_TNERF.  ray_batch [N, 12] = [o, d, near, far, t, viewdirs].
    Returns a dict of the requested outputs among rgb_map disp_map acc_map depth_map weights raw z_out."""
    kind, packed, Lp, Ld, Lt = net.packed()
    rb = _lib.dev_f32(ray_batch, "ray_batch")
    a, out, _keep = pass_args(rb, kind, packed, (Lp, Ld, Lt), int(n_samples), 4, 0, dict(z_vals=z_vals, t_rand=t_rand, noise=noise), want,
                              lindisp=lindisp, white_bkgd=white_bkgd, who="render_pass_tnerf")
    _lib.check(_lib.lib().swnerf_render_pass(a, _lib.stream_of(rb)), "render_pass")
    return out


def render_pass_train_tnerf(ray_batch, net, n_samples, *, z_vals=None, lindisp=False, t_rand=None, noise=None, white_bkgd=False):
    """One differentiable fused T-NeRF pass (train_pass.fused_train_pass): dict with rgb_map disp_map acc_map raw z."""
    return fused_train_pass("tnerf", ray_batch, net, n_samples, z_vals=z_vals, lindisp=lindisp, t_rand=t_rand, noise=noise, white_bkgd=white_bkgd)


def _rng(N, S, perturb, raw_noise_std, pytest, dev, need_t_rand):
    """The random tensors of render_rays in the reference's order: t_rand (run_tnerf.py:461-468; its pytest branch scales by
    raw_noise_std, kept), then the sigma noise of raw2outputs (:367-374)."""
    t_rand = noise = None
    if need_t_rand and perturb > 0.:
        t_rand = torch.rand((N, S), device=dev)
        if pytest:
            np.random.seed(0)
            t_rand = torch.Tensor(np.random.rand(N, S) * raw_noise_std).to(dev)
    if raw_noise_std > 0.:
        noise = torch.randn((N, S), device=dev) * raw_noise_std
        if pytest:
            np.random.seed(0)
            noise = torch.Tensor(np.random.rand(N, S) * raw_noise_std).to(dev)
    return t_rand, noise


def render_rays(ray_batch, network_fn, network_query_fn, N_samples, retraw=False, lindisp=False, perturb=0., N_importance=0,
                network_fine=None, white_bkgd=False, raw_noise_std=0., verbose=False, pytest=False, z_vals=None,
                use_two_models_for_fine=False):
    """run_tnerf.py:395-500 -> {rgb_map, disp_map, acc_map, z_vals (, raw)}.  One net; N_importance only prints the
    reference's warning.  The parameter list is the reference's; the opt-in to the fused TRAINING pass is `fused_train`
    (the context manager below, or batchify_rays' keyword): under grad it is taken when the fused pass's conditions hold and
    2 <= S <= 256; where they do not, the call falls through to the op path as without it."""
    N_rays = ray_batch.shape[0]
    dev = ray_batch.device
    if z_vals is None and N_importance > 0:
        print("Warning: N_importance is set but only a single model is used.")
    S = int(N_samples) if z_vals is None else int(z_vals.shape[-1])
    t_rand, noise = _rng(N_rays, S, perturb, raw_noise_std, pytest, dev, z_vals is None)
    train = _FUSED_TRAIN.get() and wants_grad([network_fn])
    bands = tnerf_plan(network_query_fn, network_fn, allow_train=train) if ray_batch.shape[-1] == 12 else None
    if bands is not None and wants_grad([network_fn]) and not (train and N_rays > 0 and 2 <= S <= TRAIN_FUSED_MAX_SAMPLES):
        bands = None
    if bands is not None:
        # run_network's assertion (run_tnerf.py:52), which the fused pass - it reads each ray's own time - would not need
        assert len(torch.unique(ray_batch[:, 8])) == 1, "Only accepts all points from same time"
        if train:
            p = render_pass_train_tnerf(ray_batch, network_fn, S, z_vals=z_vals, lindisp=lindisp, t_rand=t_rand, noise=noise,
                                        white_bkgd=white_bkgd)
            return result_dict(p, retraw, z_vals=p["z"])
        want = ["rgb_map", "disp_map", "acc_map"] + (["raw"] if retraw else []) + (["z_out"] if z_vals is None else [])
        o = render_pass_tnerf(ray_batch, network_fn, S, z_vals=z_vals, lindisp=lindisp, t_rand=t_rand, noise=noise,
                              white_bkgd=white_bkgd, want=want)
        return result_dict(o, retraw, z_vals=o["z_out"] if z_vals is None else z_vals)
    # the op path (differentiable)
    rays_o, rays_d = ray_batch[:, 0:3], ray_batch[:, 3:6]
    viewdirs = ray_batch[:, -3:] if ray_batch.shape[-1] > 9 else None
    frame_time = torch.reshape(ray_batch[..., 6:9], [-1, 1, 3])[..., 2]
    if z_vals is None:
        z_vals = sample_coarse(ray_batch.detach(), S, lindisp, t_rand)
    pts = rays_o[..., None, :] + rays_d[..., None, :] * z_vals[..., :, None]
    raw = network_query_fn(pts, viewdirs, frame_time, network_fn)
    rgb_map, disp_map, acc_map, weights, depth_map = raw2outputs(raw, z_vals, rays_d, raw_noise_std, white_bkgd, pytest=pytest,
                                                                 noise=noise)
    return result_dict({'rgb_map': rgb_map, 'disp_map': disp_map, 'acc_map': acc_map, 'raw': raw}, retraw, z_vals=z_vals)


def batchify_rays(rays_flat, chunk=1024 * 32, **kwargs):
    """run_tnerf.py:90-103 (this module's render_rays, looked up per call).  One keyword more than the reference passes on:
    fused_train (default False) - under grad, the chunks take the fused training pass (see `fused_train`)."""
    on = bool(kwargs.pop("fused_train", False))
    with fused_train(on or _FUSED_TRAIN.get()):
        return batchify_rays_with(render_rays, rays_flat, chunk, **kwargs)


def render(H, W, focal, chunk=1024 * 32, rays=None, c2w=None, ndc=True, near=0., far=1., frame_time=None,
           use_viewdirs=False, c2w_staticcam=None, **kwargs):
    """run_tnerf.py:106-172 -> [rgb_map, disp_map, acc_map, extras]."""
    if c2w is not None:
        rays_o, rays_d = get_rays(H, W, focal, c2w)
    else:
        rays_o, rays_d = rays
    if use_viewdirs:
        viewdirs = rays_d
        if c2w_staticcam is not None:
            rays_o, rays_d = get_rays(H, W, focal, c2w_staticcam)
        viewdirs = viewdirs / torch.norm(viewdirs, dim=-1, keepdim=True)
        viewdirs = torch.reshape(viewdirs, [-1, 3]).float()
    sh = rays_d.shape
    if ndc:
        rays_o, rays_d = ndc_rays(H, W, focal, 1., rays_o, rays_d)
    rays_o = torch.reshape(rays_o, [-1, 3]).float()
    rays_d = torch.reshape(rays_d, [-1, 3]).float()
    near = near * torch.ones_like(rays_d[..., :1])
    far = far * torch.ones_like(rays_d[..., :1])
    frame_time = frame_time * torch.ones_like(rays_d[..., :1])
    rays = torch.cat([rays_o, rays_d, near, far, frame_time], -1)
    if use_viewdirs:
        rays = torch.cat([rays, viewdirs], -1)
    return image_outputs(batchify_rays(rays, chunk, **kwargs), sh)


def render_path(render_poses, render_times, hwf, chunk, render_kwargs, gt_imgs=None, savedir=None, render_factor=0,
                save_also_gt=False, i_offset=0):
    """run_tnerf.py:175-235 -> (rgbs, disps) as numpy arrays; PNGs under savedir/estim (and savedir/gt)."""
    H, W, focal = hwf
    if render_factor != 0:
        H, W, focal = H // render_factor, W // render_factor, focal / render_factor
    if savedir is not None:
        os.makedirs(os.path.join(savedir, "estim"), exist_ok=True)
        if save_also_gt:
            os.makedirs(os.path.join(savedir, "gt"), exist_ok=True)
    rgbs, disps = [], []
    for i, (c2w, frame_time) in enumerate(zip(render_poses, render_times)):
        rgb, disp, acc, _ = render(H, W, focal, chunk=chunk, rays=None, c2w=c2w[:3, :4], frame_time=frame_time, **render_kwargs)
        rgbs.append(rgb.cpu().numpy())
        disps.append(disp.cpu().numpy())
        if savedir is not None:
            write_png(os.path.join(savedir, "estim", '{:03d}.png'.format(i + i_offset)), to8b(rgbs[-1]))
            if save_also_gt:
                write_png(os.path.join(savedir, "gt", '{:03d}.png'.format(i + i_offset)), to8b(gt_imgs[i]))
    return np.stack(rgbs, 0), np.stack(disps, 0)
