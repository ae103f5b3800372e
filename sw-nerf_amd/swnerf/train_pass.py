"""The fused render passes under autograd: ONE torch.autograd.Function (`_FusedTrainPass`) and one front function
(`fused_train_pass`) for the four net kinds that have a fused training pass - what differs between them is the table KINDS.

    canon   vallina_NeRF / NeRFOriginal with view directions (the reference's step is render -> img2mse ->
            loss.backward(), nerf/run.py:684-708).  forward = swnerf_render_pass_train: the inference pass that also saves
            activations, ReLU masks, the encodings and raw; backward = swnerf_render_pass_backward (one wave per ray: compositing
            backward in LDS, then the dX chain per tile) + one TN MFMA GEMM per Linear layer.  No [M,90] embedding, no cat, no
            pts tensor ever reaches HBM.
    noview  the same net with use_viewdirs=False: 8-column rays, raw [N,S,out_ch], swnerf_render_pass_backward_noview.
    dnerf   DirectTemporalNeRF at t != 0 (model.py:128-151; the loss of d_nerf/run_dnerf.py:690-725 puts gradients on the image
            and on position_delta).  forward = swnerf_render_pass_train_dnerf: deformation net -> x + dx -> canonical net ->
            compositing in one kernel, saving both nets' activations / masks / encodings as side stores; backward =
            swnerf_render_pass_backward_dnerf: per ray the compositing backward, then per tile the canonical dX chain incl.
            d gamma(x+dx) -> d(x+dx) through the sin/cos Jacobian, + the upstream gradient of position_delta, then the
            deformation net's dX chain - ONE weight ring over both transposed streams; then one TN GEMM per Linear layer of both.
    tnerf   TNeRF (the step of t_nerf/run_tnerf.py:680-720).  forward = swnerf_render_pass_train_tnerf: the inference pass, bit
            for bit, that also saves the post-ELU activations and the encodings; backward = swnerf_render_pass_backward_tnerf
            (ELU' from the saved activations) + one TN GEMM per weight block (`feature` is un-folded from G in
            swnerf_tnerf_feature_finish).

Gradients flow to the net's parameters only (rays are data; the depths of the fine pass are detached in the reference,
nerf/run.py:398).  The knobs are read at call time through the modules that own them - render.TRAIN_BWD_CHUNK_ROWS,
render.PASS_HOOK, render_dnerf.DNERF_CHUNK_DIV (tests and bench.py set them there) - and render.pass_args with them: those
modules import this one, so they are imported inside the functions."""
from collections import namedtuple

import torch

from . import _lib
from .model import _CANON_ORDER, _NOVIEW_ORDER, _TNERF_ORDER
from .wgrad import WeightGrads, _Fan, _chunk_gemms

TRAIN_FUSED_MAX_SAMPLES = 256      # include/swnerf.h: swnerf_render_pass_train


def chunked_backward(rb, act_rows, div, widths, launch, gemm_jobs, rest_on_main=True):
    """The backward of a fused training pass, per CHUNK of rays.  The gradient buffer [rows, 2432] is as large as the saved
    activations; the dX chain and the GEMMs that consume it run per chunk, so only one chunk of it is ever alive (GEMMs
    accumulate: C += A^T.B).  A chunk is TRAIN_BWD_CHUNK_ROWS // div rows (393 216 at the C2 shape: large enough for the
    split-K GEMMs to fill the chip), whole rays, a multiple of 4.  widths: {name: columns} of the buffers a chunk holds;
    launch(r0, r1, bufs) runs the backward kernel on rays r0:r1; gemm_jobs(a0, a1, m, bufs) -> the jobs of wgrad._chunk_gemms
    on the rows a0:a1 of the saved tensors (m = a1 - a0 rows of every buffer), which fan out over side streams (wgrad._Fan)."""
    from . import render
    N = rb.shape[0]
    rows_per_ray = act_rows // N
    chunk = max(4, (render.TRAIN_BWD_CHUNK_ROWS // div // rows_per_ray) // 4 * 4)
    bufs = {k: torch.empty((min(N, chunk) * rows_per_ray, w), dtype=torch.float32, device=rb.device) for k, w in widths.items()}
    fan = _Fan(rb.device)
    for r0 in range(0, N, chunk):
        r1 = min(N, r0 + chunk)
        launch(r0, r1, bufs)
        _chunk_gemms(_lib.lib(), fan, (r1 - r0) * rows_per_ray, gemm_jobs(r0 * rows_per_ray, r1 * rows_per_ray, (r1 - r0) * rows_per_ray, bufs),
                     rest_on_main=rest_on_main)


def f32_grads(*gs):
    """Upstream gradients as the kernels read them (an output the loss does not use arrives as None and stays None)."""
    return [None if g is None else g.contiguous().float() for g in gs]


def ray_ptrs(r0, r1, *ts, per_ray=1):
    """Pointers to the rows of rays r0:r1 of each tensor (None stays NULL)."""
    return [_lib.ptr(None if t is None else t[r0 * per_ray:r1 * per_ray]) for t in ts]


# ---- what differs between the kinds ------------------------------------------------------------------------------------------
def _static_saved(L, rows, new):
    return dict(act=new(rows, L.swnerf_act_floats_per_row()), bits=new(L.swnerf_mask_floats(rows)), xs=new(rows, L.swnerf_xs_floats_per_row()))


def _dnerf_saved(L, rows, new):
    nact, nxs, nbits = L.swnerf_act_floats_per_row(), L.swnerf_xs_floats_per_row(), L.swnerf_mask_floats(rows)
    return dict(act=new(rows, nact), bits=new(nbits), xs=new(rows, nxs), act_d=new(rows, nact), bits_d=new(nbits), xs_d=new(rows, nxs))


def _tnerf_saved(L, rows, new):
    return dict(act=new(rows, L.swnerf_tnerf_act_floats_per_row()), xs=new(rows, L.swnerf_tnerf_xs_floats_per_row()))


def _canon_streams(net):
    kind, packed, Lp, Ld, _ = net.packed()
    return kind, packed, (Lp, Ld, 0), 4


def _noview_streams(net):
    packed, Lp, out_ch = net.packed_noview()
    return _lib.NET_NOVIEW, packed, (Lp, 0, 0), out_ch


def _time_streams(net):
    kind, packed, *bands = net.packed()
    return kind, packed, tuple(bands), 4


# streams(net) -> (kind id, packed, bands, out_ch); packed_bwd(net); order(net): the parameter names behind *params
# saved(L, rows, new): the buffers the forward entry fills, in the order their pointers follow `args`
# fwd / bwd: the entries (swnerf_<name>; `fwd` is the who= label too); keys: the front function's dict
# slots: the backward entry's arguments after packed_bwd and before the stream - a saved / output / upstream-gradient tensor
#   (the rows of rays r0:r1), a scalar of the launch (cols n S white out_ch L_pos) or a chunk buffer (whole)
# wgrads: (WeightGrads kind, parameter slice, net attributes of Cpos / Cdir / Ct, chunk()'s grad / act / enc / draw) per net
# widths: {chunk buffer: columns, None = the act row}; rest_on_main: wgrad._chunk_gemms (the no-view net and T-NeRF have no
#   fused narrow kernel)
# run_deform, extra_out: pass_args; cols: the ray-batch width to insist on; hook: render.PASS_HOOK around the forward launch
#   (bench.py times the static fine passes through it)
# dnerf_div: two gradient buffers per chunk, TRAIN_BWD_CHUNK_ROWS // DNERF_CHUNK_DIV rows each, so that a chunk holds what the
#   static backward's does (a whole fine pass in one chunk: 15 GB of gradients, 29.6 GiB peak for a 4096-ray step)
_Kind = namedtuple("_Kind", "streams packed_bwd order saved fwd keys bwd slots wgrads widths rest_on_main run_deform extra_out cols hook dnerf_div",
                   defaults=(0, [], None, False, False))
_STATIC_SLOTS = "bits raw z rb cols noise n S white g_rgb g_disp g_acc g_raw grad d_raw"
KINDS = {
    "canon": _Kind(streams=_canon_streams, packed_bwd=lambda net: net.packed_bwd(), order=lambda net: _CANON_ORDER, saved=_static_saved,
                   fwd="render_pass_train", hook=True, keys="rgb_map disp_map acc_map raw",
                   bwd="render_pass_backward", slots=_STATIC_SLOTS,
                   wgrads=[("canon", slice(None), "input_ch", "input_ch_views", None, "grad act xs d_raw")],
                   widths={"grad": None, "d_raw": 4}, rest_on_main=True),
    "noview": _Kind(streams=_noview_streams, packed_bwd=lambda net: net.packed_bwd_noview(), order=lambda net: _NOVIEW_ORDER, saved=_static_saved,
                    fwd="render_pass_train", hook=True, keys="rgb_map disp_map acc_map raw",
                    bwd="render_pass_backward_noview", slots=_STATIC_SLOTS.replace("white", "white out_ch"),
                    wgrads=[("noview", slice(None), "input_ch", None, None, "grad act xs d_raw")],
                    widths={"grad": None, "d_raw": 8}, rest_on_main=False),
    "dnerf": _Kind(streams=_time_streams, packed_bwd=lambda net: net.packed_bwd(_lib.BWD_DNERF_FUSED), order=lambda net: net._pack_params()[1],
                   saved=_dnerf_saved, fwd="render_pass_train_dnerf", run_deform=1, extra_out=["dx"], keys="rgb_map disp_map acc_map dx z raw",
                   bwd="render_pass_backward_dnerf",
                   slots="bits bits_d raw z rb cols noise dx g_dx n S white L_pos g_rgb g_disp g_acc g_raw grad grad_d d_raw d_dx",
                   wgrads=[("canon", slice(0, 24), "input_ch", "input_ch_views", None, "grad act xs d_raw"),        # the 24 `_occ` tensors
                           ("deform", slice(24, None), "input_ch", None, None, "grad_d act_d xs_d d_dx")],          # the 18 `_time` / `_time_out`
                   widths={"grad": None, "grad_d": None, "d_raw": 4, "d_dx": 4}, dnerf_div=True, rest_on_main=True),
    "tnerf": _Kind(streams=_time_streams, packed_bwd=lambda net: net.packed_bwd(), order=lambda net: _TNERF_ORDER, saved=_tnerf_saved,
                   fwd="render_pass_train_tnerf", cols=12, keys="rgb_map disp_map acc_map raw z",
                   bwd="render_pass_backward_tnerf", slots=_STATIC_SLOTS.replace("bits", "act"),
                   wgrads=[("tnerf", slice(None), "in_feat", "dir_feat", "time_feat", "grad act xs d_raw")],
                   widths={"grad": None, "d_raw": 4}, rest_on_main=False),
}


class _FusedTrainPass(torch.autograd.Function):
    """forward(kind, net, rb, z_vals, S, lindisp, t_rand, noise, white_bkgd, n_importance, u, *params) -> rgb_map, disp_map,
    acc_map, raw, z, dx, z_fine, z_std (None where the kind or the call has none).  raw is an output as well (retraw=True is
    what the reference's train() passes, nerf/run.py:685): a gradient arriving on it is added to d raw in the backward kernel."""

    @staticmethod
    def forward(ctx, kind, net, rb, z_vals, S, lindisp, t_rand, noise, white_bkgd, n_importance, u, *params):
        from . import render
        k = KINDS[kind]
        net_kind, packed, bands, out_ch = k.streams(net)
        L = _lib.lib()
        N = rb.shape[0]
        saved = k.saved(L, L.swnerf_train_rows(N, S), lambda *shape: torch.empty(shape, dtype=torch.float32, device=rb.device))
        a, o, _keep = render.pass_args(rb, net_kind, packed, bands, S, out_ch, k.run_deform, dict(z_vals=z_vals, t_rand=t_rand, noise=noise, u=u),
                                       ["rgb_map", "disp_map", "acc_map", "raw"] + k.extra_out + ([] if z_vals is not None else ["z_out"]),
                                       n_importance, lindisp=lindisp, white_bkgd=white_bkgd, who=k.fwd)
        z = z_vals if z_vals is not None else o["z_out"]
        hook = render.PASS_HOOK if k.hook else None
        if hook is not None:
            hook("begin", N, S)
        _lib.check(getattr(L, "swnerf_" + k.fwd)(a, *[_lib.ptr(t) for t in saved.values()], _lib.stream_of(rb)), k.fwd)
        if hook is not None:
            hook("end", N, S)
        ctx.kind, ctx.net, ctx.S, ctx.white, ctx.bands, ctx.out_ch, ctx.names = kind, net, S, bool(white_bkgd), bands, out_ch, list(saved)
        ctx.save_for_backward(rb, z, o["raw"], o.get("dx"), noise, *saved.values(), *params)
        dead = [t for t in (z, o.get("z_fine"), o.get("z_std")) if t is not None]
        ctx.mark_non_differentiable(*dead)
        ctx.set_materialize_grads(False)       # an output the loss does not use arrives as None (no zero fill, no read of zeros in the kernel)
        return o["rgb_map"], o["disp_map"], o["acc_map"], o["raw"], z, o.get("dx"), o.get("z_fine"), o.get("z_std")

    @staticmethod
    def backward(ctx, *grads_out):
        k, net = KINDS[ctx.kind], ctx.net
        rb, z, raw, dx, noise, *rest = ctx.saved_tensors
        params = rest[len(ctx.names):]
        t = dict(zip(ctx.names, rest), rb=rb, z=z, raw=raw, dx=dx, noise=noise)
        t["g_rgb"], t["g_disp"], t["g_acc"], t["g_raw"], _gz, t["g_dx"], _gf, _gs = f32_grads(*grads_out)
        L = _lib.lib()
        N, cols = rb.shape
        st = _lib.stream_of(rb)
        attr = lambda name: getattr(net, name) if name else 0
        wgs = [WeightGrads(L, wk, params[sl], fused=True, Cpos=attr(cp), Cdir=attr(cd), Ct=attr(ct), bands=ctx.bands)
               for wk, sl, cp, cd, ct, _ in k.wgrads]
        packed_bwd = k.packed_bwd(net)
        scalars = dict(cols=cols, S=ctx.S, white=int(ctx.white), out_ch=ctx.out_ch, L_pos=ctx.bands[0])

        def launch(r0, r1, bufs):
            scalars["n"] = r1 - r0
            args = [scalars[s] if s in scalars else _lib.ptr(bufs[s]) if s in bufs else
                    ray_ptrs(r0, r1, t[s], per_ray=1 if t[s] is None else t[s].shape[0] // N)[0] for s in k.slots.split()]
            _lib.check(getattr(L, "swnerf_" + k.bwd)(_lib.ptr(packed_bwd), *args, st), k.bwd)

        def jobs(a0, a1, m, bufs):
            return [lambda st_, part, wg=wg, b=w[5].split(): wg.chunk(st_, m, bufs[b[0]][:m], t[b[1]][a0:a1], t[b[2]][a0:a1], bufs[b[3]][:m], part=part)
                    for wg, w in zip(wgs, k.wgrads)]

        div = 1
        if k.dnerf_div:
            from . import render_dnerf
            div = render_dnerf.DNERF_CHUNK_DIV
        act = t["act"]
        chunked_backward(rb, act.shape[0], div, {b: w or act.shape[1] for b, w in k.widths.items()}, launch, jobs, rest_on_main=k.rest_on_main)
        g = [gi for wg in wgs for gi in wg.finish(st)]
        # one None per forward argument in front of *params
        return (None,) * (len(ctx.needs_input_grad) - len(params)) + tuple(gi.to(p.dtype) for gi, p in zip(g, params))


def fused_train_pass(kind, ray_batch, net, n_samples, *, z_vals=None, lindisp=False, t_rand=None, noise=None, white_bkgd=False,
                     n_importance=0, u=None):
    """One differentiable fused pass of `net` as `kind` (a key of KINDS): dict with rgb_map disp_map acc_map raw, for the static
    kinds z_fine z_std when n_importance > 0, for D-NeRF dx and z, for T-NeRF z."""
    k = KINDS[kind]
    rb = _lib.dev_f32(ray_batch.detach(), "ray_batch", k.cols)
    S = int(n_samples)
    chk = lambda t, name, last=S: None if t is None else _lib.dev_f32(t.detach(), name, last)
    z_vals, t_rand, noise, u = chk(z_vals, "z_vals"), chk(t_rand, "t_rand"), chk(noise, "noise"), chk(u, "u", int(n_importance))
    sd = dict(net.named_parameters())
    outs = _FusedTrainPass.apply(kind, net, rb, z_vals, S, bool(lindisp), t_rand, noise, bool(white_bkgd), int(n_importance), u,
                                 *[sd[n] for n in k.order(net)])
    out = dict(zip("rgb_map disp_map acc_map raw z dx z_fine z_std".split(), outs))
    return {key: out[key] for key in k.keys.split() + (["z_fine", "z_std"] if n_importance > 0 else [])}
