"""The dX chain is ONE function (csrc/mlp_bwd.h) - as a tested property: the per-row kernels, fed what the fused backward
kernels computed for their own chain (their d raw, their ReLU masks, their d dx), must reproduce the fused kernels' gradient
buffers bit for bit.  5 rays x 33 samples on given depths: two workgroups, the second with one live wave; a partial last tile
whose padded rows must come out zero.  Same weights, same transposed streams, same segment order, same seeds - so equality, no
tolerance (profiles/bwd_chain.md has the outcome against the library from before the chain was one function)."""
import numpy as np
import pytest
import torch

import cases
from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
N, S = 5, 33
TILE_ROWS = (S + 31) // 32 * 32                  # padded rows per ray
SENTINEL = -777.25                               # every output starts from it: a column neither kernel writes compares equal


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def inputs(dev):
    """rays, sorted depths in [near, far] and upstream gradients on every output of the pass, g_raw included"""
    g = cases.g8_inputs(n=N)
    rng = np.random.default_rng(33)
    z = np.sort(rng.uniform(2., 6., (N, S)).astype(np.float32), axis=-1)
    up = dict(g_rgb=rng.standard_normal((N, 3)), g_disp=rng.standard_normal(N), g_acc=rng.standard_normal(N),
              g_raw=1e-2 * rng.standard_normal((N, S, 4)), g_pd=1e-2 * rng.standard_normal((N, S, 3)))
    return g, T(z).to(dev), {k: T(v.astype(np.float32)).to(dev) for k, v in up.items()}


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32)


def _same(a, b, what):
    a, b = _bits(a), _bits(b)
    if not np.array_equal(a, b):
        i = np.argwhere(a != b)[0]
        raise AssertionError(f"{what}: {int((a != b).sum())} of {a.size} elements differ, first at {tuple(int(v) for v in i)}: "
                             f"{a.view(np.float32)[tuple(i)]!r} vs {b.view(np.float32)[tuple(i)]!r}")


def _filled(dev, *shape):
    return torch.full(shape, SENTINEL, dtype=torch.float32, device=dev)


def _padded(dev):
    """per padded row of a ray: whether its sample exists, and the sample it reads (the last one past S)"""
    s = torch.arange(TILE_ROWS, device=dev)
    return (s < S).repeat(N), s.clamp(max=S - 1)


def _zero_past_S(buf, cols, what, dev):
    live, _ = _padded(dev)
    dead = buf[~live][:, cols]
    assert dead.shape[0] == N * (TILE_ROWS - S) and bool((dead == 0).all()), f"{what}: rows of samples past S are not all zero"
    assert bool((buf[live][:, cols] != 0).any()), f"{what}: no gradient on the live rows"


def test_static_chain_per_row_equals_fused(dev, inputs):
    """swnerf_render_pass_train -> swnerf_render_pass_backward, then swnerf_mlp_backward_dx over all padded rows on the fused
    kernel's own d_raw and bits with the same SWNERF_BWD_CANON stream: the same grad [rows, SW_ACT_LD]."""
    import swnerf._lib as _lib, swnerf.model as model, swnerf.render as render
    g, z, up = inputs
    L = _lib.lib()
    net = model.vallina_NeRF(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=5, skips=[4], use_viewdirs=True)
    net.load_state_dict({k: T(v) for k, v in cases.weights_static()[1].items()})
    net = net.to(dev)
    rb = O.make_ray_batch(T(g["rays_o"]), T(g["rays_d"]), 2., 6.).to(dev).contiguous()
    kind, packed, Lp, Ld, _ = net.packed()
    rows, nact, st = L.swnerf_train_rows(N, S), L.swnerf_act_floats_per_row(), _lib.stream_of(rb)
    assert rows == N * TILE_ROWS
    act, bits, xs = _filled(dev, rows, nact), _filled(dev, L.swnerf_mask_floats(rows)), _filled(dev, rows, L.swnerf_xs_floats_per_row())
    a, o, _keep = render.pass_args(rb, kind, packed, (Lp, Ld, 0), S, 4, 0, dict(z_vals=z), ["rgb_map", "disp_map", "acc_map", "raw"], white_bkgd=True)
    _lib.check(L.swnerf_render_pass_train(a, _lib.ptr(act), _lib.ptr(bits), _lib.ptr(xs), st), "render_pass_train")
    bwd = net.packed_bwd()
    grad, d_raw = _filled(dev, rows, nact), _filled(dev, rows, 4)
    _lib.check(L.swnerf_render_pass_backward(_lib.ptr(bwd), _lib.ptr(bits), _lib.ptr(o["raw"]), _lib.ptr(z), _lib.ptr(rb), rb.shape[1], None, N, S, 1,
                                             _lib.ptr(up["g_rgb"]), _lib.ptr(up["g_disp"]), _lib.ptr(up["g_acc"]), _lib.ptr(up["g_raw"]),
                                             _lib.ptr(grad), _lib.ptr(d_raw), st), "render_pass_backward")
    grad_rows = _filled(dev, rows, nact)
    _lib.check(L.swnerf_mlp_backward_dx(_lib.ptr(bwd), _lib.ptr(bits), _lib.ptr(d_raw), rows, _lib.ptr(grad_rows), st), "mlp_backward_dx")
    torch.cuda.synchronize()
    _same(grad_rows, grad, "static net: per-row grad vs fused grad")
    written = torch.cat([torch.arange(0, 2048), torch.arange(model.SW_ACT_HV, nact)]).to(dev)   # h_0..h_7 and the views hidden
    for buf, what in ((grad, "fused grad"), (grad_rows, "per-row grad")):
        _zero_past_S(buf, written, what, dev)


@pytest.mark.parametrize("with_g_pd", [False, True])
def test_dnerf_chains_per_row_equal_fused(dev, inputs, with_g_pd):
    """swnerf_render_pass_train_dnerf -> swnerf_render_pass_backward_dnerf at t = 0.5, then the deformation chain
    (swnerf_deform_backward_dx on the fused g_dx[:, :3] and bits_d, SWNERF_BWD_DEFORM stream) and the canonical chain with the input
    gradient (swnerf_mlp_backward_dx_pts on the fused d_raw, bits and pts = o + d z + dx formed in fp32 in the kernel's order,
    SWNERF_BWD_CANON_INPUT_GRAD stream): the same grad_d and grad, and without g_position_delta the same d x on the live rows."""
    import swnerf._lib as _lib, swnerf.embedder as embedder, swnerf.model as model, swnerf.render as render
    g, z, up = inputs
    L = _lib.lib()
    embed_fn, _ = embedder.get_embedder(10, 3, 0)
    net = model.DirectTemporalNeRF(D=8, W=256, input_ch=63, input_ch_views=27, input_ch_time=21, output_ch=5, skips=[4],
                                   use_viewdirs=True, embed_fn=embed_fn, zero_canonical=True)
    net.load_state_dict({k: T(v) for k, v in cases.weights_dnerf().items()})
    net = net.to(dev)
    rb = O.make_ray_batch(T(g["rays_o"]), T(g["rays_d"]), 2., 6., frame_time=0.5).to(dev).contiguous()
    kind, packed, Lp, Ld, Lt = net.packed()
    rows, nact, nxs, st = L.swnerf_train_rows(N, S), L.swnerf_act_floats_per_row(), L.swnerf_xs_floats_per_row(), _lib.stream_of(rb)
    nbits = L.swnerf_mask_floats(rows)
    act, bits, xs = _filled(dev, rows, nact), _filled(dev, nbits), _filled(dev, rows, nxs)
    act_d, bits_d, xs_d = _filled(dev, rows, nact), _filled(dev, nbits), _filled(dev, rows, nxs)
    a, o, _keep = render.pass_args(rb, kind, packed, (Lp, Ld, Lt), S, 4, 1, dict(z_vals=z), ["rgb_map", "disp_map", "acc_map", "raw", "dx"], white_bkgd=True)
    _lib.check(L.swnerf_render_pass_train_dnerf(a, _lib.ptr(act), _lib.ptr(bits), _lib.ptr(xs), _lib.ptr(act_d), _lib.ptr(bits_d), _lib.ptr(xs_d), st),
               "render_pass_train_dnerf")
    grad, grad_d, d_raw, g_dx = _filled(dev, rows, nact), _filled(dev, rows, nact), _filled(dev, rows, 4), _filled(dev, rows, 4)
    _lib.check(L.swnerf_render_pass_backward_dnerf(
        _lib.ptr(net.packed_bwd(_lib.BWD_DNERF_FUSED)), _lib.ptr(bits), _lib.ptr(bits_d), _lib.ptr(o["raw"]), _lib.ptr(z), _lib.ptr(rb), rb.shape[1], None,
        _lib.ptr(o["dx"]), _lib.ptr(up["g_pd"] if with_g_pd else None), N, S, 1, Lp, _lib.ptr(up["g_rgb"]), _lib.ptr(up["g_disp"]), _lib.ptr(up["g_acc"]),
        _lib.ptr(up["g_raw"]), _lib.ptr(grad), _lib.ptr(grad_d), _lib.ptr(d_raw), _lib.ptr(g_dx), st), "render_pass_backward_dnerf")
    # the deformation net's chain
    d_dx = g_dx[:, :3].contiguous()
    grad_d_rows = _filled(dev, rows, nact)
    _lib.check(L.swnerf_deform_backward_dx(_lib.ptr(net.packed_bwd(_lib.BWD_DEFORM)), _lib.ptr(bits_d), _lib.ptr(d_dx), rows, _lib.ptr(grad_d_rows), st),
               "deform_backward_dx")
    # the canonical net's chain with the input gradient, on the points the fused forward formed: (o + d z) + dx, one rounding each
    live, s_of = _padded(dev)
    pts = ((rb[:, None, 0:3] + rb[:, None, 3:6] * z[:, s_of, None]) + o["dx"][:, s_of, :]).reshape(rows, 3).contiguous()
    grad_rows, d_pts = _filled(dev, rows, nact), _filled(dev, rows, 3)
    _lib.check(L.swnerf_mlp_backward_dx_pts(_lib.ptr(net._occ.packed_bwd(_lib.BWD_CANON_INPUT_GRAD)), _lib.ptr(bits), _lib.ptr(d_raw), _lib.ptr(pts), rows, Lp,
                                            _lib.ptr(grad_rows), _lib.ptr(d_pts), st), "mlp_backward_dx_pts")
    torch.cuda.synchronize()
    _same(grad_d_rows, grad_d, "D-NeRF: per-row grad_d vs fused grad_d")
    _same(grad_rows, grad, "D-NeRF: per-row grad vs fused grad")
    if not with_g_pd:
        _same(d_pts[live], d_dx[live], "D-NeRF: per-row d_pts vs fused g_dx[:, :3] on the live rows")
    trunk = torch.arange(0, 2048, device=dev)
    _zero_past_S(grad_d, trunk, "fused grad_d", dev)
    _zero_past_S(grad_d_rows, trunk, "per-row grad_d", dev)
    _zero_past_S(grad, trunk, "fused grad", dev)
    _zero_past_S(grad_rows, trunk, "per-row grad", dev)
