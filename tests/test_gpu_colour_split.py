"""The colour branch as its own pass (include/swnerf.h swnerf_render_pass_ws; csrc/render_pass.h phase A, csrc/colour_kernels.hip
phases B and C): with a workspace the fused static pass stashes its live rows (alpha != 0, and sample 0), a persistent kernel colours
them packed 32 to a view segment across rays, and a last kernel forms the colour sums and rgb_map.  How many rows a ray can stash
follows from the workspace's size: tests/test_gpu_deferred_view.py runs at the least one (about 60 rows per ray, so its rays with
more live rows also take the in-line fall-back); here
  * the full workspace (swnerf_view_ws_floats: every tile stashes) over that module's live patterns, both amplitudes, white
    background on and off;
  * a workspace of exactly 100 rows per ray at S = 192: a ray then mixes tiles that stash and tiles that run in line;
  * the edges of the packing: fewer than 32 stashed rows in the whole launch, an exact multiple of 32, a segment that spans three
    rays, one ray, five rays;
  * a workspace used again after an all-live launch for a sparse one (stale rows, counts and colours would show);
  * a NaN in the rgb bias, which must reach every ray through the packed kernel;
  * a two-net render call against the same call with `raw` requested, whose fine pass runs in line.
Every comparison is torch.equal (NaN patterns included) against the launch without a workspace.  Workspaces are prefilled with NaN
(as floats; as the integers of the bookkeeping that is 0x7fc00000): a cell read before it was written would show or fault the
index checks below."""
import copy

import numpy as np
import pytest
import torch

from test_gpu_fused_tail import Gate, same, net_of, rays_of
import test_gpu_deferred_view as dv

pytestmark = pytest.mark.gpu
DEV = dv.DEV
N = dv.N
OUTS = dv.OUTS
ROW_FLOATS = 257                                 # one stashed row: 256 activations and its sample index (include/swnerf.h)


def full_floats(n, S):
    from swnerf import _lib
    return int(_lib.lib().swnerf_view_ws_floats(n, S))


def nan_ws(floats):
    return torch.full((floats,), float("nan"), dtype=torch.float32, device=DEV)


def launch(net, rb, S, *, ws, noise=None, z_vals=None, n_importance=0, white=False, want=OUTS):
    """swnerf_render_pass at the C ABI with or without the workspace -> (return code, outputs); dv.launch with white_bkgd"""
    import swnerf.render as render
    from swnerf import _lib
    kind, packed, Lp, Ld, Lt = net.packed()
    a, out, _keep = render.pass_args(rb, kind, packed, (Lp, Ld, Lt), S, 4, 0, dict(z_vals=z_vals, t_rand=None, noise=noise, u=None),
                                     want, n_importance, white_bkgd=white)
    for t in out.values():
        t.fill_(-7.0)
    if ws is None:
        rc = _lib.lib().swnerf_render_pass(a, _lib.stream_of(rb))
    else:
        rc = _lib.lib().swnerf_render_pass_ws(a, _lib.ptr(ws), ws.numel(), _lib.stream_of(rb))
    torch.cuda.synchronize()
    return rc, out


def stashed_total(ws, n):
    """the launch header's last prefix entry: stashed rows of the whole launch (csrc/render_pass.h: int off[n_rays + 1] in front)"""
    return int(ws[:n + 1].view(torch.int32)[n])


def compare(g, what, defer, inline):
    for k in inline:
        g.true(bool(torch.isfinite(inline[k]).all()) or k == "disp_map", f"{what}: the inline launch's {k} is not finite")
        g.true(same(defer[k], inline[k]), f"{what}: {k} differs between the workspace launch and the inline launch "
                                          f"({int((defer[k] != inline[k]).sum())} elements)")


@pytest.mark.parametrize("white", [False, True], ids=["black", "white"])
@pytest.mark.parametrize("amp", [1e4, 1.0], ids=["opaque", "mild"])
@pytest.mark.parametrize("case", ["S33", "S64_resample", "S192_fine"])
def test_full_workspace_equals_inline_launch(case, amp, white):
    """every tile stashes: the stashed rows of the launch are exactly its live rows and canaries, and every output is the in-line
    launch's"""
    S, given, Ni = dv.CASES[case]
    net, rb = net_of("canon"), rays_of("canon", n=N)
    kw = dict(noise=dv.noise_of(S, amp), z_vals=dv.sorted_depths(rb, S) if given else None, n_importance=Ni, white=white)
    rc0, inline = launch(net, rb, S, ws=None, **kw)
    ws = nan_ws(full_floats(N, S))
    rc1, defer = launch(net, rb, S, ws=ws, **kw)
    assert rc0 == 0 and rc1 == 0
    g = Gate()
    compare(g, f"{case} amp={amp:g} white={white}", defer, inline)
    m = dv.live_mask(S)
    m[:, 0] = True                               # the canary
    g.true(stashed_total(ws, N) == int(m.sum()), f"{stashed_total(ws, N)} rows were stashed, the launch has {int(m.sum())} live rows and canaries")
    g.finish(f"colour split, full workspace, {case} amp={amp:g} white={white}")


@pytest.mark.parametrize("amp", [1e4, 1.0], ids=["opaque", "mild"])
def test_hundred_rows_per_ray_mix_stash_and_inline(amp):
    """R = 100 at S = 192: a tile stashes while 32 more rows are certain to fit, so a ray with many live rows stashes its first
    tiles and runs the others in line"""
    S, R = 192, 100
    net, rb = net_of("canon"), rays_of("canon", n=N)
    kw = dict(noise=dv.noise_of(S, amp), z_vals=dv.sorted_depths(rb, S))
    _, inline = launch(net, rb, S, ws=None, **kw)
    ws = nan_ws(full_floats(N, S) - N * ROW_FLOATS * (S - R))
    rc, defer = launch(net, rb, S, ws=ws, **kw)
    assert rc == 0
    g = Gate()
    compare(g, f"R=100 amp={amp:g}", defer, inline)
    # what the rule stashes: tiles in order, each one while the rows so far + 32 <= R
    m = dv.live_mask(S)
    m[:, 0] = True
    per_tile = m.reshape(N, S // 32, 32).sum(2)
    want, mixed = 0, 0
    for r in range(N):
        wr, inl = 0, 0
        for c in per_tile[r]:
            if wr + 32 <= R:
                wr += int(c)
            else:
                inl += 1
        want += wr
        mixed += bool(wr and inl)
    assert mixed >= 8                            # the case does what it says
    g.true(stashed_total(ws, N) == want, f"{stashed_total(ws, N)} rows were stashed, the rule gives {want}")
    g.finish(f"colour split, 100 rows per ray, amp={amp:g}")


# live rows per ray (sample 0 among them) -> stashed rows of the launch; S = 64
PACKING = {
    "below_32": [3, 1, 7, 2, 5],                 # 18 rows: one padded segment
    "exactly_64": [16, 16, 10, 12, 10],          # two full segments, no padding; the boundary falls inside ray 1 / on a ray's end
    "three_rays_in_a_segment": [20, 5, 20],      # rows 0..31 lie in rays 0, 1 and 2
    "one_ray": [40],                             # a full and a padded segment of one ray
    "five_rays": [64, 1, 33, 1, 31],             # 130 rows: a ray of whole segments, canary-only rays between
}


@pytest.mark.parametrize("white", [False, True], ids=["black", "white"])
@pytest.mark.parametrize("name", list(PACKING))
def test_packing_edges(name, white):
    S, counts = 64, PACKING[name]
    n = len(counts)
    rng = np.random.default_rng(17 + n)
    m = np.zeros((n, S), dtype=bool)
    for r, c in enumerate(counts):
        m[r, 0] = True
        m[r, 1 + rng.choice(S - 1, size=c - 1, replace=False)] = True
    noise = torch.from_numpy(np.where(m, np.float32(1.0), np.float32(-1e4))).to(DEV)
    net, rb = net_of("canon"), rays_of("canon", n=n)
    _, inline = launch(net, rb, S, ws=None, noise=noise, white=white)
    ws = nan_ws(full_floats(n, S))
    rc, defer = launch(net, rb, S, ws=ws, noise=noise, white=white)
    assert rc == 0
    g = Gate()
    compare(g, name, defer, inline)
    g.true(stashed_total(ws, n) == sum(counts), f"{stashed_total(ws, n)} rows were stashed, the pattern has {sum(counts)}")
    g.finish(f"colour split, packing edge {name} white={white}")


def test_workspace_used_again_after_an_all_live_launch():
    """an all-live launch fills every row, count and colour of the workspace; the sparse launch behind it on the same workspace
    must read none of them"""
    S = 64
    net, rb = net_of("canon"), rays_of("canon", n=N)
    ws = nan_ws(full_floats(N, S))
    rc, _ = launch(net, rb, S, ws=ws, noise=torch.full((N, S), 1.0, device=DEV), white=True)
    assert rc == 0 and stashed_total(ws, N) == N * S
    noise = dv.noise_of(S, 1.0)
    _, inline = launch(net, rb, S, ws=None, noise=noise, white=True)
    rc, defer = launch(net, rb, S, ws=ws, noise=noise, white=True)
    assert rc == 0
    g = Gate()
    compare(g, "second use", defer, inline)
    g.finish("colour split, workspace used again")


def test_poisoned_rgb_bias_reaches_every_ray_through_the_packed_kernel():
    """one NaN in rgb_linear.bias[0], full workspace (no row is coloured in line): red of EVERY ray is NaN, the rest finite"""
    S = 64
    net = copy.deepcopy(net_of("canon"))
    net._pack_cache = {}
    with torch.no_grad():
        net.rgb_linear.bias[0] = float("nan")
    rb = rays_of("canon", n=N)
    rc, out = launch(net, rb, S, ws=nan_ws(full_floats(N, S)), noise=dv.noise_of(S, 1e4))
    assert rc == 0
    g = Gate()
    g.true(bool(torch.isnan(out["rgb_map"][:, 0]).all()), f"{int((~torch.isnan(out['rgb_map'][:, 0])).sum())} rays have a finite red behind a NaN rgb bias")
    g.true(bool(torch.isfinite(out["rgb_map"][:, 1:]).all()), "the other channels do not depend on bias[0]")
    g.true(bool(torch.isfinite(out["acc_map"]).all()), "acc_map does not depend on the colours")
    g.finish("colour split, poisoned rgb bias")


def test_two_net_render_equals_the_call_with_raw():
    """render_rays with two nets, 64 + 128 samples, 67 rays: with `raw` requested the fine pass runs in line; the maps of both calls
    are the same bits.  The coarse maps also against a coarse launch that runs in line."""
    import swnerf.render as render
    from swnerf import synth, model, embedder
    from oracle import nerf_oracle as O
    embed_fn, input_ch = embedder.get_embedder(10, 3, 0)
    embeddirs_fn, input_ch_views = embedder.get_embedder(4, 3, 0)
    nets = []
    for seed, ab in (synth.NET_COARSE, synth.NET_FINE):
        sd = synth.nerf_state_dict(seed, alpha_bias=ab)
        m = model.vallina_NeRF(D=8, W=256, input_ch=input_ch, input_ch_views=input_ch_views, output_ch=5, skips=[4], use_viewdirs=True)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        nets.append(m.to(DEV).eval())
    query = lambda inputs, viewdirs, network_fn: render.run_network(inputs, viewdirs, network_fn, embed_fn=embed_fn,
                                                                    embeddirs_fn=embeddirs_fn, netchunk=1024 * 64)
    K, c2w = synth.lego_camera(400, 400)
    o, d = synth.pick_rays(400, 400, K, c2w, N, seed=9)
    rb = O.make_ray_batch(torch.from_numpy(o), torch.from_numpy(d), 2., 6.).to(DEV)
    kw = dict(N_samples=64, N_importance=128, network_fine=nets[1], white_bkgd=True, perturb=0., raw_noise_std=0.)
    with torch.no_grad():
        split = render.render_rays(rb, nets[0], query, retraw=False, **kw)
        inline = render.render_rays(rb, nets[0], query, retraw=True, **kw)
        coarse = render.render_pass(rb, nets[0], 64, white_bkgd=True, want=["rgb_map", "disp_map", "acc_map", "raw"])
    torch.cuda.synchronize()
    g = Gate()
    for k in ("rgb_map", "disp_map", "acc_map", "rgb0", "disp0", "acc0", "z_std"):
        g.true(same(split[k], inline[k]), f"{k} differs between the two calls ({int((split[k] != inline[k]).sum())} elements)")
    for k in ("rgb", "disp", "acc"):
        g.true(same(split[k + "0"], coarse[k + "_map"]), f"{k}0 differs from the in-line coarse launch")
    g.true(bool(torch.isfinite(split["rgb_map"]).all()), "rgb_map is not finite")
    g.finish("colour split, two-net render call")

