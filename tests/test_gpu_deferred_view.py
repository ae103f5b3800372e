"""The deferred colour branch of the fused inference pass (include/swnerf.h swnerf_render_pass_ws, csrc/render_pass.h): with a
workspace the pass runs the view layer and the rgb head only on a ray's sample 0 and on its samples with alpha != 0, compacted over
the ray's tiles; without one on every sample.  Both launches must give the same bits.

All cases: 67 rays (a last workgroup of three waves) of the seeded canon net the other fused-pass tests use (dead density head:
sigma = B_SIGMA everywhere), liveness forced through `noise`: a dead sample gets -1e4 (alpha == 0 exactly), a live one +1e4
(alpha == 1: the issue's setting) or +1 ("mild": alpha about 0.05, so that many live rows carry a weight that is not negligible
and a colour scattered to the wrong sample would show in rgb_map).  One launch holds every live pattern, one per ray:
  live rows per ray  0 (only the canary) 1 31 32 33 63 64 65 all      x
  position           front | back | every other sample | seeded random
(36 rays; the other 31 rays take seeded random counts and positions.)  Over S in {33, 64, 192} these hit: no view segment before
the drain, a fill exactly at a tile boundary, one and two view-only turns, a padded partial tile, a tile whose live rows leave no
room for pending ones, and wrap-around of the 64-row ring (S = 192 with 65 and more live rows).
The workspace is prefilled with NaN: a row read before it was written would show."""
import copy

import numpy as np
import pytest
import torch

from test_gpu_fused_tail import Gate, same, net_of, rays_of

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
N = 67
COUNTS = (0, 1, 31, 32, 33, 63, 64, 65, -1)      # -1: all
PLACES = ("front", "back", "alternate", "random")
OUTS = ["rgb_map", "disp_map", "acc_map", "depth_map", "weights", "z_out"]
WS_FLOATS = 64 * 256


def live_mask(S, seed=5):
    """[N, S] bool: the live pattern of every ray"""
    rng = np.random.default_rng(seed + S)
    m = np.zeros((N, S), dtype=bool)
    combos = [(c, p) for c in COUNTS for p in PLACES]
    for r in range(N):
        c, p = combos[r] if r < len(combos) else (int(rng.integers(0, S + 1)), "random")
        c = S if c < 0 else min(c, S)
        if p == "front":
            m[r, :c] = True
        elif p == "back":
            m[r, S - c:] = True
        elif p == "alternate":
            idx = np.concatenate([np.arange(0, S, 2), np.arange(1, S, 2)])[:c]      # every other sample first, then the gaps
            m[r, idx] = True
        else:
            m[r, rng.choice(S, size=c, replace=False)] = True
    return m


def noise_of(S, amp):
    return torch.from_numpy(np.where(live_mask(S), np.float32(amp), np.float32(-1e4))).to(DEV)


def sorted_depths(rb, S, seed=11):
    """[N, S] given depths of a fine pass: sorted, uneven, inside the ray's near / far"""
    rng = np.random.default_rng(seed)
    t = np.sort(rng.random((N, S)).astype(np.float32), axis=1)
    near, far = rb[:, 6:7].cpu().numpy(), rb[:, 7:8].cpu().numpy()
    return torch.from_numpy((near + (far - near) * t).astype(np.float32)).to(DEV)


def launch(net, rb, S, want, *, ws, noise=None, z_vals=None, n_importance=0):
    """swnerf_render_pass at the C ABI with or without the workspace -> (return code, outputs)"""
    import swnerf.render as render
    from swnerf import _lib
    kind, packed, Lp, Ld, Lt = net.packed()
    a, out, _keep = render.pass_args(rb, kind, packed, (Lp, Ld, Lt), S, 4, 0, dict(z_vals=z_vals, t_rand=None, noise=noise, u=None),
                                     want, n_importance)
    for t in out.values():
        t.fill_(-7.0)                            # an output the launch leaves unwritten differs from every computed value
    if ws is None:
        rc = _lib.lib().swnerf_render_pass(a, _lib.stream_of(rb))
    else:
        rc = _lib.lib().swnerf_render_pass_ws(a, _lib.ptr(ws), ws.numel(), _lib.stream_of(rb))
    torch.cuda.synchronize()
    return rc, out


def workspace(n=N):
    return torch.full((n * WS_FLOATS,), float("nan"), dtype=torch.float32, device=DEV)


CASES = {"S33": (33, False, 0), "S64": (64, False, 0), "S64_resample": (64, False, 128), "S192_fine": (192, True, 0)}


@pytest.mark.parametrize("amp", [1e4, 1.0], ids=["opaque", "mild"])
@pytest.mark.parametrize("case", list(CASES))
def test_workspace_launch_equals_inline_launch(case, amp):
    """every output of the launch with the workspace is torch.equal (bits) to the launch without one (swnerf_render_pass)"""
    S, given, Ni = CASES[case]
    net, rb = net_of("canon"), rays_of("canon", n=N)
    kw = dict(noise=noise_of(S, amp), z_vals=sorted_depths(rb, S) if given else None, n_importance=Ni)
    rc0, inline = launch(net, rb, S, OUTS, ws=None, **kw)
    rc1, defer = launch(net, rb, S, OUTS, ws=workspace(), **kw)
    assert rc0 == 0 and rc1 == 0
    g = Gate()
    for k in inline:                             # OUTS, and z_fine / z_std when the launch resamples
        g.true(bool(torch.isfinite(inline[k]).all()) or k == "disp_map", f"{case}: the inline launch's {k} is not finite")
        g.true(same(defer[k], inline[k]), f"{case} amp={amp:g}: {k} differs between the workspace launch and the inline launch "
                                          f"({int((defer[k] != inline[k]).sum())} elements)")
    # the patterns do what the case list says: some ray has more live rows than the ring holds, some ray none but its canary
    live = live_mask(S).sum(1)
    assert live.min() == 0 and live.max() == S
    g.finish(f"deferred colour branch {case} amp={amp:g}")


def test_raw_requested_gives_the_inline_raw():
    """`raw` needs every row's colour: a launch with the workspace and raw requested returns the inline launch's raw and maps"""
    S = 64
    net, rb = net_of("canon"), rays_of("canon", n=N)
    noise = noise_of(S, 1.0)
    _, inline = launch(net, rb, S, OUTS + ["raw"], ws=None, noise=noise)
    rc, defer = launch(net, rb, S, OUTS + ["raw"], ws=workspace(), noise=noise)
    assert rc == 0
    g = Gate()
    for k in inline:
        g.true(same(defer[k], inline[k]), f"raw requested: {k} differs")
    g.true(bool(torch.isfinite(defer["raw"]).all()), "raw holds an element that was never written")
    g.finish("deferred colour branch, raw requested")


def test_poisoned_rgb_bias_reaches_every_ray():
    """one NaN in rgb_linear.bias[0]: channel 0 of EVERY ray's rgb_map is NaN with the workspace on - also of the rays whose only
    evaluated row is the canary (sample 0) - and acc_map stays finite"""
    S = 64
    net = copy.deepcopy(net_of("canon"))
    net._pack_cache = {}
    with torch.no_grad():
        net.rgb_linear.bias[0] = float("nan")
    rb = rays_of("canon", n=N)
    rc, out = launch(net, rb, S, OUTS, ws=workspace(), noise=noise_of(S, 1e4))
    assert rc == 0
    only_canary = np.flatnonzero(live_mask(S).sum(1) == 0)
    assert only_canary.size >= 4
    g = Gate()
    g.true(bool(torch.isnan(out["rgb_map"][:, 0]).all()), f"{int((~torch.isnan(out['rgb_map'][:, 0])).sum())} rays have a finite red behind a NaN rgb bias")
    g.true(bool(torch.isnan(out["rgb_map"][only_canary, 0]).all()), "a ray whose only evaluated row is the canary has a finite red")
    g.true(bool(torch.isfinite(out["rgb_map"][:, 1:]).all()), "the other channels do not depend on bias[0]")
    g.true(bool(torch.isfinite(out["acc_map"]).all()), "acc_map does not depend on the colours")
    g.finish("deferred colour branch, poisoned rgb bias")


def test_short_workspace_is_refused():
    """a workspace one float short of n_rays * 64 * 256 is the argument error, and nothing is launched"""
    S = 33
    net, rb = net_of("canon"), rays_of("canon", n=N)
    rc, out = launch(net, rb, S, OUTS, ws=workspace()[:-1], noise=noise_of(S, 1e4))
    assert rc == -1                              # SWNERF_E_ARG
    from swnerf import _lib
    assert "view_ws" in _lib.lib().swnerf_last_error().decode()
    for k, t in out.items():
        assert bool((t == -7.0).all()), f"{k} was written by a refused launch"
